"""Shared by tests/test_policy_full_host.py and tests/test_gpu_policy_full_rollout.py: the test policies of thermal districts (ONE weight scale,
fixed by the CPU conditioning test), the FIVE env-dependent planes of the observation vectors rebuilt on the host (`policy_util.HostObservations`),
the thermal districts, and the closed loop on the CPU oracle with the four heads scattered into the action columns."""
import copy
from dataclasses import replace
from functools import lru_cache

import numpy as np

from golden_util import golden
from citylearn_amd import abi
from citylearn_amd.observations import SRC_OUT, SRC_STATE, ObservationLayout
from citylearn_amd.policy import CLPF_NA, StorageMLPPolicy, noise_host
from policy_util import HostObservations

# The weight scale of every test policy: first-layer rows uniform in +-W1_SCALE / sqrt(n_obs), output rows uniform in +-W2_SCALE / sqrt(H), output
# biases in +-0.4 W2_SCALE (policy_util's 0.2 at its scale).  Chosen on the CPU, before any GPU run, by
# test_policy_full_host.py::test_closed_loop_is_well_conditioned: every head's action moved by the teacher-forced tolerance through the float64
# oracle loop over 48 steps, worst deviation in units of the plain bar 1e-4 + 1e-4 |ref| (the issue admits 0.1).  Here an action error reaches
# `net` DIRECTLY through the tanks' capacity (hundreds of kWh per action unit), so what matters is the tolerance itself, which is proportional
# to the size of the actions, i.e. to W2_SCALE -- not the loop gain as on the 2022 battery district.  Worst `net` reading over H = 4 / 16 / 32:
#   (0.25, 0.5), policy_util's start:  g2020_cz1 0.122 (H = 4: over the 0.1), t16 0.069
#   (0.25, 0.25):                      g2020_cz1 0.056, t1 0.009, t2 0.018, t16 0.066
#   (0.25, 0.125), chosen:             g2020_cz1 0.038, t1 0.023, t2 0.004, t16 0.030; soc <= 0.0032, cs <= 0.0074 (tolerances 1.9e-8 .. 5.8e-8)
# ds reads 0.0000 everywhere: over these 48 hours the DHW tanks of the fixture stay empty in the oracle whatever the head asks for (the head's
# action still goes through the unit's clipping, and the kernel has to agree that the plane stays 0).  Actions span about +-0.09 of the bounds.
W1_SCALE, W2_SCALE = 0.25, 0.125

# the planes of the state / output arrays the five terms read, in CLPF_D_* order: soc, cs, hs, ds, previous net
THERMAL_PLANES = ((SRC_STATE, abi.CLS_B_SOC), (SRC_STATE, abi.CLS_CS_SOC), (SRC_STATE, abi.CLS_HS_SOC), (SRC_STATE, abi.CLS_DS_SOC), (SRC_OUT, abi.CLO_NET))


def make_storage_policy(layout: ObservationLayout, H: int, n_sets: int = 1, seed: int = 0, sigma=None, shared: bool = False) -> StorageMLPPolicy:
    n_obs = max(len(n) for n in layout.building_names)
    nb = 1 if shared else len(layout.building_names)
    rng = np.random.RandomState(2000 + seed)
    w1 = rng.uniform(-1, 1, size=(n_sets, nb, H, n_obs)) * W1_SCALE / np.sqrt(n_obs)
    b1 = rng.uniform(-0.5, 0.5, size=(n_sets, nb, H))
    w2 = rng.uniform(-1, 1, size=(n_sets, nb, CLPF_NA, H)) * W2_SCALE / np.sqrt(H)
    b2 = rng.uniform(-1, 1, size=(n_sets, nb, CLPF_NA)) * 0.4 * W2_SCALE
    return StorageMLPPolicy(w1, b1, w2, b2, sigma=sigma)


OUTAGE_SUFFIX = '_outage'
OUTAGE_NAMES = ('g2020_cz1_outage', 't1_outage', 't2_outage', 't16_outage')


@lru_cache(maxsize=None)
def thermal_district(name: str):
    """Districts cut from / repeated out of g2020_cz1's nine buildings (buildings 2 and 3 have no DHW storage): 't1' building 0; 't2' buildings
    1 and 2 -- one with and one without DHW; 't16' / 't17' tiled + jittered to 16 (nw = 16, the kernel's limit) / 17 buildings (refused).
    '<name>_outage': `outage_district` of that district."""
    from citylearn_amd.synthetic import tile_district
    if name.endswith(OUTAGE_SUFFIX):
        return outage_district(name[:-len(OUTAGE_SUFFIX)])
    g = golden('g2020_cz1')
    if name == 'g2020_cz1':
        return g.spec()
    if name == 't1':
        return g.spec(buildings=[0])
    if name == 't2':
        return g.spec(buildings=[1, 2])
    return tile_district(g.spec(), {'t16': 16, 't17': 17}[name])


def outage_rows(i: int):
    """The episode steps at which building i of an outage district is without the grid: none for i % 3 == 2 (those waves take the kernel's
    branch without outage in the same workgroup at the same step); for the others 5 + i % 9 .. 8 + i % 9 (staggered per building, straddling
    a launch boundary at step 6), 22 .. 26 (common to all: across the day boundary at t = 24 and a KPI fold at step 24) and 40 .. 41.  Never
    step 0, which `reset()` books before any kernel runs (tests/test_gpu_check.py)."""
    if i % 3 == 2:
        return []
    return list(range(5 + i % 9, 9 + i % 9)) + list(range(22, 27)) + [40, 41]


@lru_cache(maxsize=None)
def outage_district(name: str):
    """`thermal_district(name)` with a power outage: every building a `copy.copy` with a `series` dict of its own whose 'power_outage' is 1
    on `outage_rows(i)` of episode 0, `outage.simulate` on (deterministic signal), and the three tanks charged to 0.5 where they have a
    capacity (the battery starts as the schema has it), so that a storage has something to discharge when the grid goes away.  No LSTM stage,
    no device action: the policy packer accepts it.  The cached original and the shared series arrays are left as they are."""
    src = thermal_district(name)
    start, _ = src.episode_window(0)
    out = []
    for i, b in enumerate(src.buildings):
        c = copy.copy(b)
        c.series = dict(b.series)
        signal = np.zeros_like(b.series['power_outage'])
        signal[[start + r for r in outage_rows(i)]] = 1
        c.series['power_outage'] = signal
        c.outage = replace(b.outage, simulate=True, stochastic=False)
        for key in ('cooling_storage', 'heating_storage', 'dhw_storage'):
            tank = getattr(b, key)
            if tank.capacity > 0:
                setattr(c, key, replace(tank, initial_soc=0.5))
        out.append(c)
    return replace(src, buildings=out)


def outage_mask(tab, K: int):
    """bool [K, n_bldg]: the (step, building) pairs of the first K rows of the episode tables that carry an outage."""
    return tab.outage[:K] > 0


def replay_noise(pt, seed, E, t, env_offset=0):
    """[E, n_bldg, 4] the kernel's standard normals of step t (0 where the head has no column or sigma 0)."""
    B = pt.cols.shape[0]
    z = np.zeros((E, B, CLPF_NA))
    for b in range(B):
        for a in range(CLPF_NA):
            if pt.cols[b, a] >= 0 and pt.sigma_bldg[b, a] > 0:
                z[:, b, a] = noise_host(seed, env_offset + np.arange(E), int(pt.cols[b, a]), t)
    return z


def scatter_heads(pt, a, n_act_cols):
    """Head actions [E, n_bldg, 4] -> the env's action layout [n_act_cols, E] (float32)."""
    acts = np.zeros((n_act_cols, a.shape[0]), dtype=np.float32)
    b, h = np.nonzero(pt.cols >= 0)
    acts[pt.cols[b, h]] = a[:, b, h].T
    return acts


def host_closed_loop(spec, tab, layout, policy, pt, K, E, reward='RewardFunction', perturb=None, seed=0, env_offset=0, round_f32=False):
    """K steps from reset of the CPU oracle (float64) driven by `policy.actions_host` on the observations the env would hand out.  `perturb`
    (float): every action is moved by +-perturb (a fixed random sign per (step, env, building, head)).  Returns a dict of [K, n_bldg, E] arrays
    ('action': [K, 4, n_bldg, E]; 'dnet': [K, E])."""
    from oracle.c_oracle import COracle, OS, OO
    ora = COracle(spec, tab, E, reward=reward)
    hobs = HostObservations(layout, tab, THERMAL_PLANES)
    B = len(spec.buildings)
    out = {k: np.zeros((K, B, E)) for k in ('soc', 'cs', 'hs', 'ds', 'degcap', 'net', 'reward')}
    out['action'] = np.zeros((K, CLPF_NA, B, E))
    out['dnet'] = np.zeros((K, E))
    rng = np.random.RandomState(77)
    noisy = bool(np.any(pt.sigma_bldg > 0))
    for t in range(K):
        if t == 0:
            x = hobs.at(0, None, reset=True, E=E)
        else:
            x = hobs.at(t, *[ora.state[:, :, OS[k]].T for k in ('SOC', 'CS', 'HS', 'DS')], ora.out[:, :, OO['NET']].T)
        a = policy.actions_host(x, pt, noise=replay_noise(pt, seed, E, t, env_offset) if noisy else None)          # [E, B, 4]
        if round_f32:
            a = a.astype(np.float32).astype(np.float64)
        if perturb:
            a = np.where(pt.cols >= 0, np.clip(a + perturb * rng.choice([-1.0, 1.0], size=a.shape), pt.low_bldg, pt.high_bldg), 0.0)
        o, oe = ora.step(scatter_heads(pt, a, ora.n_act_cols), t)
        out['action'][t] = a.transpose(2, 1, 0)
        for k, key in (('soc', 'SOC'), ('cs', 'CS'), ('hs', 'HS'), ('ds', 'DS'), ('degcap', 'DEGCAP')):
            out[k][t] = ora.state[:, :, OS[key]].T
        out['net'][t] = o[:, :, OO['NET']].T
        out['reward'][t] = o[:, :, OO['REWARD']].T
        out['dnet'][t] = oe[:, 0]
    return out
