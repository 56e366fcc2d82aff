"""Shared by the central-agent thermal policy tests (tests/test_policy_full_central_host.py, tests/test_gpu_policy_full_central_rollout.py): the test
policies, the central-agent observation vectors of a thermal batch rebuilt on the host over the FIVE env-dependent planes, the closed loop on the
CPU oracle with the four heads scattered into the action columns, and the float32 torch evaluation's deviation."""
import numpy as np
import torch

from citylearn_amd.observations import ObservationLayout
from citylearn_amd.policy import CLPF_NA, CentralStorageMLPPolicy
from policy_central_util import central_layout           # noqa: F401
from policy_full_util import THERMAL_PLANES, replay_noise, scatter_heads, thermal_district          # noqa: F401
from policy_util import HostEntry           # noqa: F401  (`clpfca_mlp` has `clpf_mlp`'s fields: the thermal entry's harness serves it as it is)

# The weight scale of every central thermal test policy: first-layer rows uniform in +-W1_SCALE / sqrt(n_cols), head rows uniform in
# +-W2_SCALE / sqrt(H), first-layer biases in +-0.5, head biases in +-0.4 W2_SCALE (tests/policy_full_util.py's).  Chosen on the CPU, before any GPU
# run, by test_policy_full_central_host.py::test_closed_loop_is_well_conditioned: the oracle loop with every action rounded through float32 and
# moved by the GPU teacher-forced tolerance (4 x a float32 torch evaluation's deviation) must keep soc, cs, ds and net within
# 0.1 x (1e-4 + 1e-4 |ref|) over K = 48 while the actions span a range.  As in tests/policy_full_util.py an action error reaches `net` directly
# through the tanks' capacity, so what matters is the tolerance itself, i.e. the size of the actions (W2_SCALE); the central hidden layer adds
# that an error of one building comes back into EVERY head through the 5 B env-dependent columns.  Readings (worst of soc / cs / ds / net in units
# of the plain bar, normalised layout; H = 4 / 32 / 64):
#   (0.25, 0.125), tests/policy_full_util.py's scale:  g2020_cz1 0.010 / 0.032 / 0.014, t1 0.004 / 0.040 / 0.003, t2 0.003 / 0.003 / 0.005,
#                                                     t16 0.018 / 0.034 / 0.063 (all of them net; soc <= 0.0042, cs <= 0.0088)
#   (0.125, 0.125), chosen:                           g2020_cz1 0.016 / 0.020 / 0.014, t1 0.002 / 0.009 / 0.004, t2 0.003 / 0.012 / 0.004,
#                                                     t16 0.015 / 0.026 / 0.015 (net again; soc <= 0.0039, cs <= 0.0084); teacher-forced
#                                                     tolerance 1.1e-8 .. 6.3e-8; |action| max 0.014 .. 0.092, range 0.023 .. 0.151
# Both are admitted; the smaller first layer has the margin at sixteen buildings x 64 units, the worst shape of the larger one.  ds reads 0.0000
# everywhere, as in tests/policy_full_util.py: over these 48 hours the fixture's DHW tanks stay empty in the oracle whatever the head asks for.
W1_SCALE, W2_SCALE = 0.125, 0.125


def make_central_storage_policy(layout: ObservationLayout, H: int, n_sets: int = 1, seed: int = 0, sigma=None) -> CentralStorageMLPPolicy:
    n_cols, B = layout.n_cols, len(layout.building_names)
    rng = np.random.RandomState(4000 + seed)
    w1 = rng.uniform(-1, 1, size=(n_sets, H, n_cols)) * W1_SCALE / np.sqrt(n_cols)
    b1 = rng.uniform(-0.5, 0.5, size=(n_sets, H))
    w2 = rng.uniform(-1, 1, size=(n_sets, B, CLPF_NA, H)) * W2_SCALE / np.sqrt(H)
    b2 = rng.uniform(-1, 1, size=(n_sets, B, CLPF_NA)) * 0.4 * W2_SCALE
    return CentralStorageMLPPolicy(w1, b1, w2, b2, sigma=sigma)


class CentralStorageObservations:
    """The central-agent observation vectors [E, n_cols] of a thermal batch at table row r from the planes soc, cs, hs, ds, previous net
    [n_bldg, E] each (float64; `THERMAL_PLANES` order): the arithmetic of `ObservationTables.host_row` (row + plane * col_scale for the
    env-dependent columns; row 0 / the reset table as they are)."""

    def __init__(self, layout: ObservationLayout, tab):
        assert layout.central_agent
        self.obs = layout.episode(tab, reset_table=True)
        src = self.obs.col_src
        kind, plane = src >> 28, (src >> 20) & 0xFF
        self.bldg = np.where(src >= 0, src & 0xFFFFF, 0)
        self.is_term = [(src >= 0) & (kind == k) & (plane == p) for k, p in THERMAL_PLANES]            # [n_cols] each
        assert np.array_equal(src >= 0, np.logical_or.reduce(self.is_term))
        assert all(layout.columns[c][0] == self.bldg[c] for c in np.nonzero(src >= 0)[0])              # every such column is the building's OWN
        self.scale = self.obs.col_scale.astype(np.float64)
        self.n_cols = len(src)

    def at(self, r: int, *planes, reset: bool = False, E: int = None):
        E = np.shape(planes[0])[1] if E is None else E
        if reset:
            return np.broadcast_to((self.obs.reset_table[r] if r else self.obs.table[0])[None], (E, self.n_cols)).copy()
        assert len(planes) == len(self.is_term)
        x = np.broadcast_to(self.obs.table[r][None], (E, self.n_cols)).copy()
        for is_d, v in zip(self.is_term, planes):
            x += np.where(is_d[None], np.asarray(v, dtype=np.float64).T[:, self.bldg] * self.scale[None], 0.0)
        return x


def host_closed_loop(spec, tab, layout, pol, pt, K, E, reward='RewardFunction', perturb=None, seed=0, env_offset=0, round_f32=False):
    """tests/policy_full_util.py's `host_closed_loop` for a central policy: K steps from reset of the CPU oracle (float64) driven by
    `pol.actions_host` on the central-agent vector the env would hand out, the heads scattered by `scatter_heads`.  Returns a dict of
    [K, n_bldg, E] arrays ('action': [K, 4, n_bldg, E]; 'dnet': [K, E])."""
    from oracle.c_oracle import COracle, OS, OO
    ora = COracle(spec, tab, E, reward=reward)
    cobs = CentralStorageObservations(layout, tab)
    B = len(spec.buildings)
    out = {k: np.zeros((K, B, E)) for k in ('soc', 'cs', 'hs', 'ds', 'degcap', 'net', 'reward')}
    out['action'] = np.zeros((K, CLPF_NA, B, E))
    out['dnet'] = np.zeros((K, E))
    rng = np.random.RandomState(77)
    noisy = bool(np.any(pt.sigma_bldg > 0))
    for t in range(K):
        if t == 0:
            x = cobs.at(0, reset=True, E=E)
        else:
            x = cobs.at(t, *[ora.state[:, :, OS[k]].T for k in ('SOC', 'CS', 'HS', 'DS')], ora.out[:, :, OO['NET']].T)
        a = pol.actions_host(x, pt, noise=replay_noise(pt, seed, E, t, env_offset) if noisy else None)          # [E, B, 4]
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


def f32_torch_deviation(pol: CentralStorageMLPPolicy, x, pt, device='cpu', noise=None, set_index: int = 0) -> float:
    """max |float32 torch evaluation of the unsplit MLP - float64| on central-agent vectors x [..., n_cols], over the heads that have a column
    (`noise`: the standard normals [..., n_bldg, 4], handed to both; `pt`: the policy's `pack`, for the bounds, sigmas and columns)."""
    ref = pol.actions_host(x, pt, noise=noise, set_index=set_index)
    t = lambda v: torch.as_tensor(np.array(v), dtype=torch.float32, device=device)
    w1, b1, w2, b2 = (t(v[set_index]) for v in pol._full())
    h = torch.tanh(t(x) @ w1.t() + b1)
    lo, hi = t(pt.low_bldg), t(pt.high_bldg)
    a = 0.5 * (hi + lo) + 0.5 * (hi - lo) * torch.tanh(torch.einsum('baj,...j->...ba', w2, h) + b2)
    if noise is not None:
        a = a + t(pt.sigma_bldg) * t(noise)
    d = np.abs(torch.clamp(a, lo, hi).cpu().numpy().astype(np.float64) - ref)
    return float(np.where(pt.cols >= 0, d, 0.0).max())
