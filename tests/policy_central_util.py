"""Shared by the central-agent policy tests (tests/test_policy_central_host.py, tests/test_gpu_policy_central_rollout.py): the test policies, the
central-agent observation vectors of a batch rebuilt on the host, the closed loop on the CPU oracle, the float32 torch evaluation's deviation,
and the library's entry point on host memory."""
import numpy as np
import torch

from citylearn_amd import abi
from citylearn_amd.observations import SRC_OUT, SRC_STATE, ObservationLayout
from citylearn_amd.policy import CentralMLPPolicy, noise_host
from policy_util import HostEntry           # noqa: F401  (`clpca_mlp` has `clpol_mlp`'s fields: the lean entry's harness serves it as it is)

# The weight scale of every central test policy: first-layer rows uniform in +-W1_SCALE / sqrt(n_cols), head rows uniform in
# +-W2_SCALE / sqrt(H), biases as tests/policy_util.py's.  Chosen on the CPU, before any GPU run, by
# test_policy_central_host.py::test_closed_loop_is_well_conditioned, which repeats tests/test_policy_deep_host.py's criteria: the oracle loop
# perturbed by the GPU teacher-forced tolerance (4 x a float32 torch evaluation's deviation, every action rounded through float32) must keep soc
# and net within 0.1 x (1e-4 + 1e-4 |ref|) over K = 48 while the actions span a range.  A central hidden layer couples every building to every
# other: an action error of building b reaches net_b through the battery's nominal power and comes back into EVERY head through the 2 B
# env-dependent columns.  Readings (worst of soc / net in units of the plain bar, normalised layout; H = 4 / 32 / 64):
#   (0.25, 0.5), tests/policy_util.py's scale:  g2022_all 0.021 / 0.048 / 0.056, het17 0.015 / 0.037 / 0.078, b1 0.002 / 0.009 / 0.006,
#                                               b32 0.031 / 0.061 / 0.121 -- NOT admitted at 32 buildings x 64 units
#   (0.25, 0.25):                               g2022_all 0.018 / 0.028 / 0.038, het17 0.011 / 0.023 / 0.043, b32 0.032 / 0.054 / 0.168
#   (0.125, 0.25):                              g2022_all 0.015 / 0.021 / 0.037, het17 0.011 / 0.022 / 0.066, b32 0.023 / 0.035 / 0.102
#   (0.1, 0.2):                                 g2022_all 0.011 / 0.022 / 0.044, het17 0.006 / 0.019 / 0.049, b32 0.049 / 0.031 / 0.051
#   (0.125, 0.125), chosen:                     g2022_all 0.014 / 0.034 / 0.028, het17 0.011 / 0.023 / 0.039, b1 0.002 / 0.001 / 0.000,
#                                               b32 0.032 / 0.026 / 0.046; teacher-forced tolerance 8e-8 .. 1.5e-7 (b1: 9e-9 .. 3e-8);
#                                               |action| max 0.18 .. 0.25, range 0.36 .. 0.48 (b1: 0.006 .. 0.029, range 0.003 .. 0.006)
# The reading is not monotone in the scale: what amplifies is a battery that runs into a limit, where the accumulated soc error times the
# capacity lands in net at once; the tolerance itself grows with the sums' mass (H = 64 over b32's 155 columns is the worst shape throughout).
W1_SCALE, W2_SCALE = 0.125, 0.125

LEAN_PLANES = ((SRC_STATE, abi.CLS_B_SOC), (SRC_OUT, abi.CLO_NET))


def central_layout(spec, normalize=True) -> ObservationLayout:
    return ObservationLayout(spec, 'current', normalize, central_agent=True)


def make_central_policy(layout: ObservationLayout, H: int, n_sets: int = 1, seed: int = 0, sigma=None) -> CentralMLPPolicy:
    n_cols, B = layout.n_cols, len(layout.building_names)
    rng = np.random.RandomState(3000 + seed)
    w1 = rng.uniform(-1, 1, size=(n_sets, H, n_cols)) * W1_SCALE / np.sqrt(n_cols)
    b1 = rng.uniform(-0.5, 0.5, size=(n_sets, H))
    w2 = rng.uniform(-1, 1, size=(n_sets, B, H)) * W2_SCALE / np.sqrt(H)
    b2 = rng.uniform(-0.2, 0.2, size=(n_sets, B))
    return CentralMLPPolicy(w1, b1, w2, b2, sigma=sigma)


class CentralObservations:
    """The central-agent observation vectors [E, n_cols] of a batch at table row r from the soc and previous-net planes [n_bldg, E] (float64): the
    arithmetic of `ObservationTables.host_row` (row + plane * col_scale for the env-dependent columns; row 0 / the reset table as they are)."""

    def __init__(self, layout: ObservationLayout, tab):
        assert layout.central_agent
        self.obs = layout.episode(tab, reset_table=True)
        src = self.obs.col_src
        kind, plane = src >> 28, (src >> 20) & 0xFF
        self.bldg = np.where(src >= 0, src & 0xFFFFF, 0)
        self.is_term = [(src >= 0) & (kind == k) & (plane == p) for k, p in LEAN_PLANES]               # [n_cols] each: soc, net
        assert np.array_equal(src >= 0, self.is_term[0] | self.is_term[1])
        assert all(layout.columns[c][0] == self.bldg[c] for c in np.nonzero(src >= 0)[0])              # every such column is the building's OWN
        self.scale = self.obs.col_scale.astype(np.float64)
        self.n_cols = len(src)

    def at(self, r: int, soc=None, net=None, reset: bool = False, E: int = None):
        E = np.shape(soc)[1] if E is None else E
        if reset:
            return np.broadcast_to((self.obs.reset_table[r] if r else self.obs.table[0])[None], (E, self.n_cols)).copy()
        x = np.broadcast_to(self.obs.table[r][None], (E, self.n_cols)).copy()
        for is_d, v in zip(self.is_term, (soc, net)):
            x += np.where(is_d[None], np.asarray(v, dtype=np.float64).T[:, self.bldg] * self.scale[None], 0.0)
        return x


def host_closed_loop(spec, tab, layout, pol, pt, K, E, reward='RewardFunction', perturb=None, seed=0, env_offset=0, round_f32=False):
    """tests/policy_util.py's `host_closed_loop` for a central policy: K steps from reset of the CPU oracle (float64) driven by
    `pol.actions_host` on the central-agent vector the env would hand out.  Returns a dict of [K, n_bldg, E] arrays (district net: [K, E])."""
    from oracle.c_oracle import COracle, OS, OO
    ora = COracle(spec, tab, E, reward=reward)
    cobs = CentralObservations(layout, tab)
    es, sig = pt.es_cols, pt.sigma_bldg
    B = len(spec.buildings)
    out = {k: np.zeros((K, B, E)) for k in ('action', 'soc', 'degcap', 'net', 'reward')}
    out['dnet'] = np.zeros((K, E))
    rng = np.random.RandomState(77)
    for t in range(K):
        x = cobs.at(0, reset=True, E=E) if t == 0 else cobs.at(t, ora.state[:, :, OS['SOC']].T, ora.out[:, :, OO['NET']].T)
        z = None
        if np.any(sig > 0):
            z = np.stack([noise_host(seed, env_offset + np.arange(E), es[b], t) if sig[b] > 0 else np.zeros(E) for b in range(B)], axis=1)
        a = pol.actions_host(x, noise=z, tables=pt)                           # [E, B]
        if round_f32:
            a = a.astype(np.float32).astype(np.float64)
        if perturb:
            a = np.clip(a + perturb * rng.choice([-1.0, 1.0], size=a.shape), pt.low_bldg, pt.high_bldg)
        acts = np.zeros((ora.n_act_cols, E), dtype=np.float32)
        acts[es[es >= 0]] = a.T[es >= 0]
        o, oe = ora.step(acts, t)
        out['action'][t] = a.T
        out['soc'][t] = ora.state[:, :, OS['SOC']].T
        out['degcap'][t] = ora.state[:, :, OS['DEGCAP']].T
        out['net'][t] = o[:, :, OO['NET']].T
        out['reward'][t] = o[:, :, OO['REWARD']].T
        out['dnet'][t] = oe[:, 0]
    return out


def f32_torch_deviation(pol: CentralMLPPolicy, x, pt, device='cpu', noise=None, set_index: int = 0) -> float:
    """max |float32 torch evaluation of the unsplit MLP - float64| on central-agent vectors x [..., n_cols], over the buildings that have a storage
    action (`noise`: the standard normals, handed to both; `pt`: the policy's `pack`, for the bounds, sigmas and columns)."""
    ref = pol.actions_host(x, tables=pt, noise=noise, set_index=set_index)
    t = lambda v: torch.as_tensor(np.array(v), dtype=torch.float32, device=device)
    w1, b1, w2, b2 = (t(v[set_index]) for v in pol._full())
    h = torch.tanh(t(x) @ w1.t() + b1)
    lo, hi = t(pt.low_bldg), t(pt.high_bldg)
    a = 0.5 * (hi + lo) + 0.5 * (hi - lo) * torch.tanh(h @ w2.t() + b2)
    if noise is not None:
        a = a + t(pt.sigma_bldg) * t(noise)
    d = np.abs(torch.clamp(a, lo, hi).cpu().numpy().astype(np.float64) - ref)
    return float(np.where(pt.cols >= 0, d, 0.0).max())
