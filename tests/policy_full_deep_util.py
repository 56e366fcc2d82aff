"""Shared by the deep thermal policy tests (tests/test_policy_full_deep_host.py, tests/test_gpu_policy_full_deep_rollout.py): the test policies
with two hidden layers and four storage heads, the float32 torch evaluation's deviation through three layers, the operand split's bound on every
head, and the library's entry point on host memory.  The districts, the noise replay, the scatter of the heads and the closed loop on the CPU
oracle are tests/policy_full_util.py's (`host_closed_loop` only needs `actions_host` with `StorageMLPPolicy`'s signature)."""
import numpy as np
import torch

from citylearn_amd.observations import ObservationLayout
from citylearn_amd.policy import ACT_SCALE, CLPF_NA, DeepStorageMLPPolicy
from policy_deep_util import split_sum_bound
from policy_full_util import W1_SCALE, W2_SCALE, host_closed_loop                  # noqa: F401
from policy_util import HostEntry

# First layer and head rows at tests/policy_full_util.py's scales (0.25, 0.125), the middle layer's rows uniform in +-scale / sqrt(H1).
# MID_SCALE: the tests that do not run the loop freely (teacher-forced actions, the two families, replay, bit-for-bit) -- nothing amplifies there,
# and a full-size middle layer makes layer 2 carry the action.
# FREE_MID_SCALE: the free-running comparison against the CPU oracle.  Chosen on the CPU before any GPU run by
# test_policy_full_deep_host.py::test_closed_loop_is_well_conditioned, which perturbs the float64 oracle loop by each kernel family's FULL
# teacher-forced tolerance -- 4 x a float32 torch evaluation's deviation, for the matrix-core family plus `split_bound` -- and wants soc, cs, hs,
# ds and net within 0.1 x the plain bar over K = 48.  As on the one-layer thermal policy an action error reaches `net` directly through the tanks'
# capacity, so what matters is the size of the tolerance, and `split_bound` grows with sum |w3| sum |W2|.  Worst `net` reading over g2020_cz1, t1,
# t2, t16 and the shapes (4, 4) / (16, 32) / (32, 32), exact-fp32 family | matrix-core family:
#   1.0  (g2020_cz1, t16 read):  t16 (32, 32) 0.362 | t16 (16, 32) 0.205, g2020_cz1 (16, 32) over the 0.1 too (split_bound up to 6.9e-7): not used
#   0.25 (g2020_cz1, t16 read):  0.071 at t16 (32, 32) | g2020_cz1 (32, 32) 0.119, t16 (32, 32) 0.356: the matrix-core family is over the 0.1
#   0.05, policy_deep_util's, chosen:  g2020_cz1 0.015 / 0.012 / 0.030 | 0.015 / 0.021 / 0.048;  t1 <= 0.003 | <= 0.006;  t2 <= 0.004 | <= 0.006;
#         t16 0.010 / 0.018 / 0.062 | 0.013 / 0.022 / 0.062 -- maximum over the 24 cells 0.062; tolerances 1.5e-8 .. 5.9e-8 | 2.1e-8 .. 1.1e-7
# soc, cs, hs and ds read at most 0.017.  The actions still span 0.03 (t1) .. 0.15 (t16) of the bounds across buildings and steps.
MID_SCALE = 1.0
FREE_MID_SCALE = 0.05


def make_deep_storage_policy(layout: ObservationLayout, H1: int, H2: int, n_sets: int = 1, seed: int = 0, sigma=None, shared: bool = False,
                             mid_scale: float = None) -> DeepStorageMLPPolicy:
    n_obs = max(len(n) for n in layout.building_names)
    nb = 1 if shared else len(layout.building_names)
    rng = np.random.RandomState(2000 + seed)
    w1 = rng.uniform(-1, 1, size=(n_sets, nb, H1, n_obs)) * W1_SCALE / np.sqrt(n_obs)
    b1 = rng.uniform(-0.5, 0.5, size=(n_sets, nb, H1))
    w2 = rng.uniform(-1, 1, size=(n_sets, nb, H2, H1)) * (MID_SCALE if mid_scale is None else mid_scale) / np.sqrt(H1)
    b2 = rng.uniform(-0.5, 0.5, size=(n_sets, nb, H2))
    w3 = rng.uniform(-1, 1, size=(n_sets, nb, CLPF_NA, H2)) * W2_SCALE / np.sqrt(H2)
    b3 = rng.uniform(-1, 1, size=(n_sets, nb, CLPF_NA)) * 0.4 * W2_SCALE
    return DeepStorageMLPPolicy(w1, b1, w2, b2, w3, b3, sigma=sigma)


def f32_torch_deviation(pol: DeepStorageMLPPolicy, x, pt, device='cpu', noise=None, set_index: int = 0) -> float:
    """max |float32 torch evaluation of the three layers - float64| on observation vectors x [..., B, n_obs], over the heads that exist
    (`noise`: the standard normals [..., B, 4], handed to both; `pt`: the policy's `pack`, for the bounds, sigmas and columns)."""
    ref = pol.actions_host(x, pt, noise=noise, set_index=set_index)
    t = lambda v: torch.as_tensor(np.array(v), dtype=torch.float32, device=device)
    w1, b1, w2, b2, w3, b3 = (t(v[set_index]) for v in pol._full(x.shape[-2]))
    h1 = torch.tanh(torch.einsum('bjc,...bc->...bj', w1, t(x)) + b1)
    h2 = torch.tanh(torch.einsum('bij,...bj->...bi', w2, h1) + b2)
    lo, hi = t(pt.low_bldg), t(pt.high_bldg)
    a = 0.5 * (hi + lo) + 0.5 * (hi - lo) * torch.tanh(torch.einsum('bai,...bi->...ba', w3, h2) + b3)
    if noise is not None:
        a = a + t(pt.sigma_bldg) * t(noise)
    d = np.abs(torch.clamp(a, lo, hi).cpu().numpy().astype(np.float64) - ref)
    return float(np.where(pt.cols >= 0, d, 0.0).max())


def split_bound(pol: DeepStorageMLPPolicy, pt, set_index: int = 0) -> float:
    """`policy_deep_util.split_bound` for four heads: how far the matrix-core family's action of any head may lie from the exact-fp32 arithmetic
    because of the operand split alone, in float64 from the weights with no fitted constant.  The scaled layer-2 sum of unit i moves by at most
    split_sum_bound(ACT_SCALE W2_i) (|h1| <= 1), its tanh by dz_i = that over |ACT_SCALE| (|tanh'| <= 1), head a's action by
    half_a sum_i |w3_ai| dz_i (|tanh'| <= 1 again); worst head that has a column."""
    _, _, w2, _, w3, _ = (v[set_index] for v in pol._full(pt.cols.shape[0]))
    dz = split_sum_bound(ACT_SCALE * w2) / abs(ACT_SCALE)                                 # [B, H2]
    da = 0.5 * (pt.high_bldg - pt.low_bldg) * (np.abs(w3) * dz[:, None, :]).sum(axis=2)   # [B, 4]
    return float(da[pt.cols >= 0].max())


class DeepFullHostEntry(HostEntry):
    """`policy_util.HostEntry` for `clpfd_rollout_mlp_f32`: the struct's second-layer fields get valid defaults (n_hidden2 = 16, l2 = the buffer);
    `call(..., l2=None | HostEntry.ODD)` and `n_hidden2=` / `flags=` / `n_device_cols=` override them like any other field."""

    def call(self, d, **kw):
        buf = np.zeros(64, dtype=np.float32)
        self._keep = buf
        kw.setdefault('n_hidden2', 16)
        kw.setdefault('l2', buf.ctypes.data)
        return super().call(d, **kw)
