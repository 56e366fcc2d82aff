"""Shared by the deep-policy tests (tests/test_policy_deep_host.py, tests/test_gpu_policy_deep_rollout.py): the test policies with two hidden
layers, their closed loop on the CPU oracle, the float32 torch evaluation's deviation through three layers, and the library's entry point on
host memory."""
import numpy as np
import torch

from citylearn_amd.observations import ObservationLayout
from citylearn_amd.policy import DeepMLPPolicy
from policy_util import W1_SCALE, W2_SCALE, HostEntry, host_closed_loop          # noqa: F401  (host_closed_loop takes a DeepMLPPolicy as it is:
#                                                                                  `actions_host` and the tables' host side have MLPPolicy's surface)

# The middle layer's rows are uniform in +-scale / sqrt(H1); first layer and output rows at tests/policy_util.py's scales.
# MID_SCALE: the tests that do not run the loop freely (teacher-forced actions, replay, the two families, bit-for-bit) -- nothing amplifies there,
# and a full-size middle layer makes layer 2 carry the action.
# FREE_MID_SCALE: the free-running comparison against the CPU oracle.  Chosen on the CPU before any GPU run by
# test_policy_deep_host.py::test_closed_loop_is_well_conditioned, which perturbs the oracle loop by each kernel family's FULL teacher-forced
# tolerance -- 4 x a float32 evaluation's deviation, for the matrix-core family plus `split_bound` -- and wants soc / net within 0.1 x the plain
# bar over K = 48.  `split_bound` grows with sum |w3| sum |W2| and an action error reaches `net` through the battery's nominal power at once, so
# at 1 / sqrt(H1) the matrix-core tolerance (split_bound 6e-7 .. 3.9e-6) moved net by 0.21 / 1.44 / 1.27 x the bar at (4, 4) / (16, 32) / (32, 32)
# on g2022_all (the exact-fp32 tolerance alone: 0.039 / 0.087 / 0.052), at 0.25 by 0.07 / 0.25 / 0.27, at 0.05 by 0.04 / 0.06 / 0.08 (het17: 0.09 at (32, 32)) -- the
# scale the 0.1 x condition admits for both families.  The actions still span 0.44 .. 0.50 of [-1, 1] across buildings and steps there.
MID_SCALE = 1.0
FREE_MID_SCALE = 0.05


def make_deep_policy(layout: ObservationLayout, H1: int, H2: int, n_sets: int = 1, seed: int = 0, sigma=None, shared: bool = False,
                     mid_scale: float = None) -> DeepMLPPolicy:
    n_obs = max(len(n) for n in layout.building_names)
    nb = 1 if shared else len(layout.building_names)
    rng = np.random.RandomState(2000 + seed)
    w1 = rng.uniform(-1, 1, size=(n_sets, nb, H1, n_obs)) * W1_SCALE / np.sqrt(n_obs)
    b1 = rng.uniform(-0.5, 0.5, size=(n_sets, nb, H1))
    w2 = rng.uniform(-1, 1, size=(n_sets, nb, H2, H1)) * (MID_SCALE if mid_scale is None else mid_scale) / np.sqrt(H1)
    b2 = rng.uniform(-0.5, 0.5, size=(n_sets, nb, H2))
    w3 = rng.uniform(-1, 1, size=(n_sets, nb, H2)) * W2_SCALE / np.sqrt(H2)
    b3 = rng.uniform(-0.2, 0.2, size=(n_sets, nb))
    return DeepMLPPolicy(w1, b1, w2, b2, w3, b3, sigma=sigma)


def f32_torch_deviation(pol: DeepMLPPolicy, x, pt, device='cpu', noise=None, set_index: int = 0) -> float:
    """max |float32 torch evaluation of the three layers - float64| on observation vectors x [..., B, n_obs], over the buildings that have a
    storage action (`noise`: the standard normals, handed to both; `pt`: the policy's `pack`, for the bounds, sigmas and columns)."""
    ref = pol.actions_host(x, tables=pt, noise=noise, set_index=set_index)
    t = lambda v: torch.as_tensor(np.array(v), dtype=torch.float32, device=device)
    w1, b1, w2, b2, w3, b3 = (t(v[set_index]) for v in pol._full(x.shape[-2]))
    h1 = torch.tanh(torch.einsum('bjc,...bc->...bj', w1, t(x)) + b1)
    h2 = torch.tanh(torch.einsum('bij,...bj->...bi', w2, h1) + b2)
    lo, hi = t(pt.low_bldg), t(pt.high_bldg)
    a = 0.5 * (hi + lo) + 0.5 * (hi - lo) * torch.tanh((w3 * h2).sum(dim=-1) + b3)
    if noise is not None:
        a = a + t(pt.sigma_bldg) * t(noise)
    d = np.abs(torch.clamp(a, lo, hi).cpu().numpy().astype(np.float64) - ref)
    return float(np.where(pt.cols >= 0, d, 0.0).max())


def split_sum_bound(a: np.ndarray, b_abs=1.0) -> np.ndarray:
    """Bound on |sum_j a_j b_j - (the three partial products i + j <= 1 of the two-term f16 split of both operands)| over the last axis of `a`
    (`a`: [..., rows, K] one building's matrix per leading index; |b_j| <= b_abs), for the scaled split of csrc/cl_policy_deep.h:
    a' = sw a with max |a'| in [2^13, 2^14), b' = 2^12 b, x' = x0 + 2^-11 x1 + r.  Round to nearest gives |r| <= 2^-22 |x'| (|x1| <= |x'|),
    and even if the hardware flushes every subnormal f16 to zero |r| grows by less than 2^-13 (a flushed x0 is below 2^-14, a flushed x1 stands
    for less than 2^-25): in units of a that is 2^-13 / sw <= 2^-26 max |a|, in units of b 2^-25.  Per product
    |r_a| |b| + |a| |r_b| + |r_a| |r_b| + |a1 b1|, the dropped product |a1 b1| <= 2^-22 |a| |b|."""
    a = np.abs(np.asarray(a, dtype=np.float64))
    ra = 2.0 ** -22 * a + 2.0 ** -26 * a.max(axis=(-2, -1), keepdims=True)
    rb = 2.0 ** -22 * b_abs + 2.0 ** -25
    return (ra * b_abs + a * rb + ra * rb + 2.0 ** -22 * a * b_abs).sum(axis=-1)


def split_bound(pol: DeepMLPPolicy, pt, set_index: int = 0) -> float:
    """How far the matrix-core family's action may lie from the exact-fp32 arithmetic because of the operand split alone, in float64 from the
    weights with no fitted constant: the scaled layer-2 sum of unit i moves by at most split_sum_bound(ACT_SCALE W2_i) (|h1| <= 1), its tanh by
    that over |ACT_SCALE| (|tanh'| <= 1), the action by half_b sum_i |w3_bi| of it (|tanh'| <= 1 again); worst driven building."""
    from citylearn_amd.policy import ACT_SCALE
    _, _, w2, _, w3, _ = (v[set_index] for v in pol._full(len(pt.cols)))
    dz = split_sum_bound(ACT_SCALE * w2) / abs(ACT_SCALE)                                 # [B, H2]
    da = 0.5 * (pt.high_bldg - pt.low_bldg) * (np.abs(w3) * dz).sum(axis=1)
    return float(da[pt.cols >= 0].max())


class DeepHostEntry(HostEntry):
    """`policy_util.HostEntry` for `clpd_rollout_mlp_f32`: the struct's second-layer fields get valid defaults (n_hidden2 = 16, l2 = the
    buffer); `call(..., l2=None | HostEntry.ODD)` and `n_hidden2=` / `reserved2=` / `flags=` override them like any other field."""

    def call(self, d, **kw):
        buf = np.zeros(64, dtype=np.float32)
        self._keep = buf
        kw.setdefault('n_hidden2', 16)
        kw.setdefault('l2', buf.ctypes.data)
        return super().call(d, **kw)
