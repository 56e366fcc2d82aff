"""Shared by the tests of the central-agent policy with two hidden layers (tests/test_policy_central_deep_host.py,
tests/test_gpu_policy_central_deep_rollout.py): the test policies, the float32 torch evaluation's deviation through three layers, and the
library's entry point on host memory.  The central-agent observation vectors and the closed loop on the CPU oracle are
tests/policy_central_util.py's: `host_closed_loop` takes a `DeepCentralMLPPolicy` as it is (`actions_host` and the tables' host side have
`CentralMLPPolicy`'s surface)."""
import numpy as np
import torch

from citylearn_amd.observations import ObservationLayout
from citylearn_amd.policy import DeepCentralMLPPolicy
from policy_central_util import W1_SCALE, W2_SCALE, CentralObservations, central_layout, host_closed_loop          # noqa: F401
from policy_deep_util import DeepHostEntry          # noqa: F401  (`clpcd_mlp` has `clpd_mlp`'s fields: the deep entry's harness serves it as it is)

# First-layer rows uniform in +-W1_SCALE / sqrt(n_cols) and head rows in +-W2_SCALE / sqrt(H2): tests/policy_central_util.py's (0.125, 0.125).
# The middle layer's rows are uniform in +-MID_SCALE / sqrt(H1), its biases in +-0.5 as tests/policy_deep_util.py's.
# MID_SCALE is fixed on the CPU, before any GPU run, by test_policy_central_deep_host.py::test_closed_loop_is_well_conditioned -- the criteria of
# test_policy_central_host.py's test unchanged: the oracle loop perturbed by 4 x a float32 torch evaluation's deviation (every action rounded
# through float32) keeps soc and net within 0.1 x (1e-4 + 1e-4 |ref|) over K = 48 while the actions span a range.  The start is the deep tests'
# free-running middle layer, 0.05 (tests/policy_deep_util.py FREE_MID_SCALE).  ONE scale serves every test here: there is no second kernel family
# whose tolerance a full-size middle layer would have to expose.
# Readings (worst of soc / net in units of the plain bar, normalised layout; (H1, H2) = (4, 4) / (32, 32) / (64, 64) / (64, 4)):
#   0.05:          g2022_all 0.017 / 0.027 / 0.025 / 0.015, het17 0.010 / 0.015 / 0.019 / 0.019, b32 0.022 / 0.027 / 0.031 / 0.024,
#                  b1 0.000 / 0.000 / 0.000 / 0.009 -- NOT admitted: b1's actions do not move with the observations (range 1.8e-4 / 5e-5 /
#                  1.5e-4 / 6e-5 against the 1e-4 asked for): a middle layer this small leaves h2 = tanh(b2) whatever the first layer says
#   0.25:          g2022_all 0.022 / 0.024 / 0.015 / 0.023, het17 0.022 / 0.020 / 0.015 / 0.029, b32 0.033 / 0.032 / 0.022 / 0.022,
#                  b1 0.000 / 0.000 / 0.000 / 0.004 (range 8.7e-4 / 2.3e-4 / 7.6e-4 / 2.9e-4)
#   1.0, chosen:   g2022_all 0.030 / 0.032 / 0.025 / 0.032, het17 0.027 / 0.018 / 0.042 / 0.024, b32 0.030 / 0.034 / 0.028 / 0.029,
#                  b1 0.000 / 0.000 / 0.000 / 0.008 (range 3.2e-3 / 1.0e-3 / 3.1e-3 / 1.2e-3); teacher-forced tolerance 6e-8 .. 9.8e-8
#                  (b1: 2e-8 .. 6e-8); |action| max 0.19 .. 0.23, range 0.30 .. 0.44 on the districts of 17 and 32 buildings
# Unlike the per-building deep kernel's matrix-core tolerance, nothing here grows with the middle layer: the readings stay at the one-hidden-layer
# central policies' level (0.014 .. 0.046) at every scale, so the full-size middle layer -- with which layer 2 carries the action -- is admitted.
MID_SCALE = 1.0


def make_deep_central_policy(layout: ObservationLayout, H1: int, H2: int, n_sets: int = 1, seed: int = 0, sigma=None,
                             mid_scale: float = None) -> DeepCentralMLPPolicy:
    n_cols, B = layout.n_cols, len(layout.building_names)
    rng = np.random.RandomState(4000 + seed)
    w1 = rng.uniform(-1, 1, size=(n_sets, H1, n_cols)) * W1_SCALE / np.sqrt(n_cols)
    b1 = rng.uniform(-0.5, 0.5, size=(n_sets, H1))
    w2 = rng.uniform(-1, 1, size=(n_sets, H2, H1)) * (MID_SCALE if mid_scale is None else mid_scale) / np.sqrt(H1)
    b2 = rng.uniform(-0.5, 0.5, size=(n_sets, H2))
    w3 = rng.uniform(-1, 1, size=(n_sets, B, H2)) * W2_SCALE / np.sqrt(H2)
    b3 = rng.uniform(-0.2, 0.2, size=(n_sets, B))
    return DeepCentralMLPPolicy(w1, b1, w2, b2, w3, b3, sigma=sigma)


def f32_torch_deviation(pol: DeepCentralMLPPolicy, x, pt, device='cpu', noise=None, set_index: int = 0) -> float:
    """max |float32 torch evaluation of the three layers - float64| on central-agent vectors x [..., n_cols], over the buildings that have a
    storage action (`noise`: the standard normals, handed to both; `pt`: the policy's `pack`, for the bounds, sigmas and columns)."""
    ref = pol.actions_host(x, tables=pt, noise=noise, set_index=set_index)
    t = lambda v: torch.as_tensor(np.array(v), dtype=torch.float32, device=device)
    w1, b1, w2, b2, w3, b3 = (t(v[set_index]) for v in pol._full())
    h1 = torch.tanh(t(x) @ w1.t() + b1)
    h2 = torch.tanh(h1 @ w2.t() + b2)
    lo, hi = t(pt.low_bldg), t(pt.high_bldg)
    a = 0.5 * (hi + lo) + 0.5 * (hi - lo) * torch.tanh(h2 @ w3.t() + b3)
    if noise is not None:
        a = a + t(pt.sigma_bldg) * t(noise)
    d = np.abs(torch.clamp(a, lo, hi).cpu().numpy().astype(np.float64) - ref)
    return float(np.where(pt.cols >= 0, d, 0.0).max())
