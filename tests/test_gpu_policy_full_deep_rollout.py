"""The closed-loop rollout of thermal districts under a policy with TWO hidden layers on the GPU (`StepEngine.rollout_policy` /
`VectorCityLearnEnv.rollout_policy` with a `DeepStorageMLPPolicy`: one launch of `cl_rollout_full_policy_deep_kernel<PREC, MMA, MARL>`,
csrc/cl_policy_full_deep.h), both kernel families wherever a case names none: (1) its actions teacher-forced against the float64 MLP, (2) the two
families against each other on the same inputs, (3) its trajectory replayed through `step()`, (4) free-running against the CPU oracle, (5) launch
splitting, checkpoints, episode windows x parameter sets x env offsets and seeds bit for bit, the noise's bound, (6) the outage district, (7) the
env-level call and the refusals.  Weights: tests/policy_full_deep_util.py (scales fixed by tests/test_policy_full_deep_host.py's conditioning
test).  Small batches only: 64 envs (one tile), 260 (ragged, crosses a CL_ROW0_BLOCK: two parameter sets live), 4096 once per family."""
import numpy as np
import pytest
import torch

from golden_util import check_worst, golden, record_worst
from citylearn_amd import _lib, abi, policy
from citylearn_amd.engine import StepEngine
from citylearn_amd.observations import ObservationLayout
from policy_full_deep_util import FREE_MID_SCALE, f32_torch_deviation, host_closed_loop, make_deep_storage_policy, split_bound
from policy_full_util import THERMAL_PLANES, outage_mask, replay_noise, thermal_district
from policy_util import HostObservations
from test_gpu_policy_full_rollout import _net_is_zero_on_outage_rows_only, _replay          # (b)'s tolerances and the outage check, as they are

pytestmark = pytest.mark.gpu

KINDS = ['RewardFunction', 'MARL', 'IndependentSACReward', 'SolarPenaltyReward']
A, R, N, S = policy.CLPF_T_ACTION, policy.CLPF_T_REWARD, policy.CLPF_T_NET, policy.CLPF_T_SOC
NA = policy.CLPF_NA
BLOCK = abi.CL_ROW0_BLOCK
FAMILIES = [0, 1]
SHAPES = [(4, 4), (4, 32), (32, 4), (16, 32), (32, 32)]
GAUSS_MAX = float(np.sqrt(-2.0 * np.log(2.0 ** -25)))            # Box-Muller on u1 >= 2^-25: |z| <= 5.887


def _kernel(f64, mma, kind='RewardFunction'):
    return f"cl_rollout_full_policy_deep_kernel<{2 if f64 == 'chain' else 0}, {mma}, {'true' if kind == 'MARL' else 'false'}>"


def _setup(E, f64='chain', kind='RewardFunction', H=(16, 32), mma=0, sigma=None, district='g2020_cz1', mid_scale=None, seed=None, **kw):
    """Two parameter sets wherever the batch crosses a CL_ROW0_BLOCK: block g runs set g % 2."""
    spec = thermal_district(district)
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    blocks = -(-E // BLOCK)
    sob = [g % 2 for g in range(blocks)] if blocks > 1 else None
    pol = make_deep_storage_policy(layout, *H, n_sets=2 if sob else 1, seed=sum(H) if seed is None else seed, sigma=sigma, mid_scale=mid_scale)
    pt = pol.pack(layout, tab, device='cuda:0', set_of_block=sob, matrix_cores=bool(mma))
    eng = StepEngine(tab, E, reward=kind, f64_maps=f64, **kw)
    eng.trace_kernels()
    return spec, tab, layout, pol, pt, eng


def _roll(eng, pt, K, seed=0):
    ret = torch.zeros(eng.n_env, device='cuda')
    traj = torch.full((K, policy.CLPF_NT, eng.n_bldg, eng.n_env), float('nan'), device='cuda')
    eng.rollout_policy(K, pt, seed=seed, ret_env=ret, traj=traj)
    assert not torch.isnan(traj).any()
    return ret, traj


def _teacher_forced(tab, layout, pol, pt, traj, seed=0, row0=0, env_offset=0, sets=None):
    """(kernel's worst |action - float64 MLP| over the heads that exist, a float32 torch evaluation's, on the recorded inputs of every step);
    `sets`: the parameter set of every block of CL_ROW0_BLOCK envs (default: `_setup`'s g % 2 where the policy has two sets)."""
    K, E = traj.shape[0], traj.shape[3]
    hobs = HostObservations(layout, tab, THERMAL_PLANES)
    tr = traj.cpu().numpy().astype(np.float64)
    xs = [hobs.at(row0, None, reset=True, E=E)] + [hobs.at(row0 + k, *tr[k - 1, S:S + 4], tr[k - 1, N]) for k in range(1, K)]
    x = np.stack(xs)                                                                  # [K, E, B, n_obs]
    z = None
    if np.any(pt.sigma_bldg > 0):
        z = np.stack([replay_noise(pt, seed, E, k, env_offset) for k in range(K)])
    got = tr[:, A:A + NA].transpose(0, 3, 2, 1)                                       # [K, 4, B, E] -> [K, E, B, 4]
    assert not got[:, :, pt.cols < 0].any()                                           # a head without a column: plane written as 0
    dev_kernel = dev_f32 = 0.0
    for g in range(-(-E // BLOCK)):
        s = (g % 2 if pol.n_sets > 1 else 0) if sets is None else sets[g]
        sl = slice(g * BLOCK, min(E, (g + 1) * BLOCK))
        zg = None if z is None else z[:, sl]
        ref = pol.actions_host(x[:, sl], pt, noise=zg, set_index=s)
        dev_kernel = max(dev_kernel, float(np.abs(got[:, sl] - ref).max()))
        dev_f32 = max(dev_f32, f32_torch_deviation(pol, x[:, sl], pt, device='cuda', noise=zg, set_index=s))
    return dev_kernel, dev_f32


def _gate(pol, pt, dev_f32, mma):
    """4 x the float32 torch deviation on the same inputs (the project's gate), for the matrix-core family plus the split's bound (worst set)."""
    return 4.0 * dev_f32 + (max(split_bound(pol, pt, s) for s in range(pol.n_sets)) if mma else 0.0)


def _check_1(E, f64, H, mma, sigma, district, K=24):
    spec, tab, layout, pol, pt, eng = _setup(E, f64, H=H, mma=mma, sigma=sigma, district=district)
    _, traj = _roll(eng, pt, K, seed=11)
    assert eng.last_kernels == _kernel(f64, mma), eng.last_kernels
    dev_kernel, dev_f32 = _teacher_forced(tab, layout, pol, pt, traj, seed=11)
    gate = _gate(pol, pt, dev_f32, mma)
    print(f'teacher-forced {district} E={E} f64={f64} H={H} MMA={mma} sigma={sigma}: kernel {dev_kernel:.3e}  float32 torch {dev_f32:.3e}  '
          f'ratio {dev_kernel / dev_f32:.2f}  gate {gate:.3e}')
    record_worst({'kernel': dev_kernel, 'float32_torch': dev_f32, 'gate': gate}, f'deep thermal policy teacher-forced {district} E={E} f64_maps={f64} H={H} MMA={mma} sigma={sigma}')
    assert dev_f32 > 0 and dev_kernel <= gate, (dev_kernel, dev_f32, gate)
    act = traj[:, A:A + NA].cpu().numpy().transpose(0, 3, 2, 1)[:, :, pt.cols >= 0]
    assert np.abs(act).max() > 0.01 and np.ptp(act) > 0.02                            # a policy that does something
    return tab, pt, traj


# ---- 1. teacher-forced -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sigma', [None, 0.1])
@pytest.mark.parametrize('mma', FAMILIES)
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('H', SHAPES)
def test_1_teacher_forced_actions(H, f64, mma, sigma):
    """(1) Every recorded action of every head recomputed in float64 from the previous step's recorded planes (the reset observation at step 0;
    the noise replayed from the Philox stream), K = 24, nine buildings x 260 envs: a ragged tile, two parameter sets live.  Gate: 4 x the worst
    deviation of a float32 torch evaluation of the unsplit MLP on the same inputs, for MMA = 1 plus `split_bound`.  Measured on MI355X:
    profiles/policy_full_deep_parity.md; both figures are printed here."""
    _check_1(260, f64, H, mma, sigma, 'g2020_cz1')


@pytest.mark.parametrize('mma', FAMILIES)
@pytest.mark.parametrize('E,district,H', [(64, 'g2020_cz1', (16, 32)), (4096, 'g2020_cz1', (16, 32)), (64, 't16', (32, 32)), (64, 't1', (16, 32)),
                                          (64, 't2', (16, 32))])
def test_1_teacher_forced_geometry_edges(E, district, H, mma):
    """(1) on one tile and on 4096 envs; on sixteen buildings at 32 x 32 (nw = 16 and 104 448 bytes of LDS: the opt-in above 64 KiB); on one
    building (one wave owns every reduction row) and on two, one with and one without DHW storage (the head's plane is written as 0)."""
    spec, tab, layout = thermal_district(district), None, None
    assert len(spec.buildings) == {'g2020_cz1': 9, 't16': 16, 't1': 1, 't2': 2}[district]
    tab, pt, traj = _check_1(E, 'chain' if mma == 0 else False, H, mma, 0.1, district)
    if district == 't16':
        assert _lib.policy_full_deep_lds_bytes(16, 32, 32, bool(mma)) == 104448 > 64 * 1024
    if district == 't2':
        assert pt.cols[0, policy.CLPF_A_DS] >= 0 and pt.cols[1, policy.CLPF_A_DS] < 0 and not traj[:, A + policy.CLPF_A_DS, 1].any()


# ---- 2. the two families -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('H', [(4, 4), (16, 32), (32, 32)])
def test_2_the_two_families_on_the_same_inputs(H, f64):
    """(2) The same policy and the same inputs through both families, one step at a time from one state (the exact family's, carried by a
    checkpoint): every head's action within `split_bound` + the exact family's own tolerance (4 x the float32 torch deviation on these inputs)."""
    E, K = 260, 8
    spec, tab, layout, pol, pt0, e0 = _setup(E, f64, H=H, mma=0, sigma=0.1)
    pt1 = pol.pack(layout, tab, device='cuda:0', set_of_block=[0, 1], matrix_cores=True)
    e1 = StepEngine(tab, E, f64_maps=f64)
    e1.trace_kernels()
    worst, steps = 0.0, []
    for k in range(K):
        e1.load_state_dict(e0.state_dict())
        _, t0 = _roll(e0, pt0, 1, seed=6)
        _, t1 = _roll(e1, pt1, 1, seed=6)
        assert e0.last_kernels == _kernel(f64, 0) and e1.last_kernels == _kernel(f64, 1) and e0.t == e1.t == k + 1
        worst = max(worst, float((t0[:, A:A + NA] - t1[:, A:A + NA]).abs().max()))
        steps.append(t0)
    _, dev_f32 = _teacher_forced(tab, layout, pol, pt0, torch.cat(steps), seed=6)
    bound = _gate(pol, pt1, dev_f32, 1)
    print(f'two families H={H} f64={f64}: |action difference| {worst:.3e}, split_bound + 4 x float32 deviation {bound:.3e}')
    record_worst({'difference': worst, 'bound': bound}, f'deep thermal policy two families H={H} f64_maps={f64}')
    assert worst <= bound


# ---- 3. replay ---------------------------------------------------------------------------------------------------------------------------
def _check_3(kind, E, f64, mma, district, H=(16, 32)):
    spec, tab, layout, pol, pt, eng = _setup(E, f64, kind, H=H, mma=mma, sigma=0.1, district=district)
    ret, traj = _roll(eng, pt, 30, seed=5)
    assert eng.last_kernels == _kernel(f64, mma, kind), eng.last_kernels
    _replay(tab, pt, eng, ret, traj, kind, f64)


@pytest.mark.parametrize('mma', FAMILIES)
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('kind', KINDS)
def test_3_replay_through_single_steps(kind, f64, mma):
    """(3) K = 30 (across a day boundary), noise on, 260 envs: the recorded actions of all four heads through `step()` of a second engine --
    all six state planes, net, reward, the district sums and the return, at tests/test_gpu_policy_full_rollout.py::_replay's tolerances.  MARL
    is instantiated in both families."""
    _check_3(kind, 260, f64, mma, 'g2020_cz1')


@pytest.mark.parametrize('mma', FAMILIES)
@pytest.mark.parametrize('district', ['t1', 't16'])
def test_3_replay_geometry_edges(district, mma):
    """(3) on one building and on sixteen at 32 x 32, one tile, MARL (the exchange row with one wave and with sixteen)."""
    _check_3('MARL', 64, 'chain', mma, district, H=(32, 32))


# ---- 4. free-running ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mma', FAMILIES)
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('kind', KINDS)
def test_4_free_running_against_the_cpu(kind, f64, mma):
    """(4) K = 48 from reset at the free-running scale: the host loop of `COracle.step` + `actions_host` (float64) against one launch, at the
    plain bar 1e-4 + 1e-4 |ref| on soc, cs, ds, degraded capacity, net, reward and district net."""
    E, K = 64, 48
    spec, tab, layout, pol, pt, eng = _setup(E, f64, kind, H=(16, 32), mma=mma, mid_scale=FREE_MID_SCALE)
    want = host_closed_loop(spec, tab, layout, pol, pt, K, E, reward=kind)
    _, traj = _roll(eng, pt, K)
    tr = traj.cpu().numpy().astype(np.float64)
    bar = lambda got, ref: float((np.abs(got - ref) / (1e-4 + 1e-4 * np.abs(ref))).max())
    worst = {'soc': bar(tr[:, S], want['soc']), 'cs': bar(tr[:, S + 1], want['cs']), 'ds': bar(tr[:, S + 3], want['ds']),
             'net': bar(tr[:, N], want['net']), 'reward': bar(tr[:, R], want['reward']),
             'district_net': bar(tr[:, N].sum(axis=1), want['dnet']),
             'degraded_capacity': bar(eng.degraded_capacity.cpu().numpy(), want['degcap'][-1])}
    print(f'free-running {kind} f64={f64} MMA={mma}:', {k: round(v, 4) for k, v in worst.items()})
    assert np.abs(want['cs']).max() > 0.05 and not tr[:, S + 2].any() and eng.last_kernels == _kernel(f64, mma, kind)
    check_worst(worst, f'deep thermal policy rollout {kind} f64={f64} MMA={mma}')


# ---- 5. bit for bit ----------------------------------------------------------------------------------------------------------------------
def _check_5_split(f64, mma, district):
    E = 260
    spec, tab, layout, pol, pt, one = _setup(E, f64, 'MARL', mma=mma, sigma=0.1, district=district)
    ret1, traj1 = _roll(one, pt, 12, seed=3)
    assert one.last_kernels == _kernel(f64, mma, 'MARL'), one.last_kernels
    for restore in (False, True):
        eng = StepEngine(tab, E, reward='MARL', f64_maps=f64)
        ret, parts = torch.zeros(E, device='cuda'), []
        for n, K in enumerate((5, 7)):
            if n == 1 and restore:
                sd = eng.state_dict()
                eng = StepEngine(tab, E, reward='MARL', f64_maps=f64)
                eng.load_state_dict(sd)
            traj = torch.empty((K, policy.CLPF_NT, eng.n_bldg, E), device='cuda')
            eng.rollout_policy(K, pt, seed=3, ret_env=ret, traj=traj)
            parts.append(traj)
        assert eng.t == 12 and torch.equal(torch.cat(parts), traj1), restore
        assert torch.equal(eng.state, one.state) and torch.equal(eng.out_bldg[:2], one.out_bldg[:2]) and torch.equal(eng.out_env, one.out_env)
        torch.testing.assert_close(ret, ret1, rtol=1e-6, atol=1e-4)               # (two partial sums instead of one)
    return tab, traj1


@pytest.mark.parametrize('mma', FAMILIES)
@pytest.mark.parametrize('f64', ['chain', False])
def test_5_split_launches_and_checkpoint_are_bit_identical(f64, mma):
    """(5) One launch of K = 12 equals 5 + 7 bit for bit (the previous net travels through out_bldg, t == 0 uses net_reset), also with a
    checkpoint restored into a fresh engine in between; MARL, noise on, two parameter sets."""
    _check_5_split(f64, mma, 'g2020_cz1')


@pytest.mark.parametrize('mma', FAMILIES)
@pytest.mark.parametrize('f64', ['chain', False])
def test_5_windows_sets_and_env_offsets(f64, mma):
    """(5) Two env blocks with different episode windows AND different parameter sets in one launch: each block equals, bit for bit, an engine
    of its own with that window, that set and its env offset (noise on: the half batches reproduce the whole batch's streams); block 1's
    actions are its window's and its set's (teacher-forced)."""
    spec = thermal_district('g2020_cz1')
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    pol = make_deep_storage_policy(layout, 16, 32, n_sets=2, seed=2, sigma=0.1)
    K, n_steps, rows = 24, 200, [0, 131]
    pack = lambda sob: pol.pack(layout, tab, device='cuda:0', set_of_block=sob, matrix_cores=bool(mma))
    whole = StepEngine(tab, 2 * BLOCK, f64_maps=f64, n_steps=n_steps, env_row0=rows)
    whole.trace_kernels()
    _, traj = _roll(whole, pack([0, 1]), K, seed=9)
    assert whole.last_kernels == _kernel(f64, mma), whole.last_kernels
    assert not torch.equal(traj[:, A:A + NA, :, :BLOCK], traj[:, A:A + NA, :, BLOCK:])
    for g in range(2):
        part = StepEngine(tab, BLOCK, f64_maps=f64, n_steps=n_steps, env_row0=[rows[g]], env_offset=BLOCK * g)
        _, tr = _roll(part, pack([g]), K, seed=9)
        sl = slice(BLOCK * g, BLOCK * (g + 1))
        assert torch.equal(tr, traj[:, :, :, sl]), g
        assert torch.equal(part.state, whole.state[:, :, sl]) and torch.equal(part.out_env, whole.out_env[:, sl])
    pt_host = pol.pack(layout, tab, matrix_cores=bool(mma))
    dev_kernel, dev_f32 = _teacher_forced(tab, layout, pol, pt_host, traj[:, :, :, BLOCK:], seed=9, row0=rows[1], env_offset=BLOCK, sets=[1])
    print(f'window 1 / set 1 teacher-forced MMA={mma}: kernel {dev_kernel:.3e}  float32 torch {dev_f32:.3e}')
    assert dev_kernel <= 4.0 * dev_f32 + (split_bound(pol, pt_host, 1) if mma else 0.0)


@pytest.mark.parametrize('mma', FAMILIES)
def test_5_seeds_and_the_noise_bound(mma):
    """(5) The same seed gives the same trajectory bit for bit, another seed another.  At step 0 every env sees the reset observation, so a noisy
    launch's actions differ from the deterministic launch's by sigma z alone: within sigma x the Box-Muller bound sqrt(-2 ln 2^-25) = 5.887 (+ one
    float32 rounding of the sum), not all the same over the envs, and 0 where the head has no column."""
    E, sigma = 260, 0.02
    spec, tab, layout, pol, pt, eng = _setup(E, False, mma=mma, sigma=sigma)
    _, traj = _roll(eng, pt, 12, seed=1)
    _, again = _roll(_setup(E, False, mma=mma, sigma=sigma)[5], pt, 12, seed=1)
    _, other = _roll(_setup(E, False, mma=mma, sigma=sigma)[5], pt, 12, seed=2)
    assert torch.equal(again, traj) and not torch.equal(other[:, A:A + NA], traj[:, A:A + NA])
    quiet = policy.DeepStorageMLPPolicy(pol.w1, pol.b1, pol.w2, pol.b2, pol.w3, pol.b3)
    _, det = _roll(_setup(E, False, mma=mma)[5], quiet.pack(layout, tab, device='cuda:0', set_of_block=[0, 1], matrix_cores=bool(mma)), 1)
    has = torch.as_tensor(pt.cols >= 0, device='cuda').t()[:, :, None]                           # [4, B, 1]
    d = (traj[0, A:A + NA] - det[0, A:A + NA]).abs()
    assert float(d.max()) <= sigma * GAUSS_MAX + 1e-6 and not bool(d[(~has).expand_as(d)].any())
    assert float(d[has.expand_as(d)].max()) > sigma and bool((d[:, :, :1] != d).any())
    lo = torch.as_tensor(pt.low_bldg.T, dtype=torch.float32, device='cuda')[None, :, :, None]
    hi = torch.as_tensor(pt.high_bldg.T, dtype=torch.float32, device='cuda')[None, :, :, None]
    act = traj[:, A:A + NA]
    assert bool(((act >= lo) & (act <= hi) | ~has[None]).all())


# ---- 6. the outage district --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mma', FAMILIES)
@pytest.mark.parametrize('f64', ['chain', False])
def test_6_outage_teacher_forced(f64, mma):
    """(1) on the nine-building outage district at E = 260, noise on: after an outage row the observation carries a net of exactly 0 and socs the
    outage unit wrote; net is exactly 0 on the outage (row, building) pairs and on no other."""
    tab, pt, traj = _check_1(260, f64, (16, 32), mma, 0.1, 'g2020_cz1_outage')
    assert _net_is_zero_on_outage_rows_only(tab, traj) and outage_mask(tab, 24).any()


@pytest.mark.parametrize('mma', FAMILIES)
@pytest.mark.parametrize('kind,f64', [('RewardFunction', 'chain'), ('MARL', False)])
def test_6_outage_replay(kind, f64, mma):
    """(3) on the outage district at E = 260 (`_replay` also checks net == 0 on the outage pairs and on no other)."""
    _check_3(kind, 260, f64, mma, 'g2020_cz1_outage')


@pytest.mark.parametrize('mma', FAMILIES)
def test_6_outage_split_launches(mma):
    """(5) on the outage district: the boundary at step 5 is the first outage row of building 0 (the net the next launch reads back from out_bldg
    is an outage row's 0)."""
    tab, traj = _check_5_split('chain', mma, 'g2020_cz1_outage')
    m = outage_mask(tab, 12)
    assert _net_is_zero_on_outage_rows_only(tab, traj) and not m[:5].any() and m[5, 0] and m[6, 1]


# ---- 7. env level ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mma', FAMILIES)
def test_7_env_level_equals_capture_rollout_with_the_torch_mlp(mma, monkeypatch):
    """(7) `VectorCityLearnEnv.rollout_policy(policy, K, record=True)` against `capture_rollout` driven by `torch_policy` over
    `observations='tensor'`, at the tolerances of tests/test_gpu_policy_full_rollout.py::test_g: per-step actions at the teacher-forced tolerance
    (4 x a float32 evaluation's deviation, measured here on the recorded inputs; MMA = 1: plus `split_bound`), once more for the float32 torch
    policy's own deviation, widened by what the two paths' state tolerance (2e-6 on the socs, 2e-5 on net, relative + absolute) can move an action
    through THREE layers: dz1_j = sum_d |W1_j,d| scale_d tol_d, dz2_i = sum_j |W2_ij| dz1_j, da = half_a sum_i |w3_ai| dz2_i (tanh' <= 1);
    returns at rtol 1e-5 / atol 1e-3.  The tables cache honours `update()`; `kpi=True` names the replay route."""
    from citylearn_amd.vector_env import VectorCityLearnEnv
    monkeypatch.setattr(policy, 'default_thermal_matrix_cores', lambda h1, h2, n_bldg=None: bool(mma))      # (the env packs with matrix_cores=None)
    g = golden('g2020_cz1')
    E, K = 256, 24
    a, b = (VectorCityLearnEnv(g.schema_path, E, observations='tensor', normalize_observations=True) for _ in range(2))
    a.engine.trace_kernels()
    pol = make_deep_storage_policy(a.layout, 16, 32, seed=4)
    with pytest.raises(NotImplementedError, match='no KPI kernel for a policy with two hidden layers.*record=True.*CLPF_T_ACTION.*kpi=True'):
        a.rollout_policy(pol, K, kpi=True)
    ret, traj = a.rollout_policy(pol, K, record=True)
    assert a._t == K == a.engine.t and traj.shape == (K, policy.CLPF_NT, a.n_bldg, E) and a.engine.last_kernels == _kernel('chain' if a.engine.f64_chain else False, mma)
    pt_host = pol.pack(a.layout, a.tables)
    assert pt_host.matrix_cores == bool(mma)
    f = pol.torch_policy(b.layout, b.tables, b.device)
    acts = torch.zeros((K, b.n_act_cols, E), device='cuda')

    def recorded(obs, i):
        acts[i].copy_(f(obs, i))
        return acts[i]
    cap = b.capture_rollout(recorded, K)
    _, rewards, _ = cap.run()
    torch.cuda.synchronize()
    dev_kernel, dev_f32 = _teacher_forced(a.tables, a.layout, pol, pt_host, traj)
    hobs = HostObservations(a.layout, a.tables, THERMAL_PLANES)
    w1, _, w2, _, w3, _ = (v[0] for v in pol._full(a.n_bldg))                      # [B, H1, n_obs], [B, H2, H1], [B, 4, H2]
    tr = traj.cpu().numpy().astype(np.float64)
    tols = [2e-6 * (1 + np.abs(tr[:, S + d]).max()) for d in range(4)] + [2e-5 * (1 + np.abs(tr[:, N]).max())]
    dz1 = sum(np.abs(w1 * np.where(hobs.is_term[d], hobs.scale, 0.0)[:, None, :]).sum(axis=2) * tols[d] for d in range(5))        # [B, H1]
    dz2 = np.einsum('bij,bj->bi', np.abs(w2), dz1)                                 # [B, H2]
    half = 0.5 * (pt_host.high_bldg - pt_host.low_bldg)                            # [B, 4]
    widen = float((half * (np.abs(w3) * dz2[:, None, :]).sum(axis=2)).max())
    tol = 4.0 * dev_f32 + dev_f32 + widen + (split_bound(pol, pt_host) if mma else 0.0)
    b_idx, h_idx = np.nonzero(pt_host.cols >= 0)
    got = traj[:, A:A + NA][:, torch.as_tensor(h_idx, device='cuda'), torch.as_tensor(b_idx, device='cuda')]      # [K, heads, E]
    want = acts[:, torch.as_tensor(pt_host.cols[b_idx, h_idx], device='cuda')]
    worst = float((got - want).abs().max())
    print(f'env level MMA={mma}: |action difference| {worst:.3e}, tolerance {tol:.3e} (float32 deviation {dev_f32:.3e}, state term {widen:.3e})')
    assert worst <= tol
    torch.testing.assert_close(ret, rewards.sum(dim=0) if rewards.dim() == 2 else rewards.sum(dim=(0, 1)), rtol=1e-5, atol=1e-3)
    torch.testing.assert_close(a.engine.state, b.engine.state, rtol=2e-6, atol=2e-6)
    # the cache: the same policy object is not packed again, `update()` is honoured
    (cached_pol, cached), = a._policy_tables.values()
    a.rollout_policy(pol, 1)
    assert cached_pol is pol and next(iter(a._policy_tables.values()))[1] is cached and cached.version == 0
    a.reset()
    pol.update(w3=-pol.w3)
    _, flipped = a.rollout_policy(pol, 1, record=True)
    fresh = next(iter(a._policy_tables.values()))[1]
    assert fresh is not cached and fresh.version == 1 and torch.equal(fresh.out[..., :-1], -cached.out[..., :-1])
    assert not torch.equal(flipped[0, A:A + NA], traj[0, A:A + NA])
    dev_kernel, dev_f32 = _teacher_forced(a.tables, a.layout, pol, pol.pack(a.layout, a.tables), flipped)
    assert dev_kernel <= _gate(pol, fresh, dev_f32, mma)


def test_7_refusals():
    """(7) `kpi=True` raises `NotImplementedError` naming the replay route -- on the engine with and without KPIs, and on a 17-building thermal
    env, where the refusal comes before the library's n_bldg > 16; `chunked=True` on the engine is a `ValueError` (no chunked kernel at all);
    seventeen buildings and a `kpi=True` engine are the library's refusals; a `DeepStorageMLPPolicy` on a battery + PV env is sent to
    `clpd_rollout_mlp_f32` by name and a `DeepMLPPolicy` on a thermal env is the packer's refusal by name.  Every plane stays what it was, and
    the engine still runs afterwards."""
    from citylearn_amd.synthetic import tile_district
    from citylearn_amd.vector_env import VectorCityLearnEnv
    from policy_deep_util import make_deep_policy
    E, K = 64, 4
    spec, tab, layout, pol, pt, plain = _setup(E, False, H=(8, 8))
    spec17, tab17, lay17, pol17, pt17, eng17 = _setup(E, False, H=(8, 8), district='t17')
    route = 'no KPI kernel for a policy with two hidden layers.*replay its action planes \\(policy.CLPF_T_ACTION \\+ head.*kpi=True'
    cases = [('kpi=True', plain, pt, {'kpi': True}, NotImplementedError, route),
             ('kpi=True on a kpi engine', StepEngine(tab, E, f64_maps=False, kpi=True), pt, {'kpi': True}, NotImplementedError, route),
             ('kpi engine', StepEngine(tab, E, f64_maps=False, kpi=True), pt, {}, _lib.EngineError, 'clpfd_rollout_mlp_f32.*CLD_KPI'),
             ('chunked=True', plain, pt, {'chunked': True}, ValueError, 'no building-chunked policy kernel for DeepStoragePolicyTables at all'),
             ('chunked=True, 17 buildings', eng17, pt17, {'chunked': True}, ValueError, 'no building-chunked policy kernel for DeepStoragePolicyTables at all'),
             ('f64_maps=True', StepEngine(tab, E, f64_maps=True), pt, {}, _lib.EngineError, 'clpfd_rollout_mlp_f32.*CLD_F64_MAPS'),
             ('17 buildings', eng17, pt17, {}, _lib.EngineError, 'clpfd_rollout_mlp_f32: n_bldg=17 > 16 would be a building-chunked launch'),
             ('tables of another engine', plain, pt17, {}, ValueError, 'policy tables are packed for')]
    for name, eng, tables, kw, exc, match in cases:
        ret = torch.full((E,), 3.0, device='cuda')
        traj = torch.full((K, policy.CLPF_NT, eng.n_bldg, E), -7.0, device='cuda')
        before = [x.clone() for x in (eng.state, eng.out_bldg, eng._out_env, ret, traj)]
        with pytest.raises(exc, match=match):
            eng.rollout_policy(K, tables, ret_env=ret, traj=traj, **kw)
        torch.cuda.synchronize()
        assert eng.t == 0, name
        for x, was in zip((eng.state, eng.out_bldg, eng._out_env, ret, traj), before):
            assert torch.equal(x, was), name
    _roll(plain, pt, K)
    assert plain.last_kernels == _kernel(False, 0)
    # env level
    env17 = VectorCityLearnEnv(tile_district(golden('g2020_cz1').spec(), 17), E, observations='tensor', normalize_observations=True)
    dpol17 = make_deep_storage_policy(env17.layout, 8, 8)
    with pytest.raises(NotImplementedError, match='no KPI kernel for a policy with two hidden layers.*record=True.*kpi=True'):
        env17.rollout_policy(dpol17, K, kpi=True)
    with pytest.raises(_lib.EngineError, match='clpfd_rollout_mlp_f32: n_bldg=17 > 16'):
        env17.rollout_policy(dpol17, K)
    lean = VectorCityLearnEnv(golden('g2022_all').schema_path, E, observations='tensor', normalize_observations=True)
    with pytest.raises(_lib.EngineError, match='clpfd_rollout_mlp_f32: thermal / outage districts only.*clpd_rollout_mlp_f32'):
        lean.rollout_policy(make_deep_storage_policy(lean.layout, 8, 8), K)
    thermal = VectorCityLearnEnv(golden('g2020_cz1').schema_path, E, observations='tensor', normalize_observations=True)
    with pytest.raises(ValueError, match="the policy kernel only has the building's own electrical_storage_soc"):
        thermal.rollout_policy(make_deep_policy(thermal.layout, 8, 8), K)
    assert lean._t == thermal._t == env17._t == 0
