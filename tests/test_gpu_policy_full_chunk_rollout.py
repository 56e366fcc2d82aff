"""The building-chunked closed-loop policy rollout of thermal districts on the GPU (`StepEngine.rollout_policy(chunked=True)` /
`VectorCityLearnEnv.rollout_policy` with a `StorageMLPPolicy` on a district of more than 16 buildings: one launch of
`cl_rollout_full_policy_chunk_kernel`, csrc/cl_policy_full.h at CHUNK = true, and one of `cl_finish_kernel`): (1) against the one-row kernel on the
sixteen-building district, (2) its trajectory replayed through `step()`, (3) its actions teacher-forced against the float64 MLP, (4) free-running
against the CPU oracle, (5) launch splitting and checkpoints bit for bit, (6) episode windows x parameter sets x env offsets bit for bit, (7) the
accumulated return, (8) the env-level call against `capture_rollout`, (9) refusals.  Helpers and tolerances: tests/test_gpu_policy_full_rollout.py
(`_replay`, `_teacher_forced`); districts: tests/policy_full_chunk_util.py; weights: tests/policy_full_util.py (scale fixed by the conditioning
tests of tests/test_policy_full_host.py and tests/test_policy_full_chunk_host.py).  The float64 chain exists at one env per lane only."""
import numpy as np
import pytest
import torch

from golden_util import check_worst, record_worst
from citylearn_amd import _lib, abi, policy
from citylearn_amd.engine import StepEngine
from citylearn_amd.observations import ObservationLayout
from policy_full_chunk_util import chunk_district, default_chunks
from policy_full_util import THERMAL_PLANES, host_closed_loop, make_storage_policy, outage_mask
from policy_util import HostObservations
from test_gpu_policy_full_rollout import A, N, NA, R, S, _net_is_zero_on_outage_rows_only, _replay, _teacher_forced

pytestmark = pytest.mark.gpu

KINDS = ['RewardFunction', 'IndependentSACReward', 'SolarPenaltyReward']          # (MARL couples the buildings inside a step: refused, test 9)
PRECISIONS = [('chain', 1), (False, 1), (False, 2)]                                # (f64_maps, envs per lane)


def _setup(district, E, f64='chain', kind='RewardFunction', H=16, sigma=None, b_chunk=0, vec=0, n_sets=1, set_of_block=None, **kw):
    spec = chunk_district(district)
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    pol = make_storage_policy(layout, H, n_sets=n_sets, seed=H, sigma=sigma)
    pt = pol.pack(layout, tab, device='cuda:0', set_of_block=set_of_block)
    tuning = {}
    if b_chunk:
        tuning['b_chunk'] = b_chunk
    if vec and f64 != 'chain':
        tuning['vec'] = vec
    eng = StepEngine(tab, E, reward=kind, f64_maps=f64, tuning=tuning or None, **kw)
    eng.trace_kernels()
    return spec, tab, layout, pol, pt, eng


def _roll(eng, pt, K, seed=0, chunked=True):
    ret = torch.zeros(eng.n_env, device='cuda')
    traj = torch.full((K, policy.CLPF_NT, eng.n_bldg, eng.n_env), float('nan'), device='cuda')
    eng.rollout_policy(K, pt, seed=seed, ret_env=ret, traj=traj, **({'chunked': True} if chunked else {}))
    assert not torch.isnan(traj).any()
    return ret, traj


def _names(f64, vec=0):
    """`last_kernels` of a chunked call: the chunk kernel's instantiation and the fold, nothing else."""
    return f"cl_rollout_full_policy_chunk_kernel<{1 if f64 == 'chain' else (vec or 2)}, {2 if f64 == 'chain' else 0}>+cl_finish_kernel"


# ---- 1. against the one-row kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('f64,vec', PRECISIONS)
@pytest.mark.parametrize('b_chunk', [8, 6])
def test_1_sixteen_buildings_equal_the_one_row_kernel(b_chunk, f64, vec, kind):
    """(1) 't16' cut 8 + 8 and 6 + 6 + 4 (a last chunk with two waves without a building) against `cl_rollout_full_policy_kernel` on the same
    district: same seed, sigma = 0.1, K = 30, E = 260 (ragged tile).  Record, state planes and out_bldg[:2] at `_replay`'s tolerances (2e-6 on
    actions and socs, 2e-5 on net and reward); out_env at 1e-4 and the return at rtol 1e-5 / atol 1e-3: the district sums are associated per chunk
    first.  Each wave runs the one-row kernel's arithmetic on its building, so the per-building planes are expected to be EQUAL bit for bit:
    recorded per case (`bit_equal`), not gated."""
    E, K = 260, 30
    spec, tab, layout, pol, pt, one = _setup('t16', E, f64, kind, sigma=0.1, vec=vec)
    ret1, traj1 = _roll(one, pt, K, seed=5, chunked=False)
    assert one.last_kernels == f"cl_rollout_full_policy_kernel<{1 if f64 == 'chain' else vec}, {2 if f64 == 'chain' else 0}, false>", one.last_kernels
    eng = _setup('t16', E, f64, kind, sigma=0.1, vec=vec, b_chunk=b_chunk)[5]
    ret, traj = _roll(eng, pt, K, seed=5)
    assert eng.last_kernels == _names(f64, vec), eng.last_kernels
    torch.testing.assert_close(traj[:, A:A + NA], traj1[:, A:A + NA], rtol=2e-6, atol=2e-6)
    torch.testing.assert_close(traj[:, S:S + 4], traj1[:, S:S + 4], rtol=2e-6, atol=2e-6)
    torch.testing.assert_close(traj[:, N], traj1[:, N], rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(traj[:, R], traj1[:, R], rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(eng.state[:6], one.state[:6], rtol=2e-6, atol=2e-6)
    torch.testing.assert_close(eng.out_bldg[:2], one.out_bldg[:2], rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(eng.out_env, one.out_env, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(ret, ret1, rtol=1e-5, atol=1e-3)
    bit = torch.equal(traj, traj1) and torch.equal(eng.state[:6], one.state[:6]) and torch.equal(eng.out_bldg[:2], one.out_bldg[:2])
    sums = float(((eng.out_env - one.out_env).abs() / (1e-4 + 1e-4 * one.out_env.abs())).max())
    print(f't16 b_chunk={b_chunk} f64={f64} vec={vec} {kind}: per-building planes bit-equal {bit}; district sums {sums:.4f} x the plain bar')
    record_worst({'bit_equal': float(bit), 'district_sums': sums, 'return': float((ret - ret1).abs().max())},
                 f'chunked thermal policy rollout vs one-row kernel t16 b_chunk={b_chunk} {kind} f64_maps={f64} vec={vec}')


# ---- 2. replay through single steps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('E', [64, 260])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('district,b_chunk', [('t17', 0), ('t17', 8), ('t17', 16), ('t24', 8), ('t33', 0), ('t17_outage', 0)])
def test_2_replay_through_single_steps(district, b_chunk, kind, E, f64):
    """(2) K = 30 (across a day boundary), noise on, `_replay`'s tolerances: 17 buildings cut 6 + 6 + 5 (the default), 8 + 8 + 1 and 16 + 1
    (workgroup rows of ONE building beside full ones: seven / fifteen waves that only meet the barriers), 24 as three full chunks of eight, 33
    as 7 + 7 + 7 + 7 + 5, and the 17-building outage district (net exactly 0 on the outage rows and on no others: `_replay`)."""
    spec, tab, layout, pol, pt, eng = _setup(district, E, f64, kind, sigma=0.1, b_chunk=b_chunk)
    if not b_chunk:
        assert default_chunks(eng.n_bldg)[0] == {17: 6, 33: 7}[eng.n_bldg]
    ret, traj = _roll(eng, pt, 30, seed=5)
    assert eng.last_kernels == _names(f64), eng.last_kernels
    _replay(tab, pt, eng, ret, traj, kind, f64)


@pytest.mark.parametrize('f64', ['chain', False])
def test_2_config_4_district_replayed(f64):
    """(2) at the size the kernel is for: BASELINE config 4's 1024 buildings (128 chunks of eight: every wave of the fold adds eight chunks, in
    two passes of its 64-chunk stride) x 64 envs, K = 30, noise on, `_replay`'s tolerances -- a fault in the chunk indexing of the scratch rows
    or the return rows that only shows beyond 16 / 64 chunks would show here."""
    spec, tab, layout, pol, pt, eng = _setup('t1024', 64, f64, sigma=0.1)
    assert default_chunks(eng.n_bldg) == (8, 128)
    ret, traj = _roll(eng, pt, 30, seed=5)
    assert eng.last_kernels == _names(f64), eng.last_kernels
    _replay(tab, pt, eng, ret, traj, 'RewardFunction', f64)


def test_2_without_a_return_buffer():
    """(2) `ret_env=None`: the fold behind the chunk kernel launches NQ workgroup rows instead of NQ + 1.  The smallest shape that chunks -- 17
    buildings cut 6 + 6 + 5 (the default), 64 envs, K = 4: every plane bit for bit what a twin engine that keeps the return leaves, and against
    single steps at `_replay`'s tolerances (the return it checks is the twin's)."""
    E, K = 64, 4
    spec, tab, layout, pol, pt, eng = _setup('t17', E, sigma=0.1)
    twin = _setup('t17', E, sigma=0.1)[5]
    ret, traj_twin = _roll(twin, pt, K, seed=5)
    traj = torch.full_like(traj_twin, float('nan'))
    eng.rollout_policy(K, pt, seed=5, traj=traj, chunked=True)
    assert eng.last_kernels == twin.last_kernels == _names('chain'), eng.last_kernels
    for got, want in ((traj, traj_twin), (eng.state[:6], twin.state[:6]), (eng.out_bldg[:2], twin.out_bldg[:2]), (eng.out_env, twin.out_env)):
        assert torch.equal(got, want)
    _replay(tab, pt, eng, ret, traj, 'RewardFunction', 'chain')


# ---- 3. teacher-forced actions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H', [4, 16, 32])
@pytest.mark.parametrize('f64,vec', PRECISIONS)
def test_3_teacher_forced_actions(f64, vec, H):
    """(3) Every recorded action of every head of 't17' recomputed in float64 from the previous step's recorded planes, noise replayed from the
    Philox stream (E = 260, K = 24).  Gate: 4 x the worst deviation of a float32 torch evaluation of the unsplit MLP on the same inputs."""
    spec, tab, layout, pol, pt, eng = _setup('t17', 260, f64, H=H, sigma=0.1, vec=vec)
    _, traj = _roll(eng, pt, 24, seed=11)
    assert eng.last_kernels == _names(f64, vec), eng.last_kernels
    dev_kernel, dev_f32 = _teacher_forced(tab, layout, pol, pt, traj, seed=11)
    print(f'teacher-forced t17 vec={vec} f64={f64} H={H}: kernel {dev_kernel:.3e}  float32 torch {dev_f32:.3e}  ratio {dev_kernel / dev_f32:.2f}')
    record_worst({'kernel': dev_kernel, 'float32_torch': dev_f32, 'ratio': dev_kernel / dev_f32}, f'chunked thermal policy teacher-forced t17 f64_maps={f64} vec={vec} H={H}')
    assert dev_f32 > 0 and dev_kernel <= 4.0 * dev_f32, (dev_kernel, dev_f32)


# ---- 4. free-running against the CPU ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('district', ['t17', 't33', 't17_outage'])
def test_4_free_running_against_the_cpu(district, f64):
    """(4) K = 48 from reset, H = 16, E = 64: the host loop of `COracle.step` + `actions_host` (float64) against one chunked launch, at the plain
    bar 1e-4 + 1e-4 |ref| on soc, cs, ds, net, reward, district net and degraded capacity.  On the outage district net is exactly 0 on the outage
    (row, building) pairs and on no others."""
    E, K = 64, 48
    spec, tab, layout, pol, pt, eng = _setup(district, E, f64, H=16)
    want = host_closed_loop(spec, tab, layout, pol, pt, K, E)
    _, traj = _roll(eng, pt, K)
    assert eng.last_kernels == _names(f64), eng.last_kernels
    tr = traj.cpu().numpy().astype(np.float64)
    bar = lambda got, ref: float((np.abs(got - ref) / (1e-4 + 1e-4 * np.abs(ref))).max())
    worst = {'soc': bar(tr[:, S], want['soc']), 'cs': bar(tr[:, S + 1], want['cs']), 'ds': bar(tr[:, S + 3], want['ds']),
             'net': bar(tr[:, N], want['net']), 'reward': bar(tr[:, R], want['reward']),
             'district_net': bar(eng.district_net.cpu().numpy().astype(np.float64), want['dnet'][-1]),
             'district_net_of_record': bar(tr[:, N].sum(axis=1), want['dnet']),
             'degraded_capacity': bar(eng.degraded_capacity.cpu().numpy(), want['degcap'][-1])}
    print(f'free-running {district} f64={f64}:', {k: round(v, 4) for k, v in worst.items()})
    assert np.abs(want['cs']).max() > 0.05 and not tr[:, S + 2].any()
    if district.endswith('_outage'):
        m = outage_mask(tab, K)
        assert m.any() and _net_is_zero_on_outage_rows_only(tab, traj) and not want['net'][m].any()
    check_worst(worst, f'chunked thermal policy rollout {district} f64={f64}')


# ---- 5. split launches and checkpoint ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', ['chain', False])
def test_5_split_launches_and_checkpoint_are_bit_identical(f64):
    """(5) 't33': launches of 1, 5, 24 and 25 steps from t0 = 0 equal one 55-step launch bit for bit in record, state, out_bldg[:2] and out_env
    (the previous net travels through out_bldg, t == 0 uses net_reset; every launch ends with its own fold), with a checkpoint restored into a
    fresh engine between two of them; the return at rtol 1e-6 / atol 1e-4 (four partial sums instead of one).  Then one `step()` with zero
    actions on both engines: equal district sums -- the chunked launches left the reserved plane's marker and ticket words usable -- which are
    the sums of the per-building planes (float32 sums of 33 nets of up to ~50 kWh: rtol 1e-5 / atol 1e-3)."""
    E = 320
    spec, tab, layout, pol, pt, one = _setup('t33', E, f64, sigma=0.1)
    ret1, traj1 = _roll(one, pt, 55, seed=3)
    assert one.last_kernels == _names(f64), one.last_kernels
    eng = StepEngine(tab, E, f64_maps=f64)
    ret, parts = torch.zeros(E, device='cuda'), []
    for n, K in enumerate((1, 5, 24, 25)):
        if n == 2:
            sd = eng.state_dict()
            eng = StepEngine(tab, E, f64_maps=f64)
            eng.load_state_dict(sd)
        traj = torch.empty((K, policy.CLPF_NT, eng.n_bldg, E), device='cuda')
        eng.rollout_policy(K, pt, seed=3, ret_env=ret, traj=traj, chunked=True)
        parts.append(traj)
    assert eng.t == 55 and torch.equal(torch.cat(parts), traj1)
    assert torch.equal(eng.state, one.state) and torch.equal(eng.out_bldg[:2], one.out_bldg[:2]) and torch.equal(eng.out_env, one.out_env)
    torch.testing.assert_close(ret, ret1, rtol=1e-6, atol=1e-4)
    zero = torch.zeros((eng.n_act_cols, E), device='cuda')
    eng.step(zero)
    one.step(zero)
    assert eng.t == one.t == 56 and torch.equal(eng.out_env, one.out_env) and torch.equal(eng.district_reward, one.district_reward)
    assert torch.equal(eng.state, one.state) and torch.equal(eng.net, one.net)
    torch.testing.assert_close(eng.district_net, eng.net.sum(dim=0), rtol=1e-5, atol=1e-3)
    torch.testing.assert_close(eng.district_reward, eng.reward_bldg.sum(dim=0), rtol=1e-5, atol=1e-3)


# ---- 6. episode windows x parameter sets x env offsets ----------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', ['chain', False])
def test_6_windows_sets_and_env_offsets(f64):
    """(6) tests/test_gpu_policy_full_rollout.py::_check_e on 't17': two env blocks with different episode windows AND different parameter sets
    in one chunked launch; each block equals, bit for bit, an engine of its own with that window, that set and its env offset (noise on: the half
    batches reproduce the whole batch's streams, which are keyed by the global env whatever the chunk geometry)."""
    spec = chunk_district('t17')
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    pol = make_storage_policy(layout, 16, n_sets=2, seed=2, sigma=0.1)
    K, n_steps, rows = 24, 200, [0, 131]
    whole = StepEngine(tab, 512, f64_maps=f64, n_steps=n_steps, env_row0=rows)
    whole.trace_kernels()
    _, traj = _roll(whole, pol.pack(layout, tab, device='cuda:0', set_of_block=[0, 1]), K, seed=9)
    assert whole.last_kernels == _names(f64), whole.last_kernels
    assert not torch.equal(traj[:, A:A + NA, :, :256], traj[:, A:A + NA, :, 256:])
    for g in range(2):
        part = StepEngine(tab, 256, f64_maps=f64, n_steps=n_steps, env_row0=[rows[g]], env_offset=256 * g)
        _, tr = _roll(part, pol.pack(layout, tab, device='cuda:0', set_of_block=[g]), K, seed=9)
        sl = slice(256 * g, 256 * (g + 1))
        assert torch.equal(tr, traj[:, :, :, sl]), g
        assert torch.equal(part.state, whole.state[:, :, sl]) and torch.equal(part.out_env, whole.out_env[:, sl])
    single = policy.StorageMLPPolicy(pol.w1[1:2], pol.b1[1:2], pol.w2[1:2], pol.b2[1:2], sigma=0.1)
    dev_kernel, dev_f32 = _teacher_forced(tab, layout, single, single.pack(layout, tab), traj[:, :, :, 256:], seed=9, row0=rows[1], env_offset=256)
    print(f'window 1 / set 1 teacher-forced: kernel {dev_kernel:.3e}  float32 torch {dev_f32:.3e}')
    assert dev_kernel <= 4.0 * dev_f32


# ---- 7. the return is accumulated -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', ['chain', False])
def test_7_ret_env_is_accumulated(f64):
    """(7) `ret_env` is added to, not overwritten: a pre-filled one ends at its old value plus the return a zeroed one ends at (the fold adds ONE
    number per env: bit for bit), also over a second launch; and a launch of no steps leaves it alone."""
    E, K = 260, 12
    spec, tab, layout, pol, pt, a = _setup('t17', E, f64, sigma=0.1)
    b = _setup('t17', E, f64, sigma=0.1)[5]
    r0 = torch.zeros(E, device='cuda')
    a.rollout_policy(K, pt, seed=2, ret_env=r0, chunked=True)
    pre = torch.linspace(-300.0, 500.0, E, device='cuda')
    r1 = pre.clone()
    b.rollout_policy(K, pt, seed=2, ret_env=r1, chunked=True)
    assert r0.abs().min() > 0 and torch.equal(r1, pre + r0)
    mid = r1.clone()
    b.rollout_policy(0, pt, seed=2, ret_env=r1, chunked=True)
    assert torch.equal(r1, mid) and b.t == K
    r2 = torch.zeros(E, device='cuda')
    a.rollout_policy(K, pt, seed=2, ret_env=r2, chunked=True)
    b.rollout_policy(K, pt, seed=2, ret_env=r1, chunked=True)
    assert torch.equal(r1, mid + r2) and torch.equal(a.state, b.state)


# ---- 8. env level -----------------------------------------------------------------------------------------------------------------------
def test_8_env_level_routes_by_itself_and_equals_capture_rollout():
    """(8) `VectorCityLearnEnv.rollout_policy(policy, K, record=True)` on 17 buildings routes to the chunked launch by itself; against
    `capture_rollout` driven by `torch_policy` over `observations='tensor'`, at the tolerances of
    tests/test_gpu_policy_full_rollout.py::test_g: per-step actions at the teacher-forced tolerance widened by what the two paths' state
    tolerance (2e-6 on the socs, 2e-5 on net) can move an action through the five dependent weights, and once more for the float32 torch
    policy's own deviation; returns at rtol 1e-5 / atol 1e-3; states at 2e-6.  `kpi=True` names the gap."""
    from citylearn_amd.synthetic import tile_district
    from citylearn_amd.vector_env import VectorCityLearnEnv
    from golden_util import golden
    E, K = 256, 24
    a, b = (VectorCityLearnEnv(tile_district(golden('g2020_cz1').spec(), 17), E, observations='tensor', normalize_observations=True) for _ in range(2))
    a.engine.trace_kernels()
    pol = make_storage_policy(a.layout, 16, seed=4)
    with pytest.raises(NotImplementedError, match='KPI'):
        a.rollout_policy(pol, K, kpi=True)
    ret, traj = a.rollout_policy(pol, K, record=True)
    assert a._t == K == a.engine.t and traj.shape == (K, policy.CLPF_NT, 17, E)
    assert a.engine.last_kernels == _names('chain' if a.engine.f64_chain else False), a.engine.last_kernels
    pt_host = pol.pack(a.layout, a.tables)
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
    w1, w2 = pol._full(a.n_bldg)[0][0], pol._full(a.n_bldg)[2][0]                  # [B, H, n_obs], [B, 4, H]
    tr = traj.cpu().numpy().astype(np.float64)
    tols = [2e-6 * (1 + np.abs(tr[:, S + d]).max()) for d in range(4)] + [2e-5 * (1 + np.abs(tr[:, N]).max())]
    gain = sum(np.abs(w1 * np.where(hobs.is_term[d], hobs.scale, 0.0)[:, None, :]).sum(axis=2) * tols[d] for d in range(5))      # [B, H]
    half = 0.5 * (pt_host.high_bldg - pt_host.low_bldg)                            # [B, 4]
    widen = float((half * (np.abs(w2) * gain[:, None, :]).sum(axis=2)).max())
    tol = 4.0 * dev_f32 + dev_f32 + widen
    b_idx, h_idx = np.nonzero(pt_host.cols >= 0)
    got = traj[:, A:A + NA][:, torch.as_tensor(h_idx, device='cuda'), torch.as_tensor(b_idx, device='cuda')]      # [K, heads, E]
    want = acts[:, torch.as_tensor(pt_host.cols[b_idx, h_idx], device='cuda')]
    worst = float((got - want).abs().max())
    print(f'env level, 17 buildings: |action difference| {worst:.3e}, tolerance {tol:.3e} (float32 deviation {dev_f32:.3e}, state term {widen:.3e})')
    assert worst <= tol
    torch.testing.assert_close(ret, rewards.sum(dim=0) if rewards.dim() == 2 else rewards.sum(dim=(0, 1)), rtol=1e-5, atol=1e-3)
    torch.testing.assert_close(a.engine.state, b.engine.state, rtol=2e-6, atol=2e-6)


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------
def test_9_refusals_leave_every_plane_untouched():
    """(9) A MARL engine and a `kpi=True` engine (the library's refusals, by name), 17 buildings in chunks of five (four chunks need 20 rows of
    the reserved plane's 17), `kpi=True` in the call, `MLPPolicy` tables -- and, with default arguments, the one-row kernel's refusal as before:
    state, output planes, district sums, return and record stay what they were."""
    E, K = 64, 4
    spec, tab, layout, pol, pt, plain = _setup('t17', E, False)
    lean_pt = policy.PolicyTables(pt.pre, pt.dep, pt.out, pt.net_reset, pt.act_low, pt.act_high, None, None, pt.cols[:, 0], pt.low_bldg[:, 0],
                                  pt.high_bldg[:, 0], pt.sigma_bldg[:, 0], 0)
    cases = [('MARL', _setup('t17', E, False, 'MARL')[5], pt, {}, _lib.EngineError, 'CLR_MARL.*cannot couple the buildings inside a step'),
             ('kpi engine', StepEngine(tab, E, f64_maps=False, kpi=True), pt, {}, _lib.EngineError, 'CLD_KPI'),
             ('b_chunk=5', _setup('t17', E, False, b_chunk=5)[5], pt, {}, _lib.EngineError, 'b_chunk=5 leaves no room for the 4 chunk partial sums'),
             ('kpi=True', plain, pt, {'kpi': True}, NotImplementedError, 'KPI'),
             ('MLPPolicy tables', plain, lean_pt, {}, ValueError, 'StoragePolicyTables'),
             ('not chunked', plain, pt, {'chunked': False}, _lib.EngineError, 'n_bldg=17 > 16 would be a building-chunked launch')]
    for name, eng, tables, kw, exc, match in cases:
        ret = torch.full((E,), 3.0, device='cuda')
        traj = torch.full((K, policy.CLPF_NT if tables is pt else policy.CLPOL_NT, eng.n_bldg, E), -7.0, device='cuda')
        before = [x.clone() for x in (eng.state, eng.out_bldg, eng._out_env, ret, traj)]
        t_before = eng.t
        with pytest.raises(exc, match=match):
            eng.rollout_policy(K, tables, ret_env=ret, traj=traj, **{'chunked': True, **kw})
        torch.cuda.synchronize()
        assert eng.t == t_before, name
        for x, was in zip((eng.state, eng.out_bldg, eng._out_env, ret, traj), before):
            assert torch.equal(x, was), name
    # ... and after all that the engine still runs
    _roll(plain, pt, K)
    assert plain.last_kernels == _names(False), plain.last_kernels
