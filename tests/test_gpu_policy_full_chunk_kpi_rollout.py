"""The building-chunked closed-loop policy rollout of thermal districts that keeps the streaming KPIs (`StepEngine.rollout_policy(chunked=True,
kpi=True)` / `VectorCityLearnEnv(kpi=True).rollout_policy(kpi=True)` with a `StorageMLPPolicy` on a district of more than 16 buildings: per call
`cl_rollout_full_policy_chunk_kpi_kernel`, `cl_kpi_series_chunk_kernel` and `cl_finish_kernel`, csrc/cl_policy_full.h at KPI = CHUNK = true and csrc/cl_policy_full_chunk_kpi.h,
``libcitylearn_amd_policy_full_chunk_kpi.so``).

The references: (1) the one-row KPI kernel on the sixteen-building district; (2, 3, 6, 8) the SINGLE-STEP path with `kpi=True` fed the recorded
actions, and at 1024 buildings a float64 restatement of the district series; (4, 5, 7) two ways of running the kernel that must agree bit for bit --
windows, split launches with a checkpoint, env blocks; (9) refusals.  Helpers and tolerances: tests/test_gpu_policy_full_kpi_rollout.py
(`_compare_kpi`, `_replay`, `_outage_sums_moved`), tests/test_gpu_rollout_kpi.py (`_finalised_close`); districts: tests/policy_full_chunk_util.py;
weights: tests/policy_full_util.py.  H = 16 throughout (the `CONDITIONED` table).  Reference engines are built without `tuning`; only the engine
under test takes `b_chunk`.  Measured readings: profiles/policy_full_chunk_kpi_parity.md."""
import numpy as np
import pytest
import torch

from golden_util import golden, record_worst
from citylearn_amd import _lib, abi, policy
from citylearn_amd.engine import StepEngine
from citylearn_amd.observations import ObservationLayout
from policy_full_chunk_util import chunk_district, default_chunks
from policy_full_util import make_storage_policy, outage_mask
from test_gpu_policy_full_kpi_rollout import OUTAGE, _compare_kpi, _outage_sums_moved, _replay
from test_gpu_policy_full_rollout import A, N, NA, R, S, _scatter
from test_gpu_rollout_geometry import _prec
from test_gpu_rollout_kpi import REWARD_CLASS, _finalised_close

pytestmark = pytest.mark.gpu

KINDS = ['RewardFunction', 'IndependentSACReward', 'SolarPenaltyReward']          # (MARL couples the buildings inside a step: refused, test 9)
H = 16
DAY_N = [abi.CLKE_DAY_N, abi.CLKE_PER_COND + abi.CLKE_DAY_N]
MON_N = [abi.CLKE_MON_N, abi.CLKE_PER_COND + abi.CLKE_MON_N]


def _names(f64):
    """`last_kernels` of a call: the three launches, nothing else."""
    return f'cl_rollout_full_policy_chunk_kpi_kernel<{_prec(f64)}>+cl_kpi_series_chunk_kernel+cl_finish_kernel'


def _setup(district, E, f64='chain', kind='RewardFunction', sigma=None, b_chunk=0, n_sets=1, set_of_block=None, **kw):
    spec = chunk_district(district)
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    pol = make_storage_policy(layout, H, n_sets=n_sets, seed=H, sigma=sigma)
    pt = pol.pack(layout, tab, device='cuda:0', set_of_block=set_of_block)
    eng = StepEngine(tab, E, reward=kind, kpi=True, f64_maps=f64, tuning={'b_chunk': b_chunk} if b_chunk else None, **kw)
    assert not eng.lean and eng.kpi and eng.f64_chain == (f64 == 'chain') and not eng.kpi_shared_baseline
    eng.trace_kernels()
    return spec, tab, layout, pol, pt, eng


def _roll(eng, pt, K, seed=0, record=True, chunked=True):
    ret = torch.zeros(eng.n_env, device='cuda')
    traj = torch.full((K, policy.CLPF_NT, eng.n_bldg, eng.n_env), float('nan'), device='cuda') if record else None
    eng.rollout_policy(K, pt, seed=seed, ret_env=ret, traj=traj, kpi=True, **({'chunked': True} if chunked else {}))
    assert traj is None or not torch.isnan(traj).any()
    return ret, traj


def _planes(eng):
    """Every plane a caller reads (of out_bldg all but the reserved one: its scratch rows hold the LAST call's chunk sums and shares of the return)."""
    return [x.clone() for x in (eng.state, eng.out_bldg[:abi.CLO_RESERVED], eng.out_env, eng.kpi_bldg, eng.kpi_env)]


# ---- 1. against the one-row KPI kernel --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('b_chunk', [8, 6])
def test_1_sixteen_buildings_equal_the_one_row_kpi_kernel(b_chunk, f64):
    """(1) 't16' cut 8 + 8 and 6 + 6 + 4 (a last chunk with two waves without a building) against `cl_rollout_full_policy_kpi_kernel` on the same
    district: same seed, sigma = 0.1, K = 30 (across the day group at 24, a partial ring fold behind it), E = 260 (ragged tile).  Record, state
    and out_bldg[:2] at tests/test_gpu_policy_full_chunk_rollout.py test 1's tolerances, the KPI planes by `_compare_kpi` (outage planes and
    group counters bit-equal).  Whether kpi_bldg is bit-equal -- each wave runs the one-row kernel's arithmetic on its building -- is recorded."""
    E, K = 260, 30
    spec, tab, layout, pol, pt, one = _setup('t16', E, f64, sigma=0.1)
    ret1, traj1 = _roll(one, pt, K, seed=5, chunked=False)
    assert one.last_kernels == f'cl_rollout_full_policy_kpi_kernel<{_prec(f64)}, false>', one.last_kernels
    eng = _setup('t16', E, f64, sigma=0.1, b_chunk=b_chunk)[5]
    ret, traj = _roll(eng, pt, K, seed=5)
    assert eng.last_kernels == _names(f64), eng.last_kernels
    torch.testing.assert_close(traj[:, A:A + NA], traj1[:, A:A + NA], rtol=2e-6, atol=2e-6)
    torch.testing.assert_close(traj[:, S:S + 4], traj1[:, S:S + 4], rtol=2e-6, atol=2e-6)
    torch.testing.assert_close(traj[:, N], traj1[:, N], rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(traj[:, R], traj1[:, R], rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(eng.state[:6], one.state[:6], rtol=2e-6, atol=2e-6)
    torch.testing.assert_close(eng.out_bldg[:2], one.out_bldg[:2], rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(eng.out_env, one.out_env, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(ret, ret1, rtol=1e-5, atol=1e-3)
    _compare_kpi(eng, one, f't16 b_chunk={b_chunk} f64={f64}')
    assert float(eng.kpi_env[DAY_N].min()) == 1.0 == float(eng.kpi_env[DAY_N].max())
    bit = torch.equal(eng.kpi_bldg, one.kpi_bldg)
    print(f't16 b_chunk={b_chunk} f64={f64}: kpi_bldg bit-equal {bit}, record bit-equal {torch.equal(traj, traj1)}')
    record_worst({'kpi_bldg_bit_equal': float(bit), 'record_bit_equal': float(torch.equal(traj, traj1))},
                 f'chunked thermal policy kpi rollout vs one-row kpi kernel t16 b_chunk={b_chunk} f64_maps={f64}')


# ---- 2. against single steps ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('E', [64, 260])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('district,b_chunk', [('t17', 0), ('t17', 8), ('t17', 16), ('t24', 0), ('t33', 0), ('t17_outage', 0)])
def test_2_kpis_equal_single_steps(district, b_chunk, kind, E, f64):
    """(2) K = 30, noise on, the recorded head planes fed step by step to a second `kpi=True` engine (`_replay`: the record, state, outputs, KPI
    planes and, under the chain, the CLD_DETAIL_MIN planes): 17 buildings cut 6 + 6 + 5 (a wave without a building), 8 + 8 + 1 and 16 + 1 (rows
    of ONE building beside seven / fifteen waves that only run the barrier schedule and park zeros), 24, 33, and the outage district."""
    K = 30
    spec, tab, layout, pol, pt, eng = _setup(district, E, f64, kind, sigma=0.1, b_chunk=b_chunk)
    if not b_chunk:
        assert default_chunks(eng.n_bldg)[0] == {17: 6, 24: 8, 33: 7}[eng.n_bldg]
    ret, traj = _roll(eng, pt, K, seed=5)
    assert eng.last_kernels == _names(f64), eng.last_kernels
    ref = StepEngine(tab, E, reward=kind, kpi=True, f64_maps=f64)
    _replay(ref, pt, traj, eng, ret, f'chunked thermal policy kpi rollout vs single steps {district} b_chunk={b_chunk} {kind} E={E} f64_maps={f64}', tab=tab)
    assert bool(tab.outage[:K].any()) == district.endswith('_outage')
    assert eng.t == K and float(eng.kpi_env[DAY_N].min()) == 1.0 == float(eng.kpi_env[DAY_N].max())
    assert bool((eng.kpi_bldg[abi.CLK_B_NET] != 0).all())


def test_2_without_a_return_buffer():
    """(2) `ret_env=None`: the fold behind the two kernels launches NQ workgroup rows instead of NQ + 1.  The smallest shape that chunks -- 17
    buildings cut 6 + 6 + 5 (the default), 64 envs, K = 4: every plane a caller reads bit for bit what a twin engine that keeps the return leaves,
    and against single steps at `_replay`'s tolerances (the return it checks is the twin's)."""
    E, K = 64, 4
    spec, tab, layout, pol, pt, eng = _setup('t17', E, sigma=0.1)
    twin = _setup('t17', E, sigma=0.1)[5]
    ret, traj_twin = _roll(twin, pt, K, seed=5)
    traj = torch.full_like(traj_twin, float('nan'))
    eng.rollout_policy(K, pt, seed=5, traj=traj, kpi=True, chunked=True)
    assert eng.last_kernels == twin.last_kernels == _names('chain'), eng.last_kernels
    assert torch.equal(traj, traj_twin)
    for got, want in zip(_planes(eng), _planes(twin)):
        assert torch.equal(got, want)
    ref = StepEngine(tab, E, kpi=True, f64_maps='chain')
    _replay(ref, pt, traj, eng, ret, 'chunked thermal policy kpi rollout vs single steps t17 E=64 f64_maps=chain ret_env=None', tab=tab)


# ---- 3. config 4's district -------------------------------------------------------------------------------------------------------------
def _series_f64(init, samples, t0=0):
    """`kpi_series_advance` (csrc/cl_rollout.h) restated in float64: `init` [12, E] the accumulators, `samples` [K, E] the district samples."""
    k = {name: init[getattr(abi, 'CLKE_' + name)].astype(np.float64).copy() for name in
         ('PREV', 'RAMP', 'DAY_SUM', 'DAY_MAX', 'DAY_LF_SUM', 'DAY_PEAK_SUM', 'DAY_N', 'MON_SUM', 'MON_MAX', 'MON_LF_SUM', 'MON_N', 'ALL_MAX')}
    for j, v in enumerate(samples):
        t = t0 + j
        if t > 0:
            k['RAMP'] += np.maximum(v - k['PREV'], 0.0)
        k['PREV'] = v.copy()
        if t > 0 and t % 24 == 0:
            k['DAY_LF_SUM'] += 1.0 - (k['DAY_SUM'] / 24.0) / k['DAY_MAX']
            k['DAY_PEAK_SUM'] += k['DAY_MAX']
            k['DAY_N'] += 1.0
            k['DAY_SUM'], k['DAY_MAX'] = np.zeros_like(v), np.full_like(v, -np.inf)
        k['DAY_SUM'] = k['DAY_SUM'] + v
        k['DAY_MAX'] = np.maximum(k['DAY_MAX'], v)
        if t > 0 and t % 730 == 0:
            k['MON_LF_SUM'] += 1.0 - (k['MON_SUM'] / 730.0) / k['MON_MAX']
            k['MON_N'] += 1.0
            k['MON_SUM'], k['MON_MAX'] = np.zeros_like(v), np.full_like(v, -np.inf)
        k['MON_SUM'] = k['MON_SUM'] + v
        k['MON_MAX'] = np.maximum(k['MON_MAX'], v)
        k['ALL_MAX'] = np.maximum(k['ALL_MAX'], v)
    out = np.zeros((abi.CLKE_PER_COND, init.shape[1]))
    for name, v in k.items():
        out[getattr(abi, 'CLKE_' + name)] = v
    return out


def _series_deviation(kpi_env, want):
    """Worst |kpi_env - want| of both series in units of `_compare_kpi`'s kpi_env tolerance (1e-2 + 1e-4 |want|); open maximum groups coincide."""
    got = kpi_env[:2 * abi.CLKE_PER_COND].cpu().numpy().astype(np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got)) and np.array_equal(got[~fin], want[~fin])
    return float((np.abs(got[fin] - want[fin]) / (1e-2 + 1e-4 * np.abs(want[fin]))).max())


@pytest.mark.parametrize('f64', ['chain', False])
def test_3_config_4_district(f64):
    """(3) BASELINE config 4's 1024 buildings (128 chunks of eight) x 64 envs, K = 30, noise on, against single steps.  The record, the state
    and out_bldg[:2] at `_replay`'s tolerances, kpi_bldg at `_compare_kpi`'s.  The two district series are sums of 1024 buildings, outside what
    the project's kpi_env tolerance was set on, so they are MEASURED: both series in float64 on the host from the reference engine's per-step net
    and CLO_BASE_NET planes (`_series_f64`), and the launch's worst deviation from that gated at 4 x the single-step path's own deviation from it
    (the project's margin for another correct float32 evaluation, tests/test_gpu_policy_full_kpi_rollout.py::test_4_teacher_forced_actions), with
    `_compare_kpi`'s tolerance as the floor.  Readings (profiles/policy_full_chunk_kpi_parity.md), in units of 1e-2 + 1e-4 |ref|: chain launch
    0.0034, single steps 0.0073; fp32 launch 0.0039, single steps 0.0079."""
    E, K = 64, 30
    spec, tab, layout, pol, pt, eng = _setup('t1024', E, f64, sigma=0.1)
    assert default_chunks(eng.n_bldg) == (8, 128)
    ret, traj = _roll(eng, pt, K, seed=5)
    assert eng.last_kernels == _names(f64), eng.last_kernels
    ref = StepEngine(tab, E, kpi=True, f64_maps=f64)
    init = ref.kpi_env.cpu().numpy()
    ret_ref = torch.zeros(E, device='cuda')
    nets, bases = [], []
    for k in range(K):
        ref.step(_scatter(pt, traj[k, A:A + NA], ref.n_act_cols))
        ret_ref += ref.district_reward
        torch.testing.assert_close(traj[k, S:S + 4], ref.state[[0, 3, 4, 5]], rtol=2e-6, atol=2e-6)
        torch.testing.assert_close(traj[k, N], ref.net, rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(traj[k, R], ref.reward_bldg, rtol=2e-5, atol=2e-5)
        nets.append(ref.net.cpu().numpy().astype(np.float64).sum(axis=0))
        bases.append(ref.out_bldg[abi.CLO_BASE_NET].cpu().numpy().astype(np.float64).sum(axis=0))
    torch.testing.assert_close(eng.state[:6], ref.state[:6], rtol=2e-6, atol=2e-6)
    torch.testing.assert_close(eng.out_bldg[:2], ref.out_bldg[:2], rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(ret, ret_ref, rtol=1e-5, atol=1e-3)
    torch.testing.assert_close(eng.kpi_bldg, ref.kpi_bldg, rtol=1e-4, atol=1e-3)
    assert torch.equal(eng.kpi_bldg[OUTAGE], ref.kpi_bldg[OUTAGE])
    for row in DAY_N + MON_N:
        assert torch.equal(eng.kpi_env[row], ref.kpi_env[row]), row
    P = abi.CLKE_PER_COND
    want = np.concatenate([_series_f64(init[:P], np.array(nets)), _series_f64(init[P:2 * P], np.array(bases))])
    dev_launch, dev_steps = _series_deviation(eng.kpi_env, want), _series_deviation(ref.kpi_env, want)
    print(f't1024 f64={f64}: district series against float64, in units of 1e-2 + 1e-4 |ref|: launch {dev_launch:.4f}, single steps {dev_steps:.4f}')
    record_worst({'launch': dev_launch, 'single_steps': dev_steps}, f'chunked thermal policy kpi rollout district series vs float64 t1024 f64_maps={f64}')
    assert dev_launch <= max(4.0 * dev_steps, 1.0), (dev_launch, dev_steps)


# ---- 4. windows -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', ['chain', False])
def test_4_windows_do_not_show(f64):
    """(4) 't17', K = 30 as calls of 7 (five of them, the last of two steps), 8 (the ring's length) and 64 steps (one call): every plane, the
    record and the KPI planes bit-equal across the three; the return at rtol 1e-6 / atol 1e-4 (as many partial sums as calls)."""
    got = []
    for window in (7, 8, 64):
        spec, tab, layout, pol, pt, eng = _setup('t17', 260, f64, sigma=0.1)
        assert eng.policy_kpi_window == 64
        eng.policy_kpi_window = window
        ret, traj = _roll(eng, pt, 30, seed=5)
        assert eng.last_kernels == _names(f64) and eng.t == 30
        assert eng._series_scratch.numel() == min(window, 30) * 2 * 3 * 260
        got.append((_planes(eng), traj, ret))
    for planes, traj, ret in got[:2]:
        assert all(torch.equal(x, y) for x, y in zip(planes, got[2][0])) and torch.equal(traj, got[2][1])
        torch.testing.assert_close(ret, got[2][2], rtol=1e-6, atol=1e-4)
    assert float(got[2][0][4][DAY_N].min()) == 1.0


# ---- 5. split launches and checkpoint ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('district', ['t17', 't17_outage'])
def test_5_split_launches_and_checkpoint_are_bit_identical(district, f64):
    """(5) Launches of 1, 5, 24 and 25 steps, with a `state_dict` round trip into a fresh engine in between, equal one 55-step launch bit for bit
    in the record, state, out_bldg, out_env and both KPI planes (the district samples' association does not depend on how K is cut; the series
    close their groups on the absolute step index); the return at rtol 1e-6 / atol 1e-4.  On the outage district a launch that saw no outage row
    of a building leaves the sums an earlier launch moved alone (`_outage_sums_moved`)."""
    E = 320
    spec, tab, layout, pol, pt, one = _setup(district, E, f64, sigma=0.1)
    ret1, traj1 = _roll(one, pt, 55, seed=3)
    assert one.last_kernels == _names(f64), one.last_kernels
    mk = lambda: StepEngine(tab, E, kpi=True, f64_maps=f64)
    eng = mk()
    ret, parts = torch.zeros(E, device='cuda'), []
    reset_outage = eng.kpi_bldg[OUTAGE].clone()
    m = outage_mask(tab, 55)
    assert bool(m.any()) == district.endswith('_outage')
    for n, K in enumerate((1, 5, 24, 25)):
        if n == 2:
            sd = eng.state_dict()
            eng = mk()
            eng.load_state_dict(sd)
        traj = torch.empty((K, policy.CLPF_NT, eng.n_bldg, E), device='cuda')
        before = eng.kpi_bldg[OUTAGE].clone()
        eng.rollout_policy(K, pt, seed=3, ret_env=ret, traj=traj, kpi=True, chunked=True)
        parts.append(traj)
        if m.any():
            _outage_sums_moved(eng, before, m[eng.t - K:eng.t].any(axis=0))
        else:
            assert torch.equal(eng.kpi_bldg[OUTAGE], reset_outage)
    if m.any():
        _outage_sums_moved(one, reset_outage, m.any(axis=0))
    assert eng.t == 55 and torch.equal(torch.cat(parts), traj1)
    # (every plane of out_bldg but the reserved one: its scratch rows hold the LAST launch's shares of the return)
    assert torch.equal(eng.state, one.state) and torch.equal(eng.out_env, one.out_env)
    assert torch.equal(eng.out_bldg[:abi.CLO_RESERVED], one.out_bldg[:abi.CLO_RESERVED])
    assert torch.equal(eng.kpi_bldg, one.kpi_bldg) and torch.equal(eng.kpi_env, one.kpi_env)
    torch.testing.assert_close(ret, ret1, rtol=1e-6, atol=1e-4)


# ---- 6. month boundary ------------------------------------------------------------------------------------------------------------------
def test_6_month_boundary():
    """(6) 't17' has 744 rows: 720 steps (twelve windows), then 20 more -- t = 730 closes the month group inside the second launch, which is
    replayed through single steps from a `state_dict` copy of what the first one left."""
    E = 8
    spec, tab, layout, pol, pt, eng = _setup('t17', E, 'chain', sigma=0.1)
    ref = StepEngine(tab, E, kpi=True, f64_maps='chain')
    _roll(eng, pt, 720, seed=4, record=False)
    assert eng.t == 720 and float(eng.kpi_env[MON_N].max()) == 0.0 and float(eng.kpi_env[DAY_N].min()) == 29.0
    ref.load_state_dict(eng.state_dict())
    ret, traj = _roll(eng, pt, 20, seed=4)
    _replay(ref, pt, traj, eng, ret, 'chunked thermal policy kpi rollout vs single steps t17 month boundary')
    assert eng.t == 740 and float(eng.kpi_env[MON_N].min()) == 1.0 == float(eng.kpi_env[MON_N].max())


# ---- 7. env blocks ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', ['chain', False])
def test_7_windows_sets_and_env_offsets(f64):
    """(7) Two env blocks with different `env_row0` and different parameter sets in one 512-env launch of 't17': each block equals, bit for bit,
    a 256-env engine of its own with that window, that set and its env offset -- the KPI planes too."""
    spec = chunk_district('t17')
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    pol = make_storage_policy(layout, H, n_sets=2, seed=2, sigma=0.1)
    K, n_steps, rows = 30, 200, [0, 131]
    whole = StepEngine(tab, 512, kpi=True, f64_maps=f64, n_steps=n_steps, env_row0=rows)
    whole.trace_kernels()
    _, traj = _roll(whole, pol.pack(layout, tab, device='cuda:0', set_of_block=[0, 1]), K, seed=9)
    assert whole.last_kernels == _names(f64), whole.last_kernels
    assert not torch.equal(traj[:, A:A + NA, :, :256], traj[:, A:A + NA, :, 256:])
    for g in range(2):
        part = StepEngine(tab, 256, kpi=True, f64_maps=f64, n_steps=n_steps, env_row0=[rows[g]], env_offset=256 * g)
        _, tr = _roll(part, pol.pack(layout, tab, device='cuda:0', set_of_block=[g]), K, seed=9)
        sl = slice(256 * g, 256 * (g + 1))
        assert torch.equal(tr, traj[:, :, :, sl]), g
        assert torch.equal(part.state, whole.state[:, :, sl]) and torch.equal(part.out_env, whole.out_env[:, sl])
        assert torch.equal(part.out_bldg[:abi.CLO_RESERVED], whole.out_bldg[:abi.CLO_RESERVED, :, sl])
        assert torch.equal(part.kpi_bldg, whole.kpi_bldg[:, :, sl]) and torch.equal(part.kpi_env, whole.kpi_env[:, sl]), g
    base = whole.kpi_bldg[abi.CLK_B_NET]
    assert bool((base != 0).all()) and float(base[0, 0]) != float(base[0, 256])


# ---- 8. the env-level call --------------------------------------------------------------------------------------------------------------
def _check_8(f64, spec, name):
    from citylearn_amd.vector_env import VectorCityLearnEnv
    E, K = 64, 57
    mk = lambda: VectorCityLearnEnv(spec, E, kpi=True, reward_function=REWARD_CLASS, f64_maps=f64)
    a, b = mk(), mk()
    b.engine.trace_kernels()
    layout = ObservationLayout(b.spec, 'current', False)
    pol = make_storage_policy(layout, H, seed=8, sigma=0.05)
    ret, traj = b.rollout_policy(pol, K, seed=3, record=True, kpi=True)
    assert b.engine.last_kernels == _names(f64) and b.time_step == K and b.engine.n_bldg == 17
    pt = pol.pack(layout, b.tables)
    ret_ref = torch.zeros(E, device='cuda')
    for k in range(K):
        ret_ref += a.step(_scatter(pt, traj[k, A:A + NA], a.n_act_cols))[1].sum(dim=0)
    torch.testing.assert_close(ret, ret_ref, rtol=1e-5, atol=1e-3)
    _compare_kpi(b.engine, a.engine, f'finalised {name}')
    got, want = b.evaluate(), a.evaluate()
    _finalised_close(got, want)
    assert got[0] and got[1] and any(bool(torch.isfinite(v).all()) for v in got[1].values())
    return got


@pytest.mark.parametrize('f64', ['chain', False])
def test_8_env_level_call_and_evaluate(f64):
    """(8) `VectorCityLearnEnv(tile_district(g2020_cz1, 17), 64, kpi=True).rollout_policy(pol, 57, record=True, kpi=True)` routes to the chunked KPI
    call by itself; then `evaluate()`, against an env that steps the recorded actions: `_compare_kpi` and `_finalised_close`."""
    from citylearn_amd.synthetic import tile_district
    _check_8(f64, tile_district(golden('g2020_cz1').spec(), 17), 't17')


@pytest.mark.parametrize('f64', ['chain', False])
def test_8_env_level_call_under_an_outage(f64):
    """The same on 't17_outage': the two unserved-energy KPIs of the district come out finite and in (0, 1]."""
    got = _check_8(f64, chunk_district('t17_outage'), 't17_outage')
    for name in ('power_outage_normalized_unserved_energy_total', 'annual_normalized_unserved_energy_total'):
        v = got[1][name]
        assert bool(torch.isfinite(v).all()) and bool((v > 0).all()) and bool((v <= 1).all()), (name, v)


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------
def test_9_refusals_leave_every_plane_untouched():
    """(9) A MARL engine, an engine without KPIs (`NotImplementedError`), 17 buildings in chunks of five (no room in the reserved plane), two envs
    per lane, `f64_maps=True`: state, outputs, KPI planes, return, record and `t` stay what they were; afterwards the engine still runs."""
    E, K = 64, 4
    spec, tab, layout, pol, pt, good = _setup('t17', E, False)
    mk = lambda **kw: StepEngine(tab, E, kpi=True, **{'f64_maps': False, **kw})
    cases = [('MARL', mk(reward='MARL'), _lib.EngineError, 'CLR_MARL.*cannot couple the buildings inside a step'),
             ('no KPIs', StepEngine(tab, E, f64_maps=False), NotImplementedError, 'built without the streaming KPI accumulators'),
             ('b_chunk=5', mk(tuning={'b_chunk': 5}), _lib.EngineError, 'b_chunk=5 leaves no room for the 4 chunk partial sums'),
             ('vec=2', mk(tuning={'vec': 2}), _lib.EngineError, '2 envs per lane'),
             ('f64_maps', mk(f64_maps=True), _lib.EngineError, 'CLD_F64_MAPS')]
    for name, eng, exc, match in cases:
        eng.step(torch.zeros((eng.n_act_cols, E), device='cuda'))
        ret = torch.full((E,), 3.0, device='cuda')
        traj = torch.full((K, policy.CLPF_NT, eng.n_bldg, E), -7.0, device='cuda')
        live = [x for x in (eng.state, eng.out_bldg, eng._out_env, eng.kpi_bldg, eng.kpi_env, ret, traj) if x is not None]
        before = [x.clone() for x in live]
        with pytest.raises(exc, match=match):
            eng.rollout_policy(K, pt, ret_env=ret, traj=traj, kpi=True, chunked=True)
        torch.cuda.synchronize()
        assert eng.t == 1, name
        for x, was in zip(live, before):
            assert torch.equal(x, was), name
    # ... a step range that ends beyond the episode is refused as a whole, not at a later window
    good.policy_kpi_window = 2
    before = _planes(good)
    with pytest.raises(_lib.EngineError, match='outside'):
        good.rollout_policy(K, pt, kpi=True, chunked=True, t0=good.dims.n_steps - 3)
    torch.cuda.synchronize()
    assert good.t == 0 and all(torch.equal(x, y) for x, y in zip(before, _planes(good)))
    # ... and after all that the engine still runs
    _roll(good, pt, K)
    assert good.last_kernels == _names(False) and good.t == K
