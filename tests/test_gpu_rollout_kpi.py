"""The fused K-step rollout that keeps the streaming KPI accumulators (`StepEngine.rollout(fused=True)` on a `kpi=True` engine:
`cl_rollout_seq_f32` under `CLD_ROLLOUT_FUSED`, kernel `cl_rollout_kpi_kernel`) against the SINGLE-STEP path (`StepEngine.step` with
`kpi=True`: `cl_step_lean_kpi_kernel` / `cl_step_lean_kpi_chain_kernel`), which test_env_gpu.py::test_streaming_kpi_accumulators and
test_gpu_parity.py pin to the KPI library and the reference-run fixtures.  The fused rollout follows single steps to 2e-6 .. 2e-5, not bit
for bit (test_gpu_rollout.py), so the accumulators are compared at the tolerances the project uses for two paths on the same trajectory
(test_f64_chain_with_streaming_kpis, test_rollout_with_streaming_kpis_and_large_districts): rtol 1e-4 with atol 1e-3 on `kpi_bldg` and
atol 1e-2 on `kpi_env`; finalised KPIs at rtol 1e-4 / atol 1e-5 per building and rtol 1e-3 / atol 1e-4 for the district series.  Group
counters and the -inf of an open maximum group must match exactly."""
import numpy as np
import pytest
import torch

from golden_util import golden
from citylearn_amd import _lib, abi
from citylearn_amd.engine import StepEngine

pytestmark = pytest.mark.gpu

REWARD_CLASS = 'citylearn.reward_function.RewardFunction'


def _actions(spec, K, E, seed):
    low, high = spec.action_limits()
    gen = torch.Generator(device='cuda').manual_seed(seed)
    lo, hi = torch.from_numpy(low).cuda(), torch.from_numpy(high).cuda()
    return lo[None, :, None] + torch.rand((K, len(low), E), device='cuda', generator=gen) * (hi - lo)[None, :, None]


def _fused(eng, K, **kw):
    """One fused launch that ran cl_rollout_kpi_kernel and no step kernel."""
    eng.rollout(K, fused=True, **kw)
    assert 'cl_rollout_kpi_kernel<' in eng.last_kernels and 'cl_step' not in eng.last_kernels and '+' not in eng.last_kernels, eng.last_kernels


def _compare_kpi_planes(b, a, what=''):
    """`b` (fused) against `a` (single steps): every plane of kpi_bldg / kpi_env."""
    torch.testing.assert_close(b.kpi_bldg, a.kpi_bldg, rtol=1e-4, atol=1e-3, msg=lambda m: f'kpi_bldg {what}: {m}')
    ke_b, ke_a = b.kpi_env.clone(), a.kpi_env.clone()
    inf_b, inf_a = torch.isinf(ke_b), torch.isinf(ke_a)
    assert torch.equal(inf_b, inf_a) and torch.equal(ke_b[inf_b], ke_a[inf_a]), f'open maximum groups {what}'
    ke_b[inf_b] = 0.0; ke_a[inf_a] = 0.0
    torch.testing.assert_close(ke_b, ke_a, rtol=1e-4, atol=1e-2, msg=lambda m: f'kpi_env {what}: {m}')
    for cond in (0, abi.CLKE_PER_COND):
        for row in (abi.CLKE_DAY_N, abi.CLKE_MON_N):
            assert torch.equal(b.kpi_env[cond + row], a.kpi_env[cond + row]), f'group counter {cond + row} {what}'
    # what the step kernel leaves alone stays at its reset value here too
    for row in (abi.CLK_UNSERVED_OUTAGE, abi.CLK_EXPECTED_OUTAGE, abi.CLK_UNSERVED_ALL):
        assert torch.equal(b.kpi_bldg[row], a.kpi_bldg[row])


def _compare_step_outputs(b, a, ret=None, ret_ref=None, chain=False):
    torch.testing.assert_close(b.state, a.state, rtol=2e-6, atol=2e-6)
    torch.testing.assert_close(b.out_bldg[:2], a.out_bldg[:2], rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(b.out_env, a.out_env, rtol=1e-4, atol=1e-4)
    if ret is not None:
        torch.testing.assert_close(ret, ret_ref, rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('E', [64, 192, 260, 4096])
@pytest.mark.parametrize('kind', ['RewardFunction', 'MARL', 'IndependentSACReward', 'SolarPenaltyReward'])
def test_fused_kpi_rollout_equals_single_steps(kind, E, f64):
    """K = 30 open-loop steps from t0 = 0 (a day boundary inside the launch, the t = 0 quirk of the baseline): state, last outputs, district
    sums, return and every KPI plane; full and ragged (260) env tiles, one and several env blocks."""
    spec = golden('g2022_all').spec()
    tab = spec.episode_tables(0)
    K = 30
    acts = _actions(spec, K, E, 9)
    a, b = StepEngine(tab, E, reward=kind, kpi=True, f64_maps=f64), StepEngine(tab, E, reward=kind, kpi=True, f64_maps=f64)
    assert a.kpi_shared_baseline and b.f64_chain == (f64 == 'chain')
    b.trace_kernels()
    ret, ret_ref = torch.zeros(E, device='cuda'), torch.zeros(E, device='cuda')
    for k in range(K):
        a.step(acts[k])
        ret_ref += a.district_reward
    _fused(b, K, actions=acts, ret_env=ret)
    assert b.last_kernels.endswith(', 2>' if f64 == 'chain' else ', 0>'), b.last_kernels
    assert b.t == a.t == K
    _compare_step_outputs(b, a, ret, ret_ref)
    _compare_kpi_planes(b, a)
    assert float(b.kpi_bldg.abs().sum()) > 0 and float(b.kpi_env[abi.CLKE_DAY_N].min()) == 1.0


@pytest.mark.parametrize('vec', [1, 2])
@pytest.mark.parametrize('f64', ['chain', False])
def test_group_boundaries_across_consecutive_launches(f64, vec):
    """Launches of 1, 5, 24, 25 and 53 steps one after the other from t0 = 0: they start in the middle of a day, end on a day boundary, span two
    days and more folds of the district series than one; compared with single steps after EVERY launch.  Both pack widths (forced)."""
    spec = golden('g2022_all').spec()
    tab = spec.episode_tables(0)
    E = 320
    tun = dict(vec=vec)
    a, b = StepEngine(tab, E, kpi=True, f64_maps=f64), StepEngine(tab, E, kpi=True, f64_maps=f64, tuning=tun)
    b.trace_kernels()
    for n, K in enumerate((1, 5, 24, 25, 53)):
        acts = _actions(spec, K, E, 100 + n)
        for k in range(K):
            a.step(acts[k])
        _fused(b, K, actions=acts)
        assert f'cl_rollout_kpi_kernel<{vec}, ' in b.last_kernels
        assert a.t == b.t
        _compare_step_outputs(b, a)
        _compare_kpi_planes(b, a, f'after launch {n} (t = {b.t})')
    assert float(b.kpi_env[abi.CLKE_DAY_N].max()) == 4.0 == float(b.kpi_env[abi.CLKE_PER_COND + abi.CLKE_DAY_N, 0])


def test_month_boundary_inside_a_launch():
    """t0 = 700, K = 48 crosses t = 720 (a day) and t = 730 (the month group) in one launch; the 700 steps before it run as fused launches of 100."""
    g = golden('g2022_p1_year')
    spec = g.spec()
    tab = spec.episode_tables(0)
    E = 8
    a, b = StepEngine(tab, E, kpi=True), StepEngine(tab, E, kpi=True)
    b.trace_kernels()
    for n in range(7):
        acts = _actions(spec, 100, E, n)
        for k in range(100):
            a.step(acts[k])
        _fused(b, 100, actions=acts)
    _compare_kpi_planes(b, a, 'at t = 700')
    assert float(b.kpi_env[abi.CLKE_MON_N].max()) == 0.0
    acts = _actions(spec, 48, E, 77)
    for k in range(48):
        a.step(acts[k])
    _fused(b, 48, actions=acts)
    assert b.t == 748
    _compare_step_outputs(b, a)
    _compare_kpi_planes(b, a, 'at t = 748')
    assert float(b.kpi_env[abi.CLKE_MON_N].min()) == 1.0 and float(b.kpi_env[abi.CLKE_PER_COND + abi.CLKE_MON_N, 0]) == 1.0


@pytest.mark.parametrize('kind,f64', [('RewardFunction', 'chain'), ('MARL', False)])
def test_on_device_policy(kind, f64):
    """The Philox policy inside the fused KPI launch against single steps fed with the host's replay of the stream
    (test_rollout_with_streaming_kpis_and_large_districts' construction: one-ulp action differences are possible)."""
    spec = golden('g2022_all').spec()
    tab = spec.episode_tables(0)
    E, K, seed = 192, 30, 9
    low, high = spec.action_limits()
    cols = len(low)
    lib = _lib.load()
    u = np.array([[[lib.cl_philox_uniform(seed, e, col, t) for e in range(E)] for col in range(cols)] for t in range(K)], dtype=np.float64)
    host = torch.from_numpy((low.astype(np.float64)[None, :, None] + u * (high - low).astype(np.float64)[None, :, None]).astype(np.float32)).cuda()
    c, d = StepEngine(tab, E, reward=kind, kpi=True, f64_maps=f64), StepEngine(tab, E, reward=kind, kpi=True, f64_maps=f64)
    d.trace_kernels()
    d.set_action_limits(low, high)
    _fused(d, K, seed=seed)
    for k in range(K):
        c.step(host[k])
    torch.testing.assert_close(d.state, c.state, rtol=2e-5, atol=2e-5)
    _compare_kpi_planes(d, c)


@pytest.mark.parametrize('env_offset', [0, 4096])
def test_episode_offsets_per_env_block(env_offset):
    """`env_row0` (three env blocks, 640 envs = 2.5 blocks: a ragged last block) and `env_offset`: every block's baseline sums and baseline series
    land at the block's first env and nowhere else; on-device policy (the env offset keys it) against the launch sequence's policy kernel."""
    spec = golden('g2022_all').spec()
    tab = spec.episode_tables(0)
    E, K, n_steps = 640, 30, 200
    row0 = [0, 300, 77]
    kw = dict(kpi=True, n_steps=n_steps, env_row0=row0, env_offset=env_offset)
    a, b = StepEngine(tab, E, **kw), StepEngine(tab, E, **kw)
    b.trace_kernels()
    low, high = spec.action_limits()
    for e in (a, b):
        e.set_action_limits(low, high)
    a.rollout(K, seed=5)                                  # default for kpi=True: the launch sequence = single steps bit for bit
    _fused(b, K, seed=5)
    torch.testing.assert_close(b.state, a.state, rtol=2e-5, atol=2e-5)
    _compare_kpi_planes(b, a)
    first = torch.zeros(E, dtype=torch.bool, device='cuda')
    first[::abi.CL_ROW0_BLOCK] = True
    base = b.kpi_bldg[abi.CLK_B_NET]
    assert bool((base[:, first] != 0).all()) and bool((base[:, ~first] == 0).all())
    assert bool((b.kpi_env[abi.CLKE_PER_COND + abi.CLKE_PREV][first] != 0).all()) and bool((b.kpi_env[abi.CLKE_PER_COND + abi.CLKE_PREV][~first] == 0).all())
    # the three blocks replay different windows: different baselines
    assert len({float(base[0, i]) for i in (0, 256, 512)}) == 3


def _finalised_close(got, ref):
    (gb, gd), (rb, rd) = got, ref
    assert set(gb) == set(rb) and set(gd) == set(rd)
    for name in rb:
        torch.testing.assert_close(gb[name], rb[name], rtol=1e-4, atol=1e-5, equal_nan=True, msg=lambda m: f'{name}: {m}')
    for name in rd:
        torch.testing.assert_close(gd[name], rd[name], rtol=1e-3, atol=1e-4, equal_nan=True, msg=lambda m: f'district {name}: {m}')


def test_vector_env_rollout_evaluate_and_checkpoint():
    """`VectorCityLearnEnv(kpi=True)`: `rollout(K, actions, fused=True)` + `evaluate()` against an env stepped through the same actions; a mix of
    `step()`, `rollout(fused=True)` and `rollout()` in one episode; a `state_dict()` taken between two fused launches continues to the same KPIs in
    a fresh env."""
    from citylearn_amd.vector_env import VectorCityLearnEnv
    g = golden('g2022_all')
    E = 64
    mk = lambda: VectorCityLearnEnv(g.schema_path, E, kpi=True, reward_function=REWARD_CLASS)
    a, b = mk(), mk()
    b.engine.trace_kernels()
    spec = a.district_spec
    acts = _actions(spec, 60, E, 3)
    ret_ref = torch.zeros(E, device='cuda')
    for k in range(30):
        ret_ref += a.step(acts[k])[1].sum(dim=0)
    ret = b.rollout(30, acts[:30], fused=True)
    assert 'cl_rollout_kpi_kernel' in b.engine.last_kernels and b.time_step == a.time_step == 30
    torch.testing.assert_close(ret, ret_ref, rtol=1e-4, atol=1e-2)
    _finalised_close(b.evaluate(), a.evaluate())
    # mixed: a single step, a fused launch, the default (launch sequence) -- and a checkpoint in between
    for k in range(30, 60):
        a.step(acts[k])
    b.step(acts[30])
    b.rollout(12, acts[31:43], fused=True)
    sd = b.state_dict()
    b.rollout(9, acts[43:52])
    assert 'cl_step_lean_kpi' in b.engine.last_kernels
    b.rollout(8, acts[52:60], fused=True)
    assert b.time_step == 60
    _compare_kpi_planes(b.engine, a.engine, 'mixed episode')
    _finalised_close(b.evaluate(), a.evaluate())
    c = mk()
    c.load_state_dict(sd)
    assert c.time_step == 43 and torch.equal(c.engine.kpi_env, sd['engine']['kpi_env'])
    c.rollout(17, acts[43:60], fused=True)
    _compare_kpi_planes(c.engine, a.engine, 'restored episode')
    _finalised_close(c.evaluate(), a.evaluate())


def _year_kpis(fused):
    """Finalised streaming KPIs of the fixture's own actions over the whole year, env 0, as {'level|name|cost_function': value}."""
    from citylearn_amd.vector_env import VectorCityLearnEnv
    g = golden('g2022_p1_year')
    E, K = 4, g.facts['steps']
    env = VectorCityLearnEnv(g.schema_path, E, kpi=True, reward_function=REWARD_CLASS)
    env.engine.trace_kernels()
    acts = torch.from_numpy(g.ref['actions'][:K]).cuda()[:, :, None].expand(-1, -1, E).contiguous()
    t = 0
    while t < K:
        n = min(24, K - t)
        if fused:
            env.rollout(n, acts[t:t + n], fused=True)
            assert 'cl_rollout_kpi_kernel' in env.engine.last_kernels
        else:
            for k in range(t, t + n):
                env.step(acts[k])
        t += n
    building, district = env.evaluate()
    names = [b.name for b in env.district_spec.buildings]
    ref = dict(zip([str(x) for x in g.ref['kpi_names']], [float(x) for x in g.ref['kpi_values']]))
    got = {}
    for key in ref:                                      # 'level|name|cost_function', as test_full_year_free_running_kpis spells them
        level, bname, fn = key.split('|')
        if level == 'district' and fn in district:
            got[key] = float(district[fn][0])
        elif level != 'district' and fn in building and bname in names:
            got[key] = float(building[fn][names.index(bname), 0])
    return got, ref


# KPI names of the year fixture that the SINGLE-STEP streaming path reproduces at rtol 1e-4 / atol 1e-6 (established with `_year_kpis(False)`
# alone, before the fused path was compared: all 35 that are not discomfort names): the floor below keeps the year test from passing by skipping names.
YEAR_NAMES_FLOOR = 35


def test_full_year_of_fused_launches_against_the_reference_run():
    """g2022_p1_year (BASELINE config 1), the fixture's actions as an open-loop tensor, fused launches of K = 24 to the end of the 8 759-step
    episode (the last one shorter): the finalised KPIs against the reference run's, at test_full_year_free_running_kpis' rtol 1e-4 / atol 1e-6,
    for every name the streaming accumulators produce (the discomfort names are constants of the data files, skipped as there)."""
    got, ref = _year_kpis(fused=True)
    n = 0
    for k, v in ref.items():
        if k.split('|')[-1].startswith(('discomfort', 'one_minus_thermal')) or np.isnan(v):
            continue
        assert k in got, k
        print(f'{k}: fused {got[k]:.9g} reference {v:.9g} rel {abs(got[k] - v) / max(abs(v), 1e-30):.3g}')
        np.testing.assert_allclose(got[k], v, rtol=1e-4, atol=1e-6, err_msg=k)
        n += 1
    assert n >= YEAR_NAMES_FLOOR, n


@pytest.mark.parametrize('case', ['thermal', 'tiled48', 'evs', 'f64_maps'])
def test_refusals_leave_everything_untouched(case):
    """`fused=True` with `kpi=True` on a district the fused KPI kernel does not cover raises the library's CL_EINVAL -- it does not degrade to
    the launch sequence -- and neither the state nor a KPI plane moves."""
    from citylearn_amd.synthetic import tile_district
    kw = {}
    if case == 'thermal':
        spec = golden('g2020_cz1').spec()
    elif case == 'tiled48':
        spec = tile_district(golden('g2022_all').spec(), 48)
    elif case == 'evs':
        spec = golden('g2022_evs').spec()
    else:
        spec, kw = golden('g2022_all').spec(), dict(f64_maps=True)
    tab = spec.episode_tables(0)
    E, K = 64, 6
    eng = StepEngine(tab, E, kpi=True, **kw)
    acts = _actions(spec, K, E, 1)[:, :eng.n_act_cols].contiguous() if case != 'evs' else \
        torch.zeros((K, eng.n_act_cols, E), device='cuda')
    eng.step(acts[0])
    eng.trace_kernels()
    before = [x.clone() for x in (eng.state, eng.kpi_bldg, eng.kpi_env, eng.out_bldg)]
    with pytest.raises(_lib.EngineError) as e:
        eng.rollout(K - 1, actions=acts[1:], fused=True)
    assert e.value.code == abi.CL_EINVAL and 'CLD_ROLLOUT_FUSED' in str(e.value)
    assert eng.t == 1
    for x, y in zip(before, (eng.state, eng.kpi_bldg, eng.kpi_env, eng.out_bldg)):
        assert torch.equal(x, y)
    eng.rollout(K - 1, actions=acts[1:])                  # the default still runs them as the launch sequence
    assert eng.t == K and 'cl_rollout_kpi_kernel' not in eng.last_kernels


def test_default_choice_is_unchanged():
    """`rollout()` on a `kpi=True` engine without `fused` keeps the launch sequence (bit-identical to single steps, which existing tests require)."""
    spec = golden('g2022_all').spec()
    tab = spec.episode_tables(0)
    eng = StepEngine(tab, 64, kpi=True)
    eng.trace_kernels()
    eng.rollout(6, actions=_actions(spec, 6, 64, 2))
    assert 'cl_step_lean_kpi' in eng.last_kernels and 'cl_rollout_kpi_kernel' not in eng.last_kernels, eng.last_kernels
    eng.rollout(6, actions=_actions(spec, 6, 64, 3), fused=False)
    assert 'cl_step_lean_kpi' in eng.last_kernels, eng.last_kernels
