"""The closed-loop policy rollout that keeps the streaming KPIs (`StepEngine.rollout_policy(kpi=True)` / `VectorCityLearnEnv.rollout_policy(kpi=True)`:
one launch of `cl_rollout_policy_kpi_kernel`, csrc/cl_policy.h at KPI = true, ``libcitylearn_amd_policy_kpi.so``).

Nothing here compares the kernel with itself, except where two launches of it must agree (split launches, env blocks).  The references are the
ones the two kernels it is made of are held to: the SINGLE-STEP path with `kpi=True` fed the recorded actions (tests/test_gpu_rollout_kpi.py's
`_compare_kpi_planes` / `_compare_step_outputs` / `_finalised_close`, imported), the float64 MLP on the recorded inputs and the CPU oracle's
closed loop (tests/test_gpu_policy_rollout.py's `_teacher_forced`, tests/policy_util.py), on g2022_all and the districts of
tests/district_util.py.  Shapes: E = 64 (one tile at one env per lane), E = 260 (a ragged tile, two env blocks), one case at E = 4096 with the
library's own geometry.  Measured readings of checks 2 - 4: profiles/policy_kpi_parity.md (scripts/policy_kpi_parity_table.py)."""
import numpy as np
import pytest
import torch

from district_util import HET_UNDRIVEN, district
from golden_util import check_worst, golden, record_worst
from citylearn_amd import _lib, abi, policy
from citylearn_amd.engine import StepEngine
from citylearn_amd.observations import ObservationLayout
from policy_util import host_closed_loop, make_policy
from test_gpu_policy_rollout import A, KINDS, N, R, S, _teacher_forced
from test_gpu_rollout_geometry import _bar, _prec, _step_actions
from test_gpu_rollout_kpi import REWARD_CLASS, _compare_kpi_planes, _compare_step_outputs, _finalised_close

pytestmark = pytest.mark.gpu


def _spec(name):
    return golden(name).spec() if name.startswith('g20') else district(name)


def _setup(name, E, f64, kind='RewardFunction', H=16, sigma=None, vec=None, n_sets=1, **kw):
    spec = _spec(name)
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    pol = make_policy(layout, H, n_sets=n_sets, seed=H, sigma=sigma)
    pt = pol.pack(layout, tab, device='cuda:0')
    eng = StepEngine(tab, E, reward=kind, kpi=True, f64_maps=f64, tuning=dict(vec=vec) if vec else None, **kw)
    assert eng.lean and eng.kpi and eng.f64_chain == (f64 == 'chain')
    eng.trace_kernels()
    return spec, tab, layout, pol, pt, eng


def _roll(eng, pt, K, seed=0, record=True):
    ret = torch.zeros(eng.n_env, device='cuda')
    traj = torch.full((K, policy.CLPOL_NT, eng.n_bldg, eng.n_env), float('nan'), device='cuda') if record else None
    eng.rollout_policy(K, pt, seed=seed, ret_env=ret, traj=traj, kpi=True)
    assert traj is None or not torch.isnan(traj).any()
    return ret, traj


def _replay(ref, pt, traj, eng=None, ret=None, label=None):
    """Feed the recorded actions step by step to `ref.step()` (a `kpi=True` engine in the state the launch started from): per-step soc / net /
    reward planes at test_gpu_policy_rollout.py::test_b's tolerances; with `eng`, check 2's comparisons of what the launch left."""
    worst = {}
    ret_ref = torch.zeros(ref.n_env, device='cuda')
    for k in range(traj.shape[0]):
        ref.step(_step_actions(ref, pt, traj[k, A]))
        ret_ref += ref.district_reward
        for key, got, want in (('soc', traj[k, S], ref.soc), ('net', traj[k, N], ref.net), ('reward', traj[k, R], ref.reward_bldg)):
            worst[key] = max(worst.get(key, 0.0), _bar(got, want))
        torch.testing.assert_close(traj[k, S], ref.soc, rtol=2e-6, atol=2e-6)
        torch.testing.assert_close(traj[k, N], ref.net, rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(traj[k, R], ref.reward_bldg, rtol=2e-5, atol=2e-5)
    if eng is not None:
        worst.update(state=_bar(eng.state, ref.state), out_env=_bar(eng.out_env, ref.out_env), kpi_bldg=_bar(eng.kpi_bldg, ref.kpi_bldg),
                     kpi_env=_bar(eng.kpi_env, ref.kpi_env))
        if ret is not None:
            worst['return'] = _bar(ret, ret_ref)
        print(label, {k: round(v, 4) for k, v in worst.items()})
        record_worst(worst, label)
        assert eng.t == ref.t
        _compare_step_outputs(eng, ref, ret, ret_ref if ret is not None else None)
        _compare_kpi_planes(eng, ref, label)
    return ret_ref


# ---- 1. one launch --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('vec', [1, 2])
@pytest.mark.parametrize('f64', ['chain', False])
def test_1_one_launch(f64, vec):
    spec, tab, layout, pol, pt, eng = _setup('g2022_all', 260, f64, vec=vec)
    _roll(eng, pt, 9, record=False)
    assert eng.last_kernels == f'cl_rollout_policy_kpi_kernel<{vec}, {_prec(f64)}>', eng.last_kernels
    assert eng.t == 9 and float(eng.kpi_bldg.abs().sum()) > 0


# ---- 2. KPIs against the single-step path -----------------------------------------------------------------------------------------------
def _check_2(name, kind, E, f64, vec):
    K = 30                                                           # crosses a day group (t = 24) and leaves a partial fold (30 = 3 x 8 + 6)
    spec, tab, layout, pol, pt, eng = _setup(name, E, f64, kind, sigma=0.1, vec=vec)
    ret, traj = _roll(eng, pt, K, seed=5)
    want = vec or 1
    assert eng.last_kernels == f'cl_rollout_policy_kpi_kernel<{want}, {_prec(f64)}>', eng.last_kernels
    ref = StepEngine(tab, E, reward=kind, kpi=True, f64_maps=f64)
    _replay(ref, pt, traj, eng, ret, f'policy kpi rollout vs single steps {name} {kind} E={E} f64_maps={f64} vec={vec}')
    assert eng.t == K and torch.equal(traj[K - 1, N], eng.net) and torch.equal(traj[K - 1, S], eng.soc) and torch.equal(traj[K - 1, R], eng.reward_bldg)
    assert float(eng.kpi_bldg.abs().sum()) > 0 and float(eng.kpi_env[abi.CLKE_DAY_N].min()) == 1.0
    return eng, ref, traj


@pytest.mark.parametrize('vec', [1, 2])
@pytest.mark.parametrize('E', [64, 260])
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('kind', KINDS)
def test_2_kpis_equal_single_steps(kind, f64, E, vec):
    """K = 30 closed-loop steps with sigma = 0.1 and the record on; `traj[:, A]` fed step by step to a second `kpi=True` engine's `step()`:
    every KPI plane, the state, the last outputs, the district sums and the return at the two-paths tolerances (return rtol 1e-5 / atol 1e-3),
    the per-step planes at test_b's."""
    _check_2('g2022_all', kind, E, f64, vec)


@pytest.mark.parametrize('vec', [1, 2])
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('kind', ['RewardFunction', 'MARL'])
@pytest.mark.parametrize('name', ['b1', 'b2', 'b32', 'het17'])
def test_2_kpis_equal_single_steps_on_the_geometry_districts(name, kind, f64, vec):
    """The same on one building (one wave), two (no wave without a second building), 32 (sixteen waves: at two envs per lane the LDS request is
    above 64 KiB and the launch opts in -- asserted from the formula) and het17 (no battery / idle action / no PV / a shorter observation vector)."""
    eng, ref, traj = _check_2(name, kind, 260, f64, vec)
    if name == 'b32':
        assert (_lib.policy_kpi_lds_bytes(16, vec) > 65536) == (vec == 2)
    if name == 'het17':
        undriven = list(HET_UNDRIVEN)
        assert bool((traj[:, A, undriven] == 0).all()) and torch.equal(eng.state[:, undriven], ref.state[:, undriven])


@pytest.mark.parametrize('f64', ['chain', False])
def test_2_default_geometry_at_4096_envs(f64):
    _check_2('g2022_all', 'MARL', 4096, f64, None)


# ---- 3. finalised KPIs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('name', ['g2022_all', 'b1', 'het17'])
def test_3_finalised_kpis(name, f64):
    """`VectorCityLearnEnv(kpi=True).rollout_policy(pol, 57, kpi=True)` + `evaluate()` against an env that steps the recorded actions."""
    from citylearn_amd.vector_env import VectorCityLearnEnv
    spec = _spec(name)
    E, K = 64, 57
    mk = lambda: VectorCityLearnEnv(spec, E, kpi=True, reward_function=REWARD_CLASS, f64_maps=f64)
    a, b = mk(), mk()
    b.engine.trace_kernels()
    layout = ObservationLayout(b.spec, 'current', False)
    pol = make_policy(layout, 16, seed=8, sigma=0.05)
    ret, traj = b.rollout_policy(pol, K, seed=3, record=True, kpi=True)
    assert b.engine.last_kernels == f'cl_rollout_policy_kpi_kernel<1, {_prec(f64)}>' and b.time_step == K
    pt = pol.pack(layout, b.tables)
    ret_ref = torch.zeros(E, device='cuda')
    for k in range(K):
        ret_ref += a.step(_step_actions(a.engine, pt, traj[k, A]))[1].sum(dim=0)
    torch.testing.assert_close(ret, ret_ref, rtol=1e-5, atol=1e-3)
    _compare_kpi_planes(b.engine, a.engine, name)
    got, want = b.evaluate(), a.evaluate()
    _finalised_close(got, want)
    assert got[0] and got[1] and any(bool(torch.isfinite(v).all()) for v in got[1].values())
    fin = lambda g, r: max([_bar(g[n], r[n]) for n in r if bool(torch.isfinite(r[n]).any())] or [0.0])
    record_worst({'building': fin(got[0], want[0]), 'district': fin(got[1], want[1])}, f'policy kpi finalised {name} f64_maps={f64}')


# ---- 4. the policy is still the policy ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('vec', [1, 2])
@pytest.mark.parametrize('sigma', [None, 0.1])
@pytest.mark.parametrize('H', [4, 32])
@pytest.mark.parametrize('f64', ['chain', False])
def test_4_teacher_forced_actions(f64, H, sigma, vec):
    """Every recorded action recomputed in float64 from the recorded inputs; gate: 4 x a float32 torch evaluation's deviation."""
    E, K = 260, 24
    spec, tab, layout, pol, pt, eng = _setup('g2022_all', E, f64, H=H, sigma=sigma, vec=vec)
    _, traj = _roll(eng, pt, K, seed=11)
    assert eng.last_kernels == f'cl_rollout_policy_kpi_kernel<{vec}, {_prec(f64)}>'
    dev_kernel, dev_f32 = _teacher_forced(eng, tab, layout, pol, pt, traj, seed=11)
    print(f'teacher-forced vec={vec} f64={f64} H={H} sigma={sigma}: kernel {dev_kernel:.3e}  float32 torch {dev_f32:.3e}  ratio {dev_kernel / dev_f32:.2f}')
    record_worst({'kernel': dev_kernel, 'float32_torch': dev_f32, 'ratio': dev_kernel / dev_f32}, f'policy kpi teacher-forced f64_maps={f64} vec={vec} H={H} sigma={sigma}')
    assert dev_f32 > 0 and dev_kernel <= 4.0 * dev_f32, (dev_kernel, dev_f32)


@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('kind', ['MARL', 'RewardFunction'])
def test_4_free_running_against_the_cpu(kind, f64):
    """K = 48 from reset: the host loop of `COracle.step` + `actions_host` (float64) against one launch at the plain bar."""
    E, K = 64, 48
    spec, tab, layout, pol, pt, eng = _setup('g2022_all', E, f64, kind, H=16)
    want = host_closed_loop(spec, tab, layout, pol, pt, K, E, reward=kind)
    _, traj = _roll(eng, pt, K)
    tr = traj.cpu().numpy().astype(np.float64)
    bar = lambda got, ref: float((np.abs(got - ref) / (1e-4 + 1e-4 * np.abs(ref))).max())
    worst = {'soc': bar(tr[:, S], want['soc']), 'net': bar(tr[:, N], want['net']), 'reward': bar(tr[:, R], want['reward']),
             'district_net': bar(tr[:, N].sum(axis=1), want['dnet']),
             'degraded_capacity': bar(eng.degraded_capacity.cpu().numpy(), want['degcap'][-1])}
    print(f'free-running {kind} f64={f64}:', {k: round(v, 4) for k, v in worst.items()})
    check_worst(worst, f'policy kpi free-running {kind} f64_maps={f64}')


# ---- 5. split launches ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('vec', [1, 2])
@pytest.mark.parametrize('f64', ['chain', False])
def test_5_split_launches_and_checkpoint_are_bit_identical(f64, vec):
    """Launches of 1, 5, 24 and 25 steps, with a `state_dict` round trip into a fresh engine in between, equal one 55-step launch bit for bit --
    the record, the state, the outputs and every KPI plane: same kernel, same order of additions (the folds of the district series close on the
    absolute step index).  MARL, noise on."""
    E = 320
    spec, tab, layout, pol, pt, one = _setup('g2022_all', E, f64, 'MARL', sigma=0.1, vec=vec)
    ret1, traj1 = _roll(one, pt, 55, seed=3)
    mk = lambda: StepEngine(tab, E, reward='MARL', kpi=True, f64_maps=f64, tuning=dict(vec=vec))
    eng = mk()
    ret, parts = torch.zeros(E, device='cuda'), []
    for n, K in enumerate((1, 5, 24, 25)):
        if n == 2:
            sd = eng.state_dict()
            eng = mk()
            eng.load_state_dict(sd)
        traj = torch.empty((K, policy.CLPOL_NT, eng.n_bldg, E), device='cuda')
        eng.rollout_policy(K, pt, seed=3, ret_env=ret, traj=traj, kpi=True)
        parts.append(traj)
    assert eng.t == 55 and torch.equal(torch.cat(parts), traj1)
    assert torch.equal(eng.state, one.state) and torch.equal(eng.out_bldg[:2], one.out_bldg[:2]) and torch.equal(eng.out_env, one.out_env)
    assert torch.equal(eng.kpi_bldg, one.kpi_bldg) and torch.equal(eng.kpi_env, one.kpi_env)
    torch.testing.assert_close(ret, ret1, rtol=1e-6, atol=1e-4)               # (four partial sums instead of one)


def test_5_month_boundary_inside_a_launch():
    """720 steps in one launch, then 20 more: t = 730 closes the month group inside the second launch.  The second launch against single steps
    from the state the first one left (a `state_dict` round trip into the reference engine), at check 2's tolerances."""
    g = golden('g2022_p1_year')
    spec = g.spec()
    tab = spec.episode_tables(0)
    E = 8
    layout = ObservationLayout(spec, 'current', True)
    pol = make_policy(layout, 8, seed=2, sigma=0.1)
    pt = pol.pack(layout, tab, device='cuda:0')
    eng, ref = StepEngine(tab, E, kpi=True), StepEngine(tab, E, kpi=True)
    eng.trace_kernels()
    _roll(eng, pt, 720, seed=4, record=False)
    assert eng.t == 720 and float(eng.kpi_env[abi.CLKE_MON_N].max()) == 0.0 and float(eng.kpi_env[abi.CLKE_DAY_N].min()) == 29.0
    ref.load_state_dict(eng.state_dict())
    ret, traj = _roll(eng, pt, 20, seed=4)
    _replay(ref, pt, traj, eng, ret, 'policy kpi rollout vs single steps g2022_p1_year month boundary')
    assert eng.t == 740
    assert float(eng.kpi_env[abi.CLKE_MON_N].min()) == 1.0 == float(eng.kpi_env[abi.CLKE_MON_N].max())
    assert float(eng.kpi_env[abi.CLKE_PER_COND + abi.CLKE_MON_N, 0]) == 1.0


# ---- 6. windows, sets, offsets ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', ['chain', False])
def test_6_windows_sets_and_env_offsets(f64):
    """Two env blocks with different `env_row0` and different parameter sets in one 512-env launch: each block equals, bit for bit, a 256-env
    engine of its own with that window, that set and its env offset -- the KPI planes too, the baseline rows at the block's first env included."""
    spec = golden('g2022_all').spec()
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    pol = make_policy(layout, 16, n_sets=2, seed=2, sigma=0.1)
    K, n_steps, rows = 30, 200, [0, 131]
    whole = StepEngine(tab, 512, kpi=True, f64_maps=f64, n_steps=n_steps, env_row0=rows)
    _, traj = _roll(whole, pol.pack(layout, tab, device='cuda:0', set_of_block=[0, 1]), K, seed=9)
    assert not torch.equal(traj[:, A, :, :256], traj[:, A, :, 256:])
    for g in range(2):
        part = StepEngine(tab, 256, kpi=True, f64_maps=f64, n_steps=n_steps, env_row0=[rows[g]], env_offset=256 * g)
        _, tr = _roll(part, pol.pack(layout, tab, device='cuda:0', set_of_block=[g]), K, seed=9)
        sl = slice(256 * g, 256 * (g + 1))
        assert torch.equal(tr, traj[:, :, :, sl]), g
        assert torch.equal(part.state, whole.state[:, :, sl]) and torch.equal(part.out_env, whole.out_env[:, sl])
        assert torch.equal(part.kpi_bldg, whole.kpi_bldg[:, :, sl]) and torch.equal(part.kpi_env, whole.kpi_env[:, sl]), g
    first = torch.zeros(512, dtype=torch.bool, device='cuda')
    first[::abi.CL_ROW0_BLOCK] = True
    base = whole.kpi_bldg[abi.CLK_B_NET]
    assert bool((base[:, first] != 0).all()) and bool((base[:, ~first] == 0).all()) and float(base[0, 0]) != float(base[0, 256])
    assert bool((whole.kpi_env[abi.CLKE_PER_COND + abi.CLKE_PREV][first] != 0).all())


# ---- 7. refusals and defaults -----------------------------------------------------------------------------------------------------------
def _planes(eng):
    return [x.clone() for x in (eng.state, eng.out_bldg, eng.out_env, eng.kpi_bldg, eng.kpi_env) if x is not None]


def _unchanged(eng, before):
    return all(torch.equal(x, y) for x, y in zip(before, _planes(eng)))


def test_7_keyword_and_engine_must_agree():
    from citylearn_amd.vector_env import VectorCityLearnEnv
    g = golden('g2022_all')
    E = 64
    pol = make_policy(ObservationLayout(g.spec(), 'current', False), 8, seed=1)
    plain, kenv = VectorCityLearnEnv(g.schema_path, E), VectorCityLearnEnv(g.schema_path, E, kpi=True)
    for env in (plain, kenv):
        env.step(torch.zeros((env.n_act_cols, E), device='cuda'))
    before = _planes(plain.engine)
    with pytest.raises(ValueError, match='kpi=True'):
        plain.rollout_policy(pol, 4, kpi=True)
    assert plain.time_step == 1 and _unchanged(plain.engine, before)
    with pytest.raises(ValueError, match='kpi=True'):
        plain.engine.rollout_policy(4, pol.pack(ObservationLayout(g.spec(), 'current', False), plain.tables, device='cuda:0'), kpi=True)
    assert _unchanged(plain.engine, before)
    before = _planes(kenv.engine)
    with pytest.raises(Exception, match='CLD_KPI'):                  # kpi=False is today's call: the policy library refuses a kpi=True env
        kenv.rollout_policy(pol, 4)
    assert kenv.time_step == 1 and _unchanged(kenv.engine, before)
    kenv.rollout_policy(pol, 4, kpi=True)
    assert kenv.time_step == 5 and not _unchanged(kenv.engine, before)


@pytest.mark.parametrize('case', ['thermal', 'tiled33', 'f64_maps'])
def test_7_refusals_leave_everything_untouched(case):
    """Districts the kernel does not cover are refused by the LIBRARY (CL_EINVAL, naming the cause), and no plane moves.  The tables handed over
    are shaped for the district and otherwise empty: the refusal comes before anything reads them."""
    from citylearn_amd.synthetic import tile_district
    kw = {}
    if case == 'thermal':
        spec, word = golden('g2020_cz1').spec(), 'CLD_LEAN'
    elif case == 'tiled33':
        spec, word = tile_district(golden('g2022_all').spec(), 33), 'n_bldg=33'
    else:
        spec, kw, word = golden('g2022_all').spec(), dict(f64_maps=True), 'CLD_F64_MAPS'
    tab = spec.episode_tables(0)
    E = 64
    eng = StepEngine(tab, E, kpi=True, **kw)
    eng.step(torch.zeros((eng.n_act_cols, E), device='cuda'))
    z = lambda *shape: torch.zeros(shape, device='cuda')
    B = eng.n_bldg
    pt = policy.PolicyTables(z(1, eng.n_ts_rows, B, 8), z(1, B, 2, 8), z(1, B, 9), None, z(eng.n_act_cols) - 1, z(eng.n_act_cols) + 1, None, None,
                             np.arange(B), -np.ones(B), np.ones(B), np.zeros(B), 0)
    before = _planes(eng)
    with pytest.raises(_lib.EngineError) as e:
        eng.rollout_policy(5, pt, kpi=True)
    assert e.value.code == abi.CL_EINVAL and 'clpk_rollout_mlp_kpi_f32' in str(e.value) and word in str(e.value)
    assert eng.t == 1 and _unchanged(eng, before)
