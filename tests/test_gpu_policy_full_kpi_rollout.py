"""The closed-loop policy rollout of THERMAL districts that keeps the streaming KPIs (`StepEngine.rollout_policy(kpi=True)` /
`VectorCityLearnEnv.rollout_policy(kpi=True)` with a `StorageMLPPolicy`: one launch of `cl_rollout_full_policy_kpi_kernel`,
csrc/cl_policy_full.h at KPI = true, ``libcitylearn_amd_policy_full_kpi.so``).

Nothing here compares the kernel with itself, except where two launches of it must agree (split launches, env blocks).  The references: the
SINGLE-STEP path with `kpi=True` fed the recorded actions (`cl_step_full_kpi_kernel` in fp32; under the float64 chain the step with the
`CLD_DETAIL_MIN` planes + `cl_kpi_kernel`), at tests/test_gpu_policy_full_rollout.py::_replay's and tests/test_gpu_rollout_kpi.py's two-paths
tolerances; the float64 MLP on the recorded inputs; the CPU oracle's closed loop.  The outage branch (`clv::unit_step<.., OUT = true>`, `saw_outage` and the
two sums CLK_UNSERVED_OUTAGE / CLK_EXPECTED_OUTAGE) runs on the outage districts of tests/policy_full_util.py (`outage_district`: g2020_cz1 and
its cuts with chosen outage rows and charged tanks; no LSTM stage, so the packer accepts them) -- tests 2, 3, 5, 6 and 7 each have a case there;
the single-step reference is itself pinned on that district against the C oracle by tests/test_gpu_outage_thermal.py.  Measured readings:
profiles/policy_full_kpi_parity.md."""
import numpy as np
import pytest
import torch

from golden_util import check_worst, golden, record_worst
from citylearn_amd import _lib, abi, policy
from citylearn_amd.engine import StepEngine
from citylearn_amd.observations import ObservationLayout
from policy_full_util import host_closed_loop, make_storage_policy, outage_mask, thermal_district
from test_gpu_policy_full_rollout import A, KINDS, N, NA, R, S, _scatter, _teacher_forced
from test_gpu_rollout_geometry import _bar, _prec
from test_gpu_rollout_kpi import REWARD_CLASS, _finalised_close

pytestmark = pytest.mark.gpu

DETAIL_MIN = [abi.CLO_COOL_DEM, abi.CLO_HEAT_DEM, abi.CLO_BASE_NET, abi.CLO_EXPECTED, abi.CLO_SERVED]
OUTAGE = [abi.CLK_UNSERVED_OUTAGE, abi.CLK_EXPECTED_OUTAGE]


def _setup(E, f64='chain', kind='RewardFunction', H=16, sigma=None, n_sets=1, district='g2020_cz1', **kw):
    spec = thermal_district(district)
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    pol = make_storage_policy(layout, H, n_sets=n_sets, seed=H, sigma=sigma)
    pt = pol.pack(layout, tab, device='cuda:0')
    eng = StepEngine(tab, E, reward=kind, kpi=True, f64_maps=f64, **kw)
    assert not eng.lean and eng.kpi and eng.f64_chain == (f64 == 'chain') and not eng.kpi_shared_baseline
    assert bool(eng.detail) == (f64 == 'chain')                      # the chain engine carries CLD_WRITE_DETAIL | CLD_DETAIL_MIN, the fp32 one nothing
    eng.trace_kernels()
    return spec, tab, layout, pol, pt, eng


def _roll(eng, pt, K, seed=0, record=True):
    ret = torch.zeros(eng.n_env, device='cuda')
    traj = torch.full((K, policy.CLPF_NT, eng.n_bldg, eng.n_env), float('nan'), device='cuda') if record else None
    eng.rollout_policy(K, pt, seed=seed, ret_env=ret, traj=traj, kpi=True)
    assert traj is None or not torch.isnan(traj).any()
    return ret, traj


def _compare_kpi(b, a, what=''):
    """`b` (the launch) against `a` (single steps): tests/test_gpu_rollout_kpi.py::_compare_kpi_planes's numbers; the two outage planes bit-equal."""
    torch.testing.assert_close(b.kpi_bldg, a.kpi_bldg, rtol=1e-4, atol=1e-3, msg=lambda m: f'kpi_bldg {what}: {m}')
    ke_b, ke_a = b.kpi_env.clone(), a.kpi_env.clone()
    inf_b, inf_a = torch.isinf(ke_b), torch.isinf(ke_a)
    assert torch.equal(inf_b, inf_a) and torch.equal(ke_b[inf_b], ke_a[inf_a]), f'open maximum groups {what}'
    ke_b[inf_b] = 0.0; ke_a[inf_a] = 0.0
    torch.testing.assert_close(ke_b, ke_a, rtol=1e-4, atol=1e-2, msg=lambda m: f'kpi_env {what}: {m}')
    for cond in (0, abi.CLKE_PER_COND):
        for row in (abi.CLKE_DAY_N, abi.CLKE_MON_N):
            assert torch.equal(b.kpi_env[cond + row], a.kpi_env[cond + row]), f'group counter {cond + row} {what}'
    assert torch.equal(b.kpi_bldg[OUTAGE], a.kpi_bldg[OUTAGE])


def _outage_sums_moved(eng, before, has):
    """The two outage sums against their values `before` the launch(es): bit-equal for the buildings without an outage row (`has` [n_bldg] bool),
    moved for the others -- the expected energy for every env, the unserved energy for some env of every such building -- and
    0 <= unserved <= expected everywhere."""
    has = torch.as_tensor(np.asarray(has), device=eng.kpi_bldg.device)
    now = eng.kpi_bldg[OUTAGE]
    assert torch.equal(now[:, ~has], before[:, ~has])
    assert bool((now[1][has] > before[1][has]).all()) and bool((now[0][has] > before[0][has]).any(dim=1).all())
    assert bool((now[0] >= 0).all()) and bool((now[0] <= now[1]).all())


def _replay(ref, pt, traj, eng, ret, label, tab=None):
    """The recorded head planes scattered to action columns and fed step by step to `ref.step()` (a `kpi=True` engine in the state the launch
    started from): tests/test_gpu_policy_full_rollout.py::_replay's tolerances, then the KPI planes and (chain) the CLD_DETAIL_MIN planes.
    `tab`: the episode tables of a district with outage rows (from step 0; one episode window)."""
    K = traj.shape[0]
    t_first = ref.t
    worst = {}
    ret_ref = torch.zeros(ref.n_env, device='cuda')
    reset_outage = ref.kpi_bldg[OUTAGE].clone()
    for k in range(K):
        ref.step(_scatter(pt, traj[k, A:A + NA], ref.n_act_cols))
        ret_ref += ref.district_reward
        for key, got, want in (('soc', traj[k, S:S + 4], ref.state[[0, 3, 4, 5]]), ('net', traj[k, N], ref.net), ('reward', traj[k, R], ref.reward_bldg)):
            worst[key] = max(worst.get(key, 0.0), _bar(got, want))
        torch.testing.assert_close(traj[k, S:S + 4], ref.state[[0, 3, 4, 5]], rtol=2e-6, atol=2e-6)
        torch.testing.assert_close(traj[k, N], ref.net, rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(traj[k, R], ref.reward_bldg, rtol=2e-5, atol=2e-5)
    worst.update(state=_bar(eng.state, ref.state), out_env=_bar(eng.out_env, ref.out_env), kpi_bldg=_bar(eng.kpi_bldg, ref.kpi_bldg),
                 kpi_env=_bar(eng.kpi_env, ref.kpi_env), kpi_outage=_bar(eng.kpi_bldg[OUTAGE], ref.kpi_bldg[OUTAGE]), **{'return': _bar(ret, ret_ref)})
    if eng.f64_chain:
        worst['detail'] = _bar(eng.out_bldg[DETAIL_MIN], ref.out_bldg[DETAIL_MIN])
    print(label, {k: round(v, 4) for k, v in worst.items()})
    record_worst(worst, label)
    assert eng.t == ref.t
    torch.testing.assert_close(eng.state[:6], ref.state[:6], rtol=2e-6, atol=2e-6)
    torch.testing.assert_close(eng.out_bldg[:2], ref.out_bldg[:2], rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(eng.out_env, ref.out_env, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(ret, ret_ref, rtol=1e-5, atol=1e-3)
    _compare_kpi(eng, ref, label)
    if eng.f64_chain:
        torch.testing.assert_close(eng.out_bldg[DETAIL_MIN], ref.out_bldg[DETAIL_MIN], rtol=2e-5, atol=2e-5)
        assert float(eng.out_bldg[abi.CLO_EXPECTED].abs().sum()) > 0
    m = None if tab is None else outage_mask(tab, t_first + K)[t_first:]
    if m is None or not m.any():
        assert torch.equal(eng.kpi_bldg[OUTAGE], reset_outage)
    else:
        assert torch.equal(traj[:, N] == 0, torch.as_tensor(m, device='cuda')[:, :, None].expand(-1, -1, traj.shape[3]))
        _outage_sums_moved(eng, reset_outage, m.any(axis=0))
        _outage_sums_moved(ref, reset_outage, m.any(axis=0))
    assert torch.equal(traj[K - 1, N], eng.net) and torch.equal(traj[K - 1, S], eng.soc) and torch.equal(traj[K - 1, R], eng.reward_bldg)


# ---- 1. one launch --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', ['chain', False])
def test_1_one_launch(f64):
    spec, tab, layout, pol, pt, eng = _setup(260, f64)
    _roll(eng, pt, 9, record=False)
    assert eng.last_kernels == f'cl_rollout_full_policy_kpi_kernel<{_prec(f64)}, false>', eng.last_kernels
    assert eng.t == 9 and float(eng.kpi_bldg.abs().sum()) > 0


# ---- 2. KPIs against the single-step path -----------------------------------------------------------------------------------------------
def _check_2(name, kind, E, f64):
    K = 30                                                           # crosses a day group (t = 24) and leaves a partial fold (30 = 3 x 8 + 6)
    spec, tab, layout, pol, pt, eng = _setup(E, f64, kind, sigma=0.1, district=name)
    ret, traj = _roll(eng, pt, K, seed=5)
    assert eng.last_kernels == f"cl_rollout_full_policy_kpi_kernel<{_prec(f64)}, {'true' if kind == 'MARL' else 'false'}>", eng.last_kernels
    ref = StepEngine(tab, E, reward=kind, kpi=True, f64_maps=f64)
    _replay(ref, pt, traj, eng, ret, f'thermal policy kpi rollout vs single steps {name} {kind} E={E} f64_maps={f64}', tab=tab)
    assert bool(tab.outage[:K].any()) == name.endswith('_outage')
    assert eng.t == K and float(eng.kpi_env[abi.CLKE_DAY_N].min()) == 1.0 == float(eng.kpi_env[abi.CLKE_PER_COND + abi.CLKE_DAY_N].min())
    assert bool((eng.kpi_bldg[abi.CLK_B_NET] != 0).all())           # every env keeps its own baseline, not only its block's first
    return eng


@pytest.mark.parametrize('E', [64, 260])
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('kind', KINDS)
def test_2_kpis_equal_single_steps(kind, f64, E):
    """K = 30 closed-loop steps with sigma = 0.1 and the record on, the recorded head planes fed step by step to a second `kpi=True` engine."""
    _check_2('g2020_cz1', kind, E, f64)


@pytest.mark.parametrize('E', [64, 260])
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('kind', KINDS)
def test_2_kpis_equal_single_steps_under_an_outage(kind, f64, E):
    """The same on the nine-building outage district: the launch meets outage rows 5 .. 16 (staggered) and 22 .. 26 (common, across the day
    group and a fold), in six of its nine waves.  The two outage sums: bit-equal to the single-step path's (`_compare_kpi`), moved for the
    buildings with outage rows, at their reset value for buildings 2, 5 and 8, 0 <= unserved <= expected (`_replay`)."""
    _check_2('g2020_cz1_outage', kind, E, f64)


@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('kind', ['RewardFunction', 'MARL'])
@pytest.mark.parametrize('name', ['t1', 't2', 't16', 't1_outage', 't2_outage', 't16_outage'])
def test_2_kpis_equal_single_steps_on_the_geometry_districts(name, kind, f64):
    """One building (one wave folds both series), two (one without DHW storage), sixteen (the largest LDS request: above 64 KiB, the launch opts in);
    and their outage versions (the one wave at times on an outage row alone; sixteen with five buildings that never see one)."""
    eng = _check_2(name, kind, 64, f64)
    assert (_lib.policy_full_kpi_lds_bytes(eng.n_bldg) > 65536) == name.startswith('t16')


# ---- 3. finalised KPIs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', ['chain', False])
def test_3_finalised_kpis(f64):
    """`VectorCityLearnEnv(kpi=True).rollout_policy(spolicy, 57, kpi=True)` + `evaluate()` against an env that steps the recorded actions."""
    _check_3(f64, golden('g2020_cz1').schema_path, 'g2020_cz1')


@pytest.mark.parametrize('f64', ['chain', False])
def test_3_finalised_kpis_under_an_outage(f64):
    """The same through an env built from the nine-building outage district's spec: every outage row of the fixture is inside the 57 steps, and
    the two unserved-energy KPIs of the district come out finite and positive (on the plain district the outage one is 0 / 0)."""
    got = _check_3(f64, thermal_district('g2020_cz1_outage'), 'g2020_cz1_outage')
    for name in ('power_outage_normalized_unserved_energy_total', 'annual_normalized_unserved_energy_total'):
        v = got[1][name]
        assert bool(torch.isfinite(v).all()) and bool((v > 0).all()) and bool((v <= 1).all()), (name, v)
    per_building = got[0]['power_outage_normalized_unserved_energy_total']
    assert bool(torch.isfinite(per_building[[0, 1, 3, 4, 6, 7]]).all()) and not bool(torch.isfinite(per_building[[2, 5, 8]]).any())


def _check_3(f64, schema, name):
    from citylearn_amd.vector_env import VectorCityLearnEnv
    E, K = 64, 57
    mk = lambda: VectorCityLearnEnv(schema, E, kpi=True, reward_function=REWARD_CLASS, f64_maps=f64)
    a, b = mk(), mk()
    b.engine.trace_kernels()
    layout = ObservationLayout(b.spec, 'current', False)
    pol = make_storage_policy(layout, 16, seed=8, sigma=0.05)
    ret, traj = b.rollout_policy(pol, K, seed=3, record=True, kpi=True)
    assert b.engine.last_kernels == f'cl_rollout_full_policy_kpi_kernel<{_prec(f64)}, false>' and b.time_step == K
    pt = pol.pack(layout, b.tables)
    ret_ref = torch.zeros(E, device='cuda')
    for k in range(K):
        ret_ref += a.step(_scatter(pt, traj[k, A:A + NA], a.n_act_cols))[1].sum(dim=0)
    torch.testing.assert_close(ret, ret_ref, rtol=1e-5, atol=1e-3)
    _compare_kpi(b.engine, a.engine, 'finalised')
    got, want = b.evaluate(), a.evaluate()
    _finalised_close(got, want)
    assert got[0] and got[1] and any(bool(torch.isfinite(v).all()) for v in got[1].values())
    fin = lambda g_, r_: max([_bar(g_[n], r_[n]) for n in r_ if bool(torch.isfinite(r_[n]).any())] or [0.0])
    record_worst({'building': fin(got[0], want[0]), 'district': fin(got[1], want[1])}, f'thermal policy kpi finalised {name} f64_maps={f64}')
    return got


# ---- 4. the policy is still the policy ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sigma', [None, 0.1])
@pytest.mark.parametrize('H', [4, 32])
@pytest.mark.parametrize('f64', ['chain', False])
def test_4_teacher_forced_actions(f64, H, sigma):
    """Every recorded action recomputed in float64 from the recorded inputs; gate: 4 x a float32 torch evaluation's deviation."""
    E, K = 260, 24
    spec, tab, layout, pol, pt, eng = _setup(E, f64, H=H, sigma=sigma)
    _, traj = _roll(eng, pt, K, seed=11)
    dev_kernel, dev_f32 = _teacher_forced(tab, layout, pol, pt, traj, seed=11)
    print(f'teacher-forced f64={f64} H={H} sigma={sigma}: kernel {dev_kernel:.3e}  float32 torch {dev_f32:.3e}  ratio {dev_kernel / dev_f32:.2f}')
    record_worst({'kernel': dev_kernel, 'float32_torch': dev_f32, 'ratio': dev_kernel / dev_f32}, f'thermal policy kpi teacher-forced f64_maps={f64} H={H} sigma={sigma}')
    assert dev_f32 > 0 and dev_kernel <= 4.0 * dev_f32, (dev_kernel, dev_f32)


def test_4_free_running_against_the_cpu():
    """K = 48 from reset: the host loop of `COracle.step` + `actions_host` (float64) against one launch, at the plain bar."""
    E, K = 64, 48
    spec, tab, layout, pol, pt, eng = _setup(E, 'chain', H=16)
    want = host_closed_loop(spec, tab, layout, pol, pt, K, E)
    _, traj = _roll(eng, pt, K)
    tr = traj.cpu().numpy().astype(np.float64)
    bar = lambda got, ref: float((np.abs(got - ref) / (1e-4 + 1e-4 * np.abs(ref))).max())
    worst = {'soc': bar(tr[:, S], want['soc']), 'cs': bar(tr[:, S + 1], want['cs']), 'ds': bar(tr[:, S + 3], want['ds']),
             'net': bar(tr[:, N], want['net']), 'reward': bar(tr[:, R], want['reward']), 'district_net': bar(tr[:, N].sum(axis=1), want['dnet']),
             'degraded_capacity': bar(eng.degraded_capacity.cpu().numpy(), want['degcap'][-1])}
    print('free-running:', {k: round(v, 4) for k, v in worst.items()})
    check_worst(worst, 'thermal policy kpi free-running RewardFunction f64_maps=chain')


# ---- 5. split launches ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', ['chain', False])
def test_5_split_launches_and_checkpoint_are_bit_identical(f64):
    """Launches of 1, 5, 24 and 25 steps, with a `state_dict` round trip into a fresh engine in between, equal one 55-step launch bit for bit --
    the record, the state, the outputs and every KPI plane (the folds of the district series close on the absolute step index).  MARL, noise on."""
    _check_5(f64, 'g2020_cz1', (1, 5, 24, 25))


@pytest.mark.parametrize('split', [(1, 5, 24, 25), (30, 25), (27, 13, 15)], ids=lambda x: '+'.join(map(str, x)))
@pytest.mark.parametrize('f64', ['chain', False])
def test_5_split_launches_under_an_outage(f64, split):
    """The same on the nine-building outage district, every KPI plane bit for bit.  1 + 5 + 24 + 25: the first launch meets no outage row (it
    must not store the two outage sums), the boundary at step 6 lies inside the first outage of buildings 0 and 1.  30 + 25 and 27 + 13 + 15: a
    launch that saw no outage row of a building (the middle one, rows 27 .. 39: of none) must leave alone the sums an earlier launch moved."""
    _check_5(f64, 'g2020_cz1_outage', split)


def _check_5(f64, district, split):
    E = 320
    spec, tab, layout, pol, pt, one = _setup(E, f64, 'MARL', sigma=0.1, district=district)
    ret1, traj1 = _roll(one, pt, 55, seed=3)
    assert one.last_kernels == f'cl_rollout_full_policy_kpi_kernel<{_prec(f64)}, true>', one.last_kernels
    mk = lambda: StepEngine(tab, E, reward='MARL', kpi=True, f64_maps=f64)
    eng = mk()
    ret, parts = torch.zeros(E, device='cuda'), []
    reset_outage = eng.kpi_bldg[OUTAGE].clone()
    m = outage_mask(tab, 55)
    for n, K in enumerate(split):
        if n == 2:
            sd = eng.state_dict()
            eng = mk()
            eng.load_state_dict(sd)
        traj = torch.empty((K, policy.CLPF_NT, eng.n_bldg, E), device='cuda')
        before = eng.kpi_bldg[OUTAGE].clone()
        eng.rollout_policy(K, pt, seed=3, ret_env=ret, traj=traj, kpi=True)
        parts.append(traj)
        if m.any():
            seen = m[eng.t - K:eng.t].any(axis=0)
            _outage_sums_moved(eng, before, seen)
            if not seen.any() and eng.t > 26:  # (the sums an earlier launch moved are still there)
                assert not torch.equal(before, reset_outage)
    if m.any():
        _outage_sums_moved(one, reset_outage, m.any(axis=0))
    assert eng.t == 55 and torch.equal(torch.cat(parts), traj1)
    assert torch.equal(eng.state, one.state) and torch.equal(eng.out_bldg, one.out_bldg) and torch.equal(eng.out_env, one.out_env)
    assert torch.equal(eng.kpi_bldg, one.kpi_bldg) and torch.equal(eng.kpi_env, one.kpi_env)
    torch.testing.assert_close(ret, ret1, rtol=1e-6, atol=1e-4)               # (four partial sums instead of one)


# ---- 6. month boundary ------------------------------------------------------------------------------------------------------------------
def test_6_month_boundary_inside_a_launch():
    """g2020_cz1 has 744 rows: 720 steps in one launch, then 20 more -- t = 730 closes the month group inside the second launch, which is replayed
    through single steps from a `state_dict` copy of what the first one left."""
    E = 8
    spec, tab, layout, pol, pt, eng = _setup(E, 'chain', H=8, sigma=0.1)
    ref = StepEngine(tab, E, kpi=True, f64_maps='chain')
    _roll(eng, pt, 720, seed=4, record=False)
    mon = [abi.CLKE_MON_N, abi.CLKE_PER_COND + abi.CLKE_MON_N]
    assert eng.t == 720 and float(eng.kpi_env[mon].max()) == 0.0 and float(eng.kpi_env[abi.CLKE_DAY_N].min()) == 29.0
    ref.load_state_dict(eng.state_dict())
    ret, traj = _roll(eng, pt, 20, seed=4)
    _replay(ref, pt, traj, eng, ret, 'thermal policy kpi rollout vs single steps g2020_cz1 month boundary')
    assert eng.t == 740 and float(eng.kpi_env[mon].min()) == 1.0 == float(eng.kpi_env[mon].max())


def test_6_launch_ending_on_an_outage_row():
    """K = 25 on the nine-building outage district: the last step (24) lies inside the common outage 22 .. 26, so the `CLD_DETAIL_MIN` planes the
    chain launch leaves in `out_bldg` for the next KPI pass are an OUTAGE step's (expected and served energy, baseline net, delivered demands)
    -- against the single steps (`_replay`: 2e-5), and the served energy of an outage row differs from the expected one somewhere."""
    E, K = 64, 25
    spec, tab, layout, pol, pt, eng = _setup(E, 'chain', sigma=0.1, district='g2020_cz1_outage')
    ref = StepEngine(tab, E, kpi=True, f64_maps='chain')
    ret, traj = _roll(eng, pt, K, seed=4)
    assert eng.last_kernels == 'cl_rollout_full_policy_kpi_kernel<2, false>', eng.last_kernels
    _replay(ref, pt, traj, eng, ret, 'thermal policy kpi rollout vs single steps g2020_cz1_outage launch ending on an outage row', tab=tab)
    dark = torch.as_tensor(outage_mask(tab, K)[K - 1], device='cuda')
    assert dark.tolist() == [i % 3 != 2 for i in range(9)] and not eng.net[dark].any() and bool((eng.net[~dark] != 0).all())
    ex, sv = eng.out_bldg[abi.CLO_EXPECTED], eng.out_bldg[abi.CLO_SERVED]
    assert bool((sv[dark] <= ex[dark]).all()) and bool((sv[dark] < ex[dark]).any()) and bool((ex[dark] > 0).all())


# ---- 7. windows, sets, offsets ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', ['chain', False])
def test_7_windows_sets_and_env_offsets(f64):
    """Two env blocks with different `env_row0` and different parameter sets in one 512-env launch: each block equals, bit for bit, a 256-env
    engine of its own with that window, that set and its env offset -- the KPI planes too."""
    _check_7(f64, 'g2020_cz1')


@pytest.mark.parametrize('f64', ['chain', False])
def test_7_windows_sets_and_env_offsets_under_an_outage(f64):
    """The same on the nine-building outage district: the outage rows lie in block 0's window (rows 0 .. 29) only -- block 1 (rows 131 .. 160)
    keeps its outage sums at the reset value while block 0's move, in one launch."""
    _check_7(f64, 'g2020_cz1_outage')


def _check_7(f64, district):
    spec = thermal_district(district)
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    pol = make_storage_policy(layout, 16, n_sets=2, seed=2, sigma=0.1)
    K, n_steps, rows = 30, 200, [0, 131]
    whole = StepEngine(tab, 512, kpi=True, f64_maps=f64, n_steps=n_steps, env_row0=rows)
    whole.trace_kernels()
    reset_outage = whole.kpi_bldg[OUTAGE].clone()
    _, traj = _roll(whole, pol.pack(layout, tab, device='cuda:0', set_of_block=[0, 1]), K, seed=9)
    assert whole.last_kernels == f'cl_rollout_full_policy_kpi_kernel<{_prec(f64)}, false>', whole.last_kernels
    assert not torch.equal(traj[:, A:A + NA, :, :256], traj[:, A:A + NA, :, 256:])
    for g in range(2):
        part = StepEngine(tab, 256, kpi=True, f64_maps=f64, n_steps=n_steps, env_row0=[rows[g]], env_offset=256 * g)
        _, tr = _roll(part, pol.pack(layout, tab, device='cuda:0', set_of_block=[g]), K, seed=9)
        sl = slice(256 * g, 256 * (g + 1))
        assert torch.equal(tr, traj[:, :, :, sl]), g
        assert torch.equal(part.state, whole.state[:, :, sl]) and torch.equal(part.out_env, whole.out_env[:, sl])
        assert torch.equal(part.out_bldg, whole.out_bldg[:, :, sl])
        assert torch.equal(part.kpi_bldg, whole.kpi_bldg[:, :, sl]) and torch.equal(part.kpi_env, whole.kpi_env[:, sl]), g
    base = whole.kpi_bldg[abi.CLK_B_NET]
    assert bool((base != 0).all()) and float(base[0, 0]) != float(base[0, 256])
    if tab.outage.any():
        assert tab.outage[:K].any() and not tab.outage[rows[1]:rows[1] + K].any()
        now = whole.kpi_bldg[OUTAGE]
        assert torch.equal(now[:, :, 256:], reset_outage[:, :, 256:])
        has = torch.as_tensor(tab.outage[:K].any(axis=0), device='cuda')
        assert torch.equal(now[:, ~has, :256], reset_outage[:, ~has, :256]) and bool((now[1][has][:, :256] > reset_outage[1][has][:, :256]).all())
        assert bool((now[0] >= 0).all()) and bool((now[0] <= now[1]).all()) and bool((now[0][has][:, :256] > 0).any(dim=1).all())
    else:
        assert torch.equal(whole.kpi_bldg[OUTAGE], reset_outage)


# ---- 8. refusals and defaults -----------------------------------------------------------------------------------------------------------
def _planes(eng):
    return [x.clone() for x in (eng.state, eng.out_bldg, eng.out_env, eng.kpi_bldg, eng.kpi_env) if x is not None]


def _unchanged(eng, before):
    return all(torch.equal(x, y) for x, y in zip(before, _planes(eng)))


def test_8_keyword_and_engine_must_agree():
    from citylearn_amd.vector_env import VectorCityLearnEnv
    g = golden('g2020_cz1')
    E = 64
    layout = ObservationLayout(g.spec(), 'current', False)
    pol = make_storage_policy(layout, 8, seed=1)
    plain, kenv = VectorCityLearnEnv(g.schema_path, E), VectorCityLearnEnv(g.schema_path, E, kpi=True)
    for env in (plain, kenv):
        env.step(torch.zeros((env.n_act_cols, E), device='cuda'))
        env.engine.trace_kernels()
    before = _planes(plain.engine)
    with pytest.raises(NotImplementedError, match='KPI'):
        plain.rollout_policy(pol, 4, kpi=True)
    assert plain.time_step == 1 and _unchanged(plain.engine, before)
    with pytest.raises(NotImplementedError, match='KPI'):
        plain.engine.rollout_policy(4, pol.pack(layout, plain.tables, device='cuda:0'), kpi=True)
    assert _unchanged(plain.engine, before)
    before = _planes(kenv.engine)
    with pytest.raises(_lib.EngineError, match='CLD_KPI'):           # kpi=False is the call without KPIs: clpf_rollout_mlp_f32 refuses a kpi=True env
        kenv.rollout_policy(pol, 4)
    assert kenv.time_step == 1 and _unchanged(kenv.engine, before)
    kenv.rollout_policy(pol, 4, kpi=True)
    assert kenv.time_step == 5 and not _unchanged(kenv.engine, before)
    assert kenv.engine.last_kernels == 'cl_rollout_full_policy_kpi_kernel<2, false>'
    plain.rollout_policy(pol, 4)                                     # without kpi=True: the launch it always was
    assert plain.engine.last_kernels.startswith('cl_rollout_full_policy_kernel<') and plain.time_step == 5


@pytest.mark.parametrize('case', ['t17', 'lean', 'f64_maps'])
def test_8_refusals_leave_everything_untouched(case):
    """Districts the kernel does not cover are refused by the LIBRARY (CL_EINVAL, naming the cause), and no plane moves.  The tables handed over
    are shaped for the district and otherwise empty: the refusal comes before anything reads them."""
    kw = {}
    if case == 't17':
        spec, word = thermal_district('t17'), 'n_bldg=17'
    elif case == 'lean':
        spec, word = golden('g2022_all').spec(), 'clpk_rollout_mlp_kpi_f32'
    else:
        spec, kw, word = golden('g2020_cz1').spec(), dict(f64_maps=True), 'CLD_F64_MAPS'
    tab = spec.episode_tables(0)
    E = 64
    eng = StepEngine(tab, E, kpi=True, **kw)
    eng.step(torch.zeros((eng.n_act_cols, E), device='cuda'))
    z = lambda *shape: torch.zeros(shape, device='cuda')
    B = eng.n_bldg
    pt = policy.StoragePolicyTables(z(1, eng.n_ts_rows, B, 8), z(1, B, 5, 8), z(1, B, 4, 9), None, z(eng.n_act_cols) - 1, z(eng.n_act_cols) + 1, None, None,
                                    -np.ones((B, 4), dtype=np.int64), np.zeros((B, 4)), np.zeros((B, 4)), np.zeros((B, 4)), 0, 0)
    before = _planes(eng)
    with pytest.raises(_lib.EngineError) as e:
        eng.rollout_policy(5, pt, kpi=True)
    assert e.value.code == abi.CL_EINVAL and 'clpfk_rollout_mlp_kpi_f32' in str(e.value) and word in str(e.value)
    assert eng.t == 1 and _unchanged(eng, before)
