"""The two fused rollout kernels -- `cl_rollout_kpi_kernel` (csrc/cl_rollout.h) and `cl_rollout_policy_kernel` (csrc/cl_policy.h) -- at the
launch geometries their hand-written bookkeeping depends on, beyond the one 17-building district of tests/test_gpu_rollout_kpi.py and
tests/test_gpu_policy_rollout.py: the districts of tests/district_util.py (1, 2, 16, 31, 32 buildings: one wave, no wave without a second
building, the 16-wave limit with and without a half-empty last wave; and `het17`, whose buildings differ: no battery, an inactive storage
action, no PV, a shorter observation vector), both precision models, both pack widths (forced), and an `nw` override above the default.

Nothing here compares a kernel with itself: section 0 first pins the SINGLE-STEP path (`StepEngine.step`) on every district to the float64 CPU
oracle at the plain bar; the fused kernels are then compared with that path, with the float64 MLP on recorded inputs, and with the oracle's
closed loop.  Only where two launches of the SAME kernel must agree (split launches, the `nw` override) is `torch.equal` the check.

Every tolerance is inherited: the plain bar 1e-4 + 1e-4 |ref| against the oracle (golden_util.check_worst), the two-paths-on-one-trajectory
tolerances of test_gpu_rollout_kpi.py's `_compare_step_outputs` / `_compare_kpi_planes` / `_finalised_close` (imported, not copied), and
4 x a float32 torch evaluation for teacher-forced actions.  Measured readings: profiles/fused_rollout_geometry_parity.md."""
import re

import numpy as np
import pytest
import torch

from district_util import DISTRICTS, HET_UNDRIVEN, district, es_columns
from golden_util import check_worst, record_worst
from citylearn_amd import _lib, abi, policy
from citylearn_amd.engine import StepEngine
from citylearn_amd.observations import ObservationLayout
from policy_util import HostObservations, f32_torch_deviation, host_closed_loop, make_policy
from test_gpu_policy_rollout import A, N, R, S, _roll, _teacher_forced
from test_gpu_rollout_kpi import REWARD_CLASS, _actions, _compare_kpi_planes, _compare_step_outputs, _finalised_close, _fused

pytestmark = pytest.mark.gpu

KINDS = ['RewardFunction', 'MARL', 'IndependentSACReward', 'SolarPenaltyReward']
SMALL = ('b1', 'b32', 'het17')                      # where the issue asks for the long forms (finalised KPIs, split launches)
# every district with the two rewards that differ in structure (per-building / coupled through the district net); b32 and het17 with all four
DISTRICT_KINDS = [(d, k) for d in DISTRICTS for k in (KINDS if d in ('b32', 'het17') else KINDS[:2])]


def _bar(got, ref):
    """Worst |got - ref| in units of the plain bar 1e-4 + 1e-4 |ref| (infinities -- open maximum groups -- must coincide and are left out)."""
    g = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    r = ref.detach().cpu().numpy().astype(np.float64) if isinstance(ref, torch.Tensor) else np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(r)
    assert np.array_equal(fin, np.isfinite(g))
    return float((np.abs(g[fin] - r[fin]) / (1e-4 + 1e-4 * np.abs(r[fin]))).max()) if fin.any() else 0.0


def _tables(name):
    spec = district(name)
    return spec, spec.episode_tables(0)


def _prec(f64):
    return 2 if f64 == 'chain' else 0


# ---- 0. the reference side: single steps against the float64 oracle on every district ------------------------------------------------------
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', DISTRICTS)
def test_single_step_path_against_the_oracle(name, kind, f64):
    """`StepEngine.step` (what every comparison below takes as the reference) against `COracle` in float64, K = 48 random actions per env,
    teacher-forced from the oracle's state like test_gpu_parity.py::test_batch_against_c_oracle_distinct_actions, E = 68 (not a multiple of
    the tile), plain bar.  On het17 this is also the first GPU check of a building without a battery (`present=False`) next to batteries in
    a lean district, of an inactive storage action, and of action columns that are not the building index."""
    from oracle.c_oracle import COracle, OS, OO
    from test_gpu_parity import _err, _teach
    spec, tab = _tables(name)
    E, K = 68, 48
    eng, ora = StepEngine(tab, E, reward=kind, f64_maps=f64), COracle(spec, tab, E, reward=kind)
    assert eng.lean and eng.f64_chain == (f64 == 'chain') and eng.n_act_cols == ora.n_act_cols
    low, high = spec.action_limits()
    rng = np.random.RandomState(5)
    worst = {}
    for t in range(K):
        a = rng.uniform(low[:, None], high[:, None], size=(len(low), E)).astype(np.float32)
        a[:, 0] = 0.0
        a[:, 1], a[:, 2] = low, high
        _teach(eng, ora, OS)
        eng.step(torch.from_numpy(a).cuda(), t)
        out, oe = ora.step(a, t)
        for key, got, ref in (('soc', eng.soc, ora.state[:, :, OS['SOC']].T), ('net', eng.net, out[:, :, OO['NET']].T),
                              ('reward', eng.reward_bldg, out[:, :, OO['REWARD']].T), ('d_net', eng.district_net, oe[:, 0]),
                              ('district_reward', eng.district_reward, oe[:, 3])):
            worst[key] = max(worst.get(key, 0.0), _err(got.cpu().numpy(), ref, 1e-4, 1e-4))
    check_worst(worst, f'single steps {name} {kind} f64_maps={f64}')


# ---- 1. cl_rollout_kpi_kernel --------------------------------------------------------------------------------------------------------------
def _kpi_lds_floats(nw, tile):
    """`rollout_kpi_lds_floats` of csrc/cl_rollout.h, with that header's constants."""
    text = (_lib.CSRC / 'cl_rollout.h').read_text()
    s, nb = (int(re.search(rf'constexpr int {k} = (\d+);', text).group(1)) for k in ('CL_RKPI_S', 'CL_RKPI_NB'))
    return s * nw * tile + abi.CLKE_PER_COND * tile + 16 + s * 4 * nb + 5 * nb


@pytest.mark.parametrize('vec', [1, 2])
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('E', [260, 64])
@pytest.mark.parametrize('name,kind', DISTRICT_KINDS)
def test_kpi_rollout_equals_single_steps(name, kind, E, f64, vec):
    """K = 30 open-loop steps from t0 = 0, then a second launch of 27 (it begins in the middle of a day, crosses t = 48 and ends on a partial
    fold of the district series): state, last outputs, district sums, return and every KPI plane against single steps after each launch.
    E = 260: a ragged tile and two env blocks.  The forced instantiation is the one that ran; at 31 / 32 buildings and two envs per lane
    that is a launch whose LDS request (76 480 bytes) has to be opted into -- asserted from the kernel's own formula, so that the case
    cannot stop covering that path unnoticed."""
    spec, tab = _tables(name)
    a = StepEngine(tab, E, reward=kind, kpi=True, f64_maps=f64)
    b = StepEngine(tab, E, reward=kind, kpi=True, f64_maps=f64, tuning=dict(vec=vec))
    assert a.lean and b.lean and a.kpi_shared_baseline and b.f64_chain == (f64 == 'chain')
    nw = (a.n_bldg + 1) // 2
    if name in ('b31', 'b32'):
        assert nw == 16
        if vec == 2:
            assert _kpi_lds_floats(16, 128) * 4 > 65536
    b.trace_kernels()
    ret, ret_ref = torch.zeros(E, device='cuda'), torch.zeros(E, device='cuda')
    worst = {}
    for n, K in enumerate((30, 27)):
        acts = _actions(spec, K, E, 40 + n)
        for k in range(K):
            a.step(acts[k])
            ret_ref += a.district_reward
        _fused(b, K, actions=acts, ret_env=ret)
        assert b.last_kernels == f'cl_rollout_kpi_kernel<{vec}, {_prec(f64)}>', b.last_kernels
        assert a.t == b.t
        for key, got, ref in (('state', b.state, a.state), ('net', b.net, a.net), ('reward', b.reward_bldg, a.reward_bldg),
                              ('out_env', b.out_env, a.out_env), ('return', ret, ret_ref), ('kpi_bldg', b.kpi_bldg, a.kpi_bldg),
                              ('kpi_env', b.kpi_env, a.kpi_env)):
            worst[key] = max(worst.get(key, 0.0), _bar(got, ref))
        print(f'{name} {kind} E={E} f64={f64} vec={vec} after launch {n}:', {k: round(v, 4) for k, v in worst.items()})
        _compare_step_outputs(b, a, ret, ret_ref)
        _compare_kpi_planes(b, a, f'{name} after launch {n} (t = {b.t})')
    record_worst(worst, f'kpi rollout vs single steps {name} {kind} E={E} f64_maps={f64} vec={vec}')
    assert b.t == 57 and float(b.kpi_bldg.abs().sum()) > 0 and float(b.kpi_env[abi.CLKE_DAY_N].min()) == 2.0
    if name == 'het17':
        # the building without a battery never had its state planes written; the one with an idle action kept its battery's losses
        assert torch.equal(b.state[:, HET_UNDRIVEN[0]], a.state[:, HET_UNDRIVEN[0]])


@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('name', SMALL)
def test_kpi_rollout_finalised_kpis(name, f64):
    """`VectorCityLearnEnv(kpi=True)`: `rollout(fused=True)` twice (30 + 27 steps) + `evaluate()` against an env stepped through the same
    actions."""
    from citylearn_amd.vector_env import VectorCityLearnEnv
    spec = district(name)
    E = 64
    mk = lambda: VectorCityLearnEnv(spec, E, kpi=True, reward_function=REWARD_CLASS, f64_maps=f64)
    a, b = mk(), mk()
    b.engine.trace_kernels()
    acts = _actions(spec, 57, E, 3)
    for k in range(30):
        a.step(acts[k])
    b.rollout(30, acts[:30], fused=True)
    assert 'cl_rollout_kpi_kernel' in b.engine.last_kernels and 'cl_step' not in b.engine.last_kernels
    _finalised_close(b.evaluate(), a.evaluate())
    for k in range(30, 57):
        a.step(acts[k])
    b.rollout(27, acts[30:], fused=True)
    assert b.time_step == a.time_step == 57
    _compare_kpi_planes(b.engine, a.engine, name)
    _finalised_close(b.evaluate(), a.evaluate())


@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('name', ['b32', 'het17'])
def test_kpi_rollout_on_device_policy_and_episode_windows(name, f64):
    """test_gpu_rollout_kpi.py::test_episode_offsets_per_env_block on the two districts: three env blocks with their own `env_row0` (640 envs:
    a ragged last block), the Philox policy inside the launch against the launch sequence's policy kernel; every block's baseline sums and
    baseline series land at the block's first env and nowhere else."""
    spec = district(name)
    tab = spec.episode_tables(0)
    E, K, n_steps = 640, 30, 200
    row0 = [0, 300, 77]
    kw = dict(kpi=True, n_steps=n_steps, env_row0=row0, f64_maps=f64)
    a, b = StepEngine(tab, E, **kw), StepEngine(tab, E, **kw)
    b.trace_kernels()
    low, high = spec.action_limits()
    for e in (a, b):
        e.set_action_limits(low, high)
    a.rollout(K, seed=5)                                  # the launch sequence = single steps bit for bit
    _fused(b, K, seed=5)
    record_worst({'state': _bar(b.state, a.state), 'kpi_bldg': _bar(b.kpi_bldg, a.kpi_bldg), 'kpi_env': _bar(b.kpi_env, a.kpi_env)},
                 f'kpi rollout, on-device policy + windows {name} f64_maps={f64}')
    torch.testing.assert_close(b.state, a.state, rtol=2e-5, atol=2e-5)
    _compare_kpi_planes(b, a)
    first = torch.zeros(E, dtype=torch.bool, device='cuda')
    first[::abi.CL_ROW0_BLOCK] = True
    base = b.kpi_bldg[abi.CLK_B_NET]
    assert bool((base[:, first] != 0).all()) and bool((base[:, ~first] == 0).all())
    assert bool((b.kpi_env[abi.CLKE_PER_COND + abi.CLKE_PREV][first] != 0).all()) and bool((b.kpi_env[abi.CLKE_PER_COND + abi.CLKE_PREV][~first] == 0).all())
    assert len({float(base[0, i]) for i in (0, 256, 512)}) == 3
    # the last building's five sums (lane n_bldg - 1 of the owner wave: the end of the [32] rows at 32 buildings) are its own
    torch.testing.assert_close(b.kpi_bldg[abi.CLK_EXPECTED_ALL, -1], a.kpi_bldg[abi.CLK_EXPECTED_ALL, -1], rtol=1e-4, atol=1e-3)
    assert float(b.kpi_bldg[abi.CLK_EXPECTED_ALL, -1, 0]) > 0


# ---- 2. cl_rollout_policy_kernel -----------------------------------------------------------------------------------------------------------
def _policy_setup(name, E, f64, kind='RewardFunction', H=16, sigma=None, vec=None, **kw):
    spec, tab = _tables(name)
    layout = ObservationLayout(spec, 'current', True)
    pol = make_policy(layout, H, seed=H, sigma=sigma)
    pt = pol.pack(layout, tab, device='cuda:0')
    tuning = {**({'vec': vec} if vec else {}), **kw.pop('tuning', {})}
    eng = StepEngine(tab, E, reward=kind, f64_maps=f64, tuning=tuning or None, **kw)
    assert eng.lean
    eng.trace_kernels()
    return spec, tab, layout, pol, pt, eng


def _step_actions(eng, pt, plane):
    """The action tensor `step()` takes, from a recorded action plane [n_bldg, E]: building b's action goes to ITS column (`pt.es_cols`;
    in het17 column b is not building b), a building without a column has none."""
    es = torch.as_tensor(pt.es_cols, device=plane.device)
    acts = torch.zeros((eng.n_act_cols, plane.shape[1]), device=plane.device)
    acts[es[es >= 0]] = plane[es >= 0]
    return acts


@pytest.mark.parametrize('sigma', [None, 0.1])
@pytest.mark.parametrize('H', [4, 32])
@pytest.mark.parametrize('vec', [1, 2])
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('name', DISTRICTS)
def test_policy_teacher_forced_actions(name, f64, vec, H, sigma):
    """(a) of test_gpu_policy_rollout.py on every district: each recorded action recomputed in float64 from the recorded inputs; gate
    4 x a float32 torch evaluation's deviation.  het17: the two buildings without a storage action record action 0 exactly, and their soc
    plane is the single-step path's (the battery that idles keeps its losses; the absent one stays where reset put it); the building with the
    shorter observation vector is fed the zero-padded vector (`HostObservations`)."""
    E, K = 260, 24
    spec, tab, layout, pol, pt, eng = _policy_setup(name, E, f64, H=H, sigma=sigma, vec=vec)
    _, traj = _roll(eng, pt, K, seed=11)
    assert eng.last_kernels == f'cl_rollout_policy_kernel<{vec}, {_prec(f64)}>', eng.last_kernels
    if name == 'het17':
        undriven = list(HET_UNDRIVEN)
        assert np.array_equal(np.nonzero(pt.es_cols < 0)[0], sorted(undriven))
        assert bool((traj[:, A, undriven] == 0).all())
        ref = StepEngine(tab, E, f64_maps=f64)
        for k in range(K):
            ref.step(_step_actions(ref, pt, traj[k, A]))
            assert torch.equal(traj[k, S, undriven], ref.soc[undriven]), k
        assert torch.equal(eng.state[:, undriven], ref.state[:, undriven])
        # the driven buildings' actions reach the bounds' interior: the policy does something
        assert float(traj[:, A].abs().max()) > 0.05
    # (the recomputation masks the undriven buildings: their reference action is the MLP's, their recorded one 0 by construction)
    drv = np.nonzero(pt.es_cols >= 0)[0]
    dev_kernel, dev_f32 = _teacher_forced_driven(eng, tab, layout, pol, pt, traj, drv, seed=11)
    print(f'teacher-forced {name} vec={vec} f64={f64} H={H} sigma={sigma}: kernel {dev_kernel:.3e}  float32 torch {dev_f32:.3e}  ratio {dev_kernel / dev_f32:.2f}')
    record_worst({'kernel': dev_kernel, 'float32_torch': dev_f32, 'ratio': dev_kernel / dev_f32},
                 f'teacher-forced {name} f64_maps={f64} vec={vec} H={H} sigma={sigma}')
    assert dev_f32 > 0 and dev_kernel <= 4.0 * dev_f32, (dev_kernel, dev_f32)


def _teacher_forced_driven(eng, tab, layout, pol, pt, traj, drv, seed=0):
    """`_teacher_forced` where every building is driven; otherwise its recomputation for the driven buildings `drv` alone (an undriven
    building has no action column, hence no noise stream, and its MLP output is not an action of the rollout): the same float64 reference
    and float32 torch evaluation (`actions_host`, `f32_torch_deviation`) over those buildings' weights, inputs and bounds."""
    if len(drv) == eng.n_bldg:
        return _teacher_forced(eng, tab, layout, pol, pt, traj, seed=seed)
    from types import SimpleNamespace
    K, E = traj.shape[0], traj.shape[3]
    hobs = HostObservations(layout, tab)
    tr = traj.cpu().numpy().astype(np.float64)
    x = np.stack([hobs.at(0, np.zeros((eng.n_bldg, E)), None, reset=True)] + [hobs.at(k, tr[k - 1, S], tr[k - 1, N]) for k in range(1, K)])[:, :, drv]
    z = None
    if np.any(pt.sigma_bldg > 0):
        z = np.stack([np.stack([policy.noise_host(seed, np.arange(E), pt.es_cols[b], k) for b in drv], axis=1) for k in range(K)])
    sub = policy.MLPPolicy(pol.w1[:, drv], pol.b1[:, drv], pol.w2[:, drv], pol.b2[:, drv])
    bounds = SimpleNamespace(low_bldg=pt.low_bldg[drv], high_bldg=pt.high_bldg[drv], sigma_bldg=pt.sigma_bldg[drv])
    ref = sub.actions_host(x, noise=z, tables=bounds)                                 # [K, E, driven]
    dev_kernel = float(np.abs(tr[:, A][:, drv].transpose(0, 2, 1) - ref).max())
    return dev_kernel, f32_torch_deviation(sub, x, bounds, device='cuda', noise=z)


@pytest.mark.parametrize('vec', [1, 2])
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('kind', ['MARL', 'RewardFunction'])
@pytest.mark.parametrize('name', DISTRICTS)
def test_policy_replay_through_single_steps(name, kind, f64, vec):
    """(b): the recorded actions fed step by step to a second engine's `step()` through the buildings' own action columns: state, last
    outputs, district sums, return and the trajectory planes at (b)'s tolerances; E = 260."""
    E, K = 260, 30
    spec, tab, layout, pol, pt, eng = _policy_setup(name, E, f64, kind, sigma=0.1, vec=vec)
    ret, traj = _roll(eng, pt, K, seed=5)
    assert eng.last_kernels == f'cl_rollout_policy_kernel<{vec}, {_prec(f64)}>', eng.last_kernels
    ref = StepEngine(tab, E, reward=kind, f64_maps=f64)
    ret_ref = torch.zeros(E, device='cuda')
    worst = {}
    for k in range(K):
        ref.step(_step_actions(ref, pt, traj[k, A]))
        ret_ref += ref.district_reward
        for key, got, want in (('soc', traj[k, S], ref.soc), ('net', traj[k, N], ref.net), ('reward', traj[k, R], ref.reward_bldg)):
            worst[key] = max(worst.get(key, 0.0), _bar(got, want))
        torch.testing.assert_close(traj[k, S], ref.soc, rtol=2e-6, atol=2e-6)
        torch.testing.assert_close(traj[k, N], ref.net, rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(traj[k, R], ref.reward_bldg, rtol=2e-5, atol=2e-5)
    worst.update(state=_bar(eng.state, ref.state), out_env=_bar(eng.out_env, ref.out_env), **{'return': _bar(ret, ret_ref)})
    print(f'replay {name} {kind} f64={f64} vec={vec}:', {k: round(v, 4) for k, v in worst.items()})
    record_worst(worst, f'policy rollout vs single steps {name} {kind} f64_maps={f64} vec={vec}')
    torch.testing.assert_close(eng.state, ref.state, rtol=2e-6, atol=2e-6)
    torch.testing.assert_close(eng.out_bldg[:2], ref.out_bldg[:2], rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(eng.out_env, ref.out_env, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(ret, ret_ref, rtol=1e-5, atol=1e-3)
    assert eng.t == K and torch.equal(traj[K - 1, N], eng.net) and torch.equal(traj[K - 1, S], eng.soc) and torch.equal(traj[K - 1, R], eng.reward_bldg)


@pytest.mark.parametrize('vec', [1, 2])
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('kind', ['RewardFunction', 'MARL'])
@pytest.mark.parametrize('name', DISTRICTS)
def test_policy_free_running_against_the_cpu(name, kind, f64, vec):
    """(c): K = 48 from reset, the host loop of `COracle.step` + `actions_host` (float64, zero-padded observation vectors) against one launch at
    the plain bar on soc, degraded capacity, net, reward and district net.  The loop's conditioning on b1, b32 and het17 is
    tests/test_policy_host.py::test_closed_loop_is_well_conditioned_on_the_geometry_districts."""
    E, K = 64, 48
    spec, tab, layout, pol, pt, eng = _policy_setup(name, E, f64, kind, H=16, vec=vec)
    want = host_closed_loop(spec, tab, layout, pol, pt, K, E, reward=kind)
    _, traj = _roll(eng, pt, K)
    assert eng.last_kernels == f'cl_rollout_policy_kernel<{vec}, {_prec(f64)}>', eng.last_kernels
    tr = traj.cpu().numpy().astype(np.float64)
    bar = lambda got, ref: float((np.abs(got - ref) / (1e-4 + 1e-4 * np.abs(ref))).max())
    worst = {'soc': bar(tr[:, S], want['soc']), 'net': bar(tr[:, N], want['net']), 'reward': bar(tr[:, R], want['reward']),
             'district_net': bar(tr[:, N].sum(axis=1), want['dnet']),
             'degraded_capacity': bar(eng.degraded_capacity.cpu().numpy(), want['degcap'][-1])}
    print(f'free-running {name} {kind} f64={f64} vec={vec}:', {k: round(v, 4) for k, v in worst.items()})
    check_worst(worst, f'policy rollout free-running {name} {kind} f64_maps={f64} vec={vec}')


@pytest.mark.parametrize('vec', [1, 2])
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('name', SMALL)
def test_policy_split_launches_are_bit_identical(name, f64, vec):
    """(d): launches of 1, 5, 24 and 25 steps from t0 = 0 equal one 55-step launch bit for bit: state, outputs, trajectory; MARL, noise on."""
    E = 320
    spec, tab, layout, pol, pt, one = _policy_setup(name, E, f64, 'MARL', sigma=0.1, vec=vec)
    ret1, traj1 = _roll(one, pt, 55, seed=3)
    eng = StepEngine(tab, E, reward='MARL', f64_maps=f64, tuning=dict(vec=vec))
    eng.trace_kernels()
    ret, parts = torch.zeros(E, device='cuda'), []
    for K in (1, 5, 24, 25):
        traj = torch.empty((K, policy.CLPOL_NT, eng.n_bldg, E), device='cuda')
        eng.rollout_policy(K, pt, seed=3, ret_env=ret, traj=traj)
        assert eng.last_kernels == f'cl_rollout_policy_kernel<{vec}, {_prec(f64)}>'
        parts.append(traj)
    assert eng.t == 55 and torch.equal(torch.cat(parts), traj1)
    assert torch.equal(eng.state, one.state) and torch.equal(eng.out_bldg[:2], one.out_bldg[:2]) and torch.equal(eng.out_env, one.out_env)
    torch.testing.assert_close(ret, ret1, rtol=1e-6, atol=1e-4)               # (four partial sums instead of one)


# ---- 3. an `nw` above the default ----------------------------------------------------------------------------------------------------------
NW_CASES = [('g2022_all', 16), ('b2', 2)]


@pytest.mark.parametrize('vec', [1, 2])
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('kind', ['RewardFunction', 'MARL'])
@pytest.mark.parametrize('name,nw', NW_CASES)
def test_nw_override_kpi_rollout(name, nw, kind, f64, vec):
    """`tuning=dict(nw=..)` above the default split (17 buildings on 16 waves: the series owners move to wave 15 and waves 1 .. 15 own one
    building each; 2 buildings on 2 waves) against the same engine at the default `nw`.  What belongs to ONE building does not depend on the
    split and is compared bit for bit: state, net, the per-building KPI sums, the env block's baseline sums and baseline series (folded in
    building order).  The district sums are added in WAVE order, which follows the building order only at the default split: `out_env`, the
    return, the control district series of `kpi_env` and -- under MARL, whose per-building reward reads the district net -- the reward plane
    are compared at `_compare_step_outputs` / `_compare_kpi_planes`' tolerances instead."""
    spec, tab = _tables(name)
    E = 260
    a = StepEngine(tab, E, reward=kind, kpi=True, f64_maps=f64, tuning=dict(vec=vec))
    b = StepEngine(tab, E, reward=kind, kpi=True, f64_maps=f64, tuning=dict(vec=vec, nw=nw))
    assert nw > (a.n_bldg + 1) // 2 and nw <= a.n_bldg
    a.trace_kernels(), b.trace_kernels()
    ra, rb = torch.zeros(E, device='cuda'), torch.zeros(E, device='cuda')
    for n, K in enumerate((30, 27)):
        acts = _actions(spec, K, E, 60 + n)
        for e, r in ((a, ra), (b, rb)):
            _fused(e, K, actions=acts, ret_env=r)
            assert e.last_kernels == f'cl_rollout_kpi_kernel<{vec}, {_prec(f64)}>'
        assert torch.equal(b.state, a.state) and torch.equal(b.net, a.net) and torch.equal(b.kpi_bldg, a.kpi_bldg)
        assert torch.equal(b.kpi_env[abi.CLKE_PER_COND:], a.kpi_env[abi.CLKE_PER_COND:])
        if kind != 'MARL':
            assert torch.equal(b.reward_bldg, a.reward_bldg)
        _compare_step_outputs(b, a, rb, ra)
        _compare_kpi_planes(b, a, f'{name} nw={nw} after launch {n}')


@pytest.mark.parametrize('vec', [1, 2])
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('kind', ['RewardFunction', 'MARL'])
@pytest.mark.parametrize('name,nw', NW_CASES)
def test_nw_override_policy_rollout(name, nw, kind, f64, vec):
    """The same override on the policy kernel (noise on): state, the action / net / soc planes of the trajectory and the last net bit for bit
    (the policy reads soc and net, never the reward); the reward planes bit for bit unless MARL couples them through the wave-ordered district
    net; `out_env` and the return at `_compare_step_outputs`' tolerances (see test_nw_override_kpi_rollout)."""
    E, K = 260, 55
    spec, tab, layout, pol, pt, a = _policy_setup(name, E, f64, kind, sigma=0.1, vec=vec)
    b = StepEngine(tab, E, reward=kind, f64_maps=f64, tuning=dict(vec=vec, nw=nw))
    b.trace_kernels()
    (ra, ta), (rb, tb) = _roll(a, pt, K, seed=7), _roll(b, pt, K, seed=7)
    assert a.last_kernels == b.last_kernels == f'cl_rollout_policy_kernel<{vec}, {_prec(f64)}>'
    assert torch.equal(b.state, a.state) and torch.equal(b.net, a.net)
    for plane in (A, N, S):
        assert torch.equal(tb[:, plane], ta[:, plane]), plane
    if kind != 'MARL':
        assert torch.equal(tb[:, R], ta[:, R]) and torch.equal(b.reward_bldg, a.reward_bldg)
    torch.testing.assert_close(tb[:, R], ta[:, R], rtol=2e-5, atol=2e-5)
    _compare_step_outputs(b, a, rb, ra)
