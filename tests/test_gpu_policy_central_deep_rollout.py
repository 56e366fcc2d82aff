"""The closed-loop rollout under a central-agent policy with TWO hidden layers on the GPU (`StepEngine.rollout_policy` /
`VectorCityLearnEnv.rollout_policy` with a `policy.DeepCentralMLPPolicy`: one launch of `cl_rollout_policy_central_deep_kernel`,
csrc/cl_policy_central.h at DEEP = true), in tests/test_gpu_policy_central_rollout.py's six groups: (1) its actions teacher-forced against the float64 MLP
over the recorded planes of ALL buildings, (2) its record replayed through `step()`, MARL included, (3) free-running against the CPU oracle,
(4) launch splitting, checkpoints, episode windows x parameter sets x env offsets and the wave count bit for bit, (5) the env-level call against
`capture_rollout` with the same MLP in torch, (6) the refusals.  Weights: tests/policy_central_deep_util.py (their scale fixed by
tests/test_policy_central_deep_host.py's conditioning test)."""
import numpy as np
import pytest
import torch

from golden_util import check_worst, golden, record_worst
from citylearn_amd import _lib, policy
from citylearn_amd.engine import StepEngine
from district_util import HET_UNDRIVEN, district
from policy_central_deep_util import CentralObservations, central_layout, f32_torch_deviation, host_closed_loop, make_deep_central_policy

pytestmark = pytest.mark.gpu

KINDS = ['RewardFunction', 'MARL', 'IndependentSACReward', 'SolarPenaltyReward']     # every lean reward kind
A, R, N, S = policy.CLPOL_T_ACTION, policy.CLPOL_T_REWARD, policy.CLPOL_T_NET, policy.CLPOL_T_SOC
F64 = ['chain', False]
NAMES6 = ('w1', 'b1', 'w2', 'b2', 'w3', 'b3')


def _setup(name, E, f64='chain', kind='RewardFunction', H=(16, 16), sigma=None, n_sets=1, set_of_block=None, seed=None, **kw):
    spec = district(name)
    tab = spec.episode_tables(0)
    layout = central_layout(spec)
    pol = make_deep_central_policy(layout, *H, n_sets=n_sets, seed=sum(H) if seed is None else seed, sigma=sigma)
    pt = pol.pack(layout, tab, device='cuda:0', set_of_block=set_of_block)
    eng = StepEngine(tab, E, reward=kind, f64_maps=f64, **kw)
    eng.trace_kernels()
    return spec, tab, layout, pol, pt, eng


def _roll(eng, pt, K, seed=0):
    ret = torch.zeros(eng.n_env, device='cuda')
    traj = torch.full((K, policy.CLPOL_NT, eng.n_bldg, eng.n_env), float('nan'), device='cuda')
    eng.rollout_policy(K, pt, seed=seed, ret_env=ret, traj=traj)
    assert not torch.isnan(traj).any()
    assert eng.last_kernels.startswith(f'cl_rollout_policy_central_deep_kernel<{2 if eng.f64_chain else 0}'), eng.last_kernels
    return ret, traj


def _teacher_forced(eng, tab, layout, pol, pt, traj, seed=0, row0=0, env_offset=0):
    """(kernel's worst |action - float64 MLP| over the driven buildings, a float32 torch evaluation's, on the recorded planes of all buildings of
    every step); the undriven buildings' action plane must be 0."""
    K, E = traj.shape[0], traj.shape[3]
    cobs = CentralObservations(layout, tab)
    tr = traj.cpu().numpy().astype(np.float64)
    x = np.stack([cobs.at(row0, reset=True, E=E)] + [cobs.at(row0 + k, tr[k - 1, S], tr[k - 1, N]) for k in range(1, K)])
    z = None
    sig, es = pt.sigma_bldg, pt.es_cols
    if np.any(sig > 0):
        z = np.stack([np.stack([policy.noise_host(seed, env_offset + np.arange(E), es[b], k) if es[b] >= 0 else np.zeros(E) for b in range(eng.n_bldg)], axis=1)
                      for k in range(K)])
    ref = pol.actions_host(x, noise=z, tables=pt)                                     # [K, E, B]
    got = tr[:, A].transpose(0, 2, 1)
    assert np.all(got[:, :, es < 0] == 0.0)
    return float(np.abs(got - ref)[:, :, es >= 0].max()), f32_torch_deviation(pol, x, pt, device='cuda', noise=z)


# ---- 1. teacher-forced actions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sigma', [0.1, None])
@pytest.mark.parametrize('f64', F64)
@pytest.mark.parametrize('name', ['g2022_all', 'het17', 'b1', 'b2', 'b31', 'b32'])
@pytest.mark.parametrize('H', [(4, 4), (32, 32), (64, 64), (4, 64), (64, 4)])
def test_1_teacher_forced_actions(H, name, f64, sigma):
    """(1) Every recorded action recomputed in float64 from the recorded soc / net planes of ALL buildings (the step before; the reset observation
    at step 0; the noise replayed from the Philox stream), E = 260: a ragged last tile and two env blocks.  Gate: 4 x the worst deviation of a
    float32 torch evaluation of the same MLP on the same inputs -- the project's gate for its policy kernels, measured here.  b1 is the one-wave
    workgroup whose wave owns every group of both layers; b32 at H2 = 4 leaves fifteen waves without a layer-2 group, which still cross the
    barrier behind it.  The figures are printed and recorded (profiles/policy_central_deep_parity.md)."""
    spec, tab, layout, pol, pt, eng = _setup(name, 260, f64, H=H, sigma=sigma)
    _, traj = _roll(eng, pt, 24, seed=11)
    dev_kernel, dev_f32 = _teacher_forced(eng, tab, layout, pol, pt, traj, seed=11)
    if name == 'het17':
        assert sorted(np.nonzero(pt.es_cols < 0)[0]) == sorted(HET_UNDRIVEN)
    tag = f'{name} f64={f64} H={H[0]}x{H[1]} sigma={sigma}'
    print(f'teacher-forced {tag}: kernel {dev_kernel:.3e}  float32 torch {dev_f32:.3e}  ratio {dev_kernel / dev_f32:.2f}')
    record_worst({'kernel': dev_kernel, 'float32_torch': dev_f32, 'ratio': dev_kernel / dev_f32}, f'deep central teacher-forced {tag}', 4.0)
    assert dev_f32 > 0 and dev_kernel <= 4.0 * dev_f32, (dev_kernel, dev_f32)


# ---- 2. replay ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', F64)
@pytest.mark.parametrize('name', ['g2022_all', 'het17'])
@pytest.mark.parametrize('kind', KINDS)
def test_2_replay_through_single_steps(kind, name, f64):
    """(2) The recorded actions fed step by step to a second engine's `step()`: state, last outputs, district sums, return and the record's planes
    at the tolerances of tests/test_gpu_policy_central_rollout.py::test_2, for every lean reward kind -- MARL rides on the step's third barrier.
    The undriven buildings' action plane is 0."""
    E, K = 260, 30
    spec, tab, layout, pol, pt, eng = _setup(name, E, f64, kind, H=(32, 24), sigma=0.1)
    ret, traj = _roll(eng, pt, K, seed=5)
    assert bool((traj[:, A][:, torch.as_tensor(pt.es_cols < 0)] == 0).all())
    acts = torch.zeros((K, eng.n_act_cols, E), device='cuda')
    driven = np.nonzero(pt.es_cols >= 0)[0]
    acts[:, torch.as_tensor(pt.es_cols[driven])] = traj[:, A][:, torch.as_tensor(driven)]
    ref = StepEngine(tab, E, reward=kind, f64_maps=f64)
    ret_ref = torch.zeros(E, device='cuda')
    for k in range(K):
        ref.step(acts[k])
        ret_ref += ref.district_reward
        torch.testing.assert_close(traj[k, S], ref.soc, rtol=2e-6, atol=2e-6)
        torch.testing.assert_close(traj[k, N], ref.net, rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(traj[k, R], ref.reward_bldg, rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(eng.state, ref.state, rtol=2e-6, atol=2e-6)
    torch.testing.assert_close(eng.out_bldg[:2], ref.out_bldg[:2], rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(eng.out_env, ref.out_env, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(ret, ret_ref, rtol=1e-5, atol=1e-3)
    assert eng.t == K and torch.equal(traj[K - 1, N], eng.net) and torch.equal(traj[K - 1, S], eng.soc) and torch.equal(traj[K - 1, R], eng.reward_bldg)


# ---- 3. free-running ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', F64)
@pytest.mark.parametrize('H', [(4, 4), (32, 32), (64, 64), (64, 4)])
@pytest.mark.parametrize('name', ['g2022_all', 'het17', 'b1', 'b32'])
def test_3_free_running_against_the_cpu(name, H, f64):
    """(3) K = 48 from reset: the host loop of `COracle.step` + `actions_host` (float64) against one launch, at the plain bar 1e-4 + 1e-4 |ref|
    on soc, degraded capacity, net, reward and district net -- the policies of the CPU conditioning test (test_policy_central_deep_host.py),
    under which the loop stays within 0.1 x the bar when perturbed by the full teacher-forced tolerance."""
    E, K = 64, 48
    spec, tab, layout, pol, pt, eng = _setup(name, E, f64, H=H)
    want = host_closed_loop(spec, tab, layout, pol, pt, K, E)
    _, traj = _roll(eng, pt, K)
    tr = traj.cpu().numpy().astype(np.float64)
    bar = lambda got, ref: float((np.abs(got - ref) / (1e-4 + 1e-4 * np.abs(ref))).max())
    worst = {'soc': bar(tr[:, S], want['soc']), 'net': bar(tr[:, N], want['net']), 'reward': bar(tr[:, R], want['reward']),
             'district_net': bar(tr[:, N].sum(axis=1), want['dnet']),
             'degraded_capacity': bar(eng.degraded_capacity.cpu().numpy(), want['degcap'][-1])}
    print(f'free-running {name} H={H} f64={f64}:', {k: round(v, 4) for k, v in worst.items()})
    check_worst(worst, f'deep central policy rollout {name} H={H[0]}x{H[1]} f64={f64}')


# ---- 4. bit for bit ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', F64)
def test_4a_split_launches_and_checkpoint_are_bit_identical(f64):
    """(4) Launches of 1, 5, 24 and 25 steps from t0 = 0 equal one 55-step launch bit for bit (the previous net of EVERY building travels through
    out_bldg into X, t == 0 uses net_reset), with a checkpoint restored into a fresh engine between two of them; MARL, noise on, a ragged tile."""
    E = 260
    spec, tab, layout, pol, pt, one = _setup('g2022_all', E, f64, 'MARL', H=(24, 40), sigma=0.1)
    ret1, traj1 = _roll(one, pt, 55, seed=3)
    eng = StepEngine(tab, E, reward='MARL', f64_maps=f64)
    ret, parts = torch.zeros(E, device='cuda'), []
    for n, K in enumerate((1, 5, 24, 25)):
        if n == 2:
            sd = eng.state_dict()
            eng = StepEngine(tab, E, reward='MARL', f64_maps=f64)
            eng.load_state_dict(sd)
        traj = torch.empty((K, policy.CLPOL_NT, eng.n_bldg, E), device='cuda')
        eng.rollout_policy(K, pt, seed=3, ret_env=ret, traj=traj)
        parts.append(traj)
    assert eng.t == 55 and torch.equal(torch.cat(parts), traj1)
    assert torch.equal(eng.state, one.state) and torch.equal(eng.out_bldg[:2], one.out_bldg[:2]) and torch.equal(eng.out_env, one.out_env)
    torch.testing.assert_close(ret, ret1, rtol=1e-6, atol=1e-4)               # (four partial sums instead of one)


@pytest.mark.parametrize('f64', F64)
def test_4b_windows_sets_and_env_offsets(f64):
    """(4) Two env blocks with different episode windows AND different parameter sets in one launch: each block equals, bit for bit, an engine
    of its own with that window, that set and its env offset (noise on: the half batches reproduce the whole batch's streams)."""
    spec = district('g2022_all')
    tab = spec.episode_tables(0)
    layout = central_layout(spec)
    pol = make_deep_central_policy(layout, 16, 8, n_sets=2, seed=2, sigma=0.1)
    K, n_steps, rows = 24, 200, [0, 131]
    whole = StepEngine(tab, 512, f64_maps=f64, n_steps=n_steps, env_row0=rows)
    whole.trace_kernels()
    _, traj = _roll(whole, pol.pack(layout, tab, device='cuda:0', set_of_block=[0, 1]), K, seed=9)
    assert not torch.equal(traj[:, A, :, :256], traj[:, A, :, 256:])
    for g in range(2):
        part = StepEngine(tab, 256, f64_maps=f64, n_steps=n_steps, env_row0=[rows[g]], env_offset=256 * g)
        part.trace_kernels()
        _, tr = _roll(part, pol.pack(layout, tab, device='cuda:0', set_of_block=[g]), K, seed=9)
        sl = slice(256 * g, 256 * (g + 1))
        assert torch.equal(tr, traj[:, :, :, sl]), g
        assert torch.equal(part.state, whole.state[:, :, sl]) and torch.equal(part.out_env, whole.out_env[:, sl])
    # ... and the actions of block 1 are its window's and its set's (layer 2 included): teacher-forced like (1)
    single = policy.DeepCentralMLPPolicy(*(getattr(pol, n)[1:2] for n in NAMES6), sigma=0.1)
    dev_kernel, dev_f32 = _teacher_forced(whole, tab, layout, single, single.pack(layout, tab), traj[:, :, :, 256:], seed=9, row0=rows[1], env_offset=256)
    print(f'window 1 / set 1 teacher-forced: kernel {dev_kernel:.3e}  float32 torch {dev_f32:.3e}')
    assert dev_kernel <= 4.0 * dev_f32


@pytest.mark.parametrize('kind', ['MARL', 'RewardFunction'])
@pytest.mark.parametrize('name,H,nws', [('g2022_all', (32, 32), (9, 12, 16)), ('g2022_all', (64, 64), (9, 12, 16)), ('b2', (8, 12), (1, 2)),
                                        ('b31', (64, 4), (16,)), ('het17', (4, 64), (9, 16))])
def test_4c_the_wave_count_changes_no_action(name, H, nws, kind):
    """(4) `tuning=dict(nw=...)` deals the groups of BOTH hidden layers and the buildings to the waves differently; every sum that feeds an action
    has a fixed order, so the action / net / soc planes and the state are bit-identical to the default geometry's.  The reward plane, the
    district sums and the returns, whose fold order follows nw, are held at (2)'s tolerances."""
    E, K = 260, 20
    spec, tab, layout, pol, pt, base = _setup(name, E, 'chain', kind, H=H, sigma=0.1)
    ret0, traj0 = _roll(base, pt, K, seed=4)
    for nw in nws:
        eng = StepEngine(tab, E, reward=kind, f64_maps='chain', tuning=dict(nw=nw))
        eng.trace_kernels()
        ret, traj = _roll(eng, pt, K, seed=4)
        for p in (A, N, S):
            assert torch.equal(traj[:, p], traj0[:, p]), (nw, p)
        assert torch.equal(eng.state, base.state) and torch.equal(eng.out_bldg[0], base.out_bldg[0])
        torch.testing.assert_close(traj[:, R], traj0[:, R], rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(eng.out_env, base.out_env, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(ret, ret0, rtol=1e-5, atol=1e-3)


def test_4d_return_accumulates_and_a_zero_step_launch_changes_nothing():
    """(4) `ret_env` is accumulated, not overwritten; a 0-step launch leaves state, outputs, district sums and return what they were."""
    E = 260
    spec, tab, layout, pol, pt, eng = _setup('g2022_all', E, H=(8, 12))
    ret = torch.full((E,), 5.0, device='cuda')
    eng.rollout_policy(6, pt, ret_env=ret)
    fresh = StepEngine(tab, E)
    ret0 = torch.zeros(E, device='cuda')
    fresh.rollout_policy(6, pt, ret_env=ret0)
    assert torch.equal(ret, ret0 + 5.0) or torch.allclose(ret, ret0 + 5.0, rtol=1e-6, atol=1e-5)
    assert float((ret - 5.0).abs().max()) > 0
    before = [x.clone() for x in (eng.state, eng.out_bldg, eng._out_env, ret)]
    eng.rollout_policy(0, pt, ret_env=ret)
    torch.cuda.synchronize()
    assert eng.t == 6 and all(torch.equal(x, was) for x, was in zip((eng.state, eng.out_bldg, eng._out_env, ret), before))


# ---- 5. env level ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('normalize', [True, False])
def test_5_env_level_equals_capture_rollout_with_the_torch_mlp(normalize):
    """(5) `VectorCityLearnEnv(..., central_agent=True).rollout_policy(deep central, K, record=True)` against `capture_rollout` driven by its
    `torch_policy`: the tolerance is built as tests/test_gpu_policy_central_rollout.py::test_5 builds it -- the teacher-forced tolerance (4 x a
    float32 evaluation's deviation, measured here on the recorded inputs), once more for the float32 torch policy's own deviation, widened by
    what the two paths' state tolerance (2e-6 on soc, 2e-5 on net, relative + absolute) can move an action through ALL buildings' inputs and
    both hidden layers: da_b = half_b sum_i |w3[b][i]| sum_j |W2[i][j]| sum_b' (|W1[j][soc_b']| scale tol_soc + |W1[j][net_b']| scale tol_net)
    (tanh' <= 1 in every layer); returns at rtol 1e-5 / atol 1e-3.  An env built with central_agent=False raises ValueError."""
    from citylearn_amd.vector_env import VectorCityLearnEnv
    g = golden('g2022_all')
    E, K = 256, 24
    a, b = (VectorCityLearnEnv(g.schema_path, E, observations='tensor', normalize_observations=normalize, central_agent=True) for _ in range(2))
    assert a.central_agent and a.layout.central_agent
    a.engine.trace_kernels()
    pol = make_deep_central_policy(a.layout, 32, 24, seed=4)
    ret, traj = a.rollout_policy(pol, K, record=True)
    assert a._t == K == a.engine.t and a.engine.last_kernels.startswith('cl_rollout_policy_central_deep_kernel<'), a.engine.last_kernels
    pt_host = pol.pack(a.layout, a.tables)                                     # (host copy: bounds, columns, sigmas for the reference)
    f = pol.torch_policy(b.layout, b.tables, b.device)
    acts = torch.zeros((K, b.n_act_cols, E), device='cuda')

    def recorded(obs, i):
        acts[i].copy_(f(obs, i))
        return acts[i]
    cap = b.capture_rollout(recorded, K)
    _, rewards, _ = cap.run()
    torch.cuda.synchronize()
    dev_kernel, dev_f32 = _teacher_forced(a.engine, a.tables, a.layout, pol, pt_host, traj)
    cobs = CentralObservations(a.layout, a.tables)
    w1, _, w2, _, w3, _ = (v[0] for v in pol._full(a.n_bldg))                    # [H1, n_cols], [H2, H1], [B, H2]
    tr = traj.cpu().numpy().astype(np.float64)
    tol_soc, tol_net = 2e-6 * (1 + np.abs(tr[:, S]).max()), 2e-5 * (1 + np.abs(tr[:, N]).max())
    g_soc = np.abs(w1 * np.where(cobs.is_term[0], cobs.scale, 0.0)[None, :]).sum(axis=1)         # [H1]: over all buildings' soc columns
    g_net = np.abs(w1 * np.where(cobs.is_term[1], cobs.scale, 0.0)[None, :]).sum(axis=1)
    d_h2 = np.abs(w2) @ (g_soc * tol_soc + g_net * tol_net)                                        # [H2]
    half = 0.5 * (pt_host.high_bldg - pt_host.low_bldg)
    widen = float((half * (np.abs(w3) @ d_h2)).max())
    tol = 4.0 * dev_f32 + dev_f32 + widen
    es = torch.as_tensor(pt_host.es_cols)
    worst = float((traj[:, A] - acts[:, es]).abs().max())
    print(f'env level normalize={normalize}: |action difference| {worst:.3e}, tolerance {tol:.3e} (float32 deviation {dev_f32:.3e}, state term {widen:.3e}); '
          f'kernel teacher-forced {dev_kernel:.3e}')
    assert worst <= tol and dev_kernel <= 4.0 * dev_f32
    torch.testing.assert_close(ret, rewards.sum(dim=0) if rewards.dim() == 2 else rewards.sum(dim=(0, 1)), rtol=1e-5, atol=1e-3)
    torch.testing.assert_close(a.engine.state, b.engine.state, rtol=2e-6, atol=2e-6)
    with pytest.raises(NotImplementedError, match='a central-agent policy has no KPI kernel.*record=True.*kpi=True'):
        a.rollout_policy(pol, 2, kpi=True)
    # the per-building env's observation tensor is not the vector the weights are defined over
    c = VectorCityLearnEnv(g.schema_path, E, observations='tensor', normalize_observations=normalize, central_agent=False)
    state = c.engine.state.clone()
    with pytest.raises(ValueError, match='a DeepCentralMLPPolicy needs an env built with central_agent=True'):
        c.rollout_policy(pol, K)
    assert c._t == 0 and torch.equal(c.engine.state, state)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def test_6_refusals_leave_every_plane_untouched():
    """A thermal district (foreign tables: `ValueError`; tables of its own shape: the library's CLD_LEAN refusal), 33 buildings, a `kpi=True`
    engine, `f64_maps=True`, two envs per lane, a bad wave count (the library's refusals, by name), `kpi=True` (the central
    `NotImplementedError` with the route, on an engine with and without KPIs), `chunked=True` (`ValueError`: no chunked kernel at all) and tables
    of another engine (`ValueError`): state, output planes, district sums, return and record stay what they were.  Afterwards the
    one-hidden-layer central tables still reach their own kernel on the same engine, and the deep central ones theirs."""
    from citylearn_amd.synthetic import tile_district
    from policy_central_util import make_central_policy
    E, K = 64, 4
    spec, tab, layout, pol, pt, plain = _setup('g2022_all', E, False)
    g33 = tile_district(golden('g2022_all').spec(), 33)
    tab33 = g33.episode_tables(0)
    lay33 = central_layout(g33)
    pt33 = make_deep_central_policy(lay33, 8, 8).pack(lay33, tab33, device='cuda:0')
    spec32, tab32, lay32, pol32, pt32, eng32 = _setup('b32', E, False, H=(64, 64))
    th_spec = golden('g2020_cz1').spec()
    thermal = StepEngine(th_spec.episode_tables(0), E, f64_maps=False)
    assert not thermal.lean
    # central tables that DO match a thermal engine's shape (nine 2022 buildings over as many rows, the bounds of its 25 action columns): the library's
    th_rows = th_spec.episode_tables(0, window=(th_spec.simulation_start_time_step, th_spec.simulation_start_time_step + pt.n_rows - 1))
    thermal9 = StepEngine(th_rows, E, f64_maps=False)
    spec9 = golden('g2022_all').spec(buildings=list(range(9)))
    lay9 = central_layout(spec9)
    pt9 = make_deep_central_policy(lay9, 8, 8).pack(lay9, spec9.episode_tables(0), device='cuda:0')
    pt9.act_low, pt9.act_high = (torch.full((thermal9.n_act_cols,), v, device='cuda') for v in (-1.0, 1.0))
    assert not thermal9.lean and (pt9.n_rows, pt9.n_bldg) == (thermal9.n_ts_rows, thermal9.n_bldg) == (pt.n_rows, 9)
    route = 'DeepCentralPolicyTables: a central-agent policy has no KPI kernel.*replay its action plane.*kpi=True'
    cases = [('thermal district', thermal, pt, {}, ValueError, 'policy tables (are packed for|hold)'),
             ('thermal district, tables of its shape', thermal9, pt9, {}, _lib.EngineError, 'clpcd_rollout_mlp_f32: only battery \\+ PV districts \\(CLD_LEAN\\)'),
             ('33 buildings', StepEngine(tab33, E, f64_maps=False), pt33, {}, _lib.EngineError, 'clpcd_rollout_mlp_f32: n_bldg=33 > 32'),
             ('kpi engine', StepEngine(tab, E, f64_maps=False, kpi=True), pt, {}, _lib.EngineError, 'clpcd_rollout_mlp_f32.*CLD_KPI'),
             ('kpi=True on a kpi engine', StepEngine(tab, E, f64_maps=False, kpi=True), pt, {'kpi': True}, NotImplementedError, route),
             ('kpi=True', plain, pt, {'kpi': True}, NotImplementedError, route),
             ('chunked=True', plain, pt, {'chunked': True}, ValueError, 'no building-chunked policy kernel for DeepCentralPolicyTables at all'),
             ('f64_maps=True', StepEngine(tab, E, f64_maps=True), pt, {}, _lib.EngineError, 'clpcd_rollout_mlp_f32.*CLD_F64_MAPS'),
             ('vec=2', StepEngine(tab, E, f64_maps=False, tuning=dict(vec=2)), pt, {}, _lib.EngineError,
              'no deep central policy rollout kernel at 2 envs per lane: it runs at one env per lane'),
             ('nw=8', StepEngine(tab, E, f64_maps=False, tuning=dict(nw=8)), pt, {}, _lib.EngineError, 'bad nw 8'),
             ('tables of another engine', plain, pt32, {}, ValueError, 'policy tables are packed for'),
             ('tables of 33 buildings', eng32, pt33, {}, ValueError, 'policy tables are packed for')]
    for name, eng, tables, kw, exc, match in cases:
        ret = torch.full((E,), 3.0, device='cuda')
        traj = torch.full((K, policy.CLPOL_NT, eng.n_bldg, E), -7.0, device='cuda')
        before = [x.clone() for x in (eng.state, eng.out_bldg, eng._out_env, ret, traj)]
        t_before = eng.t
        with pytest.raises(exc, match=match):
            eng.rollout_policy(K, tables, ret_env=ret, traj=traj, **kw)
        torch.cuda.synchronize()
        assert eng.t == t_before, name
        for x, was in zip((eng.state, eng.out_bldg, eng._out_env, ret, traj), before):
            assert torch.equal(x, was), name
    # the one-hidden-layer central tables still go to THEIR kernel on the same engine, the deep central ones to theirs (b32 at 64 x 64 units:
    # the largest launch, which opts in to more than 64 KiB of LDS)
    plain.rollout_policy(K, make_central_policy(layout, 16).pack(layout, tab, device='cuda:0'))
    assert plain.last_kernels.startswith('cl_rollout_policy_central_kernel<'), plain.last_kernels
    plain.reset()
    _roll(plain, pt, K)
    _roll(eng32, pt32, K)
    assert _lib.policy_central_deep_lds_bytes(16, 32, 64, 64) > 64 * 1024
