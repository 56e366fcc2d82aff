"""The closed-loop rollout of THERMAL districts under a central-agent policy with TWO hidden layers on the GPU (`StepEngine.rollout_policy` /
`VectorCityLearnEnv.rollout_policy` with a `policy.DeepCentralStorageMLPPolicy`: one launch of `cl_rollout_full_policy_central_deep_kernel`,
csrc/cl_policy_full_central_deep.h): (1) its head actions teacher-forced against the float64 MLP over the recorded planes of ALL buildings, (2) its
record replayed through `step()`, MARL and the outage branch included, (3) free-running against the CPU oracle, (4) launch splitting, checkpoints,
episode windows x parameter sets x env offsets bit for bit, (5) the env-level call against `capture_rollout` with the same MLP in torch, (6) the
refusals.  Weights: tests/policy_full_central_deep_util.py (their scale fixed by tests/test_policy_full_central_deep_host.py's conditioning test).
Every tolerance is the existing thermal / central tests': the 4 x gate of the teacher-forced tests, `_replay` of
tests/test_gpu_policy_full_rollout.py, `check_worst`'s plain bar.  Every case runs at E <= 260 and K <= 55."""
import numpy as np
import pytest
import torch

from golden_util import check_worst, golden, record_worst
from citylearn_amd import _lib, policy
from citylearn_amd.engine import StepEngine
from policy_full_central_deep_util import (CentralStorageObservations, central_layout, f32_torch_deviation, host_closed_loop,
                                           make_deep_central_storage_policy, replay_noise, thermal_district)
from policy_full_util import outage_mask
from test_gpu_policy_full_rollout import KINDS, _replay

pytestmark = pytest.mark.gpu

A, R, N, S = policy.CLPF_T_ACTION, policy.CLPF_T_REWARD, policy.CLPF_T_NET, policy.CLPF_T_SOC
NA = policy.CLPF_NA
F64 = ['chain', False]
NAMES = ('w1', 'b1', 'w2', 'b2', 'w3', 'b3')


def _kernel(eng, kind='RewardFunction'):
    return f"cl_rollout_full_policy_central_deep_kernel<{2 if eng.f64_chain else 0}, {'true' if kind == 'MARL' else 'false'}>"


def _setup(name, E, f64='chain', kind='RewardFunction', H=(16, 16), sigma=None, n_sets=1, set_of_block=None, seed=None, normalize=True, **kw):
    spec = thermal_district(name)
    tab = spec.episode_tables(0)
    layout = central_layout(spec, normalize)
    pol = make_deep_central_storage_policy(layout, *H, n_sets=n_sets, seed=sum(H) if seed is None else seed, sigma=sigma)
    pt = pol.pack(layout, tab, device='cuda:0', set_of_block=set_of_block)
    eng = StepEngine(tab, E, reward=kind, f64_maps=f64, **kw)
    eng.trace_kernels()
    return spec, tab, layout, pol, pt, eng


def _roll(eng, pt, K, seed=0, kind='RewardFunction', ret=None):
    ret = torch.zeros(eng.n_env, device='cuda') if ret is None else ret
    traj = torch.full((K, policy.CLPF_NT, eng.n_bldg, eng.n_env), float('nan'), device='cuda')
    eng.rollout_policy(K, pt, seed=seed, ret_env=ret, traj=traj)
    assert not torch.isnan(traj).any()
    assert eng.last_kernels == _kernel(eng, kind), eng.last_kernels
    return ret, traj


def _teacher_forced(tab, layout, pol, pt, traj, seed=0, row0=0, env_offset=0):
    """(kernel's worst |action - float64 MLP| over the heads that exist, a float32 torch evaluation's, on the recorded planes of all buildings of
    every step); the planes of the heads a building lacks must be 0."""
    K, E = traj.shape[0], traj.shape[3]
    cobs = CentralStorageObservations(layout, tab)
    tr = traj.cpu().numpy().astype(np.float64)
    x = np.stack([cobs.at(row0, reset=True, E=E)] + [cobs.at(row0 + k, *tr[k - 1, S:S + 4], tr[k - 1, N]) for k in range(1, K)])
    z = None
    if np.any(pt.sigma_bldg > 0):
        z = np.stack([replay_noise(pt, seed, E, k, env_offset) for k in range(K)])
    ref = pol.actions_host(x, pt, noise=z)                                            # [K, E, B, 4]
    got = tr[:, A:A + NA].transpose(0, 3, 2, 1)                                       # [K, 4, B, E] -> [K, E, B, 4]
    assert not got[:, :, pt.cols < 0].any()                                           # a head without a column: plane written as 0
    return float(np.abs(got - ref).max()), f32_torch_deviation(pol, x, pt, device='cuda', noise=z)


# ---- 1. teacher-forced actions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sigma', [0.1, None])
@pytest.mark.parametrize('f64', F64)
@pytest.mark.parametrize('name', ['g2020_cz1', 't1', 't2', 't16'])
@pytest.mark.parametrize('H', [(4, 4), (32, 32), (64, 64), (4, 64), (64, 4)])
def test_1_teacher_forced_actions(H, name, f64, sigma):
    """(1) Every recorded head action recomputed in float64 from the recorded soc / cs / hs / ds / net planes of ALL buildings (the step before;
    the reset observation at step 0; the noise replayed from the Philox stream), E = 260: a ragged last tile and two env blocks.  Gate: 4 x the
    worst deviation of a float32 torch evaluation of the same MLP on the same inputs -- the project's gate for its policy kernels.  t1 is the
    one-wave workgroup whose wave owns every group of both layers; t2 has a building with and one without DHW storage; t16 at H2 = 4 leaves
    fifteen of its sixteen waves without a layer-2 group -- they cross barrier A2 all the same --, and t16 at 64 x 64 is the launch that opts in
    to more than 64 KiB of LDS.  The figures are printed and recorded (`CL_PARITY_REPORT`; profiles/policy_full_central_deep_parity.md)."""
    spec, tab, layout, pol, pt, eng = _setup(name, 260, f64, H=H, sigma=sigma)
    _, traj = _roll(eng, pt, 24, seed=11)
    dev_kernel, dev_f32 = _teacher_forced(tab, layout, pol, pt, traj, seed=11)
    if name == 't2':
        assert pt.cols[0, policy.CLPF_A_DS] >= 0 and pt.cols[1, policy.CLPF_A_DS] < 0
    if name == 't16' and H == (64, 64):
        assert _lib.policy_full_central_deep_lds_bytes(16, 64, 64) == 125184 > 64 * 1024
    print(f'teacher-forced {name} f64={f64} H={H} sigma={sigma}: kernel {dev_kernel:.3e}  float32 torch {dev_f32:.3e}  ratio {dev_kernel / dev_f32:.2f}')
    record_worst({'kernel': dev_kernel, 'float32_torch': dev_f32, 'ratio': dev_kernel / dev_f32},
                 f'deep central thermal teacher-forced {name} f64={f64} H={H[0]}x{H[1]} sigma={sigma}', 4.0)
    assert dev_f32 > 0 and dev_kernel <= 4.0 * dev_f32, (dev_kernel, dev_f32)


# ---- 2. replay ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', F64)
@pytest.mark.parametrize('name', ['g2020_cz1', 'g2020_cz1_outage', 't2_outage'])
@pytest.mark.parametrize('kind', KINDS)
def test_2_replay_through_single_steps(kind, name, f64):
    """(2) The recorded head planes fed step by step to a second engine's `step()`: all state planes, net, reward, the district sums and the return
    at the tolerances of tests/test_gpu_policy_full_rollout.py's replay (`_replay`, which on an outage district also holds net exactly 0 on the
    outage rows and on no other), for every reward kind the thermal policy kernel takes -- MARL rides on the step's last barrier.  Two
    launches, 6 + 24 steps, at H = (32, 24): on the outage districts the boundary falls inside building 0's first outage, and the common outage
    rows 22 .. 26 straddle t = 24."""
    E, K0, K1 = 260, 6, 24
    spec, tab, layout, pol, pt, eng = _setup(name, E, f64, kind, H=(32, 24), sigma=0.1)
    ret, first = _roll(eng, pt, K0, seed=5, kind=kind)
    _, second = _roll(eng, pt, K1, seed=5, kind=kind, ret=ret)
    traj = torch.cat([first, second])
    if name.endswith('_outage'):
        m = outage_mask(tab, K0 + K1)
        assert m[K0 - 1, 0] and m[K0, 0] and m[23].any() and m[24].any() and not m[:1].any()
    else:
        assert not tab.outage.any()
    _replay(tab, pt, eng, ret, traj, kind, f64)


# ---- 3. free-running ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', F64)
@pytest.mark.parametrize('H', [(4, 4), (32, 32), (64, 64), (64, 4)])
@pytest.mark.parametrize('name', ['g2020_cz1', 't1', 't16'])
def test_3_free_running_against_the_cpu(name, H, f64):
    """(3) K = 48 from reset: the host loop of `COracle.step` + `actions_host` (float64) against one launch, at the plain bar 1e-4 + 1e-4 |ref|
    on soc, cs, ds, degraded capacity, net, reward and district net -- the policies of the CPU conditioning test
    (test_policy_full_central_deep_host.py), under which the loop stays within 0.1 x the bar when perturbed by the full teacher-forced tolerance."""
    E, K = 64, 48
    spec, tab, layout, pol, pt, eng = _setup(name, E, f64, H=H)
    want = host_closed_loop(spec, tab, layout, pol, pt, K, E)
    _, traj = _roll(eng, pt, K)
    tr = traj.cpu().numpy().astype(np.float64)
    bar = lambda got, ref: float((np.abs(got - ref) / (1e-4 + 1e-4 * np.abs(ref))).max())
    worst = {'soc': bar(tr[:, S], want['soc']), 'cs': bar(tr[:, S + 1], want['cs']), 'ds': bar(tr[:, S + 3], want['ds']),
             'net': bar(tr[:, N], want['net']), 'reward': bar(tr[:, R], want['reward']),
             'district_net': bar(tr[:, N].sum(axis=1), want['dnet']),
             'degraded_capacity': bar(eng.degraded_capacity.cpu().numpy(), want['degcap'][-1])}
    print(f'free-running {name} H={H} f64={f64}:', {k: round(v, 4) for k, v in worst.items()})
    assert not tr[:, S + 2].any()
    check_worst(worst, f'deep central thermal policy rollout {name} H={H[0]}x{H[1]} f64={f64}')


# ---- 4. bit for bit ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', F64)
def test_4a_split_launches_and_checkpoint_are_bit_identical(f64):
    """(4) Launches of 1, 5, 24 and 25 steps from t0 = 0 equal one 55-step launch bit for bit (the state and the previous net of EVERY building
    travel through the state planes and out_bldg into X, t == 0 uses net_reset), with a checkpoint restored into a fresh engine between two of
    them; MARL, noise on, a ragged tile."""
    E = 260
    spec, tab, layout, pol, pt, one = _setup('g2020_cz1', E, f64, 'MARL', H=(24, 40), sigma=0.1)
    ret1, traj1 = _roll(one, pt, 55, seed=3, kind='MARL')
    eng = StepEngine(tab, E, reward='MARL', f64_maps=f64)
    ret, parts = torch.zeros(E, device='cuda'), []
    for n, K in enumerate((1, 5, 24, 25)):
        if n == 2:
            sd = eng.state_dict()
            eng = StepEngine(tab, E, reward='MARL', f64_maps=f64)
            eng.load_state_dict(sd)
        eng.trace_kernels()
        traj = torch.empty((K, policy.CLPF_NT, eng.n_bldg, E), device='cuda')
        eng.rollout_policy(K, pt, seed=3, ret_env=ret, traj=traj)
        assert eng.last_kernels == _kernel(eng, 'MARL'), eng.last_kernels
        parts.append(traj)
    assert eng.t == 55 and torch.equal(torch.cat(parts), traj1)
    assert torch.equal(eng.state, one.state) and torch.equal(eng.out_bldg[:2], one.out_bldg[:2]) and torch.equal(eng.out_env, one.out_env)
    torch.testing.assert_close(ret, ret1, rtol=1e-6, atol=1e-4)               # (four partial sums instead of one)


@pytest.mark.parametrize('f64', F64)
def test_4b_windows_sets_and_env_offsets(f64):
    """(4) Two env blocks with different episode windows AND different parameter sets in one launch: each block equals, bit for bit, an engine
    of its own with that window, that set and its env offset (noise on: the half batches reproduce the whole batch's streams)."""
    spec = thermal_district('g2020_cz1')
    tab = spec.episode_tables(0)
    layout = central_layout(spec)
    pol = make_deep_central_storage_policy(layout, 16, 24, n_sets=2, seed=2, sigma=0.1)
    K, n_steps, rows = 24, 200, [0, 131]
    whole = StepEngine(tab, 260, f64_maps=f64, n_steps=n_steps, env_row0=rows)
    whole.trace_kernels()
    _, traj = _roll(whole, pol.pack(layout, tab, device='cuda:0', set_of_block=[0, 1]), K, seed=9)
    for g, (lo, hi) in enumerate(((0, 256), (256, 260))):
        part = StepEngine(tab, hi - lo, f64_maps=f64, n_steps=n_steps, env_row0=[rows[g]], env_offset=lo)
        part.trace_kernels()
        _, tr = _roll(part, pol.pack(layout, tab, device='cuda:0', set_of_block=[g]), K, seed=9)
        assert torch.equal(tr, traj[:, :, :, lo:hi]), g
        assert torch.equal(part.state, whole.state[:, :, lo:hi]) and torch.equal(part.out_env, whole.out_env[:, lo:hi])
    # ... and the actions of block 1 are its window's and its set's: teacher-forced like (1)
    single = policy.DeepCentralStorageMLPPolicy(*(getattr(pol, n)[1:2] for n in NAMES), sigma=0.1)
    dev_kernel, dev_f32 = _teacher_forced(tab, layout, single, single.pack(layout, tab), traj[:, :, :, 256:], seed=9, row0=rows[1], env_offset=256)
    print(f'window 1 / set 1 teacher-forced: kernel {dev_kernel:.3e}  float32 torch {dev_f32:.3e}')
    assert dev_kernel <= 4.0 * dev_f32


def test_4c_return_accumulates_and_a_zero_step_launch_changes_nothing():
    """(4) `ret_env` is accumulated, not overwritten; a 0-step launch leaves state, outputs, district sums and return what they were."""
    E = 260
    spec, tab, layout, pol, pt, eng = _setup('g2020_cz1', E, H=(8, 12))
    ret = torch.full((E,), 5.0, device='cuda')
    eng.rollout_policy(6, pt, ret_env=ret)
    assert eng.last_kernels == _kernel(eng), eng.last_kernels
    fresh = StepEngine(tab, E)
    fresh.trace_kernels()
    ret0 = torch.zeros(E, device='cuda')
    fresh.rollout_policy(6, pt, ret_env=ret0)
    assert fresh.last_kernels == _kernel(fresh), fresh.last_kernels
    assert torch.equal(ret, ret0 + 5.0) or torch.allclose(ret, ret0 + 5.0, rtol=1e-6, atol=1e-5)
    assert float((ret - 5.0).abs().max()) > 0
    before = [x.clone() for x in (eng.state, eng.out_bldg, eng._out_env, ret)]
    eng.rollout_policy(0, pt, ret_env=ret)
    torch.cuda.synchronize()
    assert eng.last_kernels == _kernel(eng), eng.last_kernels
    assert eng.t == 6 and all(torch.equal(x, was) for x, was in zip((eng.state, eng.out_bldg, eng._out_env, ret), before))


# ---- 5. env level ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('normalize', [True, False])
def test_5_env_level_equals_capture_rollout_with_the_torch_mlp(normalize):
    """(5) `VectorCityLearnEnv(..., central_agent=True).rollout_policy(deep central, K, record=True)` against `capture_rollout` driven by
    `torch_policy`: the tolerance is built as tests/test_gpu_policy_full_central_rollout.py::test_5 builds it, carried through both hidden layers
    -- the teacher-forced tolerance (4 x a float32 evaluation's deviation, measured here on the recorded inputs), once more for the float32 torch
    policy's own deviation, widened by what the two paths' state tolerance (2e-6 on the socs, 2e-5 on net, relative + absolute) can move an
    action through ALL buildings' inputs: dh1[j] = sum_b' sum_d |W1[j][column of b' term d]| scale tol_d, dh2[i] = sum_j |W2[i][j]| dh1[j],
    da[b][a] = half[b][a] sum_i |w3[b][a][i]| dh2[i] (tanh' <= 1 in every layer); returns at rtol 1e-5 / atol 1e-3.  `kpi=True` names the head
    planes, an env built with central_agent=False raises `ValueError` (`chunked=True` on the engine: test_6)."""
    from citylearn_amd.vector_env import VectorCityLearnEnv
    g = golden('g2020_cz1')
    E, K = 256, 24
    a, b = (VectorCityLearnEnv(g.schema_path, E, observations='tensor', normalize_observations=normalize, central_agent=True) for _ in range(2))
    assert a.central_agent and a.layout.central_agent
    a.engine.trace_kernels()
    pol = make_deep_central_storage_policy(a.layout, 32, 24, seed=4)
    with pytest.raises(NotImplementedError, match=r'a central-agent policy has no KPI kernel.*record=True.*policy\.CLPF_T_ACTION \+ head.*policy\.head_columns.*kpi=True'):
        a.rollout_policy(pol, 2, kpi=True)
    ret, traj = a.rollout_policy(pol, K, record=True)
    assert a._t == K == a.engine.t and traj.shape == (K, policy.CLPF_NT, a.n_bldg, E) and policy.CLPF_NT == 10
    assert a.engine.last_kernels == _kernel(a.engine), a.engine.last_kernels
    pt_host = pol.pack(a.layout, a.tables)                                     # (host copy: bounds, columns, sigmas for the reference)
    f = pol.torch_policy(b.layout, b.tables, b.device)
    acts = torch.zeros((K, b.n_act_cols, E), device='cuda')

    def recorded(obs, i):
        acts[i].copy_(f(obs, i))
        return acts[i]
    cap = b.capture_rollout(recorded, K)
    _, rewards, _ = cap.run()
    torch.cuda.synchronize()
    dev_kernel, dev_f32 = _teacher_forced(a.tables, a.layout, pol, pt_host, traj)
    cobs = CentralStorageObservations(a.layout, a.tables)
    w1, _, w2, _, w3, _ = (v[0] for v in pol._full(a.n_bldg))                    # [H1, n_cols], [H2, H1], [B, 4, H2]
    tr = traj.cpu().numpy().astype(np.float64)
    tols = [2e-6 * (1 + np.abs(tr[:, S + d]).max()) for d in range(4)] + [2e-5 * (1 + np.abs(tr[:, N]).max())]
    gain1 = sum(np.abs(w1 * np.where(cobs.is_term[d], cobs.scale, 0.0)[None, :]).sum(axis=1) * tols[d] for d in range(5))     # [H1]
    gain2 = np.abs(w2) @ gain1                                                    # [H2]
    half = 0.5 * (pt_host.high_bldg - pt_host.low_bldg)                          # [B, 4]
    widen = float((half * (np.abs(w3) * gain2[None, None, :]).sum(axis=2)).max())
    tol = 4.0 * dev_f32 + dev_f32 + widen
    b_idx, h_idx = np.nonzero(pt_host.cols >= 0)
    got = traj[:, A:A + NA][:, torch.as_tensor(h_idx, device='cuda'), torch.as_tensor(b_idx, device='cuda')]      # [K, heads, E]
    want = acts[:, torch.as_tensor(pt_host.cols[b_idx, h_idx], device='cuda')]
    worst = float((got - want).abs().max())
    print(f'env level normalize={normalize}: |action difference| {worst:.3e}, tolerance {tol:.3e} (float32 deviation {dev_f32:.3e}, state term {widen:.3e}); '
          f'kernel teacher-forced {dev_kernel:.3e}')
    assert worst <= tol and dev_kernel <= 4.0 * dev_f32
    torch.testing.assert_close(ret, rewards.sum(dim=0) if rewards.dim() == 2 else rewards.sum(dim=(0, 1)), rtol=1e-5, atol=1e-3)
    torch.testing.assert_close(a.engine.state, b.engine.state, rtol=2e-6, atol=2e-6)
    # the per-building env's observation tensor is not the vector the weights are defined over
    c = VectorCityLearnEnv(g.schema_path, E, observations='tensor', normalize_observations=normalize, central_agent=False)
    state = c.engine.state.clone()
    with pytest.raises(ValueError, match='needs an env built with central_agent=True'):
        c.rollout_policy(pol, K)
    assert c._t == 0 and torch.equal(c.engine.state, state)


def test_5b_env_level_seventeen_buildings_are_the_librarys_refusal():
    """(5) A 17-building thermal env built with central_agent=True: no chunked launch is asked for, the library refuses by name."""
    from citylearn_amd.vector_env import VectorCityLearnEnv
    from dataclasses import replace
    env = VectorCityLearnEnv(replace(thermal_district('t17'), central_agent=True), 64, observations='tensor')
    assert env.central_agent and env.layout.central_agent and env.n_bldg == 17
    pol = make_deep_central_storage_policy(env.layout, 8, 12)
    state = env.engine.state.clone()
    with pytest.raises(_lib.EngineError, match='clpfcd_rollout_mlp_f32: n_bldg=17 > 16'):
        env.rollout_policy(pol, 4)
    assert env._t == 0 and torch.equal(env.engine.state, state)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def test_6_refusals_leave_every_plane_untouched():
    """A battery + PV district (foreign tables: `ValueError`; tables of its shape: the library's CLD_LEAN refusal), 17 buildings, a `kpi=True`
    engine, `f64_maps=True`, two envs per lane (the library's refusals, by name), `kpi=True` (`NotImplementedError` with the route over the head
    planes, on an engine with and without KPIs), `chunked=True` (`ValueError`: no chunked kernel at all) and tables of another engine
    (`ValueError`): state, output planes, district sums, return and record stay what they were.  Afterwards `CentralStorageMLPPolicy` and
    `DeepCentralMLPPolicy` tables still reach their own kernels on their engines, and the new ones theirs."""
    from policy_central_deep_util import make_deep_central_policy
    from policy_full_central_util import make_central_storage_policy
    E, K = 64, 4
    spec, tab, layout, pol, pt, plain = _setup('g2020_cz1', E, False)
    spec17, tab17, lay17, pol17, pt17, eng17 = _setup('t17', E, False, H=(8, 12))
    spec2, tab2, lay2, pol2, pt2, eng2 = _setup('t2', E, False, H=(64, 64))
    # a battery + PV district of nine buildings, and deep central thermal tables that DO match its shape (rows, buildings, action columns): the library's
    lean_spec = golden('g2022_all').spec(buildings=list(range(9)))
    lean_tab = lean_spec.episode_tables(0)
    lean = StepEngine(lean_tab, E, f64_maps=False)
    lean.trace_kernels()
    assert lean.lean
    start = spec.simulation_start_time_step
    tab_rows = spec.episode_tables(0, window=(start, start + lean.n_ts_rows - 1))
    pt9 = pol.pack(layout, tab_rows, device='cuda:0')
    pt9.act_low, pt9.act_high = (torch.full((lean.n_act_cols,), v, device='cuda') for v in (-1.0, 1.0))
    assert (pt9.n_rows, pt9.n_bldg) == (lean.n_ts_rows, lean.n_bldg) and pt9.n_rows != pt.n_rows
    route = r'a central-agent policy has no KPI kernel.*replay its action planes \(policy\.CLPF_T_ACTION \+ head.*policy\.head_columns\).*kpi=True'
    cases = [('battery + PV district', lean, pt, {}, ValueError, 'policy tables (are packed for|hold)'),
             ('battery + PV district, tables of its shape', lean, pt9, {}, _lib.EngineError, 'clpfcd_rollout_mlp_f32: thermal / outage districts only'),
             ('17 buildings', eng17, pt17, {}, _lib.EngineError, 'clpfcd_rollout_mlp_f32: n_bldg=17 > 16'),
             ('kpi engine', StepEngine(tab, E, f64_maps=False, kpi=True), pt, {}, _lib.EngineError, 'clpfcd_rollout_mlp_f32.*CLD_KPI'),
             ('kpi=True on a kpi engine', StepEngine(tab, E, f64_maps=False, kpi=True), pt, {'kpi': True}, NotImplementedError, route),
             ('kpi=True', plain, pt, {'kpi': True}, NotImplementedError, route),
             ('chunked=True', plain, pt, {'chunked': True}, ValueError, 'no building-chunked policy kernel for DeepCentralStoragePolicyTables at all'),
             ('f64_maps=True', StepEngine(tab, E, f64_maps=True), pt, {}, _lib.EngineError, 'clpfcd_rollout_mlp_f32.*CLD_F64_MAPS'),
             ('vec=2', StepEngine(tab, E, f64_maps=False, tuning=dict(vec=2)), pt, {}, _lib.EngineError,
              'no deep central thermal policy rollout kernel at 2 envs per lane: it runs at one env per lane'),
             ('tables of another engine', plain, pt2, {}, ValueError, 'policy tables are packed for'),
             ('tables of 17 buildings', eng2, pt17, {}, ValueError, 'policy tables are packed for')]
    for name, eng, tables, kw, exc, match in cases:
        ret = torch.full((E,), 3.0, device='cuda')
        traj = torch.full((K, policy.CLPF_NT, eng.n_bldg, E), -7.0, device='cuda')
        before = [x.clone() for x in (eng.state, eng.out_bldg, eng._out_env, ret, traj)]
        t_before = eng.t
        with pytest.raises(exc, match=match):
            eng.rollout_policy(K, tables, ret_env=ret, traj=traj, **kw)
        torch.cuda.synchronize()
        assert eng.t == t_before, name
        for x, was in zip((eng.state, eng.out_bldg, eng._out_env, ret, traj), before):
            assert torch.equal(x, was), name
    # the one-hidden-layer central thermal tables and the battery + PV deep central tables still go to THEIR kernels on their engines, the new ones
    # to theirs
    plain.rollout_policy(K, make_central_storage_policy(layout, 16).pack(layout, tab, device='cuda:0'))
    assert plain.last_kernels.startswith('cl_rollout_full_policy_central_kernel<'), plain.last_kernels
    plain.reset()
    lean_layout = central_layout(lean_spec)
    lean.rollout_policy(K, make_deep_central_policy(lean_layout, 16, 24).pack(lean_layout, lean_tab, device='cuda:0'))
    assert lean.last_kernels.startswith('cl_rollout_policy_central_deep_kernel<'), lean.last_kernels
    _roll(plain, pt, K)
    _roll(eng2, pt2, K)
