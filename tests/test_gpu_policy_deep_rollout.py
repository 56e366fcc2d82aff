"""The closed-loop rollout of a policy with two hidden layers on the GPU (`StepEngine.rollout_policy` / `VectorCityLearnEnv.rollout_policy` with a
`policy.DeepMLPPolicy`: one launch of `cl_rollout_policy_deep_kernel`, csrc/cl_policy_deep.h): (1) its actions teacher-forced against the float64
MLP, (2) its record replayed through `step()`, (3) free-running against the CPU oracle, (5) launch splitting, checkpoints, episode windows x
parameter sets x env offsets bit for bit, (4) the two kernel families (layer 2 in exact fp32 / on the f16 matrix cores with split operands) against each other, (6) the env-level call
against `capture_rollout` with the same MLP in torch, (7) the refusals.  Weights:
tests/policy_deep_util.py (the free-running test's scale fixed by tests/test_policy_deep_host.py's conditioning test)."""
import numpy as np
import pytest
import torch

from golden_util import check_worst, golden, record_worst
from citylearn_amd import _lib, policy
from citylearn_amd.engine import StepEngine
from citylearn_amd.observations import ObservationLayout
from district_util import HET_UNDRIVEN, district
from policy_deep_util import FREE_MID_SCALE, f32_torch_deviation, host_closed_loop, make_deep_policy, split_bound
from policy_util import HostObservations

pytestmark = pytest.mark.gpu

KINDS = ['RewardFunction', 'IndependentSACReward', 'SolarPenaltyReward']           # (MARL is the library's refusal)
A, R, N, S = policy.CLPOL_T_ACTION, policy.CLPOL_T_REWARD, policy.CLPOL_T_NET, policy.CLPOL_T_SOC
F64 = ['chain', False]
MMA = [0, 1]                                                                      # the kernel family: `pack(matrix_cores=)`


def _setup(name, E, f64='chain', kind='RewardFunction', H=(16, 16), sigma=None, n_sets=1, set_of_block=None, seed=None, mma=0, mid_scale=None, **kw):
    spec = district(name)
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    pol = make_deep_policy(layout, *H, n_sets=n_sets, seed=sum(H) if seed is None else seed, sigma=sigma, mid_scale=mid_scale)
    pt = pol.pack(layout, tab, device='cuda:0', set_of_block=set_of_block, matrix_cores=bool(mma))
    eng = StepEngine(tab, E, reward=kind, f64_maps=f64, **kw)
    eng.trace_kernels()
    return spec, tab, layout, pol, pt, eng


def _kernel(eng, pt):
    return f'cl_rollout_policy_deep_kernel<1, {2 if eng.f64_chain else 0}, {int(pt.matrix_cores)}>'


def _roll(eng, pt, K, seed=0):
    ret = torch.zeros(eng.n_env, device='cuda')
    traj = torch.full((K, policy.CLPOL_NT, eng.n_bldg, eng.n_env), float('nan'), device='cuda')
    eng.rollout_policy(K, pt, seed=seed, ret_env=ret, traj=traj)
    assert not torch.isnan(traj).any() and eng.last_kernels == _kernel(eng, pt), eng.last_kernels
    return ret, traj


def _teacher_forced(eng, tab, layout, pol, pt, traj, seed=0, row0=0, env_offset=0):
    """(kernel's worst |action - float64 MLP| over the driven buildings, a float32 torch evaluation's, on the recorded inputs of every step); the
    undriven buildings' action plane must be 0."""
    K, E = traj.shape[0], traj.shape[3]
    hobs = HostObservations(layout, tab)
    tr = traj.cpu().numpy().astype(np.float64)
    x = np.stack([hobs.at(row0, np.zeros((eng.n_bldg, E)), None, reset=True)] + [hobs.at(row0 + k, tr[k - 1, S], tr[k - 1, N]) for k in range(1, K)])
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
@pytest.mark.parametrize('mma', MMA)
@pytest.mark.parametrize('f64', F64)
@pytest.mark.parametrize('name', ['g2022_all', 'het17', 'b1'])
@pytest.mark.parametrize('H', [(4, 4), (8, 32), (32, 8), (16, 16), (32, 32)])
def test_1_teacher_forced_actions(H, name, f64, mma):
    """(1) Every recorded action recomputed in float64 from the recorded inputs (soc / net of the step before; the reset observation at step 0;
    the noise replayed from the Philox stream), E = 260: the last tile is ragged.  Gate: 4 x the worst deviation of a float32 torch evaluation
    of the same three layers on the same inputs -- the project's gate for its policy kernels; the exact-fp32 family is the same arithmetic class
    (v_exp_f32 / v_rcp_f32 tanh units, fp32 fused multiply-adds).  The matrix-core family gets `split_bound` on top: what splitting both operands
    of layer 2 into two f16 terms can move the action by, computed in float64 from the weights with no fitted constant
    (tests/policy_deep_util.py).  E = 260 leaves the second 32-env pass of the last tile partly empty.  b1 is the one-wave workgroup (nw = 1) whose
    wave has no second building.  The figures are printed and recorded
    (profiles/policy_deep_parity.md)."""
    spec, tab, layout, pol, pt, eng = _setup(name, 260, f64, H=H, sigma=0.1, mma=mma)
    _, traj = _roll(eng, pt, 24, seed=11)
    dev_kernel, dev_f32 = _teacher_forced(eng, tab, layout, pol, pt, traj, seed=11)
    if name == 'het17':
        assert sorted(np.nonzero(pt.es_cols < 0)[0]) == sorted(HET_UNDRIVEN)
    sb = split_bound(pol, pt) if mma else 0.0
    print(f'teacher-forced {name} f64={f64} H={H} mma={mma}: kernel {dev_kernel:.3e}  float32 torch {dev_f32:.3e}  ratio {dev_kernel / dev_f32:.2f}  split_bound {sb:.3e}')
    record_worst({'kernel': dev_kernel, 'float32_torch': dev_f32, 'ratio': dev_kernel / dev_f32, 'split_bound': sb},
                 f'deep teacher-forced {name} f64={f64} H={H} mma={mma}', 4.0)
    assert dev_f32 > 0 and dev_kernel <= 4.0 * dev_f32 + sb, (dev_kernel, dev_f32, sb)


# ---- 2. replay ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mma', MMA)
@pytest.mark.parametrize('f64', F64)
@pytest.mark.parametrize('name', ['g2022_all', 'het17'])
@pytest.mark.parametrize('kind', KINDS)
def test_2_replay_through_single_steps(kind, name, f64, mma):
    """(2) The recorded actions fed step by step to a second engine's `step()`: state, last outputs, district sums, return and the record's planes
    at the tolerances of tests/test_gpu_policy_rollout.py::test_b.  The undriven buildings' action plane is 0."""
    E, K = 260, 30
    spec, tab, layout, pol, pt, eng = _setup(name, E, f64, kind, H=(16, 32), sigma=0.1, mma=mma)
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
# (b32: 32 buildings at 32 x 32 units, and 32 buildings of matrix-core rows at any size, exceed a CU's LDS -- (7)'s refusals)
FREE = [(n, H, m) for m in MMA for n in ('g2022_all', 'het17', 'b1') for H in ((4, 4), (16, 32), (32, 32))] + [('b32', (4, 4), 0), ('b32', (16, 32), 0)]


@pytest.mark.parametrize('f64', F64)
@pytest.mark.parametrize('name,H,mma', FREE)
def test_3_free_running_against_the_cpu(name, H, f64, mma):
    """(3) K = 48 from reset: the host loop of `COracle.step` + `actions_host` (float64) against one launch, at the plain bar 1e-4 + 1e-4 |ref|
    on soc, degraded capacity, net, reward and district net -- the policies of the CPU conditioning test (test_policy_deep_host.py: middle layer
    at `FREE_MID_SCALE`, under which the loop stays within 0.1 x the bar when perturbed by either family's full teacher-forced tolerance).  b32 at
    32 x 32 units exceeds a CU's LDS and is (7)'s refusal, as b32 is in the matrix-core family at every size; b1 is the one-wave workgroup."""
    E, K = 64, 48
    spec, tab, layout, pol, pt, eng = _setup(name, E, f64, H=H, mma=mma, mid_scale=FREE_MID_SCALE)
    want = host_closed_loop(spec, tab, layout, pol, pt, K, E)
    _, traj = _roll(eng, pt, K)
    tr = traj.cpu().numpy().astype(np.float64)
    bar = lambda got, ref: float((np.abs(got - ref) / (1e-4 + 1e-4 * np.abs(ref))).max())
    worst = {'soc': bar(tr[:, S], want['soc']), 'net': bar(tr[:, N], want['net']), 'reward': bar(tr[:, R], want['reward']),
             'district_net': bar(tr[:, N].sum(axis=1), want['dnet']),
             'degraded_capacity': bar(eng.degraded_capacity.cpu().numpy(), want['degcap'][-1])}
    print(f'free-running {name} H={H} f64={f64} mma={mma}:', {k: round(v, 4) for k, v in worst.items()})
    check_worst(worst, f'deep policy rollout {name} H={H} f64={f64} mma={mma}')


# ---- 4. the two families -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', F64)
@pytest.mark.parametrize('name,H', [('g2022_all', (32, 32)), ('het17', (8, 32)), ('g2022_all', (32, 8)), ('g2022_all', (4, 4))])
def test_4_the_two_families_against_each_other(name, H, f64):
    """(4) The exact-fp32 and the matrix-core family on IDENTICAL inputs, so that the closed loop amplifies nothing: the first step from reset,
    and one step from a checkpoint the exact-fp32 engine left after 12 steps, restored into both (same seed, noise on).  The actions differ by
    at most `split_bound` + two float32 roundings of the action; whether the other planes come out bit-equal is recorded, not gated."""
    E = 260
    spec, tab, layout, pol, pt0, e0 = _setup(name, E, f64, H=H, sigma=0.1, mma=0)
    pt1 = pol.pack(layout, tab, device='cuda:0', matrix_cores=True)
    e1 = StepEngine(tab, E, f64_maps=f64)
    e1.trace_kernels()
    tol = split_bound(pol, pt0) + 2 * 2.0 ** -24 * float(max(np.abs(pt0.low_bldg).max(), np.abs(pt0.high_bldg).max()))
    worst, equal = 0.0, {}
    for stage in ('reset', 'checkpoint'):
        if stage == 'checkpoint':
            _roll(e0, pt0, 11, seed=7)
            sd = e0.state_dict()
            e0.load_state_dict(sd)
            e1.load_state_dict(sd)
        (_, t0), (_, t1) = _roll(e0, pt0, 1, seed=7), _roll(e1, pt1, 1, seed=7)
        d = float((t0[:, A] - t1[:, A]).abs().max())
        worst = max(worst, d)
        equal[stage] = {n: bool(torch.equal(t0[:, p], t1[:, p])) for n, p in (('action', A), ('net', N), ('soc', S), ('reward', R))}
        assert d <= tol, (stage, d, tol)
        assert float(t0[:, A].abs().max()) > 0.01
    print(f'families {name} H={H} f64={f64}: |action difference| {worst:.3e}, split_bound + 2 roundings {tol:.3e}; bit-equal planes {equal}')
    record_worst({'action_difference': worst, 'bound': tol}, f'deep families {name} H={H} f64={f64}', tol)


# ---- 5. bit for bit ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mma', MMA)
@pytest.mark.parametrize('f64', F64)
def test_5a_split_launches_and_checkpoint_are_bit_identical(f64, mma):
    """(5) Launches of 1, 5, 24 and 25 steps from t0 = 0 equal one 55-step launch bit for bit (the previous net travels through out_bldg, t == 0
    uses net_reset), with a checkpoint restored into a fresh engine between two of them; noise on, a ragged last tile."""
    E = 260
    spec, tab, layout, pol, pt, one = _setup('g2022_all', E, f64, 'SolarPenaltyReward', H=(8, 12), sigma=0.1, mma=mma)
    ret1, traj1 = _roll(one, pt, 55, seed=3)
    eng = StepEngine(tab, E, reward='SolarPenaltyReward', f64_maps=f64)
    ret, parts = torch.zeros(E, device='cuda'), []
    for n, K in enumerate((1, 5, 24, 25)):
        if n == 2:
            sd = eng.state_dict()
            eng = StepEngine(tab, E, reward='SolarPenaltyReward', f64_maps=f64)
            eng.load_state_dict(sd)
        traj = torch.empty((K, policy.CLPOL_NT, eng.n_bldg, E), device='cuda')
        eng.rollout_policy(K, pt, seed=3, ret_env=ret, traj=traj)
        parts.append(traj)
    assert eng.t == 55 and torch.equal(torch.cat(parts), traj1)
    assert torch.equal(eng.state, one.state) and torch.equal(eng.out_bldg[:2], one.out_bldg[:2]) and torch.equal(eng.out_env, one.out_env)
    torch.testing.assert_close(ret, ret1, rtol=1e-6, atol=1e-4)               # (four partial sums instead of one)


@pytest.mark.parametrize('mma', MMA)
@pytest.mark.parametrize('f64', F64)
def test_5b_windows_sets_and_env_offsets(f64, mma):
    """(5) Two env blocks with different episode windows AND different parameter sets in one launch: each block equals, bit for bit, an engine
    of its own with that window, that set and its env offset (noise on: the half batches reproduce the whole batch's streams)."""
    spec = district('g2022_all')
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    pol = make_deep_policy(layout, 16, 8, n_sets=2, seed=2, sigma=0.1)
    K, n_steps, rows = 24, 200, [0, 131]
    whole = StepEngine(tab, 512, f64_maps=f64, n_steps=n_steps, env_row0=rows)
    whole.trace_kernels()
    _, traj = _roll(whole, pol.pack(layout, tab, device='cuda:0', set_of_block=[0, 1], matrix_cores=bool(mma)), K, seed=9)
    assert not torch.equal(traj[:, A, :, :256], traj[:, A, :, 256:])
    for g in range(2):
        part = StepEngine(tab, 256, f64_maps=f64, n_steps=n_steps, env_row0=[rows[g]], env_offset=256 * g)
        part.trace_kernels()
        _, tr = _roll(part, pol.pack(layout, tab, device='cuda:0', set_of_block=[g], matrix_cores=bool(mma)), K, seed=9)
        sl = slice(256 * g, 256 * (g + 1))
        assert torch.equal(tr, traj[:, :, :, sl]), g
        assert torch.equal(part.state, whole.state[:, :, sl]) and torch.equal(part.out_env, whole.out_env[:, sl])
    # ... and the actions of block 1 are its window's and its set's: teacher-forced like (1)
    single = policy.DeepMLPPolicy(*(getattr(pol, n)[1:2] for n in ('w1', 'b1', 'w2', 'b2', 'w3', 'b3')), sigma=0.1)
    dev_kernel, dev_f32 = _teacher_forced(whole, tab, layout, single, single.pack(layout, tab), traj[:, :, :, 256:], seed=9, row0=rows[1], env_offset=256)
    print(f'window 1 / set 1 teacher-forced mma={mma}: kernel {dev_kernel:.3e}  float32 torch {dev_f32:.3e}')
    assert dev_kernel <= 4.0 * dev_f32 + (split_bound(single, single.pack(layout, tab)) if mma else 0.0)


@pytest.mark.parametrize('mma', MMA)
def test_5c_return_accumulates_and_a_zero_step_launch_changes_nothing(mma):
    """(5) `ret_env` is accumulated, not overwritten; a 0-step launch leaves state, outputs, district sums and return what they were."""
    E = 260
    spec, tab, layout, pol, pt, eng = _setup('g2022_all', E, H=(8, 8), mma=mma)
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


# ---- 6. env level ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mma', MMA)
@pytest.mark.parametrize('normalize', [True, False])
def test_6_env_level_equals_capture_rollout_with_the_torch_mlp(normalize, mma, monkeypatch):
    """(6) `VectorCityLearnEnv.rollout_policy(deep, K, record=True)` against `capture_rollout` driven by `deep.torch_policy`: the tolerance is
    built as tests/test_gpu_policy_rollout.py::test_g builds it -- the teacher-forced tolerance (4 x a float32 evaluation's deviation, measured
    here on the recorded inputs), once more for the float32 torch policy's own deviation, widened by what the two paths' state tolerance (2e-6 on
    soc, 2e-5 on net, relative + absolute) can move an action through THREE layers: dz1_j = |W1_j,soc| scale tol_soc + |W1_j,net| scale tol_net,
    dz2_i = sum_j |W2_ij| dz1_j, da = half sum_i |w3_i| dz2_i (tanh' <= 1); returns at rtol 1e-5 / atol 1e-3."""
    from citylearn_amd.vector_env import VectorCityLearnEnv
    monkeypatch.setattr(policy, 'default_matrix_cores', lambda h1, h2, n_bldg=None: bool(mma))      # (the env packs with matrix_cores=None: both families through it)
    g = golden('g2022_all')
    E, K = 256, 24
    a, b = (VectorCityLearnEnv(g.schema_path, E, observations='tensor', normalize_observations=normalize) for _ in range(2))
    a.engine.trace_kernels()
    pol = make_deep_policy(a.layout, 16, 32, seed=4)
    ret, traj = a.rollout_policy(pol, K, record=True)
    pt_host = pol.pack(a.layout, a.tables)
    assert a._t == K == a.engine.t and pt_host.matrix_cores == bool(mma) and a.engine.last_kernels == _kernel(a.engine, pt_host)
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
    hobs = HostObservations(a.layout, a.tables)
    w1, _, w2, _, w3, _ = (v[0] for v in pol._full(a.n_bldg))                    # [B, H1, n_obs], [B, H2, H1], [B, H2]
    tr = traj.cpu().numpy().astype(np.float64)
    tol_soc, tol_net = 2e-6 * (1 + np.abs(tr[:, S]).max()), 2e-5 * (1 + np.abs(tr[:, N]).max())
    g_soc = np.abs(w1 * np.where(hobs.is_term[0], hobs.scale, 0.0)[:, None, :]).sum(axis=2)      # [B, H1]
    g_net = np.abs(w1 * np.where(hobs.is_term[1], hobs.scale, 0.0)[:, None, :]).sum(axis=2)
    dz2 = np.einsum('bij,bj->bi', np.abs(w2), g_soc * tol_soc + g_net * tol_net)
    half = 0.5 * (pt_host.high_bldg - pt_host.low_bldg)
    widen = float((half * (np.abs(w3) * dz2).sum(axis=1)).max())
    tol = 4.0 * dev_f32 + dev_f32 + widen + (split_bound(pol, pt_host) if mma else 0.0)
    worst = float((traj[:, A] - acts[:, :a.n_bldg]).abs().max())
    print(f'env level normalize={normalize} mma={mma}: |action difference| {worst:.3e}, tolerance {tol:.3e} (float32 deviation {dev_f32:.3e}, state term {widen:.3e})')
    assert worst <= tol
    torch.testing.assert_close(ret, rewards.sum(dim=0) if rewards.dim() == 2 else rewards.sum(dim=(0, 1)), rtol=1e-5, atol=1e-3)
    torch.testing.assert_close(a.engine.state, b.engine.state, rtol=2e-6, atol=2e-6)
    with pytest.raises(NotImplementedError, match='no KPI kernel for a policy with two hidden layers.*record=True'):
        a.rollout_policy(pol, 2, kpi=True)


@pytest.mark.parametrize('name,H,mma', [('b32', (16, 32), 0), ('b32', (24, 24), 0), ('b31', (32, 16), 0), ('b16', (16, 32), 1), ('b16', (16, 16), 0)])
def test_6b_the_env_picks_a_family_that_fits(name, H, mma):
    """(6) `VectorCityLearnEnv.rollout_policy` packs with ``matrix_cores=None``: the matrix-core family where H1 x H2 >= 512 AND its rows fit the
    district.  31 and 32 buildings (sixteen waves) do not fit it at any size, so they run the exact-fp32 family -- the env call works on up
    to 32 buildings; 16 buildings take the matrix cores from 512 up.  Actions teacher-forced at (1)'s gate."""
    from citylearn_amd.vector_env import VectorCityLearnEnv
    E, K = 64, 24
    env = VectorCityLearnEnv(district(name), E, observations='tensor', normalize_observations=True)
    env.engine.trace_kernels()
    pol = make_deep_policy(env.layout, *H, seed=3, sigma=0.1)
    assert policy.default_matrix_cores(*H, env.engine.n_bldg) == bool(mma) and policy.default_matrix_cores(*H) == (H[0] * H[1] >= 512)
    ret, traj = env.rollout_policy(pol, K, seed=2, record=True)
    pt = pol.pack(env.layout, env.tables)
    assert pt.matrix_cores == bool(mma) and env.engine.last_kernels == _kernel(env.engine, pt), env.engine.last_kernels
    dev_kernel, dev_f32 = _teacher_forced(env.engine, env.tables, env.layout, pol, pt, traj, seed=2)
    print(f'env default family {name} H={H}: MMA={mma}, kernel {dev_kernel:.3e}  float32 torch {dev_f32:.3e}')
    assert dev_f32 > 0 and dev_kernel <= 4.0 * dev_f32 + (split_bound(pol, pt) if mma else 0.0)
    assert ret.shape == (E,) and bool(torch.isfinite(ret).all()) and float(traj[:, A].abs().max()) > 0.01


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------
def test_7_refusals_leave_every_plane_untouched():
    """ A MARL engine, a `kpi=True` engine, `f64_maps=True`, 33 buildings and 32 buildings at 32 x 32 units (the library's refusals, by
    name), `kpi=True` (`NotImplementedError` with the route, on an engine with and without KPIs), `chunked=True` (`ValueError`: no chunked
    kernel at all), a thermal district (foreign tables: `ValueError`; tables of its own shape: the library's CLD_LEAN refusal) and `PolicyTables` /
    `DeepPolicyTables` of another engine or of the one-hidden-layer kind on that engine (`ValueError` / the library
    of THEIR kind): state, output planes, district sums, return and record stay what they were.  Afterwards the engine still runs."""
    from citylearn_amd.synthetic import tile_district
    from policy_util import make_policy
    E, K = 64, 4
    spec, tab, layout, pol, pt, plain = _setup('g2022_all', E, False)
    g33 = tile_district(golden('g2022_all').spec(), 33)
    tab33 = g33.episode_tables(0)
    lay33 = ObservationLayout(g33, 'current', True)
    pt33 = make_deep_policy(lay33, 8, 8).pack(lay33, tab33, device='cuda:0')
    spec32, tab32, lay32, pol32, pt32, eng32 = _setup('b32', E, False, H=(32, 32))
    th_spec = golden('g2020_cz1').spec()
    thermal = StepEngine(th_spec.episode_tables(0), E, f64_maps=False)
    assert not thermal.lean
    with pytest.raises(ValueError):                                             # the packer: a thermal building's observations / action columns
        make_deep_policy(ObservationLayout(th_spec, 'current', True), 8, 8).pack(ObservationLayout(th_spec, 'current', True), th_spec.episode_tables(0))
    # ... and deep tables that DO match a thermal engine's shape (nine 2022 buildings over as many rows, the bounds of its 25 action columns): the library's
    th_rows = th_spec.episode_tables(0, window=(th_spec.simulation_start_time_step, th_spec.simulation_start_time_step + pt.n_rows - 1))
    thermal9 = StepEngine(th_rows, E, f64_maps=False)
    spec9 = golden('g2022_all').spec(buildings=list(range(9)))
    lay9 = ObservationLayout(spec9, 'current', True)
    pt9 = make_deep_policy(lay9, 8, 8).pack(lay9, spec9.episode_tables(0), device='cuda:0')
    pt9.act_low, pt9.act_high = (torch.full((thermal9.n_act_cols,), v, device='cuda') for v in (-1.0, 1.0))
    assert not thermal9.lean and (pt9.n_rows, pt9.n_bldg) == (thermal9.n_ts_rows, thermal9.n_bldg) == (pt.n_rows, 9)
    lean_pt32 = make_policy(lay32, 16).pack(lay32, tab32, device='cuda:0')
    route = 'no KPI kernel for a policy with two hidden layers.*replay its action plane.*kpi=True'
    cases = [('MARL', StepEngine(tab, E, reward='MARL', f64_maps=False), pt, {}, _lib.EngineError, 'clpd_rollout_mlp_f32: reward kind CLR_MARL.*no barrier'),
             ('kpi engine', StepEngine(tab, E, f64_maps=False, kpi=True), pt, {}, _lib.EngineError, 'clpd_rollout_mlp_f32.*CLD_KPI'),
             ('kpi=True on a kpi engine', StepEngine(tab, E, f64_maps=False, kpi=True), pt, {'kpi': True}, NotImplementedError, route),
             ('kpi=True', plain, pt, {'kpi': True}, NotImplementedError, route),
             ('chunked=True', plain, pt, {'chunked': True}, ValueError, 'no building-chunked policy kernel for DeepPolicyTables at all'),
             ('f64_maps=True', StepEngine(tab, E, f64_maps=True), pt, {}, _lib.EngineError, 'clpd_rollout_mlp_f32.*CLD_F64_MAPS'),
             ('thermal district', thermal, pt, {}, ValueError, 'policy tables (are packed for|hold)'),
             ('thermal district, tables of its shape', thermal9, pt9, {}, _lib.EngineError, 'clpd_rollout_mlp_f32: only battery \\+ PV districts \\(CLD_LEAN\\)'),
             ('PolicyTables of another engine', plain, lean_pt32, {}, ValueError, 'policy tables are packed for'),
             ('33 buildings', StepEngine(tab33, E, f64_maps=False), pt33, {}, _lib.EngineError, 'clpd_rollout_mlp_f32: n_bldg=33 > 32'),
             ('32 buildings at 32 x 32', eng32, pt32, {}, _lib.EngineError, 'deep policy rollout would need 164864 bytes of LDS'),
             ('32 buildings on the matrix cores', eng32, make_deep_policy(lay32, 4, 4).pack(lay32, tab32, device='cuda:0', matrix_cores=True), {},
              _lib.EngineError, 'deep policy rollout would need 164864 bytes of LDS'),
             ('tables of another engine', plain, pt32, {}, ValueError, 'policy tables are packed for'),
             ('deep tables of 33 buildings', eng32, pt33, {}, ValueError, 'policy tables are packed for')]
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
    # the one-hidden-layer tables still go to THEIR kernel on the same engine, the deep ones to theirs
    lean_pt = make_policy(layout, 16).pack(layout, tab, device='cuda:0')
    plain.rollout_policy(K, lean_pt)
    assert plain.last_kernels.startswith('cl_rollout_policy_kernel<'), plain.last_kernels
    plain.reset()
    _roll(plain, pt, K)
    _roll(plain, pol.pack(layout, tab, device='cuda:0', matrix_cores=True), K)
