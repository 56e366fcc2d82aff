"""The closed-loop policy rollout on the GPU (`StepEngine.rollout_policy` / `VectorCityLearnEnv.rollout_policy`: one launch of
`cl_rollout_policy_kernel`, csrc/cl_policy.h) on g2022_all: (a) its actions teacher-forced against the float64 MLP, (b) its trajectory
replayed through `step()`, (c) free-running against the CPU oracle, (d) launch splitting and checkpoints bit for bit, (e) episode windows x
parameter sets x env offsets bit for bit, (f) noise bounds and determinism, (g) the env-level call against `capture_rollout` with the same MLP in
torch, (h) one launch + the KPI replay recipe.  Weights: tests/policy_util.py (scale fixed by tests/test_policy_host.py's conditioning test)."""
import numpy as np
import pytest
import torch

from golden_util import check_worst, golden
from citylearn_amd import abi, policy
from citylearn_amd.engine import StepEngine
from citylearn_amd.observations import ObservationLayout
from policy_util import HostObservations, f32_torch_deviation, host_closed_loop, make_policy

pytestmark = pytest.mark.gpu

KINDS = ['RewardFunction', 'MARL', 'IndependentSACReward', 'SolarPenaltyReward']
A, R, N, S = policy.CLPOL_T_ACTION, policy.CLPOL_T_REWARD, policy.CLPOL_T_NET, policy.CLPOL_T_SOC


def _setup(E, f64='chain', kind='RewardFunction', H=16, sigma=None, n_sets=1, normalize=True, set_of_block=None, **kw):
    spec = golden('g2022_all').spec()
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', normalize)
    pol = make_policy(layout, H, n_sets=n_sets, seed=H, sigma=sigma)
    pt = pol.pack(layout, tab, device='cuda:0', set_of_block=set_of_block)
    eng = StepEngine(tab, E, reward=kind, f64_maps=f64, **kw)
    eng.trace_kernels()
    return spec, tab, layout, pol, pt, eng


def _roll(eng, pt, K, seed=0):
    ret = torch.zeros(eng.n_env, device='cuda')
    traj = torch.full((K, policy.CLPOL_NT, eng.n_bldg, eng.n_env), float('nan'), device='cuda')
    eng.rollout_policy(K, pt, seed=seed, ret_env=ret, traj=traj)
    assert not torch.isnan(traj).any()
    return ret, traj


def _teacher_forced(eng, tab, layout, pol, pt, traj, seed=0, row0=0, env_offset=0):
    """(kernel's worst |action - float64 MLP|, a float32 torch evaluation's, on the recorded inputs of every step)."""
    K, E = traj.shape[0], traj.shape[3]
    hobs = HostObservations(layout, tab)
    tr = traj.cpu().numpy().astype(np.float64)
    xs = [hobs.at(row0, np.zeros((eng.n_bldg, E)), None, reset=True)] + [hobs.at(row0 + k, tr[k - 1, S], tr[k - 1, N]) for k in range(1, K)]
    x = np.stack(xs)
    z = None
    sig = pt.sigma_bldg
    if np.any(sig > 0):
        z = np.stack([np.stack([policy.noise_host(seed, env_offset + np.arange(E), pt.es_cols[b], k) for b in range(eng.n_bldg)], axis=1)
                      for k in range(K)])
    ref = pol.actions_host(x, noise=z, tables=pt)                                     # [K, E, B]
    dev_kernel = float(np.abs(tr[:, A].transpose(0, 2, 1) - ref).max())
    return dev_kernel, f32_torch_deviation(pol, x, pt, device='cuda', noise=z)


@pytest.mark.parametrize('sigma', [None, 0.1])
@pytest.mark.parametrize('H', [4, 16, 32])
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('E,vec', [(64, 1), (260, 2), (4096, 0)])
def test_a_teacher_forced_actions(E, vec, f64, H, sigma):
    """(a) Every recorded action recomputed in float64 from the recorded inputs (soc / net of the step before; the reset observation at step 0;
    the noise replayed from the Philox stream).  Gate: 4 x the worst deviation of a float32 torch evaluation of the unsplit MLP on the same
    inputs -- the kernel adds v_exp_f32 / v_rcp_f32 at 1 ulp each and the split's one extra rounding, nothing grosser.  Measured on MI355X
    (profiles/policy_rollout_parity.md): see that file; both figures are printed here."""
    spec, tab, layout, pol, pt, eng = _setup(E, f64, H=H, sigma=sigma, tuning=dict(vec=vec) if vec else None)
    K = 24
    _, traj = _roll(eng, pt, K, seed=11)
    dev_kernel, dev_f32 = _teacher_forced(eng, tab, layout, pol, pt, traj, seed=11)
    print(f'teacher-forced E={E} vec={vec} f64={f64} H={H} sigma={sigma}: kernel {dev_kernel:.3e}  float32 torch {dev_f32:.3e}  ratio {dev_kernel / dev_f32:.2f}')
    assert dev_f32 > 0 and dev_kernel <= 4.0 * dev_f32, (dev_kernel, dev_f32)


@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('E', [64, 192, 260, 4096])
@pytest.mark.parametrize('kind', KINDS)
def test_b_replay_through_single_steps(kind, E, f64):
    """(b) The recorded actions fed step by step to a second engine's `step()`: state, last outputs, district sums, return and the trajectory
    planes at the tolerances of two paths on one trajectory (tests/test_gpu_rollout_kpi.py::_compare_step_outputs)."""
    spec, tab, layout, pol, pt, eng = _setup(E, f64, kind, sigma=0.1)
    K = 30
    ret, traj = _roll(eng, pt, K, seed=5)
    ref = StepEngine(tab, E, reward=kind, f64_maps=f64)
    ret_ref = torch.zeros(E, device='cuda')
    for k in range(K):
        ref.step(traj[k, A].contiguous())
        ret_ref += ref.district_reward
        torch.testing.assert_close(traj[k, S], ref.soc, rtol=2e-6, atol=2e-6)
        torch.testing.assert_close(traj[k, N], ref.net, rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(traj[k, R], ref.reward_bldg, rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(eng.state, ref.state, rtol=2e-6, atol=2e-6)
    torch.testing.assert_close(eng.out_bldg[:2], ref.out_bldg[:2], rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(eng.out_env, ref.out_env, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(ret, ret_ref, rtol=1e-5, atol=1e-3)
    assert eng.t == K and torch.equal(traj[K - 1, N], eng.net) and torch.equal(traj[K - 1, S], eng.soc) and torch.equal(traj[K - 1, R], eng.reward_bldg)


@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('kind', KINDS)
def test_c_free_running_against_the_cpu(kind, f64):
    """(c) K = 48 from reset: the host loop of `COracle.step` + `actions_host` (float64) against one launch, at the plain bar 1e-4 + 1e-4 |ref|
    on soc, degraded capacity, net, reward and district net."""
    E, K = 64, 48
    spec, tab, layout, pol, pt, eng = _setup(E, f64, kind, H=16)
    want = host_closed_loop(spec, tab, layout, pol, pt, K, E, reward=kind)
    _, traj = _roll(eng, pt, K)
    tr = traj.cpu().numpy().astype(np.float64)
    bar = lambda got, ref: float((np.abs(got - ref) / (1e-4 + 1e-4 * np.abs(ref))).max())
    worst = {'soc': bar(tr[:, S], want['soc']), 'net': bar(tr[:, N], want['net']), 'reward': bar(tr[:, R], want['reward']),
             'district_net': bar(tr[:, N].sum(axis=1), want['dnet']),
             'degraded_capacity': bar(eng.degraded_capacity.cpu().numpy(), want['degcap'][-1])}
    print(f'free-running {kind} f64={f64}:', {k: round(v, 4) for k, v in worst.items()})
    check_worst(worst, f'policy rollout {kind} f64={f64}')


@pytest.mark.parametrize('vec', [1, 2])
@pytest.mark.parametrize('f64', ['chain', False])
def test_d_split_launches_and_checkpoint_are_bit_identical(f64, vec):
    """(d) Launches of 1, 5, 24 and 25 steps from t0 = 0 equal one 55-step launch bit for bit (the previous net travels through out_bldg, t == 0
    uses net_reset), with a checkpoint restored into a fresh engine between two of them; MARL, noise on, both pack widths."""
    E = 320
    spec, tab, layout, pol, pt, one = _setup(E, f64, 'MARL', sigma=0.1, tuning=dict(vec=vec))
    ret1, traj1 = _roll(one, pt, 55, seed=3)
    assert f'cl_rollout_policy_kernel<{vec}, ' in one.last_kernels
    eng = StepEngine(tab, E, reward='MARL', f64_maps=f64, tuning=dict(vec=vec))
    ret, parts = torch.zeros(E, device='cuda'), []
    for n, K in enumerate((1, 5, 24, 25)):
        if n == 2:
            sd = eng.state_dict()
            eng = StepEngine(tab, E, reward='MARL', f64_maps=f64, tuning=dict(vec=vec))
            eng.load_state_dict(sd)
        traj = torch.empty((K, policy.CLPOL_NT, eng.n_bldg, E), device='cuda')
        eng.rollout_policy(K, pt, seed=3, ret_env=ret, traj=traj)
        parts.append(traj)
    assert eng.t == 55 and torch.equal(torch.cat(parts), traj1)
    assert torch.equal(eng.state, one.state) and torch.equal(eng.out_bldg[:2], one.out_bldg[:2]) and torch.equal(eng.out_env, one.out_env)
    torch.testing.assert_close(ret, ret1, rtol=1e-6, atol=1e-4)               # (four partial sums instead of one)


@pytest.mark.parametrize('f64', ['chain', False])
def test_e_windows_sets_and_env_offsets(f64):
    """(e) Two env blocks with different episode windows AND different parameter sets in one launch: each block equals, bit for bit, an engine
    of its own with that window, that set and its env offset (noise on: the half batches reproduce the whole batch's streams)."""
    spec = golden('g2022_all').spec()
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    pol = make_policy(layout, 16, n_sets=2, seed=2, sigma=0.1)
    K, n_steps, rows = 24, 200, [0, 131]
    whole = StepEngine(tab, 512, f64_maps=f64, n_steps=n_steps, env_row0=rows)
    _, traj = _roll(whole, pol.pack(layout, tab, device='cuda:0', set_of_block=[0, 1]), K, seed=9)
    assert not torch.equal(traj[:, A, :, :256], traj[:, A, :, 256:])
    for g in range(2):
        part = StepEngine(tab, 256, f64_maps=f64, n_steps=n_steps, env_row0=[rows[g]], env_offset=256 * g)
        _, tr = _roll(part, pol.pack(layout, tab, device='cuda:0', set_of_block=[g]), K, seed=9)
        sl = slice(256 * g, 256 * (g + 1))
        assert torch.equal(tr, traj[:, :, :, sl]), g
        assert torch.equal(part.state, whole.state[:, :, sl]) and torch.equal(part.out_env, whole.out_env[:, sl])
    # ... and the actions of block 1 are its window's and its set's: teacher-forced like (a)
    single = policy.MLPPolicy(pol.w1[1:2], pol.b1[1:2], pol.w2[1:2], pol.b2[1:2], sigma=0.1)
    dev_kernel, dev_f32 = _teacher_forced(whole, tab, layout, single, single.pack(layout, tab), traj[:, :, :, 256:], seed=9, row0=rows[1], env_offset=256)
    print(f'window 1 / set 1 teacher-forced: kernel {dev_kernel:.3e}  float32 torch {dev_f32:.3e}')
    assert dev_kernel <= 4.0 * dev_f32


def test_f_noise_stays_inside_the_bounds_and_no_noise_is_deterministic():
    """(f) sigma > 0 (large: 0.8): every action inside [low, high], and both bounds reached; sigma = 0: no env differs from env 0 of its block."""
    spec, tab, layout, pol, pt, eng = _setup(512, sigma=0.8)
    _, traj = _roll(eng, pt, 24, seed=1)
    lo, hi = pt.act_low[:eng.n_bldg, None], pt.act_high[:eng.n_bldg, None]
    assert bool((traj[:, A] >= lo).all()) and bool((traj[:, A] <= hi).all())
    assert bool((traj[:, A] == lo).any()) and bool((traj[:, A] == hi).any()) and float(traj[:, A].std()) > 0.3
    spec, tab, layout, pol, pt, eng = _setup(512, sigma=None)
    _, traj = _roll(eng, pt, 24)
    assert torch.equal(traj, traj[:, :, :, :1].expand_as(traj))
    assert float(traj[:, A].abs().max()) > 0.05


@pytest.mark.parametrize('normalize', [True, False])
def test_g_env_level_equals_capture_rollout_with_the_torch_mlp(normalize):
    """(g) `VectorCityLearnEnv.rollout_policy(policy, K, record=True)` against `capture_rollout` driven by the same MLP written in torch over
    `observations='tensor'`: the kernel's inputs are the env's observations.  Per-step actions at the teacher-forced tolerance (4 x a float32
    evaluation's deviation, measured here on the recorded inputs) widened by what the two paths' state tolerance (2e-6 on soc, 2e-5 on net,
    relative + absolute) can move an action: half sum_j |w2_j| (|W1_j,soc| scale_soc tol_soc + |W1_j,net| scale_net tol_net), tanh' <= 1 --
    and once more for the float32 torch policy's own deviation; returns at rtol 1e-5 / atol 1e-3."""
    from citylearn_amd.vector_env import VectorCityLearnEnv
    g = golden('g2022_all')
    E, K = 256, 24
    a, b = (VectorCityLearnEnv(g.schema_path, E, observations='tensor', normalize_observations=normalize) for _ in range(2))
    pol = make_policy(a.layout, 16, seed=4)
    ret, traj = a.rollout_policy(pol, K, record=True)
    assert a._t == K == a.engine.t
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
    w1, w2 = pol._full(a.n_bldg)[0][0], pol._full(a.n_bldg)[2][0]                  # [B, H, n_obs], [B, H]
    tr = traj.cpu().numpy().astype(np.float64)
    tol_soc, tol_net = 2e-6 * (1 + np.abs(tr[:, S]).max()), 2e-5 * (1 + np.abs(tr[:, N]).max())
    g_soc = np.abs(w1 * np.where(hobs.is_term[0], hobs.scale, 0.0)[:, None, :]).sum(axis=2)      # [B, H]
    g_net = np.abs(w1 * np.where(hobs.is_term[1], hobs.scale, 0.0)[:, None, :]).sum(axis=2)
    half = 0.5 * (pt_host.high_bldg - pt_host.low_bldg)
    widen = float((half * (np.abs(w2) * (g_soc * tol_soc + g_net * tol_net)).sum(axis=1)).max())
    tol = 4.0 * dev_f32 + dev_f32 + widen
    got, want = traj[:, A], acts[:, :a.n_bldg]
    worst = float((got - want).abs().max())
    print(f'env level normalize={normalize}: |action difference| {worst:.3e}, tolerance {tol:.3e} (float32 deviation {dev_f32:.3e}, state term {widen:.3e})')
    assert worst <= tol
    torch.testing.assert_close(ret, rewards.sum(dim=0) if rewards.dim() == 2 else rewards.sum(dim=(0, 1)), rtol=1e-5, atol=1e-3)
    torch.testing.assert_close(a.engine.state, b.engine.state, rtol=2e-6, atol=2e-6)


def test_h_one_launch_and_the_kpi_replay_recipe():
    """(h) The call is ONE launch of cl_rollout_policy_kernel; and the docstring's recipe for KPIs runs: the recorded action plane replayed through
    the fused KPI rollout of a kpi=True env gives the same return and the launch sequence's KPIs."""
    from citylearn_amd.vector_env import VectorCityLearnEnv
    g = golden('g2022_all')
    E, K = 256, 24
    env = VectorCityLearnEnv(g.schema_path, E)
    env.engine.trace_kernels()
    pol = make_policy(ObservationLayout(env.spec, 'current', False), 16, seed=8, sigma=0.05)
    ret, traj = env.rollout_policy(pol, K, seed=3, record=True)
    assert env.engine.last_kernels == f"cl_rollout_policy_kernel<1, {2 if env.engine.f64_chain else 0}>", env.engine.last_kernels
    ret2 = env.rollout_policy(pol, K, seed=3)                                  # cached tables, the next K steps
    assert env._t == 2 * K and ret2.shape == (E,) and len(env._policy_tables) == 1
    kenv = VectorCityLearnEnv(g.schema_path, E, kpi=True)
    kret = kenv.rollout(K, actions=traj[:, A].contiguous(), fused=True)
    torch.testing.assert_close(kret, ret, rtol=1e-5, atol=1e-3)
    # ... and its KPIs are those of the same actions replayed as the launch sequence (what test_gpu_rollout_kpi.py pins the fused KPI kernel to;
    # after 24 steps some district KPIs are not defined yet: the same ones in both)
    senv = VectorCityLearnEnv(g.schema_path, E, kpi=True)
    senv.rollout(K, actions=traj[:, A].contiguous(), fused=False)
    (kb, kd), (sb, sd) = kenv.evaluate(), senv.evaluate()
    assert kb and kd and set(kb) == set(sb) and set(kd) == set(sd)
    for name in kb:
        torch.testing.assert_close(kb[name], sb[name], rtol=1e-4, atol=1e-5, equal_nan=True, msg=lambda m: f'{name}: {m}')
    for name in kd:
        torch.testing.assert_close(kd[name], sd[name], rtol=1e-3, atol=1e-4, equal_nan=True, msg=lambda m: f'{name}: {m}')
    assert any(bool(torch.isfinite(v).all()) for v in kd.values())
    with pytest.raises(Exception, match='CLD_KPI'):
        kenv.rollout_policy(pol, 4)


def test_i_changed_weights_and_flexible_loads():
    """`MLPPolicy.update()` makes the env pack again (the cache is keyed by the policy's version): the rollout after it equals a fresh policy
    object with the new weights, bit for bit.  A district with EV chargers under a non-EV reward (CLD_LEAN is set: the library cannot tell) is
    refused by the engine instead of being rolled out without its flexible loads."""
    from citylearn_amd.vector_env import VectorCityLearnEnv
    g = golden('g2022_all')
    E, K = 256, 12
    a, b = VectorCityLearnEnv(g.schema_path, E), VectorCityLearnEnv(g.schema_path, E)
    layout = ObservationLayout(a.spec, 'current', False)
    pol = make_policy(layout, 8, seed=1)
    _, t0 = a.rollout_policy(pol, K, record=True)
    new = make_policy(layout, 8, seed=2)
    pol.update(w1=new.w1, b1=new.b1, w2=new.w2, b2=new.b2)
    a.reset()
    _, t1 = a.rollout_policy(pol, K, record=True)
    _, t2 = b.rollout_policy(new, K, record=True)
    assert torch.equal(t1, t2) and not torch.equal(t1[:, A], t0[:, A])
    ev = golden('g2022_evs')
    eng = StepEngine(ev.spec().episode_tables(0), 64, reward='MARL', ev_seed=1)
    assert eng.flex is not None
    with pytest.raises(NotImplementedError, match='flexible loads'):
        eng.rollout_policy(4, _setup(64)[4])
