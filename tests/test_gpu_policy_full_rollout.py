"""The closed-loop policy rollout of thermal districts on the GPU (`StepEngine.rollout_policy` / `VectorCityLearnEnv.rollout_policy` with a
`StorageMLPPolicy`: one launch of `cl_rollout_full_policy_kernel`, csrc/cl_policy_full.h) on g2020_cz1: (a) its actions teacher-forced against
the float64 MLP, (b) its trajectory replayed through `step()`, (c) free-running against the CPU oracle, (d) launch splitting and checkpoints bit
for bit, (e) episode windows x parameter sets x env offsets bit for bit, (f) noise bounds and determinism, (g) the env-level call against
`capture_rollout` with the same MLP in torch, (h) the geometry edges -- and (a) - (e), (h) again on the OUTAGE districts of
tests/policy_full_util.py (`outage_district`: the same buildings with chosen outage rows and charged tanks), where the waves of a workgroup take
`clv::unit_step<.., OUT = true>` and `OUT = false` side by side at the same step.  Weights: tests/policy_full_util.py (scale fixed by
tests/test_policy_full_host.py's conditioning test).  The float64 chain and MARL exist at one env per lane only: where a case asks for two, the
chain runs its one."""
import numpy as np
import pytest
import torch

from golden_util import check_worst, golden, record_worst
from citylearn_amd import _lib, policy
from citylearn_amd.engine import StepEngine
from citylearn_amd.observations import ObservationLayout
from policy_full_util import THERMAL_PLANES, host_closed_loop, make_storage_policy, outage_mask, replay_noise, thermal_district
from policy_util import HostObservations, f32_torch_deviation

pytestmark = pytest.mark.gpu

KINDS = ['RewardFunction', 'MARL', 'IndependentSACReward', 'SolarPenaltyReward']
A, R, N, S = policy.CLPF_T_ACTION, policy.CLPF_T_REWARD, policy.CLPF_T_NET, policy.CLPF_T_SOC
NA = policy.CLPF_NA


def _net_is_zero_on_outage_rows_only(tab, traj, row0=0):
    """On a district with outage rows: the recorded net is exactly 0 on every outage (row, building) pair -- for every env -- and on no other."""
    m = torch.as_tensor(tab.outage[row0:row0 + traj.shape[0]] > 0, device=traj.device)
    assert torch.equal(traj[:, N] == 0, m[:, :, None].expand(-1, -1, traj.shape[3]))
    return bool(m.any())


def _setup(E, f64='chain', kind='RewardFunction', H=16, sigma=None, n_sets=1, normalize=True, set_of_block=None, district='g2020_cz1', vec=0, **kw):
    spec = thermal_district(district)
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', normalize)
    pol = make_storage_policy(layout, H, n_sets=n_sets, seed=H, sigma=sigma)
    pt = pol.pack(layout, tab, device='cuda:0', set_of_block=set_of_block)
    if vec and not (f64 == 'chain' or kind == 'MARL'):
        kw['tuning'] = dict(vec=vec)
    eng = StepEngine(tab, E, reward=kind, f64_maps=f64, **kw)
    eng.trace_kernels()
    return spec, tab, layout, pol, pt, eng


def _roll(eng, pt, K, seed=0):
    ret = torch.zeros(eng.n_env, device='cuda')
    traj = torch.full((K, policy.CLPF_NT, eng.n_bldg, eng.n_env), float('nan'), device='cuda')
    eng.rollout_policy(K, pt, seed=seed, ret_env=ret, traj=traj)
    assert not torch.isnan(traj).any()
    return ret, traj


def _teacher_forced(tab, layout, pol, pt, traj, seed=0, row0=0, env_offset=0):
    """(kernel's worst |action - float64 MLP| over the heads that exist, a float32 torch evaluation's, on the recorded inputs of every step)."""
    K, E = traj.shape[0], traj.shape[3]
    hobs = HostObservations(layout, tab, THERMAL_PLANES)
    tr = traj.cpu().numpy().astype(np.float64)
    xs = [hobs.at(row0, None, reset=True, E=E)] + [hobs.at(row0 + k, *tr[k - 1, S:S + 4], tr[k - 1, N]) for k in range(1, K)]
    x = np.stack(xs)
    z = None
    if np.any(pt.sigma_bldg > 0):
        z = np.stack([replay_noise(pt, seed, E, k, env_offset) for k in range(K)])
    ref = pol.actions_host(x, pt, noise=z)                                            # [K, E, B, 4]
    got = tr[:, A:A + NA].transpose(0, 3, 2, 1)                                       # [K, 4, B, E] -> [K, E, B, 4]
    assert not got[:, :, pt.cols < 0].any()                                           # a head without a column: plane written as 0
    return float(np.abs(got - ref).max()), f32_torch_deviation(pol, x, pt, device='cuda', noise=z)


def _scatter(pt, planes, n_act_cols):
    """[4, B, E] head planes -> [n_act_cols, E]"""
    acts = torch.zeros((n_act_cols, planes.shape[2]), device=planes.device)
    b, h = np.nonzero(pt.cols >= 0)
    acts[torch.as_tensor(pt.cols[b, h], device=planes.device)] = planes[torch.as_tensor(h, device=planes.device), torch.as_tensor(b, device=planes.device)]
    return acts


def _replay(tab, pt, eng, ret, traj, kind, f64):
    """(b): the recorded actions fed step by step to a second engine's `step()` -- tests/test_gpu_policy_rollout.py::test_b's tolerances."""
    K, E = traj.shape[0], traj.shape[3]
    ref = StepEngine(tab, E, reward=kind, f64_maps=f64)
    ref.trace_kernels()
    ret_ref = torch.zeros(E, device='cuda')
    worst = {}
    for k in range(K):
        ref.step(_scatter(pt, traj[k, A:A + NA], ref.n_act_cols))
        ret_ref += ref.district_reward
        for key, got, want in (('soc', traj[k, S:S + 4], ref.state[[0, 3, 4, 5]]), ('net', traj[k, N], ref.net), ('reward', traj[k, R], ref.reward_bldg)):
            worst[key] = max(worst.get(key, 0.0), float(((got - want).abs() / (1e-4 + 1e-4 * want.abs())).max()))
        torch.testing.assert_close(traj[k, S:S + 4], ref.state[[0, 3, 4, 5]], rtol=2e-6, atol=2e-6)
        torch.testing.assert_close(traj[k, N], ref.net, rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(traj[k, R], ref.reward_bldg, rtol=2e-5, atol=2e-5)
    if tab.outage.any():
        assert _net_is_zero_on_outage_rows_only(tab, traj) and ref.last_kernels.startswith('cl_step_full_')
        record_worst(worst, f'thermal policy rollout vs single steps under an outage B={eng.n_bldg} {kind} E={E} f64_maps={f64}')
    torch.testing.assert_close(eng.state[:6], ref.state[:6], rtol=2e-6, atol=2e-6)
    torch.testing.assert_close(eng.out_bldg[:2], ref.out_bldg[:2], rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(eng.out_env, ref.out_env, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(ret, ret_ref, rtol=1e-5, atol=1e-3)
    assert eng.t == K and torch.equal(traj[K - 1, N], eng.net) and torch.equal(traj[K - 1, S], eng.soc) and torch.equal(traj[K - 1, R], eng.reward_bldg)


@pytest.mark.parametrize('sigma', [None, 0.1])
@pytest.mark.parametrize('H', [4, 16, 32])
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('E,vec', [(64, 1), (260, 2), (4096, 0)])
def test_a_teacher_forced_actions(E, vec, f64, H, sigma):
    """(a) Every recorded action of every head recomputed in float64 from the previous step's recorded planes (the reset observation at step 0;
    the noise replayed from the Philox stream).  Gate: 4 x the worst deviation of a float32 torch evaluation of the unsplit MLP on the same
    inputs, the project's gate for this tanh form.  Measured on MI355X: profiles/policy_full_parity.md; both figures are printed here."""
    _check_a(E, vec, f64, H, sigma, 'g2020_cz1')


def _check_a(E, vec, f64, H, sigma, district):
    spec, tab, layout, pol, pt, eng = _setup(E, f64, H=H, sigma=sigma, vec=vec, district=district)
    K = 24
    _, traj = _roll(eng, pt, K, seed=11)
    want_vec = 1 if f64 == 'chain' else (vec or 2)
    assert eng.last_kernels == f"cl_rollout_full_policy_kernel<{want_vec}, {2 if f64 == 'chain' else 0}, false>", eng.last_kernels
    dev_kernel, dev_f32 = _teacher_forced(tab, layout, pol, pt, traj, seed=11)
    print(f'teacher-forced {district} E={E} vec={want_vec} f64={f64} H={H} sigma={sigma}: kernel {dev_kernel:.3e}  float32 torch {dev_f32:.3e}  ratio {dev_kernel / dev_f32:.2f}')
    assert dev_f32 > 0 and dev_kernel <= 4.0 * dev_f32, (dev_kernel, dev_f32)
    return tab, traj, dev_kernel, dev_f32


@pytest.mark.parametrize('H', [4, 32])
@pytest.mark.parametrize('f64', ['chain', False])
def test_a_teacher_forced_actions_under_an_outage(f64, H):
    """(a) on the nine-building outage district at E = 260 (ragged tile; two envs per lane on the fp32 map), noise on: after an outage row the
    observation carries a net of exactly 0 and socs the outage unit wrote."""
    tab, traj, dev_kernel, dev_f32 = _check_a(260, 2, f64, H, 0.1, 'g2020_cz1_outage')
    assert _net_is_zero_on_outage_rows_only(tab, traj)
    record_worst({'kernel': dev_kernel, 'float32_torch': dev_f32, 'ratio': dev_kernel / dev_f32}, f'thermal policy teacher-forced under an outage f64_maps={f64} H={H}')


@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('E', [64, 260])
@pytest.mark.parametrize('kind', KINDS)
def test_b_replay_through_single_steps(kind, E, f64):
    """(b) K = 30 (across a day boundary), noise on: all six state planes, net, reward, the district sums and the return."""
    _check_b(kind, E, f64, 'g2020_cz1')


@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('E', [64, 260])
@pytest.mark.parametrize('kind', KINDS)
def test_b_replay_through_single_steps_under_an_outage(kind, E, f64):
    """(b) on the nine-building outage district, same tolerances; also: net exactly 0 on the outage (row, building) pairs and on no other
    (`_replay`).  The single-step reference is pinned on this district by tests/test_gpu_outage_thermal.py."""
    _check_b(kind, E, f64, 'g2020_cz1_outage')


def _check_b(kind, E, f64, district):
    spec, tab, layout, pol, pt, eng = _setup(E, f64, kind, sigma=0.1, district=district)
    ret, traj = _roll(eng, pt, 30, seed=5)
    marl = 'true' if kind == 'MARL' else 'false'
    assert eng.last_kernels == f"cl_rollout_full_policy_kernel<{1 if f64 == 'chain' or kind == 'MARL' else 2}, {2 if f64 == 'chain' else 0}, {marl}>", eng.last_kernels
    _replay(tab, pt, eng, ret, traj, kind, f64)


@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('kind', KINDS)
def test_c_free_running_against_the_cpu(kind, f64):
    """(c) K = 48 from reset: the host loop of `COracle.step` + `actions_host` (float64) against one launch, at the plain bar 1e-4 + 1e-4 |ref|
    on soc, cs, ds, degraded capacity, net, reward and district net."""
    _check_c(kind, f64, 'g2020_cz1')


@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('kind', KINDS)
def test_c_free_running_against_the_cpu_under_an_outage(kind, f64):
    """(c) on the nine-building outage district, same bar.  The tanks start charged: cs AND ds move (on the plain district the ds gate is
    vacuous), and all eleven outage rows of a building are inside the launch.  The same oracle loop on the PLAIN district differs from this
    one by up to 42 kWh of net from step 5 on, 4 x 10^5 x the bar (tests/test_policy_full_host.py): a kernel that skipped the branch fails."""
    _check_c(kind, f64, 'g2020_cz1_outage')


def _check_c(kind, f64, district):
    E, K = 64, 48
    spec, tab, layout, pol, pt, eng = _setup(E, f64, kind, H=16, district=district)
    want = host_closed_loop(spec, tab, layout, pol, pt, K, E, reward=kind)
    _, traj = _roll(eng, pt, K)
    tr = traj.cpu().numpy().astype(np.float64)
    bar = lambda got, ref: float((np.abs(got - ref) / (1e-4 + 1e-4 * np.abs(ref))).max())
    worst = {'soc': bar(tr[:, S], want['soc']), 'cs': bar(tr[:, S + 1], want['cs']), 'ds': bar(tr[:, S + 3], want['ds']),
             'net': bar(tr[:, N], want['net']), 'reward': bar(tr[:, R], want['reward']),
             'district_net': bar(tr[:, N].sum(axis=1), want['dnet']),
             'degraded_capacity': bar(eng.degraded_capacity.cpu().numpy(), want['degcap'][-1])}
    print(f'free-running {district} {kind} f64={f64}:', {k: round(v, 4) for k, v in worst.items()})
    assert np.abs(want['cs']).max() > 0.05 and not tr[:, S + 2].any()
    assert eng.last_kernels.startswith('cl_rollout_full_policy_kernel<'), eng.last_kernels
    if district == 'g2020_cz1':
        check_worst(worst, f'thermal policy rollout {kind} f64={f64}')
        return
    assert np.ptp(want['ds']) > 0.1 and np.ptp(want['cs']) > 0.1 and _net_is_zero_on_outage_rows_only(tab, traj)
    m = outage_mask(tab, K)
    assert np.array_equal(m.sum(axis=0), [0 if i % 3 == 2 else 11 for i in range(9)]) and not want['net'][m].any()
    check_worst(worst, f'thermal policy rollout under an outage {kind} f64={f64}')


@pytest.mark.parametrize('f64', ['chain', False])
def test_d_split_launches_and_checkpoint_are_bit_identical(f64):
    """(d) Launches of 1, 5, 24 and 25 steps from t0 = 0 equal one 55-step launch bit for bit (the previous net travels through out_bldg, t == 0
    uses net_reset), with a checkpoint restored into a fresh engine between two of them; MARL, noise on."""
    _check_d(f64, 'g2020_cz1')


@pytest.mark.parametrize('f64', ['chain', False])
def test_d_split_launches_and_checkpoint_are_bit_identical_under_an_outage(f64):
    """(d) on the nine-building outage district: the boundary at step 6 falls inside the first outage of buildings 0 and 1 (the net the next
    launch reads back from out_bldg is an outage row's 0), the first launch meets no outage row and the last one rows 40 .. 41."""
    _check_d(f64, 'g2020_cz1_outage')


def _check_d(f64, district):
    E = 320
    spec, tab, layout, pol, pt, one = _setup(E, f64, 'MARL', sigma=0.1, district=district)
    ret1, traj1 = _roll(one, pt, 55, seed=3)
    assert one.last_kernels == f"cl_rollout_full_policy_kernel<1, {2 if f64 == 'chain' else 0}, true>", one.last_kernels
    eng = StepEngine(tab, E, reward='MARL', f64_maps=f64)
    ret, parts = torch.zeros(E, device='cuda'), []
    for n, K in enumerate((1, 5, 24, 25)):
        if n == 2:
            sd = eng.state_dict()
            eng = StepEngine(tab, E, reward='MARL', f64_maps=f64)
            eng.load_state_dict(sd)
        traj = torch.empty((K, policy.CLPF_NT, eng.n_bldg, E), device='cuda')
        eng.rollout_policy(K, pt, seed=3, ret_env=ret, traj=traj)
        parts.append(traj)
    assert eng.t == 55 and torch.equal(torch.cat(parts), traj1)
    assert torch.equal(eng.state, one.state) and torch.equal(eng.out_bldg[:2], one.out_bldg[:2]) and torch.equal(eng.out_env, one.out_env)
    torch.testing.assert_close(ret, ret1, rtol=1e-6, atol=1e-4)               # (four partial sums instead of one)
    if district != 'g2020_cz1':
        m = outage_mask(tab, 55)
        assert _net_is_zero_on_outage_rows_only(tab, traj1) and not m[:1].any() and m[5, 0] and m[6, 0] and m[6, 1] and m[30:].any()


@pytest.mark.parametrize('f64', ['chain', False])
def test_e_windows_sets_and_env_offsets(f64):
    """(e) Two env blocks with different episode windows AND different parameter sets in one launch: each block equals, bit for bit, an engine
    of its own with that window, that set and its env offset (noise on: the half batches reproduce the whole batch's streams)."""
    _check_e(f64, 'g2020_cz1')


@pytest.mark.parametrize('f64', ['chain', False])
def test_e_windows_sets_and_env_offsets_under_an_outage(f64):
    """(e) on the nine-building outage district: block 0 (rows 0 .. 23) meets outage rows and block 1 (rows 131 .. 154) none -- workgroups of one
    launch that take different branches at the same step index."""
    _check_e(f64, 'g2020_cz1_outage')


def _check_e(f64, district):
    spec = thermal_district(district)
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    pol = make_storage_policy(layout, 16, n_sets=2, seed=2, sigma=0.1)
    K, n_steps, rows = 24, 200, [0, 131]
    whole = StepEngine(tab, 512, f64_maps=f64, n_steps=n_steps, env_row0=rows)
    whole.trace_kernels()
    _, traj = _roll(whole, pol.pack(layout, tab, device='cuda:0', set_of_block=[0, 1]), K, seed=9)
    assert whole.last_kernels == f"cl_rollout_full_policy_kernel<{1 if f64 == 'chain' else 2}, {2 if f64 == 'chain' else 0}, false>", whole.last_kernels
    assert not torch.equal(traj[:, A:A + NA, :, :256], traj[:, A:A + NA, :, 256:])
    if district != 'g2020_cz1':
        assert _net_is_zero_on_outage_rows_only(tab, traj[:, :, :, :256], rows[0]) and not _net_is_zero_on_outage_rows_only(tab, traj[:, :, :, 256:], rows[1])
    for g in range(2):
        part = StepEngine(tab, 256, f64_maps=f64, n_steps=n_steps, env_row0=[rows[g]], env_offset=256 * g)
        _, tr = _roll(part, pol.pack(layout, tab, device='cuda:0', set_of_block=[g]), K, seed=9)
        sl = slice(256 * g, 256 * (g + 1))
        assert torch.equal(tr, traj[:, :, :, sl]), g
        assert torch.equal(part.state, whole.state[:, :, sl]) and torch.equal(part.out_env, whole.out_env[:, sl])
    # ... and the actions of block 1 are its window's and its set's: teacher-forced like (a)
    single = policy.StorageMLPPolicy(pol.w1[1:2], pol.b1[1:2], pol.w2[1:2], pol.b2[1:2], sigma=0.1)
    dev_kernel, dev_f32 = _teacher_forced(tab, layout, single, single.pack(layout, tab), traj[:, :, :, 256:], seed=9, row0=rows[1], env_offset=256)
    print(f'window 1 / set 1 teacher-forced: kernel {dev_kernel:.3e}  float32 torch {dev_f32:.3e}')
    assert dev_kernel <= 4.0 * dev_f32


def test_f_noise():
    """(f) sigma > 0 (large: 0.8): every action inside its OWN column's bounds (every building has its own), both bounds reached; the same seed
    gives the same trajectory, another seed another; with a per-column sigma the zero entries leave their head deterministic -- equal over the
    envs at step 0, where every env sees the reset observation, and equal to the float64 MLP without noise at every step."""
    spec, tab, layout, pol, pt, eng = _setup(512, sigma=0.8)
    _, traj = _roll(eng, pt, 24, seed=1)
    act = traj[:, A:A + NA]
    has = torch.as_tensor(pt.cols >= 0, device='cuda').t()[None, :, :, None]                     # [1, 4, B, 1]
    lo = torch.as_tensor(pt.low_bldg.T, dtype=torch.float32, device='cuda')[None, :, :, None]
    hi = torch.as_tensor(pt.high_bldg.T, dtype=torch.float32, device='cuda')[None, :, :, None]
    assert bool(((act >= lo) & (act <= hi) | ~has).all()) and not bool(act[(~has).expand_as(act)].any())
    assert bool(((act == lo) & has).any()) and bool(((act == hi) & has).any())
    assert float(pt.high_bldg[pt.cols >= 0].min()) < 0.1 < 0.9 < float(pt.high_bldg.max())
    _, again = _roll(_setup(512, sigma=0.8)[5], pt, 24, seed=1)
    _, other = _roll(_setup(512, sigma=0.8)[5], pt, 24, seed=2)
    assert torch.equal(again, traj) and not torch.equal(other[:, A:A + NA], act)
    # per-column sigma: the cooling heads (and building 4 altogether) without noise
    spec, tab, layout, pol, pt, eng = _setup(512)
    sig = np.full(25, 0.2)
    quiet = pt.cols[:, policy.CLPF_A_CS].tolist() + pt.cols[4][pt.cols[4] >= 0].tolist()
    sig[quiet] = 0.0
    pol = policy.StorageMLPPolicy(pol.w1, pol.b1, pol.w2, pol.b2, sigma=sig)
    pt = pol.pack(layout, tab, device='cuda:0')
    _, traj = _roll(eng, pt, 12, seed=4)
    first = traj[0, A:A + NA]
    same = (first == first[:, :, :1]).all(dim=2).cpu().numpy().T                                 # [B, 4]
    assert np.array_equal(same, (pt.sigma_bldg == 0.0)), same
    dev_kernel, dev_f32 = _teacher_forced(tab, layout, pol, pt, traj, seed=4)
    assert dev_kernel <= 4.0 * dev_f32, (dev_kernel, dev_f32)


@pytest.mark.parametrize('normalize', [True, False])
def test_g_env_level_equals_capture_rollout_with_the_torch_mlp(normalize):
    """(g) `VectorCityLearnEnv.rollout_policy(policy, K, record=True)` against `capture_rollout` driven by `torch_policy` over
    `observations='tensor'`, at the tolerances of tests/test_gpu_policy_rollout.py::test_g: per-step actions at the teacher-forced tolerance
    (4 x a float32 evaluation's deviation, measured here on the recorded inputs) widened by what the two paths' state tolerance (2e-6 on the
    socs, 2e-5 on net, relative + absolute) can move an action through the five dependent weights, and once more for the float32 torch
    policy's own deviation; returns at rtol 1e-5 / atol 1e-3.  `kpi=True` names the gap."""
    from citylearn_amd.vector_env import VectorCityLearnEnv
    g = golden('g2020_cz1')
    E, K = 256, 24
    a, b = (VectorCityLearnEnv(g.schema_path, E, observations='tensor', normalize_observations=normalize) for _ in range(2))
    a.engine.trace_kernels()
    pol = make_storage_policy(a.layout, 16, seed=4)
    with pytest.raises(NotImplementedError, match='KPI'):
        a.rollout_policy(pol, K, kpi=True)
    ret, traj = a.rollout_policy(pol, K, record=True)
    assert a._t == K == a.engine.t and traj.shape == (K, policy.CLPF_NT, a.n_bldg, E)
    assert a.engine.last_kernels.startswith('cl_rollout_full_policy_kernel<') and a.engine.last_kernels.count('kernel') == 1, a.engine.last_kernels
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
    print(f'env level normalize={normalize}: |action difference| {worst:.3e}, tolerance {tol:.3e} (float32 deviation {dev_f32:.3e}, state term {widen:.3e})')
    assert worst <= tol
    torch.testing.assert_close(ret, rewards.sum(dim=0) if rewards.dim() == 2 else rewards.sum(dim=(0, 1)), rtol=1e-5, atol=1e-3)
    torch.testing.assert_close(a.engine.state, b.engine.state, rtol=2e-6, atol=2e-6)


@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('name', ['t1', 't2', 't16', 't1_outage', 't2_outage', 't16_outage'])
def test_h_geometry_edges_replayed(name, f64):
    """(h) One building (nw = 1: the wave owns every reduction row alone); two, one with and one without DHW storage; sixteen, the kernel's limit
    (nw = 16) -- each replayed through `step()` like (b) at E = 64, and teacher-forced like (a).  Their outage versions: the one wave of
    't1_outage' is at times on an outage row alone (every district sum of that step is exactly 0), both buildings of 't2_outage' have outage
    rows, 't16_outage' has five buildings without."""
    spec, tab, layout, pol, pt, eng = _setup(64, f64, sigma=0.1, district=name)
    assert eng.n_bldg == {'t1': 1, 't2': 2, 't16': 16}[name.split('_')[0]]
    if name.startswith('t2'):
        assert pt.cols[0, policy.CLPF_A_DS] >= 0 and pt.cols[1, policy.CLPF_A_DS] < 0
    ret, traj = _roll(eng, pt, 30, seed=7)
    assert eng.last_kernels == f"cl_rollout_full_policy_kernel<{1 if f64 == 'chain' else 2}, {2 if f64 == 'chain' else 0}, false>", eng.last_kernels
    _replay(tab, pt, eng, ret, traj, 'RewardFunction', f64)
    dev_kernel, dev_f32 = _teacher_forced(tab, layout, pol, pt, traj, seed=7)
    assert dev_kernel <= 4.0 * dev_f32, (dev_kernel, dev_f32)


def test_h_seventeen_buildings_are_refused_with_their_message():
    spec, tab, layout, pol, pt, eng = _setup(64, False, district='t17')
    state = eng.state.clone()
    with pytest.raises(_lib.EngineError, match='n_bldg=17 > 16 would be a building-chunked launch'):
        eng.rollout_policy(4, pt)
    assert torch.equal(eng.state, state)
    # ... and a battery + PV district with the storage tables is sent to the other library by name
    lean = StepEngine(golden('g2022_all').spec().episode_tables(0), 64)
    lean_pt = policy.StoragePolicyTables(pt.pre, pt.dep, pt.out, pt.net_reset, pt.act_low[:17].contiguous(), pt.act_high[:17].contiguous(), None, None,
                                         pt.cols, pt.low_bldg, pt.high_bldg, pt.sigma_bldg, 0, 0)
    lean_pt.n_rows = lean.n_ts_rows
    with pytest.raises(_lib.EngineError, match='clpol_rollout_mlp_f32'):
        lean.rollout_policy(4, lean_pt)
