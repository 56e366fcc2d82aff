"""The building-chunked closed-loop policy rollout of battery + PV districts on the GPU (`StepEngine.rollout_policy(chunked=True)` with
`PolicyTables` / `VectorCityLearnEnv.rollout_policy` with an `MLPPolicy` on a district of more than 32 buildings: one launch of
`cl_rollout_policy_chunk_kernel`, csrc/cl_policy_chunk.h, and one of `cl_finish_kernel`): (1) against the one-row kernel on districts one
workgroup row holds, (2) its trajectory replayed through `step()`, (3) its actions teacher-forced against the float64 MLP, (4) free-running
against the CPU oracle, (5) launch splitting and checkpoints bit for bit, (6) episode windows x parameter sets x env offsets bit for bit, (7) the
accumulated return, (8) the env-level call against `capture_rollout`, (9) refusals.  Tolerances: tests/test_gpu_policy_rollout.py::test_b's
(2e-6 on action / soc, 2e-5 on net / reward, 1e-4 on out_env, the return at rtol 1e-5 / atol 1e-3); helpers:
tests/test_gpu_rollout_geometry.py (`_step_actions`, `_teacher_forced_driven`); districts: tests/policy_chunk_util.py; weights:
tests/policy_util.py (scale fixed by the conditioning tests of tests/test_policy_host.py and tests/test_policy_chunk_host.py).  Readings on
MI355X: profiles/policy_chunk_parity.md."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from golden_util import check_worst, record_worst
from citylearn_amd import _lib, abi, policy
from citylearn_amd.engine import StepEngine
from citylearn_amd.observations import ObservationLayout
from policy_chunk_util import HET40_UNDRIVEN, chunk_district, default_chunks
from policy_util import HostObservations, host_closed_loop, make_policy
from test_gpu_policy_rollout import A, N, R, S, _teacher_forced
from test_gpu_rollout_geometry import _bar, _prec, _step_actions, _teacher_forced_driven

pytestmark = pytest.mark.gpu

KINDS = ['RewardFunction', 'IndependentSACReward', 'SolarPenaltyReward']          # (MARL couples the buildings inside a step: refused, test 9)
PRECISIONS = [('chain', 1), ('chain', 2), (False, 1), (False, 2)]                  # (f64_maps, envs per lane): every instantiation


@lru_cache(maxsize=None)
def _district(name):
    spec = chunk_district(name)
    return spec, spec.episode_tables(0), ObservationLayout(spec, 'current', True)


@lru_cache(maxsize=None)
def _packed(name, H, sigma, n_sets=1, seed=None, set_of_block=None):
    """The test policy of a district and its device tables, made once per session (at 1024 buildings `pre` is 47 MB)."""
    spec, tab, layout = _district(name)
    pol = make_policy(layout, H, n_sets=n_sets, seed=H if seed is None else seed, sigma=sigma)
    return pol, pol.pack(layout, tab, device='cuda:0', set_of_block=None if set_of_block is None else list(set_of_block))


def _setup(name, E, f64='chain', kind='RewardFunction', H=16, sigma=None, b_chunk=0, nw=0, vec=0, **kw):
    spec, tab, layout = _district(name)
    pol, pt = _packed(name, H, sigma)
    tuning = {k: v for k, v in (('b_chunk', b_chunk), ('nw', nw), ('vec', vec)) if v}
    eng = StepEngine(tab, E, reward=kind, f64_maps=f64, tuning=tuning or None, **kw)
    assert eng.lean
    eng.trace_kernels()
    return spec, tab, layout, pol, pt, eng


def _roll(eng, pt, K, seed=0, chunked=True):
    ret = torch.zeros(eng.n_env, device='cuda')
    traj = torch.full((K, policy.CLPOL_NT, eng.n_bldg, eng.n_env), float('nan'), device='cuda')
    eng.rollout_policy(K, pt, seed=seed, ret_env=ret, traj=traj, **({'chunked': True} if chunked else {}))
    assert not torch.isnan(traj).any()
    return ret, traj


def _names(f64, vec=1):
    """`last_kernels` of a chunked call: the chunk kernel's instantiation and the fold, nothing else."""
    return f'cl_rollout_policy_chunk_kernel<{vec}, {_prec(f64)}>+cl_finish_kernel'


# ---- 1. against the one-row kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('f64,vec', PRECISIONS)
@pytest.mark.parametrize('name,b_chunk,nw', [('b32', 16, 0), ('b32', 12, 0), ('b32', 16, 16), ('het17', 10, 0), ('het17', 9, 0)])
def test_1_one_row_districts_equal_the_one_row_kernel(name, b_chunk, nw, f64, vec, kind):
    """(1) 'b32' cut 16 + 16 (eight full waves), 12 + 12 + 8 (a last chunk with two waves without a building) and 16 + 16 at sixteen waves (ONE
    building per wave: every second seat empty), 'het17' cut 10 + 7 and 9 + 8 (half-filled waves, undriven buildings on both seats), against
    `cl_rollout_policy_kernel` on the same district: same seed, sigma = 0.1, K = 30, E = 260 (ragged tile).  Record, the three battery state
    planes and out_bldg[:2] at test_b's tolerances; out_env at 1e-4 and the return at rtol 1e-5 / atol 1e-3: the district sums are associated
    per chunk first.  Each seat runs the one-row kernel's arithmetic on its building, so the per-building planes are expected to be EQUAL bit for
    bit: recorded per case (`bit_equal`), not gated."""
    E, K = 260, 30
    spec, tab, layout, pol, pt, one = _setup(name, E, f64, kind, sigma=0.1, vec=vec)
    ret1, traj1 = _roll(one, pt, K, seed=5, chunked=False)
    assert one.last_kernels == f'cl_rollout_policy_kernel<{vec}, {_prec(f64)}>', one.last_kernels
    eng = _setup(name, E, f64, kind, sigma=0.1, vec=vec, b_chunk=b_chunk, nw=nw)[5]
    ret, traj = _roll(eng, pt, K, seed=5)
    assert eng.last_kernels == _names(f64, vec), eng.last_kernels
    bs = [abi.CLS_B_SOC, abi.CLS_B_EFF, abi.CLS_B_DEGCAP]                        # the three battery state planes
    torch.testing.assert_close(traj[:, A], traj1[:, A], rtol=2e-6, atol=2e-6)
    torch.testing.assert_close(traj[:, S], traj1[:, S], rtol=2e-6, atol=2e-6)
    torch.testing.assert_close(traj[:, N], traj1[:, N], rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(traj[:, R], traj1[:, R], rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(eng.state[bs], one.state[bs], rtol=2e-6, atol=2e-6)
    torch.testing.assert_close(eng.out_bldg[:2], one.out_bldg[:2], rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(eng.out_env, one.out_env, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(ret, ret1, rtol=1e-5, atol=1e-3)
    bit = torch.equal(traj, traj1) and torch.equal(eng.state[bs], one.state[bs]) and torch.equal(eng.out_bldg[:2], one.out_bldg[:2])
    sums = _bar(eng.out_env, one.out_env)
    print(f'{name} b_chunk={b_chunk} nw={nw} f64={f64} vec={vec} {kind}: per-building planes bit-equal {bit}; district sums {sums:.4f} x the plain bar')
    record_worst({'bit_equal': float(bit), 'district_sums': sums, 'return': float((ret - ret1).abs().max())},
                 f'chunked policy rollout vs one-row kernel {name} b_chunk={b_chunk} nw={nw} {kind} f64_maps={f64} vec={vec}')


# ---- 2. replay through single steps -----------------------------------------------------------------------------------------------------
def _replay(name, tab, pt, eng, ret, traj, kind, f64, label):
    """The recorded actions fed step by step to a second engine's `step()` through the buildings' own action columns: test_b's tolerances.  At
    1024 buildings the return is a float32 sum of ~30 000 rewards on either path: where the two do not meet at rtol 1e-5 / atol 1e-3 there, both
    are held against the float64 sum of the recorded reward plane, the kernel within 4 x the single-step path's own deviation."""
    K, E = traj.shape[0], traj.shape[3]
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
    ret64 = traj[:, R].double().sum(dim=(0, 1))
    dev_kernel, dev_step = float((ret.double() - ret64).abs().max()), float((ret_ref.double() - ret64).abs().max())
    worst.update(state=_bar(eng.state, ref.state), out_env=_bar(eng.out_env, ref.out_env), **{'return': _bar(ret, ret_ref)})
    print(f'replay {label}:', {k: round(v, 4) for k, v in worst.items()}, f'return vs float64 sum of the record: kernel {dev_kernel:.3e}, single steps {dev_step:.3e}')
    record_worst({**worst, 'return_dev_kernel': dev_kernel, 'return_dev_steps': dev_step}, f'chunked policy rollout vs single steps {label}')
    undriven = np.nonzero(pt.es_cols < 0)[0].tolist()
    if undriven:
        assert bool((traj[:, A, undriven] == 0).all())
    torch.testing.assert_close(eng.state, ref.state, rtol=2e-6, atol=2e-6)
    torch.testing.assert_close(eng.out_bldg[:2], ref.out_bldg[:2], rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(eng.out_env, ref.out_env, rtol=1e-4, atol=1e-4)
    if eng.n_bldg >= 1024 and not torch.allclose(ret, ret_ref, rtol=1e-5, atol=1e-3):
        assert dev_kernel <= 4.0 * dev_step, (dev_kernel, dev_step)
    else:
        torch.testing.assert_close(ret, ret_ref, rtol=1e-5, atol=1e-3)
    assert eng.t == K and torch.equal(traj[K - 1, N], eng.net) and torch.equal(traj[K - 1, S], eng.soc) and torch.equal(traj[K - 1, R], eng.reward_bldg)


@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('E', [64, 260])
@pytest.mark.parametrize('name,b_chunk,kind', [(n, 0, k) for n in ('b33', 'het40', 'b64') for k in KINDS]
                         + [('b33', 32, KINDS[0]), ('b33', 16, KINDS[0]), ('het40', 12, KINDS[0])])
def test_2_replay_through_single_steps(name, b_chunk, kind, E, f64):
    """(2) K = 30 (across a day boundary), noise on: 33 buildings cut 17 + 16 (the default: nine waves, the ninth with one building / none),
    32 + 1 (fifteen waves of the second workgroup row only meet the barriers) and 16 + 16 + 1, 40 heterogeneous ones cut 20 + 20 and
    12 + 12 + 12 + 4, 64 as two full chunks of 32; the default cuts under all three rewards.  The undriven buildings' action plane is 0."""
    spec, tab, layout, pol, pt, eng = _setup(name, E, f64, kind, sigma=0.1, b_chunk=b_chunk)
    if not b_chunk:
        assert default_chunks(eng.n_bldg) == {33: (17, 2, 9), 40: (20, 2, 10), 64: (32, 2, 16)}[eng.n_bldg]
    if name == 'het40':
        assert np.nonzero(pt.es_cols < 0)[0].tolist() == list(HET40_UNDRIVEN)
    ret, traj = _roll(eng, pt, 30, seed=5)
    assert eng.last_kernels == _names(f64), eng.last_kernels
    _replay(name, tab, pt, eng, ret, traj, kind, f64, f'{name} b_chunk={b_chunk} {kind} E={E} f64_maps={f64}')


@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('b_chunk', [0, 8])
def test_2_config_4_size_replayed(b_chunk, f64):
    """(2) at the size the kernel is for: 1024 buildings x 64 envs, K = 30, noise on -- 32 chunks of 32 (the default) and 128 chunks of eight
    (every wave of the fold adds eight chunks, in two passes of its 64-chunk stride): a fault in the chunk indexing of the scratch rows or the
    return rows that only shows beyond 16 / 64 chunks would show here."""
    spec, tab, layout, pol, pt, eng = _setup('b1024', 64, f64, sigma=0.1, b_chunk=b_chunk)
    assert default_chunks(1024) == (32, 32, 16)
    ret, traj = _roll(eng, pt, 30, seed=5)
    assert eng.last_kernels == _names(f64), eng.last_kernels
    _replay('b1024', tab, pt, eng, ret, traj, 'RewardFunction', f64, f'b1024 b_chunk={b_chunk} RewardFunction E=64 f64_maps={f64}')


def test_2_without_a_return_buffer():
    """(2) `ret_env=None`: the fold behind the chunk kernel launches NQ workgroup rows instead of NQ + 1.  The smallest shape that chunks -- 17
    buildings cut 9 + 8 (an explicit b_chunk: they fit one row), 64 envs, K = 4: every plane bit for bit what a twin engine that keeps the
    return leaves, and against single steps at `_replay`'s tolerances (the return it checks is the twin's)."""
    E, K = 64, 4
    spec, tab, layout, pol, pt, eng = _setup('het17', E, sigma=0.1, b_chunk=9)
    twin = _setup('het17', E, sigma=0.1, b_chunk=9)[5]
    ret, traj_twin = _roll(twin, pt, K, seed=5)
    traj = torch.full_like(traj_twin, float('nan'))
    eng.rollout_policy(K, pt, seed=5, traj=traj, chunked=True)
    assert eng.last_kernels == twin.last_kernels == _names('chain'), eng.last_kernels
    for got, want in ((traj, traj_twin), (eng.state, twin.state), (eng.out_bldg[:2], twin.out_bldg[:2]), (eng.out_env, twin.out_env)):
        assert torch.equal(got, want)
    _replay('het17', tab, pt, eng, ret, traj, 'RewardFunction', 'chain', 'het17 b_chunk=9 RewardFunction E=64 f64_maps=chain ret_env=None')


# ---- 3. teacher-forced actions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H', [4, 16, 32])
@pytest.mark.parametrize('f64,vec', PRECISIONS)
@pytest.mark.parametrize('name', ['b33', 'het40'])
def test_3_teacher_forced_actions(name, f64, vec, H):
    """(3) Every recorded action of the driven buildings recomputed in float64 from the previous step's recorded planes, noise replayed from the
    Philox stream (E = 260, K = 24).  Gate: 4 x the worst deviation of a float32 torch evaluation of the unsplit MLP on the same inputs."""
    spec, tab, layout, pol, pt, eng = _setup(name, 260, f64, H=H, sigma=0.1, vec=vec)
    _, traj = _roll(eng, pt, 24, seed=11)
    assert eng.last_kernels == _names(f64, vec), eng.last_kernels
    drv = np.nonzero(pt.es_cols >= 0)[0]
    dev_kernel, dev_f32 = _teacher_forced_driven(eng, tab, layout, pol, pt, traj, drv, seed=11)
    print(f'teacher-forced {name} vec={vec} f64={f64} H={H}: kernel {dev_kernel:.3e}  float32 torch {dev_f32:.3e}  ratio {dev_kernel / dev_f32:.2f}')
    record_worst({'kernel': dev_kernel, 'float32_torch': dev_f32, 'ratio': dev_kernel / dev_f32}, f'chunked policy teacher-forced {name} f64_maps={f64} vec={vec} H={H}')
    assert dev_f32 > 0 and dev_kernel <= 4.0 * dev_f32, (dev_kernel, dev_f32)


# ---- 4. free-running against the CPU ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', ['b33', 'het40'])
def test_4_free_running_against_the_cpu(name, kind, f64):
    """(4) K = 48 from reset, H = 16, E = 64: the host loop of `COracle.step` + `actions_host` (float64) against one chunked launch, at the plain
    bar 1e-4 + 1e-4 |ref| on soc, net, reward, district net and degraded capacity (conditioning: tests/test_policy_chunk_host.py)."""
    E, K = 64, 48
    spec, tab, layout, pol, pt, eng = _setup(name, E, f64, kind, H=16)
    want = host_closed_loop(spec, tab, layout, pol, pt, K, E, reward=kind)
    _, traj = _roll(eng, pt, K)
    assert eng.last_kernels == _names(f64), eng.last_kernels
    tr = traj.cpu().numpy().astype(np.float64)
    bar = lambda got, ref: float((np.abs(got - ref) / (1e-4 + 1e-4 * np.abs(ref))).max())
    worst = {'soc': bar(tr[:, S], want['soc']), 'net': bar(tr[:, N], want['net']), 'reward': bar(tr[:, R], want['reward']),
             'district_net': bar(eng.district_net.cpu().numpy().astype(np.float64), want['dnet'][-1]),
             'district_net_of_record': bar(tr[:, N].sum(axis=1), want['dnet']),
             'degraded_capacity': bar(eng.degraded_capacity.cpu().numpy(), want['degcap'][-1])}
    print(f'free-running {name} {kind} f64={f64}:', {k: round(v, 4) for k, v in worst.items()})
    check_worst(worst, f'chunked policy rollout {name} {kind} f64={f64}')


# ---- 5. split launches and checkpoint ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('name', ['b33', 'het40'])
def test_5_split_launches_and_checkpoint_are_bit_identical(name, f64):
    """(5) Launches of 1, 5, 24 and 25 steps from t0 = 0 equal one 55-step launch bit for bit in record, state, out_bldg[:2] and out_env (the
    previous net travels through out_bldg, t == 0 uses net_reset; every launch ends with its own fold), with a checkpoint restored into a fresh
    engine between two of them; the return accumulated over the four launches equals, bit for bit, the same four launches on an engine without
    the checkpoint, and one launch's at rtol 1e-6 / atol 1e-4 (four partial sums instead of one).  Then one `step()` with zero actions on both
    engines: equal district sums -- the chunked launches left the reserved plane's marker and ticket words usable."""
    E = 320
    spec, tab, layout, pol, pt, one = _setup(name, E, f64, sigma=0.1)
    ret1, traj1 = _roll(one, pt, 55, seed=3)
    assert one.last_kernels == _names(f64), one.last_kernels
    eng, straight = StepEngine(tab, E, f64_maps=f64), StepEngine(tab, E, f64_maps=f64)
    ret, ret_s, parts = torch.zeros(E, device='cuda'), torch.zeros(E, device='cuda'), []
    for n, K in enumerate((1, 5, 24, 25)):
        if n == 2:
            sd = eng.state_dict()
            eng = StepEngine(tab, E, f64_maps=f64)
            eng.load_state_dict(sd)
        traj = torch.empty((K, policy.CLPOL_NT, eng.n_bldg, E), device='cuda')
        eng.rollout_policy(K, pt, seed=3, ret_env=ret, traj=traj, chunked=True)
        straight.rollout_policy(K, pt, seed=3, ret_env=ret_s, chunked=True)
        parts.append(traj)
    assert eng.t == 55 and torch.equal(torch.cat(parts), traj1)
    assert torch.equal(eng.state, one.state) and torch.equal(eng.out_bldg[:2], one.out_bldg[:2]) and torch.equal(eng.out_env, one.out_env)
    assert torch.equal(ret, ret_s) and torch.equal(eng.state, straight.state)
    torch.testing.assert_close(ret, ret1, rtol=1e-6, atol=1e-4)
    zero = torch.zeros((eng.n_act_cols, E), device='cuda')
    eng.step(zero)
    one.step(zero)
    assert eng.t == one.t == 56 and torch.equal(eng.out_env, one.out_env) and torch.equal(eng.district_reward, one.district_reward)
    assert torch.equal(eng.state, one.state) and torch.equal(eng.net, one.net)
    torch.testing.assert_close(eng.district_net, eng.net.sum(dim=0), rtol=1e-5, atol=1e-3)
    torch.testing.assert_close(eng.district_reward, eng.reward_bldg.sum(dim=0), rtol=1e-5, atol=1e-3)


# ---- 6. episode windows x parameter sets x env offsets ----------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', ['chain', False])
def test_6_windows_sets_and_env_offsets(f64):
    """(6) 'b33': two env blocks with different episode windows AND different parameter sets in one chunked launch; each block equals, bit for
    bit, an engine of its own with that window, that set and its env offset (noise on: the half batches reproduce the whole batch's streams,
    which are keyed by the global env whatever the chunk geometry).  Block 1's actions are its window's and its set's: teacher-forced."""
    spec, tab, layout = _district('b33')
    pol = make_policy(layout, 16, n_sets=2, seed=2, sigma=0.1)
    K, n_steps, rows = 24, 200, [0, 131]
    whole = StepEngine(tab, 512, f64_maps=f64, n_steps=n_steps, env_row0=rows)
    whole.trace_kernels()
    _, traj = _roll(whole, pol.pack(layout, tab, device='cuda:0', set_of_block=[0, 1]), K, seed=9)
    assert whole.last_kernels == _names(f64), whole.last_kernels
    assert not torch.equal(traj[:, A, :, :256], traj[:, A, :, 256:])
    for g in range(2):
        part = StepEngine(tab, 256, f64_maps=f64, n_steps=n_steps, env_row0=[rows[g]], env_offset=256 * g)
        _, tr = _roll(part, pol.pack(layout, tab, device='cuda:0', set_of_block=[g]), K, seed=9)
        sl = slice(256 * g, 256 * (g + 1))
        assert torch.equal(tr, traj[:, :, :, sl]), g
        assert torch.equal(part.state, whole.state[:, :, sl]) and torch.equal(part.out_env, whole.out_env[:, sl])
    single = policy.MLPPolicy(pol.w1[1:2], pol.b1[1:2], pol.w2[1:2], pol.b2[1:2], sigma=0.1)
    dev_kernel, dev_f32 = _teacher_forced(whole, tab, layout, single, single.pack(layout, tab), traj[:, :, :, 256:], seed=9, row0=rows[1], env_offset=256)
    print(f'window 1 / set 1 teacher-forced: kernel {dev_kernel:.3e}  float32 torch {dev_f32:.3e}')
    assert dev_kernel <= 4.0 * dev_f32


# ---- 7. the return is accumulated -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f64', ['chain', False])
def test_7_ret_env_is_accumulated(f64):
    """(7) `ret_env` is added to, not overwritten: a pre-filled one ends at its old value plus the return a zeroed one ends at (the fold adds ONE
    number per env: bit for bit), also over a second launch; and a launch of no steps leaves it, the state and the outputs alone."""
    E, K = 260, 12
    spec, tab, layout, pol, pt, a = _setup('b33', E, f64, sigma=0.1)
    b = _setup('b33', E, f64, sigma=0.1)[5]
    r0 = torch.zeros(E, device='cuda')
    a.rollout_policy(K, pt, seed=2, ret_env=r0, chunked=True)
    pre = torch.linspace(-300.0, 500.0, E, device='cuda')
    r1 = pre.clone()
    b.rollout_policy(K, pt, seed=2, ret_env=r1, chunked=True)
    assert r0.abs().min() > 0 and torch.equal(r1, pre + r0)
    mid, before = r1.clone(), [x.clone() for x in (b.state, b.out_bldg[:2], b.out_env)]
    b.rollout_policy(0, pt, seed=2, ret_env=r1, chunked=True)
    assert torch.equal(r1, mid) and b.t == K and b.last_kernels == _names(f64).split('+')[0]
    for x, was in zip((b.state, b.out_bldg[:2], b.out_env), before):
        assert torch.equal(x, was)
    r2 = torch.zeros(E, device='cuda')
    a.rollout_policy(K, pt, seed=2, ret_env=r2, chunked=True)
    b.rollout_policy(K, pt, seed=2, ret_env=r1, chunked=True)
    assert torch.equal(r1, mid + r2) and torch.equal(a.state, b.state)


# ---- 8. env level -----------------------------------------------------------------------------------------------------------------------
def test_8_env_level_routes_by_itself_and_equals_capture_rollout():
    """(8) `VectorCityLearnEnv.rollout_policy(policy, K, record=True)` on 33 buildings routes to the chunked launch by itself; against
    `capture_rollout` driven by `torch_policy` over `observations='tensor'`, at the tolerances of tests/test_gpu_policy_rollout.py::test_g:
    per-step actions at the teacher-forced tolerance widened by what the two paths' state tolerance (2e-6 on soc, 2e-5 on net) can move an action
    through the two dependent weights, and once more for the float32 torch policy's own deviation; returns at rtol 1e-5 / atol 1e-3; states at
    2e-6.  `kpi=True` names the gap.  On 17 buildings the same call still launches the one-row kernel, and a thermal district routes as before
    (nine buildings: one row; seventeen: its own chunked kernel)."""
    from citylearn_amd.synthetic import tile_district
    from citylearn_amd.vector_env import VectorCityLearnEnv
    from golden_util import golden
    from policy_full_util import make_storage_policy
    E, K = 256, 24
    a, b = (VectorCityLearnEnv(chunk_district('b33'), E, observations='tensor', normalize_observations=True) for _ in range(2))
    a.engine.trace_kernels()
    pol = make_policy(a.layout, 16, seed=4)
    ret, traj = a.rollout_policy(pol, K, record=True)
    assert a._t == K == a.engine.t and traj.shape == (K, policy.CLPOL_NT, 33, E)
    assert a.engine.last_kernels == _names('chain' if a.engine.f64_chain else False), a.engine.last_kernels
    kenv = VectorCityLearnEnv(chunk_district('b33'), E, kpi=True)
    with pytest.raises(NotImplementedError, match='no chunked lean KPI kernel.*step_many'):
        kenv.rollout_policy(make_policy(ObservationLayout(kenv.spec, 'current', False), 16, seed=4), K, kpi=True)
    pt_host = pol.pack(a.layout, a.tables)
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
    assert np.array_equal(pt_host.es_cols, np.arange(33))
    worst = float((traj[:, A] - acts[:, :33]).abs().max())
    print(f'env level, 33 buildings: |action difference| {worst:.3e}, tolerance {tol:.3e} (float32 deviation {dev_f32:.3e}, state term {widen:.3e})')
    record_worst({'action_difference': worst, 'tolerance': tol}, 'chunked policy rollout env level b33 vs capture_rollout')
    assert worst <= tol
    torch.testing.assert_close(ret, rewards.sum(dim=0) if rewards.dim() == 2 else rewards.sum(dim=(0, 1)), rtol=1e-5, atol=1e-3)
    torch.testing.assert_close(a.engine.state, b.engine.state, rtol=2e-6, atol=2e-6)
    # the routing of everything else is what it was
    small = VectorCityLearnEnv(golden('g2022_all').schema_path, E, observations='tensor', normalize_observations=True)
    small.engine.trace_kernels()
    small.rollout_policy(make_policy(small.layout, 16, seed=4), 4)
    assert small.engine.last_kernels.startswith('cl_rollout_policy_kernel<') and '+' not in small.engine.last_kernels, small.engine.last_kernels
    for n, want in ((9, 'cl_rollout_full_policy_kernel<'), (17, 'cl_rollout_full_policy_chunk_kernel<')):
        spec = golden('g2020_cz1').spec()
        th = VectorCityLearnEnv(spec if n == 9 else tile_district(spec, n), 64, observations='tensor', normalize_observations=True)
        th.engine.trace_kernels()
        th.rollout_policy(make_storage_policy(th.layout, 16, seed=4), 4)
        assert th.engine.last_kernels.startswith(want), (n, th.engine.last_kernels)


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------
def test_9_refusals_leave_every_plane_untouched():
    """(9) A MARL engine, a `kpi=True` engine and `f64_maps=True` (the library's refusals, by name), `chunked=True, kpi=True` on an engine with
    and without KPIs (`NotImplementedError`: no chunked lean KPI kernel, and the route), `PolicyTables` on a thermal district (`ValueError`) --
    and, with default arguments, the one-row kernel's refusal as before: state, output planes, district sums, return and record stay what they
    were."""
    from golden_util import golden
    from citylearn_amd.synthetic import tile_district
    E, K = 64, 4
    spec, tab, layout, pol, pt, plain = _setup('b33', E, False)
    thermal = StepEngine(tile_district(golden('g2020_cz1').spec(), 33).episode_tables(0), E, f64_maps=False)
    assert not thermal.lean
    no_kernel = 'no chunked lean KPI kernel.*step_many.*kpi=True'
    cases = [('MARL', _setup('b33', E, False, 'MARL')[5], {}, _lib.EngineError, 'CLR_MARL.*cannot couple the buildings inside a step'),
             ('kpi engine', StepEngine(tab, E, f64_maps=False, kpi=True), {}, _lib.EngineError, 'clpc_rollout_mlp_f32.*CLD_KPI'),
             ('kpi=True on a kpi engine', StepEngine(tab, E, f64_maps=False, kpi=True), {'kpi': True}, NotImplementedError, no_kernel),
             ('kpi=True', plain, {'kpi': True}, NotImplementedError, no_kernel),
             ('thermal district', thermal, {}, ValueError, 'StoragePolicyTables'),
             ('f64_maps=True', StepEngine(tab, E, f64_maps=True), {}, _lib.EngineError, 'clpc_rollout_mlp_f32.*CLD_F64_MAPS'),
             ('b_chunk=33', _setup('b33', E, False, b_chunk=33)[5], {}, _lib.EngineError, 'b_chunk=33'),
             ('not chunked', plain, {'chunked': False}, _lib.EngineError, 'n_bldg=33 > 32 would be a building-chunked launch.*clpc_rollout_mlp_f32')]
    for name, eng, kw, exc, match in cases:
        ret = torch.full((E,), 3.0, device='cuda')
        traj = torch.full((K, policy.CLPOL_NT, eng.n_bldg, E), -7.0, device='cuda')
        before = [x.clone() for x in (eng.state, eng.out_bldg, eng._out_env, ret, traj)]
        t_before = eng.t
        with pytest.raises(exc, match=match):
            eng.rollout_policy(K, pt, ret_env=ret, traj=traj, **{'chunked': True, **kw})
        torch.cuda.synchronize()
        assert eng.t == t_before, name
        for x, was in zip((eng.state, eng.out_bldg, eng._out_env, ret, traj), before):
            assert torch.equal(x, was), name
    # ... and after all that the engine still runs
    _roll(plain, pt, K)
    assert plain.last_kernels == _names(False), plain.last_kernels
