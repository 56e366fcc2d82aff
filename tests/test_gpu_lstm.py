"""LSTM indoor-temperature stage + fused ComfortReward (`cl_lstm_step_f32`) against the reference's predicted
temperatures / comfort rewards on the 2023 schema.  GPU only."""
import numpy as np
import pytest
import torch

from golden_util import golden
from citylearn_amd import abi
from citylearn_amd.engine import StepEngine
from citylearn_amd.dynamics import LSTMStage

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name,split,cell', [
    ('g2023_p2', 'f16', 'auto'), ('s_baeda', 'f16', 'auto'), ('s_2023_p1', 'f16', 'auto'), ('s_2023_p3', 'f16', 'auto'), ('g2023_heat', 'f16', 'auto'),
    ('g2023_p2', 'f16', 'plain'), ('s_2023_p3', 'f16', 'plain'), ('g2023_heat', 'f16', 'plain'), ('g2023_both', 'f16', 'auto'), ('g2023_both', 'bf16', 'plain'),
    ('g2023_p2', 'bf16', 'auto'), ('s_baeda', 'bf16', 'auto'), ('g2023_heat', 'bf16', 'plain'), ('g2023_p2', None, 'auto'), ('s_2023_p3', None, 'auto'),
    # the other 2023 districts of the reference checkout (their own LSTM weights, outage seeds and buildings)
    ('s_2023_oe1', 'f16', 'auto'), ('s_2023_oe2', 'f16', 'auto'), ('s_2023_oe3', 'f16', 'auto'), ('s_2023_p32', 'f16', 'auto'), ('s_2023_p33', 'f16', 'auto')])
def test_lstm_stage_fed_with_reference_cooling(name, split, cell):
    """Isolates the stage: the delivered cooling of every step comes from the reference; temperatures within 1e-4 C
    relative and ComfortReward within 1e-4 (+1e-4) of the reference for every step and building (2023: LSTM(13 -> 16),
    3 and 6 buildings; baeda_3dem: three LSTM(11 -> 8, 2 layers) embedded in the 16-wide kernel + one LSTM(11 -> 50, 1 layer)).
    `split`: the operand format of the recurrent products -- two f16 terms (default), three bf16 terms, or the exact f32 MFMA.
    g2023_both: Building_1's model takes BOTH demands (a rewritten .pth with a fourteenth input; the reference builds the input generically,
    building.py:3039-3078) and runs on the generic kernel with delivered heating as a third env-dependent input.
    `cell`: the cell update -- 'auto' picks the common-denominator form (7 transcendentals per unit and cell) for every 2023 district and the
    plain one (10) for baeda_3dem, whose gate bound exceeds what the products admit (`dynamics.cell_update_bounds`)."""
    g = golden(name)
    spec = g.spec()
    cols = list(range(len(spec.buildings)))
    if name == 's_baeda':
        # the fourth baeda building is a one-layer LSTM(11 -> 50): the generic kernel (cl_lstm_generic_step_f32) runs beside the
        # matrix-core kernel of the other three
        from citylearn_amd.dynamics import pack_lstm, pack_lstm_generic
        lw, _ = pack_lstm(spec, spec.episode_tables(0))
        assert lw[:, abi.CLW_ACTIVE if hasattr(abi, 'CLW_ACTIVE') else 3285].tolist() == [1.0, 1.0, 1.0, 2.0]
        assert pack_lstm_generic(spec, spec.episode_tables(0))[2] == 50
    tab = spec.episode_tables(0)
    attrs = spec.reward_function.get('attributes') or {}
    E = 64
    eng = StepEngine(tab, E, detail=True)
    stage = LSTMStage(spec, tab, eng, attrs.get('band'), attrs.get('lower_exponent') or 2.0, attrs.get('higher_exponent') or 2.0, split=split,
                      cell_update=cell)
    assert stage.cell_update == ('common_denominator' if (cell == 'auto' and split is not None and name != 's_baeda') else 'plain')
    eng.trace_kernels()
    cool = torch.from_numpy(g.ref['cool_dem'][:, cols]).cuda()
    # g2023_heat (synthetic: heating device actions, hvac_mode 0-3, one heating-driven model): the delivered heating plane too
    heat = torch.from_numpy(g.ref['heat_dem'][:, cols]).cuda() if 'heat_dem' in g.ref.files else None
    worst_t = worst_r = 0.0
    for t in range(g.facts['steps']):
        temp = stage.step(t, cool[t][:, None].expand(-1, E).contiguous(), None if heat is None else heat[t][:, None].expand(-1, E).contiguous())
        tt, rr = temp.cpu().numpy(), stage.comfort.cpu().numpy()
        assert (tt[:, :1] == tt).all()
        worst_t = max(worst_t, float(np.max(np.abs(tt[:, 0] - g.ref['indoor_temp'][t][cols]))))
        ref = g.ref['reward_ComfortReward'][t][cols]
        worst_r = max(worst_r, float(np.max(np.abs(rr[:, 0] - ref) / (1e-4 + 1e-4 * np.abs(ref)))))
    assert ('cl_lstm_kernel<32,' in eng.last_kernels) == (stage.cell_update == 'common_denominator'), eng.last_kernels
    assert worst_t < 2e-3, worst_t          # deg C on ~25 C: < 1e-4 relative
    assert worst_r < 1.0, worst_r           # BASELINE.json: reward parity within 1e-4 relative (measured: 0.09)


@pytest.mark.parametrize('name', ['g2023_p2', 'g2023_heat', 'g2023_both'])
def test_energy_step_plus_lstm_free_running(name):
    """Energy step + LSTM stage chained on the GPU with the golden action sequence, free-running (g2023_heat: heating device /
    cooling-or-heating device actions, every hvac mode, a heating-driven temperature model -- building.py:3123-3158)."""
    g = golden(name)
    spec = g.spec()
    tab = spec.episode_tables(0)
    attrs = spec.reward_function['attributes']
    E = 64
    eng = StepEngine(tab, E, detail=True)
    stage = LSTMStage(spec, tab, eng, attrs['band'], attrs['lower_exponent'], attrs['higher_exponent'])
    acts = torch.from_numpy(g.ref['actions']).cuda()
    K = g.facts['steps']
    temps = np.zeros((K, 3)); rews = np.zeros((K, 3))
    for t in range(K):
        eng.step(acts[t][:, None].expand(-1, E).contiguous(), t)
        temps[t] = stage.step(t).cpu().numpy()[:, 0]
        rews[t] = stage.comfort.cpu().numpy()[:, 0]
    assert np.max(np.abs(temps - g.ref['indoor_temp'][:K])) < 5e-3
    # episode return (central agent: sum over buildings) within 1e-3 relative
    np.testing.assert_allclose(rews.sum(), g.ref['env_rewards'][:K].sum(), rtol=1e-3)
    err = np.abs(rews - g.ref['reward_ComfortReward'][:K]) / (1e-3 + 1e-3 * np.abs(g.ref['reward_ComfortReward'][:K]))
    assert err.max() < 10.0, err.max()


@pytest.mark.parametrize('name', ['g2023_p2', 'g2023_heat'])
def test_env_default_comfort_reward_and_comfort_kpis(name):
    """`CityLearnEnv` on the 2023 schema with its default reward (ComfortReward, central agent): rewards and the
    discomfort / thermal-resilience KPIs of `evaluate()` against the reference, full episode.  g2023_heat (heating devices, every
    hvac mode): every KPI of the table, i.e. also the cost KPIs whose baseline removes the partial-load heating difference
    (converted with the episode-end COP, building.py:2893-2898)."""
    from citylearn_amd.citylearn import CityLearnEnv
    g = golden(name)
    env = CityLearnEnv(g.schema_path)
    assert type(env.reward_function).__name__ == 'ComfortReward' and env._fused_comfort and env.central_agent
    K = g.facts['steps']
    got = np.zeros(K)
    for t in range(K):
        _, r, term, _, _ = env.step([[float(x) for x in g.ref['actions'][t]]])
        got[t] = r[0]
    ref = g.ref['env_rewards'][:K, 0]
    assert np.max(np.abs(got - ref) / (1e-3 + 1e-3 * np.abs(ref))) < 10.0
    np.testing.assert_allclose(got.sum(), ref.sum(), rtol=1e-3)
    frame = env.evaluate()
    mine = {f'{r.level}|{r.name}|{r.cost_function}': r.value for r in frame.itertuples() if r.value is not None and not np.isnan(r.value)}
    gref = dict(zip([str(x) for x in g.ref['kpi_names']], g.ref['kpi_values']))
    n = 0
    for k, v in gref.items():
        if k.split('|')[-1].startswith(('discomfort', 'one_minus_thermal')) or name == 'g2023_heat':
            np.testing.assert_allclose(mine[k], v, rtol=5e-3, atol=2e-3, err_msg=k)
            n += 1
    assert n >= 30


def test_vector_env_comfort_reward():
    from citylearn_amd.vector_env import VectorCityLearnEnv
    g = golden('g2023_p2')
    env = VectorCityLearnEnv(g.schema_path, n_envs=128)
    acts = torch.from_numpy(g.ref['actions']).cuda()
    tot = torch.zeros(128, device='cuda')
    for t in range(60):
        obs, reward, *_ = env.step(acts[t][:, None].expand(-1, 128).contiguous())
        assert reward.shape == (128,) and obs['indoor_dry_bulb_temperature'].shape == (3, 128)
        tot += reward
    np.testing.assert_allclose(float(tot[0]), g.ref['env_rewards'][:60, 0].sum(), rtol=2e-3)


def test_vector_env_solar_penalty_and_comfort_reward():
    """`SolarPenaltyAndComfortReward` = coefficient-weighted sum of the two stock rewards (reward_function.py:381-386):
    expected values from the reference's own per-building SolarPenaltyReward / ComfortReward of the same run."""
    from citylearn_amd.vector_env import VectorCityLearnEnv
    g = golden('g2023_p2')
    spec_attrs = g.spec().reward_function['attributes']
    coeff = (0.4, 1.7)
    env = VectorCityLearnEnv(g.schema_path, n_envs=64, central_agent=False,
                             reward_function='citylearn.reward_function.SolarPenaltyAndComfortReward',
                             reward_function_kwargs={**spec_attrs, 'coefficients': coeff})
    acts = torch.from_numpy(g.ref['actions']).cuda()
    for t in range(80):
        _, reward, *_ = env.step(acts[t][:, None].expand(-1, 64).contiguous())
        want = coeff[0] * g.ref['reward_SolarPenaltyReward'][t] + coeff[1] * g.ref['reward_ComfortReward'][t]
        np.testing.assert_allclose(reward[:, 0].cpu().numpy(), want, rtol=2e-3, atol=2e-3)      # free-running fp32


def test_bf16_mfma_operand_layout():
    """Known-answer test of the operand layout the split-bf16 LSTM kernel relies on: lane l of
    v_mfma_f32_32x32x16_bf16 supplies A[l & 31][8 (l >> 5) + 0..7] and B[8 (l >> 5) + 0..7][l & 31]; D[row][col] with
    col = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).  Asymmetric random operands (bf16-exact values)."""
    import ctypes
    from citylearn_amd import _lib
    lib = _lib.load_tune()          # layout probes live in the tuning library, not in the product one
    rng = np.random.RandomState(0)
    A = rng.randint(-64, 64, size=(32, 16)).astype(np.float32) / 16.0          # exact in bf16
    B = rng.randint(-64, 64, size=(16, 32)).astype(np.float32) / 8.0
    to_bf16 = lambda x: (x.view(np.uint32) >> 16).astype(np.uint16)
    a = torch.from_numpy(to_bf16(A).astype(np.int16)).cuda(); b = torch.from_numpy(to_bf16(B).astype(np.int16)).cuda()
    d = torch.zeros((32, 32), device='cuda')
    assert lib.cl_tune_mfma_bf16_probe(a.data_ptr(), b.data_ptr(), d.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    np.testing.assert_array_equal(d.cpu().numpy(), (A.astype(np.float64) @ B.astype(np.float64)).astype(np.float32))


def test_env_on_the_whole_baeda_district():
    """baeda_3dem end to end (4 buildings; the fourth one's LSTM(11 -> 50, 1 layer) runs in the generic kernel): the
    reference's rewards, predicted temperatures and observations for the fixture's action sequence, free-running."""
    from citylearn_amd.citylearn import CityLearnEnv
    g = golden('s_baeda')
    env = CityLearnEnv(g.schema_path)
    assert len(env.buildings) == 4 and env.observation_names == g.facts['observation_names']
    K = g.facts['steps']
    names = env.action_names
    got, temps = [], []
    for t in range(K):
        a = [float(x) for x in g.ref['actions'][t]]
        acts, p = [], 0
        for n in names:
            acts.append(a[p:p + len(n)]); p += len(n)
        _, r, _, _, _ = env.step(acts)
        got.append(r)
        temps.append(env._hist['indoor_temp'][-1])
    got, ref = np.array(got, dtype=np.float64), g.ref['env_rewards'][:K]
    assert got.shape == ref.shape
    assert np.max(np.abs(got - ref) / (1e-3 + 1e-3 * np.abs(ref))) < 10.0
    assert np.max(np.abs(np.array(temps) - g.ref['indoor_temp'][:K])) < 5e-3


def test_lstm_stage_at_full_batch_size_by_replication():
    """3 x 65 536 (the C3 shape): the batch is 128 distinct delivered-cooling columns tiled along the env axis; every env must
    reproduce, bit for bit, the corresponding env of a 128-env stage (distinct envs against a reference:
    tests/test_gpu_lstm_synthetic.py::test_trained_models_per_env, the same models at 132 envs)."""
    g = golden('g2023_p2')
    spec = g.spec()
    tab = spec.episode_tables(0)
    E, reps = 65536, 512
    stages = []
    for n in (128, E):
        eng = StepEngine(tab, n, detail=True)
        stages.append(LSTMStage(spec, tab, eng, 1.0, 2.0, 3.0))
    gen = torch.Generator(device='cuda').manual_seed(7)
    for t in range(20):
        cool = torch.rand((3, 128), device='cuda', generator=gen) * 4
        t_small = stages[0].step(t, cool.contiguous())
        t_big = stages[1].step(t, cool.repeat(1, reps).contiguous())
    torch.cuda.synchronize()
    for small, big in ((stages[0].indoor_temp, stages[1].indoor_temp), (stages[0].comfort, stages[1].comfort)):
        tiled = big.reshape(3, reps, 128)
        assert torch.equal(tiled, small.unsqueeze(1).expand_as(tiled))
    assert torch.isfinite(stages[1].indoor_temp).all() and float(stages[1].indoor_temp.std()) > 0


@pytest.mark.parametrize('name', ['g2023_p2', 'g2023_both', 'g2023_heat'])
def test_generic_kernel_agrees_with_the_matrix_core_kernel(name, monkeypatch):
    """Every 2 x 16-unit model forced onto `cl_lstm_generic_kernel` (`dynamics.FORCE_GENERIC_KERNEL`): the fallback kernel -- hidden units
    dealt to four waves, matrices staged in LDS, three env-dependent inputs -- against the reference, on the fixtures the matrix-core
    kernel is pinned on (g2023_both: a model that takes both demands, on either kernel)."""
    from citylearn_amd import dynamics
    monkeypatch.setattr(dynamics, 'FORCE_GENERIC_KERNEL', True)
    g = golden(name)
    spec = g.spec()
    tab = spec.episode_tables(0)
    attrs = spec.reward_function.get('attributes') or {}
    E = 68
    eng = StepEngine(tab, E, detail=True)
    stage = LSTMStage(spec, tab, eng, attrs.get('band'), attrs.get('lower_exponent') or 2.0, attrs.get('higher_exponent') or 2.0)
    assert stage.generic is not None and stage.generic['layers'] == 2 and not (stage.lstm_w[:, dynamics.ACTIVE] == 1.0).any()
    cool = torch.from_numpy(g.ref['cool_dem']).cuda()
    heat = torch.from_numpy(g.ref['heat_dem']).cuda() if 'heat_dem' in g.ref.files else None
    worst_t = worst_r = 0.0
    for t in range(min(150, g.facts['steps'])):
        temp = stage.step(t, cool[t][:, None].expand(-1, E).contiguous(), None if heat is None else heat[t][:, None].expand(-1, E).contiguous())
        tt, rr = temp.cpu().numpy(), stage.comfort.cpu().numpy()
        assert (tt[:, :1] == tt).all()
        worst_t = max(worst_t, float(np.max(np.abs(tt[:, 0] - g.ref['indoor_temp'][t]))))
        ref = g.ref['reward_ComfortReward'][t]
        worst_r = max(worst_r, float(np.max(np.abs(rr[:, 0] - ref) / (1e-4 + 1e-4 * np.abs(ref)))))
    assert worst_t < 2e-3 and worst_r < 1.0, (worst_t, worst_r)


def test_two_demand_model_without_its_flag_is_poisoned_not_wrong():
    """`CLD_LSTM_TWO_DEMANDS` selects the matrix-core instantiation that reads the third input ring; a caller that packs a both-demand model
    (lstm_w[CLW_DEM2] != 0) and forgets the flag gets NaN for that building's temperature -- and the right values for the others."""
    from citylearn_amd import abi, dynamics
    g = golden('g2023_both')
    spec = g.spec()
    tab = spec.episode_tables(0)
    E = 64
    eng = StepEngine(tab, E, detail=True)
    good, bad = LSTMStage(spec, tab, eng), LSTMStage(spec, tab, eng)
    assert good.dims.flags & abi.CLD_LSTM_TWO_DEMANDS and good.generic is None
    bad.dims.flags &= ~abi.CLD_LSTM_TWO_DEMANDS
    cool = torch.from_numpy(g.ref['cool_dem']).cuda()
    heat = torch.from_numpy(g.ref['heat_dem']).cuda()
    for t in range(16):
        c, h = cool[t][:, None].expand(-1, E).contiguous(), heat[t][:, None].expand(-1, E).contiguous()
        tg, tb = good.step(t, c, h).clone(), bad.step(t, c, h).clone()
    two = (good.lstm_w[:, dynamics.DEM2] != 0).cpu().numpy()
    assert two.tolist() == [True, False, False]
    assert torch.isnan(tb[0]).all() and torch.isfinite(tg).all()
    assert torch.equal(tb[1:], tg[1:])


@pytest.mark.parametrize('name', ['g2023_heat', 'g2023_p2'])
def test_evaluate_called_mid_episode(name):
    """`CityLearnEnv.evaluate()` in the middle of an episode against the reference doing the same (`kpi_mid.npz`, generated by
    `oracle/ref_harness/gen_golden.py mid_evaluate`).  With controlled heat-pump heating (g2023_heat) the reference converts the partial-load
    heating difference of every past step with the COP of the step it stands at (building.py:2893-2898): the cost KPIs of the baseline move."""
    from citylearn_amd.citylearn import CityLearnEnv
    g = golden(name)
    mid = np.load(g.dir / 'kpi_mid.npz')
    step = int(mid['step'])
    env = CityLearnEnv(g.schema_path)
    for t in range(step):
        env.step([[float(x) for x in g.ref['actions'][t]]])
    frame = env.evaluate()
    mine = {f'{r.level}|{r.name}|{r.cost_function}': r.value for r in frame.itertuples() if r.value is not None and not np.isnan(r.value)}
    ref = dict(zip([str(x) for x in mid['kpi_names']], mid['kpi_values']))
    assert len(ref) >= 40
    for k, v in ref.items():
        np.testing.assert_allclose(mine[k], v, rtol=5e-3, atol=2e-3, err_msg=k)
    if name == 'g2023_heat':
        # ... and the correction is what makes it so: with the series as the device booked it (episode-end COP) some baseline KPI is off
        env._baseline_series = lambda: env._history_array('base_net')
        raw = {f'{r.level}|{r.name}|{r.cost_function}': r.value for r in env.evaluate().itertuples() if r.value is not None and not np.isnan(r.value)}
        assert max(abs(raw[k] - v) / (2e-3 + 5e-3 * abs(v)) for k, v in ref.items()) > 1.0
