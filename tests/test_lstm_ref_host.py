"""Pins `lstm_ref_util` -- the float64 reference tests/test_gpu_lstm_synthetic.py holds the LSTM kernels against -- without a GPU: on the
fixtures' recorded temperatures, against torch's own LSTM, and the two preconditions of the free-running GPU cases (the float32 evaluation
stays well inside the bar; the envs spread far beyond it)."""
import numpy as np
import pytest
import torch

import lstm_ref_util as R
from golden_util import golden


@pytest.mark.parametrize('name,buildings', [('g2023_p2', (0, 1, 2)), ('g2023_heat', (0, 1, 2)), ('g2023_both', (0, 1, 2)), ('s_baeda', (3,))])
def test_reference_reproduces_the_fixture_temperatures(name, buildings):
    """`run_ref` fed with the recorded delivered demands reproduces `indoor_temp` of the fixture (the bar of tests/test_lstm_tables_cpu.py)."""
    g = golden(name)
    spec = g.spec()
    tab = spec.episode_tables(0)
    K = min(200, g.facts['steps'])
    cool = g.ref['cool_dem'][:K].astype(np.float64)
    heat = g.ref['heat_dem'][:K].astype(np.float64) if 'heat_dem' in g.ref.files else np.zeros_like(cool)
    for b in buildings:
        m = R.Model(spec.buildings[b], tab)
        temps = R.run_ref(m, cool[:, b:b + 1], heat[:, b:b + 1])
        worst = float(np.max(np.abs(temps[:, 0] - g.ref['indoor_temp'][:K, b])))
        print(f'{name} building {b}: worst |dT| = {worst:.3g} C over {K} steps')
        assert worst < 5e-5, (name, b, worst)


@pytest.mark.parametrize('district,b', [('mc_a', 1), ('gen_2x20', 2), ('gen_1x17', 2), ('mix_demands', 0), ('mix_demands', 1)])
def test_cell_matches_torch_lstm(district, b, tmp_path):
    """One 12-step window of `step_ref` from zero state against ``torch.nn.LSTM(...).double()`` + Linear on the same input sequence: the
    hand-written cell, its gate order and the window's ring addressing owe nothing to the project's own code."""
    g = golden('g2023_p2')
    spec = R.district_spec(g.spec(), district, tmp_path)
    tab = spec.episode_tables(0)
    m = R.Model(spec.buildings[b], tab)
    sd = torch.load(spec.buildings[b].dynamics.filepath)
    n_in = sd['l_lstm.weight_ih_l0'].shape[1]
    lstm = torch.nn.LSTM(n_in, m.H, m.layers, batch_first=True).double()
    lstm.load_state_dict({k[len('l_lstm.'):]: v.double() for k, v in sd.items() if k.startswith('l_lstm.')})
    lin = torch.nn.Linear(m.H, 1).double()
    lin.load_state_dict({'weight': sd['l_linear.weight'].double(), 'bias': sd['l_linear.bias'].double()})
    E, t = 7, 29
    rng = np.random.RandomState(3)
    rings = rng.uniform(0.0, 1.0, size=(36, E))
    cool, heat = rng.uniform(0.0, 4.0, size=E), rng.uniform(0.0, 4.0, size=E)
    temp, y, state, writes = R.step_ref(m, t, rings, R.zero_state(m, E), cool, heat)
    # the same window, assembled here: inputs of time t-11..t, the temperature of time-1, the newest demand sample(s) from this step
    x = np.zeros((E, 12, n_in))
    dem = heat if m.heating_driven else cool
    for s in range(12):
        time = t - 11 + s
        x[:, s, :] = m.exo[time][None, :]
        x[:, s, m.ic] = (dem - m.cmin) / (m.cmax - m.cmin) if s == 11 else rings[time % 12]
        x[:, s, m.it] = rings[12 + (time - 1) % 12]
        if m.i2 is not None:
            x[:, s, m.i2] = (heat - m.c2min) / (m.c2max - m.c2min) if s == 11 else rings[24 + time % 12]
    with torch.no_grad():
        out, (hn, cn) = lstm(torch.from_numpy(x))
        want = lin(out[:, -1]).numpy()[:, 0]
    np.testing.assert_allclose(y, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(temp, want * (m.tmax - m.tmin) + m.tmin, rtol=0, atol=1e-10)
    np.testing.assert_allclose(state['h0'].T, hn[0].numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(state['c1' if m.layers == 2 else 'c0'].T, cn[-1].numpy(), rtol=0, atol=1e-12)
    assert (m.i2 is not None) == (district == 'mix_demands' and b == 1) and m.heating_driven == (district == 'mix_demands' and b == 0)
    assert float(np.std(y)) > 1e-3 and set(writes) == ({5, 17, 29} if m.i2 is not None else {5, 17})


@pytest.mark.parametrize('district,gain', R.FREE_RUNNING)
def test_free_running_cases_are_well_conditioned_and_spread(district, gain, tmp_path):
    """Preconditions of the free-running GPU cases, on their own models and inputs.  Conditioning: the float32 evaluation (f16 split on the
    matrix-core models) stays within 0.25 x (1e-4 + 1e-4 |T_ref|) of the float64 one over the test's 60 steps -- a kernel at fp32 precision then has
    three quarters of the bar to itself.  Spread: at the last step the reference's standard deviation over envs is at least 100 x that bar, so an
    env mix-up cannot hide inside the tolerance."""
    g = golden('g2023_p2')
    spec = R.district_spec(g.spec(), district, tmp_path, gain)
    tab = spec.episode_tables(0)
    models = R.models_of(spec, tab)
    cool, heat = R.demand_planes(models, R.T_FREE, R.E_SYN, seed=11)
    for b, m in enumerate(models):
        if m is None:
            continue
        if district in R.GENERIC_ONLY:
            m.matrix_core = False
        ref = R.run_ref(m, cool[:, b].astype(np.float64), heat[:, b].astype(np.float64))
        f32 = R.run_ref(m, cool[:, b], heat[:, b], dtype=np.float32, split='f16')
        bar = 1e-4 + 1e-4 * np.abs(ref)
        cond = float(np.max(np.abs(f32 - ref) / bar))
        spread = float(np.std(ref[-1]) / np.max(bar[-1]))
        print(f'{district} gain {gain} building {b} ({m.layers} x {m.H}): float32 / float64 = {cond:.4f} x bar, spread = {spread:.0f} x bar')
        assert f32.dtype == np.float32 and np.isfinite(ref).all()
        assert cond < 0.25, (district, b, cond)
        assert spread >= 100.0, (district, b, spread)


def test_comfort_kpi_restatement_on_a_hand_checked_series(tmp_path):
    """`comfort_kpi_ref` on a series small enough to check by hand (occupancy gating, both sides of the band, minima / maxima seeds)."""
    g = golden('g2023_p2')
    spec = g.spec()
    m = R.Model(spec.buildings[0], spec.episode_tables(0))
    m.occupied = np.array([True, False, True, True])
    m.csp, m.hsp = np.full(4, 24.0), np.full(4, 20.0)
    temps = np.array([[27.0, 22.0], [40.0, 0.0], [17.5, 22.0], [24.5, 19.0]], dtype=np.float32)
    k = R.comfort_kpi_ref(m, temps, outage=np.array([0, 0, 1, 0]), kpi_band=2.0)
    assert k['CLKC_UNMET'].tolist() == [2.0, 0.0] and k['CLKC_HOT'].tolist() == [1.0, 0.0] and k['CLKC_COLD'].tolist() == [1.0, 0.0]
    assert k['CLKC_UNMET_OUTAGE'].tolist() == [1.0, 0.0]
    assert k['CLKC_HOT_MAX'].tolist() == [3.0, 0.0] and k['CLKC_HOT_MIN'].tolist() == [0.0, 0.0] and k['CLKC_HOT_SUM'].tolist() == [3.5, 0.0]
    assert k['CLKC_COLD_MAX'].tolist() == [2.5, 1.0] and k['CLKC_COLD_MIN'].tolist() == [0.0, 0.0] and k['CLKC_COLD_SUM'].tolist() == [2.5, 1.0]
