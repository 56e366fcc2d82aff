"""tests/district_util.py builds what tests/test_gpu_rollout_geometry.py says it runs (no GPU needed): building counts, the wave split they
produce, per-building flags and action columns as the kernels read them from the packed tables, the lean classification, and het17's
observation vectors."""
import numpy as np
import pytest

from district_util import (DISTRICTS, HET_DROPPED_OBSERVATION, HET_IDLE_ACTION, HET_NO_BATTERY, HET_NO_PV, HET_SHORT_OBS, HET_UNDRIVEN, N_BLDG,
                           building_flags, district, es_columns)
from citylearn_amd import abi
from citylearn_amd.observations import ObservationLayout
from citylearn_amd.policy import building_columns


def _lean(tab) -> bool:
    """`StepEngine`'s classification (engine.py), on the host."""
    heavy = abi.CLF_THERMAL | abi.CLF_OUTAGE | abi.CLF_DYNAMICS
    return not bool(np.any(building_flags(tab) & heavy)) and not bool(np.any(tab.ts[:, :, [abi.CLT_COOL_DEM, abi.CLT_HEAT_DEM, abi.CLT_DHW_DEM]]))


@pytest.mark.parametrize('name', DISTRICTS)
def test_every_district_is_lean_and_has_the_intended_size(name):
    spec = district(name)
    tab = spec.episode_tables(0)
    B = N_BLDG[name]
    assert len(spec.buildings) == B == tab.params.shape[0] and B <= 32
    assert _lean(tab) and tab.flex is None
    assert len({b.name for b in spec.buildings}) == B
    nw = (B + 1) // 2
    assert nw == {'b1': 1, 'b2': 1, 'b16': 8, 'b31': 16, 'b32': 16, 'het17': 9}[name]
    assert (B % 2 == 1) == (name in ('b1', 'b31', 'het17'))                       # a last wave with one building
    if name != 'het17':
        assert np.all(building_flags(tab) & abi.CLF_BATTERY) and np.array_equal(es_columns(tab), np.arange(B))
        assert np.all(tab.ts[:, :, abi.CLT_SOLAR].min(axis=0) < 0)                # every building generates
    if name in ('b16', 'b31', 'b32'):
        # the jittered device sizes keep the copies of a building distinct
        pf = tab.params_f32()
        assert len({(float(pf[i, abi.CLP_B_CAP]), float(pf[i, abi.CLP_B_POW])) for i in range(B)}) == B


def test_het17_is_what_the_geometry_tests_assume():
    spec = district('het17')
    tab = spec.episode_tables(0)
    flags, es = building_flags(tab), es_columns(tab)
    # the three seats of a building at nw = 9: a wave's first (b < 8), wave 8's only one (b = 8), a wave's second (b >= 9) -- all hit,
    # and the two undriven buildings in different waves, one on each of a wave's two seats
    changed = {HET_NO_BATTERY, HET_IDLE_ACTION, HET_NO_PV, HET_SHORT_OBS}
    assert len(changed) == 4 and any(b < 8 for b in changed) and 8 in changed and any(b >= 9 for b in changed)
    assert HET_NO_BATTERY < 8 and HET_IDLE_ACTION >= 9 and HET_NO_BATTERY % 9 != HET_IDLE_ACTION % 9
    for b in range(17):
        assert bool(flags[b] & abi.CLF_BATTERY) == (b != HET_NO_BATTERY), b
        assert (es[b] < 0) == (b in HET_UNDRIVEN), b
    # the action columns are the driven buildings in building order: column b is NOT building b behind the first undriven one
    driven = [b for b in range(17) if b not in HET_UNDRIVEN]
    assert np.array_equal(es[driven], np.arange(15)) and len(spec.action_limits()[0]) == 15 and es[16] == 14
    absent, idle = spec.buildings[HET_NO_BATTERY].electrical_storage, spec.buildings[HET_IDLE_ACTION].electrical_storage
    assert not absent.present and absent.capacity == 0.0 and idle.present and idle.capacity > 0 and idle.nominal_power > 0
    assert spec.buildings[HET_NO_PV].pv_nominal_power == 0.0 and not np.any(tab.ts[:, HET_NO_PV, abi.CLT_SOLAR])
    assert np.all(tab.ts[:, [b for b in range(17) if b != HET_NO_PV], abi.CLT_SOLAR].min(axis=0) < 0)
    for normalize in (True, False):
        lengths = [len(c) for c in building_columns(ObservationLayout(spec, 'current', normalize))]
        assert lengths[HET_SHORT_OBS] == max(lengths) - 1 and sorted(set(lengths)) == [max(lengths) - 1, max(lengths)]
        assert sum(n != max(lengths) for n in lengths) == 1
    assert HET_DROPPED_OBSERVATION not in spec.buildings[HET_SHORT_OBS].active_observations
    assert HET_DROPPED_OBSERVATION in spec.buildings[0].active_observations
    # the source district is untouched (the builder copies what it changes)
    base = district('g2022_all')
    assert base.buildings[HET_NO_BATTERY].electrical_storage.present and base.buildings[HET_NO_PV].pv_nominal_power > 0
