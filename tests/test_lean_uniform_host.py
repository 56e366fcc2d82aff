"""`engine.lean_uniform`: the `CLD_LEAN_UNIFORM` hint is derived from the host tables alone, and is set exactly when every building of a
battery + PV district has a battery driven by action column = building index under the default reward with exponent 1.  No GPU."""
from dataclasses import replace

import numpy as np

from golden_util import golden
from uniform_util import tables_2022, tables_last_without_battery
from citylearn_amd import abi
from citylearn_amd.engine import REWARD_KINDS, lean_district, lean_uniform


def _with_params(tab, edit):
    params = np.ascontiguousarray(tab.params).copy()
    edit(params)
    return replace(tab, params=params)


def test_the_flag_is_a_free_bit_of_the_header():
    taken = [v for k, v in abi.CONSTANTS.items() if k.startswith('CLD_') and k not in ('CLD_LEAN_UNIFORM', 'CLD_REWARD_SHIFT', 'CLD_REWARD_MASK')]
    assert abi.CLD_LEAN_UNIFORM == 1 << 17
    assert not any(v & abi.CLD_LEAN_UNIFORM for v in taken) and not abi.CLD_REWARD_MASK & abi.CLD_LEAN_UNIFORM


def test_set_for_the_2022_district_and_its_subsets():
    for n in (17, 16, 3):
        tab = tables_2022(n)
        assert lean_district(tab) and lean_uniform(tab) and lean_uniform(tab, 'RewardFunction')


def test_not_set_when_a_building_has_no_battery():
    tab = tables_2022()

    def clear(params):
        params.view(np.uint32)[5, abi.CLP_FLAGS] &= ~np.uint32(abi.CLF_BATTERY)
    assert not lean_uniform(_with_params(tab, clear))
    assert lean_district(tables_last_without_battery()) and not lean_uniform(tables_last_without_battery())      # ... as the loader builds it


def test_not_set_when_a_reward_exponent_is_not_one():
    def square(params):
        params.view(np.float32)[16, abi.CLP_L_RW_EXPONENT] = 2.0
    assert not lean_uniform(_with_params(tables_2022(), square))
    assert not lean_uniform(golden('g2022_all').spec().episode_tables(0, reward_exponent=2.0))


def test_not_set_for_another_reward_kind():
    tab = tables_2022()
    for kind in REWARD_KINDS:
        assert lean_uniform(tab, kind) == (kind == 'RewardFunction')


def test_not_set_when_the_storage_columns_are_not_in_building_order():
    def swap(params):
        cols = params.view(np.int32)[:, abi.CLP_ACT_ELEC_STO]
        cols[[3, 4]] = cols[[4, 3]]
    assert not lean_uniform(_with_params(tables_2022(), swap))

    def drop(params):
        params.view(np.int32)[16, abi.CLP_ACT_ELEC_STO] = -1
    assert not lean_uniform(_with_params(tables_2022(), drop))


def test_not_set_for_a_thermal_district():
    tab = golden('g2020_cz1').spec().episode_tables(0)
    assert not lean_district(tab) and not lean_uniform(tab)


def test_not_set_with_flex_tables():
    assert not lean_uniform(replace(tables_2022(), flex=object()))
