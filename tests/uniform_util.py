"""Districts for the tests of the `CLD_LEAN_UNIFORM` hint (tests/test_lean_uniform_host.py, tests/test_gpu_lean_uniform.py), derived in memory
from the committed 2022 phase_all data.  A plain module like district_util.py: no fixtures, no conftest."""
import copy
from dataclasses import replace
from functools import lru_cache

from golden_util import golden
from citylearn_amd.schema import BatterySpec


@lru_cache(maxsize=None)
def tables_2022(n_bldg: int = 17):
    """Episode tables of the first `n_bldg` buildings of the 2022 phase_all district (every one with a battery and a storage action)."""
    g = golden('g2022_all')
    spec = g.spec() if n_bldg == 17 else g.spec(buildings=list(range(n_bldg)))
    return spec.episode_tables(0)


@lru_cache(maxsize=None)
def tables_last_without_battery():
    """The 17 buildings with the LAST one's battery removed (the loader's absent device; its storage action inactive): wave 0's second building
    at the default sixteen waves."""
    g = golden('g2022_all')
    spec = g.spec(inactive_actions=[['electrical_storage'] if i == 16 else [] for i in range(17)])
    buildings = [copy.copy(b) for b in spec.buildings]
    buildings[16] = replace(buildings[16], electrical_storage=BatterySpec())
    return replace(spec, buildings=buildings).episode_tables(0)
