"""Districts for the geometry tests of the fused rollout kernels (tests/test_gpu_rollout_geometry.py), all derived from the committed g2022_all
data with what the loader offers -- `buildings=`, `inactive_actions=`, `inactive_observations=`, `synthetic.tile_district`, `dataclasses.replace`:

  b1, b2           the first one / two buildings: ONE wave per workgroup (nw = 1), which then walks a 64- or 128-wide env tile alone and owns
                   every series; b1's wave has no second building
  b16, b31, b32    tiled + jittered: an even district (no wave without a second building), and the two that need nw = 16, the kernels' limit
                   (31: the last wave owns one building; 32: `lane < n_bldg` reaches the end of the [32] LDS rows)
  het17            the 17 buildings with four of them changed -- see HET_* below.  Two waves per building pair at the default nw = 9: building b
                   is wave b's first building for b < 9, wave (b - 9)'s second for b >= 9, and building 8 is wave 8's only one.

Every one of them is still a battery + PV district (CLD_LEAN).  A plain module like flex_synth.py: no fixtures, no conftest."""
import copy
from dataclasses import replace
from functools import lru_cache

import numpy as np

from golden_util import golden
from citylearn_amd import abi
from citylearn_amd.schema import BatterySpec
from citylearn_amd.synthetic import tile_district

DISTRICTS = ('b1', 'b2', 'b16', 'b31', 'b32', 'het17')
N_BLDG = {'b1': 1, 'b2': 2, 'b16': 16, 'b31': 31, 'b32': 32, 'het17': 17}

# het17's four changed buildings, placed on all three seats a building can have at nw = 9 (and the two undriven ones in different waves):
HET_NO_BATTERY = 2         # a wave's FIRST building: no electrical storage at all (BatterySpec(), present=False: the loader's absent device), action inactive
HET_IDLE_ACTION = 13       # a wave's SECOND building: keeps its battery, but its electrical_storage action is inactive -- idles at action 0, keeps its losses
HET_NO_PV = 8              # wave 8's ONLY building: pv_nominal_power = 0
HET_SHORT_OBS = 15         # a wave's second building: its observation vector is one entry shorter
HET_DROPPED_OBSERVATION = 'carbon_intensity'       # env-independent, and ONE column also under the normalised layout (hour / month become two)
HET_UNDRIVEN = (HET_NO_BATTERY, HET_IDLE_ACTION)


@lru_cache(maxsize=None)
def district(name: str):
    """The DistrictSpec `name` (one of DISTRICTS, or 'g2022_all' itself)."""
    g = golden('g2022_all')
    if name == 'g2022_all':
        return g.spec()
    if name in ('b1', 'b2'):
        return g.spec(buildings=list(range(N_BLDG[name])))
    if name in ('b16', 'b31', 'b32'):
        return tile_district(g.spec(), N_BLDG[name])
    if name != 'het17':
        raise KeyError(name)
    n = N_BLDG['het17']
    spec = g.spec(inactive_actions=[['electrical_storage'] if i in HET_UNDRIVEN else [] for i in range(n)],
                  inactive_observations=[[HET_DROPPED_OBSERVATION] if i == HET_SHORT_OBS else [] for i in range(n)])
    buildings = [copy.copy(b) for b in spec.buildings]
    buildings[HET_NO_BATTERY] = replace(buildings[HET_NO_BATTERY], electrical_storage=BatterySpec())
    buildings[HET_NO_PV] = replace(buildings[HET_NO_PV], pv_nominal_power=0.0)
    return replace(spec, buildings=buildings)


def es_columns(tab) -> np.ndarray:
    """[n_bldg] the action column of every building's electrical storage (-1: none), as the kernels read it."""
    return np.ascontiguousarray(tab.params).view(np.int32)[:, abi.CLP_ACT_ELEC_STO].astype(np.int64)


def building_flags(tab) -> np.ndarray:
    return np.ascontiguousarray(tab.params).view(np.uint32)[:, abi.CLP_FLAGS]
