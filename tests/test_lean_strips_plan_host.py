"""Where the step plan (csrc/cl_plan.h, compiled with g++ as in tests/test_step_plan_host.py) asks for the strip mapping of the plain float64-chain
launch: it shows in the LDS request alone -- one more [NQ][tile] row behind the wave rows -- since the kernel name stays what it is.  No GPU."""
import re

import pytest

from test_step_plan_host import plan, _flags        # noqa: F401  (`plan`: the module-scoped fixture of the host shim)
from citylearn_amd import abi

NAME = 'cl_step_lean_chain_kernel<4, true>'
ROW = abi.CL_NQ * 256 * 4                            # bytes of one LDS row at four envs per lane


def _uniform(precision='chain'):
    return _flags(True, precision) | abi.CLD_LEAN_UNIFORM | abi.CLD_ES_COL_IS_BLDG


@pytest.mark.parametrize('B,E,tuning,rows', [
    (17, 65536, None, 17),                           # the headline: 16 waves + the strips' row = 69 632 bytes
    (17, 65536, dict(lean_variant=32), 16),          # the off switch: wave 0's second tile
    (17, 256, dict(vec=4), 17), (17, 64, dict(vec=4), 17),
    (9, 1000, dict(vec=4, nw=8), 9),                 # one building more than waves at another size
    (18, 256, dict(vec=4), 16), (16, 256, dict(vec=4), 16), (32, 256, dict(vec=4), 16),
    (5, 256, dict(vec=4, nw=4), 5), (4, 256, dict(vec=4, nw=3), 3)])      # (fewer than four waves: no strips)
def test_lds_rows(plan, B, E, tuning, rows):
    rc, name, err, geom = plan(B, E, _uniform(), tuning=tuning)
    assert rc == abi.CL_OK and name == NAME, (name, err)
    assert geom[3] == rows * ROW, geom
    assert geom[2] == 64 * geom[4]                   # (the block is still one wave per building lane)


def test_no_strips_outside_the_uniform_chain_launch(plan):
    for flags, tuning, kw in ((_flags(True, 'chain'), None, {}),                      # no hint: the generic body
                              (_uniform(), dict(vec=4), dict(act_stride_env=17)),     # strided actions: the generic body
                              (_uniform('fp32'), None, {}),                           # the fp32 launch carries no uniform body
                              (_uniform(), dict(vec=2, lean_variant=2), {})):         # two envs per lane
        rc, name, err, geom = plan(17, 65536, flags, tuning=tuning, **kw)
        assert rc == abi.CL_OK, err
        vec = int(re.search(r'<(\d+),', name).group(1))
        assert 'cl_step_lean' in name and geom[3] == geom[4] * abi.CL_NQ * 64 * vec * 4, (name, geom)      # the wave rows alone
    rc, name, err, geom = plan(17, 65536, _uniform() | abi.CLD_KPI, None)               # the KPI launch: its own kernel, its baseline words
    assert rc == abi.CL_OK and name.startswith('cl_step_lean_kpi_chain_kernel<4') and geom[3] == 16 * ROW + 32 * 4, (name, geom)
