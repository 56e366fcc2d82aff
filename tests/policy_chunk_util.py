"""Shared by tests/test_policy_chunk_host.py and tests/test_gpu_policy_chunk_rollout.py: the battery + PV districts of MORE than 32 buildings the
building-chunked policy rollout is tested on (`clpc_rollout_mlp_f32`, csrc/cl_policy_chunk.h), all derived from g2022_all.  Test policies and
their weight scale: tests/policy_util.py (`make_policy`).

  b33, b64, b1024   `tile_district(g2022_all, n)`: 17 + 16 (nw = 9: wave 8 of the first chunk has one building, of the second none), 32 + 32,
                    32 x 32 (BASELINE config 4's size)
  het40             `tile_district(district_util.district('het17'), 40)`, 20 + 20: buildings 2, 13, 19, 30 and 36 have no driven storage action
                    (2, 19, 36 no battery at all), buildings 8 and 25 no PV, observation vectors of 30 and 31 entries
  b32, het17        tests/district_util.py's, one workgroup row's worth: chunked only with an explicit b_chunk (against the one-row kernel)

The loop's conditioning on these districts (tests/test_policy_host.py::_conditioning: K = 48, E = 4, worst of soc / net in units of the plain bar
1e-4 + 1e-4 |ref|; the project admits 0.1), as soc / net:
    district   H = 4            H = 16           H = 32
    b33        0.013 / 0.038    0.007 / 0.036    0.011 / 0.041
    het40      0.008 / 0.071    0.009 / 0.024    0.016 / 0.056
    b64        0.027 / 0.078    0.017 / 0.057      --  / 0.161    (over the 0.1: replay tests only)
    b1024                         --  / 0.111                     (over the 0.1: replay tests only)
So the free-running comparison runs on b33 and het40; b64 at H = 32 and b1024 are replayed through single steps, never compared free-running."""
from functools import lru_cache

import district_util
from golden_util import golden

# (district, H) cells the conditioning test holds under 0.1 and the GPU tests may run free
CONDITIONED = [(name, H) for name in ('b33', 'het40') for H in (4, 16, 32)] + [('b64', 4), ('b64', 16)]

N_BLDG = {'b32': 32, 'het17': 17, 'b33': 33, 'het40': 40, 'b64': 64, 'b1024': 1024}
HET40_UNDRIVEN = (2, 13, 19, 30, 36)


@lru_cache(maxsize=None)
def chunk_district(name: str):
    from citylearn_amd.synthetic import tile_district
    if name in ('b32', 'het17'):
        return district_util.district(name)
    if name == 'het40':
        return tile_district(district_util.district('het17'), 40)
    return tile_district(golden('g2022_all').spec(), N_BLDG[name])


def default_chunks(n_bldg: int):
    """(b_chunk, n_chunks, nw) of the library's default geometry: the blind chunked rollout's 32-building workgroups, balanced."""
    nc = -(-n_bldg // 32)
    b = -(-n_bldg // nc)
    return b, -(-n_bldg // b), -(-b // 2)
