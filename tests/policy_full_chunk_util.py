"""Shared by tests/test_policy_full_chunk_host.py and tests/test_gpu_policy_full_chunk_rollout.py: the thermal districts of MORE than 16 buildings the
building-chunked policy rollout is tested on (`clpfc_rollout_mlp_f32`, csrc/cl_policy_full.h at CHUNK = true).  Test policies and their weight scale:
tests/policy_full_util.py (`make_storage_policy`).

The loop's conditioning on these districts (tests/test_policy_full_host.py::_conditioning: K = 48, E = 4, worst of soc / cs / ds / net in units of
1e-4 + 1e-4 |ref|; the project admits 0.1):
    district      H = 4    H = 16   H = 32
    t17           0.020    0.033    0.016
    t24           0.026    0.027    0.027
    t33           0.044    0.025    0.028
    t17_outage    0.138    0.018    0.018        (H = 4 is over the 0.1: the outage district runs at H = 16 or 32 only)
Actions span about +-0.09 of the bounds and every building has 2 or 3 heads."""
from functools import lru_cache

from golden_util import golden
from policy_full_util import thermal_district

# (district, H) cells the conditioning test holds under 0.1 and the GPU tests may use
CONDITIONED = [(name, H) for name in ('t17', 't24', 't33', 't17_outage') for H in (4, 16, 32) if (name, H) != ('t17_outage', 4)]

# how the default geometry cuts a district: n_chunks = ceil(n_bldg / 8), b_chunk = ceil(n_bldg / n_chunks)
DEFAULT_B_CHUNK = {17: 6, 24: 8, 33: 7, 1024: 8}


@lru_cache(maxsize=None)
def chunk_district(name: str):
    """'t16' (one workgroup row's worth: chunked only with an explicit b_chunk), 't17' (6 + 6 + 5: a last chunk with a wave without a building),
    't17_outage' -- policy_full_util's; 't24' (b_chunk = 8: three full chunks), 't33' (7 + 7 + 7 + 7 + 5) and 't1024' (BASELINE config 4's district:
    128 chunks of eight, more than the 64 chunks one pass of cl_finish_kernel's sixteen waves adds) tiled out of g2020_cz1's nine buildings."""
    from citylearn_amd.synthetic import tile_district
    if name in ('t16', 't17', 't17_outage'):
        return thermal_district(name)
    return tile_district(golden('g2020_cz1').spec(), {'t24': 24, 't33': 33, 't1024': 1024}[name])


def default_chunks(n_bldg: int):
    """(b_chunk, n_chunks) of the library's default geometry."""
    nc = -(-n_bldg // 8)
    b = -(-n_bldg // nc)
    return b, -(-n_bldg // b)
