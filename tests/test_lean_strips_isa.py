"""Static checks on the strip path in the generated gfx950 code of `cl_step_lean_chain_kernel<4, true>` (no GPU: hipcc cross-compiles to assembly;
the parser and the burst finder are tests/test_isa_store_waits.py's).  In the uniform body the last four waves of a 17-building workgroup take the
17th building as 64-env strips BEHIND their main building (csrc/cl_kernels.hip, STRIPS).  That only pays if nothing between the two pieces of
arithmetic waits for the main building's store acknowledgements:

  * the strip's four plane loads (`global_load_dword`, one env per lane -- every other plane load of the kernel is a `dwordx4`) are issued in the
    uniform body's load block, in front of its first float64 instruction, so the main building's own wait covers them;
  * the strip's parameter block, chain constants and table row are scalar loads: no vector load stands between the main building's burst and the
    strip's arithmetic;
  * no `s_waitcnt` with a vmcnt field stands between either burst of the uniform body and the float64 instruction that follows it -- a wave whose
    workgroup has no second tile goes from the first burst to the strip, one with a second tile from the second burst;
  * the kernel stays within 128 VGPRs and uses no scratch."""
import re

import pytest

from test_isa_store_waits import CHAIN, _asm, _has_vmcnt, _is_f64, _one, bodies
from citylearn_amd import _lib


@pytest.fixture(scope='module')
def chain(tmp_path_factory):
    main = _lib.LIB_SOURCES[0]
    kernels, meta = _asm(main, [], tmp_path_factory)
    k = _one(kernels, CHAIN)
    return kernels[k], meta[k]


def _next(ins, start, pred):
    return next(k for k in range(start + 1, len(ins)) if pred(ins[k]))


def _is_vector_load(x):
    return x.startswith(('global_load', 'buffer_load', 'flat_load', 'scratch_load'))


def _strip(ins):
    """(end of the generic body's last burst, the uniform body's first float64 instruction, the ends of its two bursts, the strip's first float64
    instruction, the strip's dword stores, the reduction's barrier)"""
    generic, uniform = bodies(ins)
    assert len(generic) == 2 and len(uniform) == 2, (generic, uniform)
    first_f64 = _next(ins, generic[-1][1], _is_f64)
    strip_f64 = _next(ins, uniform[-1][1], _is_f64)
    barrier = _next(ins, strip_f64, lambda x: x.startswith('s_barrier'))
    stores = [k for k in range(strip_f64, barrier) if re.match(r'global_store_dword\s.* nt$', ins[k])]
    return generic[-1][1], first_f64, [b[1] for b in uniform], strip_f64, stores, barrier


def test_strip_loads_are_issued_in_front_of_the_first_float64_instruction(chain):
    ins, _ = chain
    start, first_f64, _, _, stores, _ = _strip(ins)
    assert len(stores) == 5, stores                                   # the strip is there: soc, efficiency, capacity loss, net, reward
    loads = [k for k in range(start, len(ins)) if re.match(r'global_load_dword\s', ins[k])]
    assert len(loads) == 4, loads                                     # soc, efficiency, capacity loss, action
    assert all(k < first_f64 for k in loads), (loads, first_f64)


def test_strip_table_reads_are_scalar_loads(chain):
    ins, _ = chain
    _, _, (_, last), strip_f64, _, _ = _strip(ins)
    between = ins[last + 1:strip_f64]
    assert [x for x in between if x.startswith('s_load_dword')]
    assert not [x for x in between if _is_vector_load(x)]


def test_no_vector_wait_between_a_burst_and_the_arithmetic_behind_it(chain):
    ins, _ = chain
    _, _, ends, strip_f64, _, _ = _strip(ins)
    for end in ends:
        nxt = _next(ins, end, _is_f64)
        assert not [(k, ins[k]) for k in range(end + 1, nxt) if _has_vmcnt(ins[k])], end
    assert _next(ins, ends[-1], _is_f64) == strip_f64


def test_register_budget(chain):
    _, meta = chain
    assert meta['num_vgpr'] <= 128 and meta['private_seg_size'] == 0, meta
