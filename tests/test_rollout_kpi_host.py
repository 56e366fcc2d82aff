"""The fused K-step rollout that keeps the streaming KPI accumulators (`cl_rollout_seq_f32` under `CLD_ROLLOUT_FUSED`, kernel
`cl_rollout_kpi_kernel` in csrc/cl_rollout.h), as far as it can be checked without a GPU: the flag and the ABI version, the generated gfx950
code of every instantiation (hipcc cross-compiles to assembly), and the argument validation, which happens before any HIP call."""
import ctypes
import re

import numpy as np
import pytest

from citylearn_amd import _lib, abi
from test_isa_guards import _asm, _count


@pytest.fixture(scope='module')
def lib():
    _lib.build()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    lib.cl_last_error.restype = ctypes.c_char_p
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.cl_rollout_seq_f32.argtypes = [ctypes.POINTER(_lib.Dims), vp, vp, vp, vp, i64, i64, i64, vp, vp, ctypes.c_uint64, vp, vp, vp, vp, vp, vp,
                                       ctypes.POINTER(_lib.Flex), i32, i32, vp]
    lib.cl_rollout_f32.argtypes = [ctypes.POINTER(_lib.Dims), vp, vp, vp, vp, i64, i64, i64, vp, vp, ctypes.c_uint64, vp, vp, vp, i32, i32, vp]
    return lib


def test_flag_and_abi_version(lib):
    assert abi.CL_ABI_VERSION == 9 == lib.cl_abi_version()
    f = abi.CLD_ROLLOUT_FUSED
    assert f and f & (f - 1) == 0 and f < 1 << 32                      # one bit of the 32-bit flag word
    others = {k: v for k, v in abi.CONSTANTS.items() if k.startswith('CLD_') and k not in ('CLD_ROLLOUT_FUSED', 'CLD_REWARD_SHIFT')}
    assert 'CLD_KPI' in others and 'CLD_REWARD_MASK' in others and len(others) == 13           # twelve flag bits + the reward mask
    for name, v in others.items():
        assert not f & v, name


@pytest.fixture(scope='module')
def units(tmp_path_factory):
    (main, _), (noslp, noslp_flags) = [(u, []) if not isinstance(u, tuple) else u for u in _lib.LIB_SOURCES]
    return _asm(main, [], tmp_path_factory), _asm(noslp, noslp_flags, tmp_path_factory)


def test_kpi_rollout_kernel_isa(units):
    """Every instantiation of cl_rollout_kpi_kernel<VEC, PREC>: the caps the existing guards put on the rollout and the KPI step kernels -- no
    scratch, no packed fp32, at most 128 registers (a 1024-thread workgroup's cap) -- and the wave-uniform reads (parameter blocks, time-series
    rows, the chain's float64 constants, the policy's bounds) as scalar loads although the K loop holds barriers (they go through the constant
    address space).  The vector loads that remain are all per-lane data: the 3 state and 4 control-sum planes of each of a wave's two buildings,
    the 12 + 12 accumulators of the control and the baseline district series on their way into LDS, the env block's 5 baseline sums, and the
    open-loop action tensor (a contiguous and a strided form); the compiler shares some of them between paths, and the count is pinned as
    generated -- 42 at one env per lane (all dword), 44 at two (16 of them dwordx2: the 14 planes and the two contiguous action reads).  A
    wave-uniform read that fell back to a per-lane fetch would show up here: the first build had 79 under the chain."""
    (main, _), (kernels, meta) = units
    assert not [k for k in main if 'cl_rollout_kpi_kernel' in k]                 # lives in the no-SLP unit only
    names = [k for k in kernels if 'cl_rollout_kpi_kernel' in k]
    by = {tuple(int(x) for x in re.search(r'cl_rollout_kpi_kernelILi(\d)ELi(\d)EE', k).groups()): k for k in names}
    assert len(by) == len(names) >= 2
    assert {p for _, p in by} == {0, 2} and {v for v, _ in by} <= {1, 2}
    for (vec, prec), k in by.items():
        ins = kernels[k]
        assert meta[k]['private_seg_size'] == 0, k
        assert meta[k]['num_vgpr'] <= 128, (k, meta[k])
        assert not [i for i in ins if i.startswith(('scratch_', 'buffer_load', 'buffer_store'))], k
        assert not [i for i in ins if re.match(r'v_pk_\w+_f32', i)], k
        assert _count(ins, 's_load') >= 30, (k, _count(ins, 's_load'))
        assert _count(ins, 'global_load') == {1: 42, 2: 44}[vec], (k, _count(ins, 'global_load'))
        assert any(i.startswith('v_fma_f64') for i in ins) == (prec == 2), k        # the float64 chain only where asked for
        assert _count(ins, 's_barrier') >= 3, k                                      # the fold's pair + MARL's exchange


def _dims(n_env=64, n_bldg=17, flags=0, **kw):
    d = _lib.Dims(n_env, n_bldg, 100, n_bldg, flags)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(lib, d, *, kpi_bldg=True, kpi_env=True, flex=None, k_steps=8, t0=0, policy=False, act_low=True):
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    return lib.cl_rollout_seq_f32(ctypes.byref(d), p, p, p, None if policy else p, 64 * 17, 64, 1, p if act_low else None, p if act_low else None, 3, None, p, p, p,
                                  p if kpi_bldg else None, p if kpi_env else None, flex, t0, k_steps, None)


def test_fused_kpi_rollout_refuses_what_the_kernel_does_not_cover(lib):
    """CLD_ROLLOUT_FUSED | CLD_KPI: CL_EINVAL / CL_ENULL with a message that names the cause, before any HIP call (this runs without a GPU)."""
    base = abi.CLD_ROLLOUT_FUSED | abi.CLD_KPI | abi.CLD_LEAN
    err = lambda: lib.cl_last_error().decode()
    assert _call(lib, _dims(flags=base & ~abi.CLD_LEAN)) == abi.CL_EINVAL and 'CLD_LEAN' in err() and 'thermal' in err()
    assert _call(lib, _dims(n_bldg=33, flags=base)) == abi.CL_EINVAL and 'n_bldg=33' in err() and 'chunked' in err()
    flex = _lib.Flex()
    assert _call(lib, _dims(flags=base), flex=ctypes.byref(flex)) == abi.CL_EINVAL and 'flex != NULL' in err()
    assert _call(lib, _dims(flags=base | abi.CLD_F64_MAPS)) == abi.CL_EINVAL and 'CLD_F64_MAPS' in err()
    assert _call(lib, _dims(flags=base | abi.CLD_WRITE_DETAIL)) == abi.CL_EINVAL and 'CLD_WRITE_DETAIL' in err()
    assert _call(lib, _dims(flags=base), kpi_bldg=False) == abi.CL_ENULL and 'kpi_bldg is NULL' in err()
    assert _call(lib, _dims(flags=base), kpi_env=False) == abi.CL_ENULL and 'kpi_env is NULL' in err()
    assert _call(lib, _dims(flags=base, env_pitch=128)) == abi.CL_EINVAL and 'env_pitch=128' in err()
    assert _call(lib, _dims(flags=base | (abi.CLR_EV << abi.CLD_REWARD_SHIFT))) == abi.CL_EINVAL and 'CLR_EV' in err()
    assert _call(lib, _dims(flags=base), t0=95) == abi.CL_ERANGE
    assert _call(lib, _dims(flags=base), policy=True, act_low=False) == abi.CL_ENULL and 'act_low' in err()
    # launch-geometry overrides: fewer waves than ceil(n_bldg / 2), and more waves than buildings (a wave without any building would read
    # parameter row `w` past the end of the table)
    tun = _lib.Tuning(nw=8)
    assert _call(lib, _dims(flags=base, tuning=ctypes.pointer(tun))) == abi.CL_EINVAL and 'bad nw 8' in err()
    assert _call(lib, _dims(n_bldg=5, flags=base, tuning=ctypes.pointer(tun))) == abi.CL_EINVAL and 'bad nw 8' in err()
    tun = _lib.Tuning(nw=2)
    assert _call(lib, _dims(n_bldg=1, flags=base, tuning=ctypes.pointer(tun))) == abi.CL_EINVAL and 'bad nw 2' in err()
    # the flag without CLD_KPI forwards to cl_rollout_f32 -- whose own refusals apply -- and still never takes the launch sequence
    assert _call(lib, _dims(flags=abi.CLD_ROLLOUT_FUSED | abi.CLD_LEAN), flex=ctypes.byref(flex)) == abi.CL_EINVAL and 'flex != NULL' in err()
    assert _call(lib, _dims(flags=abi.CLD_ROLLOUT_FUSED | abi.CLD_LEAN | abi.CLD_F64_MAPS)) == abi.CL_EINVAL and 'CLD_F64_MAPS' in err()
    assert _call(lib, _dims(flags=abi.CLD_ROLLOUT_FUSED | abi.CLD_LEAN | (abi.CLR_EV << abi.CLD_REWARD_SHIFT))) == abi.CL_EINVAL and 'CLR_EV' in err()


def test_rollout_f32_points_at_the_flag(lib):
    """cl_rollout_f32 has no KPI pointers and keeps refusing CLD_KPI; its message now names the way."""
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    d = _dims(flags=abi.CLD_KPI | abi.CLD_LEAN)
    assert lib.cl_rollout_f32(ctypes.byref(d), p, p, p, p, 64 * 17, 64, 1, p, p, 3, p, p, p, 0, 8, None) == abi.CL_EINVAL
    assert 'CLD_ROLLOUT_FUSED' in lib.cl_last_error().decode()


def test_launch_sequence_validation_is_unchanged_without_the_flag(lib):
    """cl_rollout_seq_f32 without CLD_ROLLOUT_FUSED: the return codes of the same bad arguments as before the flag existed."""
    flags = abi.CLD_KPI | abi.CLD_LEAN
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    odd = ctypes.c_void_p(buf.ctypes.data + 4)
    seq = lib.cl_rollout_seq_f32
    assert seq(None, p, p, p, p, 0, 0, 1, p, p, 0, None, p, p, p, p, p, None, 0, 8, None) == abi.CL_ENULL
    assert seq(ctypes.byref(_dims(n_env=6, flags=flags)), p, p, p, p, 0, 0, 1, p, p, 0, None, p, p, p, p, p, None, 0, 8, None) == abi.CL_EALIGN
    d = _dims(flags=flags)
    assert seq(ctypes.byref(d), p, p, p, odd, 0, 0, 1, p, p, 0, None, p, p, p, p, p, None, 0, 8, None) == abi.CL_EALIGN          # actions
    assert seq(ctypes.byref(d), p, p, p, p, 0, 0, 1, p, p, 0, None, p, p, odd, p, p, None, 0, 8, None) == abi.CL_EALIGN          # ret_env
    assert seq(ctypes.byref(d), p, p, p, None, 0, 0, 1, None, p, 0, p, p, p, p, p, p, None, 0, 8, None) == abi.CL_ENULL          # policy without bounds
    assert seq(ctypes.byref(d), p, p, p, None, 0, 0, 1, p, p, 0, None, p, p, p, p, p, None, 0, 8, None) == abi.CL_ENULL          # ... without scratch planes
    assert b'policy_actions' in lib.cl_last_error()
    assert seq(ctypes.byref(d), p, p, p, p, 0, 0, 1, p, p, 0, None, p, p, p, p, p, None, 95, 8, None) == abi.CL_ERANGE
    assert seq(ctypes.byref(d), p, p, p, p, 0, 0, 1, p, p, 0, None, p, p, p, p, p, None, -1, 8, None) == abi.CL_ERANGE
    assert seq(ctypes.byref(_dims(flags=flags | (9 << abi.CLD_REWARD_SHIFT))), p, p, p, p, 0, 0, 1, p, p, 0, None, p, p, p, p, p, None, 0, 8, None) == abi.CL_EINVAL


def test_lds_request_of_the_largest_geometries():
    """`rollout_kpi_lds_floats` with the header's constants: the figures the kernel's comment quotes, and which geometries have to opt into more
    than 64 KiB of dynamic LDS (from nw = 14 at two envs per lane: 27 to 32 buildings; tests/test_gpu_rollout_geometry.py launches 31 and 32)."""
    text = (_lib.CSRC / 'cl_rollout.h').read_text()
    s, nb = (int(re.search(rf'constexpr int {k} = (\d+);', text).group(1)) for k in ('CL_RKPI_S', 'CL_RKPI_NB'))
    assert re.search(r'return \(size_t\)CL_RKPI_S \* nw \* tile \+ \(size_t\)CLKE_PER_COND \* tile \+ 16 \+ \(size_t\)CL_RKPI_S \* 4 \* CL_RKPI_NB \+ 5 \* CL_RKPI_NB;', text)
    lds = lambda nw, tile: 4 * (s * nw * tile + abi.CLKE_PER_COND * tile + 16 + s * 4 * nb + 5 * nb)
    assert lds(16, 128) == 76480 and lds(9, 128) == 47808 and '76 480' in text and '47 808' in text
    assert lds(16, 64) <= 65536 and lds(13, 128) <= 65536 < lds(14, 128) and lds(16, 128) <= 160 * 1024
