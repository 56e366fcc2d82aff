"""The building-chunked closed-loop policy rollout of thermal districts that keeps the streaming KPIs (`clpfck_rollout_mlp_kpi_f32`, kernels
`cl_rollout_full_policy_chunk_kpi_kernel`: csrc/cl_policy_full.h at KPI = CHUNK = true, and `cl_kpi_series_chunk_kernel` in csrc/cl_policy_full_chunk_kpi.h, library
``libcitylearn_amd_policy_full_chunk_kpi.so``) as far as it can be checked without a GPU: the library's symbol list, the argument validation (before
any HIP call), the scratch size, registers / scratch memory / LDS of both instantiations.  The conditioning of the closed loop on the districts the
GPU tests run (tests/test_gpu_policy_full_chunk_kpi_rollout.py, H = 16) is held by tests/test_policy_full_chunk_host.py."""
import ctypes
import re

import numpy as np
import pytest

from citylearn_amd import _lib, abi, policy
from policy_full_chunk_util import default_chunks
from policy_util import exports
from test_isa_guards import _asm

KPI = abi.CLD_KPI


@pytest.fixture(scope='module')
def lib():
    _lib.build_policy_full_chunk_kpi()
    lib = ctypes.CDLL(str(_lib.POLICY_FULL_CHUNK_KPI_LIB_PATH))
    lib.clpfck_last_error.restype = ctypes.c_char_p
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.clpfck_rollout_mlp_kpi_f32.argtypes = [ctypes.POINTER(_lib.Dims), vp, vp, vp, ctypes.POINTER(_lib.PolicyFullMLP), vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, vp]
    lib.clpfck_series_scratch_floats.restype = i64
    lib.clpfck_series_scratch_floats.argtypes = [ctypes.POINTER(_lib.Dims), i32]
    return lib


# ---- 1. the library -------------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header(lib):
    want = ['clpfck_abi_version', 'clpfck_core_abi_version', 'clpfck_last_error', 'clpfck_rollout_mlp_kpi_f32', 'clpfck_series_scratch_floats']
    assert _lib.POLICY_FULL_CHUNK_KPI_SYMBOLS == want
    assert exports(_lib.POLICY_FULL_CHUNK_KPI_LIB_PATH) == want
    assert lib.clpfck_abi_version() == _lib.POLICY_FULL_CHUNK_KPI_ABI_VERSION == 1 and lib.clpfck_core_abi_version() == abi.CL_ABI_VERSION
    # `clpf_mlp` is shared, not redefined
    assert 'typedef struct' not in abi._strip_comments(_lib.POLICY_FULL_CHUNK_KPI_HEADER.read_text())
    ext = _lib.POLICY_FULL_CHUNK_KPI
    assert ext.mlp is _lib.PolicyFullMLP and ext.n_kpi == 2 and ext.extra == (ctypes.c_void_p, ctypes.c_int64)


def test_the_other_libraries_and_the_pinned_tuples_are_what_they_were():
    lists = {'clpol': ['rollout_mlp_f32'], 'clpk': ['rollout_mlp_kpi_f32'], 'clpf': ['rollout_mlp_f32'], 'clpfk': ['rollout_mlp_kpi_f32'],
             'clpfc': ['rollout_mlp_f32']}
    assert [e.prefix for e in _lib.ALL_EXTENSIONS] == list(lists)
    for e in _lib.ALL_EXTENSIONS:
        assert e.symbols == [f'{e.prefix}_{n}' for n in ['abi_version', 'core_abi_version', 'last_error'] + lists[e.prefix]] and e.abi_version == 1
        assert e.extra == () and e.functions == ()
    assert _lib.EXTENSIONS == (_lib.POLICY, _lib.POLICY_KPI, _lib.POLICY_FULL, _lib.POLICY_FULL_KPI) and len(_lib.EXTENSIONS) == 4
    assert _lib.ALL_EXTENSIONS == _lib.EXTENSIONS + (_lib.POLICY_FULL_CHUNK,) and len(_lib.ALL_EXTENSIONS) == 5
    assert _lib.CHUNK_KPI_EXTENSIONS == (_lib.POLICY_FULL_CHUNK_KPI,)
    every = _lib.ALL_EXTENSIONS + _lib.CHUNK_KPI_EXTENSIONS
    assert len({e.path for e in every}) == 6 and len({e.prefix for e in every}) == 6
    kind = policy.StorageMLPPolicy.kind
    assert kind.ext_chunk_kpi is _lib.POLICY_FULL_CHUNK_KPI and kind.ext_chunk is _lib.POLICY_FULL_CHUNK and kind.ext_kpi is _lib.POLICY_FULL_KPI
    assert policy.MLPPolicy.kind.ext_chunk_kpi is None


def test_build_builds_the_library():
    import inspect
    import __graft_entry__
    assert '_lib.ALL_EXTENSIONS + _lib.CHUNK_KPI_EXTENSIONS' in inspect.getsource(__graft_entry__.build)


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------------
def _dims(n_env=64, n_bldg=17, flags=KPI, **kw):
    d = _lib.Dims(n_env, n_bldg, 100, 45, flags)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(lib, d, *, t0=0, k_steps=8, state=True, traj_odd=False, null=None, scratch_floats=1 << 40, **mlp_kw):
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data
    a = {k: (None if k == null else p) for k in ('params', 'ts', 'out_bldg', 'out_env', 'kpi_bldg', 'kpi_env', 'series_scratch')}
    m = dict(n_hidden=16, n_sets=1, n_device_cols=0, reserved=0, pre=p, dep=p, out=p, set_of_block=None, net_reset=None, act_low=p, act_high=p, sigma=None, seed=1)
    m.update(mlp_kw)
    mlp = _lib.PolicyFullMLP(**m)
    return lib.clpfck_rollout_mlp_kpi_f32(ctypes.byref(d) if d is not None else None, a['params'], a['ts'], p if state else None, ctypes.byref(mlp),
                                          a['out_bldg'], a['out_env'], None, p + 4 if traj_odd else None, a['kpi_bldg'], a['kpi_env'],
                                          a['series_scratch'], scratch_floats, t0, k_steps, None)


def test_refusals_name_their_cause_before_any_hip_call(lib):
    """Every refusal returns its code with a message that names the cause; the buffers are 256 bytes of host memory, so a call that got as far as a
    launch would not come back with one of these codes."""
    err = lambda: lib.clpfck_last_error().decode()
    EINVAL, ENULL, EALIGN, ERANGE = abi.CL_EINVAL, abi.CL_ENULL, abi.CL_EALIGN, abi.CL_ERANGE
    tuned = lambda **kw: ctypes.pointer(_lib.Tuning(**kw))
    assert _call(lib, None) == ENULL and 'dims is NULL' in err()
    assert _call(lib, _dims(n_env=6)) == EALIGN and 'multiple of 4' in err()
    # what differs from clpfc_rollout_mlp_f32
    assert _call(lib, _dims(flags=0)) == EINVAL and 'CLD_KPI' in err() and 'without them the call is clpfc_rollout_mlp_f32' in err()
    assert _call(lib, _dims(flags=KPI | abi.CLD_WRITE_DETAIL)) == EINVAL and 'CLD_WRITE_DETAIL' in err() and 'CLD_DETAIL_MIN' in err()
    assert _call(lib, _dims(tuning=tuned(vec=2))) == EINVAL and '2 envs per lane' in err() and 'one env per lane' in err()
    assert _call(lib, _dims(tuning=tuned(vec=4))) == EINVAL and '4 envs per lane' in err()
    for name in ('kpi_bldg', 'kpi_env', 'series_scratch'):
        assert _call(lib, _dims(), null=name) == ENULL and f'{name} is NULL' in err()
    need = 8 * 2 * 3 * 64                                            # 17 buildings: three chunks
    assert _call(lib, _dims(), scratch_floats=need - 1) == EINVAL and 'series_scratch' in err() and str(need) in err() and '3 chunks' in err()
    assert _call(lib, _dims(), scratch_floats=0) == EINVAL and 'series_scratch' in err()
    # what it shares with it
    assert _call(lib, _dims(flags=KPI | abi.CLD_LEAN)) == EINVAL and 'CLD_LEAN' in err() and 'clpk_rollout_mlp_kpi_f32' in err()
    assert _call(lib, _dims(flags=KPI | abi.CLR_MARL << abi.CLD_REWARD_SHIFT)) == EINVAL and 'CLR_MARL' in err() \
        and 'a building-chunked launch cannot couple the buildings inside a step' in err()
    assert _call(lib, _dims(flags=KPI | abi.CLR_EV << abi.CLD_REWARD_SHIFT)) == EINVAL and 'CLR_EV' in err()
    assert _call(lib, _dims(flags=KPI | 9 << abi.CLD_REWARD_SHIFT)) == EINVAL and 'unknown reward kind' in err()
    assert _call(lib, _dims(flags=KPI | abi.CLD_F64_MAPS)) == EINVAL and 'CLD_F64_MAPS' in err()
    assert _call(lib, _dims(env_pitch=128)) == EINVAL and 'env_pitch=128' in err()
    assert _call(lib, _dims(), n_device_cols=2) == EINVAL and 'device action column' in err() and 'n_device_cols=2' in err()
    assert _call(lib, _dims(), reserved=1) == EINVAL and 'reserved must be 0' in err()
    assert _call(lib, _dims(n_act_cols=65537)) == EINVAL and 'n_act_cols=65537' in err()
    for h in (0, 2, 6, 36, 64, -4):
        assert _call(lib, _dims(), n_hidden=h) == EINVAL and f'n_hidden={h}' in err()
    assert _call(lib, _dims(), n_sets=0) == EINVAL and 'n_sets=0' in err()
    for name in ('pre', 'dep', 'out', 'act_low', 'act_high'):
        assert _call(lib, _dims(), **{name: None}) == ENULL and f'mlp.{name} is NULL' in err()
    assert _call(lib, _dims(), state=False) == ENULL and 'state is NULL' in err()
    for name in ('params', 'ts', 'out_bldg', 'out_env'):
        assert _call(lib, _dims(), null=name) == ENULL and f'{name} is NULL' in err()
    odd = np.zeros(64, dtype=np.float32).ctypes.data + 4
    for name in ('pre', 'dep', 'out', 'net_reset', 'act_low', 'act_high', 'sigma'):
        assert _call(lib, _dims(), **{name: odd}) == EALIGN and f'mlp.{name} is not 16-byte aligned' in err()
    assert _call(lib, _dims(), set_of_block=odd + 1) == EALIGN and 'set_of_block' in err()
    assert _call(lib, _dims(), traj_odd=True) == EALIGN and 'traj' in err()
    assert _call(lib, _dims(), t0=95) == ERANGE and '[95, 103)' in err()
    assert _call(lib, _dims(), t0=-1) == ERANGE and _call(lib, _dims(), k_steps=-1) == ERANGE
    # the chunk geometry
    assert _call(lib, _dims(tuning=tuned(b_chunk=17))) == EINVAL and 'b_chunk=17' in err() and 'at most 16' in err()
    assert _call(lib, _dims(n_bldg=9)) == EINVAL and 'n_bldg=9' in err() and 'clpfk_rollout_mlp_kpi_f32' in err()
    assert _call(lib, _dims(n_bldg=16)) == EINVAL and 'n_bldg=16' in err() and 'clpfk_rollout_mlp_kpi_f32' in err()
    assert _call(lib, _dims(n_bldg=12, tuning=tuned(b_chunk=16))) == EINVAL and 'b_chunk=16 >= n_bldg=12' in err() and 'clpfk_rollout_mlp_kpi_f32' in err()
    assert _call(lib, _dims(tuning=tuned(b_chunk=5))) == EINVAL and 'b_chunk=5 leaves no room for the 4 chunk partial sums' in err()
    assert _call(lib, _dims(tuning=tuned(nw=8))) == EINVAL and 'bad nw 8' in err() and 'b_chunk = 6' in err()
    # CLD_WRITE_DETAIL together with CLD_DETAIL_MIN is accepted: the next check is what refuses
    assert _call(lib, _dims(flags=KPI | abi.CLD_WRITE_DETAIL | abi.CLD_DETAIL_MIN, env_pitch=128)) == EINVAL and 'env_pitch=128' in err()


def test_series_scratch_floats(lib):
    """k x 2 x n_chunks x n_env at the default geometry and at an explicit one; a geometry the call refuses is refused here, with its message."""
    for n_bldg in (17, 24, 33, 1024):
        nc = default_chunks(n_bldg)[1]
        assert nc == {17: 3, 24: 3, 33: 5, 1024: 128}[n_bldg]
        for k, E in ((1, 64), (30, 260), (64, 1024)):
            assert lib.clpfck_series_scratch_floats(ctypes.byref(_dims(n_env=E, n_bldg=n_bldg)), k) == k * 2 * nc * E
    assert lib.clpfck_series_scratch_floats(ctypes.byref(_dims(n_bldg=1024, n_env=1024)), 720) * 4 == 754974720        # 755 MB unwindowed
    assert lib.clpfck_series_scratch_floats(ctypes.byref(_dims(n_bldg=1024, n_env=1024)), 64) * 4 == 1 << 26           # 64 MiB at the window
    t = ctypes.pointer(_lib.Tuning(b_chunk=16))
    assert lib.clpfck_series_scratch_floats(ctypes.byref(_dims(tuning=t)), 30) == 30 * 2 * 2 * 64
    assert lib.clpfck_series_scratch_floats(ctypes.byref(_dims()), 0) == 0
    t = ctypes.pointer(_lib.Tuning(b_chunk=5))
    assert lib.clpfck_series_scratch_floats(ctypes.byref(_dims(tuning=t)), 30) == -abi.CL_EINVAL and 'leaves no room' in lib.clpfck_last_error().decode()
    assert lib.clpfck_series_scratch_floats(None, 30) == -abi.CL_ENULL
    assert lib.clpfck_series_scratch_floats(ctypes.byref(_dims()), -1) == -abi.CL_ERANGE


# ---- 3. generated code ----------------------------------------------------------------------------------------------------------------
def test_kernel_isa(tmp_path_factory):
    """Exactly the two instantiations of cl_rollout_full_policy_kernel<1, PREC, false, KPI = true, CHUNK = true> (csrc/cl_policy_full.h: reported as
    `cl_rollout_full_policy_chunk_kpi_kernel<PREC>`), one cl_kpi_series_chunk_kernel and one cl_finish_kernel, and no instantiation of the blind chunk
    kernel, the chunked kernel without KPIs or the one-row kernels in this unit; the rollout kernel at most 128 VGPRs (a 1024-thread
    workgroup's cap), no scratch memory, no static LDS (it is all dynamic: `_lib.policy_full_chunk_kpi_lds_bytes`)."""
    (src,) = _lib.POLICY_FULL_CHUNK_KPI_SOURCES
    kernels, meta = _asm(src, [], tmp_path_factory)
    names = [k for k in kernels if 'cl_rollout_full_policy_kernel' in k]
    by = {int(re.search(r'cl_rollout_full_policy_kernelILi1ELi(\d)ELb0ELb1ELb1EE', k).group(1)): k for k in names}
    assert sorted(by) == [0, 2] and len(names) == 2
    assert not [k for k in kernels if (re.search(r'cl_rollout_full_policy_kernelILi\dELi\dELb\dELb\dELb\dEE', k) and 'ELb0ELb1ELb1EE' not in k) or 'cl_rollout_full_kernel' in k]
    (series,) = [k for k in kernels if 'cl_kpi_series_chunk_kernel' in k]
    assert len([k for k in kernels if 'cl_finish_kernel' in k]) == 1
    text = next(tmp_path_factory.getbasetemp().glob('isa*/' + src.stem + '.s')).read_text()
    static_lds = {m.group(1): int(m.group(2)) for m in re.finditer(r'\.amdhsa_kernel (\w+)\n(?:.*\n)*?\s*\.amdhsa_group_segment_fixed_size (\d+)', text)}
    for prec, k in by.items():
        assert meta[k]['private_seg_size'] == 0, (k, meta[k])
        assert meta[k]['num_vgpr'] <= 128, (k, meta[k])
        assert static_lds[k] == 0, (k, static_lds[k])
        print(prec, meta[k])
    assert meta[series]['private_seg_size'] == 0 and meta[series]['num_vgpr'] <= 128, meta[series]
    assert static_lds[series] == 4 * (64 * 2 * 64 + 2 * abi.CLKE_PER_COND * 64)       # a batch of 64 steps' samples and the two series


def test_lds_formula():
    """`_lib.policy_full_chunk_kpi_lds_bytes` is the header's `rollout_full_policy_chunk_kpi_lds_floats` (csrc/cl_policy_full.h): ring [S][2][nw][64] + rows [nw][CLPF_ROW]."""
    head = (_lib.CSRC / 'cl_policy_full.h').read_text()
    assert re.search(r'rollout_full_policy_chunk_kpi_lds_floats\(int nw\) \{ return \(size_t\)CL_RKPI_S \* 2 \* nw \* 64 \+ \(size_t\)nw \* CLPF_ROW; \}', head)
    assert re.search(r'constexpr int CL_RKPI_S = 8;', (_lib.CSRC / 'cl_rollout.h').read_text())
    row = 4 * (policy.CLPF_ND + policy.CLPF_NA) * (policy.CLPF_MAX_HIDDEN // 4) + 8 * policy.CLPF_NA
    for nw in (1, 5, 6, 7, 8, 16):
        assert _lib.policy_full_chunk_kpi_lds_bytes(nw) == 4 * (8 * 2 * nw * 64 + nw * row)
    assert _lib.policy_full_chunk_kpi_lds_bytes(8) == 43008 and 65536 < _lib.policy_full_chunk_kpi_lds_bytes(16) == 86016 <= 160 * 1024
