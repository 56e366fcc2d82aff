"""The closed-loop policy rollout of thermal districts that keeps the streaming KPIs (`clpfk_rollout_mlp_kpi_f32`, kernel
`cl_rollout_full_policy_kpi_kernel`: csrc/cl_policy_full.h at KPI = true, library ``libcitylearn_amd_policy_full_kpi.so``) as far as it can be checked
without a GPU: the library's symbol list, the argument validation (before any HIP call), registers / scratch / LDS of every instantiation -- and
that the thermal policy library without KPIs is what it was."""
import ctypes
import re

import numpy as np
import pytest

from citylearn_amd import _lib, abi
from policy_util import exports
from test_isa_guards import _asm


@pytest.fixture(scope='module')
def lib():
    _lib.build_policy_full_kpi()
    lib = ctypes.CDLL(str(_lib.POLICY_FULL_KPI_LIB_PATH))
    lib.clpfk_last_error.restype = ctypes.c_char_p
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.clpfk_rollout_mlp_kpi_f32.argtypes = [ctypes.POINTER(_lib.Dims), vp, vp, vp, ctypes.POINTER(_lib.PolicyFullMLP), vp, vp, vp, vp, vp, vp, i32, i32, vp]
    return lib


def test_library_exports_exactly_the_header(lib):
    assert _lib.POLICY_FULL_KPI_SYMBOLS == ['clpfk_abi_version', 'clpfk_core_abi_version', 'clpfk_last_error', 'clpfk_rollout_mlp_kpi_f32']
    assert exports(_lib.POLICY_FULL_KPI_LIB_PATH) == _lib.POLICY_FULL_KPI_SYMBOLS
    assert lib.clpfk_abi_version() == _lib.POLICY_FULL_KPI_ABI_VERSION == 1 and lib.clpfk_core_abi_version() == abi.CL_ABI_VERSION
    assert _lib.POLICY_FULL_KPI in _lib.EXTENSIONS and len(_lib.EXTENSIONS) == 4
    assert _lib.POLICY_FULL_KPI.mlp is _lib.PolicyFullMLP and _lib.POLICY_FULL_KPI.n_kpi == 2
    assert not [k for k in abi.CONSTANTS if k.startswith('CLPFK')]


KPI = abi.CLD_KPI


def _dims(n_env=64, n_bldg=9, flags=KPI, **kw):
    d = _lib.Dims(n_env, n_bldg, 100, 25, flags)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(lib, d, *, t0=0, k_steps=8, state=True, traj_odd=False, null=None, **mlp_kw):
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data
    a = {k: (None if k == null else p) for k in ('params', 'ts', 'out_bldg', 'out_env', 'kpi_bldg', 'kpi_env')}
    m = dict(n_hidden=16, n_sets=1, n_device_cols=0, reserved=0, pre=p, dep=p, out=p, set_of_block=None, net_reset=None, act_low=p, act_high=p, sigma=None, seed=1)
    m.update(mlp_kw)
    mlp = _lib.PolicyFullMLP(**m)
    return lib.clpfk_rollout_mlp_kpi_f32(ctypes.byref(d) if d is not None else None, a['params'], a['ts'], p if state else None, ctypes.byref(mlp),
                                         a['out_bldg'], a['out_env'], None, p + 4 if traj_odd else None, a['kpi_bldg'], a['kpi_env'], t0, k_steps, None)


def test_refusals_name_their_cause_before_any_hip_call(lib):
    """Every buffer below is host memory (or NULL): a call that got past its checks would fault in the launch, so each return code is a refusal
    made before any HIP call."""
    err = lambda: lib.clpfk_last_error().decode()
    EINVAL, ENULL, EALIGN, ERANGE = abi.CL_EINVAL, abi.CL_ENULL, abi.CL_EALIGN, abi.CL_ERANGE
    assert _call(lib, None) == ENULL and 'dims is NULL' in err()
    assert _call(lib, _dims(n_env=6)) == EALIGN and 'multiple of 4' in err()
    assert _call(lib, _dims(flags=KPI | abi.CLD_LEAN)) == EINVAL and 'CLD_LEAN' in err() and 'clpk_rollout_mlp_kpi_f32' in err()
    assert _call(lib, _dims(flags=0)) == EINVAL and 'CLD_KPI' in err() and 'clpf_rollout_mlp_f32' in err()
    assert _call(lib, _dims(n_bldg=17, flags=KPI | abi.CLD_WRITE_DETAIL | abi.CLD_DETAIL_MIN)) == EINVAL and 'n_bldg=17' in err() and 'chunked' in err()
    assert _call(lib, _dims(flags=KPI | abi.CLD_F64_MAPS)) == EINVAL and 'CLD_F64_MAPS' in err()
    assert _call(lib, _dims(flags=KPI | abi.CLD_WRITE_DETAIL)) == EINVAL and 'CLD_WRITE_DETAIL' in err() and 'CLD_DETAIL_MIN' in err()
    assert _call(lib, _dims(flags=KPI | (abi.CLR_EV << abi.CLD_REWARD_SHIFT))) == EINVAL and 'CLR_EV' in err()
    assert _call(lib, _dims(flags=KPI | (9 << abi.CLD_REWARD_SHIFT))) == EINVAL and 'unknown reward kind' in err()
    assert _call(lib, _dims(), n_device_cols=2) == EINVAL and 'device action column' in err() and 'n_device_cols=2' in err()
    assert _call(lib, _dims(env_pitch=128)) == EINVAL and 'env_pitch=128' in err()
    for h in (0, 2, 6, 36, 64, -4):
        assert _call(lib, _dims(), n_hidden=h) == EINVAL and f'n_hidden={h}' in err()
    assert _call(lib, _dims(), n_sets=0) == EINVAL and 'n_sets=0' in err()
    for name in ('pre', 'dep', 'out', 'act_low', 'act_high'):
        assert _call(lib, _dims(), **{name: None}) == ENULL and f'mlp.{name} is NULL' in err()
    assert _call(lib, _dims(), state=False) == ENULL and 'state is NULL' in err()
    for name in ('params', 'ts', 'out_bldg', 'out_env', 'kpi_bldg', 'kpi_env'):
        assert _call(lib, _dims(), null=name) == ENULL and f'{name} is NULL' in err()
    odd = np.zeros(64, dtype=np.float32).ctypes.data + 4
    for name in ('pre', 'dep', 'out', 'net_reset', 'act_low', 'act_high', 'sigma'):
        assert _call(lib, _dims(), **{name: odd}) == EALIGN and f'mlp.{name} is not 16-byte aligned' in err()
    assert _call(lib, _dims(), set_of_block=odd + 1) == EALIGN and 'set_of_block' in err()
    assert _call(lib, _dims(), traj_odd=True) == EALIGN and 'traj' in err()
    assert _call(lib, _dims(), t0=95) == ERANGE and '[95, 103)' in err()
    assert _call(lib, _dims(), t0=-1) == ERANGE and _call(lib, _dims(), k_steps=-1) == ERANGE
    tun = _lib.Tuning(vec=4)
    assert _call(lib, _dims(tuning=ctypes.pointer(tun))) == EINVAL and '4 envs per lane' in err()
    tun = _lib.Tuning(vec=2)                             # one env per lane only: named, not silently narrowed
    for flags in (KPI, KPI | abi.CLD_F64_CHAIN, KPI | (abi.CLR_MARL << abi.CLD_REWARD_SHIFT)):
        assert _call(lib, _dims(flags=flags, tuning=ctypes.pointer(tun))) == EINVAL and '2 envs per lane' in err() and 'one env per lane' in err()
    for nw, n_bldg in ((10, 9), (17, 16), (8, 9), (1, 9)):
        tun = _lib.Tuning(nw=nw)
        assert _call(lib, _dims(n_bldg=n_bldg, tuning=ctypes.pointer(tun))) == EINVAL and f'bad nw {nw}' in err()


def test_kernel_isa(tmp_path_factory):
    """Exactly the four instantiations of cl_rollout_full_policy_kernel<1, PREC, MARL, KPI = true, CHUNK = false> (csrc/cl_policy_full.h: reported as
    `cl_rollout_full_policy_kpi_kernel<PREC, MARL>`) and none of another variant in this unit: at most 128 VGPRs (a 1024-thread workgroup's cap), no scratch
    memory, no static LDS (all dynamic: `_lib.policy_full_kpi_lds_bytes`, the header's formula, within the CU's 160 KiB at nw = 16)."""
    (src,) = _lib.POLICY_FULL_KPI_SOURCES
    kernels, meta = _asm(src, [], tmp_path_factory)
    names = [k for k in kernels if 'cl_rollout_full_policy_kernel' in k]
    by = {tuple(int(x) for x in re.search(r'cl_rollout_full_policy_kernelILi1ELi(\d)ELb(\d)ELb1ELb0EE', k).groups()): k for k in names}
    assert sorted(by) == [(0, 0), (0, 1), (2, 0), (2, 1)] and len(names) == 4
    assert not [k for k in kernels if re.search(r'cl_rollout_full_policy_kernelILi\dELi\dELb\dELb\dELb\dEE', k) and 'ELb1ELb0EE' not in k]     # no plain or CHUNK = true one here
    for key, k in by.items():
        assert meta[k]['private_seg_size'] == 0, (k, meta[k])
        assert meta[k]['num_vgpr'] <= 128, (k, meta[k])
        print(key, meta[k], len([i for i in kernels[k] if not i.startswith('LABEL')]), 'instructions')
    static = re.findall(r'\.group_segment_fixed_size:\s*(\d+)', next(tmp_path_factory.getbasetemp().glob('isa*/' + src.stem + '.s')).read_text())
    assert static and set(static) == {'0'}, static
    # the header's constexpr formula, evaluated from its text
    text = (_lib.CSRC / 'cl_policy_full.h').read_text()
    body = re.search(r'constexpr size_t rollout_full_policy_kpi_lds_floats\(int nw\) \{\s*return (.*?);\s*\}', text, flags=re.S).group(1)
    body = re.sub(r'\(size_t\)', '', body)
    full = abi._strip_comments(_lib.POLICY_FULL_HEADER.read_text())
    nd, na, mh = (int(re.search(rf'#define\s+{n}\s+(\d+)', full).group(1)) for n in ('CLPF_ND', 'CLPF_NA', 'CLPF_MAX_HIDDEN'))
    env = dict(CL_RKPI_S=8, CLKE_PER_COND=abi.CLKE_PER_COND, CL_NKB=abi.CL_NKB, CLPF_ROW=4 * (nd + na) * (mh // 4) + 8 * na)
    assert re.search(r'constexpr int CL_RKPI_S = 8;', (_lib.CSRC / 'cl_rollout.h').read_text())
    for nw in (1, 9, 16):
        assert _lib.policy_full_kpi_lds_bytes(nw) == 4 * eval(body, {}, dict(env, nw=nw)), nw
    assert _lib.policy_full_kpi_lds_bytes(9) == 82176 and _lib.policy_full_kpi_lds_bytes(16) == 141312 <= 160 * 1024


def test_the_thermal_policy_library_is_what_it_was():
    _lib.build_policy_full()
    assert exports(_lib.POLICY_FULL_LIB_PATH) == ['clpf_abi_version', 'clpf_core_abi_version', 'clpf_last_error', 'clpf_rollout_mlp_f32'] == _lib.POLICY_FULL_SYMBOLS
    full = ctypes.CDLL(str(_lib.POLICY_FULL_LIB_PATH))
    full.clpf_last_error.restype = ctypes.c_char_p
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    full.clpf_rollout_mlp_f32.argtypes = [ctypes.POINTER(_lib.Dims), vp, vp, vp, ctypes.POINTER(_lib.PolicyFullMLP), vp, vp, vp, vp, i32, i32, vp]
    assert full.clpf_abi_version() == 1
    p = np.zeros(64, dtype=np.float32).ctypes.data
    mlp = _lib.PolicyFullMLP(n_hidden=16, n_sets=1, pre=p, dep=p, out=p, act_low=p, act_high=p, seed=1)
    rc = full.clpf_rollout_mlp_f32(ctypes.byref(_dims(flags=KPI)), p, p, p, ctypes.byref(mlp), p, p, None, None, 0, 8, None)
    assert rc == abi.CL_EINVAL and 'CLD_KPI' in full.clpf_last_error().decode()
