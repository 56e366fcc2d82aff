"""The closed-loop policy rollout that keeps the streaming KPIs (`clpk_rollout_mlp_kpi_f32`, kernel `cl_rollout_policy_kernel<VEC, PREC, KPI = true, CHUNK = false>`
of csrc/cl_policy.h, reported as `cl_rollout_policy_kpi_kernel<VEC, PREC>`; library ``libcitylearn_amd_policy_kpi.so``) as far as it can be
checked without a GPU: the three libraries' symbol lists, the
argument validation (before any HIP call), the generated gfx950 code of every instantiation the host can select, and the LDS formula."""
import ctypes
import re

import numpy as np
import pytest

from citylearn_amd import _lib, abi
from test_isa_guards import _asm, _count
from policy_util import exports
from test_policy_host import _dims

KPI = abi.CLD_LEAN | abi.CLD_KPI


@pytest.fixture(scope='module')
def lib():
    _lib.build_policy_kpi()
    lib = ctypes.CDLL(str(_lib.POLICY_KPI_LIB_PATH))
    lib.clpk_last_error.restype = ctypes.c_char_p
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.clpk_rollout_mlp_kpi_f32.argtypes = [ctypes.POINTER(_lib.Dims), vp, vp, vp, ctypes.POINTER(_lib.PolicyMLP), vp, vp, vp, vp, vp, vp, i32, i32, vp]
    return lib


# ---- 1. the libraries -----------------------------------------------------------------------------------------------------------------
def test_three_libraries_export_exactly_their_headers(lib):
    assert _lib.POLICY_KPI_SYMBOLS == ['clpk_abi_version', 'clpk_core_abi_version', 'clpk_last_error', 'clpk_rollout_mlp_kpi_f32']
    assert exports(_lib.POLICY_KPI_LIB_PATH) == _lib.POLICY_KPI_SYMBOLS
    assert lib.clpk_abi_version() == _lib.POLICY_KPI_ABI_VERSION == 1 and lib.clpk_core_abi_version() == abi.CL_ABI_VERSION
    # the policy library and the main library are what they were
    _lib.build_policy()
    assert exports(_lib.POLICY_LIB_PATH) == _lib.POLICY_SYMBOLS == ['clpol_abi_version', 'clpol_core_abi_version', 'clpol_last_error', 'clpol_rollout_mlp_f32']
    assert _lib.POLICY_ABI_VERSION == 1
    _lib.build()
    main = exports(_lib.LIB_PATH)
    assert main == abi.EXPORTED_SYMBOLS and len(main) == 15 and not [s for s in main if s.startswith(('clpol_', 'clpk_'))]
    assert not [k for k in abi.CONSTANTS if k.startswith(('CLPOL', 'CLPK'))]


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------------
def _call(lib, d, *, t0=0, k_steps=8, state=True, traj_odd=False, kpi_bldg='ok', kpi_env='ok', **mlp_kw):
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data
    m = dict(n_hidden=16, n_sets=1, flags=0, reserved=0, pre=p, dep=p, out=p, set_of_block=None, net_reset=None, act_low=p, act_high=p, sigma=None, seed=1)
    m.update(mlp_kw)
    mlp = _lib.PolicyMLP(**m)
    plane = {'ok': p, 'odd': p + 4, None: None}
    return lib.clpk_rollout_mlp_kpi_f32(ctypes.byref(d) if d is not None else None, p, p, p if state else None, ctypes.byref(mlp), p, p, None,
                                        p + 4 if traj_odd else None, plane[kpi_bldg], plane[kpi_env], t0, k_steps, None)


def test_refusals_name_their_cause_before_any_hip_call(lib):
    """No device here: every one of these returns before the first HIP call, or the call would fail with a HIP error instead."""
    err = lambda: lib.clpk_last_error().decode()
    EINVAL, ENULL, EALIGN, ERANGE = abi.CL_EINVAL, abi.CL_ENULL, abi.CL_EALIGN, abi.CL_ERANGE
    kd = lambda **kw: _dims(**{'flags': KPI, **kw})
    assert _call(lib, None) == ENULL and 'dims is NULL' in err()
    assert _call(lib, kd(n_env=6)) == EALIGN and 'multiple of 4' in err()
    # CLD_KPI is required -- with and without it the rest of clpol_rollout_mlp_f32's list
    assert _call(lib, _dims()) == EINVAL and 'CLD_KPI' in err() and 'clpol_rollout_mlp_f32' in err()
    assert _call(lib, kd(flags=abi.CLD_KPI)) == EINVAL and 'CLD_LEAN' in err() and 'thermal' in err()
    assert _call(lib, kd(n_bldg=33)) == EINVAL and 'n_bldg=33' in err() and 'chunked' in err()
    assert _call(lib, kd(flags=KPI | abi.CLD_F64_MAPS)) == EINVAL and 'CLD_F64_MAPS' in err()
    assert _call(lib, kd(flags=KPI | abi.CLD_WRITE_DETAIL)) == EINVAL and 'CLD_WRITE_DETAIL' in err()
    assert _call(lib, kd(flags=KPI | (abi.CLR_EV << abi.CLD_REWARD_SHIFT))) == EINVAL and 'CLR_EV' in err()
    assert _call(lib, kd(flags=KPI | (9 << abi.CLD_REWARD_SHIFT))) == EINVAL and 'unknown reward kind' in err()
    assert _call(lib, kd(env_pitch=128)) == EINVAL and 'env_pitch=128' in err()
    for h in (0, 2, 6, 36, 64, -4):
        assert _call(lib, kd(), n_hidden=h) == EINVAL and f'n_hidden={h}' in err()
    assert _call(lib, kd(), n_sets=0) == EINVAL and 'n_sets=0' in err()
    for name in ('pre', 'dep', 'out', 'act_low', 'act_high'):
        assert _call(lib, kd(), **{name: None}) == ENULL and f'mlp.{name} is NULL' in err()
    assert _call(lib, kd(), state=False) == ENULL and 'state is NULL' in err()
    odd = np.zeros(64, dtype=np.float32).ctypes.data + 4
    for name in ('pre', 'dep', 'out', 'net_reset', 'sigma'):
        assert _call(lib, kd(), **{name: odd}) == EALIGN and f'mlp.{name} is not 16-byte aligned' in err()
    assert _call(lib, kd(), set_of_block=odd + 1) == EALIGN and 'set_of_block' in err()
    assert _call(lib, kd(), traj_odd=True) == EALIGN and 'traj' in err()
    # the KPI planes: required and aligned
    for name in ('kpi_bldg', 'kpi_env'):
        assert _call(lib, kd(), **{name: None}) == ENULL and f'{name} is NULL' in err()
        assert _call(lib, kd(), **{name: 'odd'}) == EALIGN and f'{name} is not 16-byte aligned' in err()
    assert _call(lib, kd(), t0=95) == ERANGE and '[95, 103)' in err()
    assert _call(lib, kd(), t0=-1) == ERANGE and _call(lib, kd(), k_steps=-1) == ERANGE
    tun = _lib.Tuning(vec=4)
    assert _call(lib, kd(tuning=ctypes.pointer(tun))) == EINVAL and '4 envs per lane' in err()
    tun = _lib.Tuning(nw=8)                              # 17 buildings: 8 waves x 2 buildings < 17
    assert _call(lib, kd(tuning=ctypes.pointer(tun))) == EINVAL and 'bad nw 8' in err()
    assert _call(lib, kd(n_bldg=5, tuning=ctypes.pointer(tun))) == EINVAL and 'bad nw 8' in err()       # more waves than buildings
    tun = _lib.Tuning(nw=2)
    assert _call(lib, kd(n_bldg=1, tuning=ctypes.pointer(tun))) == EINVAL and 'bad nw 2' in err()
    tun = _lib.Tuning(nw=17)
    assert _call(lib, kd(n_bldg=32, tuning=ctypes.pointer(tun))) == EINVAL and 'bad nw 17' in err()


# ---- 3. generated code ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def unit(tmp_path_factory):
    (src, flags), = _lib.POLICY_KPI_SOURCES
    assert flags == ['-fno-slp-vectorize'] and src.name == 'cl_policy_kpi.hip'
    return _asm(src, flags, tmp_path_factory)


def test_policy_kpi_kernel_isa(unit):
    """The host can select all four instantiations <1 | 2 envs per lane, PREC 0 | 2> (csrc/cl_policy_kpi.hip's launcher): each without scratch,
    within a 1024-thread workgroup's 128 registers, without buffer instructions or packed fp32, the float64 chain exactly under PREC = 2, the
    hidden activation as v_exp_f32 / v_rcp_f32, `pre` through s_load_dwordx4 and the staged `dep` / `out` rows through broadcast ds_read_b128
    (three per building and group of four hidden units, the loop not unrolled: six; three more behind the loop, where the head workgroup's
    last thread reads the baseline series' twelve contiguous accumulators back from LDS: nine).  The unit holds no other rollout or step
    kernel: beside the four, only cl_flex_reset_kernel, which cl_kernels.hip's helper cut carries into every unit that includes it (the policy
    unit too) -- and no other instantiation of its own kernel template (KPI = false, or CHUNK = true)."""
    kernels, meta = unit
    launcher = (_lib.CSRC / 'cl_policy_kpi.hip').read_text()
    selectable = sorted((int(v), int(p)) for v, p in re.findall(r'case \d+: CL_POL\((\d), (\d)\); break;', launcher))
    assert selectable == [(1, 0), (1, 2), (2, 0), (2, 2)]
    names = [k for k in meta if 'private_seg_size' in meta[k]]
    mine = [k for k in names if 'cl_rollout_policy_kernel' in k]
    by = {tuple(int(x) for x in re.search(r'cl_rollout_policy_kernelILi(\d)ELi(\d)ELb1ELb0EE', k).groups()): k for k in mine}
    assert sorted(by) == selectable and len(mine) == 4
    assert [k for k in names if k not in mine and 'cl_flex_reset_kernel' not in k] == []
    assert not [k for k in kernels if re.search(r'cl_rollout_kernel|cl_rollout_kpi_kernel|cl_rollout_policy_kernelILi\dELi\dELb(0ELb\d|1ELb1)EE|cl_step', k)]
    for (vec, prec), k in by.items():
        ins = kernels[k]
        print(f'cl_rollout_policy_kpi_kernel<{vec}, {prec}>: {meta[k]["num_vgpr"]} VGPRs, {meta[k]["private_seg_size"]} bytes of scratch')
        assert meta[k]['private_seg_size'] == 0, k
        assert meta[k]['num_vgpr'] <= 128, (k, meta[k])
        assert not [i for i in ins if i.startswith(('scratch_', 'buffer_'))], k
        assert not [i for i in ins if re.match(r'v_pk_\w+_f32', i)], k
        assert any(i.startswith('v_fma_f64') for i in ins) == (prec == 2), k
        assert _count(ins, 'v_exp_f32') >= 2 * vec and _count(ins, 'v_rcp_f32') >= 2 * vec, k
        assert _count(ins, 'ds_read_b128') == 9 and _count(ins, 's_load_dwordx4') >= 2, (k, _count(ins, 'ds_read_b128'))


# ---- 4. the LDS formula ---------------------------------------------------------------------------------------------------------------
def _header_lds_floats(nw, tile):
    """`rollout_policy_kpi_lds_floats` / `rollout_kpi_lds_floats` / CLPOL_ROW evaluated from the headers' own text."""
    rollout, pol = ((_lib.CSRC / n).read_text() for n in ('cl_rollout.h', 'cl_policy.h'))
    const = {k: int(v) for src in (rollout, pol) for k, v in re.findall(r'constexpr int (\w+) = (\d+);', src)}
    const['CLPOL_ROW'] = eval(re.search(r'constexpr int CLPOL_ROW = ([^;]+);', pol).group(1), {}, const)
    const['CLKE_PER_COND'] = abi.CLKE_PER_COND
    kpi = re.search(r'constexpr size_t rollout_kpi_lds_floats\(int nw, int tile\) \{\s*return ([^;]+);', rollout).group(1)
    mine = re.search(r'constexpr size_t rollout_policy_kpi_lds_floats\(int nw, int tile\) \{ return ([^;]+); \}', pol).group(1)
    strip = lambda e: e.replace('(size_t)', '')
    env = dict(const, nw=nw, tile=tile)
    env['rollout_kpi_lds_floats'] = lambda nw_, tile_: eval(strip(kpi), {}, dict(const, nw=nw_, tile=tile_))
    return eval(strip(mine), {}, env)


def test_lds_formula():
    for vec in (1, 2):
        for nw in range(1, 17):
            assert _lib.policy_kpi_lds_bytes(nw, vec) == 4 * _header_lds_floats(nw, 64 * vec), (nw, vec)
    # the figures the documents quote: 17 buildings (nw = 9) and the largest geometry, two envs per lane
    assert _lib.policy_kpi_lds_bytes(9, 2) == 55296 and _lib.policy_kpi_lds_bytes(16, 2) == 89792 < 160 * 1024
    # 4 (8 nw tile + 12 tile + 1200 + 208 nw) > 65 536: at two envs per lane 4928 nw > 54 592, i.e. from nw = 12; at one env per lane
    # 2880 nw > 57 664, i.e. never (nw <= 16)
    over = lambda vec: [nw for nw in range(1, 17) if _lib.policy_kpi_lds_bytes(nw, vec) > 64 * 1024]
    assert over(2) == list(range(12, 17)) and over(1) == []
    # the launcher opts in above 64 KiB and the entry point refuses above the CU's LDS: both through cl_policy_common.h's one copy
    shared, unit = (_lib.CSRC / 'cl_policy_common.h').read_text(), (_lib.CSRC / 'cl_policy_kpi.hip').read_text()
    assert 'if (lds > 64 * 1024) if (hipError_t e = ensure_dynamic_lds(' in shared and 'if (lds > CL_LDS_PER_CU) return fail(' in shared
    assert 'CL_POLICY_LAUNCH(cl_rollout_policy_kernel<V, P, true, false>)' in unit and 'check_policy_lds(lds, "policy KPI", nw, vec)' in unit
