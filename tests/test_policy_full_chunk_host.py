"""The building-chunked closed-loop policy rollout of thermal districts (`clpfc_rollout_mlp_f32`, kernel `cl_rollout_full_policy_chunk_kernel`:
csrc/cl_policy_full.h at CHUNK = true, library ``libcitylearn_amd_policy_full_chunk.so``) as far as it can be checked without a GPU: the library's symbol list,
the argument validation (before any HIP call), registers / scratch / LDS of every instantiation, and the conditioning of the closed loop on the
districts of more than 16 buildings the GPU tests run (tests/test_gpu_policy_full_chunk_rollout.py)."""
import ctypes
import re

import numpy as np
import pytest

from citylearn_amd import _lib, abi, policy
from policy_full_chunk_util import CONDITIONED, DEFAULT_B_CHUNK, chunk_district, default_chunks
from policy_util import exports
from test_isa_guards import _asm
from test_policy_full_host import _conditioning


@pytest.fixture(scope='module')
def lib():
    _lib.build_policy_full_chunk()
    lib = ctypes.CDLL(str(_lib.POLICY_FULL_CHUNK_LIB_PATH))
    lib.clpfc_last_error.restype = ctypes.c_char_p
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.clpfc_rollout_mlp_f32.argtypes = [ctypes.POINTER(_lib.Dims), vp, vp, vp, ctypes.POINTER(_lib.PolicyFullMLP), vp, vp, vp, vp, i32, i32, vp]
    return lib


# ---- 1. the library -------------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header(lib):
    assert _lib.POLICY_FULL_CHUNK_SYMBOLS == ['clpfc_abi_version', 'clpfc_core_abi_version', 'clpfc_last_error', 'clpfc_rollout_mlp_f32']
    assert exports(_lib.POLICY_FULL_CHUNK_LIB_PATH) == _lib.POLICY_FULL_CHUNK_SYMBOLS
    assert lib.clpfc_abi_version() == _lib.POLICY_FULL_CHUNK_ABI_VERSION == 1 and lib.clpfc_core_abi_version() == abi.CL_ABI_VERSION
    # the one-row library keeps its four symbols and its version; `clpf_mlp` is shared, not redefined
    assert _lib.POLICY_FULL_SYMBOLS == ['clpf_abi_version', 'clpf_core_abi_version', 'clpf_last_error', 'clpf_rollout_mlp_f32'] and _lib.POLICY_FULL_ABI_VERSION == 1
    assert 'typedef struct' not in abi._strip_comments(_lib.POLICY_FULL_CHUNK_HEADER.read_text())
    assert _lib.POLICY_FULL_CHUNK.mlp is _lib.PolicyFullMLP and _lib.POLICY_FULL_CHUNK.n_kpi == 0


def test_the_extension_tuples():
    assert _lib.EXTENSIONS == (_lib.POLICY, _lib.POLICY_KPI, _lib.POLICY_FULL, _lib.POLICY_FULL_KPI) and len(_lib.EXTENSIONS) == 4
    assert _lib.ALL_EXTENSIONS == _lib.EXTENSIONS + (_lib.POLICY_FULL_CHUNK,) and len(_lib.ALL_EXTENSIONS) == 5
    assert len({e.path for e in _lib.ALL_EXTENSIONS}) == 5 and len({e.prefix for e in _lib.ALL_EXTENSIONS}) == 5
    assert policy.StorageMLPPolicy.kind.ext_chunk is _lib.POLICY_FULL_CHUNK and policy.MLPPolicy.kind.ext_chunk is None
    assert policy.StorageMLPPolicy.kind.ext is _lib.POLICY_FULL and policy.StoragePolicyTables.kind is policy.StorageMLPPolicy.kind
    import inspect
    import __graft_entry__
    assert '_lib.ALL_EXTENSIONS' in inspect.getsource(__graft_entry__.build)


def test_default_geometry():
    """Balanced chunks of at most eight: n_chunks = ceil(n_bldg / 8), b_chunk = ceil(n_bldg / n_chunks)."""
    assert default_chunks(17) == (6, 3) and default_chunks(33) == (7, 5) and default_chunks(1024) == (8, 128) and default_chunks(24) == (8, 3)
    assert all(default_chunks(n)[0] == b for n, b in DEFAULT_B_CHUNK.items())
    for n in range(17, 200):
        b, nc = default_chunks(n)
        assert b <= 8 and (nc - 1) * b < n <= nc * b and nc * 5 < n             # every chunk has a building; the reserved plane has room


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------------
def _dims(n_env=64, n_bldg=17, flags=0, **kw):
    d = _lib.Dims(n_env, n_bldg, 100, 45, flags)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(lib, d, *, t0=0, k_steps=8, state=True, traj_odd=False, null=None, **mlp_kw):
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data
    a = {k: (None if k == null else p) for k in ('params', 'ts', 'out_bldg', 'out_env')}
    m = dict(n_hidden=16, n_sets=1, n_device_cols=0, reserved=0, pre=p, dep=p, out=p, set_of_block=None, net_reset=None, act_low=p, act_high=p, sigma=None, seed=1)
    m.update(mlp_kw)
    mlp = _lib.PolicyFullMLP(**m)
    return lib.clpfc_rollout_mlp_f32(ctypes.byref(d) if d is not None else None, a['params'], a['ts'], p if state else None, ctypes.byref(mlp),
                                     a['out_bldg'], a['out_env'], None,
                                     p + 4 if traj_odd else None, t0, k_steps, None)


def test_refusals_name_their_cause_before_any_hip_call(lib):
    """Every refusal returns its code with a message that names the cause; the buffers are 256 bytes of host memory, so a call that got as far as a
    launch would not come back with one of these codes."""
    err = lambda: lib.clpfc_last_error().decode()
    EINVAL, ENULL, EALIGN, ERANGE = abi.CL_EINVAL, abi.CL_ENULL, abi.CL_EALIGN, abi.CL_ERANGE
    tuned = lambda **kw: ctypes.pointer(_lib.Tuning(**kw))
    assert _call(lib, None) == ENULL and 'dims is NULL' in err()
    assert _call(lib, _dims(n_env=6)) == EALIGN and 'multiple of 4' in err()
    assert _call(lib, _dims(flags=abi.CLD_LEAN)) == EINVAL and 'CLD_LEAN' in err() and 'clpol_rollout_mlp_f32' in err()
    assert _call(lib, _dims(flags=abi.CLR_MARL << abi.CLD_REWARD_SHIFT)) == EINVAL and 'CLR_MARL' in err() \
        and 'a building-chunked launch cannot couple the buildings inside a step' in err()
    assert _call(lib, _dims(flags=abi.CLR_EV << abi.CLD_REWARD_SHIFT)) == EINVAL and 'CLR_EV' in err()
    assert _call(lib, _dims(flags=9 << abi.CLD_REWARD_SHIFT)) == EINVAL and 'unknown reward kind' in err()
    assert _call(lib, _dims(flags=abi.CLD_F64_MAPS)) == EINVAL and 'CLD_F64_MAPS' in err()
    assert _call(lib, _dims(flags=abi.CLD_KPI)) == EINVAL and 'CLD_KPI' in err()
    assert _call(lib, _dims(flags=abi.CLD_WRITE_DETAIL)) == EINVAL and 'CLD_WRITE_DETAIL' in err()
    assert _call(lib, _dims(env_pitch=128)) == EINVAL and 'env_pitch=128' in err()
    assert _call(lib, _dims(), n_device_cols=2) == EINVAL and 'device action column' in err() and 'n_device_cols=2' in err()
    assert _call(lib, _dims(), reserved=1) == EINVAL and 'reserved must be 0' in err()
    assert _call(lib, _dims(n_act_cols=65537)) == EINVAL and 'n_act_cols=65537' in err()
    for h in (0, 2, 6, 36, 64, -4):
        assert _call(lib, _dims(), n_hidden=h) == EINVAL and f'n_hidden={h}' in err()
    assert _call(lib, _dims(), n_sets=0) == EINVAL and 'n_sets=0' in err()
    # the buffer codes of check_policy_buffers
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
    assert _call(lib, _dims(n_bldg=40, tuning=tuned(b_chunk=20))) == EINVAL and 'b_chunk=20' in err() and 'at most 16' in err()
    # one workgroup row is the other kernel: named
    assert _call(lib, _dims(n_bldg=9)) == EINVAL and 'n_bldg=9' in err() and 'clpf_rollout_mlp_f32' in err()
    assert _call(lib, _dims(n_bldg=16)) == EINVAL and 'n_bldg=16' in err() and 'clpf_rollout_mlp_f32' in err()
    assert _call(lib, _dims(n_bldg=9, tuning=tuned(b_chunk=9))) == EINVAL and 'b_chunk=9 >= n_bldg=9' in err() and 'clpf_rollout_mlp_f32' in err()
    assert _call(lib, _dims(n_bldg=12, tuning=tuned(b_chunk=16))) == EINVAL and 'b_chunk=16 >= n_bldg=12' in err() and 'clpf_rollout_mlp_f32' in err()
    # 17 buildings in chunks of 5: four chunks need 4 x 5 = 20 rows of the reserved plane's 17 -- no room
    assert _call(lib, _dims(tuning=tuned(b_chunk=5))) == EINVAL and 'b_chunk=5 leaves no room for the 4 chunk partial sums' in err()
    assert _call(lib, _dims(n_bldg=6, tuning=tuned(b_chunk=3))) == EINVAL and 'leaves no room' in err()
    # nw is b_chunk and nothing else
    assert _call(lib, _dims(tuning=tuned(nw=8))) == EINVAL and 'bad nw 8' in err() and 'b_chunk = 6' in err()
    assert _call(lib, _dims(tuning=tuned(b_chunk=8, nw=16))) == EINVAL and 'bad nw 16' in err() and 'b_chunk = 8' in err()
    # envs per lane
    assert _call(lib, _dims(tuning=tuned(vec=4))) == EINVAL and '4 envs per lane' in err()
    assert _call(lib, _dims(flags=abi.CLD_F64_CHAIN, tuning=tuned(vec=2))) == EINVAL and 'CLD_F64_CHAIN' in err() and 'one env per lane' in err()


# ---- 3. generated code ----------------------------------------------------------------------------------------------------------------
def test_kernel_isa(tmp_path_factory):
    """Exactly the three instantiations of cl_rollout_full_policy_kernel<VEC, PREC, false, KPI = false, CHUNK = true> (csrc/cl_policy_full.h: reported
    as `cl_rollout_full_policy_chunk_kernel<VEC, PREC>`; no MARL: no barrier inside the K loop) and no instantiation of the one-row or a KPI variant in this unit; at most 128 VGPRs (a 1024-thread workgroup's cap), no scratch memory, no static LDS in the
    rollout kernel (it is all dynamic: `_lib.policy_full_chunk_lds_bytes`); cl_finish_kernel, the fold, is in the unit with its [16][64] floats."""
    (src,) = _lib.POLICY_FULL_CHUNK_SOURCES
    kernels, meta = _asm(src, [], tmp_path_factory)
    names = [k for k in kernels if 'cl_rollout_full_policy_kernel' in k]
    by = {tuple(int(x) for x in re.search(r'cl_rollout_full_policy_kernelILi(\d)ELi(\d)ELb0ELb0ELb1EE', k).groups()): k for k in names}
    assert sorted(by) == [(1, 0), (1, 2), (2, 0)] and len(names) == 3
    assert not [k for k in kernels if (re.search(r'cl_rollout_full_policy_kernelILi\dELi\dELb\dELb\dELb\dEE', k) and 'ELb0ELb0ELb1EE' not in k) or 'cl_rollout_full_kernel' in k]
    assert len([k for k in kernels if 'cl_finish_kernel' in k]) == 1
    for key, k in by.items():
        assert meta[k]['private_seg_size'] == 0, (k, meta[k])
        assert meta[k]['num_vgpr'] <= 128, (k, meta[k])
        print(key, meta[k])
    text = next(tmp_path_factory.getbasetemp().glob('isa*/' + src.stem + '.s')).read_text()
    sizes = re.findall(r'\.group_segment_fixed_size:\s*(\d+)', text)
    assert sorted(set(sizes)) == ['0', '4096'] and sizes.count('4096') == 1, sizes          # (cl_finish_kernel's part[16][64])
    # the header's formula: rollout_full_policy_chunk_lds_floats(nw, tile) = nw NQ tile + nw CLPF_ROW, CLPF_ROW = 4 (5 + 4) (32 / 4) + 8 x 4
    head = (_lib.CSRC / 'cl_policy_full.h').read_text()
    assert re.search(r'rollout_full_policy_chunk_lds_floats\(int nw, int tile\) \{ return \(size_t\)nw \* NQ \* tile \+ \(size_t\)nw \* CLPF_ROW; \}', head)
    row = 4 * (policy.CLPF_ND + policy.CLPF_NA) * (policy.CLPF_MAX_HIDDEN // 4) + 8 * policy.CLPF_NA
    for nw in (1, 5, 6, 7, 8, 16):
        for vec in (1, 2):
            assert _lib.policy_full_chunk_lds_bytes(nw, vec) == 4 * (nw * abi.CL_NQ * 64 * vec + nw * row) == _lib.policy_full_lds_bytes(nw, vec)
    assert _lib.policy_full_chunk_lds_bytes(8, 2) == 26624 and _lib.policy_full_chunk_lds_bytes(16, 2) == 53248 <= 160 * 1024


# ---- 4. conditioning ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,H', CONDITIONED)
def test_closed_loop_is_well_conditioned(name, H):
    """tests/test_policy_full_host.py::test_closed_loop_is_well_conditioned's condition, 0.1 x (1e-4 + 1e-4 |ref|) on soc, cs, ds and net, on the
    districts of more than 16 buildings (the table in tests/policy_full_chunk_util.py; 't17_outage' at H = 4 reads 0.138 and is not used)."""
    err, tol, ref, pt = _conditioning(chunk_district(name), H)
    assert 0 < tol < 1e-5, tol
    act = ref['action'].transpose(0, 2, 3, 1)[:, pt.cols >= 0]
    assert np.abs(act).max() > 0.01 and np.ptp(act) > 0.02                                # a policy that does something
    assert set((pt.cols >= 0).sum(axis=1)) <= {2, 3}                                      # every building has 2 or 3 heads
    for k in err:
        print(f'{name} H={H} {k}: worst {err[k]:.4f} x (1e-4 + 1e-4 |ref|), action tolerance {tol:.3e}')
        assert err[k] < 0.1, (k, err[k])
