"""The building-chunked closed-loop policy rollout of battery + PV districts (`clpc_rollout_mlp_f32`, kernel `cl_rollout_policy_chunk_kernel` in
csrc/cl_policy_chunk.h, library ``libcitylearn_amd_policy_chunk.so``) as far as it can be checked without a GPU: the library's symbol list, the
default geometry, the argument validation (before any HIP call), registers / scratch / LDS and the table reads of every instantiation, and the
conditioning of the closed loop on the districts of more than 32 buildings the GPU tests run free (tests/test_gpu_policy_chunk_rollout.py)."""
import ctypes
import re

import numpy as np
import pytest

from citylearn_amd import _lib, abi, policy
from policy_chunk_util import CONDITIONED, HET40_UNDRIVEN, chunk_district, default_chunks
from policy_util import exports
from test_isa_guards import _asm, _count
from test_policy_host import _conditioning


@pytest.fixture(scope='module')
def lib():
    _lib.build_policy_chunk()
    lib = ctypes.CDLL(str(_lib.POLICY_CHUNK_LIB_PATH))
    lib.clpc_last_error.restype = ctypes.c_char_p
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.clpc_rollout_mlp_f32.argtypes = [ctypes.POINTER(_lib.Dims), vp, vp, vp, ctypes.POINTER(_lib.PolicyMLP), vp, vp, vp, vp, i32, i32, vp]
    return lib


# ---- 1. the library -------------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header(lib):
    assert _lib.POLICY_CHUNK_SYMBOLS == ['clpc_abi_version', 'clpc_core_abi_version', 'clpc_last_error', 'clpc_rollout_mlp_f32']
    assert exports(_lib.POLICY_CHUNK_LIB_PATH) == _lib.POLICY_CHUNK_SYMBOLS
    assert lib.clpc_abi_version() == _lib.POLICY_CHUNK_ABI_VERSION == 1 and lib.clpc_core_abi_version() == abi.CL_ABI_VERSION
    # the one-row library keeps its four symbols and its version; `clpol_mlp` is shared, not redefined
    assert _lib.POLICY_SYMBOLS == ['clpol_abi_version', 'clpol_core_abi_version', 'clpol_last_error', 'clpol_rollout_mlp_f32'] and _lib.POLICY_ABI_VERSION == 1
    text = abi._strip_comments(_lib.POLICY_CHUNK_HEADER.read_text())
    assert 'typedef struct' not in text and '#include "citylearn_amd_policy.h"' in text
    assert _lib.POLICY_CHUNK.mlp is _lib.PolicyMLP and _lib.POLICY_CHUNK.n_kpi == 0 and _lib.POLICY_CHUNK.entry == 'rollout_mlp_f32'
    (src, flags), = _lib.POLICY_CHUNK_SOURCES
    assert flags == ['-fno-slp-vectorize'] and src.name == 'cl_policy_chunk.hip'
    unit = src.read_text()
    assert all(re.search(rf'^#define {d}$', unit, flags=re.M) for d in ('CL_TU_NOSLP', 'CL_TU_POLICY', 'CL_TU_FINISH'))


def test_the_extension_tuples():
    """The new tuple beside the pinned ones; `MLPPolicy.kind` gets two new fields and keeps `ext_chunk` / `ext_chunk_kpi` None."""
    assert _lib.LEAN_CHUNK_EXTENSIONS == (_lib.POLICY_CHUNK,)
    assert _lib.EXTENSIONS == (_lib.POLICY, _lib.POLICY_KPI, _lib.POLICY_FULL, _lib.POLICY_FULL_KPI)
    assert _lib.ALL_EXTENSIONS == _lib.EXTENSIONS + (_lib.POLICY_FULL_CHUNK,) and len(_lib.ALL_EXTENSIONS) == 5
    assert _lib.CHUNK_KPI_EXTENSIONS == (_lib.POLICY_FULL_CHUNK_KPI,)
    every = _lib.ALL_EXTENSIONS + _lib.CHUNK_KPI_EXTENSIONS + _lib.LEAN_CHUNK_EXTENSIONS
    assert len({e.path for e in every}) == 7 and len({e.prefix for e in every}) == 7
    lean, thermal = policy.MLPPolicy.kind, policy.StorageMLPPolicy.kind
    assert lean.ext_chunk is None and lean.ext_chunk_kpi is None and lean.ext_chunk_pair is _lib.POLICY_CHUNK and lean.one_row_max == 32
    assert thermal.ext_chunk is _lib.POLICY_FULL_CHUNK and thermal.ext_chunk_pair is None and thermal.one_row_max == 16
    assert policy.PolicyTables.kind is lean
    import inspect
    import __graft_entry__
    assert '_lib.ALL_EXTENSIONS + _lib.CHUNK_KPI_EXTENSIONS + _lib.LEAN_CHUNK_EXTENSIONS' in inspect.getsource(__graft_entry__.build)


def test_default_geometry():
    """The blind chunked lean rollout's 32-building workgroups, balanced: n_chunks = ceil(n_bldg / 32), b_chunk = ceil(n_bldg / n_chunks),
    nw = ceil(b_chunk / 2)."""
    assert default_chunks(33) == (17, 2, 9) and default_chunks(40) == (20, 2, 10) and default_chunks(64) == (32, 2, 16) and default_chunks(1024) == (32, 32, 16)
    for n in range(33, 201):
        b, nc, nw = default_chunks(n)
        assert b <= 32 and (nc - 1) * b < n <= nc * b                              # every chunk has a building
        assert nw <= 16 and 2 * nw >= b and nw <= b
        for n_env in (4, 64, 260):                                                 # the reserved plane has room (the library's inequality)
            assert nc * (abi.CL_NQ + 1) * n_env + (n_env + 63) // 64 + 4 <= n * n_env


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------------
def _dims(n_env=64, n_bldg=40, flags=abi.CLD_LEAN, **kw):
    d = _lib.Dims(n_env, n_bldg, 100, n_bldg, flags)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(lib, d, *, t0=0, k_steps=8, state=True, traj_odd=False, null=None, **mlp_kw):
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data
    a = {k: (None if k == null else p) for k in ('params', 'ts', 'out_bldg', 'out_env')}
    m = dict(n_hidden=16, n_sets=1, flags=0, reserved=0, pre=p, dep=p, out=p, set_of_block=None, net_reset=None, act_low=p, act_high=p, sigma=None, seed=1)
    m.update(mlp_kw)
    mlp = _lib.PolicyMLP(**m)
    return lib.clpc_rollout_mlp_f32(ctypes.byref(d) if d is not None else None, a['params'], a['ts'], p if state else None, ctypes.byref(mlp),
                                    a['out_bldg'], a['out_env'], None, p + 4 if traj_odd else None, t0, k_steps, None)


def test_refusals_name_their_cause_before_any_hip_call(lib):
    """Every refusal returns its code with a message that names the cause; the buffers are 256 bytes of host memory, so a call that got as far as a
    launch would not come back with one of these codes."""
    err = lambda: lib.clpc_last_error().decode()
    EINVAL, ENULL, EALIGN, ERANGE = abi.CL_EINVAL, abi.CL_ENULL, abi.CL_EALIGN, abi.CL_ERANGE
    LEAN = abi.CLD_LEAN
    tuned = lambda **kw: ctypes.pointer(_lib.Tuning(**kw))
    assert _call(lib, None) == ENULL and 'dims is NULL' in err()
    assert _call(lib, _dims(n_env=6)) == EALIGN and 'multiple of 4' in err()
    assert _call(lib, _dims(flags=0)) == EINVAL and 'CLD_LEAN' in err() and 'clpfc_rollout_mlp_f32' in err() and err().startswith('clpc_rollout_mlp_f32')
    assert _call(lib, _dims(flags=LEAN | (abi.CLR_MARL << abi.CLD_REWARD_SHIFT))) == EINVAL and 'CLR_MARL' in err() \
        and 'a building-chunked launch cannot couple the buildings inside a step' in err() and 'clpc_rollout_mlp_f32' in err()
    assert _call(lib, _dims(flags=LEAN | (abi.CLR_EV << abi.CLD_REWARD_SHIFT))) == EINVAL and 'CLR_EV' in err() and 'clpc_rollout_mlp_f32' in err()
    assert _call(lib, _dims(flags=LEAN | (9 << abi.CLD_REWARD_SHIFT))) == EINVAL and 'unknown reward kind' in err()
    assert _call(lib, _dims(flags=LEAN | abi.CLD_F64_MAPS)) == EINVAL and 'CLD_F64_MAPS' in err() and 'clpc_rollout_mlp_f32' in err()
    assert _call(lib, _dims(flags=LEAN | abi.CLD_KPI)) == EINVAL and 'CLD_KPI' in err() and 'clpc_rollout_mlp_f32' in err()
    assert _call(lib, _dims(flags=LEAN | abi.CLD_WRITE_DETAIL)) == EINVAL and 'CLD_WRITE_DETAIL' in err() and 'clpc_rollout_mlp_f32' in err()
    assert _call(lib, _dims(env_pitch=128)) == EINVAL and 'env_pitch=128' in err() and 'clpc_rollout_mlp_f32' in err()
    # check_lean_policy_mlp
    for h in (0, 2, 6, 36, 64, -4):
        assert _call(lib, _dims(), n_hidden=h) == EINVAL and f'n_hidden={h}' in err()
    assert _call(lib, _dims(), n_sets=0) == EINVAL and 'n_sets=0' in err()
    assert _call(lib, _dims(), reserved=1) == EINVAL and 'reserved must be 0' in err()
    assert _call(lib, _dims(), flags=1) == EINVAL and 'flags' in err()
    # check_policy_buffers
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
    # one workgroup row is the other kernel: named
    for n in (9, 17, 32):
        assert _call(lib, _dims(n_bldg=n)) == EINVAL and f'n_bldg={n}' in err() and 'clpol_rollout_mlp_f32' in err()
    assert _call(lib, _dims(n_bldg=17, tuning=tuned(b_chunk=17))) == EINVAL and 'b_chunk=17 >= n_bldg=17' in err() and 'clpol_rollout_mlp_f32' in err()
    assert _call(lib, _dims(n_bldg=12, tuning=tuned(b_chunk=16))) == EINVAL and 'b_chunk=16 >= n_bldg=12' in err() and 'clpol_rollout_mlp_f32' in err()
    # the chunk geometry
    assert _call(lib, _dims(tuning=tuned(b_chunk=33))) == EINVAL and 'b_chunk=33' in err() and 'at most 32' in err()
    assert _call(lib, _dims(n_bldg=80, tuning=tuned(b_chunk=40))) == EINVAL and 'b_chunk=40' in err() and 'at most 32' in err()
    assert _call(lib, _dims(tuning=tuned(b_chunk=-1))) == EINVAL and 'b_chunk=-1' in err()
    # nw: 2 nw >= b_chunk, nw <= 16, nw <= b_chunk
    assert _call(lib, _dims(tuning=tuned(nw=9))) == EINVAL and 'bad nw 9' in err() and 'b_chunk = 20' in err()             # 40 -> 20 + 20: ten waves
    assert _call(lib, _dims(tuning=tuned(nw=17))) == EINVAL and 'bad nw 17' in err()
    assert _call(lib, _dims(tuning=tuned(b_chunk=8, nw=9))) == EINVAL and 'bad nw 9' in err() and 'b_chunk = 8' in err()
    assert _call(lib, _dims(tuning=tuned(b_chunk=16, nw=7))) == EINVAL and 'bad nw 7' in err()
    assert _call(lib, _dims(tuning=tuned(nw=-2))) == EINVAL and 'bad nw -2' in err()
    # envs per lane
    assert _call(lib, _dims(tuning=tuned(vec=4))) == EINVAL and '4 envs per lane' in err()
    assert _call(lib, _dims(tuning=tuned(vec=-1))) == EINVAL and '-1 envs per lane' in err()
    # 40 buildings in chunks of 4: ten chunks need 10 x 5 = 50 rows of the reserved plane's 40 -- no room; 17 in chunks of 5 likewise
    assert _call(lib, _dims(tuning=tuned(b_chunk=4))) == EINVAL and 'b_chunk=4 leaves no room for the 10 chunk partial sums' in err()
    assert _call(lib, _dims(n_bldg=17, tuning=tuned(b_chunk=5))) == EINVAL and 'b_chunk=5 leaves no room for the 4 chunk partial sums' in err()
    # 10 buildings cut 5 + 5 need 10 rows of n_env floats AND the ticket / marker words
    assert _call(lib, _dims(n_bldg=10, tuning=tuned(b_chunk=5))) == EINVAL and 'leaves no room' in err()


def test_lds_beyond_a_cu_is_refused():
    """No geometry this library accepts reaches the CU's 160 KiB (sixteen waves x two envs per lane: 45 KiB) -- the refusal is the shared
    `check_policy_lds`, which the translation unit calls with its own label."""
    assert _lib.policy_chunk_lds_bytes(16, 2) == 46080 < 160 * 1024
    unit = (_lib.CSRC / 'cl_policy_chunk.hip').read_text()
    assert 'check_policy_lds(lds, "chunked policy", a.nw, vec)' in unit
    assert 'CL_LDS_PER_CU' in (_lib.CSRC / 'cl_policy_common.h').read_text()


# ---- 3. generated code ----------------------------------------------------------------------------------------------------------------
def _blocks(ins):
    """The instruction list cut at its labels: [(label | None, [instructions])]."""
    out = [(None, [])]
    for i in ins:
        if i.startswith('LABEL '):
            out.append((i.split()[1], []))
        else:
            out[-1][1].append(i)
    return out


def test_kernel_isa(tmp_path_factory):
    """Exactly the four instantiations of cl_rollout_policy_kernel<VEC, PREC, KPI = false, CHUNK = true> (csrc/cl_policy.h) and no CHUNK = false
    instantiation of it -- the one-row kernel -- or of the blind kernel in this unit; one cl_finish_kernel; at most 128 VGPRs (a 1024-thread workgroup's cap), no scratch memory, no static LDS in the rollout kernel.
    The policy tables are not fetched per lane inside the K loop: the two hidden-layer loops (one per seat, not unrolled: blocks that branch back
    to their own label) each hold one s_load_dwordx4 of `pre` and three broadcast ds_read_b128 -- six in the kernel -- and no barrier sits between
    them: the K loop holds none.  The vector loads that remain: per seat the three state planes, the previous net and the three staging reads."""
    (src, flags), = _lib.POLICY_CHUNK_SOURCES
    kernels, meta = _asm(src, flags, tmp_path_factory)
    names = [k for k in kernels if 'cl_rollout_policy_kernel' in k]
    by = {tuple(int(x) for x in re.search(r'cl_rollout_policy_kernelILi(\d)ELi(\d)ELb0ELb1EE', k).groups()): k for k in names}
    assert sorted(by) == [(1, 0), (1, 2), (2, 0), (2, 2)] and len(names) == 4
    assert not [k for k in kernels if 'cl_rollout_kernel' in k or 'cl_rollout_kpi_kernel' in k or 'cl_step' in k]
    assert len([k for k in kernels if 'cl_finish_kernel' in k]) == 1
    for (vec, prec), k in by.items():
        ins = kernels[k]
        print((vec, prec), meta[k])
        assert meta[k]['private_seg_size'] == 0, (k, meta[k])
        assert meta[k]['num_vgpr'] <= 128, (k, meta[k])
        assert not [i for i in ins if i.startswith(('scratch_', 'buffer_'))], k
        assert not [i for i in ins if re.match(r'v_pk_\w+_f32', i)], k
        assert any(i.startswith('v_fma_f64') for i in ins) == (prec == 2), k
        assert _count(ins, 'ds_read_b128') == 6, k
        assert _count(ins, 'global_load') == 14 + (vec == 2 and 2 or 0) + 1, (k, _count(ins, 'global_load'))
        blocks = _blocks(ins)
        hidden = [n for n, (label, body) in enumerate(blocks) if _count(body, 'ds_read_b128')]
        assert len(hidden) == 2, k
        for n in hidden:
            label, body = blocks[n]
            assert _count(body, 'ds_read_b128') == 3 and _count(body, 's_load_dwordx4') == 1, (k, label)
            assert _count(body, 'v_exp_f32') == 4 * vec and _count(body, 'v_rcp_f32') == 4 * vec, (k, label)
            assert [i for i in body if i.startswith('s_cbranch') and i.split()[-1] == label], (k, label)            # a loop of its own: not unrolled
            assert not _count(body, 'global_load'), (k, label)
        between = [i for _, body in blocks[hidden[0]:hidden[1] + 1] for i in body]
        assert not _count(between, 's_barrier') and _count(between, 'global_store') == 4, k                           # seat 0's record sits between them
        assert _count([i for _, body in blocks[:hidden[0]] for i in body], 's_barrier') == 1, k                       # the one behind the row staging
    text = next(tmp_path_factory.getbasetemp().glob('isa*/' + src.stem + '.s')).read_text()
    sizes = re.findall(r'\.group_segment_fixed_size:\s*(\d+)', text)
    assert sizes.count('4096') == 1 and set(sizes) == {'0', '4096'}, sizes          # (cl_finish_kernel's part[16][64]; the rollout kernel's LDS is dynamic)
    # the header's formula: the parent's, nw NQ tile + nw 2 CLPOL_ROW with CLPOL_ROW = 3 x 32 + 8
    head = (_lib.CSRC / 'cl_policy_chunk.h').read_text()
    assert re.search(r'rollout_policy_chunk_lds_floats\(int nw, int tile\) \{ return \(size_t\)nw \* NQ \* tile \+ \(size_t\)nw \* 2 \* CLPOL_ROW; \}', head)
    assert re.search(r'CLPOL_ROW = 3 \* CLPOL_MAX_H \+ 8;', (_lib.CSRC / 'cl_policy.h').read_text())
    for nw in (1, 8, 9, 10, 16):
        for vec in (1, 2):
            assert _lib.policy_chunk_lds_bytes(nw, vec) == 4 * (nw * abi.CL_NQ * 64 * vec + nw * 2 * (3 * policy.CLPOL_MAX_HIDDEN + 8))
    assert _lib.policy_chunk_lds_bytes(16, 1) == 29696 and _lib.policy_chunk_lds_bytes(16, 2) == 46080


# ---- 4. conditioning ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,H', CONDITIONED)
def test_closed_loop_is_well_conditioned(name, H):
    """tests/test_policy_host.py::test_closed_loop_is_well_conditioned's condition, 0.1 x (1e-4 + 1e-4 |ref|) on soc and net over K = 48, on the
    districts of more than 32 buildings the GPU tests run free (the table in tests/policy_chunk_util.py: 'b64' at H = 32 reads 0.161 and 'b1024'
    at H = 16 reads 0.111 on net -- those two are replayed through single steps only)."""
    err, tol, ref, pt = _conditioning(chunk_district(name), H)
    assert 0 < tol < 1e-5, tol
    driven = pt.es_cols >= 0
    act = ref['action'][:, driven]
    assert np.abs(act).max() > 0.05 and np.ptp(act) > 0.1                                 # a policy that does something
    if name == 'het40':
        assert sorted(np.nonzero(~driven)[0]) == sorted(HET40_UNDRIVEN)
    for k in ('soc', 'net'):
        print(f'{name} H={H} {k}: worst {err[k]:.4f} x (1e-4 + 1e-4 |ref|), action tolerance {tol:.3e}')
        assert err[k] < 0.1, (k, err[k])
