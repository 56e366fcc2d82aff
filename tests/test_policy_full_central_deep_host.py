"""The closed-loop rollout of THERMAL districts under a CENTRAL-AGENT policy with TWO hidden layers (`clpfcd_rollout_mlp_f32`, kernel
`cl_rollout_full_policy_central_kernel<PREC, MARL, true>` in csrc/cl_policy_full_central.h, library
``libcitylearn_amd_policy_full_central_deep.so``) as far as it can be checked without a GPU: the library's symbol list and struct, every refusal of
the host entry (before any HIP call), the LDS formula, the packer against the unsplit MLP in float64, the conditioning of the closed loop the GPU
tests run (tests/test_gpu_policy_full_central_deep_rollout.py), and the resource figures of every instantiation."""
import ctypes
import re

import numpy as np
import pytest

from golden_util import golden
from citylearn_amd import _lib, abi, policy
from citylearn_amd.observations import ObservationLayout
from citylearn_amd.policy import CLPF_NA, CLPF_ND, CentralStorageMLPPolicy, DeepCentralStorageMLPPolicy
from policy_full_central_deep_util import (CentralStorageObservations, DeepFullHostEntry, central_layout, f32_torch_deviation, host_closed_loop,
                                           make_deep_central_storage_policy, thermal_district)
from policy_util import exports
from test_isa_guards import _asm

EXT = _lib.POLICY_FULL_CENTRAL_DEEP


@pytest.fixture(scope='module')
def entry():
    return DeepFullHostEntry(EXT, n_bldg=9, flags=0, n_act_cols=25)


# ---- 1. the library -------------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header(entry):
    assert EXT.symbols == ['clpfcd_abi_version', 'clpfcd_core_abi_version', 'clpfcd_last_error', 'clpfcd_rollout_mlp_f32']
    assert exports(EXT.path) == EXT.symbols
    assert entry.lib.clpfcd_abi_version() == EXT.abi_version == 1 and entry.lib.clpfcd_core_abi_version() == abi.CL_ABI_VERSION
    assert policy.FULL_CENTRAL_DEEP_CONSTANTS == {'CLPFCD_ABI_VERSION': 1, 'CLPFCD_MAX_HIDDEN': 64, 'CLPFCD_MAX_BLDG': 16}
    src, = EXT.sources
    assert not isinstance(src, tuple) and src.name == 'cl_policy_full_central_deep.hip'     # the library's common flags, with SLP vectorisation
    assert 'compiled WITH SLP vectorisation' in src.read_text().split('#define')[0]
    assert EXT.path.name == 'libcitylearn_amd_policy_full_central_deep.so' and EXT.header.name == 'citylearn_amd_policy_full_central_deep.h'
    # the kernel is ONE template source with the one-hidden-layer kernel, which the two units include and nobody else; this unit instantiates
    # DEEP = true only
    assert not (_lib.CSRC / 'cl_policy_full_central_deep.h').exists()
    users = sorted(p.name for p in _lib.CSRC.glob('*.hip') if '#include "cl_policy_full_central.h"' in p.read_text())
    assert users == ['cl_policy_full_central.hip', 'cl_policy_full_central_deep.hip']
    assert 'CL_POLICY_LAUNCH(cl_rollout_full_policy_central_kernel<P, M, true>)' in src.read_text() and '<P, M, false>' not in src.read_text()


def test_struct_is_the_deep_thermal_policy_struct():
    """`clpfcd_mlp` is `clpfca_mlp`'s fields in order, then `n_hidden2, flags, l2` -- `clpfd_mlp`'s tail: `_lib.PolicyFullDeepMLP` and the shared
    host checks serve it."""
    def fields_of(header, name):
        text = abi._strip_comments(header.read_text())
        body = re.search(rf'typedef\s+struct\s+{name}\s*\{{(.*?)\}}\s*{name}\s*;', text, flags=re.S).group(1)
        fields = []
        for decl in body.split(';'):
            decl = decl.strip()
            if decl:
                first, *more = decl.split(',')
                fields += [re.sub(r'\[.*\]|\*', '', part).strip() for part in [first.split()[-1], *more]]
        return fields
    fields = fields_of(EXT.header, 'clpfcd_mlp')
    assert fields == fields_of(_lib.POLICY_FULL_CENTRAL.header, 'clpfca_mlp') + ['n_hidden2', 'flags', 'l2']
    assert fields == fields_of(_lib.POLICY_FULL_DEEP.header, 'clpfd_mlp') == [f for f, _ in _lib.PolicyFullDeepMLP._fields_]
    assert EXT.mlp is _lib.PolicyFullDeepMLP and ctypes.sizeof(_lib.PolicyFullDeepMLP) == 104


def test_the_extension_tuples():
    """The new tuple beside the unchanged ones, thirteen libraries, the build order, and the kind of its own."""
    assert _lib.CENTRAL_DEEP_THERMAL_EXTENSIONS == (EXT,)
    assert _lib.EXTENSIONS == (_lib.POLICY, _lib.POLICY_KPI, _lib.POLICY_FULL, _lib.POLICY_FULL_KPI)
    assert _lib.ALL_EXTENSIONS == _lib.EXTENSIONS + (_lib.POLICY_FULL_CHUNK,) and _lib.CHUNK_KPI_EXTENSIONS == (_lib.POLICY_FULL_CHUNK_KPI,)
    assert _lib.LEAN_CHUNK_EXTENSIONS == (_lib.POLICY_CHUNK,) and _lib.DEEP_EXTENSIONS == (_lib.POLICY_DEEP,)
    assert _lib.DEEP_THERMAL_EXTENSIONS == (_lib.POLICY_FULL_DEEP,) and _lib.CENTRAL_EXTENSIONS == (_lib.POLICY_CENTRAL,)
    assert _lib.CENTRAL_DEEP_EXTENSIONS == (_lib.POLICY_CENTRAL_DEEP,) and _lib.CENTRAL_THERMAL_EXTENSIONS == (_lib.POLICY_FULL_CENTRAL,)
    older = (_lib.ALL_EXTENSIONS + _lib.CHUNK_KPI_EXTENSIONS + _lib.LEAN_CHUNK_EXTENSIONS + _lib.DEEP_EXTENSIONS + _lib.DEEP_THERMAL_EXTENSIONS
             + _lib.CENTRAL_EXTENSIONS + _lib.CENTRAL_DEEP_EXTENSIONS + _lib.CENTRAL_THERMAL_EXTENSIONS)
    assert len(older) == 12 and EXT not in older
    every = older + _lib.CENTRAL_DEEP_THERMAL_EXTENSIONS
    assert len({e.path for e in every}) == 13 and len({e.prefix for e in every}) == 13
    import inspect
    import __graft_entry__
    src = inspect.getsource(__graft_entry__.build)
    assert (0 < src.index('_lib.CENTRAL_DEEP_EXTENSIONS') < src.index('_lib.CENTRAL_THERMAL_EXTENSIONS') < src.index('_lib.CENTRAL_DEEP_THERMAL_EXTENSIONS')
            < src.index('for ext, so in built:'))
    kind, one, th = DeepCentralStorageMLPPolicy.kind, CentralStorageMLPPolicy.kind, policy.StorageMLPPolicy.kind
    assert kind.terms == th.terms and kind.head_slots == th.head_slots and kind.head_shape == (CLPF_NA,) and kind.only == th.only
    assert kind.refuse_device_actions and kind.n_planes == policy.CLPF_NT == 10 and kind.one_row_max == 16 and kind.central
    assert kind.ext is EXT and kind.ext_kpi is None and kind.ext_chunk is None and kind.ext_chunk_kpi is None and kind.ext_chunk_pair is None
    assert kind.no_kpi_error is NotImplementedError and kind.max_hidden == 64 and kind.constants is policy.FULL_CENTRAL_DEEP_CONSTANTS
    assert kind.tables is policy.DeepCentralStoragePolicyTables and kind.struct is _lib.PolicyFullDeepMLP
    assert policy.DeepCentralStoragePolicyTables.kind is kind and policy.CentralStoragePolicyTables.kind is one and one is not kind
    assert one.ext is _lib.POLICY_FULL_CENTRAL and one.struct is _lib.PolicyFullMLP
    assert policy.DeepCentralPolicyTables.kind is policy.DeepCentralMLPPolicy.kind is not kind
    assert policy.DeepStoragePolicyTables.kind is policy.DeepStorageMLPPolicy.kind is not kind
    # both central thermal classes split the first layer with ONE function
    assert DeepCentralStorageMLPPolicy._pack_thermal_front is CentralStorageMLPPolicy._pack_thermal_front
    assert DeepCentralStorageMLPPolicy._pack_front is policy.CentralMLPPolicy._pack_front


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_before_any_hip_call(entry):
    """Every refusal of the entry with its code and whole message, from a call on host memory: a call that reached a launch would not return one
    of these codes."""
    e, L = entry, abi.CLD_LEAN
    EINVAL, ENULL, EALIGN, ERANGE = abi.CL_EINVAL, abi.CL_ENULL, abi.CL_EALIGN, abi.CL_ERANGE
    P = 'clpfcd_rollout_mlp_f32: '
    kind = lambda k: k << abi.CLD_REWARD_SHIFT
    HMSG = 'n_hidden=%d: the policy kernel takes 4, 8, .. 64 hidden units'
    H2MSG = 'n_hidden2=%d: the deep central thermal policy kernel takes 4, 8, .. 64 units in its second hidden layer'
    RMSG = 'clpfcd_mlp.flags / .reserved must be 0'
    NW = 'bad nw %d: the deep central thermal policy rollout runs one building per wave (nw = n_bldg = %d, at most 16)'
    for d, kw, code, msg in (
            (e.dims(flags=L), {}, EINVAL, P + 'thermal / outage districts only; a battery + PV district (CLD_LEAN) under a central-agent policy with two '
                                              'hidden layers goes to clpcd_rollout_mlp_f32 (libcitylearn_amd_policy_central_deep.so)'),
            (e.dims(n_bldg=17), {}, EINVAL, P + 'n_bldg=17 > 16: the central-agent thermal policy kernel holds the whole district in one workgroup (one '
                                                'building per wave); its hidden layers cannot be cut into building chunks'),
            (e.dims(flags=abi.CLD_F64_MAPS), {}, EINVAL, P + 'the battery map in fp32 or as the float64 chain (CLD_F64_CHAIN), not CLD_F64_MAPS'),
            (e.dims(flags=abi.CLD_KPI), {}, EINVAL, P + 'no streaming KPIs (CLD_KPI) inside this kernel -- record traj and replay CLPF_T_ACTION + head '
                                                        'through cl_rollout_seq_f32'),
            (e.dims(flags=abi.CLD_WRITE_DETAIL), {}, EINVAL, P + 'not with the detail planes (CLD_WRITE_DETAIL)'),
            (e.dims(flags=kind(abi.CLR_EV)), {}, EINVAL, P + 'reward kind CLR_EV needs the flexible-load tables'),
            (e.dims(env_pitch=128), {}, EINVAL, P + 'env_pitch=128 != n_env=64 is not implemented for this call'),
            (e.dims(n_act_cols=65537), {}, EINVAL, P + 'n_act_cols=65537 > 65536'),
            (e.dims(), dict(n_device_cols=2), EINVAL, P + 'n_device_cols=2: a building with a cooling / heating / combined device action column is not '
                                                          'covered (the policy has storage heads only)'),
            (e.dims(), dict(n_hidden=0), EINVAL, HMSG % 0),
            (e.dims(), dict(n_hidden=6), EINVAL, HMSG % 6),
            (e.dims(), dict(n_hidden=68), EINVAL, HMSG % 68),
            (e.dims(), dict(n_sets=0), EINVAL, 'n_sets=0: at least one parameter set'),
            (e.dims(), dict(n_hidden2=0), EINVAL, H2MSG % 0),
            (e.dims(), dict(n_hidden2=6), EINVAL, H2MSG % 6),
            (e.dims(), dict(n_hidden2=68), EINVAL, H2MSG % 68),
            (e.dims(), dict(flags=1), EINVAL, RMSG),                      # (CLPFD_MATRIX_CORES of the per-building deep kernel: no such family here)
            (e.dims(), dict(reserved=1), EINVAL, RMSG),
            (e.dims(), dict(l2=None), ENULL, 'mlp.l2 is NULL'),
            (e.dims(), dict(l2=e.ODD), EALIGN, 'mlp.l2 is not 16-byte aligned'),
            (e.dims(), dict(null='state'), ENULL, 'state is NULL'),
            (e.dims(), dict(null='params'), ENULL, 'params is NULL'),
            (e.dims(), dict(odd='traj'), EALIGN, 'traj is not 16-byte aligned'),
            (e.dims(), dict(odd='ret_env'), EALIGN, 'ret_env is not 16-byte aligned'),
            (e.dims(), dict(set_of_block=e.ODD1), EALIGN, 'mlp.set_of_block is not 4-byte aligned'),
            (e.dims(), dict(t0=95), ERANGE, 'steps [95, 103) outside [0, 100)'),
            (e.dims(), dict(t0=-1), ERANGE, 'steps [-1, 7) outside [0, 100)'),
            (e.dims(), dict(k_steps=-1), ERANGE, 'steps [0, -1) outside [0, 100)'),
            (e.dims(tun=dict(vec=2)), {}, EINVAL, 'no deep central thermal policy rollout kernel at 2 envs per lane: it runs at one env per lane'),
            (e.dims(tun=dict(vec=4)), {}, EINVAL, 'no deep central thermal policy rollout kernel at 4 envs per lane'),
            (e.dims(tun=dict(nw=8)), {}, EINVAL, NW % (8, 9)),
            (e.dims(tun=dict(nw=10)), {}, EINVAL, NW % (10, 9)),
            (e.dims(n_bldg=16, tun=dict(nw=17)), {}, EINVAL, NW % (17, 16))):
        assert e.call(d, **kw) == code and e.error() == msg, (kw, e.error())
    for name in ('pre', 'dep', 'out', 'act_low', 'act_high'):
        assert e.call(e.dims(), **{name: None}) == ENULL and e.error() == f'mlp.{name} is NULL'
    for name in ('pre', 'dep', 'out', 'net_reset', 'sigma'):
        assert e.call(e.dims(), **{name: e.ODD}) == EALIGN and e.error() == f'mlp.{name} is not 16-byte aligned'
    assert e.call(None) == ENULL and e.error() == 'dims is NULL'
    # which one wins: the coverage refusals come in the order above, all in front of the struct's and the buffers'; H1 in front of H2, the widths
    # in front of flags / reserved, l2 in front of the other tables and buffers, those in front of the step range, the envs per lane and nw last
    everything = abi.CLD_F64_MAPS | abi.CLD_KPI | abi.CLD_WRITE_DETAIL | kind(abi.CLR_EV)
    bad = dict(n_hidden=6, n_hidden2=6, flags=1, l2=None, null='state')
    assert e.call(e.dims(flags=L | everything, n_bldg=17, env_pitch=128, tun=dict(vec=2)), **bad) == EINVAL and 'CLD_LEAN' in e.error()
    assert e.call(e.dims(flags=everything, n_bldg=17, env_pitch=128, tun=dict(vec=2)), **bad) == EINVAL and 'n_bldg=17 > 16' in e.error()
    assert e.call(e.dims(flags=everything, env_pitch=128, tun=dict(vec=2)), **bad) == EINVAL and 'not CLD_F64_MAPS' in e.error()
    assert e.call(e.dims(flags=everything & ~abi.CLD_F64_MAPS, env_pitch=128, tun=dict(vec=2)), **bad) == EINVAL and 'CLPF_T_ACTION + head' in e.error()
    assert e.call(e.dims(flags=abi.CLD_WRITE_DETAIL | kind(abi.CLR_EV), env_pitch=128, tun=dict(vec=2)), **bad) == EINVAL and 'CLD_WRITE_DETAIL' in e.error()
    assert e.call(e.dims(flags=kind(abi.CLR_EV), env_pitch=128, tun=dict(vec=2)), **bad) == EINVAL and 'CLR_EV' in e.error()
    assert e.call(e.dims(env_pitch=128, tun=dict(vec=2)), **bad) == EINVAL and 'env_pitch=128' in e.error()
    assert e.call(e.dims(tun=dict(vec=2)), n_device_cols=1, **bad) == EINVAL and 'n_device_cols=1' in e.error()
    assert e.call(e.dims(tun=dict(vec=2)), **bad) == EINVAL and e.error() == HMSG % 6
    assert e.call(e.dims(tun=dict(vec=2)), **{**bad, 'n_hidden': 16}) == EINVAL and e.error() == H2MSG % 6
    assert e.call(e.dims(tun=dict(vec=2)), flags=1, l2=None, null='state') == EINVAL and e.error() == RMSG
    assert e.call(e.dims(tun=dict(vec=2)), l2=None, null='state', t0=95) == ENULL and e.error() == 'mlp.l2 is NULL'
    assert e.call(e.dims(tun=dict(vec=2)), null='state', t0=95) == ENULL and e.error() == 'state is NULL'
    assert e.call(e.dims(tun=dict(vec=2)), pre=None, t0=95) == ENULL and e.error() == 'mlp.pre is NULL'
    assert e.call(e.dims(tun=dict(vec=2)), t0=95) == ERANGE
    assert e.call(e.dims(tun=dict(vec=4, nw=8))) == EINVAL and '4 envs per lane' in e.error()
    # every accepted width of either layer gets past the struct's checks (it stops at the step range here)
    for h1, h2 in ((4, 64), (64, 4), (64, 64), (24, 40)):
        assert e.call(e.dims(), n_hidden=h1, n_hidden2=h2, t0=95) == ERANGE


def _header_lds_floats(nw, n_bldg, h1, h2):
    """The formula as include/citylearn_amd_policy_full_central_deep.h writes it, evaluated from the header's text."""
    text = EXT.header.read_text()
    m = re.search(r'Dynamic LDS per workgroup, in floats.*?\n \*\s+(nw x 4 x 64.*?)\n', text, flags=re.S)
    expr = m.group(1).replace('CLPFCD_MAX_HIDDEN', str(policy.CLPFCD_MAX_HIDDEN)).replace(' x ', ' * ')
    assert re.fullmatch(r'[\w\s*+()]+', expr), expr
    return eval(expr, {'__builtins__': {}}, dict(nw=nw, n_bldg=n_bldg, n_hidden=h1, n_hidden2=h2))


def test_lds_formula():
    """`_lib.policy_full_central_deep_lds_bytes` against the header's formula and the kernel header's function (nw == n_bldg); the launch opts in
    above 64 KiB and no accepted geometry reaches a CU's 160 KiB (the entry still holds it against that, through the shared `check_policy_lds`)."""
    for n_bldg in (1, 2, 9, 16):
        for h1, h2 in ((4, 4), (4, 64), (64, 4), (24, 40), (64, 64)):
            assert _lib.policy_full_central_deep_lds_bytes(n_bldg, h1, h2) == 4 * _header_lds_floats(n_bldg, n_bldg, h1, h2), (n_bldg, h1, h2)
            # the one-hidden-layer kernel's regions + Hh2 + the staged l2
            assert (_lib.policy_full_central_deep_lds_bytes(n_bldg, h1, h2)
                    == _lib.policy_full_central_lds_bytes(n_bldg, h1) + 4 * (h2 * 64 + (h1 + 1) * h2))
    assert _lib.policy_full_central_deep_lds_bytes(16, 64, 64) == 125184 == 4 * 31296 > 64 * 1024 and 125184 < _lib.LDS_PER_CU == 163840
    assert '125 184 bytes' in EXT.header.read_text()
    assert _lib.policy_full_central_deep_lds_bytes(16, 4, 4) == 58704 < 64 * 1024 < _lib.policy_full_central_deep_lds_bytes(16, 32, 32) == 86144
    assert _lib.policy_full_central_deep_lds_bytes(9, 32, 16) == 4 * (9 * 256 + 45 * 64 + 32 * 64 + 16 * 64 + 160 * 9 + 33 * 16 + 9 * 288) == 51264
    head, unit = (_lib.CSRC / 'cl_policy_full_central.h').read_text(), (_lib.CSRC / 'cl_policy_full_central_deep.hip').read_text()
    assert ('return (size_t)nw * NQ * 64 + (size_t)CLPF_ND * n_bldg * 64 + (size_t)h1 * 64 + (size_t)h2 * 64 + (size_t)CLPF_ND * h1 * n_bldg + '
            '(size_t)(h1 + 1) * h2\n           + (size_t)nw * CLPFC_ROW;' in head
            and 'CLPFC_MAX_HIDDEN = 64;' in head and 'CLPFC_HEADS = CLPF_NA * CLPFC_MAX_HIDDEN;' in head and 'CLPFC_ROW = CLPFC_HEADS + 8 * CLPF_NA;' in head
            and 'static_assert(CLPFCD_MAX_HIDDEN == CLPFC_MAX_HIDDEN,' in unit and policy.CLPFCD_MAX_HIDDEN == 64
            and abi.CL_NQ == 4 and (CLPF_ND, CLPF_NA) == (5, 4))
    assert ('check_policy_lds(lds, "deep central thermal policy", a.nw, 1)' in unit
            and 'CL_POLICY_LAUNCH(cl_rollout_full_policy_central_kernel<P, M, true>)' in unit)
    shared = (_lib.CSRC / 'cl_policy_common.h').read_text()
    assert 'if (lds > 64 * 1024) if (hipError_t e = ensure_dynamic_lds(' in shared and 'if (lds > CL_LDS_PER_CU) return fail(' in shared


# ---- 3. the packer --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('H1,H2', [(4, 64), (24, 40)])
@pytest.mark.parametrize('name', ['g2020_cz1', 't2', 't2_outage'])
def test_packed_layers_equal_the_unsplit_mlp(name, H1, H2, normalize):
    """`pre + dep x`, `l2` and `out` rebuilt on the host in float64 from the float32 tables against `actions_host` (the unsplit MLP in float64) on
    central-agent vectors with random state, two parameter sets with `set_of_block`.  The tolerance is
    tests/test_policy_full_central_host.py's with one layer more, as tests/test_policy_central_deep_host.py carries it: every packed number has one
    float32 rounding (2^-24 relative); through tanh (slope <= 1) the action moves by at most half x 2^-24 x (the l1 mass of each layer's terms,
    propagated), taken with a factor 2.  H1 != H2 throughout: a swapped axis of l2 or out does not pass.  The first layer is bit for bit what
    `CentralStorageMLPPolicy.pack` makes of the same W1 / b1: the same zero rows for a storage a building lacks."""
    spec = thermal_district(name)
    tab = spec.episode_tables(0)
    layout = central_layout(spec, normalize)
    B = len(spec.buildings)
    pol = make_deep_central_storage_policy(layout, H1, H2, n_sets=2, seed=3, mid_scale=1.0)
    pt = pol.pack(layout, tab, set_of_block=[1, 0])
    assert isinstance(pt, policy.DeepCentralStoragePolicyTables) and isinstance(pt, policy.CentralStoragePolicyTables)
    assert (pt.n_hidden, pt.n_hidden2, pt.n_sets, pt.n_bldg, pt.n_rows) == (H1, H2, 2, B, tab.n_steps)
    assert tuple(pt.pre.shape) == (2, tab.n_steps, H1) and tuple(pt.dep.shape) == (2, H1 // 4, B, CLPF_ND, 4)
    assert tuple(pt.l2.shape) == (2, H1 + 1, H2) and tuple(pt.out.shape) == (2, B, CLPF_NA, H2 + 1) and pt.l2.is_contiguous() and pt.out.is_contiguous()
    assert tuple(pt.net_reset.shape) == (tab.n_steps, B) and pt.low_bldg.shape == pt.high_bldg.shape == pt.sigma_bldg.shape == pt.cols.shape == (B, CLPF_NA)
    assert pt.set_of_block.tolist() == [1, 0] and np.array_equal(pt.cols, policy.head_columns(tab)) and pt.n_device_cols == 0
    st = pt.struct(5)
    assert isinstance(st, _lib.PolicyFullDeepMLP)
    assert (st.n_hidden, st.n_sets, st.n_device_cols, st.reserved, st.seed, st.n_hidden2, st.flags) == (H1, 2, 0, 0, 5, H2, 0)
    assert st.pre == pt.pre.data_ptr() and st.dep == pt.dep.data_ptr() and st.l2 == pt.l2.data_ptr() and st.out == pt.out.data_ptr()
    one = CentralStorageMLPPolicy(pol.w1, pol.b1, np.zeros((1, B, CLPF_NA, H1)), np.zeros((1, B, CLPF_NA))).pack(layout, tab, set_of_block=[1, 0])
    assert np.array_equal(one.pre.numpy(), pt.pre.numpy()) and np.array_equal(one.dep.numpy(), pt.dep.numpy())
    assert np.array_equal(one.net_reset.numpy(), pt.net_reset.numpy()) and np.array_equal(one.cols, pt.cols)
    cobs = CentralStorageObservations(layout, tab)
    terms = pt.dep_terms()
    assert tuple(terms.shape) == (2, B, CLPF_ND, H1) and not terms[:, :, policy.CLPF_D_HS].any()
    bflags = np.ascontiguousarray(tab.params).view(np.uint32)[:, abi.CLP_FLAGS]
    for b in range(B):
        has_ds = bool(bflags[b] & abi.CLF_DHW_STO)
        assert bool(terms[:, b, policy.CLPF_D_DS].any()) == has_ds == (pt.cols[b, policy.CLPF_A_DS] >= 0)
    rng = np.random.RandomState(5)
    E, S, u = 5, policy.ACT_SCALE, 2.0 ** -24
    for s in range(2):
        pre, dep = pt.pre[s].numpy().astype(np.float64), terms[s].numpy().astype(np.float64)
        l2, out = pt.l2[s].numpy().astype(np.float64), pt.out[s].numpy().astype(np.float64)
        _, _, w2, b2, w3, b3 = (v[s] for v in pol._full(B))
        assert np.allclose(l2[:H1].T, S * w2, rtol=2 * u, atol=0) and np.allclose(l2[H1], S * b2, rtol=2 * u, atol=0)
        assert np.allclose(out[:, :, :H2], w3, rtol=2 * u, atol=0) and np.allclose(out[:, :, H2], b3, rtol=2 * u, atol=0)
        for r in (1, 9, 100):
            planes = [rng.uniform(0, 1, size=(B, E)) for _ in range(4)] + [rng.uniform(-3, 6, size=(B, E))]
            parts = [dep[None, :, d] * planes[d].T[:, :, None] for d in range(CLPF_ND)]                         # [E, B, H1] each, scaled
            z1 = pre[r][None] + sum(p.sum(axis=1) for p in parts)
            m1 = np.abs(pre[r][None]) + sum(np.abs(p).sum(axis=1) for p in parts)
            h1 = np.tanh(z1 / S)
            e1 = 2 * u * m1 / abs(S)
            z2 = l2[None, H1] + np.einsum('ji,ej->ei', l2[:H1], h1)                                               # [E, H2], scaled
            m2 = np.abs(l2[None, H1]) + np.einsum('ji,ej->ei', np.abs(l2[:H1]), np.abs(h1))
            e2 = (2 * u * m2 + np.einsum('ji,ej->ei', np.abs(l2[:H1]), e1)) / abs(S)
            h2 = np.tanh(z2 / S)
            z3 = out[None, :, :, H2] + np.einsum('bai,ei->eba', out[:, :, :H2], h2)
            e3 = (2 * u * (np.abs(out[None, :, :, H2]) + np.einsum('bai,ei->eba', np.abs(out[:, :, :H2]), np.abs(h2)))
                  + np.einsum('bai,ei->eba', np.abs(out[:, :, :H2]), e2))
            half = 0.5 * (pt.high_bldg - pt.low_bldg)
            got = np.clip(0.5 * (pt.high_bldg + pt.low_bldg) + half * np.tanh(z3), pt.low_bldg, pt.high_bldg)
            want = pol.actions_host(cobs.at(r, *planes), pt, set_index=s)
            present = pt.cols >= 0
            assert want.shape == (E, B, CLPF_NA) and want.dtype == np.float64 and not want[:, ~present].any()
            assert np.all(np.abs(got - want)[:, present] <= (half * e3)[:, present] + 1e-15), float(np.abs(got - want)[:, present].max())
            assert np.abs(got - want)[:, present].max() < 1e-6


def test_packer_surface():
    """`CentralStorageMLPPolicy`'s surface with six arrays: leading-1 broadcasting, `update` / `invalidate` / `version`, `set_of_block`, sigma, and
    the `ValueError`s of the constructor and the packer."""
    spec = thermal_district('g2020_cz1')
    tab = spec.episode_tables(0)
    layout = central_layout(spec)
    N, B = layout.n_cols, 9
    rng = np.random.RandomState(1)
    u = lambda a, *shape: rng.uniform(-a, a, shape)
    pol = DeepCentralStorageMLPPolicy(u(0.1, 1, 8, N), u(0.5, 3, 8), u(0.3, 1, 12, 8), u(0.5, 1, 12), u(0.3, 1, B, 4, 12), np.zeros((1, B, 4)), sigma=0.1)
    assert (pol.n_sets, pol.n_hidden, pol.n_hidden2, pol.n_obs, pol.n_bldg, pol.version) == (3, 8, 12, N, B, 0)
    pt = pol.pack(layout, tab, set_of_block=[2, 0, 1])
    assert pt.version == 0 and pt.n_sets == 3 and pt.set_of_block.tolist() == [2, 0, 1]
    assert np.all(pt.sigma_bldg[pt.cols >= 0] == 0.1) and not pt.sigma_bldg[pt.cols < 0].any() and tuple(pt.sigma.shape) == (25,)
    assert bool((pt.out == pt.out[:1]).all()) and bool((pt.l2 == pt.l2[:1]).all()) and bool((pt.dep == pt.dep[:1]).all())
    assert not bool((pt.pre[0] == pt.pre[1]).all())
    cobs = CentralStorageObservations(layout, tab)
    x = cobs.at(3, *[np.full((B, 2), 0.5)] * 4, np.zeros((B, 2)))
    a0 = pol.actions_host(x, pt)
    assert a0.shape == (2, B, 4) and not np.array_equal(pol.actions_host(x, pt, set_index=1), a0)
    z = np.ones((2, B, 4))
    assert np.allclose(pol.actions_host(x, pt, noise=z), np.where(pt.cols >= 0, np.clip(a0 + 0.1, pt.low_bldg, pt.high_bldg), 0.0))
    six = lambda p, **kw: DeepCentralStorageMLPPolicy(p.w1, p.b1, p.w2, p.b2, p.w3, p.b3, **kw)
    ppt = six(pol, sigma=np.linspace(0, 0.24, 25)).pack(layout, tab)
    assert np.allclose(ppt.sigma_bldg[ppt.cols >= 0], np.linspace(0, 0.24, 25)[ppt.cols[ppt.cols >= 0]])
    with pytest.raises(ValueError, match='sigma: a non-negative scalar'):
        six(pol, sigma=[0.1, 0.2]).pack(layout, tab)
    mid = 0.5 * (pt.high_bldg + pt.low_bldg)
    pol.update(w3=-pol.w3)
    assert pol.version == 1 and pol.pack(layout, tab).version == 1
    assert np.allclose((pol.actions_host(x, pt) - mid)[:, pt.cols >= 0], -(a0 - mid)[:, pt.cols >= 0])          # (b3 = 0: the heads are odd in w3)
    pol.invalidate()
    assert pol.version == 2
    with pytest.raises(ValueError, match='w2: shape'):
        pol.update(w2=np.zeros((1, 8, 12)))
    with pytest.raises(ValueError, match='set_of_block outside'):
        pol.pack(layout, tab, set_of_block=[3])
    zz = np.zeros
    good = ((1, 8, N), (1, 8), (1, 12, 8), (1, 12), (1, B, 4, 12), (1, B, 4))
    swap = lambda i, shape: tuple(shape if k == i else s for k, s in enumerate(good))
    for shapes, msg in ((swap(0, (1, 1, 8, N)), 'w1 .n_sets, H1, n_cols.'),
                        (swap(4, (1, B, 12)), 'w3 .n_sets, n_bldg, 4, H2.'),
                        (((1, 6, N), (1, 6), (1, 12, 6), (1, 12), (1, B, 4, 12), (1, B, 4)), 'H1=6'),
                        (((1, 68, N), (1, 68), (1, 12, 68), (1, 12), (1, B, 4, 12), (1, B, 4)), 'H1=68'),
                        (((1, 8, N), (1, 8), (1, 6, 8), (1, 6), (1, B, 4, 6), (1, B, 4)), 'H2=6'),
                        (((1, 8, N), (1, 8), (1, 68, 8), (1, 68), (1, B, 4, 68), (1, B, 4)), 'H2=68'),
                        (swap(1, (1, 4)), 'about H1'),
                        (swap(2, (1, 12, 4)), 'about H1'),
                        (swap(2, (1, 8, 12)), 'H1'),                               # W2 handed over transposed
                        (swap(3, (1, 8)), 'about H2'),
                        (swap(4, (1, B, 4, 8)), 'about H2'),
                        (((1, 8, N), (1, 8), (1, 12, 8), (1, 12), (1, B, 3, 12), (1, B, 3)), 'do not have 4 heads'),
                        (swap(5, (1, B - 1, 4)), 'about n_bldg')):
        with pytest.raises(ValueError, match=msg):
            DeepCentralStorageMLPPolicy(*[zz(s) for s in shapes])
    big = DeepCentralStorageMLPPolicy(zz((1, 64, N)), zz((1, 64)), zz((1, 4, 64)), zz((1, 4)), zz((1, B, 4, 4)), zz((1, B, 4))).pack(layout, tab)
    assert (big.n_hidden, big.n_hidden2) == (64, 4) and tuple(big.l2.shape) == (1, 65, 4) and tuple(big.out.shape) == (1, B, 4, 5)
    with pytest.raises(ValueError, match='do not broadcast to 3 sets'):
        DeepCentralStorageMLPPolicy(zz((2, 8, N)), zz((3, 8)), *[zz(s) for s in good[2:]]).pack(layout, tab)
    # the layout must be the central agent's, of this length, over this many buildings
    with pytest.raises(ValueError, match='a DeepCentralStorageMLPPolicy is defined over.*central_agent=False'):
        pol.pack(ObservationLayout(spec, 'current', True, central_agent=False), tab)
    with pytest.raises(ValueError, match='central_agent=False'):
        pol.torch_policy(ObservationLayout(spec, 'current', True, central_agent=False), tab, 'cpu')
    with pytest.raises(ValueError, match=f'w1 takes {N} observations, the central-agent vector has'):
        pol.pack(central_layout(spec, normalize=False), tab)
    spec2 = thermal_district('t2')
    lay2 = central_layout(spec2)
    with pytest.raises(ValueError, match='heads for 9 buildings, the district has 2'):
        DeepCentralStorageMLPPolicy(zz((1, 8, lay2.n_cols)), *[zz(s) for s in good[1:]]).pack(lay2, spec2.episode_tables(0))
    with pytest.raises(ValueError, match='observation_mode="reference"'):
        lay_ref = ObservationLayout(spec, 'reference', True, central_agent=True)
        DeepCentralStorageMLPPolicy(zz((1, 8, lay_ref.n_cols)), *[zz(s) for s in good[1:]]).pack(lay_ref, tab)


def test_packer_refuses_the_lstm_stage_and_device_actions():
    """g2023_p2, as tests/test_policy_full_central_host.py's test of the same name: the indoor temperature is fed by the LSTM stage (SRC_TEMP) and
    the buildings have device actions -- `CentralStorageMLPPolicy.pack`'s messages, the observation first; with the observation out of the way,
    the device action."""
    spec = golden('g2023_p2').spec()
    tab = spec.episode_tables(0)
    layout = central_layout(spec)
    B = len(spec.buildings)
    pol = DeepCentralStorageMLPPolicy(np.zeros((1, 8, layout.n_cols)), np.zeros((1, 8)), np.zeros((1, 12, 8)), np.zeros((1, 12)),
                                      np.zeros((1, B, 4, 12)), np.zeros((1, B, 4)))
    with pytest.raises(ValueError, match=r"'indoor_dry_bulb_temperature\w*' of building 0 .*the thermal policy kernel only has.*LSTM stage"):
        pol.pack(layout, tab)
    good = layout.episode

    def without_temperature(tab_, reset_table=False):
        o = good(tab_, reset_table=reset_table)
        for c in np.nonzero(o.col_src >= 0)[0]:
            kind, plane = int(o.col_src[c]) >> 28, (int(o.col_src[c]) >> 20) & 0xFF
            if (kind, plane) not in ((0, abi.CLS_B_SOC), (0, abi.CLS_CS_SOC), (0, abi.CLS_HS_SOC), (0, abi.CLS_DS_SOC), (1, abi.CLO_NET)):
                o.col_src[c] = -1
                if o.reset_table is not None:
                    o.reset_table[1:, c] = o.table[1:, c]
        return o
    layout.episode = without_temperature
    with pytest.raises(ValueError, match=r"action 'cooling\w*device' of building 0 \(column \d+\): the thermal policy kernel has storage heads only"):
        pol.pack(layout, tab)
    del layout.episode


def test_torch_policy_is_the_same_mlp():
    """`torch_policy` over a central-agent observation tensor against `actions_host`, in float64 on the CPU; action columns without a head stay 0."""
    import torch
    spec = thermal_district('g2020_cz1')
    tab = spec.episode_tables(0)
    layout = central_layout(spec)
    pol = make_deep_central_storage_policy(layout, 16, 24, seed=2, mid_scale=1.0)
    pt = pol.pack(layout, tab)
    cobs = CentralStorageObservations(layout, tab)
    rng = np.random.RandomState(2)
    x = cobs.at(11, *[rng.uniform(0, 1, (9, 6)) for _ in range(4)], rng.uniform(-2, 4, (9, 6)))
    f = pol.torch_policy(layout, tab, 'cpu', dtype=torch.float64)
    got = f(torch.from_numpy(x)).numpy().astype(np.float64)                   # [n_act, E] (float32 on the way out)
    want = pol.actions_host(x, pt)                                            # [E, B, 4]
    b, h = np.nonzero(pt.cols >= 0)
    assert got.shape == (25, 6) and len(b) == 25 and np.allclose(got[pt.cols[b, h]], want[:, b, h].T, rtol=0, atol=2e-7)
    assert float(np.abs(want[:, b, h]).max()) > 0.01
    # layer 2 matters: another middle layer, other actions
    other = DeepCentralStorageMLPPolicy(pol.w1, pol.b1, -pol.w2, pol.b2, pol.w3, pol.b3)
    assert np.abs(other.actions_host(x, pt) - want)[:, b, h].max() > 1e-3


# ---- 4. conditioning of the closed loop -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H1,H2', [(4, 4), (32, 32), (64, 64), (64, 4)])
@pytest.mark.parametrize('name', ['g2020_cz1', 't1', 't2', 't16'])
def test_closed_loop_is_well_conditioned(name, H1, H2):
    """tests/test_policy_full_central_host.py::test_closed_loop_is_well_conditioned, its state criterion unchanged and its action
    criterion adapted (below: no |action| > 0.05, smaller thresholds on t1 / t2), for the test policies with two hidden layers
    of the free-running GPU test, before any GPU run: the CPU oracle stepped K = 48 from reset with `actions_host` in float64, against the
    same loop with every action rounded through float32 and moved by the GPU teacher-forced tolerance -- 4 x the worst deviation of a float32
    torch evaluation on this trajectory's own observations: soc, cs, ds and net must stay within 0.1 x (1e-4 + 1e-4 |ref|), while the policy
    does something.  Fixes policy_full_central_deep_util.MID_SCALE (readings there)."""
    spec = thermal_district(name)
    K, E = 48, 4
    tab = spec.episode_tables(0)
    layout = central_layout(spec)
    pol = make_deep_central_storage_policy(layout, H1, H2, seed=H1 + H2)
    pt = pol.pack(layout, tab)
    ref = host_closed_loop(spec, tab, layout, pol, pt, K, E)
    cobs = CentralStorageObservations(layout, tab)
    x = np.stack([cobs.at(t, *[ref[k][t - 1] for k in ('soc', 'cs', 'hs', 'ds', 'net')]) for t in range(1, K)])
    tol = 4.0 * f32_torch_deviation(pol, x, pt)
    got = host_closed_loop(spec, tab, layout, pol, pt, K, E, perturb=tol, round_f32=True)
    assert 0 < tol < 1e-5, tol
    act = ref['action'].transpose(0, 3, 2, 1)[:, :, pt.cols >= 0]
    # a policy that does something.  The sizes follow from the weight scales, not from a run: a head's sum is b3 (+-0.4 W2_SCALE = +-0.05) plus H2
    # products of a weight in +-W2_SCALE / sqrt(H2) and an h2 of rms <= 0.5 (tanh of a bias in +-0.5 plus a sum of rms ~ 0.3), i.e. rms <~ 0.04,
    # times half <= 1: actions of a few hundredths.  So (a) the many heads of g2020_cz1 / t16 (25 / 40 independent draws) must span more than
    # 0.05 between them -- tests/test_policy_full_central_host.py's range; its |action| > 0.05 is that test's ONE-layer size and is not asked for
    # here: the second tanh halves what reaches the heads; (b) t1 / t2 have ONE seeded draw of three to five heads per shape, where all the closed
    # loop needs is an action that is not 0 and moves with the observations: tests/test_policy_central_deep_host.py's thresholds for its
    # one-building district; (c) everywhere the loop must be DRIVEN: some head moves with the observations by more than 1000 x the perturbation.
    assert np.ptp(act) > 0.05 if name in ('g2020_cz1', 't16') else (np.abs(act).max() > 1e-3 and np.ptp(act) > 1e-4)
    moves = float(np.ptp(act.reshape(-1, act.shape[-1]), axis=0).max())
    assert moves > 1e3 * tol, (moves, tol)
    assert not ref['hs'].any() and (np.abs(ref['cs']).max() > 0.05 or name in ('t1', 't2'))
    for k in ('soc', 'cs', 'ds', 'net'):
        err = float((np.abs(got[k] - ref[k]) / (1e-4 + 1e-4 * np.abs(ref[k]))).max())
        print(f'{name} H1={H1} H2={H2} {k}: worst {err:.4f} x (1e-4 + 1e-4 |ref|), action tolerance {tol:.3e}, |action| max {np.abs(act).max():.3f}, '
              f'range {np.ptp(act):.3f}')
        assert err < 0.1, (name, k, err)


# ---- 5. generated code ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def central_deep_unit(tmp_path_factory):
    src, = EXT.sources
    return _asm(src, [], tmp_path_factory)


def test_central_deep_thermal_kernel_resources(central_deep_unit):
    """Every instantiation of cl_rollout_full_policy_central_kernel<PREC, MARL, true> -- the fp32 map and the float64 chain, with and without the
    MARL exchange: no scratch memory and at most 128 registers, a 1024-thread workgroup's limit.  The unit holds no other rollout or step kernel."""
    kernels, meta = central_deep_unit
    names = [k for k in kernels if 'cl_rollout_full_policy_central_kernel' in k]
    by = {}
    for k in names:
        m = re.search(r'cl_rollout_full_policy_central_kernelILi(\d)ELb(\d)ELb1EE', k)
        by[(int(m.group(1)), bool(int(m.group(2))))] = k
    assert sorted(by) == [(0, False), (0, True), (2, False), (2, True)] and len(names) == 4
    assert not [k for k in kernels if k not in names and ('cl_rollout' in k or 'cl_step' in k)]
    for key, k in by.items():
        assert meta[k]['private_seg_size'] == 0, k
        assert meta[k]['num_vgpr'] <= 128, (k, meta[k])
