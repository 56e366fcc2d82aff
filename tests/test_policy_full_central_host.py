"""The closed-loop rollout of THERMAL districts under a CENTRAL-AGENT policy (`clpfca_rollout_mlp_f32`, kernel
`cl_rollout_full_policy_central_kernel<PREC, MARL, false>` in csrc/cl_policy_full_central.h, library ``libcitylearn_amd_policy_full_central.so``)
as far as it can be checked without a GPU: the library's symbol list and struct, every refusal of the host entry (before any HIP call), the LDS formula, the packer
against the unsplit MLP in float64, the conditioning of the closed loop the GPU tests run (tests/test_gpu_policy_full_central_rollout.py), and the
resource figures of every instantiation."""
import ctypes
import re

import numpy as np
import pytest

from golden_util import golden
from citylearn_amd import _lib, abi, policy
from citylearn_amd.observations import ObservationLayout
from citylearn_amd.policy import CLPF_NA, CLPF_ND, CentralStorageMLPPolicy
from policy_full_central_util import (CentralStorageObservations, HostEntry, central_layout, f32_torch_deviation, host_closed_loop,
                                      make_central_storage_policy, thermal_district)
from policy_util import exports
from test_isa_guards import _asm

EXT = _lib.POLICY_FULL_CENTRAL


@pytest.fixture(scope='module')
def entry():
    return HostEntry(EXT, n_bldg=9, flags=0, n_act_cols=25)


# ---- 1. the library -------------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header(entry):
    assert EXT.symbols == ['clpfca_abi_version', 'clpfca_core_abi_version', 'clpfca_last_error', 'clpfca_rollout_mlp_f32']
    assert exports(EXT.path) == EXT.symbols
    assert entry.lib.clpfca_abi_version() == EXT.abi_version == 1 and entry.lib.clpfca_core_abi_version() == abi.CL_ABI_VERSION
    assert policy.FULL_CENTRAL_CONSTANTS == {'CLPFCA_ABI_VERSION': 1, 'CLPFCA_MAX_HIDDEN': 64, 'CLPFCA_MAX_BLDG': 16}
    src, = EXT.sources
    assert not isinstance(src, tuple) and src.name == 'cl_policy_full_central.hip'          # the library's common flags, with SLP vectorisation
    assert 'compiled WITH SLP vectorisation' in src.read_text().split('#define')[0]
    assert (_lib.CSRC / 'cl_policy_full_central.h').exists() and EXT.path.name == 'libcitylearn_amd_policy_full_central.so'
    assert EXT.header.name == 'citylearn_amd_policy_full_central.h'


def test_struct_is_the_thermal_policy_struct():
    """`clpfca_mlp` keeps `clpf_mlp`'s field names and order: `_lib.PolicyFullMLP` and the shared host checks serve it."""
    def fields(header, name):
        text = abi._strip_comments(header.read_text())
        body = re.search(rf'typedef\s+struct\s+{name}\s*\{{(.*?)\}}\s*{name}\s*;', text, flags=re.S).group(1)
        out = []
        for decl in body.split(';'):
            decl = decl.strip()
            if decl:
                first, *more = decl.split(',')
                out += [re.sub(r'\[.*\]|\*', '', part).strip() for part in [first.split()[-1], *more]]
        return out
    mine = fields(EXT.header, 'clpfca_mlp')
    assert [f for f, _ in _lib.PolicyFullMLP._fields_] == mine == fields(_lib.POLICY_FULL.header, 'clpf_mlp')
    assert EXT.mlp is _lib.PolicyFullMLP and ctypes.sizeof(_lib.PolicyFullMLP) == 88


def test_the_extension_tuples():
    """The new tuple beside the unchanged ones, twelve libraries, the build order, and the kind of its own."""
    assert _lib.CENTRAL_THERMAL_EXTENSIONS == (EXT,)
    assert _lib.EXTENSIONS == (_lib.POLICY, _lib.POLICY_KPI, _lib.POLICY_FULL, _lib.POLICY_FULL_KPI)
    assert _lib.ALL_EXTENSIONS == _lib.EXTENSIONS + (_lib.POLICY_FULL_CHUNK,) and _lib.CHUNK_KPI_EXTENSIONS == (_lib.POLICY_FULL_CHUNK_KPI,)
    assert _lib.LEAN_CHUNK_EXTENSIONS == (_lib.POLICY_CHUNK,) and _lib.DEEP_EXTENSIONS == (_lib.POLICY_DEEP,)
    assert _lib.DEEP_THERMAL_EXTENSIONS == (_lib.POLICY_FULL_DEEP,) and _lib.CENTRAL_EXTENSIONS == (_lib.POLICY_CENTRAL,)
    assert _lib.CENTRAL_DEEP_EXTENSIONS == (_lib.POLICY_CENTRAL_DEEP,)
    older = (_lib.ALL_EXTENSIONS + _lib.CHUNK_KPI_EXTENSIONS + _lib.LEAN_CHUNK_EXTENSIONS + _lib.DEEP_EXTENSIONS + _lib.DEEP_THERMAL_EXTENSIONS
             + _lib.CENTRAL_EXTENSIONS + _lib.CENTRAL_DEEP_EXTENSIONS)
    assert len(older) == 11 and EXT not in older
    every = older + _lib.CENTRAL_THERMAL_EXTENSIONS
    assert len({e.path for e in every}) == 12 and len({e.prefix for e in every}) == 12
    import inspect
    import __graft_entry__
    src = inspect.getsource(__graft_entry__.build)
    assert 0 < src.index('_lib.CENTRAL_DEEP_EXTENSIONS') < src.index('_lib.CENTRAL_THERMAL_EXTENSIONS') < src.index('for ext, so in built:')
    kind, th = CentralStorageMLPPolicy.kind, policy.StorageMLPPolicy.kind
    assert kind.terms == th.terms and kind.head_slots == th.head_slots and kind.head_shape == (CLPF_NA,) and kind.only == th.only
    assert kind.refuse_device_actions and kind.n_planes == policy.CLPF_NT == 10 and kind.one_row_max == 16 and kind.central
    assert kind.ext is EXT and kind.ext_kpi is None and kind.ext_chunk is None and kind.ext_chunk_kpi is None and kind.ext_chunk_pair is None
    assert kind.no_kpi_error is NotImplementedError and kind.max_hidden == 64 and kind.constants is policy.FULL_CENTRAL_CONSTANTS
    assert kind.tables is policy.CentralStoragePolicyTables and kind.struct is _lib.PolicyFullMLP
    assert policy.CentralStoragePolicyTables.kind is kind and policy.CentralPolicyTables.kind is policy.CentralMLPPolicy.kind is not kind
    assert policy.StoragePolicyTables.kind is th and th is not kind and not th.central


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_before_any_hip_call(entry):
    """Every refusal of the entry with its code and whole message, from a call on host memory: a call that reached a launch would not return one
    of these codes."""
    e, L = entry, abi.CLD_LEAN
    EINVAL, ENULL, EALIGN, ERANGE = abi.CL_EINVAL, abi.CL_ENULL, abi.CL_EALIGN, abi.CL_ERANGE
    P = 'clpfca_rollout_mlp_f32: '
    kind = lambda k: k << abi.CLD_REWARD_SHIFT
    HMSG = 'n_hidden=%d: the policy kernel takes 4, 8, .. 64 hidden units'
    NW = 'bad nw %d: the central thermal policy rollout runs one building per wave (nw = n_bldg = %d, at most 16)'
    for d, kw, code, msg in (
            (e.dims(flags=L), {}, EINVAL, P + 'thermal / outage districts only; a battery + PV district (CLD_LEAN) under a central-agent policy goes to '
                                              'clpca_rollout_mlp_f32 (libcitylearn_amd_policy_central.so)'),
            (e.dims(n_bldg=17), {}, EINVAL, P + 'n_bldg=17 > 16: the central-agent thermal policy kernel holds the whole district in one workgroup (one '
                                                'building per wave); its hidden layer cannot be cut into building chunks'),
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
            (e.dims(), dict(reserved=1), EINVAL, 'clpfca_mlp.reserved must be 0'),
            (e.dims(), dict(null='state'), ENULL, 'state is NULL'),
            (e.dims(), dict(null='params'), ENULL, 'params is NULL'),
            (e.dims(), dict(odd='traj'), EALIGN, 'traj is not 16-byte aligned'),
            (e.dims(), dict(odd='ret_env'), EALIGN, 'ret_env is not 16-byte aligned'),
            (e.dims(), dict(set_of_block=e.ODD1), EALIGN, 'mlp.set_of_block is not 4-byte aligned'),
            (e.dims(), dict(t0=95), ERANGE, 'steps [95, 103) outside [0, 100)'),
            (e.dims(), dict(t0=-1), ERANGE, 'steps [-1, 7) outside [0, 100)'),
            (e.dims(), dict(k_steps=-1), ERANGE, 'steps [0, -1) outside [0, 100)'),
            (e.dims(tun=dict(vec=2)), {}, EINVAL, 'no central thermal policy rollout kernel at 2 envs per lane: it runs at one env per lane'),
            (e.dims(tun=dict(vec=4)), {}, EINVAL, 'no central thermal policy rollout kernel at 4 envs per lane'),
            (e.dims(tun=dict(nw=8)), {}, EINVAL, NW % (8, 9)),
            (e.dims(tun=dict(nw=10)), {}, EINVAL, NW % (10, 9)),
            (e.dims(n_bldg=16, tun=dict(nw=17)), {}, EINVAL, NW % (17, 16))):
        assert e.call(d, **kw) == code and e.error() == msg, (kw, e.error())
    for name in ('pre', 'dep', 'out', 'act_low', 'act_high'):
        assert e.call(e.dims(), **{name: None}) == ENULL and e.error() == f'mlp.{name} is NULL'
    for name in ('pre', 'dep', 'out', 'net_reset', 'sigma'):
        assert e.call(e.dims(), **{name: e.ODD}) == EALIGN and e.error() == f'mlp.{name} is not 16-byte aligned'
    assert e.call(None) == ENULL and e.error() == 'dims is NULL'
    # which one wins: the coverage refusals come in the order above, all in front of the struct's and the buffers', the envs per lane last
    everything = abi.CLD_F64_MAPS | abi.CLD_KPI | abi.CLD_WRITE_DETAIL | kind(abi.CLR_EV)
    bad = dict(n_hidden=6, null='state')
    assert e.call(e.dims(flags=L | everything, n_bldg=17, env_pitch=128, tun=dict(vec=2)), **bad) == EINVAL and 'CLD_LEAN' in e.error()
    assert e.call(e.dims(flags=everything, n_bldg=17, env_pitch=128, tun=dict(vec=2)), **bad) == EINVAL and 'n_bldg=17 > 16' in e.error()
    assert e.call(e.dims(flags=everything, env_pitch=128, tun=dict(vec=2)), **bad) == EINVAL and 'not CLD_F64_MAPS' in e.error()
    assert e.call(e.dims(flags=everything & ~abi.CLD_F64_MAPS, env_pitch=128, tun=dict(vec=2)), **bad) == EINVAL and 'CLPF_T_ACTION + head' in e.error()
    assert e.call(e.dims(flags=abi.CLD_WRITE_DETAIL | kind(abi.CLR_EV), env_pitch=128, tun=dict(vec=2)), **bad) == EINVAL and 'CLD_WRITE_DETAIL' in e.error()
    assert e.call(e.dims(flags=kind(abi.CLR_EV), env_pitch=128, tun=dict(vec=2)), **bad) == EINVAL and 'CLR_EV' in e.error()
    assert e.call(e.dims(env_pitch=128, tun=dict(vec=2)), **bad) == EINVAL and 'env_pitch=128' in e.error()
    assert e.call(e.dims(tun=dict(vec=2)), **bad) == EINVAL and e.error() == HMSG % 6
    assert e.call(e.dims(tun=dict(vec=2)), null='state') == ENULL and e.error() == 'state is NULL'
    assert e.call(e.dims(tun=dict(vec=2)), t0=95) == ERANGE
    assert e.call(e.dims(tun=dict(vec=4, nw=8))) == EINVAL and '4 envs per lane' in e.error()


def _header_lds_floats(nw, n_bldg, h):
    """The formula as include/citylearn_amd_policy_full_central.h writes it, evaluated from the header's text."""
    text = EXT.header.read_text()
    m = re.search(r'Dynamic LDS per workgroup, in floats.*?\n \*\s+(nw x 4 x 64.*?)\n', text, flags=re.S)
    expr = m.group(1).replace('CLPFCA_MAX_HIDDEN', str(policy.CLPFCA_MAX_HIDDEN)).replace(' x ', ' * ')
    assert re.fullmatch(r'[\w\s*+()]+', expr), expr
    return eval(expr, {'__builtins__': {}}, dict(nw=nw, n_bldg=n_bldg, n_hidden=h))


def test_lds_formula():
    """`_lib.policy_full_central_lds_bytes` against the header's formula and the kernel header's function (nw == n_bldg); the launch opts in above
    64 KiB and no accepted geometry reaches a CU's 160 KiB (the entry still holds it against that, through the shared `check_policy_lds`)."""
    for n_bldg in (1, 2, 9, 16):
        for h in (4, 32, 64):
            assert _lib.policy_full_central_lds_bytes(n_bldg, h) == 4 * _header_lds_floats(n_bldg, n_bldg, h), (n_bldg, h)
    assert _lib.policy_full_central_lds_bytes(16, 64) == 92160 > 64 * 1024 and 92160 < _lib.LDS_PER_CU == 163840
    assert _lib.policy_full_central_lds_bytes(16, 4) == 57600 < 64 * 1024 < _lib.policy_full_central_lds_bytes(16, 32) == 73728
    assert _lib.policy_full_central_lds_bytes(9, 32) == 4 * (9 * 256 + 45 * 64 + 32 * 64 + 160 * 9 + 9 * 288) == 45056
    head, unit = (_lib.CSRC / 'cl_policy_full_central.h').read_text(), (_lib.CSRC / 'cl_policy_full_central.hip').read_text()
    assert ('return (size_t)nw * NQ * 64 + (size_t)CLPF_ND * n_bldg * 64 + (size_t)h * 64 + (size_t)CLPF_ND * h * n_bldg + (size_t)nw * CLPFC_ROW;' in head
            and 'CLPFC_MAX_HIDDEN = 64;' in head and 'CLPFC_HEADS = CLPF_NA * CLPFC_MAX_HIDDEN;' in head and 'CLPFC_ROW = CLPFC_HEADS + 8 * CLPF_NA;' in head
            and 'static_assert(CLPFCA_MAX_HIDDEN == CLPFC_MAX_HIDDEN,' in unit and policy.CLPFCA_MAX_HIDDEN == 64
            and abi.CL_NQ == 4 and (CLPF_ND, CLPF_NA) == (5, 4))
    assert ('check_policy_lds(lds, "central thermal policy", a.nw, 1)' in unit
            and 'CL_POLICY_LAUNCH(cl_rollout_full_policy_central_kernel<P, M, false>)' in unit and '<P, M, true>' not in unit)
    shared = (_lib.CSRC / 'cl_policy_common.h').read_text()
    assert 'if (lds > 64 * 1024) if (hipError_t e = ensure_dynamic_lds(' in shared and 'if (lds > CL_LDS_PER_CU) return fail(' in shared


# ---- 3. the packer --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('name', ['g2020_cz1', 't2', 't2_outage'])
def test_packed_layers_equal_the_unsplit_mlp(name, normalize):
    """`pre + dep x` and `out` rebuilt on the host in float64 from the float32 tables against `actions_host` (the unsplit MLP in float64) on
    central-agent vectors with random state, two parameter sets with `set_of_block`.  Every packed number carries one float32 rounding (2^-24
    relative); through tanh (slope <= 1) the action moves by at most half x 2^-24 x (the l1 mass of each layer's terms, propagated), taken with
    a factor 2 -- tests/test_policy_central_host.py's bound over five terms and four heads.  No building of the fixtures has a heating tank: the
    heat-storage rows of `dep` are 0; a building without DHW storage has a zero DHW row and no DHW head."""
    spec = thermal_district(name)
    tab = spec.episode_tables(0)
    layout = central_layout(spec, normalize)
    B, N, H = len(spec.buildings), layout.n_cols, 32
    pol = make_central_storage_policy(layout, H, n_sets=2, seed=3)
    pt = pol.pack(layout, tab, set_of_block=[1, 0])
    assert isinstance(pt, policy.CentralStoragePolicyTables) and (pt.n_hidden, pt.n_sets, pt.n_bldg, pt.n_rows) == (H, 2, B, tab.n_steps)
    assert tuple(pt.pre.shape) == (2, tab.n_steps, H) and tuple(pt.dep.shape) == (2, H // 4, B, CLPF_ND, 4) and tuple(pt.out.shape) == (2, B, CLPF_NA, H + 1)
    assert tuple(pt.net_reset.shape) == (tab.n_steps, B) and pt.low_bldg.shape == pt.high_bldg.shape == pt.sigma_bldg.shape == pt.cols.shape == (B, CLPF_NA)
    assert pt.set_of_block.tolist() == [1, 0] and np.array_equal(pt.cols, policy.head_columns(tab)) and pt.n_device_cols == 0
    st = pt.struct(5)
    assert (st.n_hidden, st.n_sets, st.n_device_cols, st.reserved, st.seed) == (H, 2, 0, 0, 5) and st.pre == pt.pre.data_ptr() and st.dep == pt.dep.data_ptr()
    cobs = CentralStorageObservations(layout, tab)
    if name == 'g2020_cz1':
        assert (N, int(sum(t.sum() for t in cobs.is_term))) == ((88, 34) if normalize else (N, 34))
    terms = pt.dep_terms()
    assert tuple(terms.shape) == (2, B, CLPF_ND, H) and not terms[:, :, policy.CLPF_D_HS].any() and not cobs.is_term[policy.CLPF_D_HS].any()
    bflags = np.ascontiguousarray(tab.params).view(np.uint32)[:, abi.CLP_FLAGS]
    for b in range(B):
        has_ds = bool(bflags[b] & abi.CLF_DHW_STO)
        assert bool(terms[:, b, policy.CLPF_D_DS].any()) == has_ds == (pt.cols[b, policy.CLPF_A_DS] >= 0)
        assert terms[:, b, policy.CLPF_D_SOC].any() and terms[:, b, policy.CLPF_D_CS].any() and terms[:, b, policy.CLPF_D_NET].any()
    if name.startswith('t2'):
        assert pt.cols[0, policy.CLPF_A_DS] >= 0 and pt.cols[1, policy.CLPF_A_DS] < 0
    rng = np.random.RandomState(5)
    E, S, u = 5, policy.ACT_SCALE, 2.0 ** -24
    for s in range(2):
        pre, dep, out = pt.pre[s].numpy().astype(np.float64), terms[s].numpy().astype(np.float64), pt.out[s].numpy().astype(np.float64)
        _, _, w2, b2 = (v[s] for v in pol._full(B))
        assert np.allclose(out[:, :, :H], w2, rtol=2 * u, atol=0) and np.allclose(out[:, :, H], b2, rtol=2 * u, atol=0)
        # dep in the kernel's order: group g, building b, term d, four units
        raw, g = pt.dep[s].numpy(), H // 4 - 1
        for d in range(CLPF_ND):
            assert np.array_equal(raw[g, B - 1, d], terms[s].numpy()[B - 1, d, 4 * g:4 * g + 4])
        for r in (1, 9, 100):
            planes = [rng.uniform(0, 1, size=(B, E)) for _ in range(4)] + [rng.uniform(-3, 6, size=(B, E))]
            parts = [dep[None, :, d] * planes[d].T[:, :, None] for d in range(CLPF_ND)]                         # [E, B, H] each, scaled
            z1 = pre[r][None] + sum(p.sum(axis=1) for p in parts)
            m1 = np.abs(pre[r][None]) + sum(np.abs(p).sum(axis=1) for p in parts)
            h = np.tanh(z1 / S)
            e1 = 2 * u * m1 / abs(S)
            z2 = out[None, :, :, H] + np.einsum('baj,ej->eba', out[:, :, :H], h)
            e2 = (2 * u * (np.abs(out[None, :, :, H]) + np.einsum('baj,ej->eba', np.abs(out[:, :, :H]), np.abs(h)))
                  + np.einsum('baj,ej->eba', np.abs(out[:, :, :H]), e1))
            half = 0.5 * (pt.high_bldg - pt.low_bldg)
            got = np.clip(0.5 * (pt.high_bldg + pt.low_bldg) + half * np.tanh(z2), pt.low_bldg, pt.high_bldg)
            # (the planes of a storage a building lacks are 0 in the kernel; here the packer's zero rows make them irrelevant)
            want = pol.actions_host(cobs.at(r, *planes), pt, set_index=s)
            present = pt.cols >= 0
            assert want.shape == (E, B, CLPF_NA) and want.dtype == np.float64 and not want[:, ~present].any()
            assert np.all(np.abs(got - want)[:, present] <= (half * e2)[:, present] + 1e-15), float(np.abs(got - want)[:, present].max())
            assert np.abs(got - want)[:, present].max() < 1e-6
    # the reset observation's net is what net_reset reproduces through dep
    net_cols = np.nonzero(cobs.is_term[policy.CLPF_D_NET])[0]
    x0 = cobs.at(7, reset=True, E=1)[0]
    back = cobs.obs.table[8][net_cols] + pt.net_reset[7].numpy().astype(np.float64)[cobs.bldg[net_cols]] * cobs.scale[net_cols]
    assert np.allclose(back, x0[net_cols], rtol=1e-6, atol=1e-6)


def test_packer_surface():
    """The constructor's and the packer's `ValueError`s, sigma as a scalar or per column, `update` / `invalidate` / `version`."""
    spec = thermal_district('g2020_cz1')
    tab = spec.episode_tables(0)
    layout = central_layout(spec)
    N, B = layout.n_cols, 9
    rng = np.random.RandomState(1)
    pol = CentralStorageMLPPolicy(rng.uniform(-0.1, 0.1, (1, 8, N)), rng.uniform(-0.5, 0.5, (3, 8)), rng.uniform(-0.3, 0.3, (1, B, 4, 8)), np.zeros((1, B, 4)),
                                  sigma=0.1)
    assert (pol.n_sets, pol.n_hidden, pol.n_obs, pol.n_bldg, pol.version) == (3, 8, N, B, 0)
    pt = pol.pack(layout, tab, set_of_block=[2, 0, 1])
    assert pt.version == 0 and pt.n_sets == 3 and pt.set_of_block.tolist() == [2, 0, 1]
    assert np.all(pt.sigma_bldg[pt.cols >= 0] == 0.1) and not pt.sigma_bldg[pt.cols < 0].any() and tuple(pt.sigma.shape) == (25,)
    assert bool((pt.out == pt.out[:1]).all()) and bool((pt.dep == pt.dep[:1]).all()) and not bool((pt.pre[0] == pt.pre[1]).all())
    cobs = CentralStorageObservations(layout, tab)
    x = cobs.at(3, *[np.full((B, 2), 0.5)] * 4, np.zeros((B, 2)))
    a0 = pol.actions_host(x, pt)
    assert a0.shape == (2, B, 4) and not np.array_equal(pol.actions_host(x, pt, set_index=1), a0)
    z = np.ones((2, B, 4))
    assert np.allclose(pol.actions_host(x, pt, noise=z), np.where(pt.cols >= 0, np.clip(a0 + 0.1, pt.low_bldg, pt.high_bldg), 0.0))
    per_col = CentralStorageMLPPolicy(pol.w1, pol.b1, pol.w2, pol.b2, sigma=np.linspace(0, 0.24, 25))
    ppt = per_col.pack(layout, tab)
    assert np.allclose(ppt.sigma_bldg[ppt.cols >= 0], np.linspace(0, 0.24, 25)[ppt.cols[ppt.cols >= 0]])
    with pytest.raises(ValueError, match='sigma: a non-negative scalar'):
        CentralStorageMLPPolicy(pol.w1, pol.b1, pol.w2, pol.b2, sigma=[0.1, 0.2]).pack(layout, tab)
    mid = 0.5 * (pt.high_bldg + pt.low_bldg)
    pol.update(w2=-pol.w2)
    assert pol.version == 1 and pol.pack(layout, tab).version == 1
    assert np.allclose((pol.actions_host(x, pt) - mid)[:, pt.cols >= 0], -(a0 - mid)[:, pt.cols >= 0])          # (b2 = 0: the heads are odd in w2)
    pol.invalidate()
    assert pol.version == 2
    with pytest.raises(ValueError, match='w2: shape'):
        pol.update(w2=np.zeros((1, B, 4, 4)))
    with pytest.raises(ValueError, match='set_of_block outside'):
        pol.pack(layout, tab, set_of_block=[3])
    zz = np.zeros
    for shapes, msg in ((((1, 1, 8, N), (1, 8), (1, B, 4, 8), (1, B, 4)), 'w1 .n_sets, H, n_cols.'),
                        (((1, 8, N), (1, 8), (1, B, 8), (1, B)), 'w2 .n_sets, n_bldg, 4, H.'),
                        (((1, 6, N), (1, 6), (1, B, 4, 6), (1, B, 4)), 'H=6'),
                        (((1, 68, N), (1, 68), (1, B, 4, 68), (1, B, 4)), 'H=68'),
                        (((1, 8, N), (1, 4), (1, B, 4, 8), (1, B, 4)), 'about H'),
                        (((1, 8, N), (1, 8), (1, B, 4, 4), (1, B, 4)), 'about H'),
                        (((1, 8, N), (1, 8), (1, B, 3, 8), (1, B, 3)), 'do not have 4 heads'),
                        (((1, 8, N), (1, 8), (1, B, 4, 8), (1, B - 1, 4)), 'about n_bldg')):
        with pytest.raises(ValueError, match=msg):
            CentralStorageMLPPolicy(*[zz(s) for s in shapes])
    assert CentralStorageMLPPolicy(zz((1, 64, N)), zz((1, 64)), zz((1, B, 4, 64)), zz((1, B, 4))).pack(layout, tab).n_hidden == 64
    with pytest.raises(ValueError, match='do not broadcast to 3 sets'):
        CentralStorageMLPPolicy(zz((2, 8, N)), zz((3, 8)), zz((1, B, 4, 8)), zz((1, B, 4))).pack(layout, tab)
    # the layout must be the central agent's, of this length, over this many buildings
    with pytest.raises(ValueError, match='central_agent=False'):
        pol.pack(ObservationLayout(spec, 'current', True, central_agent=False), tab)
    with pytest.raises(ValueError, match='central_agent=False'):
        pol.torch_policy(ObservationLayout(spec, 'current', True, central_agent=False), tab, 'cpu')
    with pytest.raises(ValueError, match=f'w1 takes {N} observations, the central-agent vector has'):
        pol.pack(central_layout(spec, normalize=False), tab)
    spec2 = thermal_district('t2')
    lay2 = central_layout(spec2)
    with pytest.raises(ValueError, match='heads for 9 buildings, the district has 2'):
        CentralStorageMLPPolicy(zz((1, 8, lay2.n_cols)), zz((1, 8)), zz((1, B, 4, 8)), zz((1, B, 4))).pack(lay2, spec2.episode_tables(0))
    with pytest.raises(ValueError, match='observation_mode="reference"'):
        lay_ref = ObservationLayout(spec, 'reference', True, central_agent=True)
        CentralStorageMLPPolicy(zz((1, 8, lay_ref.n_cols)), zz((1, 8)), zz((1, B, 4, 8)), zz((1, B, 4))).pack(lay_ref, tab)


def test_packer_refuses_the_lstm_stage_and_device_actions():
    """g2023_p2, as tests/test_policy_full_host.py::test_packer_refusals: the indoor temperature is fed by the LSTM stage (SRC_TEMP) and the
    buildings have device actions -- `StorageMLPPolicy.pack`'s messages, the observation first; with the observation out of the way, the device
    action."""
    spec = golden('g2023_p2').spec()
    tab = spec.episode_tables(0)
    layout = central_layout(spec)
    B = len(spec.buildings)
    pol = CentralStorageMLPPolicy(np.zeros((1, 8, layout.n_cols)), np.zeros((1, 8)), np.zeros((1, B, 4, 8)), np.zeros((1, B, 4)))
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
    pol = make_central_storage_policy(layout, 16, seed=2)
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


# ---- 4. conditioning of the closed loop -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H', [4, 32, 64])
@pytest.mark.parametrize('name', ['g2020_cz1', 't1', 't2', 't16'])
def test_closed_loop_is_well_conditioned(name, H):
    """tests/test_policy_central_host.py::test_closed_loop_is_well_conditioned for the central thermal test policies of the free-running GPU test,
    before any GPU run: the CPU oracle stepped K = 48 from reset with `actions_host` in float64, against the same loop with every action rounded
    through float32 and moved by the GPU teacher-forced tolerance -- 4 x the worst deviation of a float32 torch evaluation on this trajectory's
    own observations: soc, cs, ds and net must stay within 0.1 x (1e-4 + 1e-4 |ref|), while the policy does something.  Fixes
    policy_full_central_util.W1_SCALE / W2_SCALE (readings there)."""
    spec = thermal_district(name)
    K, E = 48, 4
    tab = spec.episode_tables(0)
    layout = central_layout(spec)
    pol = make_central_storage_policy(layout, H, seed=H)
    pt = pol.pack(layout, tab)
    ref = host_closed_loop(spec, tab, layout, pol, pt, K, E)
    cobs = CentralStorageObservations(layout, tab)
    x = np.stack([cobs.at(t, *[ref[k][t - 1] for k in ('soc', 'cs', 'hs', 'ds', 'net')]) for t in range(1, K)])
    tol = 4.0 * f32_torch_deviation(pol, x, pt)
    got = host_closed_loop(spec, tab, layout, pol, pt, K, E, perturb=tol, round_f32=True)
    assert 0 < tol < 1e-5, tol
    act = ref['action'].transpose(0, 3, 2, 1)[:, :, pt.cols >= 0]
    # a policy that does something: many heads span a range; t1 / t2 have ONE seeded draw of three to five heads per shape, where all the
    # closed loop needs is actions that are not 0 and move with the observations
    assert (np.abs(act).max() > 0.05 and np.ptp(act) > 0.05) if name in ('g2020_cz1', 't16') else (np.abs(act).max() > 1e-2 and np.ptp(act) > 1e-2)
    # (no fixture has a heating tank; a cooling tank fills where some head asks for it -- among many buildings one always does, the one or two
    # cooling heads of t1 / t2 may all ask an empty tank to discharge)
    assert not ref['hs'].any() and (np.abs(ref['cs']).max() > 0.05 or name in ('t1', 't2'))
    for k in ('soc', 'cs', 'ds', 'net'):
        err = float((np.abs(got[k] - ref[k]) / (1e-4 + 1e-4 * np.abs(ref[k]))).max())
        print(f'{name} H={H} {k}: worst {err:.4f} x (1e-4 + 1e-4 |ref|), action tolerance {tol:.3e}, |action| max {np.abs(act).max():.3f}, '
              f'range {np.ptp(act):.3f}')
        assert err < 0.1, (name, k, err)


# ---- 5. generated code ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def central_unit(tmp_path_factory):
    src, = EXT.sources
    return _asm(src, [], tmp_path_factory)


def test_central_thermal_kernel_resources(central_unit):
    """Every instantiation of cl_rollout_full_policy_central_kernel<PREC, MARL> -- the fp32 map and the float64 chain, with and without the MARL
    exchange: no scratch memory and at most 128 registers, a 1024-thread workgroup's limit.  The unit holds no other rollout or step kernel."""
    kernels, meta = central_unit
    names = [k for k in kernels if 'cl_rollout_full_policy_central_kernel' in k]
    by = {}
    for k in names:
        m = re.search(r'cl_rollout_full_policy_central_kernelILi(\d)ELb(\d)ELb0EE', k)
        by[(int(m.group(1)), bool(int(m.group(2))))] = k
    assert sorted(by) == [(0, False), (0, True), (2, False), (2, True)] and len(names) == 4
    assert not [k for k in kernels if k not in names and ('cl_rollout' in k or 'cl_step' in k)]
    for key, k in by.items():
        assert meta[k]['private_seg_size'] == 0, k
        assert meta[k]['num_vgpr'] <= 128, (k, meta[k])
