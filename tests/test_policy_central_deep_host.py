"""The closed-loop rollout under a CENTRAL-AGENT policy with TWO hidden layers (`clpcd_rollout_mlp_f32`, kernel
`cl_rollout_policy_central_kernel<PREC, DEEP = true>` of csrc/cl_policy_central.h, library ``libcitylearn_amd_policy_central_deep.so``) as far as it can be
checked without a GPU: the library's symbol list and struct, every refusal of the host entry (before any HIP call), the LDS formula, the packer
against the unsplit MLP in float64, the conditioning of the closed loop the GPU tests run (tests/test_gpu_policy_central_deep_rollout.py), and
the resource figures of every instantiation."""
import ctypes
import re

import numpy as np
import pytest

from golden_util import golden
from citylearn_amd import _lib, abi, policy
from citylearn_amd.observations import ObservationLayout
from citylearn_amd.policy import CentralMLPPolicy, DeepCentralMLPPolicy
from district_util import HET_UNDRIVEN, district
from policy_central_deep_util import (CentralObservations, DeepHostEntry, central_layout, f32_torch_deviation, host_closed_loop,
                                      make_deep_central_policy)
from policy_util import exports
from test_isa_guards import _asm

EXT = _lib.POLICY_CENTRAL_DEEP


@pytest.fixture(scope='module')
def entry():
    return DeepHostEntry(EXT, n_bldg=17, flags=abi.CLD_LEAN)


# ---- 1. the library -------------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header(entry):
    assert EXT.symbols == ['clpcd_abi_version', 'clpcd_core_abi_version', 'clpcd_last_error', 'clpcd_rollout_mlp_f32']
    assert exports(EXT.path) == EXT.symbols
    assert entry.lib.clpcd_abi_version() == EXT.abi_version == 1 and entry.lib.clpcd_core_abi_version() == abi.CL_ABI_VERSION
    assert policy.CENTRAL_DEEP_CONSTANTS == {'CLPCD_ABI_VERSION': 1, 'CLPCD_MAX_HIDDEN': 64, 'CLPCD_MAX_BLDG': 32}
    (src, flags), = EXT.sources
    assert flags == ['-fno-slp-vectorize'] and src.name == 'cl_policy_central_deep.hip'
    assert EXT.path.name == 'libcitylearn_amd_policy_central_deep.so'
    # the kernel source is the central pair's one header, which the two central units include and nobody else
    users = sorted(p.name for p in _lib.CSRC.glob('*.hip') if '#include "cl_policy_central.h"' in p.read_text())
    assert users == ['cl_policy_central.hip', 'cl_policy_central_deep.hip'] and not (_lib.CSRC / 'cl_policy_central_deep.h').exists()


def test_struct_is_the_deep_policy_struct():
    """`clpcd_mlp` is `clpca_mlp`'s fields in order, then `n_hidden2, reserved2, l2` -- the extension `clpd_mlp` makes of `clpol_mlp`:
    `_lib.PolicyDeepMLP` and the shared host checks serve it."""
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
    fields = fields_of(EXT.header, 'clpcd_mlp')
    central = fields_of(_lib.POLICY_CENTRAL.header, 'clpca_mlp')
    assert fields == central + ['n_hidden2', 'reserved2', 'l2']
    assert [f for f, _ in _lib.PolicyDeepMLP._fields_] == fields and EXT.mlp is _lib.PolicyDeepMLP and ctypes.sizeof(_lib.PolicyDeepMLP) == 104


def test_the_extension_tuples():
    """The new tuple beside the unchanged ones, the build function, and the kind of its own."""
    assert _lib.CENTRAL_DEEP_EXTENSIONS == (EXT,) and _lib.CENTRAL_EXTENSIONS == (_lib.POLICY_CENTRAL,)
    assert _lib.EXTENSIONS == (_lib.POLICY, _lib.POLICY_KPI, _lib.POLICY_FULL, _lib.POLICY_FULL_KPI)
    assert _lib.ALL_EXTENSIONS == _lib.EXTENSIONS + (_lib.POLICY_FULL_CHUNK,) and _lib.CHUNK_KPI_EXTENSIONS == (_lib.POLICY_FULL_CHUNK_KPI,)
    assert _lib.LEAN_CHUNK_EXTENSIONS == (_lib.POLICY_CHUNK,) and _lib.DEEP_EXTENSIONS == (_lib.POLICY_DEEP,)
    assert _lib.DEEP_THERMAL_EXTENSIONS == (_lib.POLICY_FULL_DEEP,)
    every = (_lib.ALL_EXTENSIONS + _lib.CHUNK_KPI_EXTENSIONS + _lib.LEAN_CHUNK_EXTENSIONS + _lib.DEEP_EXTENSIONS + _lib.DEEP_THERMAL_EXTENSIONS
             + _lib.CENTRAL_EXTENSIONS)
    assert len(every) == 10 and EXT not in every and len({e.path for e in every + _lib.CENTRAL_DEEP_EXTENSIONS}) == 11
    assert len({e.prefix for e in every + _lib.CENTRAL_DEEP_EXTENSIONS}) == 11          # (with the main library: eleven product libraries)
    import inspect
    import __graft_entry__
    src = inspect.getsource(__graft_entry__.build)
    assert '_lib.CENTRAL_DEEP_EXTENSIONS' in src and src.index('_lib.CENTRAL_EXTENSIONS') < src.index('_lib.CENTRAL_DEEP_EXTENSIONS')
    kind = DeepCentralMLPPolicy.kind
    assert kind.ext is EXT and kind.ext_kpi is None and kind.ext_chunk is None and kind.ext_chunk_kpi is None and kind.ext_chunk_pair is None
    assert kind.one_row_max == 32 and kind.n_planes == policy.CLPOL_NT and kind.no_kpi_error is NotImplementedError and kind.central
    assert kind.tables is policy.DeepCentralPolicyTables and kind.struct is _lib.PolicyDeepMLP and kind.max_hidden == 64
    assert policy.DeepCentralPolicyTables.kind is kind and policy.CentralPolicyTables.kind is CentralMLPPolicy.kind and CentralMLPPolicy.kind is not kind
    assert CentralMLPPolicy.kind.ext is _lib.POLICY_CENTRAL and policy.DeepPolicyTables.kind is policy.DeepMLPPolicy.kind
    # both classes split the first layer with ONE function
    assert DeepCentralMLPPolicy._pack_front is CentralMLPPolicy._pack_front


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_before_any_hip_call(entry):
    """Every refusal of the entry with its code and whole message, from a call on host memory: a call that reached a launch would not return one
    of these codes."""
    e, L = entry, abi.CLD_LEAN
    EINVAL, ENULL, EALIGN, ERANGE = abi.CL_EINVAL, abi.CL_ENULL, abi.CL_EALIGN, abi.CL_ERANGE
    P = 'clpcd_rollout_mlp_f32: '
    kind = lambda k: L | (k << abi.CLD_REWARD_SHIFT)
    HMSG = 'n_hidden=%d: the policy kernel takes 4, 8, .. 64 hidden units'
    H2MSG = 'n_hidden2=%d: the deep central policy kernel takes 4, 8, .. 64 units in its second hidden layer'
    RMSG = 'clpcd_mlp.flags / .reserved / .reserved2 must be 0'
    for d, kw, code, msg in (
            (e.dims(flags=0), {}, EINVAL, P + 'only battery + PV districts (CLD_LEAN); a thermal / outage district has no central-agent rollout kernel'),
            (e.dims(n_bldg=33), {}, EINVAL, P + 'n_bldg=33 > 32: the central-agent policy kernel holds the whole district in one workgroup (two buildings '
                                                'per wave); its hidden layers cannot be cut into building chunks'),
            (e.dims(flags=L | abi.CLD_F64_MAPS), {}, EINVAL, P + 'the battery map in fp32 or as the float64 chain (CLD_F64_CHAIN), not CLD_F64_MAPS'),
            (e.dims(flags=L | abi.CLD_KPI), {}, EINVAL, P + 'no streaming KPIs (CLD_KPI) inside this kernel -- record traj and replay CLPOL_T_ACTION '
                                                            'through cl_rollout_seq_f32'),
            (e.dims(flags=L | abi.CLD_WRITE_DETAIL), {}, EINVAL, P + 'not with the detail planes (CLD_WRITE_DETAIL)'),
            (e.dims(flags=kind(abi.CLR_EV)), {}, EINVAL, P + 'reward kind CLR_EV needs the flexible-load tables'),
            (e.dims(env_pitch=128), {}, EINVAL, P + 'env_pitch=128 != n_env=64 is not implemented for this call'),
            (e.dims(), dict(n_hidden=0), EINVAL, HMSG % 0),
            (e.dims(), dict(n_hidden=6), EINVAL, HMSG % 6),
            (e.dims(), dict(n_hidden=68), EINVAL, HMSG % 68),
            (e.dims(), dict(n_sets=0), EINVAL, 'n_sets=0: at least one parameter set'),
            (e.dims(), dict(n_hidden2=0), EINVAL, H2MSG % 0),
            (e.dims(), dict(n_hidden2=6), EINVAL, H2MSG % 6),
            (e.dims(), dict(n_hidden2=68), EINVAL, H2MSG % 68),
            (e.dims(), dict(flags=1), EINVAL, RMSG),
            (e.dims(), dict(reserved=1), EINVAL, RMSG),
            (e.dims(), dict(reserved2=1), EINVAL, RMSG),
            (e.dims(), dict(null='state'), ENULL, 'state is NULL'),
            (e.dims(), dict(null='params'), ENULL, 'params is NULL'),
            (e.dims(), dict(odd='traj'), EALIGN, 'traj is not 16-byte aligned'),
            (e.dims(), dict(odd='ret_env'), EALIGN, 'ret_env is not 16-byte aligned'),
            (e.dims(), dict(set_of_block=e.ODD1), EALIGN, 'mlp.set_of_block is not 4-byte aligned'),
            (e.dims(), dict(t0=95), ERANGE, 'steps [95, 103) outside [0, 100)'),
            (e.dims(), dict(t0=-1), ERANGE, 'steps [-1, 7) outside [0, 100)'),
            (e.dims(), dict(k_steps=-1), ERANGE, 'steps [0, -1) outside [0, 100)'),
            (e.dims(), dict(l2=None), ENULL, 'mlp.l2 is NULL'),
            (e.dims(), dict(l2=e.ODD), EALIGN, 'mlp.l2 is not 16-byte aligned'),
            (e.dims(tun=dict(vec=2)), {}, EINVAL, 'no deep central policy rollout kernel at 2 envs per lane: it runs at one env per lane'),
            (e.dims(tun=dict(vec=4)), {}, EINVAL, 'no deep central policy rollout kernel at 4 envs per lane'),
            (e.dims(tun=dict(nw=8)), {}, EINVAL, 'bad nw 8'),
            (e.dims(tun=dict(nw=17)), {}, EINVAL, 'bad nw 17'),
            (e.dims(n_bldg=5, tun=dict(nw=8)), {}, EINVAL, 'bad nw 8')):
        assert e.call(d, **kw) == code and e.error() == msg, (kw, e.error())
    for name in ('pre', 'dep', 'out', 'act_low', 'act_high'):
        assert e.call(e.dims(), **{name: None}) == ENULL and e.error() == f'mlp.{name} is NULL'
    for name in ('pre', 'dep', 'out', 'net_reset', 'sigma'):
        assert e.call(e.dims(), **{name: e.ODD}) == EALIGN and e.error() == f'mlp.{name} is not 16-byte aligned'
    assert e.call(None) == ENULL and e.error() == 'dims is NULL'
    # which one wins: the coverage refusals come in the order above, all in front of the struct's and the buffers'; H1 in front of H2
    assert e.call(e.dims(flags=abi.CLD_KPI, n_bldg=33), n_hidden=6, null='state') == EINVAL and 'CLD_LEAN' in e.error()
    assert e.call(e.dims(n_bldg=33, flags=L | abi.CLD_KPI), n_hidden=6) == EINVAL and 'n_bldg=33 > 32' in e.error()
    assert e.call(e.dims(tun=dict(vec=2)), n_hidden=6, n_hidden2=6) == EINVAL and e.error() == HMSG % 6
    assert e.call(e.dims(tun=dict(vec=2)), n_hidden2=6, l2=None) == EINVAL and e.error() == H2MSG % 6
    # every accepted width of either layer gets past the struct's checks (it stops at the step range here)
    for h1, h2 in ((4, 64), (64, 4), (64, 64), (24, 40)):
        assert e.call(e.dims(), n_hidden=h1, n_hidden2=h2, t0=95) == ERANGE


def _header_lds_floats(nw, n_bldg, h1, h2):
    """The formula as include/citylearn_amd_policy_central_deep.h writes it, evaluated from the header's text."""
    text = EXT.header.read_text()
    m = re.search(r'Dynamic LDS per workgroup, in floats.*?\n \*\s+(nw x 4 x 64.*?)\n', text, flags=re.S)
    expr = m.group(1).replace('CLPCD_MAX_HIDDEN', str(policy.CLPCD_MAX_HIDDEN)).replace(' x ', ' * ')
    assert re.fullmatch(r'[\w\s*+()]+', expr), expr
    return eval(expr, {'__builtins__': {}}, dict(nw=nw, n_bldg=n_bldg, n_hidden=h1, n_hidden2=h2))


def test_lds_formula():
    """`_lib.policy_central_deep_lds_bytes` against the header's formula and the kernel header's function; the launch opts in above 64 KiB and no
    accepted geometry reaches a CU's 160 KiB (the entry still holds it against that, through the shared `check_policy_lds`)."""
    for n_bldg in (1, 2, 17, 31, 32):
        for nw in range((n_bldg + 1) // 2, min(n_bldg, 16) + 1):
            for h1, h2 in ((4, 4), (4, 64), (64, 4), (24, 40), (64, 64)):
                assert _lib.policy_central_deep_lds_bytes(nw, n_bldg, h1, h2) == 4 * _header_lds_floats(nw, n_bldg, h1, h2), (nw, n_bldg, h1, h2)
                # the one-hidden-layer kernel's regions + Hh2 + the staged l2
                assert (_lib.policy_central_deep_lds_bytes(nw, n_bldg, h1, h2)
                        == _lib.policy_central_lds_bytes(nw, n_bldg, h1) + 4 * (h2 * 64 + (h1 + 1) * h2))
    assert _lib.policy_central_deep_lds_bytes(16, 32, 64, 64) == 107776 > 64 * 1024 and 107776 < _lib.LDS_PER_CU == 163840
    assert _lib.policy_central_deep_lds_bytes(9, 17, 32, 16) == 4 * (9 * 256 + 34 * 64 + 32 * 64 + 16 * 64 + 64 * 17 + 33 * 16 + 18 * 72) == 41856
    head, unit = (_lib.CSRC / 'cl_policy_central.h').read_text(), (_lib.CSRC / 'cl_policy_central_deep.hip').read_text()
    assert ('return (size_t)nw * NQ * 64 + (size_t)2 * n_bldg * 64 + (size_t)h1 * 64 + (size_t)h2 * 64 + (size_t)2 * h1 * n_bldg + (size_t)(h1 + 1) * h2\n'
            '           + (size_t)nw * 2 * CLPC_ROW;' in head and 'CLPC_ROW = CLPC_MAX_HIDDEN + 8;' in head and 'CLPC_MAX_HIDDEN = 64;' in head
            and abi.CL_NQ == 4)
    assert 'static_assert(CLPCD_MAX_HIDDEN == CLPC_MAX_HIDDEN' in unit and policy.CLPCD_MAX_HIDDEN == 64
    assert 'check_policy_lds(lds, "deep central policy", nw, 1)' in unit and 'CL_POLICY_LAUNCH(cl_rollout_policy_central_kernel<0, true>)' in unit
    shared = (_lib.CSRC / 'cl_policy_common.h').read_text()
    assert 'if (lds > 64 * 1024) if (hipError_t e = ensure_dynamic_lds(' in shared and 'if (lds > CL_LDS_PER_CU) return fail(' in shared


# ---- 3. the packer --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('H1,H2', [(4, 64), (64, 4), (24, 40)])
@pytest.mark.parametrize('name', ['g2022_all', 'het17'])
def test_packed_layers_equal_the_unsplit_mlp(name, H1, H2, normalize):
    """`pre + dep x`, `l2` and `out` rebuilt on the host in float64 from the float32 tables against `actions_host` (the unsplit MLP in float64)
    on central-agent vectors with random state.  The tolerance is tests/test_policy_central_host.py's with one layer more, as
    tests/test_policy_deep_host.py carries it: every packed number has one float32 rounding (2^-24 relative); through tanh (slope <= 1) the
    action moves by at most half x 2^-24 x (the l1 mass of each layer's terms, propagated), taken with a factor 2.  H1 != H2 throughout: a
    swapped axis of l2 or out does not pass.  The first layer is bit for bit what `CentralMLPPolicy.pack` makes of the same W1 / b1."""
    spec = district(name)
    tab = spec.episode_tables(0)
    layout = central_layout(spec, normalize)
    B = len(spec.buildings)
    pol = make_deep_central_policy(layout, H1, H2, n_sets=2, seed=3, mid_scale=1.0)
    pt = pol.pack(layout, tab)
    assert isinstance(pt, policy.DeepCentralPolicyTables) and (pt.n_hidden, pt.n_hidden2, pt.n_sets, pt.n_bldg, pt.n_rows) == (H1, H2, 2, B, tab.n_steps)
    assert tuple(pt.pre.shape) == (2, tab.n_steps, H1) and tuple(pt.dep.shape) == (2, H1 // 4, B, 2, 4)
    assert tuple(pt.l2.shape) == (2, H1 + 1, H2) and tuple(pt.out.shape) == (2, B, H2 + 1) and pt.l2.is_contiguous() and pt.out.is_contiguous()
    assert tuple(pt.net_reset.shape) == (tab.n_steps, B) and pt.cols is pt.es_cols and pt.low_bldg.shape == pt.high_bldg.shape == pt.sigma_bldg.shape == (B,)
    st = pt.struct(5)
    assert (st.n_hidden, st.n_sets, st.flags, st.reserved, st.seed, st.n_hidden2, st.reserved2) == (H1, 2, 0, 0, 5, H2, 0)
    assert st.pre == pt.pre.data_ptr() and st.dep == pt.dep.data_ptr() and st.l2 == pt.l2.data_ptr() and st.out == pt.out.data_ptr()
    one = CentralMLPPolicy(pol.w1, pol.b1, np.zeros((1, B, H1)), np.zeros((1, B))).pack(layout, tab)
    assert np.array_equal(one.pre.numpy(), pt.pre.numpy()) and np.array_equal(one.dep.numpy(), pt.dep.numpy())
    assert np.array_equal(one.net_reset.numpy(), pt.net_reset.numpy()) and np.array_equal(one.es_cols, pt.es_cols)
    cobs = CentralObservations(layout, tab)
    rng = np.random.RandomState(5)
    E, S, u = 5, policy.ACT_SCALE, 2.0 ** -24
    terms = pt.dep_terms()
    for s in range(2):
        pre, dep = pt.pre[s].numpy().astype(np.float64), terms[s].numpy().astype(np.float64)
        l2, out = pt.l2[s].numpy().astype(np.float64), pt.out[s].numpy().astype(np.float64)
        _, _, w2, b2, w3, b3 = (v[s] for v in pol._full(B))
        assert np.allclose(l2[:H1].T, S * w2, rtol=2 * u, atol=0) and np.allclose(l2[H1], S * b2, rtol=2 * u, atol=0)
        assert np.allclose(out[:, :H2], w3, rtol=2 * u, atol=0) and np.allclose(out[:, H2], b3, rtol=2 * u, atol=0)
        for r in (1, 9, 100):
            soc, net = rng.uniform(0, 1, size=(B, E)), rng.uniform(-3, 6, size=(B, E))
            parts = dep[None, :, 0] * soc.T[:, :, None], dep[None, :, 1] * net.T[:, :, None]                     # [E, B, H1] each, scaled
            z1 = pre[r][None] + parts[0].sum(axis=1) + parts[1].sum(axis=1)
            m1 = np.abs(pre[r][None]) + np.abs(parts[0]).sum(axis=1) + np.abs(parts[1]).sum(axis=1)
            h1 = np.tanh(z1 / S)
            e1 = 2 * u * m1 / abs(S)
            z2 = l2[None, H1] + np.einsum('ji,ej->ei', l2[:H1], h1)                                               # [E, H2], scaled
            m2 = np.abs(l2[None, H1]) + np.einsum('ji,ej->ei', np.abs(l2[:H1]), np.abs(h1))
            e2 = (2 * u * m2 + np.einsum('ji,ej->ei', np.abs(l2[:H1]), e1)) / abs(S)
            h2 = np.tanh(z2 / S)
            z3 = out[None, :, H2] + np.einsum('bi,ei->eb', out[:, :H2], h2)
            e3 = 2 * u * (np.abs(out[None, :, H2]) + np.einsum('bi,ei->eb', np.abs(out[:, :H2]), np.abs(h2))) + np.einsum('bi,ei->eb', np.abs(out[:, :H2]), e2)
            half = 0.5 * (pt.high_bldg - pt.low_bldg)
            got = np.clip(0.5 * (pt.high_bldg + pt.low_bldg) + half * np.tanh(z3), pt.low_bldg, pt.high_bldg)
            want = pol.actions_host(cobs.at(r, soc, net), tables=pt, set_index=s)
            driven = pt.es_cols >= 0
            assert want.shape == (E, B) and want.dtype == np.float64
            assert np.all(np.abs(got - want)[:, driven] <= (half * e3)[:, driven] + 1e-15), float(np.abs(got - want)[:, driven].max())
            assert np.abs(got - want)[:, driven].max() < 1e-6
    if name == 'het17':
        undriven = sorted(np.nonzero(pt.es_cols < 0)[0])
        assert undriven == sorted(HET_UNDRIVEN)
        assert all(float(terms[:, b].abs().max()) > 0 for b in undriven)          # no head, but the hidden layer reads them
    else:
        assert np.all(pt.es_cols >= 0)


def test_packer_surface():
    """`CentralMLPPolicy`'s surface: leading-1 broadcasting, `update` / `invalidate` / `version`, `set_of_block`, sigma, and the `ValueError`s
    of the constructor and the packer -- a per-building layout, a vector of another length, a thermal district's device planes."""
    spec = golden('g2022_all').spec()
    tab = spec.episode_tables(0)
    layout = central_layout(spec)
    N = layout.n_cols
    rng = np.random.RandomState(1)
    u = lambda a, *shape: rng.uniform(-a, a, shape)
    pol = DeepCentralMLPPolicy(u(0.1, 1, 8, N), u(0.5, 3, 8), u(0.3, 1, 12, 8), u(0.5, 1, 12), u(0.3, 1, 17, 12), np.zeros((1, 17)), sigma=0.1)
    assert (pol.n_sets, pol.n_hidden, pol.n_hidden2, pol.n_obs, pol.n_bldg, pol.version) == (3, 8, 12, N, 17, 0)
    pt = pol.pack(layout, tab, set_of_block=[2, 0, 1])
    assert pt.version == 0 and pt.n_sets == 3 and pt.set_of_block.tolist() == [2, 0, 1] and np.all(pt.sigma_bldg == 0.1)
    assert bool((pt.out == pt.out[:1]).all()) and bool((pt.l2 == pt.l2[:1]).all()) and bool((pt.dep == pt.dep[:1]).all())
    assert not bool((pt.pre[0] == pt.pre[1]).all())
    x = CentralObservations(layout, tab).at(3, np.full((17, 2), 0.5), np.zeros((17, 2)))
    a0 = pol.actions_host(x, tables=pt)
    assert a0.shape == (2, 17) and np.array_equal(a0, pol.actions_host(x))              # (bounds -1 / 1 are the 2022 schema's)
    assert not np.array_equal(pol.actions_host(x, set_index=1), a0)
    z = np.ones((2, 17))
    assert np.allclose(pol.actions_host(x, noise=z, tables=pt), np.clip(a0 + 0.1, -1, 1)) and np.allclose(pol.actions_host(x, noise=z), np.clip(a0 + 0.1, -1, 1))
    pol.update(w3=-pol.w3)
    assert pol.version == 1 and pol.pack(layout, tab).version == 1 and np.allclose(pol.actions_host(x), -a0)
    pol.invalidate()
    assert pol.version == 2
    with pytest.raises(ValueError, match='w2: shape'):
        pol.update(w2=np.zeros((1, 8, 12)))
    with pytest.raises(ValueError, match='set_of_block outside'):
        pol.pack(layout, tab, set_of_block=[3])
    six = lambda p, **kw: DeepCentralMLPPolicy(p.w1, p.b1, p.w2, p.b2, p.w3, p.b3, **kw)
    with pytest.raises(ValueError, match='sigma: a non-negative scalar'):
        six(pol, sigma=[0.1, 0.2]).pack(layout, tab)
    per_col = six(pol, sigma=np.linspace(0, 0.16, 17))
    assert np.allclose(per_col.pack(layout, tab).sigma_bldg, np.linspace(0, 0.16, 17))
    with pytest.raises(ValueError, match='per-column sigma needs `tables`'):
        per_col.actions_host(x, noise=z)
    zz = np.zeros
    good = ((1, 8, N), (1, 8), (1, 12, 8), (1, 12), (1, 17, 12), (1, 17))
    swap = lambda i, shape: tuple(shape if k == i else s for k, s in enumerate(good))
    for shapes, msg in ((swap(0, (1, 1, 8, N)), 'w1 .n_sets, H1, n_cols.'),
                        (((1, 6, N), (1, 6), (1, 12, 6), (1, 12), (1, 17, 12), (1, 17)), 'H1=6'),
                        (((1, 68, N), (1, 68), (1, 12, 68), (1, 12), (1, 17, 12), (1, 17)), 'H1=68'),
                        (((1, 8, N), (1, 8), (1, 6, 8), (1, 6), (1, 17, 6), (1, 17)), 'H2=6'),
                        (((1, 8, N), (1, 8), (1, 68, 8), (1, 68), (1, 17, 68), (1, 17)), 'H2=68'),
                        (swap(1, (1, 4)), 'about H1'),
                        (swap(2, (1, 12, 4)), 'about H1'),
                        (swap(2, (1, 8, 12)), 'H1'),                               # W2 handed over transposed
                        (swap(3, (1, 8)), 'about H2'),
                        (swap(4, (1, 17, 8)), 'about H2'),
                        (swap(5, (1, 16)), 'about n_bldg')):
        with pytest.raises(ValueError, match=msg):
            DeepCentralMLPPolicy(*[zz(s) for s in shapes])
    big = DeepCentralMLPPolicy(zz((1, 64, N)), zz((1, 64)), zz((1, 4, 64)), zz((1, 4)), zz((1, 17, 4)), zz((1, 17))).pack(layout, tab)
    assert (big.n_hidden, big.n_hidden2) == (64, 4) and tuple(big.l2.shape) == (1, 65, 4)
    with pytest.raises(ValueError, match='do not broadcast to 3 sets'):
        DeepCentralMLPPolicy(zz((2, 8, N)), zz((3, 8)), *[zz(s) for s in good[2:]]).pack(layout, tab)
    # the layout must be the central agent's, of this length, over this many buildings
    with pytest.raises(ValueError, match='a DeepCentralMLPPolicy is defined over.*central_agent=False'):
        pol.pack(ObservationLayout(spec, 'current', True, central_agent=False), tab)
    with pytest.raises(ValueError, match='central_agent=False'):
        pol.torch_policy(ObservationLayout(spec, 'current', True, central_agent=False), tab, 'cpu')
    with pytest.raises(ValueError, match=f'w1 takes {N} observations, the central-agent vector has'):
        pol.pack(central_layout(spec, normalize=False), tab)
    spec9 = golden('g2022_all').spec(buildings=list(range(9)))
    lay9 = central_layout(spec9)
    with pytest.raises(ValueError, match='heads for 17 buildings, the district has 9'):
        DeepCentralMLPPolicy(zz((1, 8, lay9.n_cols)), *[zz(s) for s in good[1:]]).pack(lay9, spec9.episode_tables(0))
    # a column fed by any other device plane: MLPPolicy.pack's refusal (a thermal district's storage socs)
    th = golden('g2020_cz1').spec()
    lay_th, nb = central_layout(th), len(th.buildings)
    with pytest.raises(ValueError, match="is fed by device plane.*the policy kernel only has the building's own electrical_storage_soc"):
        DeepCentralMLPPolicy(zz((1, 8, lay_th.n_cols)), zz((1, 8)), zz((1, 12, 8)), zz((1, 12)), zz((1, nb, 12)), zz((1, nb))).pack(lay_th, th.episode_tables(0))
    with pytest.raises(ValueError, match='observation_mode="reference"'):
        lay_ref = ObservationLayout(spec, 'reference', True, central_agent=True)
        DeepCentralMLPPolicy(zz((1, 8, lay_ref.n_cols)), *[zz(s) for s in good[1:]]).pack(lay_ref, tab)


def test_torch_policy_is_the_same_mlp():
    """`torch_policy` over a central-agent observation tensor against `actions_host`, in float64 on the CPU; undriven action columns stay 0."""
    import torch
    spec = district('het17')
    tab = spec.episode_tables(0)
    layout = central_layout(spec)
    pol = make_deep_central_policy(layout, 16, 24, seed=2, mid_scale=1.0)
    pt = pol.pack(layout, tab)
    cobs = CentralObservations(layout, tab)
    rng = np.random.RandomState(2)
    x = cobs.at(11, rng.uniform(0, 1, (17, 6)), rng.uniform(-2, 4, (17, 6)))
    f = pol.torch_policy(layout, tab, 'cpu', dtype=torch.float64)
    got = f(torch.from_numpy(x)).numpy().astype(np.float64)                   # [n_act, E] (float32 on the way out)
    want = pol.actions_host(x, tables=pt)                                     # [E, B]
    driven = np.nonzero(pt.es_cols >= 0)[0]
    assert got.shape[1] == 6 and np.allclose(got[pt.es_cols[driven]], want.T[driven], rtol=0, atol=2e-7)
    others = np.setdiff1d(np.arange(got.shape[0]), pt.es_cols[driven])
    assert np.all(got[others] == 0)
    # layer 2 matters: another middle layer, other actions
    other = DeepCentralMLPPolicy(pol.w1, pol.b1, -pol.w2, pol.b2, pol.w3, pol.b3)
    assert np.abs(other.actions_host(x, tables=pt) - want)[:, driven].max() > 1e-3


# ---- 4. conditioning of the closed loop -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H1,H2', [(4, 4), (32, 32), (64, 64), (64, 4)])
@pytest.mark.parametrize('name', ['g2022_all', 'het17', 'b1', 'b32'])
def test_closed_loop_is_well_conditioned(name, H1, H2):
    """tests/test_policy_central_host.py::test_closed_loop_is_well_conditioned, criteria unchanged, for the test policies with two hidden layers
    of the free-running GPU test, before any GPU run: the CPU oracle stepped K = 48 from reset with `actions_host` in float64, against the same
    loop with every action rounded through float32 and moved by the GPU teacher-forced tolerance -- 4 x the worst deviation of a float32 torch
    evaluation on this trajectory's own observations: soc and net must stay within 0.1 x (1e-4 + 1e-4 |ref|), while the policy does something.
    Fixes policy_central_deep_util.MID_SCALE (readings there)."""
    spec = district(name)
    K, E = 48, 4
    tab = spec.episode_tables(0)
    layout = central_layout(spec)
    pol = make_deep_central_policy(layout, H1, H2, seed=H1 + H2)
    pt = pol.pack(layout, tab)
    ref = host_closed_loop(spec, tab, layout, pol, pt, K, E)
    cobs = CentralObservations(layout, tab)
    x = np.stack([cobs.at(t, ref['soc'][t - 1], ref['net'][t - 1]) for t in range(1, K)])
    tol = 4.0 * f32_torch_deviation(pol, x, pt)
    got = host_closed_loop(spec, tab, layout, pol, pt, K, E, perturb=tol, round_f32=True)
    assert 0 < tol < 1e-5, tol
    driven = pt.es_cols >= 0
    act = ref['action'][:, driven]
    # a policy that does something: as in tests/test_policy_central_host.py -- many buildings span a range; b1 has ONE seeded draw of weights per
    # shape, where all the closed loop needs is an action that is not 0 and moves with the observations
    assert (np.abs(act).max() > 0.05 and np.ptp(act) > 0.1) if name != 'b1' else (np.abs(act).max() > 1e-3 and np.ptp(act) > 1e-4)
    if name == 'het17':
        assert sorted(np.nonzero(~driven)[0]) == sorted(HET_UNDRIVEN)
    for k in ('soc', 'net'):
        err = float((np.abs(got[k] - ref[k]) / (1e-4 + 1e-4 * np.abs(ref[k]))).max())
        print(f'{name} H1={H1} H2={H2} {k}: worst {err:.4f} x (1e-4 + 1e-4 |ref|), action tolerance {tol:.3e}, |action| max {np.abs(act).max():.3f}, '
              f'range {np.ptp(act):.3f}')
        assert err < 0.1, (name, k, err)


# ---- 5. generated code ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def central_deep_unit(tmp_path_factory):
    (src, flags), = EXT.sources
    return _asm(src, flags, tmp_path_factory)


def test_central_deep_kernel_resources(central_deep_unit):
    """Every instantiation of cl_rollout_policy_central_kernel<PREC, DEEP = true> -- the fp32 map and the float64 chain: no scratch memory and
    at most 128 registers, a 1024-thread workgroup's limit.  The unit holds its own kernel only: no DEEP = false instantiation of the template."""
    kernels, meta = central_deep_unit
    names = [k for k in kernels if 'cl_rollout_policy_central_kernel' in k]
    by = {int(re.search(r'cl_rollout_policy_central_kernelILi(\d)ELb1EE', k).group(1)): k for k in names}
    assert sorted(by) == [0, 2] and len(names) == 2
    assert not [k for k in kernels if 'cl_rollout_kernel' in k or 'cl_rollout_policy_kernel' in k or 'cl_step' in k]
    for prec, k in by.items():
        assert meta[k]['private_seg_size'] == 0, k
        assert meta[k]['num_vgpr'] <= 128, (k, meta[k])
