"""The closed-loop rollout under a CENTRAL-AGENT policy (`clpca_rollout_mlp_f32`, kernel `cl_rollout_policy_central_kernel` in
csrc/cl_policy_central.h, library ``libcitylearn_amd_policy_central.so``) as far as it can be checked without a GPU: the library's symbol list and
struct, every refusal of the host entry (before any HIP call), the LDS formula, the packer against the unsplit MLP in float64, the conditioning
of the closed loop the GPU tests run (tests/test_gpu_policy_central_rollout.py), and the resource figures of every instantiation."""
import ctypes
import re

import numpy as np
import pytest

from golden_util import golden
from citylearn_amd import _lib, abi, policy
from citylearn_amd.observations import ObservationLayout
from citylearn_amd.policy import CentralMLPPolicy
from district_util import HET_UNDRIVEN, district
from policy_central_util import (CentralObservations, HostEntry, central_layout, f32_torch_deviation, host_closed_loop, make_central_policy)
from policy_util import exports
from test_isa_guards import _asm

EXT = _lib.POLICY_CENTRAL


@pytest.fixture(scope='module')
def entry():
    return HostEntry(EXT, n_bldg=17, flags=abi.CLD_LEAN)


# ---- 1. the library -------------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header(entry):
    assert EXT.symbols == ['clpca_abi_version', 'clpca_core_abi_version', 'clpca_last_error', 'clpca_rollout_mlp_f32']
    assert exports(EXT.path) == EXT.symbols
    assert entry.lib.clpca_abi_version() == EXT.abi_version == 1 and entry.lib.clpca_core_abi_version() == abi.CL_ABI_VERSION
    assert policy.CENTRAL_CONSTANTS == {'CLPCA_ABI_VERSION': 1, 'CLPCA_MAX_HIDDEN': 64, 'CLPCA_MAX_BLDG': 32}
    (src, flags), = EXT.sources
    assert flags == ['-fno-slp-vectorize'] and src.name == 'cl_policy_central.hip'
    assert (_lib.CSRC / 'cl_policy_central.h').exists() and EXT.path.name == 'libcitylearn_amd_policy_central.so'


def test_struct_is_the_lean_policy_struct():
    """`clpca_mlp` keeps `clpol_mlp`'s field names and order: `_lib.PolicyMLP` and the shared host checks serve it."""
    text = abi._strip_comments(EXT.header.read_text())
    body = re.search(r'typedef\s+struct\s+clpca_mlp\s*\{(.*?)\}\s*clpca_mlp\s*;', text, flags=re.S).group(1)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            first, *more = decl.split(',')
            fields += [re.sub(r'\[.*\]|\*', '', part).strip() for part in [first.split()[-1], *more]]
    assert [f for f, _ in _lib.PolicyMLP._fields_] == fields and EXT.mlp is _lib.PolicyMLP and ctypes.sizeof(_lib.PolicyMLP) == 88


def test_the_extension_tuples():
    """The new tuple beside the unchanged ones, the build function, and the kind of its own."""
    assert _lib.CENTRAL_EXTENSIONS == (EXT,)
    assert _lib.EXTENSIONS == (_lib.POLICY, _lib.POLICY_KPI, _lib.POLICY_FULL, _lib.POLICY_FULL_KPI)
    assert _lib.ALL_EXTENSIONS == _lib.EXTENSIONS + (_lib.POLICY_FULL_CHUNK,) and _lib.CHUNK_KPI_EXTENSIONS == (_lib.POLICY_FULL_CHUNK_KPI,)
    assert _lib.LEAN_CHUNK_EXTENSIONS == (_lib.POLICY_CHUNK,) and _lib.DEEP_EXTENSIONS == (_lib.POLICY_DEEP,)
    assert _lib.DEEP_THERMAL_EXTENSIONS == (_lib.POLICY_FULL_DEEP,)
    every = _lib.ALL_EXTENSIONS + _lib.CHUNK_KPI_EXTENSIONS + _lib.LEAN_CHUNK_EXTENSIONS + _lib.DEEP_EXTENSIONS + _lib.DEEP_THERMAL_EXTENSIONS
    assert len(every) == 9 and EXT not in every and len({e.path for e in every + _lib.CENTRAL_EXTENSIONS}) == 10
    assert len({e.prefix for e in every + _lib.CENTRAL_EXTENSIONS}) == 10
    import inspect
    import __graft_entry__
    assert '_lib.CENTRAL_EXTENSIONS' in inspect.getsource(__graft_entry__.build)
    kind = CentralMLPPolicy.kind
    assert kind.ext is EXT and kind.ext_kpi is None and kind.ext_chunk is None and kind.ext_chunk_kpi is None and kind.ext_chunk_pair is None
    assert kind.one_row_max == 32 and kind.n_planes == policy.CLPOL_NT and kind.no_kpi_error is NotImplementedError and kind.central
    assert kind.tables is policy.CentralPolicyTables and kind.struct is _lib.PolicyMLP and kind.max_hidden == 64
    assert policy.CentralPolicyTables.kind is kind and policy.PolicyTables.kind is policy.MLPPolicy.kind and policy.MLPPolicy.kind is not kind
    assert not any(k.central for k in (policy.MLPPolicy.kind, policy.StorageMLPPolicy.kind, policy.DeepMLPPolicy.kind, policy.DeepStorageMLPPolicy.kind))


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_before_any_hip_call(entry):
    """Every refusal of the entry with its code and whole message, from a call on host memory: a call that reached a launch would not return one
    of these codes."""
    e, L = entry, abi.CLD_LEAN
    EINVAL, ENULL, EALIGN, ERANGE = abi.CL_EINVAL, abi.CL_ENULL, abi.CL_EALIGN, abi.CL_ERANGE
    P = 'clpca_rollout_mlp_f32: '
    kind = lambda k: L | (k << abi.CLD_REWARD_SHIFT)
    HMSG = 'n_hidden=%d: the policy kernel takes 4, 8, .. 64 hidden units'
    for d, kw, code, msg in (
            (e.dims(flags=0), {}, EINVAL, P + 'only battery + PV districts (CLD_LEAN); a thermal / outage district has no central-agent rollout kernel'),
            (e.dims(n_bldg=33), {}, EINVAL, P + 'n_bldg=33 > 32: the central-agent policy kernel holds the whole district in one workgroup (two buildings '
                                                'per wave); its hidden layer cannot be cut into building chunks'),
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
            (e.dims(), dict(flags=1), EINVAL, 'clpca_mlp.flags / .reserved must be 0'),
            (e.dims(), dict(reserved=1), EINVAL, 'clpca_mlp.flags / .reserved must be 0'),
            (e.dims(), dict(null='state'), ENULL, 'state is NULL'),
            (e.dims(), dict(null='params'), ENULL, 'params is NULL'),
            (e.dims(), dict(odd='traj'), EALIGN, 'traj is not 16-byte aligned'),
            (e.dims(), dict(odd='ret_env'), EALIGN, 'ret_env is not 16-byte aligned'),
            (e.dims(), dict(set_of_block=e.ODD1), EALIGN, 'mlp.set_of_block is not 4-byte aligned'),
            (e.dims(), dict(t0=95), ERANGE, 'steps [95, 103) outside [0, 100)'),
            (e.dims(), dict(t0=-1), ERANGE, 'steps [-1, 7) outside [0, 100)'),
            (e.dims(), dict(k_steps=-1), ERANGE, 'steps [0, -1) outside [0, 100)'),
            (e.dims(tun=dict(vec=2)), {}, EINVAL, 'no central policy rollout kernel at 2 envs per lane: it runs at one env per lane'),
            (e.dims(tun=dict(vec=4)), {}, EINVAL, 'no central policy rollout kernel at 4 envs per lane'),
            (e.dims(tun=dict(nw=8)), {}, EINVAL, 'bad nw 8'),
            (e.dims(tun=dict(nw=17)), {}, EINVAL, 'bad nw 17'),
            (e.dims(n_bldg=5, tun=dict(nw=8)), {}, EINVAL, 'bad nw 8')):
        assert e.call(d, **kw) == code and e.error() == msg, (kw, e.error())
    for name in ('pre', 'dep', 'out', 'act_low', 'act_high'):
        assert e.call(e.dims(), **{name: None}) == ENULL and e.error() == f'mlp.{name} is NULL'
    for name in ('pre', 'dep', 'out', 'net_reset', 'sigma'):
        assert e.call(e.dims(), **{name: e.ODD}) == EALIGN and e.error() == f'mlp.{name} is not 16-byte aligned'
    assert e.call(None) == ENULL and e.error() == 'dims is NULL'
    # which one wins: the coverage refusals come in the order above, all in front of the struct's and the buffers'
    assert e.call(e.dims(flags=abi.CLD_KPI, n_bldg=33), n_hidden=6, null='state') == EINVAL and 'CLD_LEAN' in e.error()
    assert e.call(e.dims(n_bldg=33, flags=L | abi.CLD_KPI), n_hidden=6) == EINVAL and 'n_bldg=33 > 32' in e.error()
    assert e.call(e.dims(tun=dict(vec=2)), n_hidden=6) == EINVAL and e.error() == HMSG % 6


def _header_lds_floats(nw, n_bldg, h):
    """The formula as include/citylearn_amd_policy_central.h writes it, evaluated from the header's text."""
    text = EXT.header.read_text()
    m = re.search(r'Dynamic LDS per workgroup, in floats.*?\n \*\s+(nw x 4 x 64.*?)\n', text, flags=re.S)
    expr = m.group(1).replace('CLPCA_MAX_HIDDEN', str(policy.CLPCA_MAX_HIDDEN)).replace(' x ', ' * ')
    assert re.fullmatch(r'[\w\s*+()]+', expr), expr
    return eval(expr, {'__builtins__': {}}, dict(nw=nw, n_bldg=n_bldg, n_hidden=h))


def test_lds_formula():
    """`_lib.policy_central_lds_bytes` against the header's formula and the kernel header's function; the launch opts in above 64 KiB and no
    accepted geometry reaches a CU's 160 KiB (the entry still holds it against that, through the shared `check_policy_lds`)."""
    for n_bldg in (1, 2, 17, 31, 32):
        for nw in range((n_bldg + 1) // 2, min(n_bldg, 16) + 1):
            for h in (4, 32, 64):
                assert _lib.policy_central_lds_bytes(nw, n_bldg, h) == 4 * _header_lds_floats(nw, n_bldg, h), (nw, n_bldg, h)
    assert _lib.policy_central_lds_bytes(16, 32, 64) == 74752 > 64 * 1024 and 74752 < _lib.LDS_PER_CU == 163840
    assert _lib.policy_central_lds_bytes(9, 17, 32) == 4 * (9 * 256 + 34 * 64 + 32 * 64 + 64 * 17 + 18 * 72) == 35648
    head, unit = (_lib.CSRC / 'cl_policy_central.h').read_text(), (_lib.CSRC / 'cl_policy_central.hip').read_text()
    assert ('return (size_t)nw * NQ * 64 + (size_t)2 * n_bldg * 64 + (size_t)h * 64 + (size_t)2 * h * n_bldg + (size_t)nw * 2 * CLPC_ROW;' in head
            and 'CLPC_ROW = CLPC_MAX_HIDDEN + 8;' in head and 'CLPC_MAX_HIDDEN = 64;' in head and abi.CL_NQ == 4)
    assert 'static_assert(CLPCA_MAX_HIDDEN == CLPC_MAX_HIDDEN' in unit and policy.CLPCA_MAX_HIDDEN == 64
    assert 'check_policy_lds(lds, "central policy", nw, 1)' in unit and 'CL_POLICY_LAUNCH(cl_rollout_policy_central_kernel<0, false>)' in unit
    shared = (_lib.CSRC / 'cl_policy_common.h').read_text()
    assert 'if (lds > 64 * 1024) if (hipError_t e = ensure_dynamic_lds(' in shared and 'if (lds > CL_LDS_PER_CU) return fail(' in shared


# ---- 3. the packer --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('name', ['g2022_all', 'het17'])
def test_packed_layers_equal_the_unsplit_mlp(name, normalize):
    """`pre + dep x` and `out` rebuilt on the host in float64 from the float32 tables against `actions_host` (the unsplit MLP in float64) on
    central-agent vectors with random state.  Every packed number carries one float32 rounding (2^-24 relative); through tanh (slope <= 1) the
    action moves by at most half x 2^-24 x (the l1 mass of each layer's terms, propagated), taken with a factor 2 -- the bound of
    tests/test_policy_deep_host.py for one layer less.  het17's undriven buildings have no head, but their dep rows are not zero."""
    spec = district(name)
    tab = spec.episode_tables(0)
    layout = central_layout(spec, normalize)
    B, N, H = len(spec.buildings), layout.n_cols, 32
    pol = make_central_policy(layout, H, n_sets=2, seed=3)
    pt = pol.pack(layout, tab)
    assert isinstance(pt, policy.CentralPolicyTables) and (pt.n_hidden, pt.n_sets, pt.n_bldg, pt.n_rows) == (H, 2, B, tab.n_steps)
    assert tuple(pt.pre.shape) == (2, tab.n_steps, H) and tuple(pt.dep.shape) == (2, H // 4, B, 2, 4) and tuple(pt.out.shape) == (2, B, H + 1)
    assert tuple(pt.net_reset.shape) == (tab.n_steps, B) and pt.cols is pt.es_cols and pt.low_bldg.shape == pt.high_bldg.shape == pt.sigma_bldg.shape == (B,)
    st = pt.struct(5)
    assert (st.n_hidden, st.n_sets, st.flags, st.reserved, st.seed) == (H, 2, 0, 0, 5) and st.pre == pt.pre.data_ptr() and st.dep == pt.dep.data_ptr()
    cobs = CentralObservations(layout, tab)
    n_dep = int(cobs.is_term[0].sum() + cobs.is_term[1].sum())
    if name == 'g2022_all':
        assert (n_dep, N) == ((34, 95) if normalize else (34, N))              # 17 buildings x (soc, net)
    rng = np.random.RandomState(5)
    E, S, u = 5, policy.ACT_SCALE, 2.0 ** -24
    terms = pt.dep_terms()
    for s in range(2):
        pre, dep, out = pt.pre[s].numpy().astype(np.float64), terms[s].numpy().astype(np.float64), pt.out[s].numpy().astype(np.float64)
        _, _, w2, b2 = (v[s] for v in pol._full(B))
        assert np.allclose(out[:, :H], w2, rtol=2 * u, atol=0) and np.allclose(out[:, H], b2, rtol=2 * u, atol=0)
        # dep in the kernel's order: group g, building b, [ws x 4 | wn x 4]
        raw = pt.dep[s].numpy()
        assert np.array_equal(raw[3, 5, 0], terms[s].numpy()[5, 0, 12:16]) and np.array_equal(raw[3, 5, 1], terms[s].numpy()[5, 1, 12:16])
        for r in (1, 9, 100):
            soc, net = rng.uniform(0, 1, size=(B, E)), rng.uniform(-3, 6, size=(B, E))
            parts = dep[None, :, 0] * soc.T[:, :, None], dep[None, :, 1] * net.T[:, :, None]                     # [E, B, H] each, scaled
            z1 = pre[r][None] + parts[0].sum(axis=1) + parts[1].sum(axis=1)
            m1 = np.abs(pre[r][None]) + np.abs(parts[0]).sum(axis=1) + np.abs(parts[1]).sum(axis=1)
            h = np.tanh(z1 / S)
            e1 = 2 * u * m1 / abs(S)
            z2 = out[None, :, H] + np.einsum('bj,ej->eb', out[:, :H], h)
            e2 = 2 * u * (np.abs(out[None, :, H]) + np.einsum('bj,ej->eb', np.abs(out[:, :H]), np.abs(h))) + np.einsum('bj,ej->eb', np.abs(out[:, :H]), e1)
            half = 0.5 * (pt.high_bldg - pt.low_bldg)
            got = np.clip(0.5 * (pt.high_bldg + pt.low_bldg) + half * np.tanh(z2), pt.low_bldg, pt.high_bldg)
            want = pol.actions_host(cobs.at(r, soc, net), tables=pt, set_index=s)
            driven = pt.es_cols >= 0
            assert want.shape == (E, B) and want.dtype == np.float64
            assert np.all(np.abs(got - want)[:, driven] <= (half * e2)[:, driven] + 1e-15), float(np.abs(got - want)[:, driven].max())
            assert np.abs(got - want)[:, driven].max() < 1e-6
    # the reset observation's net is what net_reset reproduces through dep
    net_cols = np.nonzero(cobs.is_term[1])[0]
    x0 = cobs.at(7, reset=True, E=1)[0]
    back = cobs.obs.table[8][net_cols] + pt.net_reset[7].numpy().astype(np.float64)[cobs.bldg[net_cols]] * cobs.scale[net_cols]
    assert np.allclose(back, x0[net_cols], rtol=1e-6, atol=1e-6)
    if name == 'het17':
        undriven = sorted(np.nonzero(pt.es_cols < 0)[0])
        assert undriven == sorted(HET_UNDRIVEN)
        assert all(float(terms[:, b].abs().max()) > 0 for b in undriven)          # no head, but the hidden layer reads them
    else:
        assert np.all(pt.es_cols >= 0)


def test_packer_surface():
    """`MLPPolicy`'s surface: leading-1 broadcasting, `update` / `invalidate` / `version`, `set_of_block`, sigma, and the `ValueError`s of the
    constructor and the packer -- a per-building layout, a vector of another length, a thermal district's device planes."""
    spec = golden('g2022_all').spec()
    tab = spec.episode_tables(0)
    layout = central_layout(spec)
    N = layout.n_cols
    rng = np.random.RandomState(1)
    pol = CentralMLPPolicy(rng.uniform(-0.1, 0.1, (1, 8, N)), rng.uniform(-0.5, 0.5, (3, 8)), rng.uniform(-0.3, 0.3, (1, 17, 8)), np.zeros((1, 17)), sigma=0.1)
    assert (pol.n_sets, pol.n_hidden, pol.n_obs, pol.n_bldg, pol.version) == (3, 8, N, 17, 0)
    pt = pol.pack(layout, tab, set_of_block=[2, 0, 1])
    assert pt.version == 0 and pt.n_sets == 3 and pt.set_of_block.tolist() == [2, 0, 1] and np.all(pt.sigma_bldg == 0.1)
    assert bool((pt.out == pt.out[:1]).all()) and bool((pt.dep == pt.dep[:1]).all()) and not bool((pt.pre[0] == pt.pre[1]).all())
    x = CentralObservations(layout, tab).at(3, np.full((17, 2), 0.5), np.zeros((17, 2)))
    a0 = pol.actions_host(x, tables=pt)
    assert a0.shape == (2, 17) and np.array_equal(a0, pol.actions_host(x))              # (bounds -1 / 1 are the 2022 schema's)
    assert not np.array_equal(pol.actions_host(x, set_index=1), a0)
    z = np.ones((2, 17))
    assert np.allclose(pol.actions_host(x, noise=z, tables=pt), np.clip(a0 + 0.1, -1, 1)) and np.allclose(pol.actions_host(x, noise=z), np.clip(a0 + 0.1, -1, 1))
    pol.update(w2=-pol.w2)
    assert pol.version == 1 and pol.pack(layout, tab).version == 1 and np.allclose(pol.actions_host(x), -a0)
    pol.invalidate()
    assert pol.version == 2
    with pytest.raises(ValueError, match='w2: shape'):
        pol.update(w2=np.zeros((1, 17, 4)))
    with pytest.raises(ValueError, match='set_of_block outside'):
        pol.pack(layout, tab, set_of_block=[3])
    with pytest.raises(ValueError, match='sigma: a non-negative scalar'):
        CentralMLPPolicy(pol.w1, pol.b1, pol.w2, pol.b2, sigma=[0.1, 0.2]).pack(layout, tab)
    per_col = CentralMLPPolicy(pol.w1, pol.b1, pol.w2, pol.b2, sigma=np.linspace(0, 0.16, 17))
    assert np.allclose(per_col.pack(layout, tab).sigma_bldg, np.linspace(0, 0.16, 17))
    with pytest.raises(ValueError, match='per-column sigma needs `tables`'):
        per_col.actions_host(x, noise=z)
    zz = np.zeros
    for shapes, msg in ((((1, 1, 8, N), (1, 8), (1, 17, 8), (1, 17)), 'w1 .n_sets, H, n_cols.'),
                        (((1, 6, N), (1, 6), (1, 17, 6), (1, 17)), 'H=6'),
                        (((1, 68, N), (1, 68), (1, 17, 68), (1, 17)), 'H=68'),
                        (((1, 8, N), (1, 4), (1, 17, 8), (1, 17)), 'about H'),
                        (((1, 8, N), (1, 8), (1, 17, 4), (1, 17)), 'about H'),
                        (((1, 8, N), (1, 8), (1, 17, 8), (1, 16)), 'about n_bldg')):
        with pytest.raises(ValueError, match=msg):
            CentralMLPPolicy(*[zz(s) for s in shapes])
    assert CentralMLPPolicy(zz((1, 64, N)), zz((1, 64)), zz((1, 17, 64)), zz((1, 17))).pack(layout, tab).n_hidden == 64
    with pytest.raises(ValueError, match='do not broadcast to 3 sets'):
        CentralMLPPolicy(zz((2, 8, N)), zz((3, 8)), zz((1, 17, 8)), zz((1, 17))).pack(layout, tab)
    # the layout must be the central agent's, of this length, over this many buildings
    with pytest.raises(ValueError, match='central_agent=False'):
        pol.pack(ObservationLayout(spec, 'current', True, central_agent=False), tab)
    with pytest.raises(ValueError, match='central_agent=False'):
        pol.torch_policy(ObservationLayout(spec, 'current', True, central_agent=False), tab, 'cpu')
    with pytest.raises(ValueError, match=f'w1 takes {N} observations, the central-agent vector has'):
        pol.pack(central_layout(spec, normalize=False), tab)
    spec9 = golden('g2022_all').spec(buildings=list(range(9)))
    lay9 = central_layout(spec9)
    with pytest.raises(ValueError, match='heads for 17 buildings, the district has 9'):
        CentralMLPPolicy(zz((1, 8, lay9.n_cols)), zz((1, 8)), zz((1, 17, 8)), zz((1, 17))).pack(lay9, spec9.episode_tables(0))
    # a column fed by any other device plane: MLPPolicy.pack's refusal (a thermal district's storage socs)
    th = golden('g2020_cz1').spec()
    lay_th = central_layout(th)
    with pytest.raises(ValueError, match="is fed by device plane.*the policy kernel only has the building's own electrical_storage_soc"):
        CentralMLPPolicy(zz((1, 8, lay_th.n_cols)), zz((1, 8)), zz((1, len(th.buildings), 8)), zz((1, len(th.buildings)))).pack(lay_th, th.episode_tables(0))
    with pytest.raises(ValueError, match='observation_mode="reference"'):
        lay_ref = ObservationLayout(spec, 'reference', True, central_agent=True)
        CentralMLPPolicy(zz((1, 8, lay_ref.n_cols)), zz((1, 8)), zz((1, 17, 8)), zz((1, 17))).pack(lay_ref, tab)


def test_torch_policy_is_the_same_mlp():
    """`torch_policy` over a central-agent observation tensor against `actions_host`, in float64 on the CPU; undriven action columns stay 0."""
    import torch
    spec = district('het17')
    tab = spec.episode_tables(0)
    layout = central_layout(spec)
    pol = make_central_policy(layout, 16, seed=2)
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


# ---- 4. conditioning of the closed loop -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H', [4, 32, 64])
@pytest.mark.parametrize('name', ['g2022_all', 'het17', 'b1', 'b32'])
def test_closed_loop_is_well_conditioned(name, H):
    """tests/test_policy_deep_host.py::test_closed_loop_is_well_conditioned for the central test policies of the free-running GPU test, before any
    GPU run: the CPU oracle stepped K = 48 from reset with `actions_host` in float64, against the same loop with every action rounded through
    float32 and moved by the GPU teacher-forced tolerance -- 4 x the worst deviation of a float32 torch evaluation on this trajectory's own
    observations: soc and net must stay within 0.1 x (1e-4 + 1e-4 |ref|), while the policy does something.  The central loop couples every
    building to every other.  Fixes policy_central_util.W1_SCALE / W2_SCALE (readings there)."""
    spec = district(name)
    K, E = 48, 4
    tab = spec.episode_tables(0)
    layout = central_layout(spec)
    pol = make_central_policy(layout, H, seed=H)
    pt = pol.pack(layout, tab)
    ref = host_closed_loop(spec, tab, layout, pol, pt, K, E)
    cobs = CentralObservations(layout, tab)
    x = np.stack([cobs.at(t, ref['soc'][t - 1], ref['net'][t - 1]) for t in range(1, K)])
    tol = 4.0 * f32_torch_deviation(pol, x, pt)
    got = host_closed_loop(spec, tab, layout, pol, pt, K, E, perturb=tol, round_f32=True)
    assert 0 < tol < 1e-5, tol
    driven = pt.es_cols >= 0
    act = ref['action'][:, driven]
    # a policy that does something: as in tests/test_policy_deep_host.py -- many buildings span a range; b1 has ONE seeded draw of weights per
    # shape, where all the closed loop needs is an action that is not 0 and moves with the observations
    assert (np.abs(act).max() > 0.05 and np.ptp(act) > 0.1) if name != 'b1' else (np.abs(act).max() > 1e-3 and np.ptp(act) > 1e-4)
    if name == 'het17':
        assert sorted(np.nonzero(~driven)[0]) == sorted(HET_UNDRIVEN)
    for k in ('soc', 'net'):
        err = float((np.abs(got[k] - ref[k]) / (1e-4 + 1e-4 * np.abs(ref[k]))).max())
        print(f'{name} H={H} {k}: worst {err:.4f} x (1e-4 + 1e-4 |ref|), action tolerance {tol:.3e}, |action| max {np.abs(act).max():.3f}, '
              f'range {np.ptp(act):.3f}')
        assert err < 0.1, (name, k, err)


# ---- 5. generated code ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def central_unit(tmp_path_factory):
    (src, flags), = EXT.sources
    return _asm(src, flags, tmp_path_factory)


def test_central_kernel_resources(central_unit):
    """Every instantiation of cl_rollout_policy_central_kernel<PREC, DEEP = false> -- the fp32 map and the float64 chain: no scratch memory and at
    most 128 registers, a 1024-thread workgroup's limit.  The unit holds its own kernel only: no DEEP = true instantiation of the template."""
    kernels, meta = central_unit
    names = [k for k in kernels if 'cl_rollout_policy_central_kernel' in k]
    by = {int(re.search(r'cl_rollout_policy_central_kernelILi(\d)ELb0EE', k).group(1)): k for k in names}
    assert sorted(by) == [0, 2] and len(names) == 2
    assert not [k for k in kernels if 'cl_rollout_kernel' in k or 'cl_rollout_policy_kernel' in k or 'cl_step' in k]
    for prec, k in by.items():
        assert meta[k]['private_seg_size'] == 0, k
        assert meta[k]['num_vgpr'] <= 128, (k, meta[k])
