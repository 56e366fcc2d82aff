"""The closed-loop rollout of a policy with TWO hidden layers (`clpd_rollout_mlp_f32`, kernel `cl_rollout_policy_deep_kernel` in
csrc/cl_policy_deep.h, library ``libcitylearn_amd_policy_deep.so``) as far as it can be checked without a GPU: the library's symbol list and
struct, every refusal of the host entry (before any HIP call), the packer against the unsplit MLP in float64, the conditioning of the closed
loop the GPU tests run (tests/test_gpu_policy_deep_rollout.py), and the generated gfx950 code of every instantiation."""
import ctypes
import re

import numpy as np
import pytest

from golden_util import golden
from citylearn_amd import _lib, abi, policy
from citylearn_amd.observations import ObservationLayout
from district_util import HET_UNDRIVEN, district
from policy_deep_util import DeepHostEntry, f32_torch_deviation, host_closed_loop, make_deep_policy
from policy_util import HostObservations, exports
from test_isa_guards import _asm, _count

DEEP = _lib.POLICY_DEEP


@pytest.fixture(scope='module')
def entry():
    return DeepHostEntry(DEEP, n_bldg=17, flags=abi.CLD_LEAN)


# ---- 1. the library -------------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header(entry):
    assert DEEP.symbols == ['clpd_abi_version', 'clpd_core_abi_version', 'clpd_last_error', 'clpd_rollout_mlp_f32']
    assert exports(DEEP.path) == DEEP.symbols
    assert entry.lib.clpd_abi_version() == DEEP.abi_version == 1 and entry.lib.clpd_core_abi_version() == abi.CL_ABI_VERSION
    assert policy.DEEP_CONSTANTS == {'CLPD_ABI_VERSION': 1, 'CLPD_MAX_HIDDEN': 32, 'CLPD_MATRIX_CORES': 1}
    (src, flags), = DEEP.sources
    assert flags == ['-fno-slp-vectorize'] and src.name == 'cl_policy_deep.hip'


def test_struct_layout_matches_the_header():
    text = abi._strip_comments(DEEP.header.read_text())
    body = re.search(r'typedef\s+struct\s+clpd_mlp\s*\{(.*?)\}\s*clpd_mlp\s*;', text, flags=re.S).group(1)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            first, *more = decl.split(',')
            fields += [re.sub(r'\[.*\]|\*', '', part).strip() for part in [first.split()[-1], *more]]
    assert [f for f, _ in _lib.PolicyDeepMLP._fields_] == fields
    # clpol_mlp's fields first, under the same names (the shared host checks are templates over them), then the second layer
    assert fields[:len(_lib.PolicyMLP._fields_)] == [f for f, _ in _lib.PolicyMLP._fields_] and fields[-3:] == ['n_hidden2', 'reserved2', 'l2']
    assert ctypes.sizeof(_lib.PolicyDeepMLP) == ctypes.sizeof(_lib.PolicyMLP) + 16 and _lib.PolicyDeepMLP.l2.offset == ctypes.sizeof(_lib.PolicyMLP) + 8


def test_the_extension_tuples():
    """The new tuple beside the pinned ones, and the kind of its own."""
    assert _lib.DEEP_EXTENSIONS == (DEEP,)
    every = _lib.ALL_EXTENSIONS + _lib.CHUNK_KPI_EXTENSIONS + _lib.LEAN_CHUNK_EXTENSIONS
    assert len(every) == 7 and DEEP not in every and len({e.path for e in every + _lib.DEEP_EXTENSIONS}) == 8
    import inspect
    import __graft_entry__
    assert '_lib.ALL_EXTENSIONS + _lib.CHUNK_KPI_EXTENSIONS + _lib.LEAN_CHUNK_EXTENSIONS + _lib.DEEP_EXTENSIONS' in inspect.getsource(__graft_entry__.build)
    kind = policy.DeepMLPPolicy.kind
    assert kind.ext is DEEP and kind.ext_kpi is None and kind.ext_chunk is None and kind.ext_chunk_kpi is None and kind.ext_chunk_pair is None
    assert kind.one_row_max == 32 and kind.n_planes == policy.CLPOL_NT and kind.tables is policy.DeepPolicyTables and kind.struct is _lib.PolicyDeepMLP
    assert policy.DeepPolicyTables.kind is kind and policy.PolicyTables.kind is policy.MLPPolicy.kind and policy.MLPPolicy.kind is not kind


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_before_any_hip_call(entry):
    """Every refusal of the entry with its code and whole message, from a call on host memory: a call that reached a launch would not return one
    of these codes."""
    e, L = entry, abi.CLD_LEAN
    EINVAL, ENULL, EALIGN, ERANGE = abi.CL_EINVAL, abi.CL_ENULL, abi.CL_EALIGN, abi.CL_ERANGE
    P = 'clpd_rollout_mlp_f32: '
    kind = lambda k: L | (k << abi.CLD_REWARD_SHIFT)
    for d, kw, code, msg in (
            (e.dims(flags=0), {}, EINVAL, P + 'only battery + PV districts (CLD_LEAN); a thermal / outage district has no deep closed-loop rollout kernel'),
            (e.dims(n_bldg=33), {}, EINVAL, P + 'n_bldg=33 > 32 would be a building-chunked launch, which the deep policy kernel is not '
                                                '(one workgroup row, two buildings per wave)'),
            (e.dims(flags=L | abi.CLD_F64_MAPS), {}, EINVAL, P + 'the battery map in fp32 or as the float64 chain (CLD_F64_CHAIN), not CLD_F64_MAPS'),
            (e.dims(flags=L | abi.CLD_KPI), {}, EINVAL, P + 'no streaming KPIs (CLD_KPI) inside this kernel -- record traj and replay CLPOL_T_ACTION '
                                                            'through cl_rollout_seq_f32'),
            (e.dims(flags=L | abi.CLD_WRITE_DETAIL), {}, EINVAL, P + 'not with the detail planes (CLD_WRITE_DETAIL)'),
            (e.dims(flags=kind(abi.CLR_EV)), {}, EINVAL, P + 'reward kind CLR_EV needs the flexible-load tables'),
            (e.dims(flags=kind(abi.CLR_MARL)), {}, EINVAL, P + 'reward kind CLR_MARL: the deep policy kernel has no barrier in its K loop to couple the '
                                                               'buildings inside a step'),
            (e.dims(env_pitch=128), {}, EINVAL, P + 'env_pitch=128 != n_env=64 is not implemented for this call'),
            (e.dims(), dict(n_hidden=0), EINVAL, 'n_hidden=0: the policy kernel takes 4, 8, .. 32 hidden units'),
            (e.dims(), dict(n_hidden=6), EINVAL, 'n_hidden=6: the policy kernel takes 4, 8, .. 32 hidden units'),
            (e.dims(), dict(n_hidden=36), EINVAL, 'n_hidden=36: the policy kernel takes 4, 8, .. 32 hidden units'),
            (e.dims(), dict(n_sets=0), EINVAL, 'n_sets=0: at least one parameter set'),
            (e.dims(), dict(n_hidden2=0), EINVAL, 'n_hidden2=0: the deep policy kernel takes 4, 8, .. 32 units in its second hidden layer'),
            (e.dims(), dict(n_hidden2=10), EINVAL, 'n_hidden2=10: the deep policy kernel takes 4, 8, .. 32 units in its second hidden layer'),
            (e.dims(), dict(n_hidden2=36), EINVAL, 'n_hidden2=36: the deep policy kernel takes 4, 8, .. 32 units in its second hidden layer'),
            (e.dims(), dict(flags=2), EINVAL, 'clpd_mlp.flags takes CLPD_MATRIX_CORES only, .reserved / .reserved2 must be 0'),
            (e.dims(), dict(flags=policy.CLPD_MATRIX_CORES | 4), EINVAL, 'clpd_mlp.flags takes CLPD_MATRIX_CORES only, .reserved / .reserved2 must be 0'),
            (e.dims(), dict(reserved=1), EINVAL, 'clpd_mlp.flags takes CLPD_MATRIX_CORES only, .reserved / .reserved2 must be 0'),
            (e.dims(), dict(reserved2=1), EINVAL, 'clpd_mlp.flags takes CLPD_MATRIX_CORES only, .reserved / .reserved2 must be 0'),
            (e.dims(), dict(null='state'), ENULL, 'state is NULL'),
            (e.dims(), dict(odd='traj'), EALIGN, 'traj is not 16-byte aligned'),
            (e.dims(), dict(l2=None), ENULL, 'mlp.l2 is NULL'),
            (e.dims(), dict(l2=e.ODD), EALIGN, 'mlp.l2 is not 16-byte aligned'),
            (e.dims(), dict(set_of_block=e.ODD1), EALIGN, 'mlp.set_of_block is not 4-byte aligned'),
            (e.dims(), dict(t0=95), ERANGE, 'steps [95, 103) outside [0, 100)'),
            (e.dims(), dict(t0=-1), ERANGE, 'steps [-1, 7) outside [0, 100)'),
            (e.dims(), dict(k_steps=-1), ERANGE, 'steps [0, -1) outside [0, 100)'),
            (e.dims(tun=dict(vec=2)), {}, EINVAL, 'no deep policy rollout kernel at 2 envs per lane: it runs at one env per lane'),
            (e.dims(tun=dict(vec=4)), {}, EINVAL, 'no deep policy rollout kernel at 4 envs per lane'),
            (e.dims(tun=dict(nw=8)), {}, EINVAL, 'bad nw 8'),
            (e.dims(n_bldg=5, tun=dict(nw=8)), {}, EINVAL, 'bad nw 8'),
            # sixteen waves x two buildings x 32 x 32 units: 164 864 bytes of LDS
            (e.dims(n_bldg=32), dict(n_hidden=32, n_hidden2=32), EINVAL, f'the deep policy rollout would need {_lib.policy_deep_lds_bytes(16, 32, 32)} bytes of LDS '
                                                                         'per workgroup (nw=16, 1 envs per lane): a CU has 163840'),
            # ... and the matrix-core family's rows have that size at every H1, H2
            (e.dims(n_bldg=32), dict(flags=policy.CLPD_MATRIX_CORES, n_hidden=4, n_hidden2=4), EINVAL,
             'the deep policy rollout would need 164864 bytes of LDS per workgroup (nw=16, 1 envs per lane): a CU has 163840')):
        assert e.call(d, **kw) == code and e.error() == msg, (kw, e.error())
    for name in ('pre', 'dep', 'out', 'act_low', 'act_high'):
        assert e.call(e.dims(), **{name: None}) == ENULL and e.error() == f'mlp.{name} is NULL'
    for name in ('pre', 'dep', 'out', 'net_reset', 'sigma'):
        assert e.call(e.dims(), **{name: e.ODD}) == EALIGN and e.error() == f'mlp.{name} is not 16-byte aligned'
    assert e.call(None) == ENULL and e.error() == 'dims is NULL'
    assert _lib.policy_deep_lds_bytes(16, 32, 32) == 164864 > 163840 >= max(_lib.policy_deep_lds_bytes(16, 32, 28), _lib.policy_deep_lds_bytes(15, 32, 32))


# ---- 3. the packer --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['g2022_all', 'het17'])
def test_packed_layers_equal_the_unsplit_mlp(name):
    """`pre + dep x` and the packed layer 2 / output rebuilt on the host in float64 from the float32 tables against `actions_host` (the unsplit
    MLP in float64) on observation rows with random state.  Every packed number carries one float32 rounding (2^-24 relative); through tanh
    (slope <= 1) the action moves by at most half x 2^-24 x (the l1 mass of each layer's terms, propagated), taken with a factor 2."""
    spec = district(name)
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    pol = make_deep_policy(layout, 16, 32, n_sets=2, seed=3)
    pt = pol.pack(layout, tab)
    pt = pol.pack(layout, tab, matrix_cores=False)
    assert isinstance(pt, policy.DeepPolicyTables) and (pt.n_hidden, pt.n_hidden2, pt.n_sets) == (16, 32, 2) and pt.matrix_cores is False
    assert pt.struct(0).flags == 0 and pol.pack(layout, tab, matrix_cores=True).struct(0).flags == policy.CLPD_MATRIX_CORES
    B = len(spec.buildings)
    assert tuple(pt.l2.shape) == (2, B, 17, 32) and tuple(pt.out.shape) == (2, B, 33) and tuple(pt.dep.shape) == (2, B, 2, 16)
    hobs = HostObservations(layout, tab)
    rng = np.random.RandomState(5)
    E = 5
    S = policy.ACT_SCALE
    u = 2.0 ** -24
    for s in range(2):
        pre, dep = pt.pre[s].numpy().astype(np.float64), pt.dep[s].numpy().astype(np.float64)
        l2, out = pt.l2[s].numpy().astype(np.float64), pt.out[s].numpy().astype(np.float64)
        _, _, w2, b2, w3, b3 = (v[s] for v in pol._full(B))
        assert np.allclose(l2[:, :16].transpose(0, 2, 1), S * w2, rtol=2 * u, atol=0) and np.allclose(l2[:, 16], S * b2, rtol=2 * u, atol=0)
        assert np.allclose(out[:, :32], w3, rtol=2 * u, atol=0) and np.allclose(out[:, 32], b3, rtol=2 * u, atol=0)
        for r in (1, 9, 100):
            soc, net = rng.uniform(0, 1, size=(B, E)), rng.uniform(-3, 6, size=(B, E))
            z1 = pre[r][None] + dep[None, :, 0] * soc.T[:, :, None] + dep[None, :, 1] * net.T[:, :, None]             # [E, B, H1], scaled
            m1 = np.abs(pre[r][None]) + np.abs(dep[None, :, 0] * soc.T[:, :, None]) + np.abs(dep[None, :, 1] * net.T[:, :, None])
            h1 = np.tanh(z1 / S)
            z2 = l2[None, :, 16] + np.einsum('bji,ebj->ebi', l2[:, :16], h1)
            # scaled sums' errors: layer 1's own roundings, then layer 2's own + layer 1's carried through |l2|
            e1 = 2 * u * m1 / abs(S)
            m2 = np.abs(l2[None, :, 16]) + np.einsum('bji,ebj->ebi', np.abs(l2[:, :16]), np.abs(h1))
            e2 = (2 * u * m2 + np.einsum('bji,ebj->ebi', np.abs(l2[:, :16]), e1)) / abs(S)
            h2 = np.tanh(z2 / S)
            z3 = out[None, :, 32] + np.einsum('bi,ebi->eb', out[:, :32], h2)
            e3 = 2 * u * (np.abs(out[None, :, 32]) + np.einsum('bi,ebi->eb', np.abs(out[:, :32]), np.abs(h2))) + np.einsum('bi,ebi->eb', np.abs(out[:, :32]), e2)
            half = 0.5 * (pt.high_bldg - pt.low_bldg)
            got = np.clip(0.5 * (pt.high_bldg + pt.low_bldg) + half * np.tanh(z3), pt.low_bldg, pt.high_bldg)
            want = pol.actions_host(hobs.at(r, soc, net), tables=pt, set_index=s)
            driven = pt.es_cols >= 0
            assert np.all(np.abs(got - want)[:, driven] <= (half * e3)[:, driven] + 1e-15), float(np.abs(got - want)[:, driven].max())
            assert np.abs(got - want)[:, driven].max() < 1e-6
    if name == 'het17':
        assert sorted(np.nonzero(pt.es_cols < 0)[0]) == sorted(HET_UNDRIVEN)


@pytest.mark.parametrize('H1,H2', [(4, 4), (8, 32), (32, 8), (32, 32)])
def test_matrix_core_fragments(H1, H2):
    """The second layout of the layer-2 table.  The f16 fragments reassemble, in the A-operand lane layout, to ACT_SCALE x W2 zero-padded to
    32 x 32: (A0 + 2^-11 A1) 2^12 inv within the split's derived bound |r| <= 2^-22 |x| on top of the table's one float32 rounding
    (2^-24 |x|); every stored term that is not zero is a NORMAL f16 unless the weight is below 2^-27 of the building's largest; the bias row
    is 2^12 sw ACT_SCALE b2, zero-padded; everything else is the exact-fp32 tables'.  And a numpy emulation of the kernel's two-term split
    product -- float16 casts of both scaled operands, the three partial products, float32 accumulation in the kernel's two chains, the scales
    taken out -- stays inside `split_sum_bound` (+ the accumulation's own roundings), also with every subnormal f16 flushed to zero."""
    from policy_deep_util import split_bound, split_sum_bound
    spec = golden('g2022_all').spec()
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    pol = make_deep_policy(layout, H1, H2, n_sets=2, seed=7)
    pt, pt0 = pol.pack(layout, tab, matrix_cores=True), pol.pack(layout, tab, matrix_cores=False)
    assert pt.matrix_cores and tuple(pt.l2.shape) == (2, 17, 1024 + 32 + 4) and pt.n_hidden2 == H2 and pt.n_hidden == H1
    for name in ('pre', 'dep', 'out', 'net_reset', 'act_low', 'act_high'):
        assert np.array_equal(getattr(pt, name).numpy(), getattr(pt0, name).numpy()), name
    S = policy.ACT_SCALE
    want = np.zeros((2, 17, 32, 32))
    want[:, :, :H2, :H1] = S * np.broadcast_to(pol.w2, (2, 17, H2, H1))
    t = pt.l2_fragments().astype(np.float64)                                   # [2 terms, S, B, 32, 32]
    tail = pt.l2.numpy()[:, :, 1024:].astype(np.float64)
    inv = tail[:, :, 32]
    sw = 1.0 / (4096.0 * inv)
    amax = np.abs(want).max(axis=(2, 3))
    assert np.all(np.log2(sw) == np.round(np.log2(sw))) and np.all(amax * sw >= 2.0 ** 13) and np.all(amax * sw < 2.0 ** 14) and np.all(tail[:, :, 33:] == 0)
    err = np.abs((t[0] + t[1] / 2048.0) / sw[:, :, None, None] - want)
    assert np.all(err <= (2.0 ** -22 + 2.0 ** -24) * np.abs(want) + 2.0 ** -27 * amax[:, :, None, None])
    assert np.all(t[:, :, :, H2:] == 0) and np.all(t[:, :, :, :, H1:] == 0) and np.abs(t[1]).max() > 0
    normal = lambda v: (v == 0) | (np.abs(v) >= 2.0 ** -14)
    assert np.all(normal(t[0]) | (np.abs(want) < 2.0 ** -27 * amax[:, :, None, None])) and np.all(np.abs(t[1]) <= np.abs(t[0]) * (1 + 2.0 ** -10))
    assert np.all(normal(t[1]) | (np.abs(t[1]) / 2048.0 < 2.0 ** -25))             # (a subnormal residual term stands for less than 2^-25 of W')
    assert np.allclose(tail[:, :, :H2], 4096.0 * sw[:, :, None] * S * np.broadcast_to(pol.b2, (2, 17, H2)), rtol=2.0 ** -23, atol=0) and np.all(tail[:, :, H2:32] == 0)
    # the emulation, against the exact product of the float32 operands
    rng = np.random.RandomState(H1 * 64 + H2)
    a = (S * np.broadcast_to(pol.w2, (2, 17, H2, H1))[0]).astype(np.float32)     # [B, H2, H1]
    h = np.tanh(rng.uniform(-3, 3, size=(17, 9, H1))).astype(np.float32)         # [B, envs, H1]
    h[:, 0] = 1e-6 * h[:, 0]                                                    # (tiny activations)
    h[:, 1, 0] = 0.0
    f16 = lambda x: x.astype(np.float16).astype(np.float32)
    flushed = lambda x: np.where(np.abs(x) < 2.0 ** -14, np.float32(0), x)
    exact = np.einsum('bij,bej->bei', a.astype(np.float64), h.astype(np.float64))
    mass = np.einsum('bij,bej->bei', np.abs(a).astype(np.float64), np.abs(h).astype(np.float64))
    bound = split_sum_bound(a)[:, None, :] + 4 * H1 * 2.0 ** -24 * mass         # the split (|h| <= 1) + the float32 additions of both chains
    s_w = sw[0][:, None, None].astype(np.float32)
    for flush in (False, True):
        fl = flushed if flush else (lambda x: x)
        ap, hp = a * s_w, h * np.float32(4096.0)
        a0, h0 = fl(f16(ap)), fl(f16(hp))
        a1, h1 = fl(f16((ap - a0) * np.float32(2048.0))), fl(f16((hp - h0) * np.float32(2048.0)))
        main, res = np.zeros((17, 9, H2), dtype=np.float32), np.zeros((17, 9, H2), dtype=np.float32)
        for j in range(H1):                                                     # (each f16 x f16 product is exact in float32)
            main = (main + a0[:, None, :, j] * h0[:, :, None, j]).astype(np.float32)
            res = (res + a1[:, None, :, j] * h0[:, :, None, j]).astype(np.float32)
        for j in range(H1):
            res = (res + a0[:, None, :, j] * h1[:, :, None, j]).astype(np.float32)
        z = (main.astype(np.float64) + res.astype(np.float64) / 2048.0) * inv[0][:, None, None]
        ratio = float((np.abs(z - exact) / bound).max())
        print(f'({H1}, {H2}) flush={flush}: emulated split error / bound {ratio:.3f}')
        assert ratio <= 1.0
    sb = split_bound(pol, pt)
    print(f'({H1}, {H2}): split_bound on the action {sb:.3e}')
    assert 0 < sb < 1e-5


def test_default_family_fits_the_district():
    """`pack(matrix_cores=None)`: the matrix-core family from H1 x H2 = 512 up, but never where its rows -- the 32 x 32 size at every H1, H2 --
    exceed a CU's LDS: sixteen waves, 31 or 32 buildings.  `_lib.policy_deep_mma_lds_bytes` is the library's figure (its refusal's, in
    test_refusals_name_their_cause_before_any_hip_call)."""
    assert _lib.policy_deep_mma_lds_bytes(16) == 164864 == _lib.policy_deep_lds_bytes(16, 32, 32) and _lib.policy_deep_mma_lds_bytes(15) == 154560
    assert _lib.LDS_PER_CU == 163840
    for H in ((16, 32), (32, 16), (24, 24), (32, 32), (32, 28)):
        assert policy.default_matrix_cores(*H) and all(policy.default_matrix_cores(*H, n) for n in (1, 2, 17, 29, 30))
        assert not policy.default_matrix_cores(*H, 31) and not policy.default_matrix_cores(*H, 32)
    for H in ((4, 4), (16, 16), (16, 28), (20, 24)):
        assert not policy.default_matrix_cores(*H) and not policy.default_matrix_cores(*H, 17)
    spec = district('b32')
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    pol = make_deep_policy(layout, 16, 32)
    assert pol.pack(layout, tab).matrix_cores is False and pol.pack(layout, tab, matrix_cores=True).matrix_cores is True
    g = golden('g2022_all').spec()
    lay17 = ObservationLayout(g, 'current', True)
    assert make_deep_policy(lay17, 16, 32).pack(lay17, g.episode_tables(0)).matrix_cores is True


def test_packer_surface():
    """`MLPPolicy`'s surface: leading-1 broadcasting, `update` / `invalidate` / `version`, the packer's refusals (the first layer is packed by
    `MLPPolicy.pack` itself), `matrix_cores`, and the shapes the constructor refuses."""
    spec = golden('g2022_all').spec()
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    shared = make_deep_policy(layout, 8, 12, shared=True, seed=1, sigma=0.1)
    assert shared.w1.shape[1] == 1 and shared.version == 0
    pt = shared.pack(layout, tab, matrix_cores=False)
    assert pt.version == 0 and tuple(pt.l2.shape) == (1, 17, 9, 12) and bool((pt.l2 == pt.l2[:, :1]).all()) and np.all(pt.sigma_bldg == 0.1)
    x = HostObservations(layout, tab).at(3, np.full((17, 2), 0.5), np.zeros((17, 2)))
    a0 = shared.actions_host(x, tables=pt)
    assert a0.shape == (2, 17) and np.array_equal(a0, shared.actions_host(x))           # (bounds -1 / 1 are the 2022 schema's)
    shared.update(w3=-shared.w3)
    assert shared.version == 1 and shared.pack(layout, tab).version == 1 and not np.array_equal(shared.actions_host(x), a0)
    shared.invalidate()
    assert shared.version == 2
    with pytest.raises(ValueError, match='w2: shape'):
        shared.update(w2=np.zeros((1, 1, 12, 4)))
    assert shared.pack(layout, tab).matrix_cores is policy.default_matrix_cores(8, 12)
    with pytest.raises(ValueError, match='set_of_block outside'):
        shared.pack(layout, tab, set_of_block=[1])
    z = np.zeros
    for shapes, msg in ((((1, 1, 8, 3), (1, 1, 8), (1, 1, 12, 8), (1, 1, 12), (1, 1, 12)), 'b3 .n_sets, n_bldg.'),
                        (((1, 1, 6, 3), (1, 1, 6), (1, 1, 12, 6), (1, 1, 12), (1, 1, 12), (1, 1)), 'H1=6'),
                        (((1, 1, 8, 3), (1, 1, 8), (1, 1, 36, 8), (1, 1, 36), (1, 1, 36), (1, 1)), 'H2=36'),
                        (((1, 1, 8, 3), (1, 1, 8), (1, 1, 12, 4), (1, 1, 12), (1, 1, 12), (1, 1)), 'about H1'),
                        (((1, 1, 8, 3), (1, 1, 8), (1, 1, 12, 8), (1, 1, 12), (1, 1, 16), (1, 1)), 'about H2')):
        with pytest.raises(ValueError, match=msg):
            policy.DeepMLPPolicy(*[z(s) for s in shapes], *([z((1,))] if len(shapes) == 5 else []))
    # a policy that reads another building's plane is the packer's refusal, as for MLPPolicy: 3 observations do not match the buildings'
    with pytest.raises(ValueError, match='w1 takes 3 observations'):
        policy.DeepMLPPolicy(z((1, 1, 8, 3)), z((1, 1, 8)), z((1, 1, 12, 8)), z((1, 1, 12)), z((1, 1, 12)), z((1, 1))).pack(layout, tab)


# ---- 4. conditioning of the closed loop -----------------------------------------------------------------------------------------------
# (b32 never runs in the matrix-core family: its rows exceed a CU's LDS)
@pytest.mark.parametrize('H1,H2', [(4, 4), (16, 32), (32, 32)])
@pytest.mark.parametrize('name,mma', [('g2022_all', 0), ('g2022_all', 1), ('het17', 0), ('het17', 1), ('b1', 0), ('b1', 1), ('b32', 0)])
def test_closed_loop_is_well_conditioned(name, mma, H1, H2):
    """tests/test_policy_host.py::test_closed_loop_is_well_conditioned for the deep test policies of the free-running GPU test, before any GPU
    run: the CPU oracle stepped K = 48 from reset with `actions_host` in float64, against the same loop with every action rounded through
    float32 and moved by the teacher-forced tolerance of the GPU test for that kernel family -- 4 x the worst deviation of a float32 torch
    evaluation on this trajectory's own observations, plus `split_bound` for the matrix-core family: soc and net must stay within
    0.1 x (1e-4 + 1e-4 |ref|), while the policy does something.  Fixes policy_deep_util.FREE_MID_SCALE (readings there)."""
    from policy_deep_util import FREE_MID_SCALE, split_bound
    spec = district(name)
    K, E = 48, 4
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    pol = make_deep_policy(layout, H1, H2, seed=H1 + H2, mid_scale=FREE_MID_SCALE)
    pt = pol.pack(layout, tab, matrix_cores=bool(mma))
    ref = host_closed_loop(spec, tab, layout, pol, pt, K, E)
    hobs = HostObservations(layout, tab)
    x = np.stack([hobs.at(t, ref['soc'][t - 1], ref['net'][t - 1]) for t in range(1, K)])
    tol = 4.0 * f32_torch_deviation(pol, x, pt) + (split_bound(pol, pt) if mma else 0.0)
    got = host_closed_loop(spec, tab, layout, pol, pt, K, E, perturb=tol, round_f32=True)
    assert 0 < tol < 1e-5, tol
    driven = pt.es_cols >= 0
    act = ref['action'][:, driven]
    # a policy that does something: as in tests/test_policy_host.py -- many buildings span a range; b1 has ONE seeded draw of weights per shape,
    # where all the closed loop needs is an action that is not 0 and moves with the observations
    assert (np.abs(act).max() > 0.05 and np.ptp(act) > 0.1) if name != 'b1' else (np.abs(act).max() > 1e-3 and np.ptp(act) > 1e-4)
    if name == 'het17':
        assert sorted(np.nonzero(~driven)[0]) == sorted(HET_UNDRIVEN)
    for k in ('soc', 'net'):
        err = float((np.abs(got[k] - ref[k]) / (1e-4 + 1e-4 * np.abs(ref[k]))).max())
        print(f'{name} ({H1}, {H2}) mma={mma} {k}: worst {err:.4f} x (1e-4 + 1e-4 |ref|), action tolerance {tol:.3e}, |action| max {np.abs(act).max():.3f}, '
              f'range {np.ptp(act):.3f}')
        assert err < 0.1, (name, k, err)


# ---- 5. generated code ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def deep_unit(tmp_path_factory):
    (src, flags), = DEEP.sources
    return _asm(src, flags, tmp_path_factory)


def test_deep_kernel_isa(deep_unit):
    """Every instantiation of cl_rollout_policy_deep_kernel<VEC, PREC, MMA> -- one env per lane, the fp32 map and the float64 chain, both
    families; the exact-fp32 instantiations at two envs per lane spilled to scratch memory and are not built -- : no scratch, no buffer
    instructions, no packed fp32, at most 128 registers (a 1024-thread workgroup's cap), the float64 chain only under PREC = 2.
    MMA = 0: no matrix-core instruction, layer 2's weights as broadcast ds_read_b128 (32 x 32 units take 8 reads and 128 v_fma per h1 unit, so
    the code of the eight H2 variants holds several hundred of each).  MMA = 1: six v_mfma_f32_32x32x16_f16 per building of a wave (two K
    halves x three partial products; the two 32-env passes are a loop), the f16 conversions of the split, and the cross-half exchanges as
    ds_bpermute_b32 -- three per building: soc, previous net, the partial output sum."""
    kernels, meta = deep_unit
    names = [k for k in kernels if 'cl_rollout_policy_deep_kernel' in k]
    by = {tuple(int(x) for x in re.search(r'cl_rollout_policy_deep_kernelILi(\d)ELi(\d)ELi(\d)EE', k).groups()): k for k in names}
    assert sorted(by) == [(1, 0, 0), (1, 0, 1), (1, 2, 0), (1, 2, 1)] and len(names) == 4
    assert not [k for k in kernels if 'cl_rollout_kernel' in k or 'cl_rollout_policy_kernel' in k or 'cl_step' in k]      # the unit holds its own kernel only
    for (vec, prec, mma), k in by.items():
        ins = kernels[k]
        assert meta[k]['private_seg_size'] == 0, k
        assert meta[k]['num_vgpr'] <= 128, (k, meta[k])
        assert not [i for i in ins if i.startswith(('scratch_', 'buffer_'))], k
        assert not [i for i in ins if re.match(r'v_pk_\w+_f32', i)], k
        assert any(i.startswith('v_fma_f64') for i in ins) == (prec == 2), k
        if mma:
            assert _count(ins, 'v_mfma_f32_32x32x16_f16') == 12 and _count(ins, 'v_mfma') == 12, (k, _count(ins, 'v_mfma'))
            # (the split: first terms as v_cvt_pk_f16_f32, two per instruction; the residual terms come out of v_fma_mix*_f16 directly)
            assert _count(ins, 'ds_bpermute_b32') == 6 and _count(ins, 'v_cvt_pk_f16_f32') >= 2 * 2 * 4, k
            assert _count(ins, 'v_exp_f32') >= 2 * (16 + 16) and _count(ins, 'v_rcp_f32') >= 2 * (16 + 16), k
        else:
            assert not [i for i in ins if i.startswith(('v_mfma', 'v_smfma'))], k
            assert _count(ins, 'v_exp_f32') >= 2 * (4 + 8) and _count(ins, 'v_rcp_f32') >= 2 * (4 + 8), k
            assert _count(ins, 'ds_read_b128') >= 300 and _count(ins, 'v_fma') >= 2 * 4 * (4 + 8 + 12 + 16 + 20 + 24 + 28 + 32), (k, _count(ins, 'ds_read_b128'))
            assert _count(ins, 's_load_dwordx4') >= 2, k
