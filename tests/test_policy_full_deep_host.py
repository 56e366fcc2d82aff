"""The closed-loop rollout of a THERMAL district under a policy with TWO hidden layers (`clpfd_rollout_mlp_f32`, kernel
`cl_rollout_full_policy_deep_kernel` in csrc/cl_policy_full_deep.h, library ``libcitylearn_amd_policy_full_deep.so``) as far as it can be checked
without a GPU: the library's symbol list and struct, every refusal of the host entry (before any HIP call), the packer against
`StorageMLPPolicy.pack` and the formulas in float64, the references, the conditioning of the closed loop the GPU tests run
(tests/test_gpu_policy_full_deep_rollout.py), and the resource figures of every instantiation."""
import ctypes
import re

import numpy as np
import pytest
import torch

from citylearn_amd import _lib, abi, policy
from citylearn_amd.observations import ObservationLayout
from policy_full_deep_util import (FREE_MID_SCALE, DeepFullHostEntry, f32_torch_deviation, host_closed_loop, make_deep_storage_policy,
                                   split_bound)
from policy_full_util import THERMAL_PLANES, thermal_district
from policy_util import HostObservations, exports
from test_isa_guards import _asm

EXT = _lib.POLICY_FULL_DEEP
NA, ND = policy.CLPF_NA, policy.CLPF_ND


@pytest.fixture(scope='module')
def entry():
    return DeepFullHostEntry(EXT, n_bldg=9, flags=0, n_act_cols=25)


def _district(name='g2020_cz1'):
    spec = thermal_district(name)
    return spec, spec.episode_tables(0), ObservationLayout(spec, 'current', True)


# ---- 1. the library -------------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header(entry):
    assert EXT.symbols == ['clpfd_abi_version', 'clpfd_core_abi_version', 'clpfd_last_error', 'clpfd_rollout_mlp_f32']
    assert exports(EXT.path) == EXT.symbols
    assert entry.lib.clpfd_abi_version() == EXT.abi_version == 1 and entry.lib.clpfd_core_abi_version() == abi.CL_ABI_VERSION
    assert policy.FULL_DEEP_CONSTANTS == {'CLPFD_ABI_VERSION': 1, 'CLPFD_MAX_HIDDEN': 32, 'CLPFD_MATRIX_CORES': 1}
    (src, flags), = EXT.sources
    assert src.name == 'cl_policy_full_deep.hip' and flags == ['-fno-slp-vectorize']       # (the translation unit says why, unlike cl_policy_full.hip)
    text = src.read_text()
    assert '#define CL_TU_POLICY\n#define CL_TU_POLICY_FULL\n' in text and 'CL_TU_NOSLP\n' not in text and '-fno-slp-vectorize' in text


def test_struct_layout_matches_the_header():
    text = abi._strip_comments(EXT.header.read_text())
    body = re.search(r'typedef\s+struct\s+clpfd_mlp\s*\{(.*?)\}\s*clpfd_mlp\s*;', text, flags=re.S).group(1)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            first, *more = decl.split(',')
            fields += [re.sub(r'\[.*\]|\*', '', part).strip() for part in [first.split()[-1], *more]]
    assert [f for f, _ in _lib.PolicyFullDeepMLP._fields_] == fields
    # clpf_mlp's fields first, under the same names (the shared host checks are templates over them), then the second layer
    full = _lib.PolicyFullMLP
    assert fields[:len(full._fields_)] == [f for f, _ in full._fields_] and fields[-3:] == ['n_hidden2', 'flags', 'l2']
    assert [(f, getattr(_lib.PolicyFullDeepMLP, f).offset) for f, _ in full._fields_] == [(f, getattr(full, f).offset) for f, _ in full._fields_]
    assert ctypes.sizeof(_lib.PolicyFullDeepMLP) == ctypes.sizeof(full) + 16 and _lib.PolicyFullDeepMLP.l2.offset == ctypes.sizeof(full) + 8


def test_the_extension_tuples():
    """The new tuple beside the pinned ones, the build expression, and the kind of its own."""
    assert _lib.DEEP_THERMAL_EXTENSIONS == (EXT,)
    every = _lib.ALL_EXTENSIONS + _lib.CHUNK_KPI_EXTENSIONS + _lib.LEAN_CHUNK_EXTENSIONS + _lib.DEEP_EXTENSIONS
    assert len(every) == 8 and EXT not in every and len({e.path for e in every + _lib.DEEP_THERMAL_EXTENSIONS}) == 9
    import inspect
    import __graft_entry__
    src = ' '.join(inspect.getsource(__graft_entry__.build).split())
    assert '_lib.ALL_EXTENSIONS + _lib.CHUNK_KPI_EXTENSIONS + _lib.LEAN_CHUNK_EXTENSIONS + _lib.DEEP_EXTENSIONS + _lib.DEEP_THERMAL_EXTENSIONS]' in src
    kind, thermal = policy.DeepStorageMLPPolicy.kind, policy.StorageMLPPolicy.kind
    assert kind.ext is EXT and kind.ext_kpi is None and kind.ext_chunk is None and kind.ext_chunk_kpi is None and kind.ext_chunk_pair is None
    assert kind.one_row_max == 16 and kind.n_planes == policy.CLPF_NT and kind.no_kpi_error is NotImplementedError
    assert kind.tables is policy.DeepStoragePolicyTables and kind.struct is _lib.PolicyFullDeepMLP and kind.max_hidden == 32
    assert (kind.terms, kind.head_slots, kind.head_shape, kind.refuse_device_actions, kind.only) == \
        (thermal.terms, thermal.head_slots, thermal.head_shape, True, thermal.only)
    assert policy.DeepStoragePolicyTables.kind is kind and policy.StoragePolicyTables.kind is thermal and thermal is not kind
    assert policy.DeepPolicyTables.kind is policy.DeepMLPPolicy.kind and policy.DeepMLPPolicy.kind is not kind


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_before_any_hip_call(entry):
    """Every refusal of the entry with its code and whole message, from a call on host memory: a call that reached a launch would not return one
    of these codes."""
    e = entry
    EINVAL, ENULL, EALIGN, ERANGE = abi.CL_EINVAL, abi.CL_ENULL, abi.CL_EALIGN, abi.CL_ERANGE
    P = 'clpfd_rollout_mlp_f32: '
    kind = lambda k: k << abi.CLD_REWARD_SHIFT
    H2MSG = 'n_hidden2=%d: the deep thermal policy kernel takes 4, 8, .. 32 units in its second hidden layer'
    FLAGS = 'clpfd_mlp.flags takes CLPFD_MATRIX_CORES only, .reserved must be 0'
    for d, kw, code, msg in (
            (e.dims(flags=abi.CLD_LEAN), {}, EINVAL, P + 'thermal / outage districts only; a battery + PV district (CLD_LEAN) with a two-hidden-layer policy '
                                                         'goes to clpd_rollout_mlp_f32 (libcitylearn_amd_policy_deep.so)'),
            (e.dims(n_bldg=17), {}, EINVAL, P + 'n_bldg=17 > 16 would be a building-chunked launch, which the deep thermal policy kernel is not '
                                                '(one workgroup row, one building per wave)'),
            (e.dims(flags=abi.CLD_F64_MAPS), {}, EINVAL, P + 'the battery map in fp32 or as the float64 chain (CLD_F64_CHAIN), not CLD_F64_MAPS'),
            (e.dims(flags=abi.CLD_KPI), {}, EINVAL, P + 'no streaming KPIs (CLD_KPI) inside this kernel -- record traj and replay CLPF_T_ACTION through '
                                                        'cl_rollout_seq_f32'),
            (e.dims(flags=abi.CLD_WRITE_DETAIL), {}, EINVAL, P + 'not with the detail planes (CLD_WRITE_DETAIL)'),
            (e.dims(flags=kind(abi.CLR_EV)), {}, EINVAL, P + 'reward kind CLR_EV needs the flexible-load tables'),
            (e.dims(env_pitch=128), {}, EINVAL, P + 'env_pitch=128 != n_env=64 is not implemented for this call'),
            (e.dims(n_act_cols=65537), {}, EINVAL, P + 'n_act_cols=65537 > 65536'),
            (e.dims(), dict(n_device_cols=2), EINVAL, P + 'n_device_cols=2: a building with a cooling / heating / combined device action column is not '
                                                          'covered (the policy has storage heads only)'),
            (e.dims(), dict(n_hidden=0), EINVAL, 'n_hidden=0: the policy kernel takes 4, 8, .. 32 hidden units'),
            (e.dims(), dict(n_hidden=6), EINVAL, 'n_hidden=6: the policy kernel takes 4, 8, .. 32 hidden units'),
            (e.dims(), dict(n_hidden=36), EINVAL, 'n_hidden=36: the policy kernel takes 4, 8, .. 32 hidden units'),
            (e.dims(), dict(n_sets=0), EINVAL, 'n_sets=0: at least one parameter set'),
            (e.dims(), dict(n_hidden2=0), EINVAL, H2MSG % 0),
            (e.dims(), dict(n_hidden2=10), EINVAL, H2MSG % 10),
            (e.dims(), dict(n_hidden2=36), EINVAL, H2MSG % 36),
            (e.dims(), dict(flags=2), EINVAL, FLAGS),
            (e.dims(), dict(flags=policy.CLPFD_MATRIX_CORES | 4), EINVAL, FLAGS),
            (e.dims(), dict(reserved=1), EINVAL, FLAGS),
            (e.dims(), dict(null='state'), ENULL, 'state is NULL'),
            (e.dims(), dict(odd='traj'), EALIGN, 'traj is not 16-byte aligned'),
            (e.dims(), dict(l2=None), ENULL, 'mlp.l2 is NULL'),
            (e.dims(), dict(l2=e.ODD), EALIGN, 'mlp.l2 is not 16-byte aligned'),
            (e.dims(), dict(set_of_block=e.ODD1), EALIGN, 'mlp.set_of_block is not 4-byte aligned'),
            (e.dims(), dict(t0=95), ERANGE, 'steps [95, 103) outside [0, 100)'),
            (e.dims(), dict(t0=-1), ERANGE, 'steps [-1, 7) outside [0, 100)'),
            (e.dims(), dict(k_steps=-1), ERANGE, 'steps [0, -1) outside [0, 100)'),
            (e.dims(tun=dict(nw=8)), {}, EINVAL, 'bad nw 8: the deep thermal policy rollout runs one building per wave (nw = n_bldg = 9, at most 16)'),
            (e.dims(n_bldg=5, tun=dict(nw=8)), {}, EINVAL, 'bad nw 8: the deep thermal policy rollout runs one building per wave (nw = n_bldg = 5, at most 16)'),
            (e.dims(tun=dict(vec=2)), {}, EINVAL, 'no deep thermal policy rollout kernel at 2 envs per lane: it runs at one env per lane'),
            (e.dims(tun=dict(vec=4)), {}, EINVAL, 'no deep thermal policy rollout kernel at 4 envs per lane')):
        assert e.call(d, **kw) == code and e.error() == msg, (kw, e.error())
    for name in ('pre', 'dep', 'out', 'act_low', 'act_high'):
        assert e.call(e.dims(), **{name: None}) == ENULL and e.error() == f'mlp.{name} is NULL'
    for name in ('pre', 'dep', 'out', 'net_reset', 'sigma'):
        assert e.call(e.dims(), **{name: e.ODD}) == EALIGN and e.error() == f'mlp.{name} is not 16-byte aligned'
    assert e.call(None) == ENULL and e.error() == 'dims is NULL'


def test_every_accepted_geometry_fits_a_cu():
    """The LDS of a workgroup, `_lib.policy_full_deep_lds_bytes` against the header's formula: a row is 5504 bytes at 32 x 32 in either family
    (the matrix-core row has that size at every H1, H2), so sixteen buildings need 104 448 bytes -- above the 64 KiB a launch gets without the
    opt-in, below the CU's 160 KiB: the entry's LDS refusal cannot be reached from an accepted (n_bldg, H1, H2), and `pack(matrix_cores=None)` has
    no fit to look after."""
    text = (_lib.CSRC / 'cl_policy_full_deep.h').read_text()
    assert 'return CLPF_ND * h1 + (h1 + 1) * h2 + CLPF_NA * h2 + CLPFD_TAILS;' in text and 'CLPFD_TAILS = 8 * CLPF_NA' in text
    assert 'return (size_t)nw * NQ * 64 + (size_t)nw * (mma ? CLPFD_M_ROW : clpfd_row_floats(h1, h2));' in text
    f = _lib.policy_full_deep_lds_bytes
    assert f(1, 32, 32) - f(1, 4, 4) == 4 * ((5 * 32 + 33 * 32 + 4 * 32) - (5 * 4 + 5 * 4 + 4 * 4)) and f(1, 4, 4) == 4 * (256 + 56 + 32)
    assert f(16, 32, 32) == f(16, 4, 4, True) == f(16, 32, 32, True) == 104448 and (f(16, 32, 32) - 16 * 1024) // 16 == 5504
    assert 64 * 1024 < f(16, 32, 32) < _lib.LDS_PER_CU == 163840 and f(10, 32, 32) == 65280 < 64 * 1024 < f(11, 32, 32) == 71808
    assert max(f(16, h1, h2, m) for h1 in range(4, 33, 4) for h2 in range(4, 33, 4) for m in (False, True)) == 104448


# ---- 3. the packer and the references -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['g2020_cz1', 't2'])
def test_packed_tables(name):
    """`pre` / `dep` and everything else of the first layer equal `StorageMLPPolicy.pack`'s for the same W1 / b1 bit for bit; `l2` / `out` against
    the formulas in float64 rounded once; the matrix-core layout round-trips as in tests/test_policy_deep_host.py."""
    spec, tab, layout = _district(name)
    B = len(spec.buildings)
    pol = make_deep_storage_policy(layout, 16, 32, n_sets=2, seed=3, sigma=0.1)
    pt = pol.pack(layout, tab, matrix_cores=False)
    assert isinstance(pt, policy.DeepStoragePolicyTables) and (pt.n_hidden, pt.n_hidden2, pt.n_sets, pt.n_bldg) == (16, 32, 2, B) and pt.matrix_cores is False
    front = policy.StorageMLPPolicy(pol.w1, pol.b1, np.ones((1, 1, NA, 16)), np.ones((1, 1, NA)), sigma=0.1).pack(layout, tab)
    for key in ('pre', 'dep', 'net_reset', 'act_low', 'act_high', 'sigma'):
        assert torch.equal(getattr(pt, key), getattr(front, key)), key
    for key in ('cols', 'low_bldg', 'high_bldg', 'sigma_bldg'):
        assert np.array_equal(getattr(pt, key), getattr(front, key)), key
    assert tuple(pt.dep.shape) == (2, B, ND, 16) and tuple(pt.l2.shape) == (2, B, 17, 32) and tuple(pt.out.shape) == (2, B, NA, 33)
    S = policy.ACT_SCALE
    _, _, w2, b2, w3, b3 = pol._full(B)
    f32 = lambda v: np.asarray(v, dtype=np.float64).astype(np.float32)
    assert np.array_equal(pt.l2.numpy()[:, :, :16], f32(S * w2.transpose(0, 1, 3, 2))) and np.array_equal(pt.l2.numpy()[:, :, 16], f32(S * b2))
    assert np.array_equal(pt.out.numpy()[..., :32], f32(w3)) and np.array_equal(pt.out.numpy()[..., 32], f32(b3))
    st = pt.struct(5)
    assert (st.n_hidden, st.n_sets, st.n_device_cols, st.reserved, st.n_hidden2, st.flags, st.seed) == (16, 2, 0, 0, 32, 0, 5) and st.l2 == pt.l2.data_ptr()
    # the matrix-core layout: `_l2_fragments` as `DeepMLPPolicy.pack` calls it, read back through `l2_fragments`
    pm = pol.pack(layout, tab, matrix_cores=True)
    assert pm.matrix_cores and pm.struct(0).flags == policy.CLPFD_MATRIX_CORES and tuple(pm.l2.shape) == (2, B, 1024 + 32 + 4)
    for key in ('pre', 'dep', 'out', 'net_reset', 'act_low', 'act_high'):
        assert torch.equal(getattr(pm, key), getattr(pt, key)), key
    assert np.array_equal(pm.l2.numpy(), policy._l2_fragments(np.array(w2) * S, np.array(b2) * S))
    t = pm.l2_fragments().astype(np.float64)                                   # [2 terms, S, B, 32, 32]
    tail = pm.l2.numpy()[:, :, 1024:].astype(np.float64)
    sw = 1.0 / (4096.0 * tail[:, :, 32])
    want = np.zeros((2, B, 32, 32))
    want[:, :, :32, :16] = S * w2
    amax = np.abs(want).max(axis=(2, 3))
    assert np.all(amax * sw >= 2.0 ** 13) and np.all(amax * sw < 2.0 ** 14) and np.all(tail[:, :, 33:] == 0)
    err = np.abs((t[0] + t[1] / 2048.0) / sw[:, :, None, None] - want)
    assert np.all(err <= (2.0 ** -22 + 2.0 ** -24) * np.abs(want) + 2.0 ** -27 * amax[:, :, None, None]) and np.all(t[:, :, :, :, 16:] == 0)
    assert np.allclose(tail[:, :, :32], 4096.0 * sw[:, :, None] * S * b2, rtol=2.0 ** -23, atol=0)
    sb = split_bound(pol, pm)
    print(f'{name} (16, 32): split_bound on the actions {sb:.3e}')
    assert 0 < sb < 1e-5
    if name == 't2':
        assert pt.cols[0, policy.CLPF_A_DS] >= 0 and pt.cols[1, policy.CLPF_A_DS] < 0 and not pt.dep[:, 1, policy.CLPF_D_DS].any()


def test_default_family_is_the_thermal_rule():
    """`pack(matrix_cores=None)` asks `default_thermal_matrix_cores`, a function of its own: `default_matrix_cores`'s rule was measured on another
    kernel and is not inherited.  The rule rests on the two probe logs the function's docstring quotes: the matrix-core family exactly for the
    shapes whose summary line reads "8 of 8 cases", the exact-fp32 family for every other measured shape -- read here from the committed logs."""
    import json
    spec, tab, layout = _district()
    assert policy.default_thermal_matrix_cores is not policy.default_matrix_cores
    measured = {}
    for name in ('policy_full_deep_probe.log', 'policy_full_deep_probe_shapes.log'):
        assert name in policy.default_thermal_matrix_cores.__doc__
        for line in (_lib.PKG.parent / 'profiles' / name).read_text().splitlines():
            rec = json.loads(line)
            if 'matrix_cores_faster_beyond_its_spread' in rec:
                measured[tuple(rec['shape'])] = rec['matrix_cores_faster_beyond_its_spread'] == '8 of 8 cases'
    assert len(measured) == 13 and {(16, 16): False, (32, 32): True}.items() <= measured.items()
    for shape, wins in measured.items():
        assert policy.default_thermal_matrix_cores(*shape) is wins and policy.default_thermal_matrix_cores(*shape, 16) is wins, shape
    for shape in ((4, 4), (16, 32)):
        assert make_deep_storage_policy(layout, *shape).pack(layout, tab).matrix_cores is measured.get(shape, False)
    # the fused launch against capture_rollout with the same MLP: faster by more than both spreads in every measured case
    last = json.loads((_lib.PKG.parent / 'profiles' / 'policy_full_deep_probe.log').read_text().splitlines()[-1])
    assert last == {'fused_faster_than_capture_rollout_beyond_both_spreads': '16 of 16 cases'}


def test_packer_surface():
    """`StorageMLPPolicy`'s surface: leading-1 broadcasting, `update` / `invalidate` / `version`, the packer's refusals (the first layer is packed
    by `StorageMLPPolicy.pack` itself -- a device-action column is refused by the thermal packer's message), and the shapes the constructor
    refuses."""
    spec, tab, layout = _district()
    shared = make_deep_storage_policy(layout, 8, 12, shared=True, seed=1, sigma=0.1)
    assert shared.w1.shape[1] == 1 and shared.version == 0
    pt = shared.pack(layout, tab, matrix_cores=False)
    assert pt.version == 0 and tuple(pt.l2.shape) == (1, 9, 9, 12) and bool((pt.l2 == pt.l2[:, :1]).all()) and np.all(pt.sigma_bldg[pt.cols >= 0] == 0.1)
    x = HostObservations(layout, tab, THERMAL_PLANES).at(3, *[np.full((9, 2), 0.5)] * 4, np.zeros((9, 2)))
    a0 = shared.actions_host(x, pt)
    assert a0.shape == (2, 9, NA) and not a0[:, pt.cols < 0].any() and a0[:, pt.cols >= 0].all()
    shared.update(w3=-shared.w3)
    assert shared.version == 1 and shared.pack(layout, tab).version == 1 and not np.array_equal(shared.actions_host(x, pt), a0)
    shared.invalidate()
    assert shared.version == 2
    with pytest.raises(ValueError, match='w2: shape'):
        shared.update(w2=np.zeros((1, 1, 12, 4)))
    with pytest.raises(ValueError, match='set_of_block outside'):
        shared.pack(layout, tab, set_of_block=[1])
    with pytest.raises(ValueError, match='do not broadcast to 1 sets x 9 buildings'):
        two = make_deep_storage_policy(layout, 8, 12)
        policy.DeepStorageMLPPolicy(two.w1[:, :2], two.b1, two.w2, two.b2, two.w3, two.b3).pack(layout, tab)
    z = np.zeros
    for shapes, msg in ((((1, 1, 8, 3), (1, 1, 8), (1, 1, 12, 8), (1, 1, 12), (1, 1, 12), (1, 1)), 'w3 .n_sets, n_bldg, 4, H2., b3 .n_sets, n_bldg, 4.'),
                        (((1, 1, 6, 3), (1, 1, 6), (1, 1, 12, 6), (1, 1, 12), (1, 1, 4, 12), (1, 1, 4)), 'H1=6'),
                        (((1, 1, 8, 3), (1, 1, 8), (1, 1, 36, 8), (1, 1, 36), (1, 1, 4, 36), (1, 1, 4)), 'H2=36'),
                        (((1, 1, 8, 3), (1, 1, 8), (1, 1, 12, 4), (1, 1, 12), (1, 1, 4, 12), (1, 1, 4)), 'about H1'),
                        (((1, 1, 8, 3), (1, 1, 8), (1, 1, 12, 8), (1, 1, 12), (1, 1, 4, 16), (1, 1, 4)), 'about H2'),
                        (((1, 1, 8, 3), (1, 1, 8), (1, 1, 12, 8), (1, 1, 12), (1, 1, 3, 12), (1, 1, 3)), 'do not have 4 heads')):
        with pytest.raises(ValueError, match=msg):
            policy.DeepStorageMLPPolicy(*[z(s) for s in shapes])
    with pytest.raises(ValueError, match='w1 takes 3 observations'):
        policy.DeepStorageMLPPolicy(z((1, 1, 8, 3)), z((1, 1, 8)), z((1, 1, 12, 8)), z((1, 1, 12)), z((1, 1, 4, 12)), z((1, 1, 4))).pack(layout, tab)
    # a building with a cooling DEVICE action: the thermal packer's refusal, through the first layer's pack
    params = np.array(tab.params, copy=True)
    params.view(np.int32)[2, abi.CLP_ACT_COOL_DEV] = 7
    from dataclasses import replace
    with pytest.raises(ValueError, match=r"action 'cooling_device' of building 2 \(column 7\): the thermal policy kernel has storage heads only"):
        make_deep_storage_policy(layout, 8, 12).pack(layout, replace(tab, params=params))


def test_actions_host_is_the_plain_mlp():
    """`actions_host` against a three-line numpy evaluation, noise and missing heads included; `torch_policy` in float64 against it."""
    spec, tab, layout = _district()
    pol = make_deep_storage_policy(layout, 12, 20, n_sets=2, seed=9, sigma=0.3)
    pt = pol.pack(layout, tab)
    rng = np.random.RandomState(1)
    B, E = 9, 6
    x = HostObservations(layout, tab, THERMAL_PLANES).at(17, *[rng.uniform(0, 1, size=(B, E)) for _ in range(4)], rng.uniform(-5, 30, size=(B, E)))
    z = rng.normal(size=(E, B, NA))
    s = 1
    h1 = np.tanh(np.einsum('bjc,ebc->ebj', pol.w1[s], x) + pol.b1[s])
    h2 = np.tanh(np.einsum('bij,ebj->ebi', pol.w2[s], h1) + pol.b2[s])
    o = np.tanh(np.einsum('bai,ebi->eba', pol.w3[s], h2) + pol.b3[s])
    want = np.clip(0.5 * (pt.high_bldg + pt.low_bldg) + 0.5 * (pt.high_bldg - pt.low_bldg) * o + pt.sigma_bldg * z, pt.low_bldg, pt.high_bldg)
    want = np.where(pt.cols >= 0, want, 0.0)
    got = pol.actions_host(x, pt, noise=z, set_index=s)
    assert got.shape == (E, B, NA) and np.abs(got - want).max() < 1e-15 and np.ptp(got[:, pt.cols >= 0]) > 0.1
    # torch_policy over the env's observation tensor, in float64, without noise
    from policy_full_util import scatter_heads
    hobs = HostObservations(layout, tab, THERMAL_PLANES)
    obs = np.zeros((E, len(layout.columns)))
    for b, cols in enumerate(hobs.cols):
        obs[:, cols] = x[:, b, :len(cols)]
    f = pol.torch_policy(layout, tab, 'cpu', dtype=torch.float64, set_index=s)
    acts = f(torch.from_numpy(obs)).numpy().astype(np.float64)
    ref = scatter_heads(pt, pol.actions_host(x, pt, set_index=s), acts.shape[0]).astype(np.float64)
    assert acts.shape == (25, E) and np.abs(acts - ref).max() < 1e-7 and np.abs(ref).max() > 0.01


# ---- 4. conditioning of the closed loop -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H1,H2', [(4, 4), (16, 32), (32, 32)])
@pytest.mark.parametrize('mma', [0, 1])
@pytest.mark.parametrize('name', ['g2020_cz1', 't1', 't2', 't16'])
def test_closed_loop_is_well_conditioned(name, mma, H1, H2):
    """tests/test_policy_full_host.py::test_closed_loop_is_well_conditioned for the deep test policies of the free-running GPU test, before any
    GPU run: the CPU oracle stepped K = 48 from reset with `actions_host` in float64, against the same loop with every action rounded through
    float32 and moved by the teacher-forced tolerance of the GPU test for that kernel family -- 4 x the worst deviation of a float32 torch
    evaluation on this trajectory's own observations, plus `split_bound` for the matrix-core family: every plane must stay within
    0.1 x (1e-4 + 1e-4 |ref|), while the policy does something.  Fixes policy_full_deep_util.FREE_MID_SCALE (readings there)."""
    spec, tab, layout = _district(name)
    K, E = 48, 4
    pol = make_deep_storage_policy(layout, H1, H2, seed=H1 + H2, mid_scale=FREE_MID_SCALE)
    pt = pol.pack(layout, tab, matrix_cores=bool(mma))
    ref = host_closed_loop(spec, tab, layout, pol, pt, K, E)
    hobs = HostObservations(layout, tab, THERMAL_PLANES)
    x = np.stack([hobs.at(t, *[ref[k][t - 1] for k in ('soc', 'cs', 'hs', 'ds', 'net')]) for t in range(1, K)])
    tol = 4.0 * f32_torch_deviation(pol, x, pt) + (split_bound(pol, pt) if mma else 0.0)
    got = host_closed_loop(spec, tab, layout, pol, pt, K, E, perturb=tol, round_f32=True)
    assert 0 < tol < 1e-5, tol
    act = ref['action'].transpose(0, 2, 3, 1)[:, pt.cols >= 0]
    assert np.abs(act).max() > 0.01 and np.ptp(act) > 0.02                                # a policy that does something
    for k in ('soc', 'cs', 'hs', 'ds', 'net'):
        err = float((np.abs(got[k] - ref[k]) / (1e-4 + 1e-4 * np.abs(ref[k]))).max())
        print(f'{name} ({H1}, {H2}) mma={mma} {k}: worst {err:.4f} x (1e-4 + 1e-4 |ref|), action tolerance {tol:.3e}, |action| max {np.abs(act).max():.3f}, '
              f'range {np.ptp(act):.3f}')
        assert err < 0.1, (name, k, err)


# ---- 5. generated code: resource figures only -----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def unit(tmp_path_factory):
    (src, flags), = EXT.sources
    return _asm(src, flags, tmp_path_factory)


def test_kernel_resources(unit):
    """Every instantiation the launcher can reach -- cl_rollout_full_policy_deep_kernel<PREC, MMA, MARL>: the fp32 map and the float64 chain, both
    families, without and with MARL -- keeps no scratch memory and at most 128 registers (a 1024-thread workgroup's cap)."""
    kernels, meta = unit
    names = [k for k in kernels if 'cl_rollout_full_policy_deep_kernel' in k]
    by = {tuple(int(x) for x in re.search(r'cl_rollout_full_policy_deep_kernelILi(\d)ELi(\d)ELb(\d)EE', k).groups()): k for k in names}
    assert sorted(by) == [(p, m, r) for p in (0, 2) for m in (0, 1) for r in (0, 1)] and len(names) == 8
    launcher = (_lib.CSRC / 'cl_policy_full_deep.hip').read_text()
    assert sorted(re.findall(r'CL_POLFD\((\d), (\d), (true|false)\);', launcher)) == sorted((str(p), str(m), 'true' if r else 'false') for p, m, r in by)
    for key, k in by.items():
        assert meta[k]['private_seg_size'] == 0, (key, meta[k])
        assert meta[k]['num_vgpr'] <= 128, (key, meta[k])
        print(key, meta[k])
