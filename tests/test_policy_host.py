"""The closed-loop policy rollout (`clpol_rollout_mlp_f32`, kernel `cl_rollout_policy_kernel` in csrc/cl_policy.h, library
``libcitylearn_amd_policy.so``) as far as it can be checked without a GPU: the library's symbol list and struct, the argument validation (before
any HIP call), the generated gfx950 code of every instantiation, the packer's split of the first layer against the unsplit MLP in float64, and
the conditioning of the closed loop the GPU tests run (tests/test_gpu_policy_rollout.py)."""
import ctypes
import re

import numpy as np
import pytest
import torch

from golden_util import golden
from citylearn_amd import _lib, abi, policy
from citylearn_amd.observations import ObservationLayout
from policy_util import HostObservations, exports, f32_torch_deviation, host_closed_loop, make_policy
from test_isa_guards import _asm, _count


@pytest.fixture(scope='module')
def lib():
    _lib.build_policy()
    lib = ctypes.CDLL(str(_lib.POLICY_LIB_PATH))
    lib.clpol_last_error.restype = ctypes.c_char_p
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.clpol_rollout_mlp_f32.argtypes = [ctypes.POINTER(_lib.Dims), vp, vp, vp, ctypes.POINTER(_lib.PolicyMLP), vp, vp, vp, vp, i32, i32, vp]
    return lib


# ---- 1. the library -------------------------------------------------------------------------------------------------------------------
def test_policy_library_exports_exactly_the_header(lib):
    assert _lib.POLICY_SYMBOLS == ['clpol_abi_version', 'clpol_core_abi_version', 'clpol_last_error', 'clpol_rollout_mlp_f32']
    assert exports(_lib.POLICY_LIB_PATH) == _lib.POLICY_SYMBOLS
    assert lib.clpol_abi_version() == _lib.POLICY_ABI_VERSION == 1 and lib.clpol_core_abi_version() == abi.CL_ABI_VERSION
    # the main library is what it was: its own symbols, nothing of this feature
    _lib.build()
    main = exports(_lib.LIB_PATH)
    assert main == abi.EXPORTED_SYMBOLS and not [s for s in main if 'clpol' in s]
    assert len(abi.EXPORTED_SYMBOLS) == 15 and not [k for k in abi.CONSTANTS if k.startswith('CLPOL')]


def test_policy_struct_layout_matches_the_header():
    text = abi._strip_comments(_lib.POLICY_HEADER.read_text())
    body = re.search(r'typedef\s+struct\s+clpol_mlp\s*\{(.*?)\}\s*clpol_mlp\s*;', text, flags=re.S).group(1)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            first, *more = decl.split(',')
            fields += [re.sub(r'\[.*\]|\*', '', part).strip() for part in [first.split()[-1], *more]]
    assert [f for f, _ in _lib.PolicyMLP._fields_] == fields
    assert ctypes.sizeof(_lib.PolicyMLP) == 16 + 8 * 8 + 8
    from test_abi import _doc_struct_fields                       # the stub INTEGRATION.md shows, executed
    stub = _doc_struct_fields('_PolicyMLP')
    assert [f for f, *_ in stub._fields_] == fields and ctypes.sizeof(stub) == ctypes.sizeof(_lib.PolicyMLP)
    assert policy.CLPOL_NT == 4 and sorted((policy.CLPOL_T_ACTION, policy.CLPOL_T_REWARD, policy.CLPOL_T_NET, policy.CLPOL_T_SOC)) == [0, 1, 2, 3]


def test_host_philox_is_the_library_stream():
    _lib.build()
    main = ctypes.CDLL(str(_lib.LIB_PATH))
    main.cl_philox_uniform.restype = ctypes.c_float
    main.cl_philox_uniform.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    for seed, col, t in ((0, 0, 0), (7, 3, 11), (2 ** 63 + 5, 16, 94), (policy.CLPOL_NOISE_KEY ^ 3, 2, 7)):
        env = np.arange(40) + 2 ** 31 - 20
        want = np.array([main.cl_philox_uniform(seed, int(e), col, t) for e in env], dtype=np.float64)
        assert np.array_equal(policy.philox_uniform_host(seed, env, col, t), want)
    z = np.concatenate([policy.noise_host(5, np.arange(4096), 1, t) for t in range(8)])
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02 and np.isfinite(z).all()


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------------
def _dims(n_env=64, n_bldg=17, flags=abi.CLD_LEAN, **kw):
    d = _lib.Dims(n_env, n_bldg, 100, n_bldg, flags)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(lib, d, *, t0=0, k_steps=8, state=True, traj_odd=False, **mlp_kw):
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data
    m = dict(n_hidden=16, n_sets=1, flags=0, reserved=0, pre=p, dep=p, out=p, set_of_block=None, net_reset=None, act_low=p, act_high=p, sigma=None, seed=1)
    m.update(mlp_kw)
    mlp = _lib.PolicyMLP(**m)
    return lib.clpol_rollout_mlp_f32(ctypes.byref(d) if d is not None else None, p, p, p if state else None, ctypes.byref(mlp), p, p, None,
                                     p + 4 if traj_odd else None, t0, k_steps, None)


def test_refusals_name_their_cause_before_any_hip_call(lib):
    err = lambda: lib.clpol_last_error().decode()
    EINVAL, ENULL, EALIGN, ERANGE = abi.CL_EINVAL, abi.CL_ENULL, abi.CL_EALIGN, abi.CL_ERANGE
    assert _call(lib, None) == ENULL and 'dims is NULL' in err()
    assert _call(lib, _dims(n_env=6)) == EALIGN and 'multiple of 4' in err()
    assert _call(lib, _dims(flags=0)) == EINVAL and 'CLD_LEAN' in err() and 'thermal' in err()
    assert _call(lib, _dims(n_bldg=33)) == EINVAL and 'n_bldg=33' in err() and 'chunked' in err()
    assert _call(lib, _dims(flags=abi.CLD_LEAN | abi.CLD_F64_MAPS)) == EINVAL and 'CLD_F64_MAPS' in err()
    assert _call(lib, _dims(flags=abi.CLD_LEAN | abi.CLD_KPI)) == EINVAL and 'CLD_KPI' in err() and 'traj' in err()
    assert _call(lib, _dims(flags=abi.CLD_LEAN | abi.CLD_WRITE_DETAIL)) == EINVAL and 'CLD_WRITE_DETAIL' in err()
    assert _call(lib, _dims(flags=abi.CLD_LEAN | (abi.CLR_EV << abi.CLD_REWARD_SHIFT))) == EINVAL and 'CLR_EV' in err()
    assert _call(lib, _dims(flags=abi.CLD_LEAN | (9 << abi.CLD_REWARD_SHIFT))) == EINVAL and 'unknown reward kind' in err()
    assert _call(lib, _dims(env_pitch=128)) == EINVAL and 'env_pitch=128' in err()
    for h in (0, 2, 6, 36, 64, -4):
        assert _call(lib, _dims(), n_hidden=h) == EINVAL and f'n_hidden={h}' in err()
    assert _call(lib, _dims(), n_sets=0) == EINVAL and 'n_sets=0' in err()
    for name in ('pre', 'dep', 'out', 'act_low', 'act_high'):
        assert _call(lib, _dims(), **{name: None}) == ENULL and f'mlp.{name} is NULL' in err()
    assert _call(lib, _dims(), state=False) == ENULL and 'state is NULL' in err()
    odd = np.zeros(64, dtype=np.float32).ctypes.data + 4
    for name in ('pre', 'dep', 'out', 'net_reset', 'sigma'):
        assert _call(lib, _dims(), **{name: odd}) == EALIGN and f'mlp.{name} is not 16-byte aligned' in err()
    assert _call(lib, _dims(), set_of_block=odd + 1) == EALIGN and 'set_of_block' in err()
    assert _call(lib, _dims(), traj_odd=True) == EALIGN and 'traj' in err()
    assert _call(lib, _dims(), t0=95) == ERANGE and '[95, 103)' in err()
    assert _call(lib, _dims(), t0=-1) == ERANGE and _call(lib, _dims(), k_steps=-1) == ERANGE
    tun = _lib.Tuning(vec=4)
    assert _call(lib, _dims(tuning=ctypes.pointer(tun))) == EINVAL and '4 envs per lane' in err()
    tun = _lib.Tuning(nw=8)                              # 17 buildings: 8 waves x 2 buildings < 17
    assert _call(lib, _dims(tuning=ctypes.pointer(tun))) == EINVAL and 'bad nw 8' in err()
    # ... and more waves than buildings: a wave without any building would read parameter row `w` and `net_reset[.. + w]` past the tables' end
    assert _call(lib, _dims(n_bldg=5, tuning=ctypes.pointer(tun))) == EINVAL and 'bad nw 8' in err()
    tun = _lib.Tuning(nw=2)
    assert _call(lib, _dims(n_bldg=1, tuning=ctypes.pointer(tun))) == EINVAL and 'bad nw 2' in err()


# ---- 3. generated code ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def policy_unit(tmp_path_factory):
    (src, flags), = _lib.POLICY_SOURCES
    assert flags == ['-fno-slp-vectorize']
    return _asm(src, flags, tmp_path_factory)


def test_policy_kernel_isa(policy_unit):
    """Every instantiation of cl_rollout_policy_kernel<VEC, PREC, KPI = false, CHUNK = false>: no scratch, no buffer instructions, no packed fp32, at most 128 registers (a
    1024-thread workgroup's cap), the float64 chain only under PREC = 2, the activation as v_exp_f32 / v_rcp_f32 -- and the policy tables not
    fetched per lane: inside the K loop `pre` comes through s_load_dwordx4 and `dep` / `out` through broadcast ds_read_b128 (three per building
    and group of four hidden units: six in the code, the loop is not unrolled).  The vector loads that remain, pinned as generated -- 17 in
    every instantiation: per building of a wave (two) the 3 state planes and the previous net (per-lane data; dwordx2 at two envs per lane: 8 of
    the 17) and the three staging reads of the launch prologue, in which lane j fetches hidden unit j's `dep` soc / net weight and output weight
    ON PURPOSE (one coalesced read per table instead of H scalar ones; lane 0's bias / bounds / sigma are scalar loads); inside the loop one per
    building, the capacity word CLP_L_CAP that the shared unit code of cl_unit.h reads through the parameter pointer (behind MARL's barrier the
    compiler fetches it per lane -- cl_rollout_kernel's loop has the same read); the 17th is the return row's read-modify-write of `ret_env`.
    A wave-uniform policy-table read that fell back to a per-lane fetch inside the loop would
    add to this count."""
    kernels, meta = policy_unit
    names = [k for k in kernels if 'cl_rollout_policy_kernel' in k]
    by = {tuple(int(x) for x in re.search(r'cl_rollout_policy_kernelILi(\d)ELi(\d)ELb0ELb0EE', k).groups()): k for k in names}
    assert sorted(by) == [(1, 0), (1, 2), (2, 0), (2, 2)] and len(names) == 4
    assert not [k for k in kernels if re.search(r'cl_rollout_policy_kernelILi\dELi\dELb\dELb\dEE', k) and 'ELb0ELb0EE' not in k]     # no KPI / CHUNK = true one here
    assert not [k for k in kernels if 'cl_rollout_kernel' in k or 'cl_rollout_kpi_kernel' in k or 'cl_step' in k]      # the unit holds its own kernel only
    for (vec, prec), k in by.items():
        ins = kernels[k]
        assert meta[k]['private_seg_size'] == 0, k
        assert meta[k]['num_vgpr'] <= 128, (k, meta[k])
        assert not [i for i in ins if i.startswith(('scratch_', 'buffer_'))], k
        assert not [i for i in ins if re.match(r'v_pk_\w+_f32', i)], k
        assert any(i.startswith('v_fma_f64') for i in ins) == (prec == 2), k
        assert _count(ins, 'v_exp_f32') >= 2 * vec and _count(ins, 'v_rcp_f32') >= 2 * vec, k
        assert _count(ins, 'global_load') == 17, (k, _count(ins, 'global_load'))
        assert _count(ins, 'global_load_dwordx2') == (8 if vec == 2 else 0), k
        assert _count(ins, 'ds_read_b128') == 6 and _count(ins, 's_load_dwordx4') >= 2, k
        assert _count(ins, 's_load') >= 30, (k, _count(ins, 's_load'))


# ---- 4. the packer --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('normalize', [True, False])
def test_split_first_layer_equals_the_unsplit_one(normalize):
    """`pre + dep x` rebuilt on the host from the packed float32 tables against `W1 obs + b1` in float64, for observation rows from
    `ObservationTables.host_row` with random state.  The bound is the tables' own rounding: every packed number carries one float32 rounding
    (2^-24 relative) of a term of the sum, so |error| <= 2^-23 (|pre| + |dep_soc soc| + |dep_net net|), taken with a factor 2."""
    spec = golden('g2022_all').spec()
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', normalize)
    pol = make_policy(layout, 16, n_sets=2, seed=3)
    pt = pol.pack(layout, tab)
    obs = layout.episode(tab, reset_table=True)
    cols = policy.building_columns(layout)
    rng = np.random.RandomState(0)
    B = len(cols)
    pre, dep = pt.pre.numpy().astype(np.float64) / policy.ACT_SCALE, pt.dep.numpy().astype(np.float64) / policy.ACT_SCALE
    assert pt.pre.shape == (2, tab.n_steps, B, 16) and pt.dep.shape == (2, B, 2, 16) and pt.out.shape == (2, B, 17)
    for r in (1, 2, 17, 100, tab.n_steps - 1):
        state, out_bldg = np.zeros((abi.CL_NS, B)), np.zeros((abi.CL_NO, B))
        state[abi.CLS_B_SOC] = rng.uniform(0, 1, B)
        out_bldg[abi.CLO_NET] = rng.uniform(-5, 8, B)
        row = obs.host_row(r, state=state, out_bldg=out_bldg)
        for s in range(2):
            for b in range(B):
                want = pol.w1[s, b] @ row[cols[b]] + pol.b1[s, b]
                terms = np.stack([pre[s, r, b], dep[s, b, 0] * state[abi.CLS_B_SOC, b], dep[s, b, 1] * out_bldg[abi.CLO_NET, b]])
                assert np.all(np.abs(terms.sum(axis=0) - want) <= 2.0 ** -22 * np.abs(terms).sum(axis=0) + 1e-30), (r, s, b)
    # the reset observation of an episode starting at row r: table row + dep x with the state's soc0 and net_reset[r]
    soc0 = tab.params_f32()[:, abi.CLP_B_SOC0].astype(np.float64)
    net_reset = pt.net_reset.numpy().astype(np.float64)
    for r in (0, 5):
        row = obs.reset_table[r] if r else obs.table[0]
        for b in range(B):
            want = pol.w1[0, b] @ row[cols[b]] + pol.b1[0, b]
            got = pre[0, r, b] + dep[0, b, 0] * soc0[b] + dep[0, b, 1] * net_reset[r, b]
            np.testing.assert_allclose(got, want, rtol=0, atol=2.0 ** -21 * (np.abs(pre[0, r, b]).max() + 10.0))
    # the output layer as it is: weights, bias last
    assert np.array_equal(pt.out.numpy()[:, :, :16], pol.w2.astype(np.float32)) and np.array_equal(pt.out.numpy()[:, :, 16], pol.b2.astype(np.float32))


@pytest.mark.parametrize('name, normalize', [('g2022_all', True), ('g2022_all', False), ('het17', True)])
def test_lean_policy_is_the_electrical_storage_slice_of_the_thermal_one(name, normalize):
    """`MLPPolicy` is the one-head, two-term case of `StorageMLPPolicy`: with the lean weights in head `CLPF_A_ES` (the other heads random: the
    district has no column for them) both packers give bit-identical `pre`, `net_reset`, bounds, `sigma` and `set_of_block`, the thermal `dep` rows
    `CLPF_D_SOC` / `CLPF_D_NET` are the lean rows 0 / 1, the rows of the three tanks are zero, head `CLPF_A_ES` of `out` is the lean `out`, and
    `actions_host` agrees to the last bit on a random batch with noise.

    het17 has the two places where the kinds differ by design, asserted as they are: (1) the lean soc term carries no flag gate, so the
    building WITHOUT a battery (`HET_NO_BATTERY`) keeps w1 . col_scale in its lean soc row (its soc plane stays 0, so the term adds nothing),
    where the thermal packer, which gates the term by `CLF_BATTERY`, writes 0; the building that keeps its battery but has no action
    (`HET_IDLE_ACTION`) has equal rows.  (2) for a building without an action column the lean `actions_host` returns the MLP's value (the
    kernel records 0 and the tests mask it), the thermal one 0."""
    from district_util import HET_NO_BATTERY, HET_UNDRIVEN, district
    spec = golden(name).spec() if name == 'g2022_all' else district(name)
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', normalize)
    H, ES = 8, policy.CLPF_A_ES
    lean = make_policy(layout, H, n_sets=2, seed=5, sigma=0.1)
    rng = np.random.RandomState(9)
    w2, b2 = rng.uniform(-1, 1, lean.w2.shape[:2] + (policy.CLPF_NA, H)), rng.uniform(-1, 1, lean.b2.shape + (policy.CLPF_NA,))
    w2[:, :, ES], b2[:, :, ES] = lean.w2, lean.b2
    thermal = policy.StorageMLPPolicy(lean.w1, lean.b1, w2, b2, sigma=0.1)
    a, b = lean.pack(layout, tab, set_of_block=[1, 0]), thermal.pack(layout, tab, set_of_block=[1, 0])
    for k in ('pre', 'net_reset', 'act_low', 'act_high', 'sigma', 'set_of_block'):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    B = a.n_bldg
    gated = [HET_NO_BATTERY] if name == 'het17' else []
    same = [i for i in range(B) if i not in gated]
    assert a.dep.shape == (2, B, 2, H) and b.dep.shape == (2, B, policy.CLPF_ND, H)
    assert torch.equal(a.dep[:, same, 0], b.dep[:, same, policy.CLPF_D_SOC]) and torch.equal(a.dep[:, :, 1], b.dep[:, :, policy.CLPF_D_NET])
    assert a.dep[:, same].abs().min() > 0
    if gated:
        assert not b.dep[:, gated, policy.CLPF_D_SOC].any() and a.dep[:, gated, 0].abs().min() > 0
    assert not b.dep[:, :, [policy.CLPF_D_CS, policy.CLPF_D_HS, policy.CLPF_D_DS]].any()
    assert torch.equal(a.out, b.out[:, :, ES])
    assert np.array_equal(b.cols[:, ES], a.es_cols) and np.all(np.delete(b.cols, ES, axis=1) == -1)
    for k in ('low_bldg', 'high_bldg', 'sigma_bldg'):
        assert np.array_equal(getattr(b, k)[:, ES], getattr(a, k)), k
    driven = a.es_cols >= 0
    assert sorted(np.nonzero(~driven)[0]) == (sorted(HET_UNDRIVEN) if name == 'het17' else [])
    x, z = rng.uniform(-1, 1, (5, B, lean.n_obs)), rng.normal(size=(5, B, policy.CLPF_NA))
    for s in (0, 1):
        got, want = thermal.actions_host(x, b, noise=z, set_index=s), lean.actions_host(x, noise=z[..., ES], tables=a, set_index=s)
        assert np.array_equal(got[:, driven, ES], want[:, driven]) and np.abs(want).min() > 0
        assert not got[:, ~driven].any() and not np.delete(got, ES, axis=2).any()


def test_packer_refuses_observations_it_cannot_feed():
    spec = golden('g2022_all').spec()
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    pol = make_policy(layout, 8)
    good = layout.episode

    def tampered(kind, plane, bldg, name):
        def episode(tab_, reset_table=False):
            o = good(tab_, reset_table=reset_table)
            c = [i for i, (b, k) in enumerate(layout.columns) if k == name and b == 3][0]
            o.col_src[c] = (kind << 28) | (plane << 20) | bldg
            return o
        return episode
    for kind, plane, bldg, name in ((0, abi.CLS_B_DEGCAP, 3, 'electrical_storage_soc'), (0, abi.CLS_B_SOC, 4, 'electrical_storage_soc'),
                                    (1, abi.CLO_REWARD, 3, 'net_electricity_consumption')):
        layout.episode = tampered(kind, plane, bldg, name)
        with pytest.raises(ValueError, match=name):
            pol.pack(layout, tab)
    del layout.episode
    # the reference's stale read of the t + 1 slots: the reset value is not in the table rows
    with pytest.raises(ValueError, match='reference'):
        pol.pack(ObservationLayout(spec, 'reference', True), tab)
    with pytest.raises(ValueError, match='H=6'):
        policy.MLPPolicy(np.zeros((1, 1, 6, 4)), np.zeros((1, 1, 6)), np.zeros((1, 1, 6)), np.zeros((1, 1)))
    with pytest.raises(ValueError, match='observations'):
        policy.MLPPolicy(np.zeros((1, 1, 8, 5)), np.zeros((1, 1, 8)), np.zeros((1, 1, 8)), np.zeros((1, 1))).pack(layout, tab)


# ---- 5. conditioning ------------------------------------------------------------------------------------------------------------------
def _conditioning(spec, H, K=48, E=4):
    """{'soc' | 'net': worst deviation of the perturbed loop in units of the plain bar}, the action tolerance and the reference trajectory."""
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    pol = make_policy(layout, H, seed=H)
    pt = pol.pack(layout, tab)
    ref = host_closed_loop(spec, tab, layout, pol, pt, K, E)
    hobs = HostObservations(layout, tab)
    x = np.stack([hobs.at(t, ref['soc'][t - 1], ref['net'][t - 1]) for t in range(1, K)])
    tol = 4.0 * f32_torch_deviation(pol, x, pt)
    got = host_closed_loop(spec, tab, layout, pol, pt, K, E, perturb=tol, round_f32=True)
    return {k: float((np.abs(got[k] - ref[k]) / (1e-4 + 1e-4 * np.abs(ref[k]))).max()) for k in ('soc', 'net')}, tol, ref, pt


@pytest.mark.parametrize('H', [4, 16, 32])
def test_closed_loop_is_well_conditioned(H):
    """The CPU oracle stepped K = 48 from reset on g2022_all with `actions_host` in float64, against the same loop with every action rounded
    through float32 and moved by the teacher-forced tolerance of the GPU test -- 4 x the worst deviation of a float32 torch evaluation of the
    unsplit MLP on this trajectory's own observations: soc and net must stay within 0.1 x (1e-4 + 1e-4 |ref|).  That makes the free-running GPU
    comparison (test_gpu_policy_rollout.py, (c)) a test of the kernel and not of a chaotic loop; it fixes policy_util's weight scale."""
    err, tol, ref, _ = _conditioning(golden('g2022_all').spec(), H)
    assert 0 < tol < 1e-5, tol
    assert np.abs(ref['action']).max() > 0.05 and np.ptp(ref['action']) > 0.1             # a policy that does something
    for k in ('soc', 'net'):
        print(f'H={H} {k}: worst {err[k]:.4f} x (1e-4 + 1e-4 |ref|), action tolerance {tol:.3e}')
        assert err[k] < 0.1, (k, err[k])


@pytest.mark.parametrize('H', [4, 16, 32])
@pytest.mark.parametrize('name', ['b1', 'b32', 'het17'])
def test_closed_loop_is_well_conditioned_on_the_geometry_districts(name, H):
    """The same condition, same weight scale and K = 48, on the districts of tests/district_util.py that the free-running GPU comparison of
    tests/test_gpu_rollout_geometry.py runs beyond g2022_all (the scale was chosen on the 17-building district only): one building, 32 jittered
    ones, and het17 with its undriven buildings (action 0, not perturbed: no column) and its zero-padded observation vector."""
    from district_util import HET_UNDRIVEN, district
    err, tol, ref, pt = _conditioning(district(name), H)
    assert 0 < tol < 1e-5, tol
    driven = pt.es_cols >= 0
    # a policy that does something: as on g2022_all where there are many buildings; b1 has ONE seeded draw of weights per H (|action| 0.016 at
    # H = 4), where all the closed loop needs is an action that is not 0 and moves with the observations
    act = ref['action'][:, driven]
    assert (np.abs(act).max() > 0.05 and np.ptp(act) > 0.1) if name != 'b1' else (np.abs(act).max() > 1e-3 and np.ptp(act) > 1e-4)
    if name == 'het17':
        assert sorted(np.nonzero(~driven)[0]) == sorted(HET_UNDRIVEN)
    for k in ('soc', 'net'):
        print(f'{name} H={H} {k}: worst {err[k]:.4f} x (1e-4 + 1e-4 |ref|), action tolerance {tol:.3e}')
        assert err[k] < 0.1, (name, k, err[k])


def test_ragged_observation_vectors_host_reference_equals_torch_policy():
    """het17's building with the shorter observation vector: `MLPPolicy.pack` zero-pads it, `torch_policy` masks it, `HostObservations` pads
    with zeros -- three statements of one thing.  In float64 on the CPU: (1) `actions_host` over `HostObservations` against `torch_policy` over
    the env's observation tensor (`ObservationTables.host_row`), every building, at 1e-12; (2) the packed first layer `pre + dep x` of the ragged
    building against `W1 x_padded + b1`, at the tables' own rounding (test_split_first_layer_equals_the_unsplit_one's bound).  The trailing
    first-layer weights of that building are NOT zero, so a padding that let any table value through would show."""
    from district_util import HET_SHORT_OBS, HET_UNDRIVEN, district
    spec = district('het17')
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    cols = policy.building_columns(layout)
    lengths = [len(c) for c in cols]
    n_obs = max(lengths)
    assert lengths[HET_SHORT_OBS] == n_obs - 1 and all(n == n_obs for i, n in enumerate(lengths) if i != HET_SHORT_OBS)
    pol = make_policy(layout, 16, seed=6)
    assert pol.n_obs == n_obs and np.abs(pol.w1[0, HET_SHORT_OBS, :, -1]).min() > 0
    pt = pol.pack(layout, tab)
    hobs = HostObservations(layout, tab)
    assert hobs.n_obs == n_obs and not hobs.mask[HET_SHORT_OBS, -1] and hobs.mask.sum() == sum(lengths)
    obs = layout.episode(tab, reset_table=True)
    f = pol.torch_policy(layout, tab, 'cpu', dtype=torch.float64)
    rng = np.random.RandomState(3)
    B, E = len(cols), 6
    pre, dep = pt.pre.numpy().astype(np.float64) / policy.ACT_SCALE, pt.dep.numpy().astype(np.float64) / policy.ACT_SCALE
    driven = pt.es_cols >= 0
    assert sorted(np.nonzero(~driven)[0]) == sorted(HET_UNDRIVEN)
    for r in (1, 7, 100):
        soc, net = rng.uniform(0, 1, (B, E)), rng.uniform(-5, 8, (B, E))
        rows = []
        for e in range(E):
            state, out_bldg = np.zeros((abi.CL_NS, B)), np.zeros((abi.CL_NO, B))
            state[abi.CLS_B_SOC], out_bldg[abi.CLO_NET] = soc[:, e], net[:, e]
            rows.append(obs.host_row(r, state=state, out_bldg=out_bldg))
        x = hobs.at(r, soc, net)                                                   # [E, B, n_obs]
        assert np.all(x[:, HET_SHORT_OBS, -1] == 0.0)
        want = f(torch.from_numpy(np.stack(rows))).numpy()                         # [n_act_cols, E] (float32 storage of float64 arithmetic)
        got = pol.actions_host(x, tables=pt)                                       # [E, B]
        assert want.shape == (int(driven.sum()), E)
        np.testing.assert_allclose(got[:, driven].T, want[pt.es_cols[driven]], rtol=0, atol=2.0 ** -22)
        b = HET_SHORT_OBS
        for e in range(E):
            unsplit = pol.w1[0, b] @ x[e, b] + pol.b1[0, b]
            terms = np.stack([pre[0, r, b], dep[0, b, 0] * soc[b, e], dep[0, b, 1] * net[b, e]])
            assert np.all(np.abs(terms.sum(axis=0) - unsplit) <= 2.0 ** -22 * np.abs(terms).sum(axis=0) + 1e-30), (r, e)


def test_pack_is_a_snapshot_and_the_policy_keeps_no_state():
    """`pack` leaves the policy object as it was (what `actions_host` needs travels on the tables), and `update` / `invalidate` bump the
    version `VectorCityLearnEnv.rollout_policy` keys its cache with."""
    spec = golden('g2022_all').spec()
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    pol = make_policy(layout, 8, sigma=0.1)
    before = dict(vars(pol))
    pt = pol.pack(layout, tab)
    assert vars(pol).keys() == before.keys() and all(vars(pol)[k] is before[k] for k in before)
    B = len(spec.buildings)
    assert pt.version == pol.version == 0 and pt.es_cols.shape == pt.low_bldg.shape == pt.high_bldg.shape == pt.sigma_bldg.shape == (B,)
    assert np.all(pt.low_bldg == -1.0) and np.all(pt.high_bldg == 1.0) and np.all(pt.sigma_bldg == 0.1)
    x = np.random.RandomState(0).uniform(0, 1, (5, B, pol.n_obs))
    z = np.random.RandomState(1).normal(size=(5, B))
    assert np.array_equal(pol.actions_host(x, noise=z, tables=pt), pol.actions_host(x, noise=z))          # scalar sigma, default bounds -1 / 1
    per_col = policy.MLPPolicy(pol.w1, pol.b1, pol.w2, pol.b2, sigma=np.linspace(0.0, 0.2, B))
    with pytest.raises(ValueError, match='tables'):
        per_col.actions_host(x, noise=z)
    assert np.array_equal(per_col.pack(layout, tab).sigma_bldg, np.linspace(0.0, 0.2, B))
    pol.update(w2=pol.w2 * 0.5)
    assert pol.version == 1 and pol.pack(layout, tab).version == 1 and not torch.equal(pol.pack(layout, tab).out, pt.out)
    pol.invalidate()
    assert pol.version == 2
    with pytest.raises(ValueError, match='shape'):
        pol.update(w1=np.zeros((1, 1, 8, 3)))
    assert 'policy.CLPOL_T_ACTION' in policy.__doc__ and 'abi.CLPOL' not in policy.__doc__
