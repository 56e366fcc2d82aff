"""The closed-loop policy rollout of thermal districts (`clpf_rollout_mlp_f32`, kernel `cl_rollout_full_policy_kernel` in csrc/cl_policy_full.h,
library ``libcitylearn_amd_policy_full.so``) as far as it can be checked without a GPU: the library's symbol list and struct, the argument
validation (before any HIP call), registers / scratch / LDS of every instantiation, the packer's five-plane split of the first layer against the
unsplit MLP in float64, its refusals, and the conditioning of the closed loop the GPU tests run (tests/test_gpu_policy_full_rollout.py)."""
import ctypes
import re

import numpy as np
import pytest
import torch

from golden_util import golden
from citylearn_amd import _lib, abi, policy
from citylearn_amd.observations import ObservationLayout
from policy_full_util import (OUTAGE_NAMES, THERMAL_PLANES, host_closed_loop, make_storage_policy, outage_district, outage_mask, outage_rows,
                              thermal_district)
from policy_util import HostObservations, exports, f32_torch_deviation
from test_isa_guards import _asm


@pytest.fixture(scope='module')
def lib():
    _lib.build_policy_full()
    lib = ctypes.CDLL(str(_lib.POLICY_FULL_LIB_PATH))
    lib.clpf_last_error.restype = ctypes.c_char_p
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.clpf_rollout_mlp_f32.argtypes = [ctypes.POINTER(_lib.Dims), vp, vp, vp, ctypes.POINTER(_lib.PolicyFullMLP), vp, vp, vp, vp, i32, i32, vp]
    return lib


# ---- 1. the library -------------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header(lib):
    assert _lib.POLICY_FULL_SYMBOLS == ['clpf_abi_version', 'clpf_core_abi_version', 'clpf_last_error', 'clpf_rollout_mlp_f32']
    assert exports(_lib.POLICY_FULL_LIB_PATH) == _lib.POLICY_FULL_SYMBOLS
    assert lib.clpf_abi_version() == _lib.POLICY_FULL_ABI_VERSION == 1 and lib.clpf_core_abi_version() == abi.CL_ABI_VERSION
    assert not [k for k in abi.CONSTANTS if k.startswith('CLPF')] and not [k for k in policy.CONSTANTS if k.startswith('CLPF')]


def test_struct_layout_matches_the_header():
    text = abi._strip_comments(_lib.POLICY_FULL_HEADER.read_text())
    body = re.search(r'typedef\s+struct\s+clpf_mlp\s*\{(.*?)\}\s*clpf_mlp\s*;', text, flags=re.S).group(1)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            first, *more = decl.split(',')
            fields += [re.sub(r'\[.*\]|\*', '', part).strip() for part in [first.split()[-1], *more]]
    assert [f for f, _ in _lib.PolicyFullMLP._fields_] == fields
    assert {'n_hidden', 'n_sets', 'pre', 'dep', 'out', 'set_of_block', 'net_reset', 'act_low', 'act_high', 'sigma', 'seed'} <= set(fields)
    assert ctypes.sizeof(_lib.PolicyFullMLP) == 16 + 8 * 8 + 8
    assert (policy.CLPF_NT, policy.CLPF_ND, policy.CLPF_NA) == (10, 5, 4)
    planes = [policy.CLPF_T_ACTION + a for a in range(4)] + [policy.CLPF_T_REWARD, policy.CLPF_T_NET] + [policy.CLPF_T_SOC + d for d in range(4)]
    assert sorted(planes) == list(range(10))
    assert (policy.CLPF_A_ES, policy.CLPF_A_CS, policy.CLPF_A_HS, policy.CLPF_A_DS) == (0, 1, 2, 3)


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------------
def _dims(n_env=64, n_bldg=9, flags=0, **kw):
    d = _lib.Dims(n_env, n_bldg, 100, 25, flags)
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
    return lib.clpf_rollout_mlp_f32(ctypes.byref(d) if d is not None else None, a['params'], a['ts'], p if state else None, ctypes.byref(mlp),
                                    a['out_bldg'], a['out_env'], None,
                                    p + 4 if traj_odd else None, t0, k_steps, None)


def test_refusals_name_their_cause_before_any_hip_call(lib):
    err = lambda: lib.clpf_last_error().decode()
    EINVAL, ENULL, EALIGN, ERANGE = abi.CL_EINVAL, abi.CL_ENULL, abi.CL_EALIGN, abi.CL_ERANGE
    assert _call(lib, None) == ENULL and 'dims is NULL' in err()
    assert _call(lib, _dims(n_env=6)) == EALIGN and 'multiple of 4' in err()
    assert _call(lib, _dims(flags=abi.CLD_LEAN)) == EINVAL and 'CLD_LEAN' in err() and 'clpol_rollout_mlp_f32' in err()
    assert _call(lib, _dims(n_bldg=17)) == EINVAL and 'n_bldg=17' in err() and 'chunked' in err()
    assert _call(lib, _dims(flags=abi.CLD_F64_MAPS)) == EINVAL and 'CLD_F64_MAPS' in err()
    assert _call(lib, _dims(flags=abi.CLD_KPI)) == EINVAL and 'CLD_KPI' in err()
    assert _call(lib, _dims(flags=abi.CLD_WRITE_DETAIL)) == EINVAL and 'CLD_WRITE_DETAIL' in err()
    assert _call(lib, _dims(flags=abi.CLR_EV << abi.CLD_REWARD_SHIFT)) == EINVAL and 'CLR_EV' in err()
    assert _call(lib, _dims(flags=9 << abi.CLD_REWARD_SHIFT)) == EINVAL and 'unknown reward kind' in err()
    assert _call(lib, _dims(), n_device_cols=2) == EINVAL and 'device action column' in err() and 'n_device_cols=2' in err()
    assert _call(lib, _dims(env_pitch=128)) == EINVAL and 'env_pitch=128' in err()
    for h in (0, 2, 6, 36, 64, -4):
        assert _call(lib, _dims(), n_hidden=h) == EINVAL and f'n_hidden={h}' in err()
    assert _call(lib, _dims(), n_sets=0) == EINVAL and 'n_sets=0' in err()
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
    tun = _lib.Tuning(vec=4)
    assert _call(lib, _dims(tuning=ctypes.pointer(tun))) == EINVAL and '4 envs per lane' in err()
    tun = _lib.Tuning(vec=2)                             # the chain and MARL run at one env per lane: named, not silently narrowed
    assert _call(lib, _dims(flags=abi.CLD_F64_CHAIN, tuning=ctypes.pointer(tun))) == EINVAL and 'CLD_F64_CHAIN' in err() and 'one env per lane' in err()
    assert _call(lib, _dims(flags=abi.CLR_MARL << abi.CLD_REWARD_SHIFT, tuning=ctypes.pointer(tun))) == EINVAL and 'CLR_MARL' in err()
    tun = _lib.Tuning(nw=10)                             # more waves than buildings: a wave without a building would read past the tables
    assert _call(lib, _dims(tuning=ctypes.pointer(tun))) == EINVAL and 'bad nw 10' in err()
    tun = _lib.Tuning(nw=17)
    assert _call(lib, _dims(n_bldg=16, tuning=ctypes.pointer(tun))) == EINVAL and 'bad nw 17' in err()
    tun = _lib.Tuning(nw=8)                              # ... and fewer would leave a building out
    assert _call(lib, _dims(tuning=ctypes.pointer(tun))) == EINVAL and 'bad nw 8' in err()


# ---- 3. generated code ----------------------------------------------------------------------------------------------------------------
def test_kernel_isa(tmp_path_factory):
    """Exactly the five instantiations of cl_rollout_full_policy_kernel<VEC, PREC, MARL, KPI = false, CHUNK = false> (csrc/cl_policy_full.h: reported
    as `cl_rollout_full_policy_kernel<VEC, PREC, MARL>`) and none of another variant in this unit: at most 128 VGPRs (a 1024-thread workgroup's cap), no scratch
    memory, no static LDS (it is all dynamic: `_lib.policy_full_lds_bytes`, within the CU's 160 KiB at the largest geometry)."""
    (src,) = _lib.POLICY_FULL_SOURCES
    kernels, meta = _asm(src, [], tmp_path_factory)
    names = [k for k in kernels if 'cl_rollout_full_policy_kernel' in k]
    by = {tuple(int(x) for x in re.search(r'cl_rollout_full_policy_kernelILi(\d)ELi(\d)ELb(\d)ELb0ELb0EE', k).groups()): k for k in names}
    assert sorted(by) == [(1, 0, 0), (1, 0, 1), (1, 2, 0), (1, 2, 1), (2, 0, 0)] and len(names) == 5
    assert not [k for k in kernels if re.search(r'cl_rollout_full_policy_kernelILi\dELi\dELb\dELb\dELb\dEE', k) and 'ELb0ELb0EE' not in k]     # no KPI / CHUNK = true one here
    for key, k in by.items():
        assert meta[k]['private_seg_size'] == 0, (k, meta[k])
        assert meta[k]['num_vgpr'] <= 128, (k, meta[k])
        print(key, meta[k])
    static = re.findall(r'\.group_segment_fixed_size:\s*(\d+)', next(tmp_path_factory.getbasetemp().glob('isa*/' + src.stem + '.s')).read_text())
    assert static and set(static) == {'0'}, static
    assert _lib.policy_full_lds_bytes(9, 2) == 4 * (9 * 4 * 128 + 9 * 320) == 29952
    assert _lib.policy_full_lds_bytes(16, 2) == 53248 <= 160 * 1024 and _lib.policy_full_lds_bytes(16, 1) == 36864


# ---- 4. the packer --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('normalize', [True, False])
def test_split_first_layer_equals_the_unsplit_one(normalize):
    """`pre + sum_d dep_d x_d` rebuilt on the host from the packed float32 tables against `W1 obs + b1` in float64, for observation rows from
    `ObservationTables.host_row` with random state: test_policy_host.py's bound for the two-plane split -- every packed number carries one
    float32 rounding of a term of the sum, |error| <= 2^-22 sum |terms|."""
    spec = golden('g2020_cz1').spec()
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', normalize)
    pol = make_storage_policy(layout, 16, n_sets=2, seed=3)
    pt = pol.pack(layout, tab)
    obs = layout.episode(tab, reset_table=True)
    cols = policy.building_columns(layout)
    rng = np.random.RandomState(0)
    B = len(cols)
    assert B == 9 and sorted(set(len(c) for c in cols)) == ([29, 30, 31] if normalize else [26, 27, 28])
    pre, dep = pt.pre.numpy().astype(np.float64) / policy.ACT_SCALE, pt.dep.numpy().astype(np.float64) / policy.ACT_SCALE
    assert pt.pre.shape == (2, tab.n_steps, B, 16) and pt.dep.shape == (2, B, 5, 16) and pt.out.shape == (2, B, 4, 17)
    planes = (abi.CLS_B_SOC, abi.CLS_CS_SOC, abi.CLS_HS_SOC, abi.CLS_DS_SOC)
    for r in (1, 2, 17, 100, tab.n_steps - 1):
        state, out_bldg = np.zeros((abi.CL_NS, B)), np.zeros((abi.CL_NO, B))
        for p in planes:
            state[p] = rng.uniform(0, 1, B)
        state[abi.CLS_DS_SOC, [2, 3]] = 0.0                        # (no DHW storage: the plane stays what reset left)
        state[abi.CLS_HS_SOC] = 0.0
        out_bldg[abi.CLO_NET] = rng.uniform(-5, 8, B)
        row = obs.host_row(r, state=state, out_bldg=out_bldg)
        x5 = np.stack([state[p] for p in planes] + [out_bldg[abi.CLO_NET]])         # [5, B]
        for s in range(2):
            for b in range(B):
                x = np.zeros(pol.n_obs)
                x[:len(cols[b])] = row[cols[b]]
                want = pol.w1[s, b] @ x + pol.b1[s, b]
                terms = np.concatenate([pre[s, r, b][None], dep[s, b] * x5[:, b, None]])
                assert np.all(np.abs(terms.sum(axis=0) - want) <= 2.0 ** -22 * np.abs(terms).sum(axis=0) + 1e-30), (r, s, b)
    # the heads' columns; buildings 2 and 3 have no DHW storage: a zero ds row, a head that is ignored; nobody has heating storage
    assert np.array_equal(pt.cols[:, policy.CLPF_A_HS], np.full(B, -1)) and np.array_equal(np.nonzero(pt.cols[:, policy.CLPF_A_DS] < 0)[0], [2, 3])
    assert np.all(pt.cols[:, [policy.CLPF_A_ES, policy.CLPF_A_CS]] >= 0) and sorted(pt.cols[pt.cols >= 0]) == list(range(25))
    assert not pt.dep[:, [2, 3], policy.CLPF_D_DS].any() and not pt.dep[:, :, policy.CLPF_D_HS].any()
    assert pt.dep[:, [0, 1, 4, 5, 6, 7, 8], policy.CLPF_D_DS].abs().min() > 0 and pt.dep[:, :, [policy.CLPF_D_SOC, policy.CLPF_D_CS, policy.CLPF_D_NET]].abs().min() > 0
    x = rng.uniform(0, 1, (5, B, pol.n_obs))
    a = pol.actions_host(x, pt)
    assert a.shape == (5, B, 4) and not a[:, :, policy.CLPF_A_HS].any() and not a[:, [2, 3], policy.CLPF_A_DS].any()
    changed = policy.StorageMLPPolicy(pol.w1, pol.b1, np.where(np.arange(4)[:, None] == policy.CLPF_A_HS, 9.0, pol.w2), pol.b2)
    assert np.array_equal(changed.actions_host(x, pt), a) and torch.equal(changed.pack(layout, tab).pre, pt.pre)
    # every building has its own bounds
    low, high = spec.action_limits()
    assert len(set(np.round(pt.high_bldg[:, policy.CLPF_A_CS], 6))) == B and np.array_equal(pt.high_bldg[pt.cols >= 0], np.asarray(high, dtype=np.float64)[pt.cols[pt.cols >= 0]])
    # the reset observation of an episode starting at row r: table row + dep x with the reset state (all storages start at soc 0 here) and net_reset[r]
    net_reset = pt.net_reset.numpy().astype(np.float64)
    for r in (0, 5):
        row = obs.reset_table[r] if r else obs.table[0]
        for b in range(B):
            x = np.zeros(pol.n_obs)
            x[:len(cols[b])] = row[cols[b]]
            want = pol.w1[0, b] @ x + pol.b1[0, b]
            got = pre[0, r, b] + dep[0, b, policy.CLPF_D_NET] * net_reset[r, b]
            np.testing.assert_allclose(got, want, rtol=0, atol=2.0 ** -21 * (np.abs(pre[0, r, b]).max() + 10.0))
    assert np.array_equal(pt.out.numpy()[:, :, :, :16], pol.w2.astype(np.float32)) and np.array_equal(pt.out.numpy()[:, :, :, 16], pol.b2.astype(np.float32))


def test_packer_refusals():
    """g2023_p2: the indoor temperature is fed by the LSTM stage (SRC_TEMP) and the buildings have device actions -- refused naming the column,
    the observation first; with the observation out of the way, the device action.  `MLPPolicy.pack` on g2020_cz1 raises as before."""
    spec = golden('g2023_p2').spec()
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    pol = make_storage_policy(layout, 8)
    with pytest.raises(ValueError, match=r"'indoor_dry_bulb_temperature\w*' of building 0 .*LSTM stage"):
        pol.pack(layout, tab)
    good = layout.episode

    def without_temperature(tab_, reset_table=False):
        # (every observation the stage or a detail plane feeds made env-independent: what is left to refuse is the action)
        o = good(tab_, reset_table=reset_table)
        for c in np.nonzero(o.col_src >= 0)[0]:
            kind, plane = int(o.col_src[c]) >> 28, (int(o.col_src[c]) >> 20) & 0xFF
            if (kind, plane) not in ((0, abi.CLS_B_SOC), (0, abi.CLS_CS_SOC), (0, abi.CLS_HS_SOC), (0, abi.CLS_DS_SOC), (1, abi.CLO_NET)):
                o.col_src[c] = -1
                if o.reset_table is not None:
                    o.reset_table[1:, c] = o.table[1:, c]
        return o
    layout.episode = without_temperature
    with pytest.raises(ValueError, match=r"action 'cooling\w*device' of building 0 \(column \d+\)"):
        pol.pack(layout, tab)
    del layout.episode
    # another building's plane, a detail plane
    spec = golden('g2020_cz1').spec()
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    pol = make_storage_policy(layout, 8)
    good = layout.episode

    def tampered(kind, plane, bldg, name):
        def episode(tab_, reset_table=False):
            o = good(tab_, reset_table=reset_table)
            c = [i for i, (b, k) in enumerate(layout.columns) if k == name and b == 3][0]
            o.col_src[c] = (kind << 28) | (plane << 20) | bldg
            return o
        return episode
    for kind, plane, bldg, name in ((0, abi.CLS_B_DEGCAP, 3, 'electrical_storage_soc'), (0, abi.CLS_CS_SOC, 4, 'cooling_storage_soc'),
                                    (1, abi.CLO_C_COOL, 3, 'net_electricity_consumption')):
        layout.episode = tampered(kind, plane, bldg, name)
        with pytest.raises(ValueError, match=name):
            pol.pack(layout, tab)
    del layout.episode
    with pytest.raises(ValueError, match='cooling_storage_soc'):
        from policy_util import make_policy
        make_policy(layout, 8).pack(layout, tab)
    with pytest.raises(ValueError, match='H=6'):
        policy.StorageMLPPolicy(np.zeros((1, 1, 6, 4)), np.zeros((1, 1, 6)), np.zeros((1, 1, 4, 6)), np.zeros((1, 1, 4)))
    with pytest.raises(ValueError, match='heads'):
        policy.StorageMLPPolicy(np.zeros((1, 1, 8, 4)), np.zeros((1, 1, 8)), np.zeros((1, 1, 3, 8)), np.zeros((1, 1, 3)))
    with pytest.raises(ValueError, match='observations'):
        policy.StorageMLPPolicy(np.zeros((1, 1, 8, 5)), np.zeros((1, 1, 8)), np.zeros((1, 1, 4, 8)), np.zeros((1, 1, 4))).pack(layout, tab)


# ---- 5. conditioning ------------------------------------------------------------------------------------------------------------------
def _conditioning(spec, H, K=48, E=4):
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    pol = make_storage_policy(layout, H, seed=H)
    pt = pol.pack(layout, tab)
    ref = host_closed_loop(spec, tab, layout, pol, pt, K, E)
    hobs = HostObservations(layout, tab, THERMAL_PLANES)
    x = np.stack([hobs.at(t, *[ref[k][t - 1] for k in ('soc', 'cs', 'hs', 'ds', 'net')]) for t in range(1, K)])
    tol = 4.0 * f32_torch_deviation(pol, x, pt)
    got = host_closed_loop(spec, tab, layout, pol, pt, K, E, perturb=tol, round_f32=True)
    return {k: float((np.abs(got[k] - ref[k]) / (1e-4 + 1e-4 * np.abs(ref[k]))).max()) for k in ('soc', 'cs', 'ds', 'net')}, tol, ref, pt


@pytest.mark.parametrize('H', [4, 16, 32])
@pytest.mark.parametrize('name', ['g2020_cz1', 't1', 't2', 't16'])
def test_closed_loop_is_well_conditioned(name, H):
    """The CPU oracle stepped K = 48 from reset with `actions_host` in float64, against the same loop with every action rounded through float32
    and moved by the teacher-forced tolerance of the GPU test (4 x the worst deviation of a float32 torch evaluation of the unsplit MLP on this
    trajectory's own observations): soc, cs, ds and net must stay within 0.1 x (1e-4 + 1e-4 |ref|).  That makes the free-running GPU comparison
    a test of the kernel and not of a chaotic loop; it fixes policy_full_util's weight scale.  Also on the geometry districts of test (h)."""
    err, tol, ref, pt = _conditioning(thermal_district(name), H)
    assert 0 < tol < 1e-5, tol
    act = ref['action'].transpose(0, 2, 3, 1)[:, pt.cols >= 0]
    assert np.abs(act).max() > 0.01 and np.ptp(act) > 0.02                                # a policy that does something
    for k in err:
        print(f'{name} H={H} {k}: worst {err[k]:.4f} x (1e-4 + 1e-4 |ref|), action tolerance {tol:.3e}')
        assert err[k] < 0.1, (k, err[k])


# ---- 6. the outage districts ----------------------------------------------------------------------------------------------------------
# The same measurement on `policy_full_util.outage_district` (tanks charged to 0.5, the battery as the schema has it; weight scale unchanged),
# worst of soc / cs / ds / net in units of the plain bar, K = 48, E = 4, as this test prints it -- `net` unless marked:
#   g2020_cz1_outage  H = 4: 0.0148   H = 16: 0.0145   H = 32: 0.0232
#   t1_outage               0.0023 cs         0.0117            0.0017
#   t2_outage               0.0039            0.0030 cs         0.0038
#   t16_outage              0.0123            0.0264            0.0262        maximum over the twelve cells: 0.026 (the project admits 0.1)
# soc <= 0.0045, cs <= 0.0076, ds 0.0000 (the tanks discharge at their demand, whatever the last bits of the action).  With 0.5 on all four
# storages the battery's gain takes g2020_cz1 H = 4 to 0.129: over the 0.1, not used.
@pytest.mark.parametrize('H', [4, 16, 32])
@pytest.mark.parametrize('name', OUTAGE_NAMES)
def test_closed_loop_is_well_conditioned_under_an_outage(name, H):
    """`test_closed_loop_is_well_conditioned` on the four outage districts, same condition: 0.1 x (1e-4 + 1e-4 |ref|)."""
    err, tol, ref, pt = _conditioning(thermal_district(name), H)
    assert 0 < tol < 1e-5, tol
    for k in err:
        print(f'{name} H={H} {k}: worst {err[k]:.4f} x (1e-4 + 1e-4 |ref|), action tolerance {tol:.3e}')
        assert err[k] < 0.1, (k, err[k])


def test_outage_district_leaves_its_source_alone():
    """The outage districts are copies: the cached plain districts, their storage specs and the series arrays they share keep their values, and
    every series but 'power_outage' is still the same array object."""
    for name in OUTAGE_NAMES:
        src = thermal_district(name[:-len('_outage')])
        specs = lambda b: repr((b.outage, b.cooling_storage, b.heating_storage, b.dhw_storage, b.electrical_storage))
        before = [(specs(b), b.series['power_outage'].copy()) for b in src.buildings]
        out = outage_district.__wrapped__(name[:-len('_outage')])          # built now, past the cache: `before` is a before
        assert out is not src and len(out.buildings) == len(src.buildings)
        start, _ = src.episode_window(0)
        for i, (b, c, was) in enumerate(zip(src.buildings, out.buildings, before)):
            assert c is not b and c.series is not b.series and c.outage is not b.outage
            assert specs(b) == was[0] != specs(c)
            assert not b.outage.simulate and c.outage.simulate and not c.outage.stochastic
            assert np.array_equal(b.series['power_outage'], was[1]) and not b.series['power_outage'].any()
            assert all(c.series[k] is b.series[k] for k in b.series if k != 'power_outage')
            assert np.array_equal(np.nonzero(c.series['power_outage'])[0] - start, outage_rows(i))
            for key in ('cooling_storage', 'heating_storage', 'dhw_storage'):
                assert getattr(b, key).initial_soc == 0.0 and getattr(c, key).initial_soc == (0.5 if getattr(b, key).capacity > 0 else 0.0)
            assert c.electrical_storage is b.electrical_storage
        tab = out.episode_tables(0)
        flags = tab.params[:, abi.CLP_FLAGS].view(np.int32)
        assert np.all(flags & abi.CLF_OUTAGE) and np.array_equal(tab.ts[:, :, abi.CLT_OUTAGE], tab.outage) and not tab.outage[0].any()
        assert not src.episode_tables(0).outage.any()


def test_outage_district_exercises_what_it_claims():
    """Read from the float64 oracle loop the GPU tests compare with (K = 48, H = 16, nine buildings): eleven outage rows for every building with
    i % 3 != 2 and none for the others; net exactly 0 on every outage (row, building) and nowhere else; battery soc, cooling tank and DHW tank each
    fall on an outage row (battery and cooling tank by more than their standing loss: a discharge); and the trajectory is not the plain district's."""
    K, E, H = 48, 4, 16
    spec = thermal_district('g2020_cz1_outage')
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    pol = make_storage_policy(layout, H, seed=H)
    pt = pol.pack(layout, tab)
    ref = host_closed_loop(spec, tab, layout, pol, pt, K, E)
    m = outage_mask(tab, K)
    assert m.shape == (K, 9) and np.array_equal(m.sum(axis=0), [0 if i % 3 == 2 else 11 for i in range(9)])
    assert not ref['net'][m].any() and np.all(ref['net'][~m] != 0.0)
    loss = {'soc': [b.electrical_storage.loss_coefficient for b in spec.buildings], 'cs': [b.cooling_storage.loss_coefficient for b in spec.buildings]}
    for k in ('soc', 'cs', 'ds'):
        drop = float((ref[k][1:] - ref[k][:-1])[m[1:]].min())
        print(f'{k}: largest fall on an outage row {drop:.5f}')
        assert drop < -1e-4, (k, drop)
        if k in loss:                  # ... and below what the standing loss alone leaves: a discharge
            drop = float((ref[k][1:] - ref[k][:-1] * (1.0 - np.asarray(loss[k])[None, :, None]))[m[1:]].min())
            print(f'{k}: largest discharge on an outage row {drop:.5f}')
            assert drop < -1e-4, (k, drop)
    # (the DHW tank's fall IS its standing loss, 0.5 x 0.0077 a step: the reference sizes a DHW storage action by the HEATING tank's capacity,
    # building.py:1765, which is 0 in this district -- so the plane moves under the outage branch, by the loss term only)
    assert np.ptp(ref['ds'][:, [0, 1, 4, 6, 7]]) > 0.1 and not ref['ds'][:, [2, 3]].any() and not ref['hs'].any()
    plain_spec = thermal_district('g2020_cz1')
    plain_tab = plain_spec.episode_tables(0)
    plain = host_closed_loop(plain_spec, plain_tab, layout, pol, pol.pack(layout, plain_tab), K, E)
    diff = np.abs(plain['net'] - ref['net'])
    bar = float((diff / (1e-4 + 1e-4 * np.abs(ref['net'])))[5:].max())
    print(f'plain district against the outage district: |net| differs by up to {diff[5:].max():.2f} kWh, {bar:.3g} x the plain bar')
    assert diff[5:].max() > 1.0 and bar > 1e4


@pytest.mark.parametrize('kind', ['RewardFunction', 'MARL', 'IndependentSACReward', 'SolarPenaltyReward'])
def test_c_and_python_oracles_agree_under_a_thermal_outage(kind):
    """tests/test_oracle_golden.py::test_c_and_python_oracles_agree_on_random_batch's construction, tolerances and four assertions on the
    nine-building outage district, rows 0 .. 47: the line-by-line restatement (bit-exact on the reference fixtures) against the C port on a
    cooling tank, a DHW tank and a battery in one building under an outage -- the reference the GPU outage tests lean on.

    [MARL] is the sharp case: step 21, env 2 has nine rewards of +7784.85 down to -2912.12 (each 0.01 net^2 x district net) whose sum cancels to
    74.78, so one float32 ulp of a building's net (6e-8 relative, 5e-4 on the largest term) is over the district reward's bound of 2.5e-4.
    The bound holds because cl_oracle.c states the reference's float32 / double promotions the way oracle.py has them by construction (a building's
    consumptions summed in double: building.py:2685-2693, 640-668; float32 balance / COP quotients: building.py:1641-1782, 2618-2652).  From reset
    the two are therefore equal bit for bit in net, the three socs that move, the consumptions, the battery's energy balance, efficiency and
    degraded capacity, and the last assertion of the loop keeps that so."""
    from oracle.c_oracle import COracle, OO, OS
    from oracle.oracle import DistrictOracle
    spec = thermal_district('g2020_cz1_outage')
    tab = spec.episode_tables(0)
    E = 3
    low, high = spec.action_limits()
    rng = np.random.RandomState(11)
    po, co = DistrictOracle(spec, tab, E, reward=kind), COracle(spec, tab, E, reward=kind)
    po.reset()
    m = outage_mask(tab, 48)
    for t in range(48):
        a = rng.uniform(low[:, None], high[:, None], size=(len(low), E)).astype(np.float32)
        a[:, 0] = np.where(rng.rand(len(low)) < 0.3, 0.0, a[:, 0])
        a[:, 1] = np.where(rng.rand(len(low)) < 0.5, low, high)
        p = po.step(a)
        out, oe = co.step(a, t)
        np.testing.assert_allclose(out[:, :, OO['NET']].T, p['net'], rtol=2e-6, atol=2e-5)
        np.testing.assert_allclose(co.state[:, :, OS['SOC']].T, p['soc'], rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(out[:, :, OO['REWARD']].T, p['reward'], rtol=2e-6, atol=2e-5)
        np.testing.assert_allclose(oe[:, 3], p['d_reward'], rtol=2e-6, atol=1e-4)
        # (not asked of the 2023 fixture: the tanks, and the outage rows themselves)
        np.testing.assert_allclose(co.state[:, :, OS['CS']].T, p['cs_soc'], rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(co.state[:, :, OS['DS']].T, p['ds_soc'], rtol=2e-6, atol=2e-6)
        assert not p['net'][m[t]].any() and not out[:, m[t], OO['NET']].any() and np.all(p['net'][~m[t]] != 0.0)
        for got, key in ((out[:, :, OO['NET']], 'net'), (co.state[:, :, OS['SOC']], 'soc'), (co.state[:, :, OS['CS']], 'cs_soc'), (co.state[:, :, OS['DS']], 'ds_soc'),
                         (out[:, :, OO['C_COOL']], 'c_cool'), (out[:, :, OO['C_DHW']], 'c_dhw'), (out[:, :, OO['C_NS']], 'c_ns'), (out[:, :, OO['EB']], 'eb'),
                         (co.state[:, :, OS['EFF']], 'eff'), (co.state[:, :, OS['DEGCAP']], 'degcap')):
            assert np.array_equal(got.T.astype(np.float32), p[key]), (t, key)


def test_pack_is_a_snapshot_and_the_policy_keeps_no_state():
    spec = golden('g2020_cz1').spec()
    tab = spec.episode_tables(0)
    layout = ObservationLayout(spec, 'current', True)
    pol = make_storage_policy(layout, 8, sigma=0.1)
    before = dict(vars(pol))
    pt = pol.pack(layout, tab)
    assert isinstance(pt, policy.StoragePolicyTables) and pt.n_device_cols == 0
    assert vars(pol).keys() == before.keys() and all(vars(pol)[k] is before[k] for k in before)
    B = len(spec.buildings)
    assert pt.version == pol.version == 0 and pt.cols.shape == pt.low_bldg.shape == pt.high_bldg.shape == pt.sigma_bldg.shape == (B, 4)
    assert np.all(pt.sigma_bldg[pt.cols >= 0] == 0.1) and not pt.sigma_bldg[pt.cols < 0].any()
    sig = np.linspace(0.0, 0.2, 25)
    per_col = policy.StorageMLPPolicy(pol.w1, pol.b1, pol.w2, pol.b2, sigma=sig)
    ppt = per_col.pack(layout, tab)
    assert np.array_equal(ppt.sigma_bldg[ppt.cols >= 0], sig[ppt.cols[ppt.cols >= 0]]) and np.array_equal(ppt.sigma.numpy(), sig.astype(np.float32))
    with pytest.raises(ValueError, match='sigma'):
        policy.StorageMLPPolicy(pol.w1, pol.b1, pol.w2, pol.b2, sigma=np.zeros(9)).pack(layout, tab)
    pol.update(w2=pol.w2 * 0.5)
    assert pol.version == 1 and pol.pack(layout, tab).version == 1 and not torch.equal(pol.pack(layout, tab).out, pt.out)
    pol.invalidate()
    assert pol.version == 2
    with pytest.raises(ValueError, match='shape'):
        pol.update(w1=np.zeros((1, 1, 8, 3)))
    shared = make_storage_policy(layout, 8, shared=True)
    assert shared.pack(layout, tab).dep.shape == (1, B, 5, 8)
    assert 'StorageMLPPolicy' in policy.__doc__ and 'CLPF_T_ACTION' in policy.__doc__
