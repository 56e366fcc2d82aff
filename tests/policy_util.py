"""Shared by the policy tests: the lean test policies (ONE weight scale, fixed by the CPU conditioning test of tests/test_policy_host.py) and their
closed loop on the CPU oracle; for both policies (tests/policy_full_util.py has the thermal rest) the observation vectors of a batch rebuilt
on the host from `ObservationTables` and the float32 torch evaluation's deviation."""
import numpy as np
import torch

from citylearn_amd import abi
from citylearn_amd.observations import SRC_OUT, SRC_STATE, ObservationLayout
from citylearn_amd.policy import MLPPolicy, building_columns

# The weight scale of every test policy: first-layer rows uniform in +-W1_SCALE / sqrt(n_obs), output rows uniform in +-W2_SCALE / sqrt(H).
# Chosen on the CPU, before any GPU run, by test_policy_host.py::test_closed_loop_is_well_conditioned: an action error of the teacher-forced
# tolerance reaches `net` directly through the battery's nominal power (kW per action unit) and comes back through the policy's soc / net
# weights; at (1, 1) the perturbed oracle loop moved net by up to 0.18 x the plain bar over 48 steps, at (0.5, 1) by 0.10, at (0.25, 0.5)
# by 0.04 (H = 4 / 16 / 32) -- the scale the issue's 0.1 x condition admits with room.  Actions still span about -0.36 .. 0.31 of [-1, 1].
W1_SCALE, W2_SCALE = 0.25, 0.5


def make_policy(layout: ObservationLayout, H: int, n_sets: int = 1, seed: int = 0, sigma=None, shared: bool = False) -> MLPPolicy:
    n_obs = max(len(n) for n in layout.building_names)
    nb = 1 if shared else len(layout.building_names)
    rng = np.random.RandomState(1000 + seed)
    w1 = rng.uniform(-1, 1, size=(n_sets, nb, H, n_obs)) * W1_SCALE / np.sqrt(n_obs)
    b1 = rng.uniform(-0.5, 0.5, size=(n_sets, nb, H))
    w2 = rng.uniform(-1, 1, size=(n_sets, nb, H)) * W2_SCALE / np.sqrt(H)
    b2 = rng.uniform(-0.2, 0.2, size=(n_sets, nb))
    return MLPPolicy(w1, b1, w2, b2, sigma=sigma)


# the planes of the state / output arrays the lean policy's two terms read: soc, previous net
LEAN_PLANES = ((SRC_STATE, abi.CLS_B_SOC), (SRC_OUT, abi.CLO_NET))


class HostObservations:
    """Observation vectors [E, n_bldg, n_obs] of a batch at table row r from the env-dependent planes [n_bldg, E] each (float64), in the order
    of `planes` ((source kind, plane) pairs; by default the lean policy's soc and previous net): the arithmetic of
    `ObservationTables.host_row` (row + plane * col_scale for the env-dependent columns; row 0 / the reset table as they are), vectorised.
    A building whose own vector is shorter than `n_obs` (the longest one) is padded at the end, and the padding is multiplied by zero -- what
    `pack` feeds the first layer's trailing weights of such a building (its `x` / `scale` rows stay 0 there)."""

    def __init__(self, layout: ObservationLayout, tab, planes=LEAN_PLANES):
        self.obs = layout.episode(tab, reset_table=True)
        self.cols = building_columns(layout)
        self.n_obs = max(len(c) for c in self.cols)
        self.lengths = np.array([len(c) for c in self.cols])
        self.idx = np.array([c + [c[0]] * (self.n_obs - len(c)) for c in self.cols])          # [B, n_obs] (padding: any valid column, masked)
        self.mask = np.arange(self.n_obs)[None, :] < self.lengths[:, None]                    # [B, n_obs]
        src = self.obs.col_src[self.idx]
        kind, plane = src >> 28, (src >> 20) & 0xFF
        self.is_term = [self.mask & (src >= 0) & (kind == k) & (plane == p) for k, p in planes]
        assert np.array_equal(self.mask & (src >= 0), np.logical_or.reduce(self.is_term))
        assert np.array_equal((src & 0xFFFFF)[self.mask & (src >= 0)], np.broadcast_to(np.arange(len(self.cols))[:, None], src.shape)[self.mask & (src >= 0)])
        self.scale = self.obs.col_scale[self.idx].astype(np.float64)

    def at(self, r: int, *planes, reset: bool = False, E: int = None):
        """`planes`: one array per term.  `reset`: the observation `reset()` returns for an episode that starts at row r (the planes are not
        read; E from the first one unless given)."""
        E = np.shape(planes[0])[1] if E is None else E
        if reset:
            row = (self.obs.reset_table[r] if r else self.obs.table[0])[self.idx] * self.mask
            return np.broadcast_to(row[None], (E,) + self.idx.shape).copy()
        x = np.broadcast_to((self.obs.table[r][self.idx] * self.mask)[None], (E,) + self.idx.shape).copy()
        for is_d, v in zip(self.is_term, planes, strict=True):
            x += np.where(is_d, np.asarray(v, dtype=np.float64).T[:, :, None] * self.scale, 0.0)
        return x


def host_closed_loop(spec, tab, layout, policy, pt, K, E, reward='RewardFunction', perturb=None, seed=0, env_offset=0, round_f32=False):
    """K steps from reset of the CPU oracle (float64) driven by `policy.actions_host` on the observations the env would hand out (`pt`:
    the policy's `pack` over these tables -- the buildings' action columns, bounds and sigmas; any device).
    `perturb` (float): every action is moved by +-perturb (a fixed random sign per (step, building, env)).  Returns a dict of [K, n_bldg, E]
    arrays (district net: [K, E])."""
    from oracle.c_oracle import COracle, OS, OO
    from citylearn_amd.policy import noise_host
    ora = COracle(spec, tab, E, reward=reward)
    hobs = HostObservations(layout, tab)
    pt_low, pt_high, es = pt.low_bldg, pt.high_bldg, pt.es_cols
    B = len(spec.buildings)
    out = {k: np.zeros((K, B, E)) for k in ('action', 'soc', 'degcap', 'net', 'reward')}
    out['dnet'] = np.zeros((K, E))
    rng = np.random.RandomState(77)
    sig = pt.sigma_bldg
    for t in range(K):
        if t == 0:
            x = hobs.at(0, np.zeros((B, E)), None, reset=True)
        else:
            x = hobs.at(t, ora.state[:, :, OS['SOC']].T, ora.out[:, :, OO['NET']].T)
        z = None
        if np.any(sig > 0):
            z = np.stack([noise_host(seed, env_offset + np.arange(E), es[b], t) if sig[b] > 0 else np.zeros(E) for b in range(B)], axis=1)
        a = policy.actions_host(x, noise=z, tables=pt)                        # [E, B]
        if round_f32:
            a = a.astype(np.float32).astype(np.float64)
        if perturb:
            a = np.clip(a + perturb * rng.choice([-1.0, 1.0], size=a.shape), pt_low, pt_high)
        acts = np.zeros((ora.n_act_cols, E), dtype=np.float32)
        acts[es[es >= 0]] = a.T[es >= 0]
        o, oe = ora.step(acts, t)
        out['action'][t] = a.T
        out['soc'][t] = ora.state[:, :, OS['SOC']].T
        out['degcap'][t] = ora.state[:, :, OS['DEGCAP']].T
        out['net'][t] = o[:, :, OO['NET']].T
        out['reward'][t] = o[:, :, OO['REWARD']].T
        out['dnet'][t] = oe[:, 0]
    return out


def f32_torch_deviation(pol, x, pt, device='cpu', noise=None):
    """max |float32 torch evaluation of the unsplit MLP - float64| on observation vectors x [..., B, n_obs], for either policy; with a head
    axis, over the heads that exist (`noise`: the standard normals, shaped like the actions, handed to both evaluations; `pt`: the policy's
    `pack`, for the bounds, sigmas and columns)."""
    ref = pol.actions_host(x, tables=pt, noise=noise)
    t = lambda v: torch.as_tensor(np.array(v), dtype=torch.float32, device=device)
    w1, b1, w2, b2 = (t(v[0]) for v in pol._full(x.shape[-2]))
    h = torch.tanh(torch.einsum('bjc,...bc->...bj', w1, t(x)) + b1)
    lo, hi = t(pt.low_bldg), t(pt.high_bldg)
    a = 0.5 * (hi + lo) + 0.5 * (hi - lo) * torch.tanh(pol._heads_torch(w2, h) + b2)
    if noise is not None:
        a = a + t(pt.sigma_bldg) * t(noise)
    d = np.abs(torch.clamp(a, lo, hi).cpu().numpy().astype(np.float64) - ref)
    return float((np.where(pt.cols >= 0, d, 0.0) if pol.kind.head_shape else d).max())


class HostEntry:
    """The entry point of one policy extension (a `_lib._Extension`) called on 256 bytes of HOST memory, for the refusals that come back before
    any HIP call: a call that got as far as a launch would not return one of the argument codes.  `n_bldg`, `flags`, `n_act_cols` are the
    defaults of `dims()`; `call()` returns the code, `error()` the library's message."""
    BUFFERS = ('params', 'ts', 'state', 'out_bldg', 'out_env', 'ret_env', 'traj', 'kpi_bldg', 'kpi_env', 'series_scratch')
    ODD, ODD1 = 'odd', 'odd1'              # a pointer value of `call`'s mlp fields: the buffer + 4 bytes / + 5 bytes

    def __init__(self, ext, n_bldg, flags=0, n_act_cols=None):
        import ctypes
        from citylearn_amd import _lib
        self.ext, self.defaults = ext, dict(n_bldg=n_bldg, flags=flags, n_act_cols=n_act_cols)
        ext.build()
        self.lib = lib = ctypes.CDLL(str(ext.path))
        vp, i32 = ctypes.c_void_p, ctypes.c_int32
        getattr(lib, f'{ext.prefix}_last_error').restype = ctypes.c_char_p
        self.entry = getattr(lib, f'{ext.prefix}_{ext.entry}')
        self.entry.argtypes = [ctypes.POINTER(_lib.Dims), vp, vp, vp, ctypes.POINTER(ext.mlp), vp, vp, vp, vp, *[vp] * ext.n_kpi, *ext.extra, i32, i32, vp]
        for fname, restype, argtypes in ext.functions:
            fn = getattr(lib, f'{ext.prefix}_{fname}')
            fn.restype, fn.argtypes = restype, list(argtypes)

    def error(self):
        return getattr(self.lib, f'{self.ext.prefix}_last_error')().decode()

    def dims(self, n_env=64, tun=None, **kw):
        """`cl_dims` of 100 steps; `tun`: the fields of a `cl_tuning` to hang on it; any other field by name."""
        import ctypes
        from citylearn_amd import _lib
        f = {**self.defaults, **kw}
        d = _lib.Dims(n_env, f.pop('n_bldg'), 100, 0, f.pop('flags'))
        n_act_cols = f.pop('n_act_cols')
        d.n_act_cols = d.n_bldg if n_act_cols is None else n_act_cols
        for k, v in f.items():
            setattr(d, k, v)
        if tun is not None:
            d.tuning = ctypes.pointer(_lib.Tuning(**tun))
        return d

    def call(self, d, *, t0=0, k_steps=8, null=(), odd=(), scratch_floats=1 << 40, **mlp_kw):
        """`null` / `odd`: names of BUFFERS to pass as NULL / 4 bytes off (ret_env and traj are NULL unless `odd`); `mlp_kw`: fields of the mlp
        struct, pointers as None, ODD or ODD1."""
        import ctypes
        buf = np.zeros(64, dtype=np.float32)
        p = buf.ctypes.data
        null, odd = ((v,) if isinstance(v, str) else tuple(v) for v in (null, odd))
        assert set(null + odd) <= set(self.BUFFERS)
        a = {k: (p + 4 if k in odd else None if k in null or k in ('ret_env', 'traj') else p) for k in self.BUFFERS}
        m = dict(n_hidden=16, n_sets=1, reserved=0, pre=p, dep=p, out=p, set_of_block=None, net_reset=None, act_low=p, act_high=p, sigma=None, seed=1)
        m.update({k: {self.ODD: p + 4, self.ODD1: p + 5}.get(v, v) if isinstance(v, str) else v for k, v in mlp_kw.items()})
        mlp = self.ext.mlp(**m)
        kpi = [a['kpi_bldg'], a['kpi_env']][:self.ext.n_kpi]
        extra = [a['series_scratch'], scratch_floats] if self.ext.extra else []
        return self.entry(ctypes.byref(d) if d is not None else None, a['params'], a['ts'], a['state'], ctypes.byref(mlp), a['out_bldg'], a['out_env'],
                          a['ret_env'], a['traj'], *kpi, *extra, t0, k_steps, None)


def exports(path):
    """The dynamic symbols a shared library defines (`nm -D --defined-only`), sorted."""
    import subprocess
    out = subprocess.run(['nm', '-D', '--defined-only', str(path)], capture_output=True, text=True, check=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if ' T ' in line)
