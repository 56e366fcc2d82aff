"""ctypes binding of ``libcitylearn_amd.so`` (the C-ABI in ``include/citylearn_amd.h``).

There is deliberately NO fallback: if the shared library is missing or a call fails the error propagates
(``EngineUnavailable`` / ``EngineError``).  Build with ``python -c 'import __graft_entry__ as g; g.build()'``
(or ``make -C citylearn_amd/csrc``).
"""
from __future__ import annotations

import ctypes
import os
import re
import subprocess
from pathlib import Path

from . import abi

PKG = Path(__file__).resolve().parent
LIB_PATH = PKG / 'libcitylearn_amd.so'
TUNE_LIB_PATH = PKG / 'libcitylearn_amd_tune.so'
CSRC = PKG / 'csrc'
# -amdgpu-mfma-vgpr-form: MFMA accumulators stay in VGPRs (gfx950's register file is unified), which removes the
# v_accvgpr_read copies in front of the LSTM activations (64 per window step)
HIPCC_FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-shared', '-fPIC', '-mllvm', '-amdgpu-mfma-vgpr-form']


class EngineUnavailable(RuntimeError):
    pass


class EngineError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f'citylearn_amd C-ABI error {code}: {message}')
        self.code = code


class Tuning(ctypes.Structure):
    """``cl_tuning`` (include/citylearn_amd.h): per-call launch-geometry overrides; all zero = library defaults."""
    _fields_ = [('vec', ctypes.c_int32), ('nw', ctypes.c_int32), ('no_chunks', ctypes.c_int32), ('lean_variant', ctypes.c_int32),
                ('envmajor', ctypes.c_int32), ('flex_vec', ctypes.c_int32), ('obs_variant', ctypes.c_int32),
                ('obs_rows', ctypes.c_int32), ('lstm_variant', ctypes.c_int32), ('full_variant', ctypes.c_int32),
                ('b_chunk', ctypes.c_int32), ('nt_stores', ctypes.c_int32), ('kernel_name', ctypes.c_void_p),
                ('finish', ctypes.c_int32), ('kpi_passes', ctypes.c_int32)]


class Dims(ctypes.Structure):
    """``cl_dims`` (include/citylearn_amd.h)."""
    _fields_ = [('n_env', ctypes.c_int32), ('n_bldg', ctypes.c_int32), ('n_steps', ctypes.c_int32),
                ('n_act_cols', ctypes.c_int32), ('flags', ctypes.c_uint32), ('n_ts_rows', ctypes.c_int32),
                ('env_row0', ctypes.c_void_p), ('tuning', ctypes.POINTER(Tuning)), ('env_offset', ctypes.c_int64),
                ('env_pitch', ctypes.c_int32), ('reserved0', ctypes.c_int32)]


class Flex(ctypes.Structure):
    """``cl_flex`` (include/citylearn_amd.h): EV chargers / washing machines tables and state."""
    _fields_ = [('n_ev', ctypes.c_int32), ('n_flex_bldg', ctypes.c_int32), ('n_rows', ctypes.c_int32), ('reserved', ctypes.c_int32),
                ('ev_params', ctypes.c_void_p), ('ev_ts', ctypes.c_void_p), ('charger_params', ctypes.c_void_p),
                ('charger_ts', ctypes.c_void_p), ('wm_params', ctypes.c_void_p), ('wm_ts', ctypes.c_void_p),
                ('cons_params', ctypes.c_void_p),
                ('ev_state', ctypes.c_void_p), ('wm_state', ctypes.c_void_p),
                ('flex_out', ctypes.c_void_p), ('charger_out', ctypes.c_void_p), ('drift', ctypes.c_void_p),
                ('seed', ctypes.c_uint64), ('weights', ctypes.c_float * 8)]


class PolicyMLP(ctypes.Structure):
    """``clpol_mlp`` (include/citylearn_amd_policy.h): the packed tables of a per-building MLP policy (`policy.MLPPolicy.pack`)."""
    _fields_ = [('n_hidden', ctypes.c_int32), ('n_sets', ctypes.c_int32), ('flags', ctypes.c_int32), ('reserved', ctypes.c_int32),
                ('pre', ctypes.c_void_p), ('dep', ctypes.c_void_p), ('out', ctypes.c_void_p), ('set_of_block', ctypes.c_void_p),
                ('net_reset', ctypes.c_void_p), ('act_low', ctypes.c_void_p), ('act_high', ctypes.c_void_p), ('sigma', ctypes.c_void_p),
                ('seed', ctypes.c_uint64)]


class PolicyFullMLP(ctypes.Structure):
    """``clpf_mlp`` (include/citylearn_amd_policy_full.h): the packed tables of a per-building storage MLP policy (`policy.StorageMLPPolicy.pack`)."""
    _fields_ = [('n_hidden', ctypes.c_int32), ('n_sets', ctypes.c_int32), ('n_device_cols', ctypes.c_int32), ('reserved', ctypes.c_int32),
                ('pre', ctypes.c_void_p), ('dep', ctypes.c_void_p), ('out', ctypes.c_void_p), ('set_of_block', ctypes.c_void_p),
                ('net_reset', ctypes.c_void_p), ('act_low', ctypes.c_void_p), ('act_high', ctypes.c_void_p), ('sigma', ctypes.c_void_p),
                ('seed', ctypes.c_uint64)]


class PolicyDeepMLP(ctypes.Structure):
    """``clpd_mlp`` (include/citylearn_amd_policy_deep.h): the packed tables of a per-building MLP policy with two hidden layers
    (`policy.DeepMLPPolicy.pack`) -- `PolicyMLP`'s fields, then the second layer's."""
    _fields_ = [*PolicyMLP._fields_, ('n_hidden2', ctypes.c_int32), ('reserved2', ctypes.c_int32), ('l2', ctypes.c_void_p)]


class PolicyFullDeepMLP(ctypes.Structure):
    """``clpfd_mlp`` (include/citylearn_amd_policy_full_deep.h): the packed tables of a per-building storage MLP policy with two hidden layers
    (`policy.DeepStorageMLPPolicy.pack`) -- `PolicyFullMLP`'s fields, then the second layer's (``flags``: 0 or ``CLPFD_MATRIX_CORES``;
    `PolicyFullMLP` has no flags word)."""
    _fields_ = [*PolicyFullMLP._fields_, ('n_hidden2', ctypes.c_int32), ('flags', ctypes.c_int32), ('l2', ctypes.c_void_p)]


def _compile(sources, out: Path, deps, force: bool, verbose: bool) -> Path:
    """`sources`: paths, or (path, extra flags) pairs -- translation units with flags of their own are compiled to objects first."""
    if not force and out.exists() and all(out.stat().st_mtime >= d.stat().st_mtime for d in deps):
        return out
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    units = [(s, []) if not isinstance(s, tuple) else s for s in sources]

    def run(cmd):
        if verbose:
            print(' '.join(cmd))
        subprocess.run(cmd, check=True)

    if all(not extra for _, extra in units):
        run([hipcc, *HIPCC_FLAGS, *(str(s) for s, _ in units), '-o', str(out)])
        return out
    import shutil
    tmp = out.parent / f'build_{out.stem}_{os.getpid()}'           # objects stay inside the tree (git-ignored) and are removed again
    tmp.mkdir(exist_ok=True)
    try:
        objs = []
        for src, extra in units:
            obj = tmp / (Path(src).stem + '.o')
            run([hipcc, *[f for f in HIPCC_FLAGS if f != '-shared'], *extra, '-c', str(src), '-o', str(obj)])
            objs.append(str(obj))
        run([hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', *objs, '-o', str(out)])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return out


# cl_noslp_tu.hip: the fused rollout kernel and the plain lean step kernel without SLP vectorisation (packed fp32 operations cost them
# 9 % / 4 %; csrc/cl_kernels.hip)
LIB_SOURCES = [CSRC / 'cl_kernels.hip', (CSRC / 'cl_noslp_tu.hip', ['-fno-slp-vectorize'])]


def build(force: bool = False, verbose: bool = False) -> Path:
    """Compile the HIP sources for gfx950 into the in-tree shared library (cross-compiles without a GPU)."""
    return _compile(LIB_SOURCES, LIB_PATH, sorted(CSRC.glob('*.hip')) + sorted(CSRC.glob('*.h')) + [abi.HEADER], force, verbose)


def build_variant(out: Path, extra_flags, verbose: bool = False) -> Path:
    """A second build of the library with extra compiler flags on every translation unit (diagnostic / A-B builds of scripts/)."""
    units = [(s, list(extra_flags)) if not isinstance(s, tuple) else (s[0], [*s[1], *extra_flags]) for s in LIB_SOURCES]
    return _compile(units, Path(out), [], True, verbose)


def build_tune(force: bool = False, verbose: bool = False) -> Path:
    """The microbenchmark / layout-probe kernels (csrc/cl_tune.hip) live in their own library, which the package never loads."""
    sources = [CSRC / 'cl_tune.hip']
    return _compile(sources, TUNE_LIB_PATH, sources, force, verbose)


def load_tune() -> ctypes.CDLL:
    """``libcitylearn_amd_tune.so`` for scripts/ and the MFMA layout test (not used by the package)."""
    import torch  # noqa: F401
    if not TUNE_LIB_PATH.exists():
        raise EngineUnavailable(f'{TUNE_LIB_PATH} not found (run __graft_entry__.build())')
    lib = ctypes.CDLL(str(TUNE_LIB_PATH))
    lib.cl_tune_copy_floor.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.cl_tune_mfma_bench.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.cl_tune_mfma_bf16_probe.argtypes = [ctypes.c_void_p] * 4
    return lib


class _Extension:
    """One closed-loop rollout library: a product library of its own per kernel family, so that the main library's symbol list, structs and
    translation units stay what they are (csrc/cl_<name>.hip, include/citylearn_amd_<name>.h, ``libcitylearn_amd_<name>.so``).  ``label`` names it
    in messages, ``flags`` are the translation unit's own compiler flags, ``entry`` is its rollout entry point taking ``mlp`` and ``n_kpi`` KPI
    planes, ``headers`` the other extension headers its header includes.  ``extra``: the ctypes of further entry arguments behind the KPI planes;
    ``functions``: ``(name, restype, argtypes)`` of further exported functions (``Dims`` pointer first) that `load` declares."""

    def __init__(self, name, prefix, label, flags, entry, mlp, n_kpi=0, headers=(), extra=(), functions=()):
        self.prefix, self.label, self.entry, self.mlp, self.n_kpi = prefix, label, entry, mlp, n_kpi
        self.extra, self.functions = tuple(extra), tuple(functions)
        self.path = PKG / f'libcitylearn_amd_{name}.so'
        self.header = abi.HEADER.parent / f'citylearn_amd_{name}.h'
        self.sources = [(CSRC / f'cl_{name}.hip', flags)] if flags else [CSRC / f'cl_{name}.hip']
        self.deps = [abi.HEADER, *headers, self.header]
        text = self.header.read_text()
        self.abi_version = int(re.search(rf'#define\s+{prefix.upper()}_ABI_VERSION\s+(\d+)', text).group(1))
        self.symbols = sorted(set(re.findall(rf'\b({prefix}_\w+)\s*\(', abi._strip_comments(text))))
        self._lib = None

    def build(self, force: bool = False, verbose: bool = False) -> Path:
        """Compile the extension's translation unit for gfx950 into its in-tree shared library."""
        return _compile(self.sources, self.path, sorted(CSRC.glob('*.hip')) + sorted(CSRC.glob('*.h')) + self.deps, force, verbose)

    def load(self) -> ctypes.CDLL:
        """The library (after torch, like `load`); refuses a build from another version of its own or the core header."""
        if self._lib is not None:
            return self._lib
        import torch  # noqa: F401
        if not self.path.exists():
            raise EngineUnavailable(f'{self.path} not found: the {self.label} extension is not built (run __graft_entry__.build())')
        lib = ctypes.CDLL(str(self.path))
        vp, i32 = ctypes.c_void_p, ctypes.c_int32
        abi_version, core_abi_version, last_error, entry = (getattr(lib, f'{self.prefix}_{n}') for n in ('abi_version', 'core_abi_version', 'last_error', self.entry))
        abi_version.restype = core_abi_version.restype = entry.restype = ctypes.c_int
        last_error.restype = ctypes.c_char_p
        entry.argtypes = [ctypes.POINTER(Dims), vp, vp, vp, ctypes.POINTER(self.mlp), vp, vp, vp, vp, *[vp] * self.n_kpi, *self.extra, i32, i32, vp]
        for fname, restype, argtypes in self.functions:
            fn = getattr(lib, f'{self.prefix}_{fname}')
            fn.restype, fn.argtypes = restype, list(argtypes)
        got, core = abi_version(), core_abi_version()
        if got != self.abi_version or core != abi.CL_ABI_VERSION:
            raise EngineUnavailable(f'ABI mismatch: {self.label} library {got} (core {core}), headers {self.abi_version} (core {abi.CL_ABI_VERSION}); '
                                    'rebuild the extension')
        self._lib = lib
        return lib

    def check(self, rc: int):
        if rc != 0:
            raise EngineError(rc, getattr(self.load(), f'{self.prefix}_last_error')().decode(errors='replace'))

    def rollout(self, *args):
        """Call the entry point and raise `EngineError` on a refusal."""
        self.check(getattr(self.load(), f'{self.prefix}_{self.entry}')(*args))


# The closed-loop rollout of battery + PV districts (no SLP vectorisation, like the other rollout kernels), the one that also keeps the streaming
# KPIs, and the one of THERMAL districts (compiled WITH SLP vectorisation like the main unit: the packed thermal unit of cl_full.h wants v_pk_*_f32)
POLICY = _Extension('policy', 'clpol', 'policy', ['-fno-slp-vectorize'], 'rollout_mlp_f32', PolicyMLP)
POLICY_KPI = _Extension('policy_kpi', 'clpk', 'policy KPI', ['-fno-slp-vectorize'], 'rollout_mlp_kpi_f32', PolicyMLP, n_kpi=2, headers=[POLICY.header])
POLICY_FULL = _Extension('policy_full', 'clpf', 'thermal policy', [], 'rollout_mlp_f32', PolicyFullMLP)
# ... and the thermal one that also keeps the streaming KPIs (cl_policy_full_kpi.hip, with SLP vectorisation like cl_policy_full.hip)
POLICY_FULL_KPI = _Extension('policy_full_kpi', 'clpfk', 'thermal policy KPI', [], 'rollout_mlp_kpi_f32', PolicyFullMLP, n_kpi=2, headers=[POLICY_FULL.header])
EXTENSIONS = (POLICY, POLICY_KPI, POLICY_FULL, POLICY_FULL_KPI)
# ... and the thermal one of districts of MORE than 16 buildings, a building-chunked launch (cl_policy_full_chunk.hip, with SLP vectorisation like
# cl_policy_full.hip; `clpf_mlp` again).  EXTENSIONS stays the four one-row ones, ALL_EXTENSIONS these five.
POLICY_FULL_CHUNK = _Extension('policy_full_chunk', 'clpfc', 'chunked thermal policy', [], 'rollout_mlp_f32', PolicyFullMLP, headers=[POLICY_FULL.header])
ALL_EXTENSIONS = EXTENSIONS + (POLICY_FULL_CHUNK,)
# ... and the chunked one that also keeps the streaming KPIs (cl_policy_full_chunk_kpi.hip, with SLP vectorisation; `clpf_mlp` again): behind the KPI
# planes its entry takes the scratch of the district series' chunk samples and its size, which `series_scratch_floats` tells.  A tuple of its own:
# EXTENSIONS and ALL_EXTENSIONS stay what they are; `__graft_entry__.build()` builds ALL_EXTENSIONS + CHUNK_KPI_EXTENSIONS.
POLICY_FULL_CHUNK_KPI = _Extension('policy_full_chunk_kpi', 'clpfck', 'chunked thermal policy KPI', [], 'rollout_mlp_kpi_f32', PolicyFullMLP, n_kpi=2,
                                   headers=[POLICY_FULL.header], extra=(ctypes.c_void_p, ctypes.c_int64),
                                   functions=(('series_scratch_floats', ctypes.c_int64, (ctypes.POINTER(Dims), ctypes.c_int32)),))
CHUNK_KPI_EXTENSIONS = (POLICY_FULL_CHUNK_KPI,)
# ... and the battery + PV one of districts of MORE than 32 buildings, a building-chunked launch with two buildings per wave (cl_policy_chunk.hip,
# without SLP vectorisation like cl_policy.hip; `clpol_mlp` again).  A tuple of its own once more: the tuples above stay what they are;
# `__graft_entry__.build()` builds ALL_EXTENSIONS + CHUNK_KPI_EXTENSIONS + LEAN_CHUNK_EXTENSIONS.
POLICY_CHUNK = _Extension('policy_chunk', 'clpc', 'chunked policy', ['-fno-slp-vectorize'], 'rollout_mlp_f32', PolicyMLP, headers=[POLICY.header])
LEAN_CHUNK_EXTENSIONS = (POLICY_CHUNK,)
# ... and the battery + PV one whose policy has TWO hidden layers (cl_policy_deep.hip, without SLP vectorisation like cl_policy.hip; `clpd_mlp`,
# which is `clpol_mlp` + the second layer).  A tuple of its own again: `__graft_entry__.build()` builds ALL_EXTENSIONS + CHUNK_KPI_EXTENSIONS +
# LEAN_CHUNK_EXTENSIONS + DEEP_EXTENSIONS.
POLICY_DEEP = _Extension('policy_deep', 'clpd', 'deep policy', ['-fno-slp-vectorize'], 'rollout_mlp_f32', PolicyDeepMLP, headers=[POLICY.header])
DEEP_EXTENSIONS = (POLICY_DEEP,)
# ... and the THERMAL one whose policy has two hidden layers (cl_policy_full_deep.hip; `clpfd_mlp`, which is `clpf_mlp` + the second layer).
# Without SLP vectorisation, unlike cl_policy_full.hip: with it the exact-fp32 policy block spills to scratch memory (the translation unit says
# how).  A tuple of its own: `__graft_entry__.build()` builds ALL_EXTENSIONS + CHUNK_KPI_EXTENSIONS + LEAN_CHUNK_EXTENSIONS + DEEP_EXTENSIONS +
# DEEP_THERMAL_EXTENSIONS.
POLICY_FULL_DEEP = _Extension('policy_full_deep', 'clpfd', 'deep thermal policy', ['-fno-slp-vectorize'], 'rollout_mlp_f32', PolicyFullDeepMLP,
                              headers=[POLICY_FULL.header])
DEEP_THERMAL_EXTENSIONS = (POLICY_FULL_DEEP,)
# ... and the battery + PV one under a CENTRAL-AGENT policy: one MLP over the district's observation vector (cl_policy_central.hip, without SLP
# vectorisation like cl_policy.hip; `clpca_mlp` has `clpol_mlp`'s fields, so `PolicyMLP` serves it -- only the shapes of pre / dep differ).  A tuple
# of its own: the tuples above stay what they are; `__graft_entry__.build()` builds it behind them.
POLICY_CENTRAL = _Extension('policy_central', 'clpca', 'central policy', ['-fno-slp-vectorize'], 'rollout_mlp_f32', PolicyMLP, headers=[POLICY.header])
CENTRAL_EXTENSIONS = (POLICY_CENTRAL,)
# ... and the central-agent one whose MLP has TWO hidden layers (cl_policy_central_deep.hip, without SLP vectorisation like cl_policy.hip;
# `clpcd_mlp` extends `clpca_mlp` as `clpd_mlp` extends `clpol_mlp`, so `PolicyDeepMLP` serves it).  A tuple of its own again:
# `__graft_entry__.build()` builds it behind CENTRAL_EXTENSIONS.
POLICY_CENTRAL_DEEP = _Extension('policy_central_deep', 'clpcd', 'deep central policy', ['-fno-slp-vectorize'], 'rollout_mlp_f32', PolicyDeepMLP,
                                 headers=[POLICY.header])
CENTRAL_DEEP_EXTENSIONS = (POLICY_CENTRAL_DEEP,)
# ... and the THERMAL one under a central-agent policy (cl_policy_full_central.hip; `clpfca_mlp` has `clpf_mlp`'s fields, so `PolicyFullMLP` serves
# it -- only the shapes of pre / dep differ).  With SLP vectorisation like cl_policy_full.hip (the translation unit says why).  A tuple of its
# own: the tuples above stay what they are; `__graft_entry__.build()` builds it behind CENTRAL_DEEP_EXTENSIONS.
POLICY_FULL_CENTRAL = _Extension('policy_full_central', 'clpfca', 'central thermal policy', [], 'rollout_mlp_f32', PolicyFullMLP,
                                 headers=[POLICY_FULL.header])
CENTRAL_THERMAL_EXTENSIONS = (POLICY_FULL_CENTRAL,)
# ... and the THERMAL central-agent one whose MLP has TWO hidden layers (cl_policy_full_central_deep.hip; `clpfcd_mlp` is `clpfca_mlp` + `clpfd_mlp`'s
# tail, so `PolicyFullDeepMLP` serves it): cl_policy_full_central.h's template at DEEP = true.  With SLP vectorisation like cl_policy_full_central.hip (the translation unit says why).  A tuple of its
# own: the tuples above stay what they are; `__graft_entry__.build()` builds it behind CENTRAL_THERMAL_EXTENSIONS.
POLICY_FULL_CENTRAL_DEEP = _Extension('policy_full_central_deep', 'clpfcd', 'deep central thermal policy', [], 'rollout_mlp_f32', PolicyFullDeepMLP,
                                      headers=[POLICY_FULL.header])
CENTRAL_DEEP_THERMAL_EXTENSIONS = (POLICY_FULL_CENTRAL_DEEP,)

# The names other code and the tests use: read-only views of the descriptions above (build / load / check read the description, so rebinding one
# of these changes nothing -- change the description's attribute instead)
POLICY_LIB_PATH, POLICY_HEADER, POLICY_SOURCES, POLICY_ABI_VERSION, POLICY_SYMBOLS = POLICY.path, POLICY.header, POLICY.sources, POLICY.abi_version, POLICY.symbols
build_policy, load_policy, check_policy = POLICY.build, POLICY.load, POLICY.check
POLICY_KPI_LIB_PATH, POLICY_KPI_HEADER, POLICY_KPI_SOURCES, POLICY_KPI_ABI_VERSION, POLICY_KPI_SYMBOLS = \
    POLICY_KPI.path, POLICY_KPI.header, POLICY_KPI.sources, POLICY_KPI.abi_version, POLICY_KPI.symbols
build_policy_kpi, load_policy_kpi, check_policy_kpi = POLICY_KPI.build, POLICY_KPI.load, POLICY_KPI.check
POLICY_FULL_LIB_PATH, POLICY_FULL_HEADER, POLICY_FULL_SOURCES, POLICY_FULL_ABI_VERSION, POLICY_FULL_SYMBOLS = \
    POLICY_FULL.path, POLICY_FULL.header, POLICY_FULL.sources, POLICY_FULL.abi_version, POLICY_FULL.symbols
build_policy_full, load_policy_full, check_policy_full = POLICY_FULL.build, POLICY_FULL.load, POLICY_FULL.check
POLICY_FULL_KPI_LIB_PATH, POLICY_FULL_KPI_HEADER, POLICY_FULL_KPI_SOURCES, POLICY_FULL_KPI_ABI_VERSION, POLICY_FULL_KPI_SYMBOLS = \
    POLICY_FULL_KPI.path, POLICY_FULL_KPI.header, POLICY_FULL_KPI.sources, POLICY_FULL_KPI.abi_version, POLICY_FULL_KPI.symbols
build_policy_full_kpi, load_policy_full_kpi, check_policy_full_kpi = POLICY_FULL_KPI.build, POLICY_FULL_KPI.load, POLICY_FULL_KPI.check
POLICY_FULL_CHUNK_LIB_PATH, POLICY_FULL_CHUNK_HEADER, POLICY_FULL_CHUNK_SOURCES, POLICY_FULL_CHUNK_ABI_VERSION, POLICY_FULL_CHUNK_SYMBOLS = \
    POLICY_FULL_CHUNK.path, POLICY_FULL_CHUNK.header, POLICY_FULL_CHUNK.sources, POLICY_FULL_CHUNK.abi_version, POLICY_FULL_CHUNK.symbols
build_policy_full_chunk, load_policy_full_chunk, check_policy_full_chunk = POLICY_FULL_CHUNK.build, POLICY_FULL_CHUNK.load, POLICY_FULL_CHUNK.check
POLICY_FULL_CHUNK_KPI_LIB_PATH, POLICY_FULL_CHUNK_KPI_HEADER, POLICY_FULL_CHUNK_KPI_SOURCES, POLICY_FULL_CHUNK_KPI_ABI_VERSION, POLICY_FULL_CHUNK_KPI_SYMBOLS = \
    POLICY_FULL_CHUNK_KPI.path, POLICY_FULL_CHUNK_KPI.header, POLICY_FULL_CHUNK_KPI.sources, POLICY_FULL_CHUNK_KPI.abi_version, POLICY_FULL_CHUNK_KPI.symbols
build_policy_full_chunk_kpi, load_policy_full_chunk_kpi, check_policy_full_chunk_kpi = \
    POLICY_FULL_CHUNK_KPI.build, POLICY_FULL_CHUNK_KPI.load, POLICY_FULL_CHUNK_KPI.check
POLICY_CHUNK_LIB_PATH, POLICY_CHUNK_HEADER, POLICY_CHUNK_SOURCES, POLICY_CHUNK_ABI_VERSION, POLICY_CHUNK_SYMBOLS = \
    POLICY_CHUNK.path, POLICY_CHUNK.header, POLICY_CHUNK.sources, POLICY_CHUNK.abi_version, POLICY_CHUNK.symbols
build_policy_chunk, load_policy_chunk, check_policy_chunk = POLICY_CHUNK.build, POLICY_CHUNK.load, POLICY_CHUNK.check


def policy_kpi_lds_bytes(nw: int, vec: int) -> int:
    """Dynamic LDS of one `cl_rollout_policy_kpi_kernel` workgroup of ``nw`` waves at ``vec`` envs per lane: csrc/cl_policy.h's
    `rollout_policy_kpi_lds_floats` -- the KPI kernel's ring [8][nw][tile], series [12][tile] + [16], baseline rows [8][4][32] + [5][32], then the
    policy's staged rows [nw][2][3 x 32 + 8] (tests/test_policy_kpi_host.py holds it against the header's formula)."""
    tile = 64 * vec
    return 4 * (8 * nw * tile + 12 * tile + 16 + 8 * 4 * 32 + 5 * 32 + nw * 2 * (3 * 32 + 8))


def policy_deep_lds_bytes(nw: int, h1: int, h2: int) -> int:
    """Dynamic LDS of one `cl_rollout_policy_deep_kernel` workgroup of ``nw`` waves (two buildings each, one env per lane) at ``h1`` x ``h2``
    hidden units: csrc/cl_policy_deep.h's `rollout_policy_deep_lds_floats` -- the reduction rows [nw][4][64], then per building the staged row
    [h1 / 4][2][4] + [h1 + 1][h2] + [h2] + 8 -- 164 864 bytes at sixteen waves and 32 x 32, which the library refuses (a CU has 163 840)."""
    return 4 * (nw * 4 * 64 + nw * 2 * (2 * h1 + (h1 + 1) * h2 + h2 + 8))


LDS_PER_CU = 160 * 1024        # csrc/cl_rollout.h's CL_LDS_PER_CU: what the policy entries hold a workgroup's dynamic LDS against


def policy_deep_mma_lds_bytes(nw: int) -> int:
    """... and of its matrix-core family (`clpd_mlp.flags & CLPD_MATRIX_CORES`): the reduction rows, then per building the staged row
    [32] x 4 + 8 + the A fragments [2][2][64][4] = 1160 floats at every h1, h2 -- 154 560 bytes at fifteen waves (30 buildings), 164 864 at sixteen."""
    return 4 * (nw * 4 * 64 + nw * 2 * 1160)


def policy_full_deep_lds_bytes(nw: int, h1: int, h2: int, matrix_cores: bool = False) -> int:
    """Dynamic LDS of one `cl_rollout_full_policy_deep_kernel` workgroup of ``nw`` waves (= buildings, one env per lane) at ``h1`` x ``h2`` hidden
    units: csrc/cl_policy_full_deep.h's `rollout_full_policy_deep_lds_floats` -- the reduction rows [nw][4][64], then per building the staged row
    [h1 / 4][5][4] + [h1 + 1][h2] + [4][h2] + 4 x 8, or in the matrix-core family [5][32] + [32] + [4][32] + 4 x 8 + the A fragments
    [2][2][64][4] = 1376 floats at every h1, h2 (the exact family's row at 32 x 32) -- 104 448 bytes at sixteen waves and 32 x 32."""
    row = 1376 if matrix_cores else 5 * h1 + (h1 + 1) * h2 + 4 * h2 + 32
    return 4 * (nw * 4 * 64 + nw * row)


def policy_central_lds_bytes(nw: int, n_bldg: int, h: int) -> int:
    """Dynamic LDS of one `cl_rollout_policy_central_kernel` workgroup of ``nw`` waves (two buildings each, one env per lane) over ``n_bldg``
    buildings at ``h`` hidden units: include/citylearn_amd_policy_central.h's formula (csrc/cl_policy_central.h's
    `rollout_policy_central_lds_floats`) -- the reduction rows [nw][4][64], the published soc / net planes X [2][n_bldg][64], the hidden layer
    Hh [h][64], the staged ``dep`` [h / 4][n_bldg][8], the staged out rows [nw][2][64 + 8] -- 74 752 bytes at sixteen waves, 32 buildings and 64
    units (tests/test_policy_central_host.py holds it against the header's formula)."""
    return 4 * (nw * 4 * 64 + 2 * n_bldg * 64 + h * 64 + 2 * h * n_bldg + nw * 2 * (64 + 8))


def policy_central_deep_lds_bytes(nw: int, n_bldg: int, h1: int, h2: int) -> int:
    """Dynamic LDS of one `cl_rollout_policy_central_deep_kernel` workgroup of ``nw`` waves over ``n_bldg`` buildings at ``h1`` x ``h2`` hidden
    units: include/citylearn_amd_policy_central_deep.h's formula (csrc/cl_policy_central.h's `rollout_policy_central_deep_lds_floats`) --
    `policy_central_lds_bytes`' regions at ``h1`` units, plus the second hidden layer Hh2 [h2][64] and the staged ``l2`` [h1 + 1][h2] -- 107 776
    bytes at sixteen waves, 32 buildings and 64 x 64 units (tests/test_policy_central_deep_host.py holds it against the header's formula)."""
    return 4 * (nw * 4 * 64 + 2 * n_bldg * 64 + h1 * 64 + h2 * 64 + 2 * h1 * n_bldg + (h1 + 1) * h2 + nw * 2 * (64 + 8))


def policy_full_central_lds_bytes(n_bldg: int, h: int) -> int:
    """Dynamic LDS of one `cl_rollout_full_policy_central_kernel` workgroup over ``n_bldg`` buildings (one wave each, one env per lane) at ``h``
    hidden units: include/citylearn_amd_policy_full_central.h's formula (csrc/cl_policy_full_central.h's `rollout_full_policy_central_lds_floats`)
    -- the reduction rows [n_bldg][4][64], the published planes X [5][n_bldg][64], the hidden layer Hh [h][64], the staged ``dep``
    [h / 4][n_bldg][5][4], the staged head rows [n_bldg][4 x 64 + 4 x 8] -- 92 160 bytes at sixteen buildings and 64 units
    (tests/test_policy_full_central_host.py holds it against the header's formula)."""
    return 4 * (n_bldg * 4 * 64 + 5 * n_bldg * 64 + h * 64 + 5 * h * n_bldg + n_bldg * (4 * 64 + 4 * 8))


def policy_full_central_deep_lds_bytes(n_bldg: int, h1: int, h2: int) -> int:
    """Dynamic LDS of one `cl_rollout_full_policy_central_deep_kernel` workgroup over ``n_bldg`` buildings (one wave each, one env per lane) at
    ``h1`` x ``h2`` hidden units: include/citylearn_amd_policy_full_central_deep.h's formula (csrc/cl_policy_full_central.h's
    `rollout_full_policy_central_deep_lds_floats`) -- `policy_full_central_lds_bytes`' regions at ``h1`` units, plus the second hidden layer Hh2
    [h2][64] and the staged ``l2`` [h1 + 1][h2] -- 125 184 bytes at sixteen buildings and 64 x 64 units
    (tests/test_policy_full_central_deep_host.py holds it against the header's formula)."""
    return 4 * (n_bldg * 4 * 64 + 5 * n_bldg * 64 + h1 * 64 + h2 * 64 + 5 * h1 * n_bldg + (h1 + 1) * h2 + n_bldg * (4 * 64 + 4 * 8))


def policy_chunk_lds_bytes(nw: int, vec: int) -> int:
    """Dynamic LDS of one `cl_rollout_policy_chunk_kernel` workgroup of ``nw`` waves (two buildings each) at ``vec`` envs per lane:
    csrc/cl_policy_chunk.h's `rollout_policy_chunk_lds_floats`, which is the one-row launch's formula (csrc/cl_policy.h) -- the chunk's reduction rows
    [nw][4][tile], then the staged policy rows [nw][2][3 x 32 + 8] -- 29 696 bytes at sixteen waves and one env per lane, 46 080 at two
    (tests/test_policy_chunk_host.py holds it against the header's formula)."""
    return 4 * (nw * 4 * 64 * vec + nw * 2 * (3 * 32 + 8))


def policy_full_lds_bytes(nw: int, vec: int) -> int:
    """Dynamic LDS of one `cl_rollout_full_policy_kernel` workgroup of ``nw`` waves at ``vec`` envs per lane: csrc/cl_policy_full.h's
    `rollout_full_policy_lds_floats` -- the district reduction's rows [nw][4][tile], then the staged policy rows [nw][(5 + 4) x 32 + 4 x 8]."""
    return 4 * (nw * 4 * 64 * vec + nw * ((5 + 4) * 32 + 4 * 8))


def policy_full_chunk_lds_bytes(nw: int, vec: int) -> int:
    """Dynamic LDS of one `cl_rollout_full_policy_chunk_kernel` workgroup of ``nw`` waves (= buildings of a chunk) at ``vec`` envs per lane:
    csrc/cl_policy_full.h's `rollout_full_policy_chunk_lds_floats`, which is `policy_full_lds_bytes`'s formula (the chunk's reduction rows
    [nw][4][tile], then the staged policy rows) -- 26 624 bytes at the default eight waves and two envs per lane."""
    return 4 * (nw * 4 * 64 * vec + nw * ((5 + 4) * 32 + 4 * 8))


def policy_full_kpi_lds_bytes(nw: int) -> int:
    """Dynamic LDS of one `cl_rollout_full_policy_kpi_kernel` workgroup of ``nw`` waves (one env per lane): csrc/cl_policy_full.h's
    `rollout_full_policy_kpi_lds_floats` -- the ring of both district series [8][2][nw][64], the two series [2][12][64], the staged policy rows
    [nw][(5 + 4) x 32 + 4 x 8], the units' twelve sums [nw][12][64] (tests/test_policy_full_kpi_host.py holds it against the header's formula)."""
    return 4 * (8 * 2 * nw * 64 + 2 * 12 * 64 + nw * ((5 + 4) * 32 + 4 * 8) + nw * 12 * 64)


def policy_full_chunk_kpi_lds_bytes(nw: int) -> int:
    """Dynamic LDS of one `cl_rollout_full_policy_chunk_kpi_kernel` workgroup of ``nw`` waves (= buildings of a chunk; one env per lane):
    csrc/cl_policy_full.h's `rollout_full_policy_chunk_kpi_lds_floats` -- the ring of both district series [8][2][nw][64], then the staged
    policy rows [nw][(5 + 4) x 32 + 4 x 8] (the units' twelve sums live in registers) -- 43 008 bytes at the default eight waves, 86 016 at sixteen
    (tests/test_policy_full_chunk_kpi_host.py holds it against the header's formula)."""
    return 4 * (8 * 2 * nw * 64 + nw * ((5 + 4) * 32 + 4 * 8))


_lib = None


def load() -> ctypes.CDLL:
    """Load the library (after torch, so that both share one libamdhip64 / one HIP context)."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  -- must come first: the HIP runtime torch ships is the one the kernels run on
    # CITYLEARN_AMD_LIB: an alternative build of the same library (A/B builds of scripts/: `build_variant`), never a different backend
    path = Path(os.environ['CITYLEARN_AMD_LIB']).resolve() if os.environ.get('CITYLEARN_AMD_LIB') else LIB_PATH
    if not path.exists():
        raise EngineUnavailable(f'{path} not found: the HIP extension is not built (run __graft_entry__.build())')
    lib = ctypes.CDLL(str(path))
    vp, i32, i64, u64, f32p = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_void_p
    lib.cl_abi_version.restype = ctypes.c_int
    lib.cl_last_error.restype = ctypes.c_char_p
    lib.cl_reset_f32.restype = ctypes.c_int
    lib.cl_reset_f32.argtypes = [ctypes.POINTER(Dims), vp, f32p, f32p, f32p, vp]
    lib.cl_step_f32.restype = ctypes.c_int
    lib.cl_step_f32.argtypes = [ctypes.POINTER(Dims), vp, f32p, f32p, f32p, i64, i64, f32p, f32p, f32p, f32p, i32, vp]
    lib.cl_flex_reset_f32.restype = ctypes.c_int
    lib.cl_flex_reset_f32.argtypes = [ctypes.POINTER(Dims), ctypes.POINTER(Flex), vp]
    lib.cl_step_flex_f32.restype = ctypes.c_int
    lib.cl_step_flex_f32.argtypes = [ctypes.POINTER(Dims), vp, f32p, f32p, f32p, i64, i64, f32p, f32p, f32p, f32p,
                                     ctypes.POINTER(Flex), i32, vp]
    lib.cl_step_observe_f32.restype = ctypes.c_int
    lib.cl_step_observe_f32.argtypes = [ctypes.POINTER(Dims), vp, f32p, f32p, f32p, i64, i64, f32p, f32p, f32p, f32p, i32,
                                        f32p, vp, f32p, vp, i32, f32p, i32, i32, i32, i32, vp]
    lib.cl_lstm_generic_step_f32.restype = ctypes.c_int
    lib.cl_rollout_f32.restype = ctypes.c_int
    lib.cl_rollout_f32.argtypes = [ctypes.POINTER(Dims), vp, f32p, f32p, f32p, i64, i64, i64, f32p, f32p, u64,
                                   f32p, f32p, f32p, i32, i32, vp]
    lib.cl_rollout_seq_f32.restype = ctypes.c_int
    lib.cl_rollout_seq_f32.argtypes = [ctypes.POINTER(Dims), vp, f32p, f32p, f32p, i64, i64, i64, f32p, f32p, u64, f32p,
                                       f32p, f32p, f32p, f32p, f32p, ctypes.POINTER(Flex), i32, i32, vp]
    lib.cl_finish_f32.restype = ctypes.c_int
    lib.cl_finish_f32.argtypes = [ctypes.POINTER(Dims), f32p, f32p, i32, vp]
    lib.cl_philox_uniform.restype = ctypes.c_float
    lib.cl_philox_uniform.argtypes = [u64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    got = lib.cl_abi_version()
    if got != abi.CL_ABI_VERSION:
        raise EngineUnavailable(f'ABI mismatch: library {got}, header {abi.CL_ABI_VERSION}; rebuild the extension')
    _lib = lib
    return lib


def check(rc: int):
    if rc != 0:
        raise EngineError(rc, load().cl_last_error().decode(errors='replace'))
