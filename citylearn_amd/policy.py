"""A closed-loop policy INSIDE the fused K-step rollout: a tanh MLP with one hidden layer (or two: `DeepMLPPolicy`, below) per building
over that building's own observation vector, evaluated by `cl_rollout_policy_kernel` (csrc/cl_policy.h, ``libcitylearn_amd_policy.so``,
include/citylearn_amd_policy.h).

Inference of a GIVEN policy only -- no training, no agent: the weights come from the caller (a learner in torch, an evolution strategy that
scores a population of controllers by return: one parameter set per block of ``abi.CL_ROW0_BLOCK`` envs).

    policy = MLPPolicy(w1, b1, w2, b2, sigma=0.1)                  # w1 [n_sets, n_bldg, H, n_obs] over ObservationLayout.building_names[i]
    env = VectorCityLearnEnv(schema, n_envs, observations='tensor', normalize_observations=True)
    ret, traj = env.rollout_policy(policy, 24, seed=3, record=True)    # ONE launch; traj [24, CLPOL_NT, n_bldg, n_envs]

To score the controllers with CityLearn's KPIs, build the env with ``kpi=True`` and ask for them in the same call: ONE launch of
`cl_rollout_policy_kpi_kernel` (csrc/cl_policy.h at KPI = true, ``libcitylearn_amd_policy_kpi.so``, include/citylearn_amd_policy_kpi.h) keeps the streaming
accumulators next to the policy, and `evaluate()` works afterwards as after any other rollout -- no second env, no trajectory through memory:

    kenv = VectorCityLearnEnv(schema, n_envs, observations='tensor', normalize_observations=True, kpi=True)
    ret = kenv.rollout_policy(policy, 24, seed=3, kpi=True)
    building_kpis, district_kpis = kenv.evaluate()

``kpi=False`` (the default) is the launch without KPIs, which refuses a ``kpi=True`` env.  For envs built WITHOUT KPIs the route is the
replay: record the rollout, then feed its action plane open-loop to a second, ``kpi=True`` env (battery + PV districts whose storage action
column of building b is column b, as in the 2022 schemas):

    kenv = VectorCityLearnEnv(schema, n_envs, kpi=True)
    kenv.rollout(24, actions=traj[:, policy.CLPOL_T_ACTION].contiguous(), fused=True)      # policy = this module
    building_kpis, district_kpis = kenv.evaluate()

THERMAL districts -- cooling / heating / DHW storage beside the battery, the 2020 / 2021 schemas: no LSTM stage, no device actions, up to 16
buildings -- take a `StorageMLPPolicy`: the same hidden layer with up to FOUR heads per building in the fixed order electrical, cooling, heating,
DHW storage (a head whose action column the building lacks is ignored), fed by the building's four storage socs and its previous net.  One launch
of `cl_rollout_full_policy_kernel` (csrc/cl_policy_full.h, ``libcitylearn_amd_policy_full.so``, include/citylearn_amd_policy_full.h):

    spolicy = StorageMLPPolicy(w1, b1, w2, b2, sigma=0.1)          # w2 [n_sets, n_bldg, 4, H], b2 [n_sets, n_bldg, 4]
    ret, traj = env.rollout_policy(spolicy, 24, seed=3, record=True)   # traj [24, CLPF_NT, n_bldg, n_envs]: policy.CLPF_T_ACTION + head, ..

On an env built with ``kpi=True`` the same call with ``kpi=True`` is ONE launch of `cl_rollout_full_policy_kpi_kernel`
(csrc/cl_policy_full.h at KPI = true, ``libcitylearn_amd_policy_full_kpi.so``, include/citylearn_amd_policy_full_kpi.h) that also keeps every env's
streaming KPI accumulators, so `evaluate()` scores the controllers afterwards -- no record, no second env:

    kenv = VectorCityLearnEnv(schema, n_envs, kpi=True)
    ret = kenv.rollout_policy(spolicy, 24, seed=3, kpi=True)
    building_kpis, district_kpis = kenv.evaluate()

(``kpi=True`` on an env built without KPIs raises `NotImplementedError`.)  `MLPPolicy` still refuses such a district.  A district with power
outages goes through the same two kernels (their outage branch is tested on g2020_cz1 with chosen outage rows: tests/policy_full_util.py
`outage_district`).

A thermal district of MORE than 16 buildings -- BASELINE config 4's 1024 -- takes the same `StorageMLPPolicy` through a building-chunked launch:
`cl_rollout_full_policy_chunk_kernel` (csrc/cl_policy_full.h at CHUNK = true, ``libcitylearn_amd_policy_full_chunk.so``,
include/citylearn_amd_policy_full_chunk.h) with one building per wave and balanced chunks of at most eight buildings along the grid's second
axis, then one `cl_finish_kernel` launch that adds the chunks' district sums and returns.  `VectorCityLearnEnv.rollout_policy` routes there by
itself; on the engine it is ``rollout_policy(..., chunked=True)``, the chunk size from ``tuning=dict(b_chunk=...)``.  Same policy, same noise
stream (keyed by global env, column and step: chunking does not change a draw), same record.  The packed tables are the same
`StoragePolicyTables`; at 1024 buildings ``pre`` is ``[n_sets, rows, 1024, H]`` float32 -- 48 MB per parameter set at H = 16 over the 744-row
fixture.

On an env built with ``kpi=True`` the chunked call takes ``kpi=True`` as well: `cl_rollout_full_policy_chunk_kpi_kernel`
(csrc/cl_policy_full.h at KPI = CHUNK = true and csrc/cl_policy_full_chunk_kpi.h, ``libcitylearn_amd_policy_full_chunk_kpi.so``, include/citylearn_amd_policy_full_chunk_kpi.h) keeps every unit's
twelve sums inside the launch and hands the chunks' partial samples of the two district series to `cl_kpi_series_chunk_kernel`; `cl_finish_kernel`
follows as before.  `evaluate()` then scores the 1024-building district's controllers without a record, a second env or a replay:

    kenv = VectorCityLearnEnv(schema_1024, n_envs, kpi=True)
    ret = kenv.rollout_policy(spolicy, 720, seed=3, kpi=True)      # windows of StepEngine.policy_kpi_window = 64 steps, one call each
    building_kpis, district_kpis = kenv.evaluate()

A battery + PV district of MORE than 32 buildings -- the 1024-building tiling of the 2022 schema -- takes the `MLPPolicy` through a
building-chunked launch as well: `cl_rollout_policy_chunk_kernel` (csrc/cl_policy.h at CHUNK = true, csrc/cl_policy_chunk.h, ``libcitylearn_amd_policy_chunk.so``,
include/citylearn_amd_policy_chunk.h) with two buildings per wave and the blind chunked rollout's 32-building workgroups, balanced (33 -> 17 + 16,
1024 -> 32 x 32), then one `cl_finish_kernel` launch.  `VectorCityLearnEnv.rollout_policy` routes there by itself (`_Kind.one_row_max`); on the
engine it is ``rollout_policy(..., chunked=True)`` with `PolicyTables`, chunk size and waves from ``tuning=dict(b_chunk=..., nw=...)``.  Same
policy, same noise stream, same record ``[k_steps, CLPOL_NT, n_bldg, n_envs]``.  This launch keeps NO streaming KPIs (``chunked=True, kpi=True``
with `PolicyTables` raises `NotImplementedError`): score such a district by the replay above -- record, then `StepEngine.step_many` of the action
plane on a second, ``kpi=True`` engine.

An actor with TWO hidden layers (the SAC / PPO actors of the CityLearn examples) is a `DeepMLPPolicy`: ``h1 = tanh(W1 obs + b1)``,
``h2 = tanh(W2 h1 + b2)``, ``a = clamp(mid + half tanh(w3 . h2 + b3) + sigma z, low, high)`` with H1, H2 in 4, 8, .. 32, on battery + PV districts
of up to 32 buildings: one launch of `cl_rollout_policy_deep_kernel` (csrc/cl_policy_deep.h, ``libcitylearn_amd_policy_deep.so``,
include/citylearn_amd_policy_deep.h) through the same `rollout_policy` call, with `MLPPolicy`'s record ``[k_steps, CLPOL_NT, n_bldg, n_envs]`` and
noise stream:

    deep = DeepMLPPolicy(w1, b1, w2, b2, w3, b3, sigma=0.1)        # w2 [n_sets, n_bldg, H2, H1], w3 [n_sets, n_bldg, H2]
    ret, traj = env.rollout_policy(deep, 24, seed=3, record=True)

Layer 2 runs in exact fp32 or, ``pack(matrix_cores=True)``, on the f16 matrix cores with split operands; ``matrix_cores=None`` (what the env
uses) is `default_matrix_cores`: the family profiles/policy_deep_probe.log shows faster.  No streaming KPIs (``kpi=True`` raises
`NotImplementedError`: record, then replay the action plane on a ``kpi=True`` env as above), no chunked launch (more than 32 buildings is the
library's refusal), no MARL.

On a THERMAL district of up to 16 buildings the actor with two hidden layers is a `DeepStorageMLPPolicy`: the same two layers with
`StorageMLPPolicy`'s four heads, five env-dependent inputs, record ``[k_steps, CLPF_NT, n_bldg, n_envs]`` and noise stream -- one launch of
`cl_rollout_full_policy_deep_kernel` (csrc/cl_policy_full_deep.h, ``libcitylearn_amd_policy_full_deep.so``,
include/citylearn_amd_policy_full_deep.h), one env per lane, one building per wave, every reward kind of the thermal kernel (MARL included):

    sdeep = DeepStorageMLPPolicy(w1, b1, w2, b2, w3, b3, sigma=0.1)    # w2 [n_sets, n_bldg, H2, H1], w3 [n_sets, n_bldg, 4, H2], b3 [n_sets, n_bldg, 4]
    ret, traj = env.rollout_policy(sdeep, 24, seed=3, record=True)

Layer 2 again in exact fp32 or on the f16 matrix cores; ``matrix_cores=None`` is `default_thermal_matrix_cores`, a rule measured on THIS kernel
(profiles/policy_full_deep_probe.log).  No streaming KPIs (``kpi=True`` raises `NotImplementedError`: record, then replay the heads' action
planes on a ``kpi=True`` env), no chunked launch (more than 16 buildings is the library's refusal).

CityLearn's other mode, ``central_agent=True`` -- ONE actor that sees the district's observation vector and returns every building's action, what
the Stable-Baselines3 route needs -- is a `CentralMLPPolicy`: ``h = tanh(W1 obs + b1)`` over ``ObservationLayout(..., central_agent=True).columns``
with H in 4, 8, .. 64, then one head per building that has a storage action, ``a_b = clamp(mid_b + half_b tanh(w2[b] . h + b2[b]) + sigma_b z,
low_b, high_b)``.  Battery + PV districts of up to 32 buildings, every lean reward kind (MARL included): one launch of
`cl_rollout_policy_central_kernel` (csrc/cl_policy_central.h, ``libcitylearn_amd_policy_central.so``, include/citylearn_amd_policy_central.h) through
the same `rollout_policy` call of an env built with ``central_agent=True``, with `MLPPolicy`'s record ``[k_steps, CLPOL_NT, n_bldg, n_envs]``, bounds,
sigma and noise stream:

    cenv = VectorCityLearnEnv(schema, n_envs, observations='tensor', normalize_observations=True, central_agent=True)
    central = CentralMLPPolicy(w1, b1, w2, b2, sigma=0.1)          # w1 [n_sets, H, n_cols], b1 [n_sets, H], w2 [n_sets, n_bldg, H], b2 [n_sets, n_bldg]
    ret, traj = cenv.rollout_policy(central, 24, seed=3, record=True)

The hidden layer sums over ALL buildings' soc and previous net, so the kernel exchanges them through LDS with two workgroup barriers per step; the
sums have a fixed order and ``tuning=dict(nw=...)`` changes no action.  An env built with ``central_agent=False`` raises `ValueError` (its
observation tensor is not the vector the weights are defined over); ``kpi=True`` raises `NotImplementedError` (record, then replay the action
plane on a ``kpi=True`` env); more than 32 buildings and a thermal district are the library's refusals.

A central actor with TWO hidden layers -- a SAC / PPO actor trained with ``central_agent=True`` -- is a `DeepCentralMLPPolicy`: ``h1 = tanh(W1 obs
+ b1)``, ``h2 = tanh(W2 h1 + b2)``, ``a_b = clamp(mid_b + half_b tanh(w3[b] . h2 + b3[b]) + sigma_b z, low_b, high_b)`` with H1, H2 in 4, 8, .. 64
independently, same districts, reward kinds, record and noise stream as the `CentralMLPPolicy`: one launch of
`cl_rollout_policy_central_deep_kernel` (csrc/cl_policy_central.h at DEEP = true, ``libcitylearn_amd_policy_central_deep.so``,
include/citylearn_amd_policy_central_deep.h), whose step has a third phase and barrier for layer 2 -- one H1 x H2 product per ENV, in exact fp32:

    dcentral = DeepCentralMLPPolicy(w1, b1, w2, b2, w3, b3, sigma=0.1)    # w2 [n_sets, H2, H1], b2 [n_sets, H2], w3 [n_sets, n_bldg, H2], b3 [n_sets, n_bldg]
    ret, traj = cenv.rollout_policy(dcentral, 24, seed=3, record=True)

Its refusals are the central policy's.

On a THERMAL district of up to 16 buildings (the 2020 / 2021 schemas) the central actor is a `CentralStorageMLPPolicy`: the same hidden layer over
the central-agent vector, H in 4, 8, .. 64, with `StorageMLPPolicy`'s four heads per building, bounds, sigma, noise stream and record
``[k_steps, CLPF_NT, n_bldg, n_envs]``; the env-dependent inputs are EVERY building's four storage socs and previous net.  One launch of
`cl_rollout_full_policy_central_kernel` (csrc/cl_policy_full_central.h, ``libcitylearn_amd_policy_full_central.so``,
include/citylearn_amd_policy_full_central.h), one building per wave and one env per lane, every reward kind of the thermal kernel (MARL included):

    tenv = VectorCityLearnEnv(schema_2020, n_envs, observations='tensor', normalize_observations=True, central_agent=True)
    scentral = CentralStorageMLPPolicy(w1, b1, w2, b2, sigma=0.1)     # w1 [n_sets, H, n_cols], b1 [n_sets, H], w2 [n_sets, n_bldg, 4, H], b2 [n_sets, n_bldg, 4]
    ret, traj = tenv.rollout_policy(scentral, 24, seed=3, record=True)

An env built with ``central_agent=False`` raises `ValueError`; ``kpi=True`` raises `NotImplementedError` (record, then replay the heads' action
planes ``CLPF_T_ACTION + head`` into the columns of `head_columns` on a ``kpi=True`` env); more than 16 buildings and a battery + PV district are
the library's refusals.  No local fixture has a heating tank: the heating-storage term and head are exercised by the packer test only.

Open: device-action heads, streaming KPIs in the chunked battery + PV launch, MARL in chunked launches (the libraries' refusal); for the deep
policy a KPI twin, a chunked twin, MARL, hidden layers wider than 32 or deeper than two; for the deep thermal policy a KPI twin, more than 16
buildings, device-action heads, two envs per lane, hidden layers wider than 32 or deeper than two; for both battery + PV central policies a KPI
twin, more than 32 buildings; for the deep central policy a matrix-core family of layer 2, thermal districts, hidden layers deeper than two; for
the central thermal policy a KPI twin, more than 16 buildings, two hidden layers, device-action heads.
"""
from __future__ import annotations

import math
import re
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _lib, abi
from .observations import SRC_OUT, SRC_STATE, SRC_TEMP, ObservationLayout

# tanh x = (1 - e) / (1 + e), e = 2^(ACT_SCALE x): what the kernel evaluates with one v_exp_f32 + one v_rcp_f32 per hidden unit; folded into
# the packed first layer (`pre`, `dep`)
ACT_SCALE = -2.0 * math.log2(math.e)


def _header_constants(header, prefix: str) -> dict:
    """The integer ``#define``s of an extension header that start with `prefix`."""
    text = re.sub(r'/\*.*?\*/', ' ', header.read_text(), flags=re.S)
    return {m.group(1): int(m.group(2).rstrip('ulUL'), 0) for m in re.finditer(rf'#define\s+({prefix}\w+)\s+(0x[0-9a-fA-F]+\w*|\d+)\b', text)}


CONSTANTS = _header_constants(_lib.POLICY_HEADER, 'CLPOL_')
CLPOL_NT, CLPOL_T_ACTION, CLPOL_T_REWARD, CLPOL_T_NET, CLPOL_T_SOC = (CONSTANTS[k] for k in ('CLPOL_NT', 'CLPOL_T_ACTION', 'CLPOL_T_REWARD',
                                                                                             'CLPOL_T_NET', 'CLPOL_T_SOC'))
CLPOL_NOISE_KEY, CLPOL_MAX_HIDDEN = CONSTANTS['CLPOL_NOISE_KEY'], CONSTANTS['CLPOL_MAX_HIDDEN']
# thermal districts: up to four storage heads per building (csrc/cl_policy_full.h, libcitylearn_amd_policy_full.so)
FULL_CONSTANTS = _header_constants(_lib.POLICY_FULL_HEADER, 'CLPF_')
CLPF_NT, CLPF_ND, CLPF_NA, CLPF_MAX_HIDDEN = (FULL_CONSTANTS[k] for k in ('CLPF_NT', 'CLPF_ND', 'CLPF_NA', 'CLPF_MAX_HIDDEN'))
CLPF_T_ACTION, CLPF_T_REWARD, CLPF_T_NET, CLPF_T_SOC = (FULL_CONSTANTS[k] for k in ('CLPF_T_ACTION', 'CLPF_T_REWARD', 'CLPF_T_NET', 'CLPF_T_SOC'))
CLPF_D_SOC, CLPF_D_CS, CLPF_D_HS, CLPF_D_DS, CLPF_D_NET = (FULL_CONSTANTS[k] for k in ('CLPF_D_SOC', 'CLPF_D_CS', 'CLPF_D_HS', 'CLPF_D_DS', 'CLPF_D_NET'))
CLPF_A_ES, CLPF_A_CS, CLPF_A_HS, CLPF_A_DS = (FULL_CONSTANTS[k] for k in ('CLPF_A_ES', 'CLPF_A_CS', 'CLPF_A_HS', 'CLPF_A_DS'))
assert FULL_CONSTANTS['CLPF_NOISE_KEY'] == CLPOL_NOISE_KEY                       # `noise_host` replays both kernels' streams
# two hidden layers (csrc/cl_policy_deep.h, libcitylearn_amd_policy_deep.so): the record and the noise stream are the lean kernel's
DEEP_CONSTANTS = _header_constants(_lib.POLICY_DEEP.header, 'CLPD_')
CLPD_MAX_HIDDEN, CLPD_MATRIX_CORES = DEEP_CONSTANTS['CLPD_MAX_HIDDEN'], DEEP_CONSTANTS['CLPD_MATRIX_CORES']
# two hidden layers on a thermal district (csrc/cl_policy_full_deep.h, libcitylearn_amd_policy_full_deep.so): the record and the noise stream are
# the thermal kernel's
FULL_DEEP_CONSTANTS = _header_constants(_lib.POLICY_FULL_DEEP.header, 'CLPFD_')
CLPFD_MAX_HIDDEN, CLPFD_MATRIX_CORES = FULL_DEEP_CONSTANTS['CLPFD_MAX_HIDDEN'], FULL_DEEP_CONSTANTS['CLPFD_MATRIX_CORES']
# a central agent (csrc/cl_policy_central.h, libcitylearn_amd_policy_central.so): the record and the noise stream are the lean kernel's
CENTRAL_CONSTANTS = _header_constants(_lib.POLICY_CENTRAL.header, 'CLPCA_')
CLPCA_MAX_HIDDEN, CLPCA_MAX_BLDG = CENTRAL_CONSTANTS['CLPCA_MAX_HIDDEN'], CENTRAL_CONSTANTS['CLPCA_MAX_BLDG']
# ... with two hidden layers (csrc/cl_policy_central.h at DEEP = true, libcitylearn_amd_policy_central_deep.so)
CENTRAL_DEEP_CONSTANTS = _header_constants(_lib.POLICY_CENTRAL_DEEP.header, 'CLPCD_')
CLPCD_MAX_HIDDEN, CLPCD_MAX_BLDG = CENTRAL_DEEP_CONSTANTS['CLPCD_MAX_HIDDEN'], CENTRAL_DEEP_CONSTANTS['CLPCD_MAX_BLDG']
# a central agent on a thermal district (csrc/cl_policy_full_central.h, libcitylearn_amd_policy_full_central.so): the record and the noise stream
# are the thermal kernel's
FULL_CENTRAL_CONSTANTS = _header_constants(_lib.POLICY_FULL_CENTRAL.header, 'CLPFCA_')
CLPFCA_MAX_HIDDEN, CLPFCA_MAX_BLDG = FULL_CENTRAL_CONSTANTS['CLPFCA_MAX_HIDDEN'], FULL_CENTRAL_CONSTANTS['CLPFCA_MAX_BLDG']
# ... with two hidden layers (csrc/cl_policy_full_central.h at DEEP = true, libcitylearn_amd_policy_full_central_deep.so)
FULL_CENTRAL_DEEP_CONSTANTS = _header_constants(_lib.POLICY_FULL_CENTRAL_DEEP.header, 'CLPFCD_')
CLPFCD_MAX_HIDDEN, CLPFCD_MAX_BLDG = FULL_CENTRAL_DEEP_CONSTANTS['CLPFCD_MAX_HIDDEN'], FULL_CENTRAL_DEEP_CONSTANTS['CLPFCD_MAX_BLDG']
HEAD_NAMES = ('electrical_storage', 'cooling_storage', 'heating_storage', 'dhw_storage')                  # heads in CLPF_A_* order


def building_columns(layout: ObservationLayout) -> List[List[int]]:
    """For every building, the columns of the env's observation tensor that make up ITS observation vector, in the order of
    ``layout.building_names[i]`` (a central agent's tensor keeps a shared observation once, at the first building that has it)."""
    index = {}
    for c, (i, k) in enumerate(layout.columns):
        index.setdefault((i, k), c)
    first = {}
    for c, (i, k) in enumerate(layout.columns):
        first.setdefault(k, c)
    return [[index[(i, k)] if (i, k) in index else first[k] for k in names] for i, names in enumerate(layout.building_names)]


def philox_uniform_host(seed: int, env, col: int, t: int) -> np.ndarray:
    """`cl_philox_uniform(seed, env, col, t)` (csrc/cl_philox.h: Philox4x32-10, word t & 3 of block t >> 2, 24 bits -> [0, 1)) for an array of
    env indices, in numpy -- tests/test_policy_host.py pins it to the library's function."""
    M = np.uint64(0xFFFFFFFF)
    c0 = np.asarray(env, dtype=np.uint64) & M
    c1, c2, c3 = np.full_like(c0, int(col)), np.full_like(c0, int(t) >> 2), np.zeros_like(c0)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & M, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & M
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    word = (c0, c1, c2, c3)[int(t) & 3]
    return (word >> np.uint64(8)).astype(np.float64) / 16777216.0


def noise_host(seed: int, env, col: int, t: int) -> np.ndarray:
    """The kernel's standard normal of (global env index = env_offset + env, action column, step), replayed on the host in float64:
    z = sqrt(-2 ln(u1 + 2^-25)) cos(2 pi u2) on draws 2 t and 2 t + 1 of the stream keyed seed ^ CLPOL_NOISE_KEY, with u1 + 2^-25 rounded to
    float32 as the header defines it."""
    key = (int(seed) ^ CLPOL_NOISE_KEY) & (2 ** 64 - 1)
    u1 = philox_uniform_host(key, env, col, 2 * int(t)).astype(np.float32)
    u2 = philox_uniform_host(key, env, col, 2 * int(t) + 1)
    x = (u1 + np.float32(2.0 ** -25)).astype(np.float64)
    return np.sqrt(-2.0 * np.log(x)) * np.cos(2.0 * np.pi * u2)


class _Tables:
    """A policy's `pack` result: the tables of the kind's struct (`clpol_mlp` / `clpf_mlp`) as float32 tensors on one device (the layouts of
    the header), and on the host what `actions_host(..., tables=this)` evaluates the reference with: ``cols`` (int64), ``low_bldg`` /
    ``high_bldg`` / ``sigma_bldg`` (float64) -- every head's action column (-1: none), that column's bounds and sigma."""
    kind: '_Kind'                                                        # set by the kind that names the class

    def __init__(self, pre, dep, out, net_reset, act_low, act_high, sigma, set_of_block, cols, low_bldg, high_bldg, sigma_bldg, n_device_cols, version):
        self.pre, self.dep, self.out, self.net_reset = pre, dep, out, net_reset
        self.act_low, self.act_high, self.sigma, self.set_of_block = act_low, act_high, sigma, set_of_block
        self.cols, self.low_bldg, self.high_bldg, self.sigma_bldg = cols, low_bldg, high_bldg, sigma_bldg
        self.n_device_cols = int(n_device_cols)                          # (the struct's third word: 0, device action columns are refused)
        self.version = version                                           # the policy's `version` the tables were packed from
        self.n_sets, self.n_rows, self.n_bldg, self.n_hidden = (int(x) for x in pre.shape)

    def struct(self, seed: int):
        p = lambda t: None if t is None else t.data_ptr()
        return self.kind.struct(self.n_hidden, self.n_sets, self.n_device_cols, 0, p(self.pre), p(self.dep), p(self.out), p(self.set_of_block),
                                p(self.net_reset), p(self.act_low), p(self.act_high), p(self.sigma), int(seed) & (2 ** 64 - 1))


class PolicyTables(_Tables):
    """`MLPPolicy.pack`'s result (`_Tables`), ``[n_bldg]`` on the host side: `es_cols` = every building's storage action column."""

    def __init__(self, pre, dep, out, net_reset, act_low, act_high, sigma, set_of_block, es_cols, low_bldg, high_bldg, sigma_bldg, version):
        super().__init__(pre, dep, out, net_reset, act_low, act_high, sigma, set_of_block, es_cols, low_bldg, high_bldg, sigma_bldg, 0, version)

    es_cols = property(lambda self: self.cols)


class StoragePolicyTables(_Tables):
    """`StorageMLPPolicy.pack`'s result (`_Tables`), ``[n_bldg, CLPF_NA]`` on the host side."""


class DeepPolicyTables(_Tables):
    """`DeepMLPPolicy.pack`'s result: `PolicyTables`' members for the first layer (``pre`` / ``dep``), then the second layer ``l2`` in the layout
    of the kernel family ``matrix_cores`` names, and ``out = [w3 | b3]`` ``[n_sets, n_bldg, H2 + 1]``.  ``n_hidden`` is H1, ``n_hidden2`` H2.

    ``matrix_cores=False`` (exact fp32): ``l2 [n_sets, n_bldg, H1 + 1, H2]`` -- ``ACT_SCALE * W2`` TRANSPOSED (one row per first-layer unit: the
    H2 weights the kernel's inner loop reads are consecutive), ``ACT_SCALE * b2`` as the last row.

    ``matrix_cores=True`` (f16 matrix cores, split operands): ``l2 [n_sets, n_bldg, 1024 + 32 + 4]`` -- the A-operand fragments of
    ``W' = sw * ACT_SCALE * W2`` zero-padded to 32 x 32, ``[kk][term][lane][8]`` f16 (two per float32 word) with element ``[lane][j]`` = term of
    ``W'[lane & 31][16 kk + 8 (lane >> 5) + j]``, terms ``A0 = f16(W')``, ``A1 = f16(2^11 (W' - A0))`` (`l2_fragments` reads them back); then
    ``2^12 * sw * ACT_SCALE * b2`` zero-padded to 32; then ``inv = 2^-12 / sw`` and three zeros.  ``sw`` is the power of two that puts the
    building's largest ``|ACT_SCALE * W2|`` into ``[2^13, 2^14)``: no f16 term that matters is subnormal (csrc/cl_policy_deep.h says why)."""

    def __init__(self, pre, dep, l2, out, net_reset, act_low, act_high, sigma, set_of_block, es_cols, low_bldg, high_bldg, sigma_bldg, version,
                 matrix_cores=False):
        super().__init__(pre, dep, out, net_reset, act_low, act_high, sigma, set_of_block, es_cols, low_bldg, high_bldg, sigma_bldg, 0, version)
        self.l2, self.n_hidden2, self.matrix_cores = l2, int(out.shape[-1]) - 1, bool(matrix_cores)

    es_cols = property(lambda self: self.cols)

    def struct(self, seed: int):
        p = lambda t: None if t is None else t.data_ptr()
        return self.kind.struct(self.n_hidden, self.n_sets, CLPD_MATRIX_CORES if self.matrix_cores else 0, 0, p(self.pre), p(self.dep), p(self.out),
                                p(self.set_of_block), p(self.net_reset), p(self.act_low), p(self.act_high), p(self.sigma), int(seed) & (2 ** 64 - 1),
                                self.n_hidden2, 0, p(self.l2))

    def l2_fragments(self) -> np.ndarray:
        """``matrix_cores=True``: the two f16 terms ``A0``, ``A1`` reassembled from the fragments as they are stored, float32
        ``[2, n_sets, n_bldg, 32, 32]`` (term, then ``[unit of layer 2][unit of layer 1]``): ``(A0 + 2^-11 A1) * 2^12 * inv`` is
        ``ACT_SCALE * W2``, with ``inv = l2[..., 1056]``."""
        raw = np.ascontiguousarray(self.l2.cpu().numpy()[:, :, :1024]).view(np.float16).reshape(self.n_sets, self.n_bldg, 2, 2, 64, 8)
        lane, j = np.arange(64), np.arange(8)
        w = np.zeros((2, self.n_sets, self.n_bldg, 32, 32), dtype=np.float32)
        for kk in range(2):
            k = 16 * kk + 8 * (lane[:, None] >> 5) + j[None, :]
            for term in range(2):
                w[term][:, :, (lane & 31)[:, None], k] = raw[:, :, kk, term].astype(np.float32)
        return w


class DeepStoragePolicyTables(_Tables):
    """`DeepStorageMLPPolicy.pack`'s result: `StoragePolicyTables`' members for the first layer (``pre`` / ``dep [n_sets, n_bldg, CLPF_ND, H1]``) and
    the host side ``[n_bldg, CLPF_NA]``, then the second layer ``l2`` in the layout of the kernel family ``matrix_cores`` names -- the two layouts
    of `DeepPolicyTables`, layer 2 is the same matrix problem -- and ``out = [w3 | b3]`` ``[n_sets, n_bldg, CLPF_NA, H2 + 1]``.  ``n_hidden`` is H1,
    ``n_hidden2`` H2."""

    def __init__(self, pre, dep, l2, out, net_reset, act_low, act_high, sigma, set_of_block, cols, low_bldg, high_bldg, sigma_bldg, version,
                 matrix_cores=False):
        super().__init__(pre, dep, out, net_reset, act_low, act_high, sigma, set_of_block, cols, low_bldg, high_bldg, sigma_bldg, 0, version)
        self.l2, self.n_hidden2, self.matrix_cores = l2, int(out.shape[-1]) - 1, bool(matrix_cores)

    def struct(self, seed: int):
        p = lambda t: None if t is None else t.data_ptr()
        return self.kind.struct(self.n_hidden, self.n_sets, self.n_device_cols, 0, p(self.pre), p(self.dep), p(self.out), p(self.set_of_block),
                                p(self.net_reset), p(self.act_low), p(self.act_high), p(self.sigma), int(seed) & (2 ** 64 - 1),
                                self.n_hidden2, CLPFD_MATRIX_CORES if self.matrix_cores else 0, p(self.l2))

    l2_fragments = DeepPolicyTables.l2_fragments


class CentralPolicyTables(_Tables):
    """`CentralMLPPolicy.pack`'s result.  ``pre [n_sets, n_rows, H]`` has NO building axis (one hidden layer for the district); ``dep
    [n_sets, H / 4, n_bldg, 2, 4]`` holds, per group of four hidden units and building, the four soc weights then the four net weights
    (``ACT_SCALE * W1[j][c] * col_scale[c]``, 0 where the building has no such column) -- the order the kernel walks them in; ``out = [w2 | b2]``
    ``[n_sets, n_bldg, H + 1]``.  The host side is `PolicyTables`': ``[n_bldg]`` each, `es_cols` = every building's storage action column (-1: an
    undriven building, which feeds the hidden layer and has no head)."""

    def __init__(self, pre, dep, out, net_reset, act_low, act_high, sigma, set_of_block, es_cols, low_bldg, high_bldg, sigma_bldg, version):
        self.pre, self.dep, self.out, self.net_reset = pre, dep, out, net_reset
        self.act_low, self.act_high, self.sigma, self.set_of_block = act_low, act_high, sigma, set_of_block
        self.cols, self.low_bldg, self.high_bldg, self.sigma_bldg = es_cols, low_bldg, high_bldg, sigma_bldg
        self.n_device_cols = 0                                           # (the struct's third word: clpca_mlp.flags)
        self.version = version
        self.n_sets, self.n_rows, self.n_hidden = (int(x) for x in pre.shape)
        self.n_bldg = int(out.shape[1])

    es_cols = property(lambda self: self.cols)

    def dep_terms(self) -> torch.Tensor:
        """``dep`` as ``[n_sets, n_bldg, 2, H]`` (building, term soc / net, hidden unit): `PolicyTables.dep`'s axes."""
        S, G, B = self.n_sets, self.n_hidden // 4, self.n_bldg
        return self.dep.reshape(S, G, B, 2, 4).permute(0, 2, 3, 1, 4).reshape(S, B, 2, G * 4)


class DeepCentralPolicyTables(CentralPolicyTables):
    """`DeepCentralMLPPolicy.pack`'s result: `CentralPolicyTables`' members for the first layer (``pre [n_sets, n_rows, H1]``, ``dep
    [n_sets, H1 / 4, n_bldg, 2, 4]``) and the host side, then the second layer ``l2 [n_sets, H1 + 1, H2]`` -- ``ACT_SCALE * W2`` TRANSPOSED (one row
    per first-layer unit), ``ACT_SCALE * b2`` as the last row: `DeepPolicyTables`' exact-fp32 layout without the building axis -- and
    ``out = [w3 | b3]`` ``[n_sets, n_bldg, H2 + 1]``.  ``n_hidden`` is H1, ``n_hidden2`` H2."""

    def __init__(self, pre, dep, l2, out, net_reset, act_low, act_high, sigma, set_of_block, es_cols, low_bldg, high_bldg, sigma_bldg, version):
        super().__init__(pre, dep, out, net_reset, act_low, act_high, sigma, set_of_block, es_cols, low_bldg, high_bldg, sigma_bldg, version)
        self.l2, self.n_hidden2 = l2, int(out.shape[-1]) - 1

    def struct(self, seed: int):
        p = lambda t: None if t is None else t.data_ptr()
        return self.kind.struct(self.n_hidden, self.n_sets, 0, 0, p(self.pre), p(self.dep), p(self.out), p(self.set_of_block), p(self.net_reset),
                                p(self.act_low), p(self.act_high), p(self.sigma), int(seed) & (2 ** 64 - 1), self.n_hidden2, 0, p(self.l2))


class CentralStoragePolicyTables(CentralPolicyTables):
    """`CentralStorageMLPPolicy.pack`'s result.  ``pre [n_sets, n_rows, H]`` has NO building axis; ``dep [n_sets, H / 4, n_bldg, CLPF_ND, 4]`` holds,
    per group of four hidden units and building, the four weights of each of the five terms in `CLPF_D_*` order (``ACT_SCALE * W1[j][c] *
    col_scale[c]``, 0 where the building has no such column or storage) -- the order the kernel walks them in; ``out = [w2 | b2]``
    ``[n_sets, n_bldg, CLPF_NA, H + 1]``.  The host side is `StoragePolicyTables`': ``[n_bldg, CLPF_NA]`` each, ``cols`` = every head's action
    column (-1: none)."""

    def __init__(self, pre, dep, out, net_reset, act_low, act_high, sigma, set_of_block, cols, low_bldg, high_bldg, sigma_bldg, version):
        super().__init__(pre, dep, out, net_reset, act_low, act_high, sigma, set_of_block, cols, low_bldg, high_bldg, sigma_bldg, version)
        self.n_device_cols = 0                                           # (the struct's third word: refused by `pack` otherwise)

    es_cols = property(lambda self: self.cols[:, CLPF_A_ES])

    def dep_terms(self) -> torch.Tensor:
        """``dep`` as ``[n_sets, n_bldg, CLPF_ND, H]`` (building, term, hidden unit): `StoragePolicyTables.dep`'s axes."""
        S, G, B = self.n_sets, self.n_hidden // 4, self.n_bldg
        return self.dep.reshape(S, G, B, CLPF_ND, 4).permute(0, 2, 3, 1, 4).reshape(S, B, CLPF_ND, G * 4)


class DeepCentralStoragePolicyTables(CentralStoragePolicyTables):
    """`DeepCentralStorageMLPPolicy.pack`'s result: `CentralStoragePolicyTables`' members for the first layer (``pre [n_sets, n_rows, H1]``, ``dep
    [n_sets, H1 / 4, n_bldg, CLPF_ND, 4]``) and the host side ``[n_bldg, CLPF_NA]``, then the second layer ``l2 [n_sets, H1 + 1, H2]`` --
    ``ACT_SCALE * W2`` TRANSPOSED (one row per first-layer unit), ``ACT_SCALE * b2`` as the last row: `DeepCentralPolicyTables`' layout -- and
    ``out = [w3 | b3]`` ``[n_sets, n_bldg, CLPF_NA, H2 + 1]``.  ``n_hidden`` is H1, ``n_hidden2`` H2."""

    def __init__(self, pre, dep, l2, out, net_reset, act_low, act_high, sigma, set_of_block, cols, low_bldg, high_bldg, sigma_bldg, version):
        super().__init__(pre, dep, out, net_reset, act_low, act_high, sigma, set_of_block, cols, low_bldg, high_bldg, sigma_bldg, version)
        self.l2, self.n_hidden2 = l2, int(out.shape[-1]) - 1

    def struct(self, seed: int):
        p = lambda t: None if t is None else t.data_ptr()
        return self.kind.struct(self.n_hidden, self.n_sets, self.n_device_cols, 0, p(self.pre), p(self.dep), p(self.out), p(self.set_of_block),
                                p(self.net_reset), p(self.act_low), p(self.act_high), p(self.sigma), int(seed) & (2 ** 64 - 1), self.n_hidden2, 0,
                                p(self.l2))


def _l2_fragments(w2s: np.ndarray, b2s: np.ndarray) -> np.ndarray:
    """The matrix-core layout of layer 2 (`DeepPolicyTables`) from the scaled weights ``[S, B, H2, H1]`` and biases ``[S, B, H2]`` (float64):
    float32 ``[S, B, 1024 + 32 + 4]``."""
    S, B, H2, H1 = w2s.shape
    amax = np.abs(w2s).reshape(S, B, -1).max(axis=2)
    if not np.all(np.isfinite(amax)):
        raise ValueError('w2 is not finite')
    sw = 2.0 ** np.clip(13 - np.floor(np.log2(np.where(amax > 0, amax, 1.0))), -100, 100)         # amax * sw in [2^13, 2^14)
    W = np.zeros((S, B, 32, 32), dtype=np.float32)
    W[:, :, :H2, :H1] = (w2s * sw[:, :, None, None]).astype(np.float32)
    lane, j = np.arange(64), np.arange(8)
    frag = np.zeros((S, B, 2, 2, 64, 8), dtype=np.float16)
    for kk in range(2):
        k = 16 * kk + 8 * (lane[:, None] >> 5) + j[None, :]                     # [64, 8]: the first-layer unit of (lane, slot)
        x = W[:, :, (lane & 31)[:, None], k]                                    # [S, B, 64, 8]
        t0 = x.astype(np.float16)
        frag[:, :, kk, 0] = t0
        frag[:, :, kk, 1] = ((x - t0.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)      # (residual and scaling exact in fp32)
    tail = np.zeros((S, B, 32 + 4), dtype=np.float32)
    tail[:, :, :H2] = b2s * (4096.0 * sw[:, :, None])
    tail[:, :, 32] = 1.0 / (4096.0 * sw)
    return np.concatenate([frag.reshape(S, B, -1).view(np.float32), tail], axis=2)


@dataclass(frozen=True)
class _Kind:
    """What tells the two policies apart, as data -- the packer, the references and `rollout_policy` read it and are written once."""
    terms: Tuple[tuple, ...]          # the env-dependent inputs in `dep`'s row order: ((source kind, plane), building flag that gates the term | None)
    head_slots: Tuple[int, ...]       # per head, the slot of `tab.params` that holds its action column
    head_shape: Tuple[int, ...]       # the head axis of w2 / b2 / out / cols: () for the single head without one
    refuse_device_actions: bool
    only: str                         # the wrong-plane refusal: what the kernel does have
    tables: type
    struct: type
    constants: dict                   # the header's
    max_hidden: int
    n_planes: int                     # of a recorded trajectory
    ext: '_lib._Extension'            # the rollout library, and the one that also keeps the streaming KPIs
    ext_kpi: Optional['_lib._Extension']              # (None: the kind has no KPI kernel -- `rollout_policy(kpi=True)` raises NotImplementedError)
    no_kpi_error: type                # what `rollout_policy(kpi=True)` raises on a build without KPIs
    ext_chunk: Optional['_lib._Extension'] = None      # the building-chunked rollout library (`rollout_policy(chunked=True)`), where the kind has one
    ext_chunk_kpi: Optional['_lib._Extension'] = None  # ... and the one that also keeps the streaming KPIs (`rollout_policy(chunked=True, kpi=True)`)
    ext_chunk_pair: Optional['_lib._Extension'] = None  # the chunked library of a kind that runs TWO buildings per wave (no KPI twin yet)
    one_row_max: int = 16             # buildings one workgroup row holds: beyond it `VectorCityLearnEnv.rollout_policy` asks for the chunked launch
    central: bool = False             # ONE MLP over the district's central-agent observation vector (`CentralMLPPolicy`), not one per building

    def __post_init__(self):
        self.tables.kind = self


_DEVICE_SLOTS = (('cooling_device', abi.CLP_ACT_COOL_DEV), ('heating_device', abi.CLP_ACT_HEAT_DEV), ('cooling_or_heating_device', abi.CLP_ACT_COH_DEV))
_LEAN = _Kind(terms=(((SRC_STATE, abi.CLS_B_SOC), None), ((SRC_OUT, abi.CLO_NET), None)), head_slots=(abi.CLP_ACT_ELEC_STO,), head_shape=(),
              refuse_device_actions=False,
              only="the policy kernel only has the building's own electrical_storage_soc (CLS_B_SOC) and net_electricity_consumption (CLO_NET)",
              tables=PolicyTables, struct=_lib.PolicyMLP, constants=CONSTANTS, max_hidden=CLPOL_MAX_HIDDEN, n_planes=CLPOL_NT,
              ext=_lib.POLICY, ext_kpi=_lib.POLICY_KPI, no_kpi_error=ValueError, ext_chunk_pair=_lib.POLICY_CHUNK, one_row_max=32)
_THERMAL = _Kind(terms=(((SRC_STATE, abi.CLS_B_SOC), abi.CLF_BATTERY), ((SRC_STATE, abi.CLS_CS_SOC), abi.CLF_COOL_STO), ((SRC_STATE, abi.CLS_HS_SOC), abi.CLF_HEAT_STO),
                        ((SRC_STATE, abi.CLS_DS_SOC), abi.CLF_DHW_STO), ((SRC_OUT, abi.CLO_NET), None)),           # rows CLPF_D_SOC, _CS, _HS, _DS, _NET
                 head_slots=(abi.CLP_ACT_ELEC_STO, abi.CLP_ACT_COOL_STO, abi.CLP_ACT_HEAT_STO, abi.CLP_ACT_DHW_STO), head_shape=(CLPF_NA,),    # CLPF_A_*
                 refuse_device_actions=True,
                 only="the thermal policy kernel only has the building's own storage socs (CLS_B_SOC, CLS_CS_SOC, CLS_HS_SOC, CLS_DS_SOC) and "
                      'net_electricity_consumption (CLO_NET)',
                 tables=StoragePolicyTables, struct=_lib.PolicyFullMLP, constants=FULL_CONSTANTS, max_hidden=CLPF_MAX_HIDDEN, n_planes=CLPF_NT,
                 ext=_lib.POLICY_FULL, ext_kpi=_lib.POLICY_FULL_KPI, no_kpi_error=NotImplementedError, ext_chunk=_lib.POLICY_FULL_CHUNK,
                 ext_chunk_kpi=_lib.POLICY_FULL_CHUNK_KPI, one_row_max=16)
# two hidden layers: the lean kind's inputs, head, record and one-row geometry; a library of its own and neither a KPI nor a chunked twin
_DEEP = _Kind(terms=_LEAN.terms, head_slots=_LEAN.head_slots, head_shape=(), refuse_device_actions=False, only=_LEAN.only, tables=DeepPolicyTables,
              struct=_lib.PolicyDeepMLP, constants=DEEP_CONSTANTS, max_hidden=CLPD_MAX_HIDDEN, n_planes=CLPOL_NT, ext=_lib.POLICY_DEEP, ext_kpi=None,
              no_kpi_error=NotImplementedError, one_row_max=32)
# two hidden layers on a thermal district: the thermal kind's inputs, heads, record and one-row geometry; a library of its own and neither a KPI nor
# a chunked twin
_DEEP_THERMAL = _Kind(terms=_THERMAL.terms, head_slots=_THERMAL.head_slots, head_shape=_THERMAL.head_shape, refuse_device_actions=True, only=_THERMAL.only,
                      tables=DeepStoragePolicyTables, struct=_lib.PolicyFullDeepMLP, constants=FULL_DEEP_CONSTANTS, max_hidden=CLPFD_MAX_HIDDEN,
                      n_planes=CLPF_NT, ext=_lib.POLICY_FULL_DEEP, ext_kpi=None, no_kpi_error=NotImplementedError, one_row_max=16)
# a central agent: the lean kind's inputs (of EVERY building), heads, record and one-row geometry; a library of its own and neither a KPI nor a
# chunked twin
_CENTRAL = _Kind(terms=_LEAN.terms, head_slots=_LEAN.head_slots, head_shape=(), refuse_device_actions=False, only=_LEAN.only, tables=CentralPolicyTables,
                 struct=_lib.PolicyMLP, constants=CENTRAL_CONSTANTS, max_hidden=CLPCA_MAX_HIDDEN, n_planes=CLPOL_NT, ext=_lib.POLICY_CENTRAL, ext_kpi=None,
                 no_kpi_error=NotImplementedError, one_row_max=CLPCA_MAX_BLDG, central=True)
# a central agent with two hidden layers: the central kind's inputs, heads, record and geometry; a library of its own once more
_CENTRAL_DEEP = _Kind(terms=_LEAN.terms, head_slots=_LEAN.head_slots, head_shape=(), refuse_device_actions=False, only=_LEAN.only,
                      tables=DeepCentralPolicyTables, struct=_lib.PolicyDeepMLP, constants=CENTRAL_DEEP_CONSTANTS, max_hidden=CLPCD_MAX_HIDDEN,
                      n_planes=CLPOL_NT, ext=_lib.POLICY_CENTRAL_DEEP, ext_kpi=None, no_kpi_error=NotImplementedError, one_row_max=CLPCD_MAX_BLDG,
                      central=True)
# a central agent on a thermal district: the thermal kind's inputs (of EVERY building), heads, record and one-row geometry; a library of its own and
# neither a KPI nor a chunked twin
_CENTRAL_THERMAL = _Kind(terms=_THERMAL.terms, head_slots=_THERMAL.head_slots, head_shape=(CLPF_NA,), refuse_device_actions=True, only=_THERMAL.only,
                         tables=CentralStoragePolicyTables, struct=_lib.PolicyFullMLP, constants=FULL_CENTRAL_CONSTANTS, max_hidden=CLPFCA_MAX_HIDDEN,
                         n_planes=CLPF_NT, ext=_lib.POLICY_FULL_CENTRAL, ext_kpi=None, no_kpi_error=NotImplementedError, one_row_max=CLPFCA_MAX_BLDG,
                         central=True)
# a central agent with two hidden layers on a thermal district: the central thermal kind's inputs, heads, record and geometry; a library of its own
# once more
_CENTRAL_DEEP_THERMAL = _Kind(terms=_THERMAL.terms, head_slots=_THERMAL.head_slots, head_shape=(CLPF_NA,), refuse_device_actions=True, only=_THERMAL.only,
                              tables=DeepCentralStoragePolicyTables, struct=_lib.PolicyFullDeepMLP, constants=FULL_CENTRAL_DEEP_CONSTANTS,
                              max_hidden=CLPFCD_MAX_HIDDEN, n_planes=CLPF_NT, ext=_lib.POLICY_FULL_CENTRAL_DEEP, ext_kpi=None,
                              no_kpi_error=NotImplementedError, one_row_max=CLPFCD_MAX_BLDG, central=True)
# (terms and heads above are written in the header's order)
assert (CLPF_D_SOC, CLPF_D_CS, CLPF_D_HS, CLPF_D_DS, CLPF_D_NET) == tuple(range(CLPF_ND)) and (CLPF_A_ES, CLPF_A_CS, CLPF_A_HS, CLPF_A_DS) == tuple(range(CLPF_NA))


def _head_columns(tab, kind: _Kind) -> np.ndarray:
    hc = np.ascontiguousarray(tab.params).view(np.int32)[:, list(kind.head_slots)].astype(np.int64)
    return hc if kind.head_shape else hc[:, 0]


def head_columns(tab) -> np.ndarray:
    """``[n_bldg, CLPF_NA]`` the action column of every building's electrical / cooling / heating / DHW storage (-1: none), as the kernel reads them."""
    return _head_columns(tab, _THERMAL)


class _MLPBase:
    """What `MLPPolicy` and `StorageMLPPolicy` share: everything but the class's `kind`, the contraction of the hidden layer with the head(s)
    (`_heads`, `_heads_torch`) and the signature of `actions_host`."""
    kind: _Kind

    def __init__(self, w1, b1, w2, b2, sigma=None):
        self.w1, self.b1, self.w2, self.b2 = (np.asarray(x, dtype=np.float64) for x in (w1, b1, w2, b2))
        hs = self.kind.head_shape
        if self.w1.ndim != 4 or self.b1.ndim != 3 or self.w2.ndim != 3 + len(hs) or self.b2.ndim != 2 + len(hs):
            heads = ''.join(f', {n}' for n in hs)
            raise ValueError(f'w1 [n_sets, n_bldg, H, n_obs], b1 [n_sets, n_bldg, H], w2 [n_sets, n_bldg{heads}, H], b2 [n_sets, n_bldg{heads}]')
        self.n_hidden, self.n_obs = int(self.w1.shape[2]), int(self.w1.shape[3])
        if self.n_hidden % 4 or not 4 <= self.n_hidden <= self.kind.max_hidden:
            raise ValueError(f'H={self.n_hidden}: the policy kernel takes 4, 8, .. {self.kind.max_hidden} hidden units')
        if self.b1.shape[2] != self.n_hidden or self.w2.shape[2:] != hs + (self.n_hidden,) or self.b2.shape[2:] != hs:
            raise ValueError('b1 / w2 / b2 disagree with w1 about H' + ''.join(f', or do not have {n} heads' for n in hs))
        self.n_sets = max(x.shape[0] for x in (self.w1, self.b1, self.w2, self.b2))
        self.sigma = None if sigma is None else np.asarray(sigma, dtype=np.float64)
        self.version = 0

    def invalidate(self) -> None:
        """Tell the caches that the weights changed (see `MLPPolicy`'s docstring)."""
        self.version += 1

    def update(self, w1=None, b1=None, w2=None, b2=None, sigma=None) -> None:
        """Replace some of the weight arrays (same shapes) and / or sigma, and bump `version`: the learner's step between two rollouts."""
        for name, v in (('w1', w1), ('b1', b1), ('w2', w2), ('b2', b2)):
            if v is not None:
                v = np.asarray(v, dtype=np.float64)
                if v.shape != getattr(self, name).shape:
                    raise ValueError(f'{name}: shape {v.shape} != {getattr(self, name).shape}')
                setattr(self, name, v)
        if sigma is not None:
            self.sigma = np.asarray(sigma, dtype=np.float64)
        self.invalidate()

    def _full(self, n_bldg: int):
        S, H, hs = self.n_sets, self.n_hidden, self.kind.head_shape
        try:
            return (np.broadcast_to(self.w1, (S, n_bldg, H, self.n_obs)), np.broadcast_to(self.b1, (S, n_bldg, H)),
                    np.broadcast_to(self.w2, (S, n_bldg) + hs + (H,)), np.broadcast_to(self.b2, (S, n_bldg) + hs))
        except ValueError as e:
            raise ValueError(f'the weights do not broadcast to {S} sets x {n_bldg} buildings: {e}') from None

    # ---- the reference: the UNSPLIT MLP in float64 ------------------------------------------------------------------------------
    def _actions_host(self, obs_vectors, lo, hi, noise, sigma, set_index: int) -> np.ndarray:
        """``clip(mid + half tanh(heads) + sigma() noise, lo, hi)`` in float64 numpy (`sigma` is only called where there is noise)."""
        x = np.asarray(obs_vectors, dtype=np.float64)
        w1, b1, w2, b2 = (v[set_index] for v in self._full(x.shape[-2]))
        h = np.tanh(np.einsum('bjc,...bc->...bj', w1, x) + b1)
        a = 0.5 * (hi + lo) + 0.5 * (hi - lo) * np.tanh(self._heads(w2, h) + b2)
        if noise is not None:
            a = a + sigma() * np.asarray(noise, dtype=np.float64)
        return np.clip(a, lo, hi)

    def torch_policy(self, layout: ObservationLayout, tab, device, dtype=torch.float32, set_index: int = 0):
        """The same MLP (no noise) written in torch over the env's observation TENSOR (``observations='tensor'``): returns
        ``f(obs [n_envs, n_obs_total], i=None) -> actions [n_act_cols, n_envs]`` -- a `VectorCityLearnEnv.capture_rollout` policy; what
        `rollout_policy` replaces with one launch, and what the tests compare it with."""
        cols = building_columns(layout)
        w1, b1, w2, b2 = (torch.as_tensor(np.array(v[set_index]), dtype=dtype, device=device) for v in self._full(len(cols)))
        idx = torch.as_tensor(np.array([c + [c[0]] * (self.n_obs - len(c)) for c in cols]), device=device)
        mask = torch.as_tensor(np.array([[1.0] * len(c) + [0.0] * (self.n_obs - len(c)) for c in cols]), dtype=dtype, device=device)
        hc = _head_columns(tab, self.kind)
        low, high = layout.spec.action_limits()
        sel = np.nonzero(hc >= 0)                                                # the heads that have a column
        rows = torch.as_tensor(hc[sel], device=device)
        lo = torch.as_tensor(np.asarray(low)[hc[sel]], dtype=dtype, device=device)
        hi = torch.as_tensor(np.asarray(high)[hc[sel]], dtype=dtype, device=device)
        flat = torch.as_tensor(np.ravel_multi_index(sel, hc.shape), device=device)
        n_act = len(low)

        def f(obs, i=None):
            x = obs.to(dtype)[:, idx] * mask                                     # [E, B, n_obs]
            h = torch.tanh(torch.einsum('bjc,ebc->ebj', w1, x) + b1)
            o = torch.tanh(self._heads_torch(w2, h) + b2).reshape(obs.shape[0], -1)[:, flat]          # [E, present heads]
            a = torch.clamp(0.5 * (hi + lo) + 0.5 * (hi - lo) * o, lo, hi)
            out = torch.zeros((n_act, obs.shape[0]), dtype=torch.float32, device=obs.device)
            out[rows] = a.t().to(torch.float32)
            return out
        return f

    # ---- the kernel's tables ----------------------------------------------------------------------------------------------------
    def pack(self, layout: ObservationLayout, tab, device='cpu', set_of_block=None):
        """Split the first layer along the observation tables of `layout` over the episode tables `tab` (``layout.episode(tab,
        reset_table=True)``): the env-independent columns of every table row go into ``pre`` (one matmul in float64 on `device`, rounded
        once), the ``col_scale`` of the env-dependent columns (the kind's terms, all the building's own) into ``dep``, one row per term (the
        row of a storage the building lacks stays 0), their table offsets into ``pre``.  A building observation fed by anything else on the
        device raises ``ValueError`` naming the column.  ``set_of_block``: the parameter set of every block of ``abi.CL_ROW0_BLOCK`` envs."""
        kind = self.kind
        obs = layout.episode(tab, reset_table=True)
        cols = building_columns(layout)
        n_bldg, T = len(cols), int(obs.table.shape[0])
        if any(len(c) > self.n_obs for c in cols) or not any(len(c) == self.n_obs for c in cols):
            raise ValueError(f'w1 takes {self.n_obs} observations, the buildings have {sorted(set(len(c) for c in cols))}')
        w1, b1, w2, b2 = self._full(n_bldg)
        params_i = np.ascontiguousarray(tab.params).view(np.int32)
        bflags = np.ascontiguousarray(tab.params).view(np.uint32)[:, abi.CLP_FLAGS]
        term_of = {src: k for k, (src, _) in enumerate(kind.terms)}
        table = obs.table
        x = np.zeros((T, n_bldg, self.n_obs))
        scale = np.zeros((n_bldg, len(kind.terms), self.n_obs))          # [b][term][position in the building's vector]
        net_reset = np.zeros((T, n_bldg))
        for i, bcols in enumerate(cols):
            for j, c in enumerate(bcols):
                name = f'{layout.columns[c][1]!r} of building {i} (column {c})'
                src = int(obs.col_src[c])
                if src < 0:
                    # env-independent: the reset observation of an episode that starts at row r must show the table's value
                    if T > 1 and not np.array_equal(obs.reset_table[1:, c], table[1:, c]):
                        raise ValueError(f'observation {name} is reset to a value its table row does not hold (observation_mode="reference"?): '
                                         'the policy kernel reads the tables of observation_mode="current"')
                    x[:, i, j] = table[:, c]
                    continue
                kind_, plane, b = src >> 28, (src >> 20) & 0xFF, src & 0xFFFFF
                which = term_of.get((kind_, plane))
                if which is None or b != i or layout.columns[c][0] != i:
                    raise ValueError(f'observation {name} is fed by device plane (kind {kind_}, plane {plane}, building {b}): {kind.only}'
                                     + (' -- the indoor temperature comes from the LSTM stage' if kind_ == SRC_TEMP else ''))
                offset = table[1:, c] if T > 1 else np.zeros(1)
                if np.ptp(offset) != 0.0:
                    raise ValueError(f'observation {name}: a table offset that changes with the row')
                x[:, i, j] = offset[0]
                flag = kind.terms[which][1]
                if flag is None or int(bflags[i]) & flag:                # (a storage the building lacks: its plane stays 0, the kernel skips the term)
                    scale[i, which, j] = float(obs.col_scale[c])
                if kind.terms[which][0] == (SRC_OUT, abi.CLO_NET) and scale[i, which, j] != 0.0:
                    net_reset[:, i] = (obs.reset_table[:, c] - offset[0]) / scale[i, which, j]
        if kind.refuse_device_actions:
            for i in range(n_bldg):
                for dname, slot in _DEVICE_SLOTS:
                    if params_i[i, slot] >= 0:
                        raise ValueError(f'action {dname!r} of building {i} (column {int(params_i[i, slot])}): the thermal policy kernel has storage heads '
                                         f'only {HEAD_NAMES}; a district with device actions runs through capture_rollout')
        dev = torch.device(device)
        f64 = lambda v: torch.from_numpy(np.array(v, dtype=np.float64)).to(dev)
        pre = (torch.einsum('sbjc,tbc->stbj', f64(w1), f64(x)) + f64(b1)[:, None]) * ACT_SCALE
        dep = torch.einsum('sbjc,bkc->sbkj', f64(w1), f64(scale)) * ACT_SCALE
        out = torch.cat([f64(w2), f64(b2)[..., None]], dim=-1)
        hc = _head_columns(tab, kind)
        n_act = int(params_i[:, abi.CLP_ACT_COOL_STO:abi.CLP_ACT_COH_DEV + 1].max()) + 1
        low, high = layout.spec.action_limits()
        if len(low) != n_act:
            raise ValueError(f'{len(low)} action limits for {n_act} action columns')
        at = lambda v, fill: np.where(hc >= 0, np.asarray(v, dtype=np.float64)[np.maximum(hc, 0)], fill)
        sigma = None
        if self.sigma is not None:
            sigma = np.full(n_act, float(self.sigma)) if self.sigma.ndim == 0 else self.sigma
            if sigma.shape != (n_act,) or np.any(sigma < 0):
                raise ValueError(f'sigma: a non-negative scalar or [{n_act}] (one per action column)')
        f32 = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev)
        sob = None
        if set_of_block is not None:
            sob = np.asarray(set_of_block, dtype=np.int64).reshape(-1)
            if sob.min() < 0 or sob.max() >= self.n_sets:
                raise ValueError(f'set_of_block outside [0, {self.n_sets})')
            sob = torch.from_numpy(sob.astype(np.int32)).to(dev)
        host = (hc, at(low, -1.0), at(high, 1.0), np.zeros(hc.shape) if sigma is None else at(sigma, 0.0))
        if kind.refuse_device_actions:
            host += (0,)                                                 # (n_device_cols = 0: refused above)
        return kind.tables(pre.to(torch.float32).contiguous(), dep.to(torch.float32).contiguous(), out.to(torch.float32).contiguous(),
                           f32(net_reset), f32(low), f32(high), f32(sigma), sob, *host, self.version)


class MLPPolicy(_MLPBase):
    """``a = clamp(mid + half tanh(w2 . tanh(W1 obs + b1) + b2) + sigma z, low, high)`` per building, `obs` = the building's own observation
    vector as the env defines it (``ObservationLayout.building_names[i]``: normalised or not, whatever the env was built with), (low, high) =
    the bounds of the building's electrical-storage action, z ~ N(0, 1).  The env-dependent inputs are the building's own
    ``electrical_storage_soc`` and ``net_electricity_consumption``.

    ``w1 [n_sets, n_bldg, H, n_obs]``, ``b1 [n_sets, n_bldg, H]``, ``w2 [n_sets, n_bldg, H]``, ``b2 [n_sets, n_bldg]`` (anything array-like;
    kept in float64); a leading dimension of 1 broadcasts -- shared weights over the buildings and / or one parameter set.  ``H``: 4, 8, .. 32.
    ``sigma``: None (deterministic), a scalar or ``[n_act_cols]``.

    **The packed tables are a snapshot.**  `pack` reads the weights once; `VectorCityLearnEnv.rollout_policy` caches the packed tables per
    (policy object, `version`, episode window).  Change the weights through :meth:`update` (or assign the arrays and call :meth:`invalidate`):
    both bump `version`, so the next `rollout_policy` packs again.  Arrays edited in place without that keep driving the OLD policy."""
    kind = _LEAN
    _heads = staticmethod(lambda w2, h: np.einsum('bj,...bj->...b', w2, h))
    _heads_torch = staticmethod(lambda w2, h: (w2 * h).sum(dim=-1))

    def actions_host(self, obs_vectors, noise=None, tables: Optional[PolicyTables] = None, low=None, high=None, sigma_bldg=None,
                     set_index: int = 0) -> np.ndarray:
        """float64 numpy evaluation of the plain MLP: ``obs_vectors [..., n_bldg, n_obs]`` -> actions ``[..., n_bldg]``.  ``noise``: the
        standard normals z (same shape as the result; `noise_host` replays the kernel's), scaled by each building's sigma.  The bounds of the
        buildings' storage actions and their sigmas (``[n_bldg]`` each) come from ``tables`` (a `pack` result: `low_bldg`, `high_bldg`,
        `sigma_bldg`) or from the arguments; without either: -1 / 1 and the policy's scalar sigma.  Nothing is remembered between calls."""
        pick = lambda arg, attr, default: np.asarray(arg if arg is not None else getattr(tables, attr) if tables is not None else default, dtype=np.float64)

        def sigma():
            if sigma_bldg is None and tables is None and self.sigma is not None and self.sigma.ndim:
                raise ValueError('a per-column sigma needs `tables` (or `sigma_bldg`): which column drives which building')
            return pick(sigma_bldg, 'sigma_bldg', 0.0 if self.sigma is None or self.sigma.ndim else float(self.sigma))
        return self._actions_host(obs_vectors, pick(low, 'low_bldg', -1.0), pick(high, 'high_bldg', 1.0), noise, sigma, set_index)


class StorageMLPPolicy(_MLPBase):
    """``act_a = clamp(mid_a + half_a tanh(w2[a] . tanh(W1 obs + b1) + b2[a]) + sigma_a z_a, low_a, high_a)`` per building and head a, the heads in
    the fixed order electrical, cooling, heating, DHW storage (`HEAD_NAMES`); `obs` = the building's own observation vector as the env defines
    it, (low_a, high_a) = the bounds of the building's action column of that storage.  The heads of columns a building lacks are ignored.  For
    thermal districts without the LSTM stage and without device actions (the 2020 / 2021 schemas): `cl_rollout_full_policy_kernel`.  FIVE
    env-dependent inputs: the building's own ``electrical_storage_soc`` / ``cooling_storage_soc`` / ``heating_storage_soc`` /
    ``dhw_storage_soc`` and ``net_electricity_consumption`` (``dep`` rows `CLPF_D_*`).  `pack` also refuses the indoor temperature of the LSTM
    stage (``SRC_TEMP``) and a building with a cooling / heating device ACTION.

    ``w1 [n_sets, n_bldg, H, n_obs]``, ``b1 [n_sets, n_bldg, H]``, ``w2 [n_sets, n_bldg, 4, H]``, ``b2 [n_sets, n_bldg, 4]`` (kept in float64); a
    leading dimension of 1 broadcasts.  ``H``: 4, 8, .. 32.  ``sigma``: None (deterministic), a scalar or ``[n_act_cols]``.

    The packed tables are a snapshot, as `MLPPolicy`'s: change the weights through :meth:`update` / :meth:`invalidate`, which bump `version`."""
    kind = _THERMAL
    _heads = staticmethod(lambda w2, h: np.einsum('baj,...bj->...ba', w2, h))
    _heads_torch = staticmethod(lambda w2, h: torch.einsum('baj,...bj->...ba', w2, h))

    def actions_host(self, obs_vectors, tables: StoragePolicyTables, noise=None, set_index: int = 0) -> np.ndarray:
        """float64 numpy evaluation of the plain MLP: ``obs_vectors [..., n_bldg, n_obs]`` -> actions ``[..., n_bldg, 4]`` (0 for a head whose
        column the building lacks).  ``noise``: the standard normals z (same shape as the result; `noise_host` replays the kernel's), scaled by
        each head's sigma.  The heads' columns, bounds and sigmas come from ``tables`` (a `pack` result).  Nothing is remembered between calls."""
        a = self._actions_host(obs_vectors, tables.low_bldg, tables.high_bldg, noise, lambda: tables.sigma_bldg, set_index)
        return np.where(tables.cols >= 0, a, 0.0)


def default_matrix_cores(n_hidden: int, n_hidden2: int, n_bldg: Optional[int] = None) -> bool:
    """What `DeepMLPPolicy.pack(matrix_cores=None)` resolves to: the matrix-core family where the probe's logs show it faster than the exact-fp32
    one by more than the spread (max - min) of its own seven repetitions AND its launch fits, the exact-fp32 family -- the fallback -- everywhere
    else.

    Fit: a matrix-core row is 1160 floats per building at every H1, H2, two rows per wave, so the sixteen waves of 31 or 32 buildings need
    164 864 bytes of LDS with the reduction rows and the library refuses them (a CU has 163 840; `_lib.policy_deep_mma_lds_bytes`).  With
    ``n_bldg`` given (`pack` gives it) such a district gets the exact-fp32 family, whose rows follow H1, H2: 32 buildings fit up to 32 x 28.

    The rule: ``H1 * H2 >= 512``.  The matrix-core kernel always computes the zero-padded 32 x 32 problem and costs the same at every size --
    19.2 - 19.6 us per step at 17 x 32 768 with the record under the float64 chain -- while the exact-fp32 kernel's cost follows H1 * H2:
    8.50 us at (8, 8), 16.87 at (16, 16), 26.95 / 26.79 at (16, 32) / (32, 16), 28.51 at (24, 24), 35.98 / 35.59 at (24, 32) / (32, 24), 40.67 at
    (32, 28), 44.89 at (32, 32).  Every measured shape with H1 * H2 >= 512 reads "matrix_cores_faster_beyond_its_spread: 8 of 8 cases" (two batch
    sizes x two precision models x record off / on), (8, 8) and (16, 16) read "0 of 8" (profiles/policy_deep_probe.log: (16, 16), (32, 32);
    profiles/policy_deep_probe_shapes.log: the others).  Between 256 and 512 nothing is measured, so the exact-fp32 family stays."""
    fits = n_bldg is None or _lib.policy_deep_mma_lds_bytes((int(n_bldg) + 1) // 2) <= _lib.LDS_PER_CU
    return n_hidden * n_hidden2 >= 512 and fits


class DeepMLPPolicy:
    """`MLPPolicy` with TWO hidden layers -- the shape of the SAC / PPO actors of the CityLearn examples -- per building:

        h1 = tanh(W1 obs + b1),   h2 = tanh(W2 h1 + b2),   a = clamp(mid + half tanh(w3 . h2 + b3) + sigma z, low, high)

    `obs`, the bounds, z and the env-dependent inputs (the building's own ``electrical_storage_soc`` and ``net_electricity_consumption``) are
    `MLPPolicy`'s.  Battery + PV districts of up to 32 buildings: one launch of `cl_rollout_policy_deep_kernel` (csrc/cl_policy_deep.h,
    ``libcitylearn_amd_policy_deep.so``).

    ``w1 [n_sets, n_bldg, H1, n_obs]``, ``b1 [n_sets, n_bldg, H1]``, ``w2 [n_sets, n_bldg, H2, H1]``, ``b2 [n_sets, n_bldg, H2]``,
    ``w3 [n_sets, n_bldg, H2]``, ``b3 [n_sets, n_bldg]`` (anything array-like; kept in float64); a leading dimension of 1 broadcasts.  ``H1``,
    ``H2``: 4, 8, .. 32, independent of each other.  ``sigma``: None (deterministic), a scalar or ``[n_act_cols]``.

    The packed tables are a snapshot, as `MLPPolicy`'s: change the weights through :meth:`update` / :meth:`invalidate`, which bump `version`."""
    kind = _DEEP
    _NAMES = ('w1', 'b1', 'w2', 'b2', 'w3', 'b3')

    def __init__(self, w1, b1, w2, b2, w3, b3, sigma=None):
        self.w1, self.b1, self.w2, self.b2, self.w3, self.b3 = (np.asarray(x, dtype=np.float64) for x in (w1, b1, w2, b2, w3, b3))
        if [getattr(self, n).ndim for n in self._NAMES] != [4, 3, 4, 3, 3, 2]:
            raise ValueError('w1 [n_sets, n_bldg, H1, n_obs], b1 [n_sets, n_bldg, H1], w2 [n_sets, n_bldg, H2, H1], b2 [n_sets, n_bldg, H2], '
                             'w3 [n_sets, n_bldg, H2], b3 [n_sets, n_bldg]')
        self.n_hidden, self.n_obs, self.n_hidden2 = int(self.w1.shape[2]), int(self.w1.shape[3]), int(self.w2.shape[2])
        for name, h in (('H1', self.n_hidden), ('H2', self.n_hidden2)):
            if h % 4 or not 4 <= h <= CLPD_MAX_HIDDEN:
                raise ValueError(f'{name}={h}: the deep policy kernel takes 4, 8, .. {CLPD_MAX_HIDDEN} units per hidden layer')
        if self.b1.shape[2] != self.n_hidden or self.w2.shape[3] != self.n_hidden:
            raise ValueError('b1 / w2 disagree with w1 about H1')
        if self.b2.shape[2] != self.n_hidden2 or self.w3.shape[2] != self.n_hidden2:
            raise ValueError('b2 / w3 disagree with w2 about H2')
        self.n_sets = max(getattr(self, n).shape[0] for n in self._NAMES)
        self.sigma = None if sigma is None else np.asarray(sigma, dtype=np.float64)
        self.version = 0

    def invalidate(self) -> None:
        """Tell the caches that the weights changed (see `MLPPolicy`'s docstring)."""
        self.version += 1

    def update(self, w1=None, b1=None, w2=None, b2=None, w3=None, b3=None, sigma=None) -> None:
        """Replace some of the weight arrays (same shapes) and / or sigma, and bump `version`: the learner's step between two rollouts."""
        for name, v in zip(self._NAMES, (w1, b1, w2, b2, w3, b3)):
            if v is not None:
                v = np.asarray(v, dtype=np.float64)
                if v.shape != getattr(self, name).shape:
                    raise ValueError(f'{name}: shape {v.shape} != {getattr(self, name).shape}')
                setattr(self, name, v)
        if sigma is not None:
            self.sigma = np.asarray(sigma, dtype=np.float64)
        self.invalidate()

    def _full(self, n_bldg: int):
        S, H1, H2 = self.n_sets, self.n_hidden, self.n_hidden2
        shapes = ((S, n_bldg, H1, self.n_obs), (S, n_bldg, H1), (S, n_bldg, H2, H1), (S, n_bldg, H2), (S, n_bldg, H2), (S, n_bldg))
        try:
            return tuple(np.broadcast_to(getattr(self, n), sh) for n, sh in zip(self._NAMES, shapes))
        except ValueError as e:
            raise ValueError(f'the weights do not broadcast to {S} sets x {n_bldg} buildings: {e}') from None

    # ---- the reference: the UNSPLIT MLP in float64 ------------------------------------------------------------------------------
    def actions_host(self, obs_vectors, noise=None, tables: Optional[DeepPolicyTables] = None, low=None, high=None, sigma_bldg=None,
                     set_index: int = 0) -> np.ndarray:
        """float64 numpy evaluation of the plain MLP: ``obs_vectors [..., n_bldg, n_obs]`` -> actions ``[..., n_bldg]``; the arguments are
        `MLPPolicy.actions_host`'s."""
        pick = lambda arg, attr, default: np.asarray(arg if arg is not None else getattr(tables, attr) if tables is not None else default, dtype=np.float64)
        x = np.asarray(obs_vectors, dtype=np.float64)
        w1, b1, w2, b2, w3, b3 = (v[set_index] for v in self._full(x.shape[-2]))
        h1 = np.tanh(np.einsum('bjc,...bc->...bj', w1, x) + b1)
        h2 = np.tanh(np.einsum('bij,...bj->...bi', w2, h1) + b2)
        lo, hi = pick(low, 'low_bldg', -1.0), pick(high, 'high_bldg', 1.0)
        a = 0.5 * (hi + lo) + 0.5 * (hi - lo) * np.tanh(np.einsum('bi,...bi->...b', w3, h2) + b3)
        if noise is not None:
            if sigma_bldg is None and tables is None and self.sigma is not None and self.sigma.ndim:
                raise ValueError('a per-column sigma needs `tables` (or `sigma_bldg`): which column drives which building')
            a = a + pick(sigma_bldg, 'sigma_bldg', 0.0 if self.sigma is None or self.sigma.ndim else float(self.sigma)) * np.asarray(noise, dtype=np.float64)
        return np.clip(a, lo, hi)

    def torch_policy(self, layout: ObservationLayout, tab, device, dtype=torch.float32, set_index: int = 0):
        """The same MLP (no noise) written in torch over the env's observation TENSOR: a `VectorCityLearnEnv.capture_rollout` policy
        ``f(obs [n_envs, n_obs_total], i=None) -> actions [n_act_cols, n_envs]``, as `MLPPolicy.torch_policy`."""
        cols = building_columns(layout)
        w1, b1, w2, b2, w3, b3 = (torch.as_tensor(np.array(v[set_index]), dtype=dtype, device=device) for v in self._full(len(cols)))
        idx = torch.as_tensor(np.array([c + [c[0]] * (self.n_obs - len(c)) for c in cols]), device=device)
        mask = torch.as_tensor(np.array([[1.0] * len(c) + [0.0] * (self.n_obs - len(c)) for c in cols]), dtype=dtype, device=device)
        hc = _head_columns(tab, self.kind)
        low, high = layout.spec.action_limits()
        sel = np.nonzero(hc >= 0)[0]                                             # the buildings that have a storage column
        rows, bsel = torch.as_tensor(hc[sel], device=device), torch.as_tensor(sel, device=device)
        lo = torch.as_tensor(np.asarray(low)[hc[sel]], dtype=dtype, device=device)
        hi = torch.as_tensor(np.asarray(high)[hc[sel]], dtype=dtype, device=device)
        n_act = len(low)

        def f(obs, i=None):
            x = obs.to(dtype)[:, idx] * mask                                     # [E, B, n_obs]
            h1 = torch.tanh(torch.einsum('bjc,ebc->ebj', w1, x) + b1)
            h2 = torch.tanh(torch.einsum('bij,ebj->ebi', w2, h1) + b2)
            o = torch.tanh((w3 * h2).sum(dim=-1) + b3)[:, bsel]                  # [E, driven buildings]
            a = torch.clamp(0.5 * (hi + lo) + 0.5 * (hi - lo) * o, lo, hi)
            out = torch.zeros((n_act, obs.shape[0]), dtype=torch.float32, device=obs.device)
            out[rows] = a.t().to(torch.float32)
            return out
        return f

    # ---- the kernel's tables ----------------------------------------------------------------------------------------------------
    def pack(self, layout: ObservationLayout, tab, device='cpu', set_of_block=None, matrix_cores=None) -> DeepPolicyTables:
        """The first layer split exactly as `MLPPolicy.pack` splits it (the same code and the same refusals: a one-hidden-layer policy over
        W1 / b1 is packed and its ``pre`` / ``dep`` / bounds / sigma taken), then ``l2`` and ``out`` as `DeepPolicyTables` describes them, in
        float64 rounded once.  ``matrix_cores``: the kernel family of layer 2 -- False: exact fp32 (`cl_rollout_policy_deep_kernel<1, PREC, 0>`);
        True: the f16 matrix cores with both operands split into two f16 terms (`<1, PREC, 1>`: the action moves by at most the split's
        3 x 2^-22 sum |W2| per layer-2 sum, see tests/policy_deep_util.py `split_bound`); None: `default_matrix_cores(H1, H2, n_bldg)`
        -- the faster family by the probe's logs that fits this district."""
        S, H1 = self.n_sets, self.n_hidden
        front = MLPPolicy(self.w1, self.b1, np.zeros((S, 1, H1)), np.zeros((1, 1)), sigma=self.sigma)
        ft = front.pack(layout, tab, device=device, set_of_block=set_of_block)
        if matrix_cores is None:
            matrix_cores = default_matrix_cores(self.n_hidden, self.n_hidden2, ft.n_bldg)
        _, _, w2, b2, w3, b3 = self._full(ft.n_bldg)
        dev = torch.device(device)
        f64 = lambda v: torch.from_numpy(np.array(v, dtype=np.float64)).to(dev)
        if matrix_cores:
            l2 = torch.from_numpy(_l2_fragments(np.array(w2) * ACT_SCALE, np.array(b2) * ACT_SCALE)).to(dev)
        else:
            l2 = (torch.cat([f64(w2).transpose(2, 3), f64(b2)[:, :, None, :]], dim=2) * ACT_SCALE).to(torch.float32)
        out = torch.cat([f64(w3), f64(b3)[..., None]], dim=-1)
        return DeepPolicyTables(ft.pre, ft.dep, l2.contiguous(), out.to(torch.float32).contiguous(), ft.net_reset, ft.act_low, ft.act_high,
                                ft.sigma, ft.set_of_block, ft.cols, ft.low_bldg, ft.high_bldg, ft.sigma_bldg, self.version, matrix_cores=matrix_cores)


def default_thermal_matrix_cores(n_hidden: int, n_hidden2: int, n_bldg: Optional[int] = None) -> bool:
    """What `DeepStorageMLPPolicy.pack(matrix_cores=None)` resolves to: the matrix-core family exactly where profiles/policy_full_deep_probe.log
    shows it faster than the exact-fp32 one by more than the spread (max - min) of its own seven repetitions in EVERY measured case of that shape,
    the exact-fp32 family -- the arithmetic reference -- everywhere else.  `default_matrix_cores`'s rule (H1 * H2 >= 512) is NOT inherited: that
    one was measured on another kernel (two buildings per wave, two inputs, one head, the lean unit).  Both families fit a CU's LDS at every
    accepted geometry (`_lib.policy_full_deep_lds_bytes`: 104 448 bytes at sixteen buildings), so ``n_bldg`` does not enter.

    The rule: ``H1 * H2 >= 512``.  The matrix-core kernel always computes the zero-padded 32 x 32 problem and costs the same at every size --
    16.6 - 17.0 us per step at 9 x 32 768 with the record under the float64 chain -- while the exact-fp32 kernel's cost follows H1 * H2: 9.21 us
    at (8, 8), 13.60 at (16, 16), 15.49 / 15.79 at (16, 24) / (24, 16), 15.73 at (20, 20), 16.00 / 17.11 at (16, 28) / (28, 16), 16.80 / 17.18 at
    (20, 24) / (24, 20), 17.16 / 18.53 at (16, 32) / (32, 16), 18.45 at (24, 24), 24.71 at (32, 32).  The four measured shapes with
    H1 * H2 >= 512 -- (16, 32), (32, 16), (24, 24), (32, 32) -- read "matrix_cores_faster_beyond_its_spread: 8 of 8 cases" (two batch sizes x two
    precision models x record off / on; profiles/policy_full_deep_probe.log, which also has (8, 8) and (16, 16): "0 of 8").  Below 512 no shape
    reads 8 of 8: (16, 24), (24, 16), (20, 20), (16, 28) "0 of 8", (20, 24) "1 of 8", (28, 16) and (24, 20) "3 of 8"
    (profiles/policy_full_deep_probe_shapes.log) -- near 450 the two families cost the same within their spreads, and the exact one stays.  No
    admissible product lies between 480 and 512."""
    return n_hidden * n_hidden2 >= 512


class DeepStorageMLPPolicy:
    """`StorageMLPPolicy` with TWO hidden layers -- the shape of the SAC / PPO actors of the CityLearn examples -- per building and head a, the heads
    in the fixed order electrical, cooling, heating, DHW storage (`HEAD_NAMES`):

        h1 = tanh(W1 obs + b1),   h2 = tanh(W2 h1 + b2),   act_a = clamp(mid_a + half_a tanh(w3[a] . h2 + b3[a]) + sigma_a z_a, low_a, high_a)

    `obs`, the five env-dependent inputs (the building's own four storage socs and ``net_electricity_consumption``), the heads' columns, bounds,
    sigma and the noise stream are `StorageMLPPolicy`'s; the heads of columns a building lacks are ignored.  Thermal districts without the LSTM
    stage and without device actions of up to 16 buildings: one launch of `cl_rollout_full_policy_deep_kernel` (csrc/cl_policy_full_deep.h,
    ``libcitylearn_amd_policy_full_deep.so``).

    ``w1 [n_sets, n_bldg, H1, n_obs]``, ``b1 [n_sets, n_bldg, H1]``, ``w2 [n_sets, n_bldg, H2, H1]``, ``b2 [n_sets, n_bldg, H2]``,
    ``w3 [n_sets, n_bldg, 4, H2]``, ``b3 [n_sets, n_bldg, 4]`` (anything array-like; kept in float64); a leading dimension of 1 broadcasts.
    ``H1``, ``H2``: 4, 8, .. 32, independent of each other.  ``sigma``: None (deterministic), a scalar or ``[n_act_cols]``.

    The packed tables are a snapshot, as `MLPPolicy`'s: change the weights through :meth:`update` / :meth:`invalidate`, which bump `version`."""
    kind = _DEEP_THERMAL
    _NAMES = DeepMLPPolicy._NAMES

    def __init__(self, w1, b1, w2, b2, w3, b3, sigma=None):
        self.w1, self.b1, self.w2, self.b2, self.w3, self.b3 = (np.asarray(x, dtype=np.float64) for x in (w1, b1, w2, b2, w3, b3))
        if [getattr(self, n).ndim for n in self._NAMES] != [4, 3, 4, 3, 4, 3]:
            raise ValueError('w1 [n_sets, n_bldg, H1, n_obs], b1 [n_sets, n_bldg, H1], w2 [n_sets, n_bldg, H2, H1], b2 [n_sets, n_bldg, H2], '
                             f'w3 [n_sets, n_bldg, {CLPF_NA}, H2], b3 [n_sets, n_bldg, {CLPF_NA}]')
        self.n_hidden, self.n_obs, self.n_hidden2 = int(self.w1.shape[2]), int(self.w1.shape[3]), int(self.w2.shape[2])
        for name, h in (('H1', self.n_hidden), ('H2', self.n_hidden2)):
            if h % 4 or not 4 <= h <= CLPFD_MAX_HIDDEN:
                raise ValueError(f'{name}={h}: the deep thermal policy kernel takes 4, 8, .. {CLPFD_MAX_HIDDEN} units per hidden layer')
        if self.b1.shape[2] != self.n_hidden or self.w2.shape[3] != self.n_hidden:
            raise ValueError('b1 / w2 disagree with w1 about H1')
        if self.b2.shape[2] != self.n_hidden2 or self.w3.shape[2:] != (CLPF_NA, self.n_hidden2) or self.b3.shape[2:] != (CLPF_NA,):
            raise ValueError(f'b2 / w3 disagree with w2 about H2, or w3 / b3 do not have {CLPF_NA} heads')
        self.n_sets = max(getattr(self, n).shape[0] for n in self._NAMES)
        self.sigma = None if sigma is None else np.asarray(sigma, dtype=np.float64)
        self.version = 0

    invalidate = DeepMLPPolicy.invalidate
    update = DeepMLPPolicy.update

    def _full(self, n_bldg: int):
        S, H1, H2 = self.n_sets, self.n_hidden, self.n_hidden2
        shapes = ((S, n_bldg, H1, self.n_obs), (S, n_bldg, H1), (S, n_bldg, H2, H1), (S, n_bldg, H2), (S, n_bldg, CLPF_NA, H2), (S, n_bldg, CLPF_NA))
        try:
            return tuple(np.broadcast_to(getattr(self, n), sh) for n, sh in zip(self._NAMES, shapes))
        except ValueError as e:
            raise ValueError(f'the weights do not broadcast to {S} sets x {n_bldg} buildings: {e}') from None

    # ---- the reference: the UNSPLIT MLP in float64 ------------------------------------------------------------------------------
    def actions_host(self, obs_vectors, tables: DeepStoragePolicyTables, noise=None, set_index: int = 0) -> np.ndarray:
        """float64 numpy evaluation of the plain MLP: ``obs_vectors [..., n_bldg, n_obs]`` -> actions ``[..., n_bldg, 4]`` (0 for a head whose
        column the building lacks); the arguments are `StorageMLPPolicy.actions_host`'s."""
        x = np.asarray(obs_vectors, dtype=np.float64)
        w1, b1, w2, b2, w3, b3 = (v[set_index] for v in self._full(x.shape[-2]))
        h1 = np.tanh(np.einsum('bjc,...bc->...bj', w1, x) + b1)
        h2 = np.tanh(np.einsum('bij,...bj->...bi', w2, h1) + b2)
        lo, hi = tables.low_bldg, tables.high_bldg
        a = 0.5 * (hi + lo) + 0.5 * (hi - lo) * np.tanh(np.einsum('bai,...bi->...ba', w3, h2) + b3)
        if noise is not None:
            a = a + tables.sigma_bldg * np.asarray(noise, dtype=np.float64)
        return np.where(tables.cols >= 0, np.clip(a, lo, hi), 0.0)

    def torch_policy(self, layout: ObservationLayout, tab, device, dtype=torch.float32, set_index: int = 0):
        """The same MLP (no noise) written in torch over the env's observation TENSOR: a `VectorCityLearnEnv.capture_rollout` policy
        ``f(obs [n_envs, n_obs_total], i=None) -> actions [n_act_cols, n_envs]``, as `StorageMLPPolicy.torch_policy`."""
        cols = building_columns(layout)
        w1, b1, w2, b2, w3, b3 = (torch.as_tensor(np.array(v[set_index]), dtype=dtype, device=device) for v in self._full(len(cols)))
        idx = torch.as_tensor(np.array([c + [c[0]] * (self.n_obs - len(c)) for c in cols]), device=device)
        mask = torch.as_tensor(np.array([[1.0] * len(c) + [0.0] * (self.n_obs - len(c)) for c in cols]), dtype=dtype, device=device)
        hc = _head_columns(tab, self.kind)
        low, high = layout.spec.action_limits()
        sel = np.nonzero(hc >= 0)                                                # the heads that have a column
        rows = torch.as_tensor(hc[sel], device=device)
        lo = torch.as_tensor(np.asarray(low)[hc[sel]], dtype=dtype, device=device)
        hi = torch.as_tensor(np.asarray(high)[hc[sel]], dtype=dtype, device=device)
        flat = torch.as_tensor(np.ravel_multi_index(sel, hc.shape), device=device)
        n_act = len(low)

        def f(obs, i=None):
            x = obs.to(dtype)[:, idx] * mask                                     # [E, B, n_obs]
            h1 = torch.tanh(torch.einsum('bjc,ebc->ebj', w1, x) + b1)
            h2 = torch.tanh(torch.einsum('bij,ebj->ebi', w2, h1) + b2)
            o = torch.tanh(torch.einsum('bai,ebi->eba', w3, h2) + b3).reshape(obs.shape[0], -1)[:, flat]         # [E, present heads]
            a = torch.clamp(0.5 * (hi + lo) + 0.5 * (hi - lo) * o, lo, hi)
            out = torch.zeros((n_act, obs.shape[0]), dtype=torch.float32, device=obs.device)
            out[rows] = a.t().to(torch.float32)
            return out
        return f

    # ---- the kernel's tables ----------------------------------------------------------------------------------------------------
    def pack(self, layout: ObservationLayout, tab, device='cpu', set_of_block=None, matrix_cores=None) -> DeepStoragePolicyTables:
        """The first layer split exactly as `StorageMLPPolicy.pack` splits it (the same code and the same refusals, device-action columns
        included: a one-hidden-layer storage policy over W1 / b1 is packed and its ``pre`` / ``dep`` / bounds / sigma taken), then ``l2`` and
        ``out`` as `DeepStoragePolicyTables` describes them, in float64 rounded once -- layer 2 exactly as `DeepMLPPolicy.pack` hands it over.
        ``matrix_cores``: the kernel family of layer 2 -- False: exact fp32 (`cl_rollout_full_policy_deep_kernel<PREC, 0, MARL>`); True: the f16
        matrix cores with both operands split into two f16 terms (`<PREC, 1, MARL>`: every head's action moves by at most the split's bound,
        tests/policy_full_deep_util.py `split_bound`); None: `default_thermal_matrix_cores(H1, H2, n_bldg)`."""
        S, H1 = self.n_sets, self.n_hidden
        front = StorageMLPPolicy(self.w1, self.b1, np.zeros((S, 1, CLPF_NA, H1)), np.zeros((1, 1, CLPF_NA)), sigma=self.sigma)
        ft = front.pack(layout, tab, device=device, set_of_block=set_of_block)
        if matrix_cores is None:
            matrix_cores = default_thermal_matrix_cores(self.n_hidden, self.n_hidden2, ft.n_bldg)
        _, _, w2, b2, w3, b3 = self._full(ft.n_bldg)
        dev = torch.device(device)
        f64 = lambda v: torch.from_numpy(np.array(v, dtype=np.float64)).to(dev)
        if matrix_cores:
            l2 = torch.from_numpy(_l2_fragments(np.array(w2) * ACT_SCALE, np.array(b2) * ACT_SCALE)).to(dev)
        else:
            l2 = (torch.cat([f64(w2).transpose(2, 3), f64(b2)[:, :, None, :]], dim=2) * ACT_SCALE).to(torch.float32)
        out = torch.cat([f64(w3), f64(b3)[..., None]], dim=-1)
        return DeepStoragePolicyTables(ft.pre, ft.dep, l2.contiguous(), out.to(torch.float32).contiguous(), ft.net_reset, ft.act_low, ft.act_high,
                                       ft.sigma, ft.set_of_block, ft.cols, ft.low_bldg, ft.high_bldg, ft.sigma_bldg, self.version,
                                       matrix_cores=matrix_cores)


class _CentralBase:
    """What the four central-agent policies share: everything but the class's `kind`, its number of hidden layers (`_NAMES`: the weight arrays
    in order, the head's last), the texts of its constructor's refusals and the signature of `actions_host` on a thermal district.  The heads
    are ``[n_bldg]`` or ``[n_bldg, 4]`` by `kind.head_shape`; a thermal kind (`kind.refuse_device_actions`) packs its first layer through
    `_pack_thermal_front`."""
    kind: _Kind
    _NAMES = ('w1', 'b1', 'w2', 'b2')
    _WIDTHS = ('H',)                                         # the hidden layers as the refusals name them
    _SHAPES_MSG: str                                         # the refusal of arrays of the wrong rank
    _WIDTH_MSG: str                                          # ... of a hidden width ({name}, {h}, {max})
    _MISMATCH: tuple                                         # ... of arrays that disagree: ((names, message), ..) in the order they are checked

    def __init__(self, w1, b1, w2, b2, sigma=None):
        self._setup((w1, b1, w2, b2), sigma)

    def _setup(self, arrays, sigma) -> None:
        for n, x in zip(self._NAMES, arrays):
            setattr(self, n, np.asarray(x, dtype=np.float64))
        hs, deep = self.kind.head_shape, len(self._WIDTHS) > 1
        if [getattr(self, n).ndim for n in self._NAMES] != [3, 2] * len(self._WIDTHS) + [2 + len(hs) + 1, 2 + len(hs)]:
            raise ValueError(self._SHAPES_MSG)
        self.n_hidden, self.n_obs, self.n_bldg = int(self.w1.shape[1]), int(self.w1.shape[2]), int(getattr(self, self._NAMES[-2]).shape[1])
        if deep:
            self.n_hidden2 = int(self.w2.shape[1])
        for name, h in zip(self._WIDTHS, self._hidden):
            if h % 4 or not 4 <= h <= self.kind.max_hidden:
                raise ValueError(self._WIDTH_MSG.format(name=name, h=h, max=self.kind.max_hidden))
        want = dict(zip(self._NAMES, self._shapes(None)))
        for names, msg in self._MISMATCH:
            if any(getattr(self, n).shape[1:] != want[n][1:] for n in names):
                raise ValueError(msg)
        self.n_sets = max(getattr(self, n).shape[0] for n in self._NAMES)
        self.sigma = None if sigma is None else np.asarray(sigma, dtype=np.float64)
        self.version = 0

    @property
    def _hidden(self) -> tuple:
        return (self.n_hidden, self.n_hidden2) if len(self._WIDTHS) > 1 else (self.n_hidden,)

    def _shapes(self, S) -> list:
        """The shape of every array of `_NAMES` at ``S`` parameter sets."""
        hs, widths = self.kind.head_shape, (self.n_obs,) + self._hidden
        layers = [sh for i, o in zip(widths, widths[1:]) for sh in ((S, o, i), (S, o))]
        return layers + [(S, self.n_bldg) + hs + widths[-1:], (S, self.n_bldg) + hs]

    def invalidate(self) -> None:
        """Tell the caches that the weights changed (see `MLPPolicy`'s docstring)."""
        self.version += 1

    def update(self, w1=None, b1=None, w2=None, b2=None, sigma=None) -> None:
        """Replace some of the weight arrays (same shapes) and / or sigma, and bump `version`: the learner's step between two rollouts."""
        self._replace((w1, b1, w2, b2), sigma)

    def _replace(self, arrays, sigma) -> None:
        for name, v in zip(self._NAMES, arrays):
            if v is not None:
                v = np.asarray(v, dtype=np.float64)
                if v.shape != getattr(self, name).shape:
                    raise ValueError(f'{name}: shape {v.shape} != {getattr(self, name).shape}')
                setattr(self, name, v)
        if sigma is not None:
            self.sigma = np.asarray(sigma, dtype=np.float64)
        self.invalidate()

    def _full(self, n_bldg: Optional[int] = None):
        if n_bldg is not None and n_bldg != self.n_bldg:
            raise ValueError(f'{self._NAMES[-2]} has heads for {self.n_bldg} buildings, the district has {n_bldg}')
        try:
            return tuple(np.broadcast_to(getattr(self, n), sh) for n, sh in zip(self._NAMES, self._shapes(self.n_sets)))
        except ValueError as e:
            raise ValueError(f'the weights do not broadcast to {self.n_sets} sets: {e}') from None

    # ---- the reference: the UNSPLIT MLP in float64 ------------------------------------------------------------------------------
    def _actions(self, obs, set_index, lo, hi, sigma, noise) -> np.ndarray:
        """The hidden stack, the heads, the noise and the clamp in float64; ``lo``, ``hi``, ``sigma`` per head."""
        *hidden, wo, bo = (v[set_index] for v in self._full())
        h = np.asarray(obs, dtype=np.float64)
        for w, b in zip(hidden[::2], hidden[1::2]):
            h = np.tanh(np.einsum('ij,...j->...i', w, h) + b)
        a = 0.5 * (hi + lo) + 0.5 * (hi - lo) * np.tanh(np.einsum('baj,...j->...ba' if self.kind.head_shape else 'bj,...j->...b', wo, h) + bo)
        if noise is not None:
            a = a + sigma * np.asarray(noise, dtype=np.float64)
        return np.clip(a, lo, hi)

    def actions_host(self, obs, noise=None, tables: Optional[CentralPolicyTables] = None, low=None, high=None, sigma_bldg=None,
                     set_index: int = 0) -> np.ndarray:
        """float64 numpy evaluation of the plain MLP: ``obs [..., n_cols]`` (the central-agent vector) -> actions ``[..., n_bldg]``; the other
        arguments are `MLPPolicy.actions_host`'s."""
        pick = lambda arg, attr, default: np.asarray(arg if arg is not None else getattr(tables, attr) if tables is not None else default, dtype=np.float64)
        sigma = None
        if noise is not None:
            if sigma_bldg is None and tables is None and self.sigma is not None and self.sigma.ndim:
                raise ValueError('a per-column sigma needs `tables` (or `sigma_bldg`): which column drives which building')
            sigma = pick(sigma_bldg, 'sigma_bldg', 0.0 if self.sigma is None or self.sigma.ndim else float(self.sigma))
        return self._actions(obs, set_index, pick(low, 'low_bldg', -1.0), pick(high, 'high_bldg', 1.0), sigma, noise)

    def _actions_thermal(self, obs, tables, noise, set_index) -> np.ndarray:
        """`actions_host` of a thermal kind: the heads' columns, bounds and sigmas from ``tables``; 0 for a head whose column the building lacks."""
        return np.where(tables.cols >= 0, self._actions(obs, set_index, tables.low_bldg, tables.high_bldg, tables.sigma_bldg, noise), 0.0)

    def torch_policy(self, layout: ObservationLayout, tab, device, dtype=torch.float32, set_index: int = 0):
        """The same MLP (no noise) written in torch over the env's observation TENSOR of a ``central_agent=True`` env: a
        `VectorCityLearnEnv.capture_rollout` policy ``f(obs [n_envs, n_cols], i=None) -> actions [n_act_cols, n_envs]``."""
        self._check_layout(layout)
        *hidden, wo, bo = (torch.as_tensor(np.array(v[set_index]), dtype=dtype, device=device) for v in self._full(len(layout.building_names)))
        layers = tuple(zip(hidden[::2], hidden[1::2]))
        hc = _head_columns(tab, self.kind)
        low, high = layout.spec.action_limits()
        sel = np.nonzero(hc >= 0)                                                # the heads that have a column
        rows = torch.as_tensor(hc[sel], device=device)
        lo = torch.as_tensor(np.asarray(low)[hc[sel]], dtype=dtype, device=device)
        hi = torch.as_tensor(np.asarray(high)[hc[sel]], dtype=dtype, device=device)
        flat = torch.as_tensor(np.ravel_multi_index(sel, hc.shape), device=device)
        wf, bf = wo.reshape(-1, wo.shape[-1])[flat], bo.reshape(-1)[flat]       # [present heads, H], [present heads]
        n_act = len(low)

        def f(obs, i=None):
            h = obs.to(dtype)
            for w, b in layers:
                h = torch.tanh(h @ w.t() + b)                                    # [E, H1], [E, H2]
            o = torch.tanh(h @ wf.t() + bf)                                      # [E, present heads]
            a = torch.clamp(0.5 * (hi + lo) + 0.5 * (hi - lo) * o, lo, hi)
            out = torch.zeros((n_act, obs.shape[0]), dtype=torch.float32, device=obs.device)
            out[rows] = a.t().to(torch.float32)
            return out
        return f

    def _check_layout(self, layout: ObservationLayout) -> None:
        if not layout.central_agent:
            raise ValueError(f'a {type(self).__name__} is defined over the central-agent observation vector: the layout was built with central_agent=False '
                             '(per-building vectors side by side, shared observations repeated)')
        if layout.n_cols != self.n_obs:
            raise ValueError(f'w1 takes {self.n_obs} observations, the central-agent vector has {layout.n_cols}')

    # ---- the kernel's tables ----------------------------------------------------------------------------------------------------
    def pack(self, layout: ObservationLayout, tab, device='cpu', set_of_block=None) -> CentralPolicyTables:
        """Split the first layer as `MLPPolicy.pack` splits it, over the central-agent vector of `layout` (built with ``central_agent=True``)
        and the kind's terms: the env-independent columns of every table row go into ``pre [n_sets, n_rows, H1]`` (one matmul in float64 on
        `device`, rounded once) -- no building axis --, ``W1[j][c] * col_scale[c]`` of the env-dependent columns (every building's own storage
        soc(s) and ``net_electricity_consumption``) into ``dep`` in the kernel's order (the rows of a storage the building lacks stay 0), their
        table offsets into ``pre``; ``ACT_SCALE`` is folded into both.  Then ``l2`` (two hidden layers) and ``out`` as the kind's tables class
        describes them, in float64 rounded once.  Refused: a column fed by any other device plane (`MLPPolicy.pack`'s ``ValueError``; on a
        thermal district `StorageMLPPolicy.pack`'s messages, the LSTM stage's indoor temperature among them), a reset value its table row does
        not hold, on a thermal district a building with a cooling / heating device ACTION column, a layout built with ``central_agent=False``, a
        vector of another length."""
        self._check_layout(layout)
        w1, b1, *middle, wo, bo = self._full(len(layout.building_names))
        front = self._pack_thermal_front if self.kind.refuse_device_actions else self._pack_front
        pre, dep, rest = front(layout, tab, w1, b1, device, set_of_block)
        f64 = lambda v: torch.from_numpy(np.array(v, dtype=np.float64)).to(pre.device)
        l2 = [(torch.cat([f64(w).transpose(1, 2), f64(b)[:, None, :]], dim=1) * ACT_SCALE).to(torch.float32).contiguous()
              for w, b in zip(middle[::2], middle[1::2])]
        out = torch.cat([f64(wo), f64(bo)[..., None]], dim=-1)
        return self.kind.tables(pre, dep, *l2, out.to(torch.float32).contiguous(), *rest, self.version)

    def _pack_front(self, layout: ObservationLayout, tab, w1, b1, device, set_of_block):
        """The first layer ``w1 [n_sets, H, n_cols]``, ``b1 [n_sets, H]`` (broadcast) split over the central-agent vector as `pack` describes it:
        ``(pre, dep, rest)`` with ``rest`` the tables' members behind ``out`` -- ``net_reset``, the bounds, sigma, ``set_of_block`` on `device`, the
        host side."""
        kind = self.kind
        obs = layout.episode(tab, reset_table=True)
        n_bldg, T, N = len(layout.building_names), int(obs.table.shape[0]), layout.n_cols
        params_i = np.ascontiguousarray(tab.params).view(np.int32)
        term_of = {src: k for k, (src, _) in enumerate(kind.terms)}
        table = obs.table
        x = np.zeros((T, N))
        scale = np.zeros((n_bldg, len(kind.terms), N))                   # [b][term][column of the central vector]
        net_reset = np.zeros((T, n_bldg))
        for c, (i, cname) in enumerate(layout.columns):
            name = f'{cname!r} of building {i} (column {c})'
            src = int(obs.col_src[c])
            if src < 0:
                if T > 1 and not np.array_equal(obs.reset_table[1:, c], table[1:, c]):
                    raise ValueError(f'observation {name} is reset to a value its table row does not hold (observation_mode="reference"?): '
                                     'the policy kernel reads the tables of observation_mode="current"')
                x[:, c] = table[:, c]
                continue
            kind_, plane, b = src >> 28, (src >> 20) & 0xFF, src & 0xFFFFF
            which = term_of.get((kind_, plane))
            if which is None or b != i:
                raise ValueError(f'observation {name} is fed by device plane (kind {kind_}, plane {plane}, building {b}): {kind.only}'
                                 + (' -- the indoor temperature comes from the LSTM stage' if kind_ == SRC_TEMP else ''))
            offset = table[1:, c] if T > 1 else np.zeros(1)
            if np.ptp(offset) != 0.0:
                raise ValueError(f'observation {name}: a table offset that changes with the row')
            x[:, c] = offset[0]
            scale[i, which, c] = float(obs.col_scale[c])
            if kind.terms[which][0] == (SRC_OUT, abi.CLO_NET) and scale[i, which, c] != 0.0:
                net_reset[:, i] = (obs.reset_table[:, c] - offset[0]) / scale[i, which, c]
        dev = torch.device(device)
        f64 = lambda v: torch.from_numpy(np.array(v, dtype=np.float64)).to(dev)
        S, H = self.n_sets, self.n_hidden
        pre = (torch.einsum('sjc,tc->stj', f64(w1), f64(x)) + f64(b1)[:, None]) * ACT_SCALE
        dep = torch.einsum('sjc,bkc->sjbk', f64(w1), f64(scale)) * ACT_SCALE                          # [S, H, B, 2]
        dep = dep.reshape(S, H // 4, 4, n_bldg, len(kind.terms)).permute(0, 1, 3, 4, 2)              # [S, H / 4, B, 2, 4]
        hc = _head_columns(tab, kind)
        n_act = int(params_i[:, abi.CLP_ACT_COOL_STO:abi.CLP_ACT_COH_DEV + 1].max()) + 1
        low, high = layout.spec.action_limits()
        if len(low) != n_act:
            raise ValueError(f'{len(low)} action limits for {n_act} action columns')
        at = lambda v, fill: np.where(hc >= 0, np.asarray(v, dtype=np.float64)[np.maximum(hc, 0)], fill)
        sigma = None
        if self.sigma is not None:
            sigma = np.full(n_act, float(self.sigma)) if self.sigma.ndim == 0 else self.sigma
            if sigma.shape != (n_act,) or np.any(sigma < 0):
                raise ValueError(f'sigma: a non-negative scalar or [{n_act}] (one per action column)')
        f32 = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev)
        sob = None
        if set_of_block is not None:
            sob = np.asarray(set_of_block, dtype=np.int64).reshape(-1)
            if sob.min() < 0 or sob.max() >= self.n_sets:
                raise ValueError(f'set_of_block outside [0, {self.n_sets})')
            sob = torch.from_numpy(sob.astype(np.int32)).to(dev)
        return (pre.to(torch.float32).contiguous(), dep.to(torch.float32).contiguous(),
                (f32(net_reset), f32(low), f32(high), f32(sigma), sob, hc, at(low, -1.0), at(high, 1.0),
                 np.zeros(hc.shape) if sigma is None else at(sigma, 0.0)))

    def _pack_thermal_front(self, layout: ObservationLayout, tab, w1, b1, device, set_of_block):
        """`_pack_front` over the thermal kind's five terms, with what a thermal district adds: the refusal of device ACTION columns, and zero
        weights for the terms of a storage a building lacks."""
        kind = self.kind
        pre, dep, rest = self._pack_front(layout, tab, w1, b1, device, set_of_block)
        params_i = np.ascontiguousarray(tab.params).view(np.int32)
        bflags = np.ascontiguousarray(tab.params).view(np.uint32)[:, abi.CLP_FLAGS]
        for i in range(len(layout.building_names)):
            for dname, slot in _DEVICE_SLOTS:
                if params_i[i, slot] >= 0:
                    raise ValueError(f'action {dname!r} of building {i} (column {int(params_i[i, slot])}): the thermal policy kernel has storage heads '
                                     f'only {HEAD_NAMES}; a district with device actions runs through capture_rollout')
        # a storage the building lacks: its plane stays 0 in the kernel, its weights are 0 here
        has = np.array([[flag is None or bool(int(bflags[i]) & flag) for _, flag in kind.terms] for i in range(len(layout.building_names))])
        dep = dep * torch.from_numpy(has.astype(np.float32)).to(dep.device)[None, None, :, :, None]
        return pre, dep.contiguous(), rest


class _DeepCentralBase(_CentralBase):
    """`_CentralBase` at two hidden layers."""
    _NAMES = ('w1', 'b1', 'w2', 'b2', 'w3', 'b3')
    _WIDTHS = ('H1', 'H2')

    def __init__(self, w1, b1, w2, b2, w3, b3, sigma=None):
        self._setup((w1, b1, w2, b2, w3, b3), sigma)

    def update(self, w1=None, b1=None, w2=None, b2=None, w3=None, b3=None, sigma=None) -> None:
        """Replace some of the weight arrays (same shapes) and / or sigma, and bump `version`: the learner's step between two rollouts."""
        self._replace((w1, b1, w2, b2, w3, b3), sigma)


class CentralMLPPolicy(_CentralBase):
    """CityLearn's ``central_agent=True`` actor: ONE tanh MLP with one hidden layer over the district's observation vector returns every
    building's electrical-storage action,

        h = tanh(W1 obs + b1),   a_b = clamp(mid_b + half_b tanh(w2[b] . h + b2[b]) + sigma_b z, low_b, high_b)

    `obs` = the central-agent observation vector as the env defines it (``ObservationLayout(..., central_agent=True).columns``: a shared
    observation once, normalised or not, whatever the env was built with); the bounds, sigma, z and the noise stream are `MLPPolicy`'s.  The
    env-dependent inputs are EVERY building's own ``electrical_storage_soc`` and ``net_electricity_consumption``; a building without a storage
    action column feeds the hidden layer like any other and has no head.  Battery + PV districts of up to 32 buildings: one launch of
    `cl_rollout_policy_central_kernel` (csrc/cl_policy_central.h, ``libcitylearn_amd_policy_central.so``).

    ``w1 [n_sets, H, n_cols]``, ``b1 [n_sets, H]``, ``w2 [n_sets, n_bldg, H]``, ``b2 [n_sets, n_bldg]`` (anything array-like; kept in float64); a
    leading dimension of 1 broadcasts.  ``H``: 4, 8, .. 64.  ``sigma``: None (deterministic), a scalar or ``[n_act_cols]``.

    The packed tables are a snapshot, as `MLPPolicy`'s: change the weights through :meth:`update` / :meth:`invalidate`, which bump `version`."""
    kind = _CENTRAL
    _SHAPES_MSG = 'w1 [n_sets, H, n_cols], b1 [n_sets, H], w2 [n_sets, n_bldg, H], b2 [n_sets, n_bldg]'
    _WIDTH_MSG = '{name}={h}: the central policy kernel takes 4, 8, .. {max} hidden units'
    _MISMATCH = ((('b1', 'w2', 'b2'), 'b1 / w2 disagree with w1 about H, or b2 with w2 about n_bldg'),)


class DeepCentralMLPPolicy(_DeepCentralBase):
    """`CentralMLPPolicy` with TWO hidden layers -- a SAC / PPO actor trained with ``central_agent=True``:

        h1 = tanh(W1 obs + b1),   h2 = tanh(W2 h1 + b2),   a_b = clamp(mid_b + half_b tanh(w3[b] . h2 + b3[b]) + sigma_b z, low_b, high_b)

    `obs`, the bounds, sigma, z, the noise stream and the env-dependent inputs (EVERY building's own ``electrical_storage_soc`` and
    ``net_electricity_consumption``) are `CentralMLPPolicy`'s.  Battery + PV districts of up to 32 buildings: one launch of
    `cl_rollout_policy_central_deep_kernel` (csrc/cl_policy_central.h at DEEP = true, ``libcitylearn_amd_policy_central_deep.so``), layer 2 in exact fp32.

    ``w1 [n_sets, H1, n_cols]``, ``b1 [n_sets, H1]``, ``w2 [n_sets, H2, H1]``, ``b2 [n_sets, H2]``, ``w3 [n_sets, n_bldg, H2]``,
    ``b3 [n_sets, n_bldg]`` (anything array-like; kept in float64); a leading dimension of 1 broadcasts.  ``H1``, ``H2``: 4, 8, .. 64, independent of
    each other.  ``sigma``: None (deterministic), a scalar or ``[n_act_cols]``.

    The packed tables are a snapshot, as `MLPPolicy`'s: change the weights through :meth:`update` / :meth:`invalidate`, which bump `version`."""
    kind = _CENTRAL_DEEP
    _SHAPES_MSG = 'w1 [n_sets, H1, n_cols], b1 [n_sets, H1], w2 [n_sets, H2, H1], b2 [n_sets, H2], w3 [n_sets, n_bldg, H2], b3 [n_sets, n_bldg]'
    _WIDTH_MSG = '{name}={h}: the deep central policy kernel takes 4, 8, .. {max} units per hidden layer'
    _MISMATCH = ((('b1', 'w2'), 'b1 / w2 disagree with w1 about H1'),
                 (('b2', 'w3', 'b3'), 'b2 / w3 disagree with w2 about H2, or b3 with w3 about n_bldg'))


class CentralStorageMLPPolicy(_CentralBase):
    """CityLearn's ``central_agent=True`` actor on a THERMAL district: ONE tanh MLP with one hidden layer over the district's observation vector
    returns every building's storage actions, up to four heads per building in the fixed order electrical, cooling, heating, DHW storage
    (`HEAD_NAMES`, `CLPF_A_*`),

        h = tanh(W1 obs + b1),   act[b][a] = clamp(mid + half tanh(w2[b][a] . h + b2[b][a]) + sigma z, low, high)

    for every head whose building has that action column (the others are ignored).  `obs` = the central-agent observation vector as the env
    defines it (``ObservationLayout(..., central_agent=True).columns``); the bounds, sigma, z and the noise stream -- Philox keyed by the head's
    action column -- are `StorageMLPPolicy`'s.  The env-dependent inputs are EVERY building's own ``electrical_storage_soc`` /
    ``cooling_storage_soc`` / ``heating_storage_soc`` / ``dhw_storage_soc`` and ``net_electricity_consumption``.  Thermal districts without the LSTM
    stage and without device actions (the 2020 / 2021 schemas) of up to 16 buildings: one launch of `cl_rollout_full_policy_central_kernel`
    (csrc/cl_policy_full_central.h, ``libcitylearn_amd_policy_full_central.so``).

    ``w1 [n_sets, H, n_cols]``, ``b1 [n_sets, H]``, ``w2 [n_sets, n_bldg, 4, H]``, ``b2 [n_sets, n_bldg, 4]`` (anything array-like; kept in
    float64); a leading dimension of 1 broadcasts.  ``H``: 4, 8, .. 64.  ``sigma``: None (deterministic), a scalar or ``[n_act_cols]``.

    The packed tables are a snapshot, as `MLPPolicy`'s: change the weights through :meth:`update` / :meth:`invalidate`, which bump `version`."""
    kind = _CENTRAL_THERMAL
    _SHAPES_MSG = f'w1 [n_sets, H, n_cols], b1 [n_sets, H], w2 [n_sets, n_bldg, {CLPF_NA}, H], b2 [n_sets, n_bldg, {CLPF_NA}]'
    _WIDTH_MSG = '{name}={h}: the central thermal policy kernel takes 4, 8, .. {max} hidden units'
    _MISMATCH = ((('b1', 'w2', 'b2'), f'b1 / w2 disagree with w1 about H, b2 with w2 about n_bldg, or w2 / b2 do not have {CLPF_NA} heads'),)

    def actions_host(self, obs, tables: CentralStoragePolicyTables, noise=None, set_index: int = 0) -> np.ndarray:
        """float64 numpy evaluation of the plain MLP: ``obs [..., n_cols]`` (the central-agent vector) -> actions ``[..., n_bldg, 4]`` (0 for a
        head whose column the building lacks).  ``noise``: the standard normals z (same shape as the result; `noise_host` replays the kernel's),
        scaled by each head's sigma.  The heads' columns, bounds and sigmas come from ``tables`` (a `pack` result)."""
        return self._actions_thermal(obs, tables, noise, set_index)


class DeepCentralStorageMLPPolicy(_DeepCentralBase):
    """`CentralStorageMLPPolicy` with TWO hidden layers -- a SAC / PPO actor trained with ``central_agent=True`` on a THERMAL district:

        h1 = tanh(W1 obs + b1),   h2 = tanh(W2 h1 + b2),   act[b][a] = clamp(mid + half tanh(w3[b][a] . h2 + b3[b][a]) + sigma z, low, high)

    for every head (`HEAD_NAMES`, `CLPF_A_*` order) whose building has that action column.  `obs`, the bounds, sigma, z, the noise stream -- Philox
    keyed by the head's action column -- and the env-dependent inputs (EVERY building's own storage socs and ``net_electricity_consumption``) are
    `CentralStorageMLPPolicy`'s.  Thermal districts without the LSTM stage and without device actions (the 2020 / 2021 schemas) of up to 16
    buildings: one launch of `cl_rollout_full_policy_central_deep_kernel` (csrc/cl_policy_full_central.h at DEEP = true,
    ``libcitylearn_amd_policy_full_central_deep.so``), layer 2 in exact fp32.

    ``w1 [n_sets, H1, n_cols]``, ``b1 [n_sets, H1]``, ``w2 [n_sets, H2, H1]``, ``b2 [n_sets, H2]``, ``w3 [n_sets, n_bldg, 4, H2]``,
    ``b3 [n_sets, n_bldg, 4]`` (anything array-like; kept in float64); a leading dimension of 1 broadcasts.  ``H1``, ``H2``: 4, 8, .. 64, independent
    of each other.  ``sigma``: None (deterministic), a scalar or ``[n_act_cols]``.

    The packed tables are a snapshot, as `MLPPolicy`'s: change the weights through :meth:`update` / :meth:`invalidate`, which bump `version`."""
    kind = _CENTRAL_DEEP_THERMAL
    _SHAPES_MSG = (f'w1 [n_sets, H1, n_cols], b1 [n_sets, H1], w2 [n_sets, H2, H1], b2 [n_sets, H2], w3 [n_sets, n_bldg, {CLPF_NA}, H2], '
                   f'b3 [n_sets, n_bldg, {CLPF_NA}]')
    _WIDTH_MSG = '{name}={h}: the deep central thermal policy kernel takes 4, 8, .. {max} units per hidden layer'
    _MISMATCH = ((('b1', 'w2'), 'b1 / w2 disagree with w1 about H1'),
                 (('b2', 'w3', 'b3'), f'b2 / w3 disagree with w2 about H2, b3 with w3 about n_bldg, or w3 / b3 do not have {CLPF_NA} heads'))

    def actions_host(self, obs, tables: DeepCentralStoragePolicyTables, noise=None, set_index: int = 0) -> np.ndarray:
        """float64 numpy evaluation of the plain MLP: ``obs [..., n_cols]`` (the central-agent vector) -> actions ``[..., n_bldg, 4]`` (0 for a
        head whose column the building lacks); the other arguments are `CentralStorageMLPPolicy.actions_host`'s."""
        return self._actions_thermal(obs, tables, noise, set_index)
