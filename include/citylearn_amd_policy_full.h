/* citylearn_amd_policy_full.h -- C interface of libcitylearn_amd_policy_full.so: the fused K-step rollout of a THERMAL district (cooling / heating /
 * DHW storage beside the battery: the 2020 / 2021 schemas) driven by a CLOSED-LOOP policy, a one-hidden-layer tanh MLP per building with up to
 * four storage heads, evaluated inside the rollout kernel (csrc/cl_policy_full.h).
 *
 * A library of its own beside libcitylearn_amd.so and the two battery + PV policy libraries (whose symbol lists, structs and kernels it leaves
 * untouched); it shares cl_dims / cl_tuning, the parameter / time-series / state / output plane layouts and the error codes with citylearn_amd.h.
 * Every name it exports starts with `clpf_`.  It holds no mutable state besides the thread-local error string.
 *
 * Per (env, building) and step t of the episode (table row r = env_row0[block] + t, parameter set s = set_of_block[block]):
 *     x     = (soc, cs, hs, ds, net_prev): the unit's electrical / cooling / heating / DHW storage soc before the step and its net electricity
 *             consumption of the previous step -- at t == 0: net_reset[r][b] (what the reset observation shows; NULL = 0); at the first step of a
 *             later launch: out_bldg[CLO_NET], what the previous launch left
 *     h_j   = tanh(pre[s][r][b][j] + sum_d dep[s][b][d][j] x_d)                                        j < n_hidden, d < CLPF_ND
 *     mean_a = mid[col_a] + half[col_a] tanh(out[s][b][a][n_hidden] + sum_j out[s][b][a][j] h_j)      a < CLPF_NA, mid / half from act_low / act_high
 *     act_a = clamp(mean_a + sigma[col_a] z_a, act_low[col_a], act_high[col_a])
 * with head a = CLPF_A_ES / _CS / _HS / _DS driving the building's electrical / cooling / heating / DHW STORAGE action column col_a; a head whose
 * column the building lacks is not evaluated (its rows of `out` are not read), and a term d whose storage the building lacks is skipped (its row
 * of `dep` must be 0).  z_a is a standard normal by Box-Muller from two draws of the main library's Philox stream, replayable on the host:
 *     u1 = cl_philox_uniform(seed ^ CLPF_NOISE_KEY, env_offset + env, col_a, 2 t),   u2 = cl_philox_uniform(.., 2 t + 1)
 *     z  = sqrt(-2 ln(u1 + 2^-25)) cos(2 pi u2)         (u1 + 2^-25 rounded to float32; nothing is drawn where sigma[col_a] == 0)
 *
 * The first layer is handed over in the kernel's form (citylearn_amd/policy.py::StorageMLPPolicy.pack writes it): a hidden unit's tanh is
 * (1 - e) / (1 + e), e = 2^(-2 log2(e) x), so `pre` and `dep` carry the factor -2 log2(e) as in citylearn_amd_policy.h.
 */
#ifndef CITYLEARN_AMD_POLICY_FULL_H
#define CITYLEARN_AMD_POLICY_FULL_H

#include "citylearn_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLPF_ABI_VERSION 1

#define CLPF_NOISE_KEY 0x9E3779B97F4A7C15ull   /* xor-ed into clpf_mlp.seed (the key of citylearn_amd_policy.h: `policy.noise_host` replays both) */

/* env-dependent inputs of the first layer (rows of `dep`) */
#define CLPF_ND       5
#define CLPF_D_SOC    0   /* electrical storage soc (CLS_B_SOC) */
#define CLPF_D_CS     1   /* cooling storage soc (CLS_CS_SOC) */
#define CLPF_D_HS     2   /* heating storage soc (CLS_HS_SOC) */
#define CLPF_D_DS     3   /* DHW storage soc (CLS_DS_SOC) */
#define CLPF_D_NET    4   /* net electricity consumption of the previous step (CLO_NET) */

/* heads (rows of `out`), each driving one storage action column of the building */
#define CLPF_NA       4
#define CLPF_A_ES     0
#define CLPF_A_CS     1
#define CLPF_A_HS     2
#define CLPF_A_DS     3

/* planes of one step of the trajectory record, each [n_bldg][n_env]; a plane of a device the building lacks is written as 0 */
#define CLPF_NT        10
#define CLPF_T_ACTION  0   /* + CLPF_A_*: the action the head's column was driven with (after noise and clamp) */
#define CLPF_T_REWARD  4   /* the building's reward of the step (MARL: after the district exchange) */
#define CLPF_T_NET     5   /* net electricity consumption of the step */
#define CLPF_T_SOC     6   /* + CLPF_D_SOC / _CS / _HS / _DS: the storages' soc AFTER the step -- the policy's inputs at step k are planes 5 .. 9 of step k - 1 */

#define CLPF_MAX_HIDDEN 32

typedef struct clpf_mlp {
    int32_t n_hidden, n_sets, n_device_cols, reserved;   /* n_hidden: 4, 8, .. CLPF_MAX_HIDDEN; reserved: 0.  n_device_cols: how many buildings have a
                                  * cooling / heating / combined DEVICE action column (CLP_ACT_COOL_DEV / _HEAT_DEV / _COH_DEV >= 0), counted by the caller
                                  * from its host copy of `params` (device memory, which the entry point cannot read): anything but 0 is refused */
    const float* pre;          /* [n_sets][n_ts_rows][n_bldg][n_hidden]       env-independent part of layer 1, activation scale folded in */
    const float* dep;          /* [n_sets][n_bldg][CLPF_ND][n_hidden]         weights of the five env-dependent inputs (affine map of the observation folded in) */
    const float* out;          /* [n_sets][n_bldg][CLPF_NA][n_hidden + 1]     output weights of the four heads, bias last */
    const int32_t* set_of_block; /* nullable [ceil(n_env / CL_ROW0_BLOCK)]: parameter set of every env block (NULL = set 0).  DEVICE memory: every entry
                                  * MUST lie in [0, n_sets) */
    const float* net_reset;    /* nullable [n_ts_rows][n_bldg] */
    const float* act_low; const float* act_high; const float* sigma;   /* [n_act_cols]; sigma nullable = 0 */
    uint64_t seed;
} clpf_mlp;

int clpf_abi_version(void);          /* CLPF_ABI_VERSION of the build */
int clpf_core_abi_version(void);     /* the CL_ABI_VERSION of citylearn_amd.h it was built against */
const char* clpf_last_error(void);

/* K steps t0 .. t0 + k_steps - 1 in ONE launch of cl_rollout_full_policy_kernel<envs per lane, PREC, MARL> (reported through cl_tuning.kernel_name).
 * dims: districts WITHOUT CLD_LEAN of up to 16 buildings (one building per wave, never building-chunked) whose buildings have storage action
 * columns only (no cooling / heating / combined device action), the fp32 battery map or CLD_F64_CHAIN, every reward kind but CLR_EV, env_row0 /
 * env_offset as in cl_rollout_f32; no CLD_F64_MAPS, CLD_KPI, CLD_WRITE_DETAIL, no env_pitch.  The float64 chain and CLR_MARL run at one env per
 * lane; cl_tuning.vec (1 or 2) / .nw (= n_bldg) override the geometry.
 * state / out_bldg / out_env: as cl_rollout_f32 leaves them.  ret_env (nullable [n_env]) += the district reward summed over the K steps.
 * traj (nullable [k_steps][CLPF_NT][n_bldg][n_env]): every step's planes.  Returns CL_OK or a CL_E* code (message: clpf_last_error); all
 * argument checks happen before the first HIP call. */
int clpf_rollout_mlp_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpf_mlp* mlp,
                         float* out_bldg, float* out_env, float* ret_env, float* traj, int32_t t0, int32_t k_steps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CITYLEARN_AMD_POLICY_FULL_H */
