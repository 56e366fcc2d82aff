/* citylearn_amd_policy.h -- C interface of libcitylearn_amd_policy.so: the fused K-step rollout of a battery + PV district driven by a
 * CLOSED-LOOP policy, a one-hidden-layer tanh MLP per building evaluated inside the rollout kernel (csrc/cl_policy.h).
 *
 * A library of its own beside libcitylearn_amd.so (whose symbol list, structs and flag set it leaves untouched); it shares cl_dims / cl_tuning,
 * the parameter / time-series / state / output plane layouts and the error codes with citylearn_amd.h.  Every name it exports starts with
 * `clpol_`.  Like the main library it holds no mutable state besides the thread-local error string.
 *
 * Per owned (env, building) and step t of the episode (table row r = env_row0[block] + t, parameter set s = set_of_block[block]):
 *     x_soc = the unit's soc before the step
 *     x_net = the unit's net electricity consumption of the previous step -- at t == 0: net_reset[r][b] (the value the reset observation
 *             shows; NULL = 0); at the first step of a later launch: out_bldg[CLO_NET], what the previous launch left
 *     h_j   = tanh(pre[s][r][b][j] + dep[s][b][0][j] x_soc + dep[s][b][1][j] x_net)                   j < n_hidden
 *     mean  = mid[col] + half[col] tanh(out[s][b][n_hidden] + sum_j out[s][b][j] h_j)                  mid / half from act_low / act_high
 *     a     = clamp(mean + sigma[col] z, act_low[col], act_high[col])
 * with col the building's electrical-storage action column (a building without one is not driven) and z a standard normal by Box-Muller from
 * two draws of the main library's Philox stream, replayable on the host with cl_philox_uniform:
 *     u1 = cl_philox_uniform(seed ^ CLPOL_NOISE_KEY, env_offset + env, col, 2 t),   u2 = cl_philox_uniform(.., 2 t + 1)
 *     z  = sqrt(-2 ln(u1 + 2^-25)) cos(2 pi u2)         (u1 + 2^-25 rounded to float32; nothing is drawn where sigma[col] == 0)
 *
 * THE FIRST LAYER IS HANDED OVER IN THE KERNEL'S FORM (citylearn_amd/policy.py::MLPPolicy.pack writes it): a hidden unit's tanh is evaluated as
 * (1 - e) / (1 + e), e = 2^(-2 log2(e) x), with one v_exp_f32 and one v_rcp_f32, so for weights W1, b1, w2, b2 of the plain MLP
 *     pre[s][r][b][j] = -2 log2(e) (b1[j] + sum_c W1[j][c] table[r][c]),   dep[s][b][k][j] = -2 log2(e) W1[j][c_k] col_scale[c_k]
 *     out[s][b][j]    = w2[j]   (j < n_hidden),                            out[s][b][n_hidden] = b2
 * (`table` / `col_scale`: the observation tables of cl_observe_f32; c_0 / c_1: the building's soc / net columns.)
 */
#ifndef CITYLEARN_AMD_POLICY_H
#define CITYLEARN_AMD_POLICY_H

#include "citylearn_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLPOL_ABI_VERSION 1

#define CLPOL_NOISE_KEY 0x9E3779B97F4A7C15ull   /* xor-ed into clpol_mlp.seed: the noise never shares a stream with cl_rollout_f32's uniform policy */

/* planes of one step of the trajectory record, each [n_bldg][n_env] */
#define CLPOL_NT        4
#define CLPOL_T_ACTION  0   /* the storage action the step was driven with (after noise and clamp) */
#define CLPOL_T_REWARD  1   /* the building's reward of the step (MARL: after the district exchange) */
#define CLPOL_T_NET     2   /* net electricity consumption of the step */
#define CLPOL_T_SOC     3   /* soc AFTER the step: the policy's inputs at step k are planes SOC / NET of step k - 1 */

#define CLPOL_MAX_HIDDEN 32

typedef struct clpol_mlp {
    int32_t n_hidden, n_sets, flags, reserved;   /* n_hidden: 4, 8, .. CLPOL_MAX_HIDDEN; flags / reserved: 0 */
    const float* pre;          /* [n_sets][n_ts_rows][n_bldg][n_hidden]  env-independent part of layer 1, activation scale folded in */
    const float* dep;          /* [n_sets][n_bldg][2][n_hidden]          weights of soc / previous net (affine map of the observation folded in) */
    const float* out;          /* [n_sets][n_bldg][n_hidden + 1]         output weights, bias last */
    const int32_t* set_of_block; /* nullable [ceil(n_env / CL_ROW0_BLOCK)]: parameter set of every env block (NULL = set 0).  DEVICE memory: the entry
                                  * point cannot read it -- every entry MUST lie in [0, n_sets), like cl_dims.env_row0 + n_steps <= n_ts_rows */
    const float* net_reset;    /* nullable [n_ts_rows][n_bldg] */
    const float* act_low; const float* act_high; const float* sigma;   /* [n_act_cols]; sigma nullable = 0 */
    uint64_t seed;
} clpol_mlp;

int clpol_abi_version(void);          /* CLPOL_ABI_VERSION of the build */
int clpol_core_abi_version(void);     /* the CL_ABI_VERSION of citylearn_amd.h it was built against */
const char* clpol_last_error(void);

/* K steps t0 .. t0 + k_steps - 1 in ONE launch of cl_rollout_policy_kernel<envs per lane, PREC> (reported through cl_tuning.kernel_name).
 * dims: CLD_LEAN districts of up to 32 buildings, the fp32 battery map or CLD_F64_CHAIN, every reward kind but CLR_EV, env_row0 / env_offset as
 * in cl_rollout_f32; no CLD_F64_MAPS, CLD_KPI, CLD_WRITE_DETAIL, no env_pitch.  cl_tuning.vec (1 or 2) / .nw override the geometry.
 * state / out_bldg / out_env: as cl_rollout_f32 leaves them (carried state, the last step's planes and district sums).
 * ret_env (nullable [n_env]) += the district reward summed over the K steps.  traj (nullable [k_steps][CLPOL_NT][n_bldg][n_env]): every step's
 * planes.  Returns CL_OK or a CL_E* code (message: clpol_last_error); all argument checks happen before the first HIP call. */
int clpol_rollout_mlp_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpol_mlp* mlp,
                          float* out_bldg, float* out_env, float* ret_env, float* traj, int32_t t0, int32_t k_steps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CITYLEARN_AMD_POLICY_H */
