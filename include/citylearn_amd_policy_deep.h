/* citylearn_amd_policy_deep.h -- C interface of libcitylearn_amd_policy_deep.so: the fused K-step rollout of a battery + PV district driven by a
 * CLOSED-LOOP policy with TWO hidden tanh layers per building, evaluated inside the rollout kernel (csrc/cl_policy_deep.h).
 *
 * A library of its own beside libcitylearn_amd.so and libcitylearn_amd_policy.so (whose symbol lists, structs and flag sets it leaves untouched);
 * it shares cl_dims / cl_tuning, the plane layouts and the error codes with citylearn_amd.h, and the record's planes (CLPOL_NT, CLPOL_T_*) and
 * the noise stream (CLPOL_NOISE_KEY) with citylearn_amd_policy.h.  Every name it exports starts with `clpd_`.  No mutable state besides the
 * thread-local error string.
 *
 * Per owned (env, building) and step t (table row r, parameter set s, x_soc / x_net as in citylearn_amd_policy.h):
 *     h1_j  = tanh(pre[s][r][b][j] + dep[s][b][0][j] x_soc + dep[s][b][1][j] x_net)                    j < n_hidden
 *     h2_i  = tanh(l2[s][b][n_hidden][i] + sum_j l2[s][b][j][i] h1_j)                                   i < n_hidden2, j ascending, fused multiply-adds
 *     mean  = mid[col] + half[col] tanh(out[s][b][n_hidden2] + sum_i out[s][b][i] h2_i)
 *     a     = clamp(mean + sigma[col] z, act_low[col], act_high[col])                                  z: citylearn_amd_policy.h's draw
 *
 * BOTH HIDDEN LAYERS ARE HANDED OVER IN THE KERNEL'S FORM (citylearn_amd/policy.py::DeepMLPPolicy.pack writes them): a hidden unit's tanh is
 * (1 - e) / (1 + e), e = 2^(-2 log2(e) x), so for weights W1, b1, W2, b2, w3, b3 of the plain MLP
 *     pre, dep         as citylearn_amd_policy.h defines them for W1, b1
 *     l2[s][b][j][i]   = -2 log2(e) W2[i][j]   (j < n_hidden: the TRANSPOSE, one row per h1 unit),     l2[s][b][n_hidden][i] = -2 log2(e) b2[i]
 *     out[s][b][i]     = w3[i]   (i < n_hidden2),                                                       out[s][b][n_hidden2] = b3
 *
 * Under CLPD_MATRIX_CORES `l2` holds per (set, building) 1024 + 32 + 4 floats instead, with W = -2 log2(e) W2 zero-padded to 32 x 32, sw the power
 * of two that puts the building's largest |W| into [2^13, 2^14), and W' = sw W:
 *     words 0 .. 1023   the A-operand fragments [kk][term][lane][8] as f16 (two per word): element [lane][j] is the term of
 *                       W'[lane & 31][16 kk + 8 (lane >> 5) + j], term 0 = f16(W'), term 1 = f16(2^11 (W' - term 0))
 *     words 1024 .. 1055  2^12 sw (-2 log2(e)) b2[i], zero-padded to 32
 *     word 1056           2^-12 / sw;   words 1057 .. 1059: 0
 * h2 then differs from the fp32 form by the split alone: at most 3 x 2^-22 sum_j |W[i][j]| per layer-2 sum, plus 2^-25 |W[i][j]| + 2^-26 max |W|
 * per product should the hardware flush subnormal f16 terms (csrc/cl_policy_deep.h, tests/policy_deep_util.py).
 */
#ifndef CITYLEARN_AMD_POLICY_DEEP_H
#define CITYLEARN_AMD_POLICY_DEEP_H

#include "citylearn_amd_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLPD_ABI_VERSION 1

#define CLPD_MAX_HIDDEN 32

/* clpd_mlp.flags */
#define CLPD_MATRIX_CORES 1   /* layer 2 on the f16 matrix cores (v_mfma_f32_32x32x16_f16) with both operands split into two scaled f16 terms and the
                               * three partial products i + j <= 1; `l2` is then in the FRAGMENT layout below.  Without it: exact fp32 */

typedef struct clpd_mlp {
    int32_t n_hidden, n_sets, flags, reserved;   /* n_hidden (layer 1): 4, 8, .. CLPD_MAX_HIDDEN; flags: 0 or CLPD_MATRIX_CORES; reserved: 0 */
    const float* pre;          /* [n_sets][n_ts_rows][n_bldg][n_hidden] */
    const float* dep;          /* [n_sets][n_bldg][2][n_hidden] */
    const float* out;          /* [n_sets][n_bldg][n_hidden2 + 1]        output weights over layer 2, bias last */
    const int32_t* set_of_block; /* nullable, DEVICE memory; as clpol_mlp's */
    const float* net_reset;    /* nullable [n_ts_rows][n_bldg] */
    const float* act_low; const float* act_high; const float* sigma;   /* [n_act_cols]; sigma nullable = 0 */
    uint64_t seed;
    int32_t n_hidden2, reserved2;                /* n_hidden2 (layer 2): 4, 8, .. CLPD_MAX_HIDDEN, independent of n_hidden; reserved2: 0 */
    const float* l2;           /* [n_sets][n_bldg][n_hidden + 1][n_hidden2]  layer 2 transposed, activation scale folded in, bias row last;
                                * under CLPD_MATRIX_CORES [n_sets][n_bldg][1024 + 32 + 4], see above */
} clpd_mlp;

int clpd_abi_version(void);          /* CLPD_ABI_VERSION of the build */
int clpd_core_abi_version(void);     /* the CL_ABI_VERSION of citylearn_amd.h it was built against */
const char* clpd_last_error(void);

/* K steps t0 .. t0 + k_steps - 1 in ONE launch of cl_rollout_policy_deep_kernel<envs per lane, PREC, MMA> (reported through cl_tuning.kernel_name;
 * MMA = 1 under CLPD_MATRIX_CORES).
 * dims: CLD_LEAN districts of up to 32 buildings, the fp32 battery map or CLD_F64_CHAIN, every reward kind but CLR_EV and CLR_MARL, env_row0 /
 * env_offset as in cl_rollout_f32; no CLD_F64_MAPS, CLD_KPI, CLD_WRITE_DETAIL, no env_pitch.  One env per lane (cl_tuning.vec: 0 or 1);
 * cl_tuning.nw overrides the waves.  A wave keeps both of its buildings' layer-2 weights in LDS for all K steps: a geometry whose rows exceed a
 * CU's LDS is refused (32 buildings at 32 x 32 hidden units do; 32 at 32 x 28 and 30 at 32 x 32 fit; under CLPD_MATRIX_CORES a row has the
 * 32 x 32 size at every n_hidden, n_hidden2, so 30 buildings fit and 31 do not).
 * Buffers, ret_env and traj ([k_steps][CLPOL_NT][n_bldg][n_env]) as clpol_rollout_mlp_f32.  Returns CL_OK or a CL_E* code (message:
 * clpd_last_error); all argument checks happen before the first HIP call. */
int clpd_rollout_mlp_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpd_mlp* mlp,
                         float* out_bldg, float* out_env, float* ret_env, float* traj, int32_t t0, int32_t k_steps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CITYLEARN_AMD_POLICY_DEEP_H */
