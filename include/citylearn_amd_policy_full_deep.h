/* citylearn_amd_policy_full_deep.h -- C interface of libcitylearn_amd_policy_full_deep.so: the fused K-step rollout of a THERMAL district (cooling /
 * heating / DHW storage beside the battery: the 2020 / 2021 schemas) driven by a CLOSED-LOOP policy with TWO hidden tanh layers per building and up
 * to four storage heads, evaluated inside the rollout kernel (csrc/cl_policy_full_deep.h).
 *
 * A library of its own beside libcitylearn_amd.so and the eight other policy libraries (whose symbol lists, structs and kernels it leaves
 * untouched); it shares cl_dims / cl_tuning, the plane layouts and the error codes with citylearn_amd.h, and the inputs (CLPF_ND, CLPF_D_*), the
 * heads (CLPF_NA, CLPF_A_*), the record's planes (CLPF_NT, CLPF_T_*) and the noise stream (CLPF_NOISE_KEY) with citylearn_amd_policy_full.h.  Every
 * name it exports starts with `clpfd_`.  No mutable state besides the thread-local error string.
 *
 * Per (env, building) and step t (table row r, parameter set s, x = (soc, cs, hs, ds, net_prev) as in citylearn_amd_policy_full.h):
 *     h1_j   = tanh(pre[s][r][b][j] + sum_d dep[s][b][d][j] x_d)                                        j < n_hidden, d < CLPF_ND
 *     h2_i   = tanh(l2[s][b][n_hidden][i] + sum_j l2[s][b][j][i] h1_j)                                  i < n_hidden2, j ascending, fused multiply-adds
 *     mean_a = mid[col_a] + half[col_a] tanh(out[s][b][a][n_hidden2] + sum_i out[s][b][a][i] h2_i)      a < CLPF_NA
 *     act_a  = clamp(mean_a + sigma[col_a] z_a, act_low[col_a], act_high[col_a])                        z_a: citylearn_amd_policy_full.h's draw
 * A head whose column the building lacks is not evaluated, a term d whose storage the building lacks is skipped (its row of `dep` must be 0).
 *
 * BOTH HIDDEN LAYERS ARE HANDED OVER IN THE KERNEL'S FORM (citylearn_amd/policy.py::DeepStorageMLPPolicy.pack writes them): a hidden unit's tanh
 * is (1 - e) / (1 + e), e = 2^(-2 log2(e) x), so for weights W1, b1, W2, b2, w3, b3 of the plain MLP
 *     pre, dep         as citylearn_amd_policy_full.h defines them for W1, b1
 *     l2[s][b][j][i]   = -2 log2(e) W2[i][j]   (j < n_hidden: the TRANSPOSE, one row per h1 unit),     l2[s][b][n_hidden][i] = -2 log2(e) b2[i]
 *     out[s][b][a][i]  = w3[a][i]   (i < n_hidden2),                                                    out[s][b][a][n_hidden2] = b3[a]
 * Under CLPFD_MATRIX_CORES `l2` holds per (set, building) 1024 + 32 + 4 floats instead, exactly citylearn_amd_policy_deep.h's fragment layout
 * (layer 2 is the same matrix problem): the A-operand fragments of sw (-2 log2(e)) W2 zero-padded to 32 x 32 as two scaled f16 terms, the bias row
 * 2^12 sw (-2 log2(e)) b2 zero-padded to 32, then 2^-12 / sw and three zeros.  h2 then differs from the fp32 form by the split alone (the bound
 * of citylearn_amd_policy_deep.h per layer-2 sum).
 */
#ifndef CITYLEARN_AMD_POLICY_FULL_DEEP_H
#define CITYLEARN_AMD_POLICY_FULL_DEEP_H

#include "citylearn_amd_policy_full.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLPFD_ABI_VERSION 1

#define CLPFD_MAX_HIDDEN 32

/* clpfd_mlp.flags */
#define CLPFD_MATRIX_CORES 1  /* layer 2 on the f16 matrix cores (v_mfma_f32_32x32x16_f16) with both operands split into two scaled f16 terms and the
                               * three partial products i + j <= 1; `l2` is then in the FRAGMENT layout above.  Without it: exact fp32 */

/* clpf_mlp's fields first, under the same names, then the second layer's (the way clpd_mlp extends clpol_mlp).  clpf_mlp has no flags word -- its
 * third word counts device columns -- so the word behind n_hidden2 carries the flags */
typedef struct clpfd_mlp {
    int32_t n_hidden, n_sets, n_device_cols, reserved;   /* n_hidden (layer 1): 4, 8, .. CLPFD_MAX_HIDDEN; n_device_cols: as clpf_mlp's (anything but 0 is
                                                          * refused); reserved: 0 */
    const float* pre;          /* [n_sets][n_ts_rows][n_bldg][n_hidden] */
    const float* dep;          /* [n_sets][n_bldg][CLPF_ND][n_hidden] */
    const float* out;          /* [n_sets][n_bldg][CLPF_NA][n_hidden2 + 1]   output weights of the four heads over layer 2, bias last */
    const int32_t* set_of_block; /* nullable, DEVICE memory; as clpf_mlp's */
    const float* net_reset;    /* nullable [n_ts_rows][n_bldg] */
    const float* act_low; const float* act_high; const float* sigma;   /* [n_act_cols]; sigma nullable = 0 */
    uint64_t seed;
    int32_t n_hidden2, flags;  /* n_hidden2 (layer 2): 4, 8, .. CLPFD_MAX_HIDDEN, independent of n_hidden; flags: 0 or CLPFD_MATRIX_CORES */
    const float* l2;           /* [n_sets][n_bldg][n_hidden + 1][n_hidden2]  layer 2 transposed, activation scale folded in, bias row last;
                                * under CLPFD_MATRIX_CORES [n_sets][n_bldg][1024 + 32 + 4], see above */
} clpfd_mlp;

int clpfd_abi_version(void);         /* CLPFD_ABI_VERSION of the build */
int clpfd_core_abi_version(void);    /* the CL_ABI_VERSION of citylearn_amd.h it was built against */
const char* clpfd_last_error(void);

/* K steps t0 .. t0 + k_steps - 1 in ONE launch of cl_rollout_full_policy_deep_kernel<PREC, MMA, MARL> (reported through cl_tuning.kernel_name;
 * MMA = 1 under CLPFD_MATRIX_CORES).
 * dims: districts WITHOUT CLD_LEAN of up to 16 buildings (one building per wave, never building-chunked) whose buildings have storage action
 * columns only, the fp32 battery map or CLD_F64_CHAIN, every reward kind but CLR_EV (CLR_MARL in both families), env_row0 / env_offset as in
 * cl_rollout_f32; no CLD_F64_MAPS, CLD_KPI, CLD_WRITE_DETAIL, no env_pitch.  One env per lane (cl_tuning.vec: 0 or 1); cl_tuning.nw = n_bldg.
 * A wave keeps its building's layer-2 weights in LDS for all K steps: 5504 bytes per building at 32 x 32 units in either family, 104 448 per
 * workgroup with the reduction rows at sixteen buildings -- above 64 KiB the kernel is opted in, and every accepted geometry fits a CU's 160 KiB.
 * Buffers, ret_env and traj ([k_steps][CLPF_NT][n_bldg][n_env]) as clpf_rollout_mlp_f32.  Returns CL_OK or a CL_E* code (message:
 * clpfd_last_error); all argument checks happen before the first HIP call. */
int clpfd_rollout_mlp_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpfd_mlp* mlp,
                          float* out_bldg, float* out_env, float* ret_env, float* traj, int32_t t0, int32_t k_steps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CITYLEARN_AMD_POLICY_FULL_DEEP_H */
