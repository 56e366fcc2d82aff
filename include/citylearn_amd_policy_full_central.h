/* citylearn_amd_policy_full_central.h -- C interface of libcitylearn_amd_policy_full_central.so: the fused K-step rollout of a THERMAL district
 * (cooling / heating / DHW storage beside the battery: the 2020 / 2021 schemas) driven by a CLOSED-LOOP CENTRAL-AGENT policy -- ONE tanh MLP with
 * one hidden layer over the district's observation vector that returns every building's storage actions, up to four heads per building --
 * evaluated inside the rollout kernel (csrc/cl_policy_full_central.h at DEEP = false).
 *
 * A library of its own beside libcitylearn_amd.so and the other policy libraries (whose symbol lists, structs and kernels it leaves untouched);
 * it shares cl_dims / cl_tuning, the plane layouts and the error codes with citylearn_amd.h, and the terms (CLPF_ND, CLPF_D_*), the heads
 * (CLPF_NA, CLPF_A_*), the record's planes (CLPF_NT, CLPF_T_*) and the noise stream (CLPF_NOISE_KEY) with citylearn_amd_policy_full.h.  Every
 * name it exports starts with `clpfca_`.  No mutable state besides the thread-local error string.
 *
 * Per env and step t (table row r, parameter set s; x_d[b]: building b's soc / cs / hs / ds before the step and its net of the previous step,
 * as in citylearn_amd_policy_full.h; 0 where b has no such storage), with the buildings b' = 0 .. n_bldg - 1 ascending and per building the
 * terms d in CLPF_D_* order -- one chain of fused multiply-adds from 0, to which pre is added last (the order is part of the interface):
 *     z_j    = pre[s][r][j] + sum_b' sum_d dep[s][j / 4][b'][d][j % 4] x_d[b']                          j < n_hidden
 *     h_j    = (1 - e) / (1 + e),  e = 2^z_j         (= tanh of the unscaled sum: the packer folds -2 log2(e) into pre / dep)
 *     mean_a = mid[col_a] + half[col_a] tanh(out[s][b][a][n_hidden] + sum_j out[s][b][a][j] h_j)        j ascending from 0, the bias added last;
 *                                                                                                       for every head a of building b that has
 *                                                                                                       its action column col_a
 *     act_a  = clamp(mean_a + sigma[col_a] z_a, act_low[col_a], act_high[col_a])                        z_a: citylearn_amd_policy_full.h's draw
 *
 * THE FIRST LAYER IS HANDED OVER IN THE KERNEL'S FORM (citylearn_amd/policy.py::CentralStorageMLPPolicy.pack writes it).  For weights
 * W1 [n_hidden][n_cols] over the central-agent observation vector obs[c] = table[r][c] + col_scale[c] plane[c] (a plane for every building's
 * own storage socs and net_electricity_consumption only):
 *     pre[s][r][j]            = -2 log2(e) (b1[j] + sum_c W1[j][c] table[r][c])                         NO building axis
 *     dep[s][g][b][d][u]      = -2 log2(e) W1[4 g + u][column of b's term d] col_scale                  (0 where b has no such column / storage)
 *     out[s][b][a][j]         = w2[b][a][j],   out[s][b][a][n_hidden] = b2[b][a]
 * `dep` is [n_sets][n_hidden / 4][n_bldg][CLPF_ND][4]: the twenty weights a group of four hidden units takes from one building are consecutive,
 * and the buildings of a group follow each other -- the order the kernel walks them in.
 */
#ifndef CITYLEARN_AMD_POLICY_FULL_CENTRAL_H
#define CITYLEARN_AMD_POLICY_FULL_CENTRAL_H

#include "citylearn_amd_policy_full.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLPFCA_ABI_VERSION 1

#define CLPFCA_MAX_HIDDEN 64     /* one hidden layer serves all buildings: twice the per-building width */
#define CLPFCA_MAX_BLDG 16       /* one building per wave, the whole district in one workgroup */

/* clpf_mlp's fields under the same names and in the same order; only the shapes of pre / dep differ */
typedef struct clpfca_mlp {
    int32_t n_hidden, n_sets, n_device_cols, reserved;   /* n_hidden: 4, 8, .. CLPFCA_MAX_HIDDEN; reserved: 0; n_device_cols as clpf_mlp's: anything but 0 is refused */
    const float* pre;          /* [n_sets][n_ts_rows][n_hidden] */
    const float* dep;          /* [n_sets][n_hidden / 4][n_bldg][CLPF_ND][4] */
    const float* out;          /* [n_sets][n_bldg][CLPF_NA][n_hidden + 1]        output weights of the four heads, bias last */
    const int32_t* set_of_block; /* nullable, DEVICE memory; as clpf_mlp's */
    const float* net_reset;    /* nullable [n_ts_rows][n_bldg] */
    const float* act_low; const float* act_high; const float* sigma;   /* [n_act_cols]; sigma nullable = 0 */
    uint64_t seed;
} clpfca_mlp;

int clpfca_abi_version(void);          /* CLPFCA_ABI_VERSION of the build */
int clpfca_core_abi_version(void);     /* the CL_ABI_VERSION of citylearn_amd.h it was built against */
const char* clpfca_last_error(void);

/* K steps t0 .. t0 + k_steps - 1 in ONE launch of cl_rollout_full_policy_central_kernel<PREC, MARL> (reported through cl_tuning.kernel_name).
 * dims: districts WITHOUT CLD_LEAN of up to CLPFCA_MAX_BLDG buildings whose buildings have storage action columns only, the fp32 battery map or
 * CLD_F64_CHAIN, every reward kind but CLR_EV (CLR_MARL included: the kernel's second barrier of a step carries it), env_row0 / env_offset as in
 * cl_rollout_f32; no CLD_F64_MAPS, CLD_KPI, CLD_WRITE_DETAIL, no env_pitch.  One building per wave (cl_tuning.nw: 0 or n_bldg), one env per lane
 * (cl_tuning.vec: 0 or 1).
 * Dynamic LDS per workgroup, in floats (csrc/cl_policy_full_central.h; the launch opts in above 64 KiB, a CU's 160 KiB are never reached):
 *     nw x 4 x 64  +  5 x n_bldg x 64  +  n_hidden x 64  +  5 x n_hidden x n_bldg  +  nw x (4 x CLPFCA_MAX_HIDDEN + 4 x 8)
 *     reduction rows  X (soc, cs, hs, ds, net)  Hh          staged dep                staged head rows
 * Buffers, ret_env and traj ([k_steps][CLPF_NT][n_bldg][n_env]) as clpf_rollout_mlp_f32.  Returns CL_OK or a CL_E* code (message:
 * clpfca_last_error); all argument checks happen before the first HIP call. */
int clpfca_rollout_mlp_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpfca_mlp* mlp,
                           float* out_bldg, float* out_env, float* ret_env, float* traj, int32_t t0, int32_t k_steps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CITYLEARN_AMD_POLICY_FULL_CENTRAL_H */
