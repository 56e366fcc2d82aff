/* citylearn_amd_policy_full_central_deep.h -- C interface of libcitylearn_amd_policy_full_central_deep.so: the fused K-step rollout of a THERMAL
 * district (cooling / heating / DHW storage beside the battery: the 2020 / 2021 schemas) driven by a CLOSED-LOOP CENTRAL-AGENT policy with TWO
 * hidden tanh layers -- ONE MLP of the shape of a SAC / PPO actor over the district's observation vector that returns every building's storage
 * actions, up to four heads per building -- evaluated inside the rollout kernel (csrc/cl_policy_full_central.h at DEEP = true).
 *
 * A library of its own beside libcitylearn_amd.so and the twelve other policy libraries (whose symbol lists, structs and kernels it leaves
 * untouched); it shares cl_dims / cl_tuning, the plane layouts and the error codes with citylearn_amd.h, and the terms (CLPF_ND, CLPF_D_*), the
 * heads (CLPF_NA, CLPF_A_*), the record's planes (CLPF_NT, CLPF_T_*) and the noise stream (CLPF_NOISE_KEY) with citylearn_amd_policy_full.h.  Every
 * name it exports starts with `clpfcd_`.  No mutable state besides the thread-local error string.
 *
 * Per env and step t (table row r, parameter set s; x_d[b]: building b's soc / cs / hs / ds before the step and its net of the previous step,
 * as in citylearn_amd_policy_full.h; 0 where b has no such storage).  The order of every sum is part of the interface: the buildings
 * b' = 0 .. n_bldg - 1 ascending and per building the terms d in CLPF_D_* order -- one chain of fused multiply-adds from 0, to which pre is added
 * last; layer 2 over j = 0 .. n_hidden - 1 ascending, one chain of fused multiply-adds from 0, to which the bias row is added last; the heads
 * over i = 0 .. n_hidden2 - 1 ascending, the bias last:
 *     z1_j   = pre[s][r][j] + sum_b' sum_d dep[s][j / 4][b'][d][j % 4] x_d[b']                          j < n_hidden
 *     h1_j   = (1 - e) / (1 + e),  e = 2^z1_j        (= tanh of the unscaled sum: the packer folds -2 log2(e) into pre / dep)
 *     z2_i   = l2[s][n_hidden][i] + sum_j l2[s][j][i] h1_j                                              i < n_hidden2
 *     h2_i   = (1 - e) / (1 + e),  e = 2^z2_i        (the packer folds -2 log2(e) into l2)
 *     mean_a = mid[col_a] + half[col_a] tanh(out[s][b][a][n_hidden2] + sum_i out[s][b][a][i] h2_i)      for every head a of building b that has
 *                                                                                                       its action column col_a
 *     act_a  = clamp(mean_a + sigma[col_a] z_a, act_low[col_a], act_high[col_a])                        z_a: citylearn_amd_policy_full.h's draw
 * Layer 2 is one n_hidden x n_hidden2 product per env in exact fp32; there is no matrix-core family.
 *
 * BOTH HIDDEN LAYERS ARE HANDED OVER IN THE KERNEL'S FORM (citylearn_amd/policy.py::DeepCentralStorageMLPPolicy.pack writes them).  For weights
 * W1 [n_hidden][n_cols], b1, W2 [n_hidden2][n_hidden], b2, w3, b3 of the plain MLP over the central-agent observation vector:
 *     pre, dep                as citylearn_amd_policy_full_central.h defines them for W1, b1
 *     l2[s][j][i]             = -2 log2(e) W2[i][j]   (j < n_hidden: the TRANSPOSE, one row per h1 unit),   l2[s][n_hidden][i] = -2 log2(e) b2[i]
 *     out[s][b][a][i]         = w3[b][a][i]   (i < n_hidden2),                                              out[s][b][a][n_hidden2] = b3[b][a]
 */
#ifndef CITYLEARN_AMD_POLICY_FULL_CENTRAL_DEEP_H
#define CITYLEARN_AMD_POLICY_FULL_CENTRAL_DEEP_H

#include "citylearn_amd_policy_full.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLPFCD_ABI_VERSION 1

#define CLPFCD_MAX_HIDDEN 64     /* either hidden layer: 4, 8, .. 64 units, independent of each other */
#define CLPFCD_MAX_BLDG 16       /* one building per wave, the whole district in one workgroup */

/* clpfca_mlp's fields under the same names and in the same order, then the second layer's: clpfd_mlp's tail */
typedef struct clpfcd_mlp {
    int32_t n_hidden, n_sets, n_device_cols, reserved;   /* n_hidden (layer 1): 4, 8, .. CLPFCD_MAX_HIDDEN; reserved: 0; n_device_cols as clpf_mlp's: anything but 0 is refused */
    const float* pre;          /* [n_sets][n_ts_rows][n_hidden] */
    const float* dep;          /* [n_sets][n_hidden / 4][n_bldg][CLPF_ND][4] */
    const float* out;          /* [n_sets][n_bldg][CLPF_NA][n_hidden2 + 1]       output weights of the four heads over layer 2, bias last */
    const int32_t* set_of_block; /* nullable, DEVICE memory; as clpf_mlp's */
    const float* net_reset;    /* nullable [n_ts_rows][n_bldg] */
    const float* act_low; const float* act_high; const float* sigma;   /* [n_act_cols]; sigma nullable = 0 */
    uint64_t seed;
    int32_t n_hidden2, flags;  /* n_hidden2 (layer 2): 4, 8, .. CLPFCD_MAX_HIDDEN, independent of n_hidden; flags: 0 */
    const float* l2;           /* [n_sets][n_hidden + 1][n_hidden2]              layer 2 transposed, activation scale folded in, bias row last */
} clpfcd_mlp;

int clpfcd_abi_version(void);          /* CLPFCD_ABI_VERSION of the build */
int clpfcd_core_abi_version(void);     /* the CL_ABI_VERSION of citylearn_amd.h it was built against */
const char* clpfcd_last_error(void);

/* K steps t0 .. t0 + k_steps - 1 in ONE launch of cl_rollout_full_policy_central_deep_kernel<PREC, MARL> (reported through
 * cl_tuning.kernel_name).
 * dims: districts WITHOUT CLD_LEAN of up to CLPFCD_MAX_BLDG buildings whose buildings have storage action columns only, the fp32 battery map or
 * CLD_F64_CHAIN, every reward kind but CLR_EV (CLR_MARL included: the kernel's last barrier of a step carries it), env_row0 / env_offset as in
 * cl_rollout_f32; no CLD_F64_MAPS, CLD_KPI, CLD_WRITE_DETAIL, no env_pitch.  One building per wave (cl_tuning.nw: 0 or n_bldg), one env per lane
 * (cl_tuning.vec: 0 or 1).
 * Dynamic LDS per workgroup, in floats (csrc/cl_policy_full_central.h; the launch opts in above 64 KiB, a CU's 160 KiB are never reached:
 * 125 184 bytes at sixteen buildings and 64 x 64 units):
 *     nw x 4 x 64  +  5 x n_bldg x 64  +  n_hidden x 64  +  n_hidden2 x 64  +  5 x n_hidden x n_bldg  +  (n_hidden + 1) x n_hidden2  +  nw x (4 x CLPFCD_MAX_HIDDEN + 4 x 8)
 *     reduction rows  X (soc, cs, hs, ds, net)  Hh (layer 1)   Hh2 (layer 2)     staged dep                staged l2                      staged head rows
 * Buffers, ret_env and traj ([k_steps][CLPF_NT][n_bldg][n_env]) as clpf_rollout_mlp_f32.  Returns CL_OK or a CL_E* code (message:
 * clpfcd_last_error); all argument checks happen before the first HIP call. */
int clpfcd_rollout_mlp_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpfcd_mlp* mlp,
                           float* out_bldg, float* out_env, float* ret_env, float* traj, int32_t t0, int32_t k_steps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CITYLEARN_AMD_POLICY_FULL_CENTRAL_DEEP_H */
