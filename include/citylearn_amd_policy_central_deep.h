/* citylearn_amd_policy_central_deep.h -- C interface of libcitylearn_amd_policy_central_deep.so: the fused K-step rollout of a battery + PV district
 * driven by a CLOSED-LOOP CENTRAL-AGENT policy with TWO hidden layers -- ONE tanh MLP over the district's observation vector that returns every
 * building's storage action, the shape of a SAC / PPO actor trained with central_agent=True -- evaluated inside the rollout kernel
 * (csrc/cl_policy_central.h at DEEP = true).
 *
 * A library of its own beside libcitylearn_amd.so and the other policy libraries (whose symbol lists, structs and flag sets it leaves untouched);
 * it shares cl_dims / cl_tuning, the plane layouts and the error codes with citylearn_amd.h, and the record's planes (CLPOL_NT, CLPOL_T_*) and
 * the noise stream (CLPOL_NOISE_KEY) with citylearn_amd_policy.h.  Every name it exports starts with `clpcd_`.  No mutable state besides the
 * thread-local error string.
 *
 * Per env and step t (table row r, parameter set s; x_soc[b] / x_net[b]: building b's soc before the step and its net of the previous step, as
 * in citylearn_amd_policy.h).  Every sum is ONE chain of fused multiply-adds from 0 in ascending index order -- in layer 1 the buildings
 * b' = 0 .. n_bldg - 1 with soc before net -- to which pre / the bias is added LAST (the order is part of the interface: it does not depend on
 * cl_tuning.nw):
 *     z1_j  = pre[s][r][j] + sum_b' (ws[b'][j] x_soc[b'] + wn[b'][j] x_net[b'])                        j < n_hidden
 *     h1_j  = (1 - e) / (1 + e),  e = 2^z1_j         (= tanh of the unscaled sum: the packer folds -2 log2(e) into pre / dep / l2)
 *     z2_i  = l2[s][n_hidden][i] + sum_j l2[s][j][i] h1_j                                             i < n_hidden2
 *     h2_i  = (1 - e) / (1 + e),  e = 2^z2_i
 *     mean  = mid[col] + half[col] tanh(out[s][b][n_hidden2] + sum_i out[s][b][i] h2_i)               for every building b with a storage column
 *     a     = clamp(mean + sigma[col] z, act_low[col], act_high[col])                                  z: citylearn_amd_policy.h's draw
 *
 * The first layer is citylearn_amd_policy_central.h's, in its packed form (`pre`, `dep`); the head is its head over the second hidden layer.
 * `l2` is [n_sets][n_hidden + 1][n_hidden2]: -2 log2(e) W2 TRANSPOSED (one row per first-layer unit: the n_hidden2 weights a unit feeds are
 * consecutive), -2 log2(e) b2 as the last row -- clpd_mlp.l2's exact-fp32 layout without the building axis
 * (citylearn_amd/policy.py::DeepCentralMLPPolicy.pack writes all of it).
 */
#ifndef CITYLEARN_AMD_POLICY_CENTRAL_DEEP_H
#define CITYLEARN_AMD_POLICY_CENTRAL_DEEP_H

#include "citylearn_amd_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLPCD_ABI_VERSION 1

#define CLPCD_MAX_HIDDEN 64     /* of either hidden layer */
#define CLPCD_MAX_BLDG 32

/* clpca_mlp's fields under the same names and in the same order, then the second layer's (the extension clpd_mlp makes of clpol_mlp) */
typedef struct clpcd_mlp {
    int32_t n_hidden, n_sets, flags, reserved;   /* n_hidden: 4, 8, .. CLPCD_MAX_HIDDEN; flags, reserved: 0 */
    const float* pre;          /* [n_sets][n_ts_rows][n_hidden] */
    const float* dep;          /* [n_sets][n_hidden / 4][n_bldg][2][4] */
    const float* out;          /* [n_sets][n_bldg][n_hidden2 + 1]       output weights, bias last */
    const int32_t* set_of_block; /* nullable, DEVICE memory; as clpol_mlp's */
    const float* net_reset;    /* nullable [n_ts_rows][n_bldg] */
    const float* act_low; const float* act_high; const float* sigma;   /* [n_act_cols]; sigma nullable = 0 */
    uint64_t seed;
    int32_t n_hidden2, reserved2;                /* n_hidden2: 4, 8, .. CLPCD_MAX_HIDDEN, independent of n_hidden; reserved2: 0 */
    const float* l2;           /* [n_sets][n_hidden + 1][n_hidden2] */
} clpcd_mlp;

int clpcd_abi_version(void);          /* CLPCD_ABI_VERSION of the build */
int clpcd_core_abi_version(void);     /* the CL_ABI_VERSION of citylearn_amd.h it was built against */
const char* clpcd_last_error(void);

/* K steps t0 .. t0 + k_steps - 1 in ONE launch of cl_rollout_policy_central_deep_kernel<PREC> (reported through cl_tuning.kernel_name).
 * dims: CLD_LEAN districts of up to CLPCD_MAX_BLDG buildings, the fp32 battery map or CLD_F64_CHAIN, every reward kind but CLR_EV (CLR_MARL
 * included: the kernel's third barrier of a step carries it), env_row0 / env_offset as in cl_rollout_f32; no CLD_F64_MAPS, CLD_KPI,
 * CLD_WRITE_DETAIL, no env_pitch.  One env per lane (cl_tuning.vec: 0 or 1); cl_tuning.nw overrides the waves (two buildings per wave:
 * (n_bldg + 1) / 2 <= nw <= min(n_bldg, 16)) and changes no action, net or soc: every sum that feeds them has a fixed order.
 * Dynamic LDS per workgroup, in floats (csrc/cl_policy_central.h; the launch opts in above 64 KiB, a CU's 160 KiB are never reached):
 *     nw x 4 x 64  +  2 x n_bldg x 64  +  n_hidden x 64  +  n_hidden2 x 64  +  2 x n_hidden x n_bldg  +  (n_hidden + 1) x n_hidden2  +  nw x 2 x (CLPCD_MAX_HIDDEN + 8)
 *     reduction rows  X (soc, net)       Hh1                Hh2                 staged dep                staged l2                      staged out rows
 * Buffers, ret_env and traj ([k_steps][CLPOL_NT][n_bldg][n_env]) as clpol_rollout_mlp_f32.  Returns CL_OK or a CL_E* code (message:
 * clpcd_last_error); all argument checks happen before the first HIP call. */
int clpcd_rollout_mlp_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpcd_mlp* mlp,
                          float* out_bldg, float* out_env, float* ret_env, float* traj, int32_t t0, int32_t k_steps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CITYLEARN_AMD_POLICY_CENTRAL_DEEP_H */
