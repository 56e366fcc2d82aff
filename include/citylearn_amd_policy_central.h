/* citylearn_amd_policy_central.h -- C interface of libcitylearn_amd_policy_central.so: the fused K-step rollout of a battery + PV district driven by a
 * CLOSED-LOOP CENTRAL-AGENT policy -- ONE tanh MLP with one hidden layer over the district's observation vector that returns every building's
 * storage action -- evaluated inside the rollout kernel (csrc/cl_policy_central.h).
 *
 * A library of its own beside libcitylearn_amd.so and the per-building policy libraries (whose symbol lists, structs and flag sets it leaves
 * untouched); it shares cl_dims / cl_tuning, the plane layouts and the error codes with citylearn_amd.h, and the record's planes (CLPOL_NT,
 * CLPOL_T_*) and the noise stream (CLPOL_NOISE_KEY) with citylearn_amd_policy.h.  Every name it exports starts with `clpca_`.  No mutable state
 * besides the thread-local error string.
 *
 * Per env and step t (table row r, parameter set s; x_soc[b] / x_net[b]: building b's soc before the step and its net of the previous step, as
 * in citylearn_amd_policy.h), with the buildings b' = 0 .. n_bldg - 1 ascending and soc before net -- one chain of fused multiply-adds from 0,
 * to which pre is added last (the order is part of the interface: it does not depend on cl_tuning.nw):
 *     z_j   = pre[s][r][j] + sum_b' (ws[b'][j] x_soc[b'] + wn[b'][j] x_net[b'])                        j < n_hidden
 *     h_j   = (1 - e) / (1 + e),  e = 2^z_j          (= tanh of the unscaled sum: the packer folds -2 log2(e) into pre / dep)
 *     mean  = mid[col] + half[col] tanh(out[s][b][n_hidden] + sum_j out[s][b][j] h_j)                  j ascending from 0, the bias added last; for every
 *                                                                                                      building b with a storage column
 *     a     = clamp(mean + sigma[col] z, act_low[col], act_high[col])                                  z: citylearn_amd_policy.h's draw
 *
 * THE FIRST LAYER IS HANDED OVER IN THE KERNEL'S FORM (citylearn_amd/policy.py::CentralMLPPolicy.pack writes it).  For weights W1 [n_hidden][n_cols]
 * over the central-agent observation vector obs[c] = table[r][c] + col_scale[c] plane[c] (a plane for every building's own electrical_storage_soc
 * and net_electricity_consumption only):
 *     pre[s][r][j]            = -2 log2(e) (b1[j] + sum_c W1[j][c] table[r][c])                         NO building axis
 *     dep[s][g][b][0][u]      = -2 log2(e) W1[4 g + u][soc column of b] col_scale      = ws[b][4 g + u]  (0 where b has no such column)
 *     dep[s][g][b][1][u]      = -2 log2(e) W1[4 g + u][net column of b] col_scale      = wn[b][4 g + u]
 *     out[s][b][j]            = w2[b][j],   out[s][b][n_hidden] = b2[b]
 * `dep` is [n_sets][n_hidden / 4][n_bldg][2][4]: the eight weights a group of four hidden units takes from one building are consecutive, and
 * the buildings of a group follow each other -- the order the kernel walks them in.  An UNDRIVEN building (no storage column) has dep rows
 * like any other and no head: its out row is never read.
 */
#ifndef CITYLEARN_AMD_POLICY_CENTRAL_H
#define CITYLEARN_AMD_POLICY_CENTRAL_H

#include "citylearn_amd_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLPCA_ABI_VERSION 1

#define CLPCA_MAX_HIDDEN 64     /* one hidden layer serves all buildings: twice the per-building width */
#define CLPCA_MAX_BLDG 32

/* clpol_mlp's fields under the same names and in the same order; only the shapes of pre / dep differ */
typedef struct clpca_mlp {
    int32_t n_hidden, n_sets, flags, reserved;   /* n_hidden: 4, 8, .. CLPCA_MAX_HIDDEN; flags, reserved: 0 */
    const float* pre;          /* [n_sets][n_ts_rows][n_hidden] */
    const float* dep;          /* [n_sets][n_hidden / 4][n_bldg][2][4] */
    const float* out;          /* [n_sets][n_bldg][n_hidden + 1]        output weights, bias last */
    const int32_t* set_of_block; /* nullable, DEVICE memory; as clpol_mlp's */
    const float* net_reset;    /* nullable [n_ts_rows][n_bldg] */
    const float* act_low; const float* act_high; const float* sigma;   /* [n_act_cols]; sigma nullable = 0 */
    uint64_t seed;
} clpca_mlp;

int clpca_abi_version(void);          /* CLPCA_ABI_VERSION of the build */
int clpca_core_abi_version(void);     /* the CL_ABI_VERSION of citylearn_amd.h it was built against */
const char* clpca_last_error(void);

/* K steps t0 .. t0 + k_steps - 1 in ONE launch of cl_rollout_policy_central_kernel<PREC> (reported through cl_tuning.kernel_name).
 * dims: CLD_LEAN districts of up to CLPCA_MAX_BLDG buildings, the fp32 battery map or CLD_F64_CHAIN, every reward kind but CLR_EV (CLR_MARL
 * included: the kernel's second barrier of a step carries it), env_row0 / env_offset as in cl_rollout_f32; no CLD_F64_MAPS, CLD_KPI,
 * CLD_WRITE_DETAIL, no env_pitch.  One env per lane (cl_tuning.vec: 0 or 1); cl_tuning.nw overrides the waves (two buildings per wave:
 * (n_bldg + 1) / 2 <= nw <= min(n_bldg, 16)) and changes no action, net or soc: every sum that feeds them has a fixed order.
 * Dynamic LDS per workgroup, in floats (csrc/cl_policy_central.h; the launch opts in above 64 KiB, a CU's 160 KiB are never reached):
 *     nw x 4 x 64  +  2 x n_bldg x 64  +  n_hidden x 64  +  2 x n_hidden x n_bldg  +  nw x 2 x (CLPCA_MAX_HIDDEN + 8)
 *     reduction rows  X (soc, net)       Hh                 staged dep                staged out rows
 * Buffers, ret_env and traj ([k_steps][CLPOL_NT][n_bldg][n_env]) as clpol_rollout_mlp_f32.  Returns CL_OK or a CL_E* code (message:
 * clpca_last_error); all argument checks happen before the first HIP call. */
int clpca_rollout_mlp_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpca_mlp* mlp,
                          float* out_bldg, float* out_env, float* ret_env, float* traj, int32_t t0, int32_t k_steps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CITYLEARN_AMD_POLICY_CENTRAL_H */
