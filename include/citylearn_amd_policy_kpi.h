/* citylearn_amd_policy_kpi.h -- C interface of libcitylearn_amd_policy_kpi.so: the closed-loop policy rollout of citylearn_amd_policy.h that also
 * keeps the streaming KPI accumulators of a CLD_KPI district inside the launch (csrc/cl_policy.h at KPI = true).
 *
 * A library of its own beside libcitylearn_amd.so and libcitylearn_amd_policy.so, whose symbol lists, structs and kernels it leaves untouched; it
 * shares cl_dims / cl_tuning, the plane layouts and the error codes with citylearn_amd.h and `clpol_mlp`, the trajectory planes and
 * CLPOL_NOISE_KEY with citylearn_amd_policy.h.  Every name it exports starts with `clpk_`.  Like the other two it holds no mutable state besides
 * the thread-local error string.
 *
 * A step is clpol_rollout_mlp_f32's step (same policy, same noise stream, same unit), and the accumulators are the ones cl_rollout_seq_f32 keeps
 * under CLD_ROLLOUT_FUSED | CLD_KPI, in kpi_bldg / kpi_env's layout (CLK_*, CLKE_*) and arithmetic: after the call, the KPI planes are what K
 * calls of cl_step_f32 with the recorded actions would have left.
 */
#ifndef CITYLEARN_AMD_POLICY_KPI_H
#define CITYLEARN_AMD_POLICY_KPI_H

#include "citylearn_amd_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLPK_ABI_VERSION 1

int clpk_abi_version(void);          /* CLPK_ABI_VERSION of the build */
int clpk_core_abi_version(void);     /* the CL_ABI_VERSION of citylearn_amd.h it was built against */
const char* clpk_last_error(void);

/* K steps t0 .. t0 + k_steps - 1 in ONE launch of cl_rollout_policy_kpi_kernel<envs per lane, PREC> (reported through cl_tuning.kernel_name).
 * dims: as clpol_rollout_mlp_f32 takes them, but CLD_KPI is REQUIRED: CLD_LEAN districts of up to 32 buildings, the fp32 battery map or
 * CLD_F64_CHAIN, every reward kind but CLR_EV, env_row0 / env_offset; no CLD_F64_MAPS, CLD_WRITE_DETAIL, no env_pitch.  cl_tuning.vec (1 or 2) /
 * .nw override the geometry, which is otherwise clpol_rollout_mlp_f32's.
 * state / out_bldg / out_env / ret_env / traj: as clpol_rollout_mlp_f32 leaves them.
 * kpi_bldg ([CL_NKB][n_bldg][n_env]) / kpi_env ([CL_NKE][n_env]): the accumulators, read once and written once by the launch.
 * Returns CL_OK or a CL_E* code (message: clpk_last_error); all argument checks happen before the first HIP call. */
int clpk_rollout_mlp_kpi_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpol_mlp* mlp,
                             float* out_bldg, float* out_env, float* ret_env, float* traj, float* kpi_bldg, float* kpi_env,
                             int32_t t0, int32_t k_steps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CITYLEARN_AMD_POLICY_KPI_H */
