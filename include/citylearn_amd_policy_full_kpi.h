/* citylearn_amd_policy_full_kpi.h -- C interface of libcitylearn_amd_policy_full_kpi.so: the closed-loop policy rollout of a THERMAL district
 * (citylearn_amd_policy_full.h) that also keeps the streaming KPI accumulators of a CLD_KPI district inside the launch
 * (csrc/cl_policy_full.h, its KPI switch).
 *
 * A library of its own beside libcitylearn_amd.so and the three other policy libraries, whose symbol lists, structs and kernels it leaves
 * untouched; it shares cl_dims / cl_tuning, the plane layouts and the error codes with citylearn_amd.h and `clpf_mlp`, the trajectory planes and
 * CLPF_NOISE_KEY with citylearn_amd_policy_full.h.  Every name it exports starts with `clpfk_`.  Like the others it holds no mutable state besides
 * the thread-local error string.
 *
 * A step is clpf_rollout_mlp_f32's step (same policy, same noise stream, same unit), and the accumulators are the ones cl_step_f32 keeps for a
 * thermal CLD_KPI district, in kpi_bldg / kpi_env's layout (CLK_*, CLKE_*) and arithmetic, every env with its own baseline: after the call, the KPI
 * planes are what K calls of cl_step_f32 with the recorded actions would have left.
 */
#ifndef CITYLEARN_AMD_POLICY_FULL_KPI_H
#define CITYLEARN_AMD_POLICY_FULL_KPI_H

#include "citylearn_amd_policy_full.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLPFK_ABI_VERSION 1

int clpfk_abi_version(void);          /* CLPFK_ABI_VERSION of the build */
int clpfk_core_abi_version(void);     /* the CL_ABI_VERSION of citylearn_amd.h it was built against */
const char* clpfk_last_error(void);

/* K steps t0 .. t0 + k_steps - 1 in ONE launch of cl_rollout_full_policy_kpi_kernel<PREC, MARL> (reported through cl_tuning.kernel_name).
 * dims: as clpf_rollout_mlp_f32 takes them, but CLD_KPI is REQUIRED: districts WITHOUT CLD_LEAN of up to 16 buildings with storage action columns
 * only, the fp32 battery map or CLD_F64_CHAIN, every reward kind but CLR_EV, env_row0 / env_offset; no CLD_F64_MAPS, no env_pitch.
 * CLD_WRITE_DETAIL only together with CLD_DETAIL_MIN: the launch then leaves the last step's CLO_COOL_DEM / _HEAT_DEM / _BASE_NET / _EXPECTED /
 * _SERVED planes in out_bldg.  One env per lane always (cl_tuning.vec: 0 or 1), cl_tuning.nw = n_bldg.
 * state / out_bldg / out_env / ret_env / traj: as clpf_rollout_mlp_f32 leaves them.
 * kpi_bldg ([CL_NKB][n_bldg][n_env]) / kpi_env ([CL_NKE][n_env]): the accumulators, read once and written once by the launch
 * (CLK_UNSERVED_OUTAGE / CLK_EXPECTED_OUTAGE are written only if one of the K rows is an outage row).
 * Returns CL_OK or a CL_E* code (message: clpfk_last_error); all argument checks happen before the first HIP call. */
int clpfk_rollout_mlp_kpi_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpf_mlp* mlp,
                              float* out_bldg, float* out_env, float* ret_env, float* traj, float* kpi_bldg, float* kpi_env,
                              int32_t t0, int32_t k_steps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CITYLEARN_AMD_POLICY_FULL_KPI_H */
