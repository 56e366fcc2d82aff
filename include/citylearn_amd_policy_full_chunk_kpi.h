/* citylearn_amd_policy_full_chunk_kpi.h -- C interface of libcitylearn_amd_policy_full_chunk_kpi.so: the building-chunked closed-loop policy rollout
 * of a THERMAL district of MORE THAN 16 buildings (citylearn_amd_policy_full_chunk.h) that also keeps the streaming KPI accumulators of a CLD_KPI
 * district inside the call (csrc/cl_policy_full.h, its KPI and CHUNK switches; csrc/cl_policy_full_chunk_kpi.h) -- BASELINE config 4's 1024-building district scored by CityLearn's KPIs without a
 * record, a second env or a replay.
 *
 * A library of its own beside libcitylearn_amd.so and the five other policy libraries, whose symbol lists, structs and kernels it leaves
 * untouched; it shares cl_dims / cl_tuning, the plane layouts and the error codes with citylearn_amd.h and `clpf_mlp`, the trajectory planes and
 * CLPF_NOISE_KEY with citylearn_amd_policy_full.h.  Every name it exports starts with `clpfck_`.  Like the others it holds no mutable state besides
 * the thread-local error string.
 *
 * A step is clpfc_rollout_mlp_f32's step (same policy, same noise stream, same chunk geometry), and the accumulators are the ones cl_step_f32
 * keeps for a thermal CLD_KPI district, in kpi_bldg / kpi_env's layout (CLK_*, CLKE_*), every env with its own baseline.  The per-building sums
 * keep the single-step path's arithmetic and order; a sample of a district series is the sum of the chunks' partial sums (sixteen strided partial
 * sums over the chunks, then their sum in order), an association that depends on (n_bldg, b_chunk) only: cutting K steps into several calls, at
 * any boundaries, leaves every KPI plane bit for bit what one call leaves.
 */
#ifndef CITYLEARN_AMD_POLICY_FULL_CHUNK_KPI_H
#define CITYLEARN_AMD_POLICY_FULL_CHUNK_KPI_H

#include "citylearn_amd_policy_full.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLPFCK_ABI_VERSION 1

int clpfck_abi_version(void);         /* CLPFCK_ABI_VERSION of the build */
int clpfck_core_abi_version(void);    /* the CL_ABI_VERSION of citylearn_amd.h it was built against */
const char* clpfck_last_error(void);

/* The floats of `series_scratch` a call of clpfck_rollout_mlp_kpi_f32 with these dims (n_env, n_bldg, cl_tuning.b_chunk) and k_steps needs:
 * k_steps x 2 x n_chunks x n_env, n_chunks of the geometry the call would choose.  < 0: a CL_E* code negated (dims NULL, a chunk geometry the
 * call refuses, k_steps < 0), message in clpfck_last_error. */
int64_t clpfck_series_scratch_floats(const cl_dims* dims, int32_t k_steps);

/* K steps t0 .. t0 + k_steps - 1 in THREE launches (reported through cl_tuning.kernel_name): cl_rollout_full_policy_chunk_kpi_kernel<PREC>,
 * cl_kpi_series_chunk_kernel, cl_finish_kernel.
 * dims: as clpfc_rollout_mlp_f32 takes them (chunk geometry, reserved plane, no CLD_LEAN / CLR_MARL / CLR_EV / CLD_F64_MAPS / env_pitch / device
 * action columns), but CLD_KPI is REQUIRED and CLD_WRITE_DETAIL is accepted together with CLD_DETAIL_MIN: the call then leaves the last step's
 * CLO_COOL_DEM / _HEAT_DEM / _BASE_NET / _EXPECTED / _SERVED planes in out_bldg.  One env per lane always (cl_tuning.vec: 0 or 1).
 * state / out_bldg / out_env / ret_env / traj: as clpfc_rollout_mlp_f32 leaves them.
 * kpi_bldg ([CL_NKB][n_bldg][n_env]) / kpi_env ([CL_NKE][n_env]): the accumulators, read once and written once by the call
 * (CLK_UNSERVED_OUTAGE / CLK_EXPECTED_OUTAGE of a building are written only if one of the K rows is an outage row of it).
 * series_scratch ([k_steps][2][n_chunks][n_env] floats, 16-byte aligned, scratch_floats >= clpfck_series_scratch_floats(dims, k_steps)): the
 * chunks' partial samples of the two district series on their way from the first launch to the second; its contents mean nothing afterwards.
 * A caller bounds it by cutting K steps into calls of a window of steps each (t0 and traj advancing, ret_env accumulating).
 * Returns CL_OK or a CL_E* code (message: clpfck_last_error); all argument checks happen before the first HIP call. */
int clpfck_rollout_mlp_kpi_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpf_mlp* mlp,
                               float* out_bldg, float* out_env, float* ret_env, float* traj, float* kpi_bldg, float* kpi_env,
                               float* series_scratch, int64_t scratch_floats, int32_t t0, int32_t k_steps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CITYLEARN_AMD_POLICY_FULL_CHUNK_KPI_H */
