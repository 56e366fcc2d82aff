/* citylearn_amd_policy_full_chunk.h -- C interface of libcitylearn_amd_policy_full_chunk.so: the closed-loop policy rollout of a THERMAL district
 * (citylearn_amd_policy_full.h) of MORE THAN 16 buildings, as a building-chunked launch (csrc/cl_policy_full.h, its CHUNK switch) -- BASELINE config 4's
 * 1024-building district with a controller in the loop.
 *
 * A library of its own beside libcitylearn_amd.so and the four other policy libraries, whose symbol lists, structs and kernels it leaves
 * untouched; it shares cl_dims / cl_tuning, the plane layouts and the error codes with citylearn_amd.h and `clpf_mlp`, the trajectory planes and
 * CLPF_NOISE_KEY with citylearn_amd_policy_full.h.  Every name it exports starts with `clpfc_`.  Like the others it holds no mutable state besides
 * the thread-local error string.
 *
 * A step is clpf_rollout_mlp_f32's step (same policy, same noise stream -- keyed by global env, action column and step, so the chunk geometry
 * does not change a draw -- same unit).  The buildings are cut into n_chunks chunks of b_chunk <= 16 along gridDim.y, one building per wave; the
 * last step's district sums and the K-step return are added over the chunks by one cl_finish_kernel launch behind the rollout kernel, through the
 * scratch rows of out_bldg's reserved plane (CLO_RESERVED) exactly as the chunked cl_rollout_f32 uses them: the plane's marker and ticket words
 * stay usable for the step launches that follow.
 */
#ifndef CITYLEARN_AMD_POLICY_FULL_CHUNK_H
#define CITYLEARN_AMD_POLICY_FULL_CHUNK_H

#include "citylearn_amd_policy_full.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLPFC_ABI_VERSION 1

int clpfc_abi_version(void);          /* CLPFC_ABI_VERSION of the build */
int clpfc_core_abi_version(void);     /* the CL_ABI_VERSION of citylearn_amd.h it was built against */
const char* clpfc_last_error(void);

/* K steps t0 .. t0 + k_steps - 1 in ONE launch of cl_rollout_full_policy_chunk_kernel<envs per lane, PREC> followed by one cl_finish_kernel launch
 * (both reported through cl_tuning.kernel_name).
 * dims: as clpf_rollout_mlp_f32 takes them -- districts WITHOUT CLD_LEAN with storage action columns only, the fp32 battery map or CLD_F64_CHAIN
 * (one env per lane), env_row0 / env_offset; no CLD_F64_MAPS, CLD_KPI, CLD_WRITE_DETAIL, no env_pitch -- but of MORE buildings than one workgroup
 * row holds, and without CLR_MARL and CLR_EV: a building-chunked launch cannot couple the buildings inside a step.
 * cl_tuning.b_chunk: buildings per workgroup row, at most 16 and less than n_bldg; 0 = balanced chunks of at most eight,
 * n_chunks = ceil(n_bldg / 8), b_chunk = ceil(n_bldg / n_chunks) (17 -> 6 + 6 + 5, 1024 -> 128 x 8), which needs n_bldg > 16: a district that fits
 * one workgroup row is clpf_rollout_mlp_f32's.  cl_tuning.nw: 0 or b_chunk.  cl_tuning.vec: 1 or 2 (2 only on the fp32 map).
 * The reserved plane must hold n_chunks x (NQ + 1) rows of n_env floats in front of its ticket and marker words.
 * state / out_bldg / out_env / traj: as clpf_rollout_mlp_f32 leaves them.  ret_env (nullable [n_env]) += the district reward summed over the K
 * steps.  Returns CL_OK or a CL_E* code (message: clpfc_last_error); all argument checks happen before the first HIP call. */
int clpfc_rollout_mlp_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpf_mlp* mlp,
                          float* out_bldg, float* out_env, float* ret_env, float* traj, int32_t t0, int32_t k_steps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CITYLEARN_AMD_POLICY_FULL_CHUNK_H */
