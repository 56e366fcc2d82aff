/* citylearn_amd_policy_chunk.h -- C interface of libcitylearn_amd_policy_chunk.so: the closed-loop policy rollout of a battery + PV district
 * (citylearn_amd_policy.h) of MORE THAN 32 buildings, as a building-chunked launch (csrc/cl_policy_chunk.h) -- BASELINE config 4's 1024-building
 * district with a controller in the loop.
 *
 * A library of its own beside libcitylearn_amd.so and the other policy libraries, whose symbol lists, structs and kernels it leaves untouched; it
 * shares cl_dims / cl_tuning, the plane layouts and the error codes with citylearn_amd.h and `clpol_mlp`, the trajectory planes and
 * CLPOL_NOISE_KEY with citylearn_amd_policy.h.  Every name it exports starts with `clpc_`.  Like the others it holds no mutable state besides the
 * thread-local error string.
 *
 * A step is clpol_rollout_mlp_f32's step (same policy, same noise stream -- keyed by global env, action column and step, so the chunk geometry
 * does not change a draw -- same unit).  The buildings are cut into n_chunks chunks of b_chunk <= 32 along gridDim.y, two buildings per wave
 * (wave w of a chunk owns its buildings w and w + nw); the last step's district sums and the K-step return are added over the chunks by one
 * cl_finish_kernel launch behind the rollout kernel, through the scratch rows of out_bldg's reserved plane (CLO_RESERVED) exactly as the chunked
 * cl_rollout_f32 uses them: the plane's marker and ticket words stay usable for the step launches that follow.
 */
#ifndef CITYLEARN_AMD_POLICY_CHUNK_H
#define CITYLEARN_AMD_POLICY_CHUNK_H

#include "citylearn_amd_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLPC_ABI_VERSION 1

int clpc_abi_version(void);           /* CLPC_ABI_VERSION of the build */
int clpc_core_abi_version(void);      /* the CL_ABI_VERSION of citylearn_amd.h it was built against */
const char* clpc_last_error(void);

/* K steps t0 .. t0 + k_steps - 1 in ONE launch of cl_rollout_policy_chunk_kernel<envs per lane, PREC> followed, if k_steps > 0, by one
 * cl_finish_kernel launch (both reported through cl_tuning.kernel_name).
 * dims: as clpol_rollout_mlp_f32 takes them -- CLD_LEAN districts, the fp32 battery map or CLD_F64_CHAIN, env_row0 / env_offset; no CLD_F64_MAPS,
 * CLD_KPI, CLD_WRITE_DETAIL, no env_pitch -- but of MORE buildings than one workgroup row holds, and without CLR_MARL and CLR_EV: a
 * building-chunked launch cannot couple the buildings inside a step.
 * cl_tuning.b_chunk: buildings per workgroup row, at most 32 and less than n_bldg; 0 = the blind chunked rollout's 32-building workgroups,
 * balanced: n_chunks = ceil(n_bldg / 32), b_chunk = ceil(n_bldg / n_chunks) (33 -> 17 + 16, 40 -> 20 + 20, 1024 -> 32 x 32), which needs
 * n_bldg > 32: a district that fits one workgroup row is clpol_rollout_mlp_f32's.  cl_tuning.nw: waves per workgroup, 0 = ceil(b_chunk / 2);
 * 2 nw >= b_chunk, nw <= 16, nw <= b_chunk (b_chunk = nw = 16: one building per wave).  cl_tuning.vec: 1 or 2 envs per lane; 0 = 2 where the
 * 128-env workgroups come in full rounds over env tiles x n_chunks, n_env >= 128 and n_env x n_chunks >= 32768, else 1.
 * The reserved plane must hold n_chunks x (NQ + 1) rows of n_env floats in front of its ticket and marker words.
 * state / out_bldg / out_env / traj: as clpol_rollout_mlp_f32 leaves them.  ret_env (nullable [n_env]) += the district reward summed over the K
 * steps.  Returns CL_OK or a CL_E* code (message: clpc_last_error); all argument checks happen before the first HIP call. */
int clpc_rollout_mlp_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpol_mlp* mlp,
                         float* out_bldg, float* out_env, float* ret_env, float* traj, int32_t t0, int32_t k_steps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CITYLEARN_AMD_POLICY_CHUNK_H */
