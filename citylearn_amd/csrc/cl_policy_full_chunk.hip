// cl_policy_full_chunk.hip -- the translation unit of libcitylearn_amd_policy_full_chunk.so (include/citylearn_amd_policy_full_chunk.h):
// cl_kernels.hip reduced as for cl_policy_full.hip (CL_TU_POLICY, CL_TU_POLICY_FULL) but WITH cl_finish_kernel (CL_TU_FINISH: the fold of the chunk
// partial sums, which a building-chunked launch needs behind it), cl_policy_full.h's kernel template under its CHUNK switch, its
// launcher and the `clpfc_*` entry points.  Compiled WITH SLP vectorisation like
// cl_policy_full.hip.
#define CL_TU_POLICY
#define CL_TU_POLICY_FULL
#define CL_TU_FINISH
#include "cl_kernels.hip"
#include "../../include/citylearn_amd_policy_full_chunk.h"
#include "cl_policy_full.h"

namespace {

// the launcher of this unit; key = 100 * envs per lane + 10 * PREC
int launch_policy_full_chunk(int vec, int prec, dim3 grid, unsigned block, size_t lds, hipStream_t s, const PolicyArgs& p) {
#define CL_POLFC(V, P) CL_POLICY_LAUNCH(cl_rollout_full_policy_kernel<V, P, false, false, true>)
    switch (vec * 100 + prec * 10) {
    case 200: CL_POLFC(2, 0); break;
    case 100: CL_POLFC(1, 0); break;
    case 120: CL_POLFC(1, 2); break;
    default: return (int)hipErrorInvalidValue;
    }
#undef CL_POLFC
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

CL_POLICY_ABI(clpfc, CLPFC_ABI_VERSION)

int clpfc_rollout_mlp_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpf_mlp* mlp,
                          float* out_bldg, float* out_env, float* ret_env, float* traj, int32_t t0, int32_t k_steps, void* stream) {
    const char* const entry = "clpfc_rollout_mlp_f32";
    if (int rc = check_dims(dims, false)) return rc;
    // ---- what the kernel covers ----
    if (dims->flags & CLD_LEAN)
        return fail(CL_EINVAL, "clpfc_rollout_mlp_f32: thermal / outage districts only; a battery + PV district (CLD_LEAN) goes to clpol_rollout_mlp_f32 (libcitylearn_amd_policy.so)");
    if (int rc = no_chunked_marl(dims, entry)) return rc;
    if (int rc = no_reward_ev(dims, entry)) return rc;
    if (int rc = no_f64_maps(dims, entry)) return rc;
    if (dims->flags & CLD_KPI) return fail(CL_EINVAL, "clpfc_rollout_mlp_f32: no streaming KPIs (CLD_KPI) inside a building-chunked policy launch");
    if (int rc = no_detail_planes(dims, entry)) return rc;
    if (int rc = no_pitch(dims, entry)) return rc;
    if (int rc = check_thermal_policy_mlp(entry, dims, mlp)) return rc;
    const PolicyCall call = {params, ts, state, out_bldg, out_env, ret_env, traj, nullptr, nullptr, t0, k_steps};
    if (int rc = check_policy_buffers(dims, *mlp, call, false)) return rc;

    const cl_tuning& tun = dims->tuning ? *dims->tuning : cl_tuning{};
    PolicyArgs p;
    fill_policy_args(p, dims, *mlp, CLPF_NOISE_KEY, call);
    StepArgs& a = p.r.s;
    // ---- the chunk geometry: ONE building per wave, so b_chunk buildings = waves per workgroup row
    const ChunkRule rule = {1, entry, "clpf_rollout_mlp_f32", "libcitylearn_amd_policy_full.so"};
    if (int rc = policy_chunk_geometry(dims, tun, rule, a.b_chunk, a.n_chunks)) return rc;
    if (tun.nw != 0 && tun.nw != a.b_chunk)
        return fail(CL_EINVAL, "bad nw %d: the chunked thermal policy rollout runs one building per wave (nw = b_chunk = %d)", tun.nw, a.b_chunk);
    a.nw = a.b_chunk;
    if (int rc = check_chunk_partials(a.b_chunk, a.n_chunks, dims)) return rc;
    const bool chain = dims->flags & CLD_F64_CHAIN;
    if (tun.vec != 0 && tun.vec != 1 && tun.vec != 2) return fail(CL_EINVAL, "no chunked thermal policy rollout kernel at %d envs per lane", tun.vec);
    if (tun.vec == 2 && chain)
        return fail(CL_EINVAL, "no chunked thermal policy rollout kernel at 2 envs per lane under CLD_F64_CHAIN: it runs at one env per lane");
    const int vec = tun.vec ? tun.vec : chain ? 1 : 2;
    const int tile = 64 * vec;
    const size_t lds = rollout_full_policy_chunk_lds_floats(a.nw, tile) * sizeof(float);
    if (int rc = check_policy_lds(lds, "chunked thermal policy", a.nw, vec)) return rc;
    const int prec = chain ? 2 : 0;
    name_reset(tun);
    name_add(tun, "cl_rollout_full_policy_chunk_kernel<%d, %d>", vec, prec);
    const dim3 grid((unsigned)((dims->n_env + tile - 1) / tile), (unsigned)a.n_chunks);
    const int rc = launch_policy_full_chunk(vec, prec, grid, 64u * a.nw, lds, (hipStream_t)stream, p);
    if (rc) return hip_fail((hipError_t)rc, "cl_rollout_full_policy_chunk_kernel launch");
    // the last step's district sums (and the K-step return): one fold per launch, as behind a chunked cl_rollout_f32
    if (k_steps > 0) return launch_rollout_finish(tun, a, t0 + k_steps - 1, ret_env, (hipStream_t)stream);
    return CL_OK;
}

}  // extern "C"
