// cl_policy_chunk.hip -- the translation unit of libcitylearn_amd_policy_chunk.so (include/citylearn_amd_policy_chunk.h): cl_kernels.hip reduced as
// for cl_policy.hip (CL_TU_NOSLP, CL_TU_POLICY) but WITH cl_finish_kernel (CL_TU_FINISH: the fold of the chunk partial sums, which a
// building-chunked launch needs behind it), cl_policy.h's closed-loop kernel at CHUNK = true (cl_policy_chunk.h says what that switches; reported
// as cl_rollout_policy_chunk_kernel<VEC, PREC>; no other variant is instantiated here), its launcher and the `clpc_*` entry points.  Compiled with -fno-slp-vectorize like cl_policy.hip.
#define CL_TU_NOSLP
#define CL_TU_POLICY
#define CL_TU_FINISH
#include "cl_kernels.hip"
#include "../../include/citylearn_amd_policy_chunk.h"
#include "cl_policy_chunk.h"

namespace {

// the launcher of this unit; key = 10 * envs per lane + PREC
int launch_policy_chunk(int vec, int prec, dim3 grid, unsigned block, size_t lds, hipStream_t s, const PolicyArgs& p) {
#define CL_POLC(V, P) CL_POLICY_LAUNCH(cl_rollout_policy_kernel<V, P, false, true>)
    switch (vec * 10 + prec) {
    case 10: CL_POLC(1, 0); break;
    case 20: CL_POLC(2, 0); break;
    case 12: CL_POLC(1, 2); break;
    case 22: CL_POLC(2, 2); break;
    default: return (int)hipErrorInvalidValue;
    }
#undef CL_POLC
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

CL_POLICY_ABI(clpc, CLPC_ABI_VERSION)

int clpc_rollout_mlp_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpol_mlp* mlp,
                         float* out_bldg, float* out_env, float* ret_env, float* traj, int32_t t0, int32_t k_steps, void* stream) {
    const char* const entry = "clpc_rollout_mlp_f32";
    if (int rc = check_dims(dims, false)) return rc;
    // ---- what the kernel covers ----
    if (!(dims->flags & CLD_LEAN))
        return fail(CL_EINVAL, "clpc_rollout_mlp_f32: only battery + PV districts (CLD_LEAN); a thermal / outage district of more than one workgroup row goes to "
                               "clpfc_rollout_mlp_f32 (libcitylearn_amd_policy_full_chunk.so)");
    if (int rc = no_chunked_marl(dims, entry)) return rc;
    if (int rc = no_reward_ev(dims, entry)) return rc;
    if (int rc = no_f64_maps(dims, entry)) return rc;
    if (dims->flags & CLD_KPI) return fail(CL_EINVAL, "clpc_rollout_mlp_f32: no streaming KPIs (CLD_KPI) inside a building-chunked policy launch");
    if (int rc = no_detail_planes(dims, entry)) return rc;
    if (int rc = no_pitch(dims, entry)) return rc;
    if (int rc = check_lean_policy_mlp(mlp)) return rc;
    const PolicyCall call = {params, ts, state, out_bldg, out_env, ret_env, traj, nullptr, nullptr, t0, k_steps};
    if (int rc = check_policy_buffers(dims, *mlp, call, false)) return rc;

    const cl_tuning& tun = dims->tuning ? *dims->tuning : cl_tuning{};
    PolicyArgs p;
    fill_policy_args(p, dims, *mlp, CLPOL_NOISE_KEY, call);
    StepArgs& a = p.r.s;
    // ---- the chunk geometry: TWO buildings per wave
    const ChunkRule rule = {2, entry, "clpol_rollout_mlp_f32", "libcitylearn_amd_policy.so"};
    if (int rc = policy_chunk_geometry(dims, tun, rule, a.b_chunk, a.n_chunks)) return rc;
    a.nw = tun.nw ? tun.nw : (a.b_chunk + 1) / 2;
    // (nw > b_chunk: waves that no chunk ever fills)
    if (a.nw * 2 < a.b_chunk || a.nw < 1 || a.nw > 16 || a.nw > a.b_chunk)
        return fail(CL_EINVAL, "bad nw %d: the chunked policy rollout runs two buildings per wave (b_chunk = %d: nw in %d..%d)", a.nw, a.b_chunk,
                    (a.b_chunk + 1) / 2, a.b_chunk < 16 ? a.b_chunk : 16);
    // envs per lane: the blind chunked rollout's rule (cl_rollout_f32) -- two where the 128-env workgroups come in (nearly) full rounds of one per
    // CU over env tiles x chunks; under the float64 chain too (the blind chunked lean kernel keeps the two-env pack there)
    if (tun.vec != 0 && tun.vec != 1 && tun.vec != 2) return fail(CL_EINVAL, "no chunked policy rollout kernel at %d envs per lane", tun.vec);
    const int vec = tun.vec ? tun.vec : (full_rounds(dims->n_env, a.n_chunks) ? 2 : 1);
    if (int rc = check_chunk_partials(a.b_chunk, a.n_chunks, dims)) return rc;
    const int tile = 64 * vec;
    const size_t lds = rollout_policy_chunk_lds_floats(a.nw, tile) * sizeof(float);
    if (int rc = check_policy_lds(lds, "chunked policy", a.nw, vec)) return rc;
    const int prec = (dims->flags & CLD_F64_CHAIN) ? 2 : 0;
    name_reset(tun);
    name_add(tun, "cl_rollout_policy_chunk_kernel<%d, %d>", vec, prec);
    const dim3 grid((unsigned)((dims->n_env + tile - 1) / tile), (unsigned)a.n_chunks);
    const int rc = launch_policy_chunk(vec, prec, grid, 64u * a.nw, lds, (hipStream_t)stream, p);
    if (rc) return hip_fail((hipError_t)rc, "cl_rollout_policy_chunk_kernel launch");
    // the last step's district sums (and the K-step return): one fold per launch, as behind a chunked cl_rollout_f32
    if (k_steps > 0) return launch_rollout_finish(tun, a, t0 + k_steps - 1, ret_env, (hipStream_t)stream);
    return CL_OK;
}

}  // extern "C"
