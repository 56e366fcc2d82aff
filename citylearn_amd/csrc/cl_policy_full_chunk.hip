// cl_policy_full_chunk.hip -- the translation unit of libcitylearn_amd_policy_full_chunk.so (include/citylearn_amd_policy_full_chunk.h):
// cl_kernels.hip reduced as for cl_policy_full.hip (CL_TU_POLICY, CL_TU_POLICY_FULL) but WITH cl_finish_kernel (CL_TU_FINISH: the fold of the chunk
// partial sums, which a building-chunked launch needs behind it), cl_policy_full.h for the staged-row layout (its kernel template is never
// instantiated here), cl_policy_full_chunk.h's kernel, its launcher and the `clpfc_*` entry points.  Compiled WITH SLP vectorisation like
// cl_policy_full.hip.
#define CL_TU_POLICY
#define CL_TU_POLICY_FULL
#define CL_TU_FINISH
#include "cl_kernels.hip"
#include "../../include/citylearn_amd_policy_full_chunk.h"
#include "cl_policy_full_chunk.h"

namespace {

// the launcher of this unit; key = 100 * envs per lane + 10 * PREC
int launch_policy_full_chunk(int vec, int prec, dim3 grid, unsigned block, size_t lds, hipStream_t s, const PolicyArgs& p) {
#define CL_POLFC(V, P) CL_POLICY_LAUNCH(cl_rollout_full_policy_chunk_kernel<V, P>)
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

int clpfc_abi_version(void) { return CLPFC_ABI_VERSION; }
int clpfc_core_abi_version(void) { return CL_ABI_VERSION; }
const char* clpfc_last_error(void) { return g_err; }

int clpfc_rollout_mlp_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpf_mlp* mlp,
                          float* out_bldg, float* out_env, float* ret_env, float* traj, int32_t t0, int32_t k_steps, void* stream) {
    if (int rc = check_dims(dims, false)) return rc;
    const uint32_t rk = (dims->flags & CLD_REWARD_MASK) >> CLD_REWARD_SHIFT;
    // ---- what the kernel covers ----
    if (dims->flags & CLD_LEAN)
        return fail(CL_EINVAL, "clpfc_rollout_mlp_f32: thermal / outage districts only; a battery + PV district (CLD_LEAN) goes to clpol_rollout_mlp_f32 (libcitylearn_amd_policy.so)");
    if (rk == CLR_MARL)
        return fail(CL_EINVAL, "clpfc_rollout_mlp_f32: reward kind CLR_MARL: a building-chunked launch cannot couple the buildings inside a step");
    if (rk == CLR_EV) return fail(CL_EINVAL, "clpfc_rollout_mlp_f32: reward kind CLR_EV needs the flexible-load tables");
    if (dims->flags & CLD_F64_MAPS)
        return fail(CL_EINVAL, "clpfc_rollout_mlp_f32: the battery map in fp32 or as the float64 chain (CLD_F64_CHAIN), not CLD_F64_MAPS");
    if (dims->flags & CLD_KPI) return fail(CL_EINVAL, "clpfc_rollout_mlp_f32: no streaming KPIs (CLD_KPI) inside a building-chunked policy launch");
    if (dims->flags & CLD_WRITE_DETAIL) return fail(CL_EINVAL, "clpfc_rollout_mlp_f32: not with the detail planes (CLD_WRITE_DETAIL)");
    if (int rc = no_pitch(dims, "clpfc_rollout_mlp_f32")) return rc;
    if (dims->n_act_cols > 65536) return fail(CL_EINVAL, "clpfc_rollout_mlp_f32: n_act_cols=%d > 65536", dims->n_act_cols);
    if (!mlp) return fail(CL_ENULL, "mlp is NULL");
    if (mlp->n_device_cols != 0)
        return fail(CL_EINVAL, "clpfc_rollout_mlp_f32: n_device_cols=%d: a building with a cooling / heating / combined device action column is not covered "
                               "(the policy has storage heads only)", mlp->n_device_cols);
    if (int rc = check_policy_sizes(*mlp, CLPF_MAX_HIDDEN)) return rc;
    if (mlp->reserved) return fail(CL_EINVAL, "clpf_mlp.reserved must be 0");
    const PolicyCall call = {params, ts, state, out_bldg, out_env, ret_env, traj, nullptr, nullptr, t0, k_steps};
    if (int rc = check_policy_buffers(dims, *mlp, call, false)) return rc;

    const cl_tuning& tun = dims->tuning ? *dims->tuning : cl_tuning{};
    PolicyArgs p;
    fill_policy_args(p, dims, *mlp, CLPF_NOISE_KEY, call);
    StepArgs& a = p.r.s;
    // ---- the chunk geometry: ONE building per wave, b_chunk buildings = waves per workgroup row, n_chunks rows along gridDim.y.  Default: balanced
    // chunks of at most EIGHT (what the blind packed kernel runs its chunked launches at: two or three workgroups per CU instead of one of sixteen waves)
    if (tun.b_chunk < 0) return fail(CL_EINVAL, "b_chunk=%d", tun.b_chunk);
    if (tun.b_chunk > 16) return fail(CL_EINVAL, "b_chunk=%d: a thermal policy rollout workgroup holds at most 16 buildings (one per wave)", tun.b_chunk);
    if (tun.b_chunk == 0 && dims->n_bldg <= 16)
        return fail(CL_EINVAL, "clpfc_rollout_mlp_f32: n_bldg=%d fits one workgroup row, which is clpf_rollout_mlp_f32's launch (libcitylearn_amd_policy_full.so); "
                               "a chunked launch of it takes an explicit cl_tuning.b_chunk < n_bldg", dims->n_bldg);
    if (tun.b_chunk >= dims->n_bldg)
        return fail(CL_EINVAL, "b_chunk=%d >= n_bldg=%d: one workgroup row is clpf_rollout_mlp_f32's launch (libcitylearn_amd_policy_full.so)", tun.b_chunk, dims->n_bldg);
    if (tun.b_chunk > 0) {
        a.b_chunk = tun.b_chunk;
    } else {
        const int nc = (dims->n_bldg + 7) / 8;
        a.b_chunk = (dims->n_bldg + nc - 1) / nc;
    }
    a.n_chunks = (dims->n_bldg + a.b_chunk - 1) / a.b_chunk;
    if (tun.nw != 0 && tun.nw != a.b_chunk)
        return fail(CL_EINVAL, "bad nw %d: the chunked thermal policy rollout runs one building per wave (nw = b_chunk = %d)", tun.nw, a.b_chunk);
    a.nw = a.b_chunk;
    // the reserved plane holds n_chunks x NQ partial sums, one return row per chunk and, at its tail, the ticket and marker words of the step launches
    if (((long long)a.n_chunks * (NQ + 1)) * dims->n_env + (dims->n_env + 63) / 64 + 4 > (long long)dims->n_bldg * dims->n_env)
        return fail(CL_EINVAL, "b_chunk=%d leaves no room for the %d chunk partial sums of the fused rollout", a.b_chunk, a.n_chunks);
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
    if (k_steps > 0) {
        // the last step's district sums (and the K-step return): one fold per launch, as behind a chunked cl_rollout_f32
        StepArgs f = a;
        f.t = t0 + k_steps - 1;
        name_add(tun, "cl_finish_kernel");
        hipLaunchKernelGGL(cl_finish_kernel, dim3((dims->n_env + 63) / 64, NQ + (ret_env ? 1 : 0)), dim3(1024), 0, (hipStream_t)stream, f, 0, ret_env);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_fail(e, "cl_finish_kernel launch");
    }
    return CL_OK;
}

}  // extern "C"
