// cl_policy.hip -- the translation unit of libcitylearn_amd_policy.so (include/citylearn_amd_policy.h): cl_kernels.hip reduced to the helpers the
// fused rollout kernels share (CL_TU_NOSLP's cut, minus its launchers: CL_TU_POLICY) + cl_policy.h's closed-loop kernel at KPI = false, its launcher and the
// `clpol_*` entry points.  Compiled with -fno-slp-vectorize like the other rollout kernels (citylearn_amd/_lib.py): same arithmetic, same loss to
// packed fp32.
#define CL_TU_NOSLP
#define CL_TU_POLICY
#include "cl_kernels.hip"
#include "../../include/citylearn_amd_policy.h"
#include "cl_policy.h"

namespace {

// the launcher of this unit (the main library's cl_tu_launch_* stay what they are); key = 10 * envs per lane + PREC
int launch_policy(int vec, int prec, unsigned grid, unsigned block, size_t lds, hipStream_t s, const PolicyArgs& p) {
#define CL_POL(V, P) CL_POLICY_LAUNCH(cl_rollout_policy_kernel<V, P, false, false>)
    switch (vec * 10 + prec) {
    case 10: CL_POL(1, 0); break;
    case 20: CL_POL(2, 0); break;
    case 12: CL_POL(1, 2); break;
    case 22: CL_POL(2, 2); break;
    default: return (int)hipErrorInvalidValue;
    }
#undef CL_POL
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

CL_POLICY_ABI(clpol, CLPOL_ABI_VERSION)

int clpol_rollout_mlp_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpol_mlp* mlp,
                          float* out_bldg, float* out_env, float* ret_env, float* traj, int32_t t0, int32_t k_steps, void* stream) {
    const char* const entry = "clpol_rollout_mlp_f32";
    if (int rc = check_dims(dims, false)) return rc;
    // ---- what the kernel covers ----
    if (!(dims->flags & CLD_LEAN))
        return fail(CL_EINVAL, "clpol_rollout_mlp_f32: only battery + PV districts (CLD_LEAN); a thermal / outage district has no closed-loop rollout kernel");
    if (dims->n_bldg > 32)
        return fail(CL_EINVAL, "clpol_rollout_mlp_f32: n_bldg=%d > 32 would be a building-chunked launch, which the policy kernel is not: "
                               "clpc_rollout_mlp_f32 (libcitylearn_amd_policy_chunk.so)", dims->n_bldg);
    if (int rc = no_f64_maps(dims, entry)) return rc;
    if (dims->flags & CLD_KPI)
        return fail(CL_EINVAL, "clpol_rollout_mlp_f32: no streaming KPIs (CLD_KPI) inside this kernel -- record traj and replay CLPOL_T_ACTION through cl_rollout_seq_f32");
    if (int rc = no_detail_planes(dims, entry)) return rc;
    if (int rc = no_reward_ev(dims, entry)) return rc;
    if (int rc = no_pitch(dims, entry)) return rc;
    if (int rc = check_lean_policy_mlp(mlp)) return rc;
    const PolicyCall call = {params, ts, state, out_bldg, out_env, ret_env, traj, nullptr, nullptr, t0, k_steps};
    if (int rc = check_policy_buffers(dims, *mlp, call, false)) return rc;

    const cl_tuning& tun = dims->tuning ? *dims->tuning : cl_tuning{};
    PolicyArgs p;
    fill_policy_args(p, dims, *mlp, CLPOL_NOISE_KEY, call);
    int vec;
    if (int rc = lean_policy_geometry(dims, tun, "policy", p.r.s.nw, vec)) return rc;
    const int nw = p.r.s.nw, tile = 64 * vec;
    const size_t lds = rollout_policy_lds_floats(nw, tile) * sizeof(float);
    if (int rc = check_policy_lds(lds, "policy", nw, vec)) return rc;
    const int prec = (dims->flags & CLD_F64_CHAIN) ? 2 : 0;
    name_reset(tun);
    name_add(tun, "cl_rollout_policy_kernel<%d, %d>", vec, prec);
    const int rc = launch_policy(vec, prec, (unsigned)((dims->n_env + tile - 1) / tile), 64u * nw, lds, (hipStream_t)stream, p);
    if (rc) return hip_fail((hipError_t)rc, "cl_rollout_policy_kernel launch");
    return CL_OK;
}

}  // extern "C"
