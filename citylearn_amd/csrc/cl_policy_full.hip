// cl_policy_full.hip -- the translation unit of libcitylearn_amd_policy_full.so (include/citylearn_amd_policy_full.h): cl_kernels.hip reduced to the
// helpers the fused rollout kernels share and the packed thermal unit of cl_full.h (CL_TU_POLICY cuts the launchers and entry points,
// CL_TU_POLICY_FULL the main library's small passes) + cl_policy_full.h's closed-loop kernel template without its KPI and CHUNK switches, its launcher and the `clpf_*` entry points.  NOT under
// CL_TU_NOSLP and compiled WITH SLP vectorisation, like the main translation unit: the packed unit wants v_pk_*_f32.
#define CL_TU_POLICY
#define CL_TU_POLICY_FULL
#include "cl_kernels.hip"
#include "../../include/citylearn_amd_policy_full.h"
#include "cl_policy_full.h"

namespace {

// the launcher of this unit; key = 100 * envs per lane + 10 * PREC + MARL
int launch_policy_full(int vec, int prec, bool marl, unsigned grid, unsigned block, size_t lds, hipStream_t s, const PolicyArgs& p) {
#define CL_POLF(V, P, M) CL_POLICY_LAUNCH(cl_rollout_full_policy_kernel<V, P, M, false, false>)
    switch (vec * 100 + prec * 10 + (marl ? 1 : 0)) {
    case 200: CL_POLF(2, 0, false); break;
    case 100: CL_POLF(1, 0, false); break;
    case 101: CL_POLF(1, 0, true); break;
    case 120: CL_POLF(1, 2, false); break;
    case 121: CL_POLF(1, 2, true); break;
    default: return (int)hipErrorInvalidValue;
    }
#undef CL_POLF
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

CL_POLICY_ABI(clpf, CLPF_ABI_VERSION)

int clpf_rollout_mlp_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpf_mlp* mlp,
                         float* out_bldg, float* out_env, float* ret_env, float* traj, int32_t t0, int32_t k_steps, void* stream) {
    const char* const entry = "clpf_rollout_mlp_f32";
    if (int rc = check_dims(dims, false)) return rc;
    // ---- what the kernel covers ----
    if (dims->flags & CLD_LEAN)
        return fail(CL_EINVAL, "clpf_rollout_mlp_f32: thermal / outage districts only; a battery + PV district (CLD_LEAN) goes to clpol_rollout_mlp_f32 (libcitylearn_amd_policy.so)");
    if (dims->n_bldg > 16)
        return fail(CL_EINVAL, "clpf_rollout_mlp_f32: n_bldg=%d > 16 would be a building-chunked launch, which the policy kernel is not", dims->n_bldg);
    if (int rc = no_f64_maps(dims, entry)) return rc;
    if (dims->flags & CLD_KPI) return fail(CL_EINVAL, "clpf_rollout_mlp_f32: no streaming KPIs (CLD_KPI) inside this kernel");
    if (int rc = no_detail_planes(dims, entry)) return rc;
    if (int rc = no_reward_ev(dims, entry)) return rc;
    if (int rc = no_pitch(dims, entry)) return rc;
    if (int rc = check_thermal_policy_mlp(entry, dims, mlp)) return rc;
    const PolicyCall call = {params, ts, state, out_bldg, out_env, ret_env, traj, nullptr, nullptr, t0, k_steps};
    if (int rc = check_policy_buffers(dims, *mlp, call, false)) return rc;

    const cl_tuning& tun = dims->tuning ? *dims->tuning : cl_tuning{};
    PolicyArgs p;
    fill_policy_args(p, dims, *mlp, CLPF_NOISE_KEY, call);
    StepArgs& a = p.r.s;
    if (int rc = thermal_one_row_geometry(dims, tun, "thermal policy", a.nw)) return rc;
    const bool chain = dims->flags & CLD_F64_CHAIN, marl = reward_kind(dims) == CLR_MARL;
    if (tun.vec != 0 && tun.vec != 1 && tun.vec != 2) return fail(CL_EINVAL, "no thermal policy rollout kernel at %d envs per lane", tun.vec);
    if (tun.vec == 2 && (chain || marl))
        return fail(CL_EINVAL, "no thermal policy rollout kernel at 2 envs per lane under %s: it runs at one env per lane", chain ? "CLD_F64_CHAIN" : "CLR_MARL");
    const int vec = tun.vec ? tun.vec : (chain || marl) ? 1 : 2;
    const int tile = 64 * vec;
    const size_t lds = rollout_full_policy_lds_floats(a.nw, tile) * sizeof(float);
    if (int rc = check_policy_lds(lds, "thermal policy", a.nw, vec)) return rc;
    const int prec = chain ? 2 : 0;
    name_reset(tun);
    name_add(tun, "cl_rollout_full_policy_kernel<%d, %d, %s>", vec, prec, marl ? "true" : "false");
    const int rc = launch_policy_full(vec, prec, marl, (unsigned)((dims->n_env + tile - 1) / tile), 64u * a.nw, lds, (hipStream_t)stream, p);
    if (rc) return hip_fail((hipError_t)rc, "cl_rollout_full_policy_kernel launch");
    return CL_OK;
}

}  // extern "C"
