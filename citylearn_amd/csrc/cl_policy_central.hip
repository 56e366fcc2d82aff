// cl_policy_central.hip -- the translation unit of libcitylearn_amd_policy_central.so (include/citylearn_amd_policy_central.h): cl_kernels.hip reduced
// to the helpers the fused rollout kernels share (CL_TU_POLICY, as in cl_policy.hip) + cl_policy_central.h's closed-loop kernel under a central-agent
// policy at DEEP = false (one hidden layer), its launcher and the `clpca_*` entry points.  Compiled with -fno-slp-vectorize like cl_policy.hip (citylearn_amd/_lib.py).
#define CL_TU_NOSLP
#define CL_TU_POLICY
#include "cl_kernels.hip"
#include "../../include/citylearn_amd_policy_central.h"
#include "cl_policy_central.h"

namespace {

static_assert(CLPCA_MAX_HIDDEN == CLPC_MAX_HIDDEN, "the staged out row is sized for the public header's limit");

// the launcher of this unit; key = PREC
int launch_policy_central(int prec, unsigned grid, unsigned block, size_t lds, hipStream_t s, const PolicyArgs& p) {
    switch (prec) {
    case 0: CL_POLICY_LAUNCH(cl_rollout_policy_central_kernel<0, false>); break;
    case 2: CL_POLICY_LAUNCH(cl_rollout_policy_central_kernel<2, false>); break;
    default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

CL_POLICY_ABI(clpca, CLPCA_ABI_VERSION)

int clpca_rollout_mlp_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpca_mlp* mlp,
                          float* out_bldg, float* out_env, float* ret_env, float* traj, int32_t t0, int32_t k_steps, void* stream) {
    const char* const entry = "clpca_rollout_mlp_f32";
    if (int rc = check_dims(dims, false)) return rc;
    // ---- what the kernel covers ----
    if (!(dims->flags & CLD_LEAN))
        return fail(CL_EINVAL, "clpca_rollout_mlp_f32: only battery + PV districts (CLD_LEAN); a thermal / outage district has no central-agent rollout kernel");
    if (dims->n_bldg > CLPCA_MAX_BLDG)
        return fail(CL_EINVAL, "clpca_rollout_mlp_f32: n_bldg=%d > %d: the central-agent policy kernel holds the whole district in one workgroup "
                               "(two buildings per wave); its hidden layer cannot be cut into building chunks", dims->n_bldg, CLPCA_MAX_BLDG);
    if (int rc = no_f64_maps(dims, entry)) return rc;
    if (dims->flags & CLD_KPI)
        return fail(CL_EINVAL, "clpca_rollout_mlp_f32: no streaming KPIs (CLD_KPI) inside this kernel -- record traj and replay CLPOL_T_ACTION through cl_rollout_seq_f32");
    if (int rc = no_detail_planes(dims, entry)) return rc;
    if (int rc = no_reward_ev(dims, entry)) return rc;
    if (int rc = no_pitch(dims, entry)) return rc;
    if (int rc = check_central_policy_mlp(mlp)) return rc;
    const PolicyCall call = {params, ts, state, out_bldg, out_env, ret_env, traj, nullptr, nullptr, t0, k_steps};
    if (int rc = check_policy_buffers(dims, *mlp, call, false)) return rc;

    const cl_tuning& tun = dims->tuning ? *dims->tuning : cl_tuning{};
    PolicyArgs p;
    fill_policy_args(p, dims, *mlp, CLPOL_NOISE_KEY, call);
    if (int rc = central_policy_geometry(dims, tun, "central policy", p.r.s.nw)) return rc;
    const int nw = p.r.s.nw;
    const size_t lds = rollout_policy_central_lds_floats(nw, dims->n_bldg, mlp->n_hidden) * sizeof(float);
    if (int rc = check_policy_lds(lds, "central policy", nw, 1)) return rc;
    const int prec = (dims->flags & CLD_F64_CHAIN) ? 2 : 0;
    name_reset(tun);
    name_add(tun, "cl_rollout_policy_central_kernel<%d>", prec);
    const int rc = launch_policy_central(prec, (unsigned)((dims->n_env + 63) / 64), 64u * nw, lds, (hipStream_t)stream, p);
    if (rc) return hip_fail((hipError_t)rc, "cl_rollout_policy_central_kernel launch");
    return CL_OK;
}

}  // extern "C"
