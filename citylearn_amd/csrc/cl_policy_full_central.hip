// cl_policy_full_central.hip -- the translation unit of libcitylearn_amd_policy_full_central.so (include/citylearn_amd_policy_full_central.h):
// cl_kernels.hip reduced to the helpers the fused rollout kernels share and the packed thermal unit of cl_full.h (CL_TU_POLICY + CL_TU_POLICY_FULL,
// as in cl_policy_full.hip) + cl_policy_full_central.h's closed-loop kernel under a central-agent policy at DEEP = false (one hidden layer), its
// launcher and the `clpfca_*` entry points.  Compile flags: the library's common ones and nothing else -- NOT under CL_TU_NOSLP and compiled WITH SLP vectorisation, like
// cl_policy_full.hip.  Decided from the generated code of both builds: the four instantiations take the same registers either way (70 / 106 / 106 /
// 121 VGPRs, no scratch memory -- unlike cl_policy_full_deep.hip, whose layer 2 spills under SLP), and with SLP the hidden phase's inner loop pairs
// its four fused-multiply-add chains into v_pk_fma_f32 with the plane value broadcast (op_sel_hi): 10 VALU instructions per (group, building)
// instead of 20 v_fmac_f32, next to the same ten LDS reads, and the same bits (each half is an IEEE fma).  The two builds were not timed against
// each other on the device.
#define CL_TU_POLICY
#define CL_TU_POLICY_FULL
#include "cl_kernels.hip"
#include "../../include/citylearn_amd_policy_full_central.h"
#include "cl_policy_full_central.h"

namespace {

static_assert(CLPFCA_MAX_HIDDEN == CLPFC_MAX_HIDDEN, "the staged head row is sized for the public header's limit");

// the launcher of this unit; key = 10 * PREC + MARL
int launch_policy_full_central(int prec, bool marl, unsigned grid, unsigned block, size_t lds, hipStream_t s, const PolicyArgs& p) {
#define CL_POLFCA(P, M) CL_POLICY_LAUNCH(cl_rollout_full_policy_central_kernel<P, M, false>)
    switch (prec * 10 + (marl ? 1 : 0)) {
    case 0: CL_POLFCA(0, false); break;
    case 1: CL_POLFCA(0, true); break;
    case 20: CL_POLFCA(2, false); break;
    case 21: CL_POLFCA(2, true); break;
    default: return (int)hipErrorInvalidValue;
    }
#undef CL_POLFCA
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

CL_POLICY_ABI(clpfca, CLPFCA_ABI_VERSION)

int clpfca_rollout_mlp_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpfca_mlp* mlp,
                           float* out_bldg, float* out_env, float* ret_env, float* traj, int32_t t0, int32_t k_steps, void* stream) {
    const char* const entry = "clpfca_rollout_mlp_f32";
    if (int rc = check_dims(dims, false)) return rc;
    // ---- what the kernel covers ----
    if (dims->flags & CLD_LEAN)
        return fail(CL_EINVAL, "clpfca_rollout_mlp_f32: thermal / outage districts only; a battery + PV district (CLD_LEAN) under a central-agent policy goes to "
                               "clpca_rollout_mlp_f32 (libcitylearn_amd_policy_central.so)");
    if (dims->n_bldg > CLPFCA_MAX_BLDG)
        return fail(CL_EINVAL, "clpfca_rollout_mlp_f32: n_bldg=%d > %d: the central-agent thermal policy kernel holds the whole district in one workgroup "
                               "(one building per wave); its hidden layer cannot be cut into building chunks", dims->n_bldg, CLPFCA_MAX_BLDG);
    if (int rc = no_f64_maps(dims, entry)) return rc;
    if (dims->flags & CLD_KPI)
        return fail(CL_EINVAL, "clpfca_rollout_mlp_f32: no streaming KPIs (CLD_KPI) inside this kernel -- record traj and replay CLPF_T_ACTION + head through "
                               "cl_rollout_seq_f32");
    if (int rc = no_detail_planes(dims, entry)) return rc;
    if (int rc = no_reward_ev(dims, entry)) return rc;
    if (int rc = no_pitch(dims, entry)) return rc;
    if (int rc = check_central_thermal_policy_mlp(entry, dims, mlp)) return rc;
    const PolicyCall call = {params, ts, state, out_bldg, out_env, ret_env, traj, nullptr, nullptr, t0, k_steps};
    if (int rc = check_policy_buffers(dims, *mlp, call, false)) return rc;

    const cl_tuning& tun = dims->tuning ? *dims->tuning : cl_tuning{};
    PolicyArgs p;
    fill_policy_args(p, dims, *mlp, CLPF_NOISE_KEY, call);
    StepArgs& a = p.r.s;
    if (int rc = one_env_per_lane_only(tun, "central thermal policy")) return rc;
    if (int rc = thermal_one_row_geometry(dims, tun, "central thermal policy", a.nw)) return rc;
    const bool chain = dims->flags & CLD_F64_CHAIN, marl = reward_kind(dims) == CLR_MARL;
    const size_t lds = rollout_full_policy_central_lds_floats(a.nw, dims->n_bldg, mlp->n_hidden) * sizeof(float);
    if (int rc = check_policy_lds(lds, "central thermal policy", a.nw, 1)) return rc;
    const int prec = chain ? 2 : 0;
    name_reset(tun);
    name_add(tun, "cl_rollout_full_policy_central_kernel<%d, %s>", prec, marl ? "true" : "false");
    const int rc = launch_policy_full_central(prec, marl, (unsigned)((dims->n_env + 63) / 64), 64u * a.nw, lds, (hipStream_t)stream, p);
    if (rc) return hip_fail((hipError_t)rc, "cl_rollout_full_policy_central_kernel launch");
    return CL_OK;
}

}  // extern "C"
