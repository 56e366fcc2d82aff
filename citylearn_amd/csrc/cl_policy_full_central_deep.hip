// cl_policy_full_central_deep.hip -- the translation unit of libcitylearn_amd_policy_full_central_deep.so
// (include/citylearn_amd_policy_full_central_deep.h): cl_kernels.hip reduced to the helpers the fused rollout kernels share and the packed thermal
// unit of cl_full.h (CL_TU_POLICY + CL_TU_POLICY_FULL, as in cl_policy_full_central.hip) + cl_policy_full_central.h's closed-loop kernel
// under a central-agent policy at DEEP = true (two hidden layers), its launcher and the `clpfcd_*` entry points.  Compile flags: the library's common ones and
// nothing else -- NOT under CL_TU_NOSLP and compiled WITH SLP vectorisation, like cl_policy_full_central.hip: the first hidden phase and the packed
// thermal unit are that unit's, and the second hidden phase is ONE loop of four chains over a broadcast ds_read_b128, which SLP pairs into
// v_pk_fma_f32 as it pairs the first (the same bits: each half is an IEEE fma) -- unlike cl_policy_full_deep.hip's per-building layer 2, whose
// unrolled H2 variants spill under SLP.  The register figures of the four instantiations are in cl_policy_full_central.h's header.
#define CL_TU_POLICY
#define CL_TU_POLICY_FULL
#include "cl_kernels.hip"
#include "../../include/citylearn_amd_policy_full_central_deep.h"
#include "cl_policy_full_central.h"

namespace {

static_assert(CLPFCD_MAX_HIDDEN == CLPFC_MAX_HIDDEN, "the staged head row is sized for the public header's limit");

// the launcher of this unit; key = 10 * PREC + MARL
int launch_policy_full_central_deep(int prec, bool marl, unsigned grid, unsigned block, size_t lds, hipStream_t s, const CentralDeepFullPolicyArgs& p) {
#define CL_POLFCD(P, M) CL_POLICY_LAUNCH(cl_rollout_full_policy_central_kernel<P, M, true>)
    switch (prec * 10 + (marl ? 1 : 0)) {
    case 0: CL_POLFCD(0, false); break;
    case 1: CL_POLFCD(0, true); break;
    case 20: CL_POLFCD(2, false); break;
    case 21: CL_POLFCD(2, true); break;
    default: return (int)hipErrorInvalidValue;
    }
#undef CL_POLFCD
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

CL_POLICY_ABI(clpfcd, CLPFCD_ABI_VERSION)

int clpfcd_rollout_mlp_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpfcd_mlp* mlp,
                           float* out_bldg, float* out_env, float* ret_env, float* traj, int32_t t0, int32_t k_steps, void* stream) {
    const char* const entry = "clpfcd_rollout_mlp_f32";
    if (int rc = check_dims(dims, false)) return rc;
    // ---- what the kernel covers ----
    if (dims->flags & CLD_LEAN)
        return fail(CL_EINVAL, "clpfcd_rollout_mlp_f32: thermal / outage districts only; a battery + PV district (CLD_LEAN) under a central-agent policy with two "
                               "hidden layers goes to clpcd_rollout_mlp_f32 (libcitylearn_amd_policy_central_deep.so)");
    if (dims->n_bldg > CLPFCD_MAX_BLDG)
        return fail(CL_EINVAL, "clpfcd_rollout_mlp_f32: n_bldg=%d > %d: the central-agent thermal policy kernel holds the whole district in one workgroup "
                               "(one building per wave); its hidden layers cannot be cut into building chunks", dims->n_bldg, CLPFCD_MAX_BLDG);
    if (int rc = no_f64_maps(dims, entry)) return rc;
    if (dims->flags & CLD_KPI)
        return fail(CL_EINVAL, "clpfcd_rollout_mlp_f32: no streaming KPIs (CLD_KPI) inside this kernel -- record traj and replay CLPF_T_ACTION + head through "
                               "cl_rollout_seq_f32");
    if (int rc = no_detail_planes(dims, entry)) return rc;
    if (int rc = no_reward_ev(dims, entry)) return rc;
    if (int rc = no_pitch(dims, entry)) return rc;
    if (int rc = check_central_deep_thermal_policy_mlp(entry, dims, mlp)) return rc;
    if (int rc = check_ptr(mlp->l2, "mlp.l2")) return rc;
    const PolicyCall call = {params, ts, state, out_bldg, out_env, ret_env, traj, nullptr, nullptr, t0, k_steps};
    if (int rc = check_policy_buffers(dims, *mlp, call, false)) return rc;

    const cl_tuning& tun = dims->tuning ? *dims->tuning : cl_tuning{};
    CentralDeepFullPolicyArgs p;
    fill_policy_args(p.p, dims, *mlp, CLPF_NOISE_KEY, call);
    p.l2 = mlp->l2; p.n_hidden2 = mlp->n_hidden2;
    StepArgs& a = p.p.r.s;
    if (int rc = one_env_per_lane_only(tun, "deep central thermal policy")) return rc;
    if (int rc = thermal_one_row_geometry(dims, tun, "deep central thermal policy", a.nw)) return rc;
    const bool chain = dims->flags & CLD_F64_CHAIN, marl = reward_kind(dims) == CLR_MARL;
    const size_t lds = rollout_full_policy_central_deep_lds_floats(a.nw, dims->n_bldg, mlp->n_hidden, mlp->n_hidden2) * sizeof(float);
    if (int rc = check_policy_lds(lds, "deep central thermal policy", a.nw, 1)) return rc;
    const int prec = chain ? 2 : 0;
    name_reset(tun);
    name_add(tun, "cl_rollout_full_policy_central_deep_kernel<%d, %s>", prec, marl ? "true" : "false");
    const int rc = launch_policy_full_central_deep(prec, marl, (unsigned)((dims->n_env + 63) / 64), 64u * a.nw, lds, (hipStream_t)stream, p);
    if (rc) return hip_fail((hipError_t)rc, "cl_rollout_full_policy_central_deep_kernel launch");
    return CL_OK;
}

}  // extern "C"
