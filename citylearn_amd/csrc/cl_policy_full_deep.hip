// cl_policy_full_deep.hip -- the translation unit of libcitylearn_amd_policy_full_deep.so (include/citylearn_amd_policy_full_deep.h): cl_kernels.hip
// reduced to the helpers the fused rollout kernels share and the packed thermal unit of cl_full.h (CL_TU_POLICY + CL_TU_POLICY_FULL, as in
// cl_policy_full.hip) + cl_policy_full_deep.h's closed-loop kernel with two hidden layers, its launcher and the `clpfd_*` entry points.
// Compiled with -fno-slp-vectorize (citylearn_amd/_lib.py), UNLIKE cl_policy_full.hip: the policy block needs it.  With SLP vectorisation the
// compiler pairs the layer-2 chains z2_i = fmaf(l2[j][i], h1_j, z2_i) into v_pk_fma_f32, which wants h1_j and the loop's invariants duplicated
// into register pairs, and all four exact-fp32 instantiations spill: 26 - 34 VGPRs, 88 - 104 bytes of scratch memory per lane, coming from the
// H2 >= 20 variants of the block (with H2 <= 16 alone they fit).  Without it they take 89 - 115 VGPRs and no scratch; the matrix-core ones
// take 127 either way.  The thermal unit at one env per lane loses the few v_pk_*_f32 that SLP finds across its tanks (the explicit two-env
// vector types, where packing pays, are not instantiated here).  The unit is not under CL_TU_NOSLP: that macro picks the lean kernels.
#define CL_TU_POLICY
#define CL_TU_POLICY_FULL
#include "cl_kernels.hip"
#include "../../include/citylearn_amd_policy_full_deep.h"
#include "cl_policy_full_deep.h"

namespace {

// the launcher of this unit; key = 100 * PREC + 10 * MMA + MARL
int launch_policy_full_deep(int prec, int mma, bool marl, unsigned grid, unsigned block, size_t lds, hipStream_t s, const DeepFullPolicyArgs& p) {
#define CL_POLFD(P, M, R) CL_POLICY_LAUNCH(cl_rollout_full_policy_deep_kernel<P, M, R>)
    switch (prec * 100 + mma * 10 + (marl ? 1 : 0)) {
    case 0: CL_POLFD(0, 0, false); break;
    case 1: CL_POLFD(0, 0, true); break;
    case 10: CL_POLFD(0, 1, false); break;
    case 11: CL_POLFD(0, 1, true); break;
    case 200: CL_POLFD(2, 0, false); break;
    case 201: CL_POLFD(2, 0, true); break;
    case 210: CL_POLFD(2, 1, false); break;
    case 211: CL_POLFD(2, 1, true); break;
    default: return (int)hipErrorInvalidValue;
    }
#undef CL_POLFD
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

CL_POLICY_ABI(clpfd, CLPFD_ABI_VERSION)

int clpfd_rollout_mlp_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpfd_mlp* mlp,
                          float* out_bldg, float* out_env, float* ret_env, float* traj, int32_t t0, int32_t k_steps, void* stream) {
    const char* const entry = "clpfd_rollout_mlp_f32";
    if (int rc = check_dims(dims, false)) return rc;
    // ---- what the kernel covers ----
    if (dims->flags & CLD_LEAN)
        return fail(CL_EINVAL, "clpfd_rollout_mlp_f32: thermal / outage districts only; a battery + PV district (CLD_LEAN) with a two-hidden-layer policy goes to "
                               "clpd_rollout_mlp_f32 (libcitylearn_amd_policy_deep.so)");
    if (dims->n_bldg > 16)
        return fail(CL_EINVAL, "clpfd_rollout_mlp_f32: n_bldg=%d > 16 would be a building-chunked launch, which the deep thermal policy kernel is not "
                               "(one workgroup row, one building per wave)", dims->n_bldg);
    if (int rc = no_f64_maps(dims, entry)) return rc;
    if (dims->flags & CLD_KPI)
        return fail(CL_EINVAL, "clpfd_rollout_mlp_f32: no streaming KPIs (CLD_KPI) inside this kernel -- record traj and replay CLPF_T_ACTION through cl_rollout_seq_f32");
    if (int rc = no_detail_planes(dims, entry)) return rc;
    if (int rc = no_reward_ev(dims, entry)) return rc;
    if (int rc = no_pitch(dims, entry)) return rc;
    if (int rc = check_deep_thermal_policy_mlp(entry, dims, mlp)) return rc;
    const PolicyCall call = {params, ts, state, out_bldg, out_env, ret_env, traj, nullptr, nullptr, t0, k_steps};
    if (int rc = check_policy_buffers(dims, *mlp, call, false)) return rc;
    if (int rc = check_ptr(mlp->l2, "mlp.l2")) return rc;

    const cl_tuning& tun = dims->tuning ? *dims->tuning : cl_tuning{};
    DeepFullPolicyArgs p;
    fill_policy_args(p.p, dims, *mlp, CLPF_NOISE_KEY, call);
    p.l2 = mlp->l2; p.n_hidden2 = mlp->n_hidden2;
    StepArgs& a = p.p.r.s;
    if (int rc = thermal_one_row_geometry(dims, tun, "deep thermal policy", a.nw)) return rc;
    if (int rc = one_env_per_lane_only(tun, "deep thermal policy")) return rc;
    const bool chain = dims->flags & CLD_F64_CHAIN, marl = reward_kind(dims) == CLR_MARL;
    const int mma = (mlp->flags & CLPFD_MATRIX_CORES) ? 1 : 0;
    const size_t lds = rollout_full_policy_deep_lds_floats(a.nw, mlp->n_hidden, mlp->n_hidden2, mma) * sizeof(float);
    if (int rc = check_policy_lds(lds, "deep thermal policy", a.nw, 1)) return rc;
    const int prec = chain ? 2 : 0;
    name_reset(tun);
    name_add(tun, "cl_rollout_full_policy_deep_kernel<%d, %d, %s>", prec, mma, marl ? "true" : "false");
    const int rc = launch_policy_full_deep(prec, mma, marl, (unsigned)((dims->n_env + 63) / 64), 64u * a.nw, lds, (hipStream_t)stream, p);
    if (rc) return hip_fail((hipError_t)rc, "cl_rollout_full_policy_deep_kernel launch");
    return CL_OK;
}

}  // extern "C"
