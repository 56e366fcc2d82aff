// cl_policy_deep.hip -- the translation unit of libcitylearn_amd_policy_deep.so (include/citylearn_amd_policy_deep.h): cl_kernels.hip reduced to the
// helpers the fused rollout kernels share (CL_TU_POLICY, as in cl_policy.hip) + cl_policy_deep.h's closed-loop kernel with two hidden layers, its
// launcher and the `clpd_*` entry points.  Compiled with -fno-slp-vectorize like cl_policy.hip (citylearn_amd/_lib.py).
#define CL_TU_NOSLP
#define CL_TU_POLICY
#include "cl_kernels.hip"
#include "../../include/citylearn_amd_policy_deep.h"
#include "cl_policy_deep.h"

namespace {

// the launcher of this unit; key = 100 * envs per lane + 10 * PREC + MMA
int launch_policy_deep(int vec, int prec, int mma, unsigned grid, unsigned block, size_t lds, hipStream_t s, const DeepPolicyArgs& p) {
#define CL_POL(V, P, M) CL_POLICY_LAUNCH(cl_rollout_policy_deep_kernel<V, P, M>)
    switch (vec * 100 + prec * 10 + mma) {
    case 100: CL_POL(1, 0, 0); break;
    case 120: CL_POL(1, 2, 0); break;
    case 101: CL_POL(1, 0, 1); break;
    case 121: CL_POL(1, 2, 1); break;
    default: return (int)hipErrorInvalidValue;
    }
#undef CL_POL
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

CL_POLICY_ABI(clpd, CLPD_ABI_VERSION)

int clpd_rollout_mlp_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpd_mlp* mlp,
                         float* out_bldg, float* out_env, float* ret_env, float* traj, int32_t t0, int32_t k_steps, void* stream) {
    const char* const entry = "clpd_rollout_mlp_f32";
    if (int rc = check_dims(dims, false)) return rc;
    // ---- what the kernel covers ----
    if (!(dims->flags & CLD_LEAN))
        return fail(CL_EINVAL, "clpd_rollout_mlp_f32: only battery + PV districts (CLD_LEAN); a thermal / outage district has no deep closed-loop rollout kernel");
    if (dims->n_bldg > 32)
        return fail(CL_EINVAL, "clpd_rollout_mlp_f32: n_bldg=%d > 32 would be a building-chunked launch, which the deep policy kernel is not "
                               "(one workgroup row, two buildings per wave)", dims->n_bldg);
    if (int rc = no_f64_maps(dims, entry)) return rc;
    if (dims->flags & CLD_KPI)
        return fail(CL_EINVAL, "clpd_rollout_mlp_f32: no streaming KPIs (CLD_KPI) inside this kernel -- record traj and replay CLPOL_T_ACTION through cl_rollout_seq_f32");
    if (int rc = no_detail_planes(dims, entry)) return rc;
    if (int rc = no_reward_ev(dims, entry)) return rc;
    if (reward_kind(dims) == CLR_MARL)
        return fail(CL_EINVAL, "clpd_rollout_mlp_f32: reward kind CLR_MARL: the deep policy kernel has no barrier in its K loop to couple the buildings inside a step");
    if (int rc = no_pitch(dims, entry)) return rc;
    if (int rc = check_deep_policy_mlp(mlp)) return rc;
    const PolicyCall call = {params, ts, state, out_bldg, out_env, ret_env, traj, nullptr, nullptr, t0, k_steps};
    if (int rc = check_policy_buffers(dims, *mlp, call, false)) return rc;
    if (int rc = check_ptr(mlp->l2, "mlp.l2")) return rc;

    const cl_tuning& tun = dims->tuning ? *dims->tuning : cl_tuning{};
    DeepPolicyArgs p;
    fill_policy_args(p.p, dims, *mlp, CLPOL_NOISE_KEY, call);
    p.l2 = mlp->l2; p.n_hidden2 = mlp->n_hidden2;
    int vec;
    if (int rc = deep_policy_geometry(dims, tun, p.p.r.s.nw, vec)) return rc;
    const int nw = p.p.r.s.nw, tile = 64 * vec;
    const int mma = (mlp->flags & CLPD_MATRIX_CORES) ? 1 : 0;
    const size_t lds = rollout_policy_deep_lds_floats(nw, tile, mlp->n_hidden, mlp->n_hidden2, mma) * sizeof(float);
    if (int rc = check_policy_lds(lds, "deep policy", nw, vec)) return rc;
    const int prec = (dims->flags & CLD_F64_CHAIN) ? 2 : 0;
    name_reset(tun);
    name_add(tun, "cl_rollout_policy_deep_kernel<%d, %d, %d>", vec, prec, mma);
    const int rc = launch_policy_deep(vec, prec, mma, (unsigned)((dims->n_env + tile - 1) / tile), 64u * nw, lds, (hipStream_t)stream, p);
    if (rc) return hip_fail((hipError_t)rc, "cl_rollout_policy_deep_kernel launch");
    return CL_OK;
}

}  // extern "C"
