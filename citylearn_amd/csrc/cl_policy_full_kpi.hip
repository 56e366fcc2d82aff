// cl_policy_full_kpi.hip -- the translation unit of libcitylearn_amd_policy_full_kpi.so (include/citylearn_amd_policy_full_kpi.h): cl_kernels.hip
// reduced as for cl_policy_full.hip (CL_TU_POLICY, CL_TU_POLICY_FULL), cl_policy_full.h's kernel template under its KPI switch (one env per lane), its
// launcher and the `clpfk_*` entry points.  Compiled WITH SLP vectorisation like
// cl_policy_full.hip.
#define CL_TU_POLICY
#define CL_TU_CONST_TABLES     /* cl_unit.h: the parameter / time-series reads as scalar loads inside a K loop that holds barriers */
#define CL_TU_POLICY_FULL
#include "cl_kernels.hip"
#include "../../include/citylearn_amd_policy_full_kpi.h"
#include "cl_policy_full.h"

namespace {

// the launcher of this unit; key = 10 * PREC + MARL
int launch_policy_full_kpi(int prec, bool marl, unsigned grid, unsigned block, size_t lds, hipStream_t s, const PolicyArgs& p) {
#define CL_POLFK(P, M) CL_POLICY_LAUNCH(cl_rollout_full_policy_kernel<1, P, M, true, false>)
    switch (prec * 10 + (marl ? 1 : 0)) {
    case 0: CL_POLFK(0, false); break;
    case 1: CL_POLFK(0, true); break;
    case 20: CL_POLFK(2, false); break;
    case 21: CL_POLFK(2, true); break;
    default: return (int)hipErrorInvalidValue;
    }
#undef CL_POLFK
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

CL_POLICY_ABI(clpfk, CLPFK_ABI_VERSION)

int clpfk_rollout_mlp_kpi_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpf_mlp* mlp,
                              float* out_bldg, float* out_env, float* ret_env, float* traj, float* kpi_bldg, float* kpi_env,
                              int32_t t0, int32_t k_steps, void* stream) {
    const char* const entry = "clpfk_rollout_mlp_kpi_f32";
    if (int rc = check_dims(dims, false)) return rc;
    // ---- what the kernel covers ----
    if (dims->flags & CLD_LEAN)
        return fail(CL_EINVAL, "clpfk_rollout_mlp_kpi_f32: thermal / outage districts only; a battery + PV district (CLD_LEAN) goes to clpk_rollout_mlp_kpi_f32 (libcitylearn_amd_policy_kpi.so)");
    if (!(dims->flags & CLD_KPI))
        return fail(CL_EINVAL, "clpfk_rollout_mlp_kpi_f32: the district must keep the streaming KPIs (CLD_KPI); without them the call is clpf_rollout_mlp_f32");
    if (dims->n_bldg > 16)
        return fail(CL_EINVAL, "clpfk_rollout_mlp_kpi_f32: n_bldg=%d > 16 would be a building-chunked launch, which the policy KPI kernel is not", dims->n_bldg);
    if (int rc = no_f64_maps(dims, entry)) return rc;
    if (int rc = detail_min_only(dims, entry)) return rc;
    if (int rc = no_reward_ev(dims, entry)) return rc;
    if (int rc = no_pitch(dims, entry)) return rc;
    if (int rc = check_thermal_policy_mlp(entry, dims, mlp)) return rc;
    const PolicyCall call = {params, ts, state, out_bldg, out_env, ret_env, traj, kpi_bldg, kpi_env, t0, k_steps};
    if (int rc = check_policy_buffers(dims, *mlp, call, true)) return rc;

    const cl_tuning& tun = dims->tuning ? *dims->tuning : cl_tuning{};
    PolicyArgs p;
    fill_policy_args(p, dims, *mlp, CLPF_NOISE_KEY, call);
    StepArgs& a = p.r.s;
    // cl_rollout_full_policy_kernel's geometry
    if (int rc = thermal_one_row_geometry(dims, tun, "thermal policy KPI", a.nw)) return rc;
    if (int rc = one_env_per_lane_only(tun, "thermal policy KPI")) return rc;
    const bool chain = dims->flags & CLD_F64_CHAIN, marl = reward_kind(dims) == CLR_MARL;
    const size_t lds = rollout_full_policy_kpi_lds_floats(a.nw) * sizeof(float);
    if (int rc = check_policy_lds(lds, "thermal policy KPI", a.nw, 1)) return rc;
    const int prec = chain ? 2 : 0;
    name_reset(tun);
    name_add(tun, "cl_rollout_full_policy_kpi_kernel<%d, %s>", prec, marl ? "true" : "false");
    const int rc = launch_policy_full_kpi(prec, marl, (unsigned)((dims->n_env + 63) / 64), 64u * a.nw, lds, (hipStream_t)stream, p);
    if (rc) return hip_fail((hipError_t)rc, "cl_rollout_full_policy_kpi_kernel launch");
    return CL_OK;
}

}  // extern "C"
