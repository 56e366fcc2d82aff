// cl_policy_full_kpi.hip -- the translation unit of libcitylearn_amd_policy_full_kpi.so (include/citylearn_amd_policy_full_kpi.h): cl_kernels.hip
// reduced as for cl_policy_full.hip (CL_TU_POLICY, CL_TU_POLICY_FULL), cl_policy_full.h for the staged-row layout (its kernel template is never
// instantiated here), cl_policy_full_kpi.h's kernel, its launcher and the `clpfk_*` entry points.  Compiled WITH SLP vectorisation like
// cl_policy_full.hip.
#define CL_TU_POLICY
#define CL_TU_CONST_TABLES     /* cl_unit.h: the parameter / time-series reads as scalar loads inside a K loop that holds barriers */
#define CL_TU_POLICY_FULL
#include "cl_kernels.hip"
#include "../../include/citylearn_amd_policy_full_kpi.h"
#include "cl_policy_full.h"
#include "cl_policy_full_kpi.h"

namespace {

// the launcher of this unit; key = 10 * PREC + MARL
int launch_policy_full_kpi(int prec, bool marl, unsigned grid, unsigned block, size_t lds, hipStream_t s, const PolicyArgs& p) {
#define CL_POLFK(P, M) CL_POLICY_LAUNCH(cl_rollout_full_policy_kpi_kernel<P, M>)
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

int clpfk_abi_version(void) { return CLPFK_ABI_VERSION; }
int clpfk_core_abi_version(void) { return CL_ABI_VERSION; }
const char* clpfk_last_error(void) { return g_err; }

int clpfk_rollout_mlp_kpi_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpf_mlp* mlp,
                              float* out_bldg, float* out_env, float* ret_env, float* traj, float* kpi_bldg, float* kpi_env,
                              int32_t t0, int32_t k_steps, void* stream) {
    if (int rc = check_dims(dims, false)) return rc;
    const uint32_t rk = (dims->flags & CLD_REWARD_MASK) >> CLD_REWARD_SHIFT;
    // ---- what the kernel covers ----
    if (dims->flags & CLD_LEAN)
        return fail(CL_EINVAL, "clpfk_rollout_mlp_kpi_f32: thermal / outage districts only; a battery + PV district (CLD_LEAN) goes to clpk_rollout_mlp_kpi_f32 (libcitylearn_amd_policy_kpi.so)");
    if (!(dims->flags & CLD_KPI))
        return fail(CL_EINVAL, "clpfk_rollout_mlp_kpi_f32: the district must keep the streaming KPIs (CLD_KPI); without them the call is clpf_rollout_mlp_f32");
    if (dims->n_bldg > 16)
        return fail(CL_EINVAL, "clpfk_rollout_mlp_kpi_f32: n_bldg=%d > 16 would be a building-chunked launch, which the policy KPI kernel is not", dims->n_bldg);
    if (dims->flags & CLD_F64_MAPS)
        return fail(CL_EINVAL, "clpfk_rollout_mlp_kpi_f32: the battery map in fp32 or as the float64 chain (CLD_F64_CHAIN), not CLD_F64_MAPS");
    if ((dims->flags & CLD_WRITE_DETAIL) && !(dims->flags & CLD_DETAIL_MIN))
        return fail(CL_EINVAL, "clpfk_rollout_mlp_kpi_f32: of the detail planes (CLD_WRITE_DETAIL) only the subset of CLD_DETAIL_MIN is written");
    if (rk == CLR_EV) return fail(CL_EINVAL, "clpfk_rollout_mlp_kpi_f32: reward kind CLR_EV needs the flexible-load tables");
    if (int rc = no_pitch(dims, "clpfk_rollout_mlp_kpi_f32")) return rc;
    if (dims->n_act_cols > 65536) return fail(CL_EINVAL, "clpfk_rollout_mlp_kpi_f32: n_act_cols=%d > 65536", dims->n_act_cols);
    if (!mlp) return fail(CL_ENULL, "mlp is NULL");
    if (mlp->n_device_cols != 0)
        return fail(CL_EINVAL, "clpfk_rollout_mlp_kpi_f32: n_device_cols=%d: a building with a cooling / heating / combined device action column is not covered "
                               "(the policy has storage heads only)", mlp->n_device_cols);
    if (int rc = check_policy_sizes(*mlp, CLPF_MAX_HIDDEN)) return rc;
    if (mlp->reserved) return fail(CL_EINVAL, "clpf_mlp.reserved must be 0");
    const PolicyCall call = {params, ts, state, out_bldg, out_env, ret_env, traj, kpi_bldg, kpi_env, t0, k_steps};
    if (int rc = check_policy_buffers(dims, *mlp, call, true)) return rc;

    const cl_tuning& tun = dims->tuning ? *dims->tuning : cl_tuning{};
    PolicyArgs p;
    fill_policy_args(p, dims, *mlp, CLPF_NOISE_KEY, call);
    StepArgs& a = p.r.s;
    // cl_rollout_full_policy_kernel's geometry: ONE building per wave, the whole district in one workgroup row -- so nw is n_bldg and nothing else
    a.nw = tun.nw ? tun.nw : dims->n_bldg;
    if (a.nw > 16 || a.nw > dims->n_bldg || a.nw < dims->n_bldg)
        return fail(CL_EINVAL, "bad nw %d: the thermal policy KPI rollout runs one building per wave (nw = n_bldg = %d, at most 16)", a.nw, dims->n_bldg);
    if (tun.vec == 2) return fail(CL_EINVAL, "no thermal policy KPI rollout kernel at 2 envs per lane: it runs at one env per lane");
    if (tun.vec != 0 && tun.vec != 1) return fail(CL_EINVAL, "no thermal policy KPI rollout kernel at %d envs per lane", tun.vec);
    const bool chain = dims->flags & CLD_F64_CHAIN, marl = rk == CLR_MARL;
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
