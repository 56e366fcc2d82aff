// cl_policy_kpi.hip -- the translation unit of libcitylearn_amd_policy_kpi.so (include/citylearn_amd_policy_kpi.h): cl_kernels.hip reduced to the
// helpers the fused rollout kernels share (CL_TU_NOSLP's cut, minus its launchers: CL_TU_POLICY), cl_policy.h for PolicyArgs and the staged-row layout
// (its kernel template is never instantiated here), cl_policy_kpi.h's kernel, its launcher and the `clpk_*` entry points.  Compiled with
// -fno-slp-vectorize like the other rollout kernels (citylearn_amd/_lib.py): same arithmetic, same loss to packed fp32.
#define CL_TU_NOSLP
#define CL_TU_POLICY
#include "cl_kernels.hip"
#include "../../include/citylearn_amd_policy_kpi.h"
#include "cl_policy.h"
#include "cl_policy_kpi.h"

namespace {

int pol_ptr(const void* p, const char* name, bool required = true) {
    if (!p) return required ? fail(CL_ENULL, "%s is NULL", name) : CL_OK;
    if (reinterpret_cast<uintptr_t>(p) & 15) return fail(CL_EALIGN, "%s is not 16-byte aligned", name);
    return CL_OK;
}

// the launcher of this unit (the other libraries' launchers stay what they are); key = 10 * envs per lane + PREC
int launch_policy(int vec, int prec, unsigned grid, unsigned block, size_t lds, hipStream_t s, const PolicyArgs& p) {
#define CL_POL(V, P) do { \
        if (lds > 64 * 1024) if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(cl_rollout_policy_kpi_kernel<V, P>), lds); e != hipSuccess) return (int)e; \
        hipLaunchKernelGGL((cl_rollout_policy_kpi_kernel<V, P>), dim3(grid), dim3(block), lds, s, p); } while (0)
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

int clpk_abi_version(void) { return CLPK_ABI_VERSION; }
int clpk_core_abi_version(void) { return CL_ABI_VERSION; }
const char* clpk_last_error(void) { return g_err; }

int clpk_rollout_mlp_kpi_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpol_mlp* mlp,
                             float* out_bldg, float* out_env, float* ret_env, float* traj, float* kpi_bldg, float* kpi_env,
                             int32_t t0, int32_t k_steps, void* stream) {
    // ---- cl_dims as every entry point of the main library checks it ----
    if (!dims) return fail(CL_ENULL, "dims is NULL");
    if (dims->n_env <= 0 || dims->n_bldg <= 0 || dims->n_steps <= 0 || dims->n_act_cols < 0)
        return fail(CL_EINVAL, "bad dims: n_env=%d n_bldg=%d n_steps=%d n_act_cols=%d", dims->n_env, dims->n_bldg, dims->n_steps, dims->n_act_cols);
    if (dims->n_env % 4 != 0) return fail(CL_EALIGN, "n_env=%d must be a multiple of 4 (pad the env batch)", dims->n_env);
    if (dims->n_ts_rows != 0 && dims->n_ts_rows < dims->n_steps) return fail(CL_EINVAL, "n_ts_rows=%d < n_steps=%d", dims->n_ts_rows, dims->n_steps);
    if (reinterpret_cast<uintptr_t>(dims->env_row0) & 3) return fail(CL_EALIGN, "env_row0 is not 4-byte aligned");
    const uint32_t rk = (dims->flags & CLD_REWARD_MASK) >> CLD_REWARD_SHIFT;
    if (rk > CLR_EV) return fail(CL_EINVAL, "unknown reward kind %u", rk);
    if (dims->env_offset < 0 || dims->env_offset + (int64_t)dims->n_env > (int64_t)1 << 32)
        return fail(CL_ERANGE, "env_offset=%lld with n_env=%d leaves the 32-bit env index of the random streams", (long long)dims->env_offset, dims->n_env);
    // ---- what the kernel covers ----
    if (!(dims->flags & CLD_LEAN))
        return fail(CL_EINVAL, "clpk_rollout_mlp_kpi_f32: only battery + PV districts (CLD_LEAN); a thermal / outage district has no closed-loop rollout kernel");
    if (dims->n_bldg > 32)
        return fail(CL_EINVAL, "clpk_rollout_mlp_kpi_f32: n_bldg=%d > 32 would be a building-chunked launch, which the policy KPI kernel is not", dims->n_bldg);
    if (dims->flags & CLD_F64_MAPS)
        return fail(CL_EINVAL, "clpk_rollout_mlp_kpi_f32: the battery map in fp32 or as the float64 chain (CLD_F64_CHAIN), not CLD_F64_MAPS");
    if (!(dims->flags & CLD_KPI))
        return fail(CL_EINVAL, "clpk_rollout_mlp_kpi_f32: the district must keep the streaming KPIs (CLD_KPI); without them the call is clpol_rollout_mlp_f32");
    if (dims->flags & CLD_WRITE_DETAIL) return fail(CL_EINVAL, "clpk_rollout_mlp_kpi_f32: not with the detail planes (CLD_WRITE_DETAIL)");
    if (rk == CLR_EV) return fail(CL_EINVAL, "clpk_rollout_mlp_kpi_f32: reward kind CLR_EV needs the flexible-load tables");
    if (dims->env_pitch != 0 && dims->env_pitch != dims->n_env)
        return fail(CL_EINVAL, "clpk_rollout_mlp_kpi_f32: env_pitch=%d != n_env=%d is not implemented for this call", dims->env_pitch, dims->n_env);
    if (!mlp) return fail(CL_ENULL, "mlp is NULL");
    if (mlp->n_hidden < 4 || mlp->n_hidden > CLPOL_MAX_HIDDEN || mlp->n_hidden % 4)
        return fail(CL_EINVAL, "n_hidden=%d: the policy kernel takes 4, 8, .. %d hidden units", mlp->n_hidden, CLPOL_MAX_HIDDEN);
    if (mlp->n_sets < 1) return fail(CL_EINVAL, "n_sets=%d: at least one parameter set", mlp->n_sets);
    if (mlp->flags || mlp->reserved) return fail(CL_EINVAL, "clpol_mlp.flags / .reserved must be 0");
    if (int rc = pol_ptr(params, "params")) return rc;
    if (int rc = pol_ptr(ts, "ts")) return rc;
    if (int rc = pol_ptr(state, "state")) return rc;
    if (int rc = pol_ptr(out_bldg, "out_bldg")) return rc;
    if (int rc = pol_ptr(out_env, "out_env")) return rc;
    if (int rc = pol_ptr(ret_env, "ret_env", false)) return rc;
    if (int rc = pol_ptr(traj, "traj", false)) return rc;
    if (int rc = pol_ptr(kpi_bldg, "kpi_bldg")) return rc;
    if (int rc = pol_ptr(kpi_env, "kpi_env")) return rc;
    if (int rc = pol_ptr(mlp->pre, "mlp.pre")) return rc;
    if (int rc = pol_ptr(mlp->dep, "mlp.dep")) return rc;
    if (int rc = pol_ptr(mlp->out, "mlp.out")) return rc;
    if (int rc = pol_ptr(mlp->net_reset, "mlp.net_reset", false)) return rc;
    if (int rc = pol_ptr(mlp->act_low, "mlp.act_low")) return rc;
    if (int rc = pol_ptr(mlp->act_high, "mlp.act_high")) return rc;
    if (int rc = pol_ptr(mlp->sigma, "mlp.sigma", false)) return rc;
    if (reinterpret_cast<uintptr_t>(mlp->set_of_block) & 3) return fail(CL_EALIGN, "mlp.set_of_block is not 4-byte aligned");
    if (k_steps < 0 || t0 < 0 || t0 + k_steps > dims->n_steps)
        return fail(CL_ERANGE, "steps [%d, %d) outside [0, %d)", t0, t0 + k_steps, dims->n_steps);

    const cl_tuning& tun = dims->tuning ? *dims->tuning : cl_tuning{};
    PolicyArgs p;
    RolloutArgs& r = p.r;
    StepArgs& a = r.s;
    a.params = params; a.ts = ts; a.state = state; a.actions = nullptr; a.out_bldg = out_bldg; a.out_env = out_env;
    a.kpi_bldg = kpi_bldg; a.kpi_env = kpi_env;
    a.act_stride_col = 0; a.act_stride_env = 0;
    a.flex_out = nullptr; a.n_flex_bldg = 0; a.ev_penalty_coef = 0.0f;
    a.n_env = dims->n_env; a.n_bldg = dims->n_bldg; a.n_steps = dims->n_steps; a.ld = dims->n_env;
    a.flags = dims->flags; a.t = t0; a.b_chunk = dims->n_bldg; a.n_chunks = 1; a.env_row0 = dims->env_row0; a.env_offset = (unsigned)dims->env_offset;
    a.nt = 0; a.fused_finish = 0;
    r.act_stride_step = 0; r.act_low = mlp->act_low; r.act_high = mlp->act_high; r.ret_env = ret_env; r.seed = mlp->seed ^ CLPOL_NOISE_KEY;
    r.t0 = t0; r.k_steps = k_steps;
    p.pre = mlp->pre; p.dep = mlp->dep; p.out = mlp->out; p.set_of_block = mlp->set_of_block; p.net_reset = mlp->net_reset; p.sigma = mlp->sigma;
    p.traj = traj; p.n_rows = dims->n_ts_rows ? dims->n_ts_rows : dims->n_steps; p.n_hidden = mlp->n_hidden;
    // the lean rollout's geometry: two buildings per wave, two envs per lane where the 128-env workgroups come in (nearly) full rounds of one per CU
    a.nw = tun.nw ? tun.nw : (dims->n_bldg + 1) / 2;
    // (nw > n_bldg: a wave without any building would read its parameter row -- row `w` -- past the end of the table)
    if (a.nw * 2 < dims->n_bldg || a.nw < 1 || a.nw > 16 || a.nw > dims->n_bldg) return fail(CL_EINVAL, "bad nw %d", a.nw);
    const long long wg2 = (dims->n_env + 127) / 128, rounds2 = (wg2 + 255) / 256;
    const bool full_rounds = dims->n_env >= 32768 && wg2 * 100 >= rounds2 * 256 * 85;
    const int vec = tun.vec ? tun.vec : (full_rounds ? 2 : 1);
    if (vec != 1 && vec != 2) return fail(CL_EINVAL, "no policy KPI rollout kernel at %d envs per lane", vec);
    const int tile = 64 * vec;
    const size_t lds = rollout_policy_kpi_lds_floats(a.nw, tile) * sizeof(float);
    if (lds > CL_LDS_PER_CU) return fail(CL_EINVAL, "the policy KPI rollout would need %zu bytes of LDS per workgroup (nw=%d, %d envs per lane): a CU has %d", lds, a.nw, vec, CL_LDS_PER_CU);
    const int prec = (dims->flags & CLD_F64_CHAIN) ? 2 : 0;
    name_reset(tun);
    name_add(tun, "cl_rollout_policy_kpi_kernel<%d, %d>", vec, prec);
    const int rc = launch_policy(vec, prec, (unsigned)((dims->n_env + tile - 1) / tile), 64u * a.nw, lds, (hipStream_t)stream, p);
    if (rc) return hip_fail((hipError_t)rc, "cl_rollout_policy_kpi_kernel launch");
    return CL_OK;
}

}  // extern "C"
