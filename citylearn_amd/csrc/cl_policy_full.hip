// cl_policy_full.hip -- the translation unit of libcitylearn_amd_policy_full.so (include/citylearn_amd_policy_full.h): cl_kernels.hip reduced to the
// helpers the fused rollout kernels share and the packed thermal unit of cl_full.h (CL_TU_POLICY cuts the launchers and entry points,
// CL_TU_POLICY_FULL the main library's small passes) + cl_policy_full.h's closed-loop kernel, its launcher and the `clpf_*` entry points.  NOT under
// CL_TU_NOSLP and compiled WITH SLP vectorisation, like the main translation unit: the packed unit wants v_pk_*_f32.
#define CL_TU_POLICY
#define CL_TU_POLICY_FULL
#include "cl_kernels.hip"
#include "../../include/citylearn_amd_policy_full.h"
#include "cl_policy_full.h"

namespace {

int polf_ptr(const void* p, const char* name, bool required = true) {
    if (!p) return required ? fail(CL_ENULL, "%s is NULL", name) : CL_OK;
    if (reinterpret_cast<uintptr_t>(p) & 15) return fail(CL_EALIGN, "%s is not 16-byte aligned", name);
    return CL_OK;
}

// the launcher of this unit; key = 100 * envs per lane + 10 * PREC + MARL
int launch_policy_full(int vec, int prec, bool marl, unsigned grid, unsigned block, size_t lds, hipStream_t s, const PolicyFullArgs& p) {
#define CL_POLF(V, P, M) do { \
        if (lds > 64 * 1024) if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(cl_rollout_full_policy_kernel<V, P, M>), lds); e != hipSuccess) return (int)e; \
        hipLaunchKernelGGL((cl_rollout_full_policy_kernel<V, P, M>), dim3(grid), dim3(block), lds, s, p); } while (0)
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

int clpf_abi_version(void) { return CLPF_ABI_VERSION; }
int clpf_core_abi_version(void) { return CL_ABI_VERSION; }
const char* clpf_last_error(void) { return g_err; }

int clpf_rollout_mlp_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpf_mlp* mlp,
                         float* out_bldg, float* out_env, float* ret_env, float* traj, int32_t t0, int32_t k_steps, void* stream) {
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
    if (dims->flags & CLD_LEAN)
        return fail(CL_EINVAL, "clpf_rollout_mlp_f32: thermal / outage districts only; a battery + PV district (CLD_LEAN) goes to clpol_rollout_mlp_f32 (libcitylearn_amd_policy.so)");
    if (dims->n_bldg > 16)
        return fail(CL_EINVAL, "clpf_rollout_mlp_f32: n_bldg=%d > 16 would be a building-chunked launch, which the policy kernel is not", dims->n_bldg);
    if (dims->flags & CLD_F64_MAPS)
        return fail(CL_EINVAL, "clpf_rollout_mlp_f32: the battery map in fp32 or as the float64 chain (CLD_F64_CHAIN), not CLD_F64_MAPS");
    if (dims->flags & CLD_KPI) return fail(CL_EINVAL, "clpf_rollout_mlp_f32: no streaming KPIs (CLD_KPI) inside this kernel");
    if (dims->flags & CLD_WRITE_DETAIL) return fail(CL_EINVAL, "clpf_rollout_mlp_f32: not with the detail planes (CLD_WRITE_DETAIL)");
    if (rk == CLR_EV) return fail(CL_EINVAL, "clpf_rollout_mlp_f32: reward kind CLR_EV needs the flexible-load tables");
    if (dims->env_pitch != 0 && dims->env_pitch != dims->n_env)
        return fail(CL_EINVAL, "clpf_rollout_mlp_f32: env_pitch=%d != n_env=%d is not implemented for this call", dims->env_pitch, dims->n_env);
    if (dims->n_act_cols > 65536) return fail(CL_EINVAL, "clpf_rollout_mlp_f32: n_act_cols=%d > 65536", dims->n_act_cols);
    if (!mlp) return fail(CL_ENULL, "mlp is NULL");
    if (mlp->n_device_cols != 0)
        return fail(CL_EINVAL, "clpf_rollout_mlp_f32: n_device_cols=%d: a building with a cooling / heating / combined device action column is not covered "
                               "(the policy has storage heads only)", mlp->n_device_cols);
    if (mlp->n_hidden < 4 || mlp->n_hidden > CLPF_MAX_HIDDEN || mlp->n_hidden % 4)
        return fail(CL_EINVAL, "n_hidden=%d: the policy kernel takes 4, 8, .. %d hidden units", mlp->n_hidden, CLPF_MAX_HIDDEN);
    if (mlp->n_sets < 1) return fail(CL_EINVAL, "n_sets=%d: at least one parameter set", mlp->n_sets);
    if (mlp->reserved) return fail(CL_EINVAL, "clpf_mlp.reserved must be 0");
    if (int rc = polf_ptr(params, "params")) return rc;
    if (int rc = polf_ptr(ts, "ts")) return rc;
    if (int rc = polf_ptr(state, "state")) return rc;
    if (int rc = polf_ptr(out_bldg, "out_bldg")) return rc;
    if (int rc = polf_ptr(out_env, "out_env")) return rc;
    if (int rc = polf_ptr(ret_env, "ret_env", false)) return rc;
    if (int rc = polf_ptr(traj, "traj", false)) return rc;
    if (int rc = polf_ptr(mlp->pre, "mlp.pre")) return rc;
    if (int rc = polf_ptr(mlp->dep, "mlp.dep")) return rc;
    if (int rc = polf_ptr(mlp->out, "mlp.out")) return rc;
    if (int rc = polf_ptr(mlp->net_reset, "mlp.net_reset", false)) return rc;
    if (int rc = polf_ptr(mlp->act_low, "mlp.act_low")) return rc;
    if (int rc = polf_ptr(mlp->act_high, "mlp.act_high")) return rc;
    if (int rc = polf_ptr(mlp->sigma, "mlp.sigma", false)) return rc;
    if (reinterpret_cast<uintptr_t>(mlp->set_of_block) & 3) return fail(CL_EALIGN, "mlp.set_of_block is not 4-byte aligned");
    if (k_steps < 0 || t0 < 0 || t0 + k_steps > dims->n_steps)
        return fail(CL_ERANGE, "steps [%d, %d) outside [0, %d)", t0, t0 + k_steps, dims->n_steps);

    const cl_tuning& tun = dims->tuning ? *dims->tuning : cl_tuning{};
    PolicyFullArgs p;
    RolloutArgs& r = p.r;
    StepArgs& a = r.s;
    a.params = params; a.ts = ts; a.state = state; a.actions = nullptr; a.out_bldg = out_bldg; a.out_env = out_env;
    a.kpi_bldg = nullptr; a.kpi_env = nullptr;
    a.act_stride_col = 0; a.act_stride_env = 0;
    a.flex_out = nullptr; a.n_flex_bldg = 0; a.ev_penalty_coef = 0.0f;
    a.n_env = dims->n_env; a.n_bldg = dims->n_bldg; a.n_steps = dims->n_steps; a.ld = dims->n_env;
    a.flags = dims->flags; a.t = t0; a.b_chunk = dims->n_bldg; a.n_chunks = 1; a.env_row0 = dims->env_row0; a.env_offset = (unsigned)dims->env_offset;
    a.nt = 0; a.fused_finish = 0;
    r.act_stride_step = 0; r.act_low = mlp->act_low; r.act_high = mlp->act_high; r.ret_env = ret_env; r.seed = mlp->seed ^ CLPF_NOISE_KEY;
    r.t0 = t0; r.k_steps = k_steps;
    p.pre = mlp->pre; p.dep = mlp->dep; p.out = mlp->out; p.set_of_block = mlp->set_of_block; p.net_reset = mlp->net_reset; p.sigma = mlp->sigma;
    p.traj = traj; p.n_rows = dims->n_ts_rows ? dims->n_ts_rows : dims->n_steps; p.n_hidden = mlp->n_hidden;
    // the packed thermal rollout's geometry: ONE building per wave, the whole district in one workgroup row -- so nw is n_bldg and nothing else
    // (nw > n_bldg: a wave without a building would read parameter row `w` past the end of the table; nw < n_bldg would leave buildings out)
    a.nw = tun.nw ? tun.nw : dims->n_bldg;
    if (a.nw > 16 || a.nw > dims->n_bldg || a.nw < dims->n_bldg)
        return fail(CL_EINVAL, "bad nw %d: the thermal policy rollout runs one building per wave (nw = n_bldg = %d, at most 16)", a.nw, dims->n_bldg);
    const bool chain = dims->flags & CLD_F64_CHAIN, marl = rk == CLR_MARL;
    if (tun.vec != 0 && tun.vec != 1 && tun.vec != 2) return fail(CL_EINVAL, "no thermal policy rollout kernel at %d envs per lane", tun.vec);
    if (tun.vec == 2 && (chain || marl))
        return fail(CL_EINVAL, "no thermal policy rollout kernel at 2 envs per lane under %s: it runs at one env per lane", chain ? "CLD_F64_CHAIN" : "CLR_MARL");
    const int vec = tun.vec ? tun.vec : (chain || marl) ? 1 : 2;
    const int tile = 64 * vec;
    const size_t lds = rollout_full_policy_lds_floats(a.nw, tile) * sizeof(float);
    if (lds > CL_LDS_PER_CU) return fail(CL_EINVAL, "the thermal policy rollout would need %zu bytes of LDS per workgroup (nw=%d, %d envs per lane): a CU has %d", lds, a.nw, vec, CL_LDS_PER_CU);
    const int prec = chain ? 2 : 0;
    name_reset(tun);
    name_add(tun, "cl_rollout_full_policy_kernel<%d, %d, %s>", vec, prec, marl ? "true" : "false");
    const int rc = launch_policy_full(vec, prec, marl, (unsigned)((dims->n_env + tile - 1) / tile), 64u * a.nw, lds, (hipStream_t)stream, p);
    if (rc) return hip_fail((hipError_t)rc, "cl_rollout_full_policy_kernel launch");
    return CL_OK;
}

}  // extern "C"
