// cl_policy_common.h -- what the three closed-loop policy units share (cl_policy.hip, cl_policy_kpi.hip, cl_policy_full.hip; each behind
// cl_kernels.hip's helpers and cl_rollout.h): the kernels' argument struct, the hidden unit's activation and the Box-Muller draw on the device; the
// argument checks, the argument fill and the launch macro on the host.  The ONE copy of each.  The larger pieces of a step that the kernels have in
// common (row staging, the action, the record, the write-back, the return reduction) stay written out in each kernel: as functions they change the
// generated code of the instantiations that call them (profiles/policy_refactor_isa.md).
#pragma once

#ifdef __HIPCC__
namespace {

// ---- device ---------------------------------------------------------------------------------------------------------------------------
struct PolicyArgs {
    RolloutArgs r;                         // r.s.actions == NULL, r.act_low / r.act_high: the columns' bounds, r.seed: ALREADY xor the library's noise key
    const float* __restrict__ pre;         // [n_sets][n_rows][n_bldg][H]
    const float* __restrict__ dep;         // the lean kernels read [n_sets][n_bldg][2][H], the thermal kernel [n_sets][n_bldg][CLPF_ND][H]
    const float* __restrict__ out;         // the lean kernels read [n_sets][n_bldg][H + 1], the thermal kernel [n_sets][n_bldg][CLPF_NA][H + 1]
    const int32_t* __restrict__ set_of_block;
    const float* __restrict__ net_reset;   // [n_rows][n_bldg] or NULL
    const float* __restrict__ sigma;       // [n_act_cols] or NULL
    float* __restrict__ traj;              // [K][CLPOL_NT | CLPF_NT][n_bldg][n_env] or NULL
    int n_rows, n_hidden;
};

typedef float clpol_f4 __attribute__((ext_vector_type(4)));
typedef const clpol_f4 __attribute__((address_space(4)))* clpol_c4ptr;

// A hidden unit's tanh on the sum the packer pre-scaled by -2 log2 e: (1 - e) / (1 + e) with e = 2^z -- min, v_exp_f32, sub, add, v_rcp_f32, mul.
// The min keeps e finite: (1 - inf) * 0 is a NaN.  (cl_policy.h's header has why not 2 / (1 + e) - 1.)
CL_DEV float clpol_unit(float z) {
    const float e = __builtin_amdgcn_exp2f(fminf(z, 64.0f));
    return (1.0f - e) * __builtin_amdgcn_rcpf(1.0f + e);
}

// Box-Muller on two draws of a column's Philox stream: counters 2t and 2t + 1 = words (0, 1) or (2, 3) of block t >> 1.  The caller owns the
// block: the lean kernels cache it for two steps, the thermal kernel draws it every step.
CL_DEV float clpol_gauss(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, int t) {
    const float u1 = cl::u01((t & 1) ? w2 : w0) + 0x1p-25f, u2 = cl::u01((t & 1) ? w3 : w1);
    // v_log_f32 is log2, v_cos_f32 takes revolutions
    const float rad = __builtin_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));
    return rad * __builtin_amdgcn_cosf(u2);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// The buffers of one call, as the three entry points receive them (kpi_bldg / kpi_env: NULL except for the KPI kernel)
struct PolicyCall {
    const uint32_t* params; const float* ts; float* state; float* out_bldg; float* out_env; float* ret_env; float* traj;
    float* kpi_bldg; float* kpi_env;
    int32_t t0, k_steps;
};

// n_hidden / n_sets of a clpol_mlp or clpf_mlp
template <class MLP>
int check_policy_sizes(const MLP& mlp, int max_hidden) {
    if (mlp.n_hidden < 4 || mlp.n_hidden > max_hidden || mlp.n_hidden % 4)
        return fail(CL_EINVAL, "n_hidden=%d: the policy kernel takes 4, 8, .. %d hidden units", mlp.n_hidden, max_hidden);
    if (mlp.n_sets < 1) return fail(CL_EINVAL, "n_sets=%d: at least one parameter set", mlp.n_sets);
    return CL_OK;
}

// every pointer of the call and of the policy's tables, then the step range (`kpi`: the call takes the KPI planes)
template <class MLP>
int check_policy_buffers(const cl_dims* dims, const MLP& mlp, const PolicyCall& c, bool kpi) {
    if (int rc = check_ptr(c.params, "params")) return rc;
    if (int rc = check_ptr(c.ts, "ts")) return rc;
    if (int rc = check_ptr(c.state, "state")) return rc;
    if (int rc = check_ptr(c.out_bldg, "out_bldg")) return rc;
    if (int rc = check_ptr(c.out_env, "out_env")) return rc;
    if (int rc = check_ptr(c.ret_env, "ret_env", false)) return rc;
    if (int rc = check_ptr(c.traj, "traj", false)) return rc;
    if (kpi) {
        if (int rc = check_ptr(c.kpi_bldg, "kpi_bldg")) return rc;
        if (int rc = check_ptr(c.kpi_env, "kpi_env")) return rc;
    }
    if (int rc = check_ptr(mlp.pre, "mlp.pre")) return rc;
    if (int rc = check_ptr(mlp.dep, "mlp.dep")) return rc;
    if (int rc = check_ptr(mlp.out, "mlp.out")) return rc;
    if (int rc = check_ptr(mlp.net_reset, "mlp.net_reset", false)) return rc;
    if (int rc = check_ptr(mlp.act_low, "mlp.act_low")) return rc;
    if (int rc = check_ptr(mlp.act_high, "mlp.act_high")) return rc;
    if (int rc = check_ptr(mlp.sigma, "mlp.sigma", false)) return rc;
    if (reinterpret_cast<uintptr_t>(mlp.set_of_block) & 3) return fail(CL_EALIGN, "mlp.set_of_block is not 4-byte aligned");
    if (c.k_steps < 0 || c.t0 < 0 || c.t0 + c.k_steps > dims->n_steps)
        return fail(CL_ERANGE, "steps [%d, %d) outside [0, %d)", c.t0, c.t0 + c.k_steps, dims->n_steps);
    return CL_OK;
}

// StepArgs / RolloutArgs / PolicyArgs of a checked call; the geometry (s.nw) is the caller's
template <class MLP>
void fill_policy_args(PolicyArgs& p, const cl_dims* dims, const MLP& mlp, uint64_t noise_key, const PolicyCall& c) {
    RolloutArgs& r = p.r;
    StepArgs& a = r.s;
    a.params = c.params; a.ts = c.ts; a.state = c.state; a.actions = nullptr; a.out_bldg = c.out_bldg; a.out_env = c.out_env;
    a.kpi_bldg = c.kpi_bldg; a.kpi_env = c.kpi_env;
    a.act_stride_col = 0; a.act_stride_env = 0;
    a.flex_out = nullptr; a.n_flex_bldg = 0; a.ev_penalty_coef = 0.0f;
    a.n_env = dims->n_env; a.n_bldg = dims->n_bldg; a.n_steps = dims->n_steps; a.ld = dims->n_env;
    a.flags = dims->flags; a.t = c.t0; a.b_chunk = dims->n_bldg; a.n_chunks = 1; a.env_row0 = dims->env_row0; a.env_offset = (unsigned)dims->env_offset;
    a.nt = 0; a.fused_finish = 0;
    r.act_stride_step = 0; r.act_low = mlp.act_low; r.act_high = mlp.act_high; r.ret_env = c.ret_env; r.seed = mlp.seed ^ noise_key;
    r.t0 = c.t0; r.k_steps = c.k_steps;
    p.pre = mlp.pre; p.dep = mlp.dep; p.out = mlp.out; p.set_of_block = mlp.set_of_block; p.net_reset = mlp.net_reset; p.sigma = mlp.sigma;
    p.traj = c.traj; p.n_rows = dims->n_ts_rows ? dims->n_ts_rows : dims->n_steps; p.n_hidden = mlp.n_hidden;
}

// the workgroup's dynamic LDS against what a CU has (`what`: "policy", "policy KPI", "thermal policy")
int check_policy_lds(size_t lds, const char* what, int nw, int vec) {
    if (lds > CL_LDS_PER_CU) return fail(CL_EINVAL, "the %s rollout would need %zu bytes of LDS per workgroup (nw=%d, %d envs per lane): a CU has %d", what, lds, nw, vec, CL_LDS_PER_CU);
    return CL_OK;
}

// Launch one kernel instantiation (in a launcher that has grid, block, lds, s and p, and returns a hipError_t as int): above the default 64 KiB
// of dynamic LDS the kernel is opted in first
#define CL_POLICY_LAUNCH(...) do { \
        if (lds > 64 * 1024) if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(__VA_ARGS__), lds); e != hipSuccess) return (int)e; \
        hipLaunchKernelGGL((__VA_ARGS__), dim3(grid), dim3(block), lds, s, p); } while (0)

}  // namespace
#endif  // __HIPCC__
