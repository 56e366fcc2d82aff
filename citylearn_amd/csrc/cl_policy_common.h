// cl_policy_common.h -- what the closed-loop policy units share (cl_policy.hip, cl_policy_kpi.hip, cl_policy_chunk.hip, cl_policy_deep.hip
// for battery + PV districts; cl_policy_full.hip, cl_policy_full_kpi.hip, cl_policy_full_chunk.hip, cl_policy_full_chunk_kpi.hip for thermal ones;
// each behind cl_kernels.hip's helpers and cl_rollout.h).  The ONE copy of each:
//   device  PolicyArgs, the hidden unit's activation (clpol_unit), the Box-Muller draw (clpol_gauss);
//   host    the three entry points every library exports besides its rollout (CL_POLICY_ABI);
//           the coverage refusals whose text is the same up to the entry's name (no_f64_maps, no_reward_ev, no_chunked_marl, no_detail_planes,
//           detail_min_only) -- an entry calls them in ITS order, which is behaviour (tests/test_policy_refusals_host.py pins which one wins);
//           the mlp struct's checks (check_policy_sizes, check_lean_policy_mlp, check_thermal_policy_mlp) and the buffers' (check_policy_buffers);
//           the argument fill (fill_policy_args);
//           the geometry rules: policy_chunk_geometry (b_chunk / n_chunks of a building-chunked launch), thermal_one_row_geometry,
//           one_env_per_lane_only, check_policy_lds -- cl_kernels.hip holds the ones the blind rollouts use too: full_rounds,
//           chunk_partials_fit / check_chunk_partials, launch_rollout_finish;
//           the launch macro (CL_POLICY_LAUNCH).
// What is an entry's own stays written out in it: the CLD_LEAN and CLD_KPI redirects, n_bldg > 16 / 32, its nw and envs-per-lane lines, its launcher.
// The larger pieces of a step that the kernels have in common (row staging, the action, the record, the write-back, the return reduction) are not
// here: as functions they change the generated code of the instantiations that call them (profiles/policy_refactor_isa.md).  As ONE template source
// whose variant-only statements sit under `if constexpr` they do not (profiles/policy_one_source_isa.md) -- that is how the three lean kernels
// (cl_policy.h), the central-agent pair (cl_policy_central.h) and the four per-building thermal kernels (cl_policy_full.h:
// profiles/policy_full_one_source_isa.md) share them; in the kernels still written out they wait for the same treatment.
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
// <prefix>_abi_version, <prefix>_core_abi_version, <prefix>_last_error (inside the unit's extern "C" block)
#define CL_POLICY_ABI(prefix, version) \
    int prefix##_abi_version(void) { return version; } \
    int prefix##_core_abi_version(void) { return CL_ABI_VERSION; } \
    const char* prefix##_last_error(void) { return g_err; }

// ---- what a kernel covers: the refusals that read the same in every entry (`entry`: its name) ----
inline uint32_t reward_kind(const cl_dims* dims) { return (dims->flags & CLD_REWARD_MASK) >> CLD_REWARD_SHIFT; }
inline int no_f64_maps(const cl_dims* dims, const char* entry) {
    return (dims->flags & CLD_F64_MAPS) ? fail(CL_EINVAL, "%s: the battery map in fp32 or as the float64 chain (CLD_F64_CHAIN), not CLD_F64_MAPS", entry) : CL_OK;
}
inline int no_reward_ev(const cl_dims* dims, const char* entry) {
    return reward_kind(dims) == CLR_EV ? fail(CL_EINVAL, "%s: reward kind CLR_EV needs the flexible-load tables", entry) : CL_OK;
}
inline int no_chunked_marl(const cl_dims* dims, const char* entry) {
    return reward_kind(dims) == CLR_MARL ? fail(CL_EINVAL, "%s: reward kind CLR_MARL: a building-chunked launch cannot couple the buildings inside a step", entry) : CL_OK;
}
inline int no_detail_planes(const cl_dims* dims, const char* entry) {
    return (dims->flags & CLD_WRITE_DETAIL) ? fail(CL_EINVAL, "%s: not with the detail planes (CLD_WRITE_DETAIL)", entry) : CL_OK;
}
inline int detail_min_only(const cl_dims* dims, const char* entry) {
    const bool all = (dims->flags & CLD_WRITE_DETAIL) && !(dims->flags & CLD_DETAIL_MIN);
    return all ? fail(CL_EINVAL, "%s: of the detail planes (CLD_WRITE_DETAIL) only the subset of CLD_DETAIL_MIN is written", entry) : CL_OK;
}

// The buffers of one call, as the entry points receive them (kpi_bldg / kpi_env: NULL except for the KPI kernels)
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

// the struct of a battery + PV policy (the three lean units) and of a thermal one (the four thermal units, with the action-column count that the
// kernels' 16-bit column ids admit); each where the unit has included the public header that declares the struct
#ifdef CITYLEARN_AMD_POLICY_H
inline int check_lean_policy_mlp(const clpol_mlp* mlp) {
    if (!mlp) return fail(CL_ENULL, "mlp is NULL");
    if (int rc = check_policy_sizes(*mlp, CLPOL_MAX_HIDDEN)) return rc;
    if (mlp->flags || mlp->reserved) return fail(CL_EINVAL, "clpol_mlp.flags / .reserved must be 0");
    return CL_OK;
}
#endif
#ifdef CITYLEARN_AMD_POLICY_FULL_H
inline int check_thermal_policy_mlp(const char* entry, const cl_dims* dims, const clpf_mlp* mlp) {
    if (dims->n_act_cols > 65536) return fail(CL_EINVAL, "%s: n_act_cols=%d > 65536", entry, dims->n_act_cols);
    if (!mlp) return fail(CL_ENULL, "mlp is NULL");
    if (mlp->n_device_cols != 0)
        return fail(CL_EINVAL, "%s: n_device_cols=%d: a building with a cooling / heating / combined device action column is not covered "
                               "(the policy has storage heads only)", entry, mlp->n_device_cols);
    if (int rc = check_policy_sizes(*mlp, CLPF_MAX_HIDDEN)) return rc;
    if (mlp->reserved) return fail(CL_EINVAL, "clpf_mlp.reserved must be 0");
    return CL_OK;
}
#endif

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

// ---- geometry ----
// A building-chunked launch: b_chunk buildings per workgroup row, n_chunks rows along gridDim.y.  `per_wave` buildings a wave (2: battery + PV,
// 1: thermal), so a row holds at most 16 x per_wave; the default is the blind chunked rollout's (cl_rollout_f32) -- 32-building rows for battery +
// PV, EIGHT for the packed thermal kernel (two or three workgroups per CU instead of one of sixteen waves) -- BALANCED over the chunks.  A district
// that fits one row is `one_row`'s launch (in `one_row_lib`) unless the caller asks for chunks.  The waves per row and the room in the reserved
// plane (check_chunk_partials) are the entry's own lines: the entries check them at different points.
struct ChunkRule { int per_wave; const char* entry; const char* one_row; const char* one_row_lib; };
inline int policy_chunk_geometry(const cl_dims* dims, const cl_tuning& tun, const ChunkRule& rule, int& b_chunk, int& n_chunks) {
    const bool pair = rule.per_wave == 2;
    const int b_max = 16 * rule.per_wave, b_default = pair ? 32 : 8;
    if (tun.b_chunk < 0) return fail(CL_EINVAL, "b_chunk=%d", tun.b_chunk);
    if (tun.b_chunk > b_max)
        return fail(CL_EINVAL, "b_chunk=%d: a %spolicy rollout workgroup holds at most %d buildings (%s per wave)", tun.b_chunk, pair ? "" : "thermal ", b_max,
                    pair ? "two" : "one");
    if (tun.b_chunk == 0 && dims->n_bldg <= b_max)
        return fail(CL_EINVAL, "%s: n_bldg=%d fits one workgroup row, which is %s's launch (%s); a chunked launch of it takes an explicit cl_tuning.b_chunk < n_bldg",
                    rule.entry, dims->n_bldg, rule.one_row, rule.one_row_lib);
    if (tun.b_chunk >= dims->n_bldg)
        return fail(CL_EINVAL, "b_chunk=%d >= n_bldg=%d: one workgroup row is %s's launch (%s)", tun.b_chunk, dims->n_bldg, rule.one_row, rule.one_row_lib);
    if (tun.b_chunk > 0) {
        b_chunk = tun.b_chunk;
    } else {
        const int nc = (dims->n_bldg + b_default - 1) / b_default;
        b_chunk = (dims->n_bldg + nc - 1) / nc;
    }
    n_chunks = (dims->n_bldg + b_chunk - 1) / b_chunk;
    return CL_OK;
}

// The one-row thermal rollouts: ONE building per wave, the whole district in one workgroup row -- so nw is n_bldg and nothing else (nw > n_bldg: a
// wave without a building would read parameter row `w` past the end of the table; nw < n_bldg would leave buildings out).  `what` as below.
inline int thermal_one_row_geometry(const cl_dims* dims, const cl_tuning& tun, const char* what, int& nw) {
    nw = tun.nw ? tun.nw : dims->n_bldg;
    if (nw > 16 || nw > dims->n_bldg || nw < dims->n_bldg)
        return fail(CL_EINVAL, "bad nw %d: the %s rollout runs one building per wave (nw = n_bldg = %d, at most 16)", nw, what, dims->n_bldg);
    return CL_OK;
}

// the thermal KPI kernels have no instantiation at two envs per lane (`what`: "thermal policy KPI", "chunked thermal policy KPI")
inline int one_env_per_lane_only(const cl_tuning& tun, const char* what) {
    if (tun.vec == 2) return fail(CL_EINVAL, "no %s rollout kernel at 2 envs per lane: it runs at one env per lane", what);
    if (tun.vec != 0 && tun.vec != 1) return fail(CL_EINVAL, "no %s rollout kernel at %d envs per lane", what, tun.vec);
    return CL_OK;
}

// the workgroup's dynamic LDS against what a CU has (`what`: "policy", "policy KPI", "thermal policy", ...)
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
