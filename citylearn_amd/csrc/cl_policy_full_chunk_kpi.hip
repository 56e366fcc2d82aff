// cl_policy_full_chunk_kpi.hip -- the translation unit of libcitylearn_amd_policy_full_chunk_kpi.so (include/citylearn_amd_policy_full_chunk_kpi.h):
// cl_kernels.hip reduced as for cl_policy_full_chunk.hip (CL_TU_POLICY, CL_TU_POLICY_FULL, and CL_TU_FINISH for cl_finish_kernel) with the table
// reads of cl_policy_full_kpi.hip (CL_TU_CONST_TABLES: the K loop holds barriers), cl_policy_full.h for the staged-row layout (its kernel template is
// never instantiated here), cl_policy_full_chunk_kpi.h's two kernels, their launcher and the `clpfck_*` entry points.  Compiled WITH SLP
// vectorisation like the other thermal units.
#define CL_TU_POLICY
#define CL_TU_CONST_TABLES     /* cl_unit.h: the parameter / time-series reads as scalar loads inside a K loop that holds barriers */
#define CL_TU_POLICY_FULL
#define CL_TU_FINISH
#include "cl_kernels.hip"
#include "../../include/citylearn_amd_policy_full_chunk_kpi.h"
#include "cl_policy_full_chunk_kpi.h"

namespace {

// the launcher of the rollout kernel; key = PREC
int launch_policy_full_chunk_kpi(int prec, dim3 grid, unsigned block, size_t lds, hipStream_t s, const PolicyArgs& p, float* series_scratch) {
#define CL_POLFCK(P) do { \
        if (lds > 64 * 1024) if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(cl_rollout_full_policy_chunk_kpi_kernel<P>), lds); e != hipSuccess) return (int)e; \
        hipLaunchKernelGGL((cl_rollout_full_policy_chunk_kpi_kernel<P>), grid, dim3(block), lds, s, p, series_scratch); } while (0)
    switch (prec) {
    case 0: CL_POLFCK(0); break;
    case 2: CL_POLFCK(2); break;
    default: return (int)hipErrorInvalidValue;
    }
#undef CL_POLFCK
    return (int)hipGetLastError();
}

// the chunk geometry of clpfc_rollout_mlp_f32 (ONE building per wave, b_chunk buildings = waves per workgroup row, n_chunks rows along gridDim.y;
// default: balanced chunks of at most EIGHT), with its refusals
int chunk_geometry(const cl_dims* dims, const cl_tuning& tun, int& b_chunk, int& n_chunks) {
    if (tun.b_chunk < 0) return fail(CL_EINVAL, "b_chunk=%d", tun.b_chunk);
    if (tun.b_chunk > 16) return fail(CL_EINVAL, "b_chunk=%d: a thermal policy rollout workgroup holds at most 16 buildings (one per wave)", tun.b_chunk);
    if (tun.b_chunk == 0 && dims->n_bldg <= 16)
        return fail(CL_EINVAL, "clpfck_rollout_mlp_kpi_f32: n_bldg=%d fits one workgroup row, which is clpfk_rollout_mlp_kpi_f32's launch (libcitylearn_amd_policy_full_kpi.so); "
                               "a chunked launch of it takes an explicit cl_tuning.b_chunk < n_bldg", dims->n_bldg);
    if (tun.b_chunk >= dims->n_bldg)
        return fail(CL_EINVAL, "b_chunk=%d >= n_bldg=%d: one workgroup row is clpfk_rollout_mlp_kpi_f32's launch (libcitylearn_amd_policy_full_kpi.so)", tun.b_chunk, dims->n_bldg);
    if (tun.b_chunk > 0) {
        b_chunk = tun.b_chunk;
    } else {
        const int nc = (dims->n_bldg + 7) / 8;
        b_chunk = (dims->n_bldg + nc - 1) / nc;
    }
    n_chunks = (dims->n_bldg + b_chunk - 1) / b_chunk;
    if (tun.nw != 0 && tun.nw != b_chunk)
        return fail(CL_EINVAL, "bad nw %d: the chunked thermal policy KPI rollout runs one building per wave (nw = b_chunk = %d)", tun.nw, b_chunk);
    // the reserved plane holds n_chunks x NQ partial sums, one return row per chunk and, at its tail, the ticket and marker words of the step launches
    if (((long long)n_chunks * (NQ + 1)) * dims->n_env + (dims->n_env + 63) / 64 + 4 > (long long)dims->n_bldg * dims->n_env)
        return fail(CL_EINVAL, "b_chunk=%d leaves no room for the %d chunk partial sums of the fused rollout", b_chunk, n_chunks);
    return CL_OK;
}

}  // namespace

extern "C" {

int clpfck_abi_version(void) { return CLPFCK_ABI_VERSION; }
int clpfck_core_abi_version(void) { return CL_ABI_VERSION; }
const char* clpfck_last_error(void) { return g_err; }

int64_t clpfck_series_scratch_floats(const cl_dims* dims, int32_t k_steps) {
    if (int rc = check_dims(dims, false)) return -(int64_t)rc;
    if (k_steps < 0) return -(int64_t)fail(CL_ERANGE, "k_steps=%d", k_steps);
    const cl_tuning& tun = dims->tuning ? *dims->tuning : cl_tuning{};
    int b_chunk = 0, n_chunks = 0;
    if (int rc = chunk_geometry(dims, tun, b_chunk, n_chunks)) return -(int64_t)rc;
    return (int64_t)k_steps * 2 * n_chunks * dims->n_env;
}

int clpfck_rollout_mlp_kpi_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const clpf_mlp* mlp,
                               float* out_bldg, float* out_env, float* ret_env, float* traj, float* kpi_bldg, float* kpi_env,
                               float* series_scratch, int64_t scratch_floats, int32_t t0, int32_t k_steps, void* stream) {
    if (int rc = check_dims(dims, false)) return rc;
    const uint32_t rk = (dims->flags & CLD_REWARD_MASK) >> CLD_REWARD_SHIFT;
    // ---- what the kernel covers ----
    if (dims->flags & CLD_LEAN)
        return fail(CL_EINVAL, "clpfck_rollout_mlp_kpi_f32: thermal / outage districts only; a battery + PV district (CLD_LEAN) goes to clpk_rollout_mlp_kpi_f32 (libcitylearn_amd_policy_kpi.so)");
    if (!(dims->flags & CLD_KPI))
        return fail(CL_EINVAL, "clpfck_rollout_mlp_kpi_f32: the district must keep the streaming KPIs (CLD_KPI); without them the call is clpfc_rollout_mlp_f32");
    if (rk == CLR_MARL)
        return fail(CL_EINVAL, "clpfck_rollout_mlp_kpi_f32: reward kind CLR_MARL: a building-chunked launch cannot couple the buildings inside a step");
    if (rk == CLR_EV) return fail(CL_EINVAL, "clpfck_rollout_mlp_kpi_f32: reward kind CLR_EV needs the flexible-load tables");
    if (dims->flags & CLD_F64_MAPS)
        return fail(CL_EINVAL, "clpfck_rollout_mlp_kpi_f32: the battery map in fp32 or as the float64 chain (CLD_F64_CHAIN), not CLD_F64_MAPS");
    if ((dims->flags & CLD_WRITE_DETAIL) && !(dims->flags & CLD_DETAIL_MIN))
        return fail(CL_EINVAL, "clpfck_rollout_mlp_kpi_f32: of the detail planes (CLD_WRITE_DETAIL) only the subset of CLD_DETAIL_MIN is written");
    if (int rc = no_pitch(dims, "clpfck_rollout_mlp_kpi_f32")) return rc;
    if (dims->n_act_cols > 65536) return fail(CL_EINVAL, "clpfck_rollout_mlp_kpi_f32: n_act_cols=%d > 65536", dims->n_act_cols);
    if (!mlp) return fail(CL_ENULL, "mlp is NULL");
    if (mlp->n_device_cols != 0)
        return fail(CL_EINVAL, "clpfck_rollout_mlp_kpi_f32: n_device_cols=%d: a building with a cooling / heating / combined device action column is not covered "
                               "(the policy has storage heads only)", mlp->n_device_cols);
    if (int rc = check_policy_sizes(*mlp, CLPF_MAX_HIDDEN)) return rc;
    if (mlp->reserved) return fail(CL_EINVAL, "clpf_mlp.reserved must be 0");
    const PolicyCall call = {params, ts, state, out_bldg, out_env, ret_env, traj, kpi_bldg, kpi_env, t0, k_steps};
    if (int rc = check_policy_buffers(dims, *mlp, call, true)) return rc;
    if (int rc = check_ptr(series_scratch, "series_scratch")) return rc;

    const cl_tuning& tun = dims->tuning ? *dims->tuning : cl_tuning{};
    PolicyArgs p;
    fill_policy_args(p, dims, *mlp, CLPF_NOISE_KEY, call);
    StepArgs& a = p.r.s;
    if (int rc = chunk_geometry(dims, tun, a.b_chunk, a.n_chunks)) return rc;
    a.nw = a.b_chunk;
    const long long need = (long long)k_steps * 2 * a.n_chunks * dims->n_env;
    if (scratch_floats < need)
        return fail(CL_EINVAL, "series_scratch holds %lld floats; %d steps x 2 series x %d chunks x %d envs need %lld (clpfck_series_scratch_floats)",
                    (long long)scratch_floats, k_steps, a.n_chunks, dims->n_env, need);
    if (tun.vec == 2) return fail(CL_EINVAL, "no chunked thermal policy KPI rollout kernel at 2 envs per lane: it runs at one env per lane");
    if (tun.vec != 0 && tun.vec != 1) return fail(CL_EINVAL, "no chunked thermal policy KPI rollout kernel at %d envs per lane", tun.vec);
    const bool chain = dims->flags & CLD_F64_CHAIN;
    const size_t lds = rollout_full_policy_chunk_kpi_lds_floats(a.nw) * sizeof(float);
    if (int rc = check_policy_lds(lds, "chunked thermal policy KPI", a.nw, 1)) return rc;
    const int prec = chain ? 2 : 0;
    const hipStream_t s = (hipStream_t)stream;
    name_reset(tun);
    name_add(tun, "cl_rollout_full_policy_chunk_kpi_kernel<%d>", prec);
    const dim3 grid((unsigned)((dims->n_env + 63) / 64), (unsigned)a.n_chunks);
    const int rc = launch_policy_full_chunk_kpi(prec, grid, 64u * a.nw, lds, s, p, series_scratch);
    if (rc) return hip_fail((hipError_t)rc, "cl_rollout_full_policy_chunk_kpi_kernel launch");
    if (k_steps > 0) {
        // the two district series of every env from the chunks' partial samples
        name_add(tun, "cl_kpi_series_chunk_kernel");
        hipLaunchKernelGGL(cl_kpi_series_chunk_kernel, dim3((dims->n_env + 63) / 64), dim3(1024), 0, s, a, (const float*)series_scratch, (int)t0, (int)k_steps);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_fail(e, "cl_kpi_series_chunk_kernel launch");
        // the last step's district sums (and the K-step return): one fold per call, as behind clpfc_rollout_mlp_f32
        StepArgs f = a;
        f.t = t0 + k_steps - 1;
        name_add(tun, "cl_finish_kernel");
        hipLaunchKernelGGL(cl_finish_kernel, dim3((dims->n_env + 63) / 64, NQ + (ret_env ? 1 : 0)), dim3(1024), 0, s, f, 0, ret_env);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_fail(e, "cl_finish_kernel launch");
    }
    return CL_OK;
}

}  // extern "C"
