// cl_policy_full_chunk_kpi.hip -- the translation unit of libcitylearn_amd_policy_full_chunk_kpi.so (include/citylearn_amd_policy_full_chunk_kpi.h):
// cl_kernels.hip reduced as for cl_policy_full_chunk.hip (CL_TU_POLICY, CL_TU_POLICY_FULL, and CL_TU_FINISH for cl_finish_kernel) with the table
// reads of cl_policy_full_kpi.hip (CL_TU_CONST_TABLES: the K loop holds barriers), cl_policy_full.h's kernel template under its KPI and CHUNK switches (one env
// per lane), cl_policy_full_chunk_kpi.h's series kernel, their launcher and the `clpfck_*` entry points.  Compiled WITH SLP
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
int launch_policy_full_chunk_kpi(int prec, dim3 grid, unsigned block, size_t lds, hipStream_t s, const FullPolicyChunkKpiArgs& p) {
#define CL_POLFCK(P) CL_POLICY_LAUNCH(cl_rollout_full_policy_kernel<1, P, false, true, true>)
    switch (prec) {
    case 0: CL_POLFCK(0); break;
    case 2: CL_POLFCK(2); break;
    default: return (int)hipErrorInvalidValue;
    }
#undef CL_POLFCK
    return (int)hipGetLastError();
}

// the chunk geometry of clpfc_rollout_mlp_f32 (ONE building per wave, so b_chunk buildings = waves per workgroup row) with its refusals, for the
// rollout and for the scratch size that goes with it
int chunk_geometry(const cl_dims* dims, const cl_tuning& tun, int& b_chunk, int& n_chunks) {
    const ChunkRule rule = {1, "clpfck_rollout_mlp_kpi_f32", "clpfk_rollout_mlp_kpi_f32", "libcitylearn_amd_policy_full_kpi.so"};
    if (int rc = policy_chunk_geometry(dims, tun, rule, b_chunk, n_chunks)) return rc;
    if (tun.nw != 0 && tun.nw != b_chunk)
        return fail(CL_EINVAL, "bad nw %d: the chunked thermal policy KPI rollout runs one building per wave (nw = b_chunk = %d)", tun.nw, b_chunk);
    return check_chunk_partials(b_chunk, n_chunks, dims);
}

}  // namespace

extern "C" {

CL_POLICY_ABI(clpfck, CLPFCK_ABI_VERSION)

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
    const char* const entry = "clpfck_rollout_mlp_kpi_f32";
    if (int rc = check_dims(dims, false)) return rc;
    // ---- what the kernel covers ----
    if (dims->flags & CLD_LEAN)
        return fail(CL_EINVAL, "clpfck_rollout_mlp_kpi_f32: thermal / outage districts only; a battery + PV district (CLD_LEAN) goes to clpk_rollout_mlp_kpi_f32 (libcitylearn_amd_policy_kpi.so)");
    if (!(dims->flags & CLD_KPI))
        return fail(CL_EINVAL, "clpfck_rollout_mlp_kpi_f32: the district must keep the streaming KPIs (CLD_KPI); without them the call is clpfc_rollout_mlp_f32");
    if (int rc = no_chunked_marl(dims, entry)) return rc;
    if (int rc = no_reward_ev(dims, entry)) return rc;
    if (int rc = no_f64_maps(dims, entry)) return rc;
    if (int rc = detail_min_only(dims, entry)) return rc;
    if (int rc = no_pitch(dims, entry)) return rc;
    if (int rc = check_thermal_policy_mlp(entry, dims, mlp)) return rc;
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
    if (int rc = one_env_per_lane_only(tun, "chunked thermal policy KPI")) return rc;
    const bool chain = dims->flags & CLD_F64_CHAIN;
    const size_t lds = rollout_full_policy_chunk_kpi_lds_floats(a.nw) * sizeof(float);
    if (int rc = check_policy_lds(lds, "chunked thermal policy KPI", a.nw, 1)) return rc;
    const int prec = chain ? 2 : 0;
    const hipStream_t s = (hipStream_t)stream;
    name_reset(tun);
    name_add(tun, "cl_rollout_full_policy_chunk_kpi_kernel<%d>", prec);
    const dim3 grid((unsigned)((dims->n_env + 63) / 64), (unsigned)a.n_chunks);
    const int rc = launch_policy_full_chunk_kpi(prec, grid, 64u * a.nw, lds, s, {p, series_scratch});
    if (rc) return hip_fail((hipError_t)rc, "cl_rollout_full_policy_chunk_kpi_kernel launch");
    if (k_steps > 0) {
        // the two district series of every env from the chunks' partial samples
        name_add(tun, "cl_kpi_series_chunk_kernel");
        hipLaunchKernelGGL(cl_kpi_series_chunk_kernel, dim3((dims->n_env + 63) / 64), dim3(1024), 0, s, a, (const float*)series_scratch, (int)t0, (int)k_steps);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_fail(e, "cl_kpi_series_chunk_kernel launch");
        // the last step's district sums (and the K-step return): one fold per call, as behind clpfc_rollout_mlp_f32
        return launch_rollout_finish(tun, a, t0 + k_steps - 1, ret_env, s);
    }
    return CL_OK;
}

}  // extern "C"
