// cl_policy_full_chunk_kpi.h -- cl_kpi_series_chunk_kernel: the second of the three launches of one call of the building-chunked thermal policy
// rollout with the streaming KPIs (cl_policy_full.h, CHUNK + KPI: cl_rollout_full_policy_kernel<1, PREC, false, true, true> leaves the chunks'
// partial samples of the two district series in series_scratch; cl_finish_kernel follows).  Per env, both series (2 x 12 rows of kpi_env) through
// kpi_series_advance on the absolute step index t0 + k, the district sample of step k formed from the n_chunks partials in cl_finish_kernel's
// association -- sixteen strided partial sums (chunks j, j + 16, ..), then their sum in order -- which depends on n_chunks = f(n_bldg, b_chunk) and
// on nothing else: not on K, t0, the env block or how a caller cuts K steps into launches.  Included by cl_policy_full_chunk_kpi.hip only
// (libcitylearn_amd_policy_full_chunk_kpi.so, include/citylearn_amd_policy_full_chunk_kpi.h).
#pragma once
#include "cl_policy_full.h"

#ifdef __HIPCC__
namespace {

// The two district series of 64 envs per workgroup from the chunks' partial samples: series_scratch[k][2][n_chunks][n_env], k = 0 .. k_steps - 1.
// In batches of CL_SCK_BATCH steps: all sixteen waves form the district samples of the batch (one (step, series, env) per thread and pass, every
// load independent of every other: sixteen strided partial sums over the chunks, then their sum in order -- cl_finish_kernel's association), then
// wave 0 advances the control series and wave 1 the baseline series through the batch, serially, on their LDS copy (kpi_series_advance).
constexpr int CL_SCK_BATCH = 64;
__global__ void __launch_bounds__(1024) cl_kpi_series_chunk_kernel(const StepArgs a, const float* __restrict__ series_scratch, const int t0, const int k_steps) {
    __shared__ float smp[CL_SCK_BATCH * 2 * 64];                     // [step of the batch][series][env]
    __shared__ float ser[2 * CLKE_PER_COND * 64];                    // control series [12][64], then the baseline series [12][64]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int tile_env0 = blockIdx.x * 64;
    const bool mine = w < 2 && tile_env0 + lane < a.n_env;           // this thread keeps series w of env tile_env0 + lane
    if (mine) {
        KpiSeriesAll c;
        kpi_series_get(c, a.kpi_env + (long long)w * CLKE_PER_COND * a.n_env + tile_env0 + lane, a.n_env);
        kpi_series_put(ser + (size_t)w * CLKE_PER_COND * 64 + lane, 64, c);
    }
    for (int kb = 0; kb < k_steps; kb += CL_SCK_BATCH) {             // (uniform: the barriers depend on kb and k_steps only)
        const int nb = min(CL_SCK_BATCH, k_steps - kb);
        for (int i = threadIdx.x; i < nb * 2 * 64; i += blockDim.x) {
            const int e = i & 63, jc = i >> 6;                       // jc = 2 j + series
            float acc[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) acc[u] = 0.0f;
            if (tile_env0 + e < a.n_env) {
                const float* __restrict__ src = series_scratch + (((long long)kb * 2 + jc) * a.n_chunks) * a.n_env + tile_env0 + e;
                for (int c0 = 0; c0 < a.n_chunks; c0 += 16) {
#pragma unroll
                    for (int u = 0; u < 16; ++u) acc[u] += c0 + u < a.n_chunks ? src[(long long)(c0 + u) * a.n_env] : 0.0f;
                }
            }
            float v = 0.0f;
#pragma unroll
            for (int u = 0; u < 16; ++u) v += acc[u];
            smp[i] = v;
        }
        __syncthreads();
        if (mine) {
            for (int j = 0; j < nb; ++j) kpi_series_advance(ser + (size_t)w * CLKE_PER_COND * 64 + lane, 64, t0 + kb + j, smp[(j * 2 + w) * 64 + lane]);
        }
        __syncthreads();                                             // the batch's samples are free again
    }
    if (mine && k_steps > 0) {
        KpiSeriesAll c;
        kpi_series_get(c, ser + (size_t)w * CLKE_PER_COND * 64 + lane, 64);
        kpi_series_put(a.kpi_env + (long long)w * CLKE_PER_COND * a.n_env + tile_env0 + lane, a.n_env, c);
    }
}

}  // namespace
#endif  // __HIPCC__
