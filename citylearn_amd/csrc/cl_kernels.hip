// cl_kernels.hip -- HIP kernels (gfx950 / CDNA4) + the extern "C" boundary declared in include/citylearn_amd.h.
//
// Work decomposition ("2-D tile"): a workgroup owns ENV_TILE = 64*VEC consecutive envs and ALL buildings of
// the district.  Wave w of the workgroup advances buildings w, w+NW, w+2NW, ... so that the building index is
// wave-uniform: its parameter block and its time-series row are fetched with scalar loads into SGPRs, and the
// 64 lanes of the wave touch 64*VEC consecutive floats of every state / action / output plane (one fully
// coalesced request per plane).  District sums over buildings (net, cost, emission, reward) are reduced
// through LDS in a fixed order (wave-partials -> serial sum over waves), so results are bit-reproducible
// run to run -- no atomics on the step path.
#include "cl_trace.h"
#include "cl_unit.h"
#include "cl_plan.h"
#ifndef CL_LEAN_NT_LOADS
#define CL_LEAN_NT_LOADS true          // A/B build flag: false = no non-temporal hint on any plane load of the latency-ordered lean kernels (lean_step_body's note)
#endif
#ifndef CL_LEAN_ONE_EACH
#define CL_LEAN_ONE_EACH true          // A/B build flag: false = the headline's district sums through the reducer's general loop (district_reduce, STRIPS)
#endif
#include "cl_philox.h"

#include <type_traits>
#include <mutex>
#include <stdarg.h>
#include <string.h>
#include <stdio.h>

namespace {

int hip_fail(hipError_t e, const char* what) {
    return fail(CL_EHIP, "%s: %s", what, hipGetErrorString(e));
}

// Opt a kernel into more than the default 64 KB of dynamic LDS, ONCE per (kernel, device, size): hipFuncSetAttribute is a driver call, and
// the launches that need it (building-chunked 1024-building districts) sit on the per-step path (round-5 advisor finding).  The table only
// remembers what the driver has already been told -- idempotent, so it is not state a caller could observe.
hipError_t ensure_dynamic_lds(const void* fn, size_t bytes) {
    struct Seen { const void* fn; int dev; size_t bytes; };
    static Seen seen[64];
    static int n_seen = 0;
    static std::mutex mu;
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    for (int i = 0; i < n_seen; ++i)
        if (seen[i].fn == fn && seen[i].dev == dev && seen[i].bytes >= bytes) return hipSuccess;
    if (hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes); e != hipSuccess) return e;
    for (int i = 0; i < n_seen; ++i)
        if (seen[i].fn == fn && seen[i].dev == dev) { seen[i].bytes = bytes; return hipSuccess; }
    if (n_seen < 64) seen[n_seen++] = {fn, dev, bytes};
    return hipSuccess;
}

// Two envs per lane of a fused rollout where its 128-env workgroups come in (nearly) full rounds of one per CU: 17 x 32 768 (the C5 per-GPU shard)
// 2.60 -> 2.31 us per step, 65 536 4.99 -> 4.19, 98 304 7.24 -> 6.19, 131 072 9.54 -> 8.21; 49 152 = 1.5 rounds: 4.20 vs 3.89 at one env per lane
// (scripts/rollout_vec_probe.py).  A building-chunked launch has env tiles x chunks workgroups; one workgroup row is n_chunks = 1, where
// n_env >= 32 768 makes the last term true.  The ONE copy: cl_rollout_f32, the fused KPI rollout and the lean policy rollouts (cl_policy.h,
// cl_policy_chunk.hip) all pick their envs per lane by it.
inline bool full_rounds(int n_env, int n_chunks) {
    const long long wg2 = (long long)((n_env + 127) / 128) * n_chunks, rounds2 = (wg2 + 255) / 256;
    return (long long)n_env * n_chunks >= 32768 && wg2 * 100 >= rounds2 * 256 * 85 && n_env >= 128;
}

// out_bldg's reserved plane has room for what a building-chunked fused rollout parks there: n_chunks x NQ partial sums, one return row per chunk
// and, at its tail, the marker words (and, in front of those, the ticket words of the one-step launches' in-launch fold: they stay zero between
// launches).  cl_rollout_f32 and the three chunked policy entries refuse a geometry that does not fit -- in the same words, so the refusal is here too.
inline bool chunk_partials_fit(int n_chunks, const cl_dims* dims) {
    return ((long long)n_chunks * (CL_NQ + 1)) * dims->n_env + (dims->n_env + 63) / 64 + 4 <= (long long)dims->n_bldg * dims->n_env;
}
inline int check_chunk_partials(int b_chunk, int n_chunks, const cl_dims* dims) {
    if (!chunk_partials_fit(n_chunks, dims))
        return fail(CL_EINVAL, "b_chunk=%d leaves no room for the %d chunk partial sums of the fused rollout", b_chunk, n_chunks);
    return CL_OK;
}

struct StepArgs {
    const uint32_t* __restrict__ params;
    const float* __restrict__ ts;
    float* __restrict__ state;
    const float* __restrict__ actions;
    float* __restrict__ out_bldg;
    float* __restrict__ out_env;
    float* __restrict__ kpi_bldg;
    float* __restrict__ kpi_env;
    long long act_stride_col, act_stride_env;
    const int32_t* __restrict__ env_row0;   // per-env-block episode offsets (cl_dims.env_row0) or null
    const float* __restrict__ flex_out;     // cl_flex.flex_out planes [CL_NX][n_flex_bldg][n_env] or null (cl_flex.h)
    int n_flex_bldg;
    unsigned env_offset;                    // cl_dims.env_offset (low 32 bits: the Philox counter word)
    float ev_penalty_coef;                  // > 0: some building has charging constraints; CLR_EV subtracts coef * violation
    int n_env, n_bldg, n_steps;
    int ld;        // floats between consecutive building rows of the state / out_bldg planes (cl_dims.env_pitch; = n_env unless padded).  (In the slot of
                   // the action-column count, which no kernel reads: one more word in this struct cost every detail kernel a scratch reservation)
    uint32_t flags;
    int t;
    int nw;        // waves per workgroup == building lanes
    int b_chunk;   // buildings per workgroup row (gridDim.y = n_chunks rows); == n_bldg when the grid is 1-D
    int n_chunks;
    int nt;        // plane stores carry the non-temporal hint (see pstore)
    int fused_finish;   // building-chunked launches: the last chunk of an env tile folds the chunk partial sums itself (district_reduce)
};

// StepArgs::flags, library-internal (not a CLD_* bit a caller can set: step_impl clears it, then sets it from StepPlan::strips -- with the LDS row
// the strips need): the uniform body of cl_step_lean_chain_kernel<4, ..> shares the building beyond the waves out as strips (lean_step_body, STRIPS)
constexpr uint32_t CLA_LEAN_STRIPS = (uint32_t)1 << 31;

constexpr int CL_OBS_FUSED_PER_BLDG = 4;      // observation columns per building the step launch writes itself

template <int VEC> struct Vec;
template <> struct Vec<1> { using type = float; };
template <> struct Vec<2> { using type = float __attribute__((ext_vector_type(2))); };
template <> struct Vec<4> { using type = float __attribute__((ext_vector_type(4))); };

template <int VEC>
CL_DEV void vload(float (&dst)[VEC], const float* __restrict__ p) {
    using V = typename Vec<VEC>::type;
    const V v = *reinterpret_cast<const V*>(p);
    if constexpr (VEC == 1) dst[0] = v;
    else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) dst[i] = v[i];
    }
}

// Load from a state / action plane in HBM; NT as in pstore (measured together with the nt stores on cl_step_lean_kernel in round 2,
// 17 x 65 536: 7.32 -> 7.18 us; the copy-floor pattern of scripts/launch_gap.py: 5.65 -> 5.41 us -- and measured AGAIN in round 5, where
// the hint costs the headline instantiation 1 us: which instantiations keep it is lean_step_body's `NTL`).
template <int VEC, bool NT>
CL_DEV void pload(float (&dst)[VEC], const float* __restrict__ p) {
    if constexpr (NT) {
        using V = typename Vec<VEC>::type;
        const V v = __builtin_nontemporal_load(reinterpret_cast<const V*>(p));
        if constexpr (VEC == 1) dst[0] = v;
        else {
#pragma unroll
            for (int i = 0; i < VEC; ++i) dst[i] = v[i];
        }
    } else vload<VEC>(dst, p);
}

template <int VEC>
CL_DEV void vstore(float* __restrict__ p, const float (&src)[VEC]) {
    using V = typename Vec<VEC>::type;
    V v;
    if constexpr (VEC == 1) v = src[0];
    else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[i] = src[i];
    }
    *reinterpret_cast<V*>(p) = v;
}

// Store to a state / output plane in HBM (never LDS).  NT = non-temporal (`global_store ... nt`): the lines stream through the
// XCD's L2 instead of staying dirty in it until the end-of-kernel release writes them back.  scripts/launch_gap.py: for the
// headline shape's access pattern (17.8 MB in, 22.3 MB out) the waves are alive 2.9 us either way, but the gap to the next launch's
// first wave is 3.2 us with plain stores and 2.7 us with nt ones (1.1 us for a read-only kernel, 1.8 us period for an empty one);
// cl_step_lean_kernel 17 x 65 536: 7.91 -> 7.20 us.  With a footprint of the order of the 256 MB Infinity Cache the hint costs bandwidth
// instead (17 x 262 144: +10 %), several times past it it wins again (17 x 1 048 576: 125 -> 115 us): the host sets StepArgs::nt by size.
template <int VEC, bool NT>
CL_DEV void pstore(float* __restrict__ p, const float (&src)[VEC]) {
    using V = typename Vec<VEC>::type;
    V v;
    if constexpr (VEC == 1) v = src[0];
    else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[i] = src[i];
    }
    if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<V*>(p));
    else *reinterpret_cast<V*>(p) = v;
}
struct NtOn { static constexpr bool value = true; };
struct NtOff { static constexpr bool value = false; };

// action element (col, env): coalesced when act_stride_env == 1
template <int VEC>
CL_DEV void load_action(float (&dst)[VEC], const StepArgs& a, int col, int env0) {
    if (col < 0) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) dst[i] = 0.0f;
        return;
    }
    const float* p = a.actions + (long long)col * a.act_stride_col;
    if (a.act_stride_env == 1) vload<VEC>(dst, p + env0);
    else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) dst[i] = p[(long long)(env0 + i) * a.act_stride_env];
    }
}

#include "cl_flex.h"     // flexible loads (EV chargers, EVs, washing machines): device functions + the stand-alone kernel

constexpr int NQ = CL_NQ;

// District sums over buildings: wave partials -> LDS -> fixed-order serial sum over waves (deterministic).
// `stride` is the building stride used by the caller's loop (needed by the MARL second sweep).
// FOLD: instantiations that are launched building-chunked may finish the chunk sums themselves (a.fused_finish); a template parameter
// because the fold's sixteen loads in flight would otherwise set the register budget of every kernel this is inlined into (the general
// lean kernel went from 52 to 102 VGPRs).
// (streaming KPIs, below)  One more sample of a district series costs ONE round trip: the seven accumulators that move every step are
// fetched together (kpi_series_fetch -- where the caller can, before a barrier it has to wait at anyway), then updated and stored
// (kpi_series_apply).  As `k[..] += ..` statements one after the other -- what rounds 1 - 3 had -- every load waits for the store in
// front of it (the compiler cannot tell the planes apart): five dependent round trips at the very end of every workgroup.
struct KpiSeries { float prev, ramp, dsum, dmax, msum, mmax, amax; };
CL_DEV void kpi_series_fetch(KpiSeries& s, const float* __restrict__ k, long long n_env);
CL_DEV void kpi_series_apply(float* __restrict__ k, long long n_env, int t, float v, const KpiSeries& s);
CL_DEV void kpi_series_update(float* __restrict__ k, long long n_env, int t, float v);

// DEFERRED FINISH (cl_tuning.finish = 3, a.fused_finish == 2), the fold half: every workgroup of a building-chunked launch adds up
// `opw` <= 16 district sums (quantity, env) of the PREVIOUS step out of scratch buffer (t + 1) & 1 -- n_chunks x opw partial sums -- in
// cl_finish_kernel's association and writes them to out_env.  What was tried, on the 1024 x 1024 shards (rocprofv3 averages of the step
// kernel, thermal / battery + PV; 11.5 / 7.8 us without any fold):
//  1. one district sum per wave, lane = chunk (a 64-line gather), fetched inside district_reduce behind the plane stores: 13.5 us -- on
//     gfx9 vector loads and stores share one counter and return out of order with respect to each other, so a load waited for after
//     stores were issued waits for their acknowledgements too;
//  2. the same gather fetched at the very top of the kernel: 13.9 / 9.7 us;  3. fetched behind the first building's plane loads and
//     consumed before its stores: 14.1 / 9.8 us -- so not a placement problem: the sixteen waves of a workgroup each gathered 4 bytes
//     out of the SAME 64 lines (16 consecutive envs of 64 chunk rows), 262 144 line requests per launch for 1 MB of data;
//  4. (this one) every line is requested once: thread i of the workgroup fetches partial sum (chunk i / 16, district sum i % 16) -- a
//     wave reads four 64-byte segments -- issued behind the first building's plane loads, parked in LDS before the wave's first store,
//     and added up behind district_reduce's first barrier: wave w takes district sum w, lanes 0..15 form the sixteen wave-partials of
//     cl_finish_kernel (chunks k, k + 16, k + 32, k + 48), then their sum in order: 14.4 / 8.8 us.  Piece by piece on one box
//     (profiles/r04_c4_fold_breakdown.log; 13.0 / 7.8 us with the second launch, whose own 4 - 5 us mostly overlap the next step):
//     double-buffered rows + marker only 13.7 / 8.1 -- step launches now run back to back, each starting into the previous one's
//     draining stores; + load and stash 14.9 / 8.4; + add-up without the load 14.4 / 8.6; everything 15.3 / 9.0.
// (`bx`, `by`: the workgroup's env tile and building chunk -- blockIdx.x / .y)
// (round 5) The exchange tile is [n_chunks][W] with W = 16, 32 or 64 district sums per workgroup row (`opw` rounded up; n_chunks x W <= 1024 =
// one value per thread of the 16-wave workgroup: host): launches with FEWER, LARGER chunks defer too -- the whole BASELINE config 4 on one GPU
// runs 8 chunks of 128 buildings (91 vs 103 us with 32 chunks of 32), where a workgroup row folds 64 sums, four per wave.
CL_DEV int fold_shift(int opw) { return opw <= 16 ? 4 : opw <= 32 ? 5 : 6; }
template <int TILE>
CL_DEV float fold_prefetch(const StepArgs& a, int w, int lane, long long plane, int bx, int by) {
    if (a.fused_finish != 2) return 0.0f;
    const int opw = (NQ * TILE + a.n_chunks - 1) / a.n_chunks;           // district sums of an env tile per workgroup row (<= 64: host)
    const int sh = fold_shift(opw);
    const int i = w * 64 + lane, chunk = i >> sh, j = i & ((1 << sh) - 1), o = by * opw + j;
    const int e = bx * TILE + o % TILE;
    if (chunk < a.n_chunks && j < opw && o < NQ * TILE && e < a.n_env)
        return a.out_bldg[(long long)CLO_RESERVED * plane + ((long long)((a.t + 1) & 1) * a.n_chunks + chunk) * NQ * a.n_env + (long long)(o / TILE) * a.n_env + e];
    return 0.0f;
}
CL_DEV void fold_stash(const StepArgs& a, float* lds_fold, int w, int lane, float v) {
    if (a.fused_finish == 2 && w < 16) lds_fold[w * 64 + lane] = v;        // [n_chunks][W district sums]
}
template <int TILE>
CL_DEV void fold_finish(const StepArgs& a, const float* lds_fold, int w, int lane, int bx, int by) {
    const int opw = (NQ * TILE + a.n_chunks - 1) / a.n_chunks;
    const int sh = fold_shift(opw);
    const int k = lane & 15;
    for (int j = w; j < opw; j += 16) {                                  // wave-uniform: district sums w, w + 16, ... of the row
        const int o = by * opw + j;
        if (o >= NQ * TILE || bx * TILE + o % TILE >= a.n_env) continue;
        float pk = 0.0f;
        if (k < a.n_chunks) {
#pragma unroll
            for (int c = 0; c < 4; ++c) pk += k + 16 * c < a.n_chunks ? lds_fold[((k + 16 * c) << sh) + j] : 0.0f;
        }
        float tot = 0.0f;
#pragma unroll
        for (int q = 0; q < 16; ++q) tot += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, pk), q));
        if (lane == 0) a.out_env[(long long)(o / TILE) * a.n_env + bx * TILE + o % TILE] = tot;
    }
}

// KPIS: the thread that writes an env's district net also feeds it to the env's streaming district accumulators (CLD_KPI, lean districts)
// PRESTORED: the caller has kept the wave's partial sums in its LDS row all along (cl_full.h, the C4 shard's kernel: four accumulators fewer in
// registers across the buildings of a wave) -- q_* are not read.
// Grids are (env tiles, building chunks).  Round 5 measured the chunk-major grid, (building chunks, env tiles), and dropped it.  Workgroups go
// to the eight XCDs round-robin in x-major order: with the env tiles along x every XCD steps one tile of EVERY chunk and fetches every building's parameter block and table row into its own L2 (C4 shard: 8 x 327 KB per step); with the
// chunks along x an XCD owns a few chunks for all their env tiles.  The counters confirm the traffic -- C4 shard 64.68 -> 62.46 MB per step =
// 1.039 x algorithmic -- and the clock says no: alternating builds on one box (profiles/r05e_*), thermal shard 13.12 - 13.15 us tile-major
// against 13.66 - 13.76 us chunk-major, battery + PV shard 8.80 - 8.84 against 9.00 - 9.75 us, the whole thermal config (1024 x 8192) 101.0
// against 109.9 us.  An XCD that owns four chunks touches 128 building rows of every plane instead of all 1024: its requests crowd a
// fraction of the rows the memory system interleaves over, and 2 MB of parameter re-reads (L2 misses that the Infinity Cache serves) were
// never on the critical path.
// STRIPS (lean_step_body's uniform body): with `strip_row` set, LDS row a.nw -- behind the wave rows -- holds the four quantities of building a.nw, written by the
// strip waves before the first barrier, and row 0 holds building 0 alone.  The sum starts from that row instead of from zero: (row_nw + row_0) + row_1 + ..,
// where wave 0 with two tiles gives (0 + row_0') + row_1 + .. with row_0' = (0 + b_0) + b_nw.  Same bits: row_0 = 0 + b_0 and row_nw = b_nw, the addition
// commutes, and 0 + row_0' = row_0' because row_0' is never -0 -- 0 + b_0 is not (+0 + -0 = +0 in round-to-nearest), and a sum with a term that is not -0 is not.
template <int VEC, bool FLEX = false, bool FOLD = false, bool KPIS = false, bool PRESTORED = false, bool STRIPS = false>
CL_DEV void district_reduce(const StepArgs& a, float* lds, int w, int lane, int env0, bool live, long long plane, int rkind,
                            const float (&q_net)[VEC], const float (&q_cost)[VEC], const float (&q_em)[VEC],
                            const float (&q_rw)[VEC], int stride, [[maybe_unused]] const float* lds_fold = nullptr,
                            [[maybe_unused]] bool strip_row = false) {
    constexpr int TILE = 64 * VEC;
    const int bx = blockIdx.x, by = blockIdx.y;       // env tile, building chunk
    if constexpr (!PRESTORED) {
        float* mine = lds + (size_t)w * NQ * TILE + lane * VEC;
        vstore<VEC>(mine + 0 * TILE, q_net);
        vstore<VEC>(mine + 1 * TILE, q_cost);
        vstore<VEC>(mine + 2 * TILE, q_em);
        vstore<VEC>(mine + 3 * TILE, q_rw);
    }
    const int tile_env0 = bx * TILE;
    // (STRIPS: the uniform body at four envs per lane, default reward) One workgroup row of sixteen waves -- the headline -- has exactly one district
    // sum per thread.  Its LDS column and its out_env address are worked out in FRONT of the barrier; behind it stand the strip row's read, sixteen
    // wave-row reads issued back to back, the adds in the loop's order (strip row first, then rows 0 .. 15: the same bits) and one store.  The loop
    // below spends about a hundred instructions behind the barrier on that one sum: it fetches the block-size argument (a scalar round trip), sets up
    // two nested loops for a trip count of one, and waits after every pair of reads.  Sixteen waves are known from a.nw, which the wave holds already.
    // Any other geometry takes the loop.  (The two values are made opaque in front of the barrier: left alone, the compiler sinks their arithmetic
    // behind it.  The address as an index into out_env -- a pointer would come out of the asm statement as a generic one, a flat store.  -1: an env
    // beyond the batch.)
    [[maybe_unused]] bool one_each = false;
    [[maybe_unused]] long long one_out = -1;
    [[maybe_unused]] uint32_t one_i = 0;
    if constexpr (STRIPS) {
        one_each = CL_LEAN_ONE_EACH && a.n_chunks == 1 && a.nw * 64 == NQ * TILE;
        one_i = threadIdx.x;
        const uint32_t q = one_i / TILE, e = one_i % TILE;
        one_out = tile_env0 + (int)e < a.n_env ? (long long)q * a.n_env + tile_env0 + e : -1;
        asm volatile("" : "+v"(one_out), "+v"(one_i));
    }
    // (KPIS) the control series' accumulators of the env whose district net this thread is about to write: in flight across the barrier
    [[maybe_unused]] KpiSeries pre;
    if constexpr (KPIS) {
        if (threadIdx.x < TILE && tile_env0 + (int)threadIdx.x < a.n_env) kpi_series_fetch(pre, a.kpi_env + tile_env0 + threadIdx.x, a.n_env);
    }
    __syncthreads();
    const bool coupled = rkind == CLR_MARL || (FLEX && rkind == CLR_EV);   // rewards that need the district net
    if constexpr (STRIPS) {
        if (one_each && !coupled) {
            const float* col = lds + one_i;
            const float x = col[strip_row ? (size_t)16 * NQ * TILE : 0];       // (without a strip row: row 0 once more, not used)
            float r[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) r[k] = col[(size_t)k * NQ * TILE];
            __builtin_amdgcn_sched_barrier(0);                                 // every read is issued before the first add
            float s = strip_row ? x : 0.0f;
#pragma unroll
            for (int k = 0; k < 16; ++k) s += r[k];
            if (one_out >= 0) a.out_env[one_out] = s;
            return;
        }
    }
    if (a.n_chunks > 1) {
        // Large districts: this workgroup only saw buildings [y*b_chunk, (y+1)*b_chunk).  Its partial sums go to the scratch rows of
        // out_bldg's reserved plane; cl_finish_kernel (a second launch, 4.8 us of pure latency) adds the chunks in a fixed order.
        // The alternative -- the LAST chunk of an env tile to arrive folds them inside this launch -- is built (FOLD, cl_tuning.finish = 2)
        // and measured SLOWER.  Round 1 did it with an agent-scope release / acquire pair around a counter: those fences write back and
        // invalidate the whole XCD L2 (177 us vs 21 us at 1024 buildings x 1024 envs).  Round 3 removed every fence: only the partial sums
        // and the ticket cross XCDs, so only THEY are accessed at agent scope (relaxed atomic stores / loads = write-through / L2-bypassing
        // `sc1` accesses, no cache maintenance); the order "partials complete -> ticket" is a wait for the thread's own stores (a
        // workgroup-scope release fence is an s_waitcnt) plus the workgroup barrier in front of the one thread that takes the ticket; the
        // fold itself has every thread's loads in flight at once.  Correct and deterministic (scripts/finish_stress.py: 3000 steps, two
        // engines bit-identical) -- and 16.2 us against 14.6 us for the two launches at 1024 x 1024 thermal, 16.0 against 10.5 us for
        // battery + PV (profiles/r03b_c4_fold_ab.log): write-through acknowledgement, ticket and re-read are three dependent device-scope
        // round trips of ~2 us each behind the last workgroup, more than the launch they replace.  The second launch stays the default.
        // DEFERRED FINISH (FOLD, cl_tuning.finish = 3, a.fused_finish == 2; round 4): nothing in step t + 1 reads step t's district sums
        // unless the reward couples the buildings (MARL, EV) -- so the second launch leaves the per-step critical path altogether.  The
        // scratch rows are double-buffered by step parity: this launch writes its partial sums to buffer t & 1 and every wave folds ONE
        // district sum of the PREVIOUS step out of buffer (t + 1) & 1 (plain loads of what the previous launch wrote -- no cross-workgroup
        // traffic inside a launch, no fence, no ticket), in cl_finish_kernel's summation order: out_env trails the step by one launch, and
        // cl_finish_f32 (the same cl_finish_kernel, on buffer t & 1) brings it up to date when somebody wants to read it -- the host's
        // lazy read, or the end of a captured rollout.  A marker word per buffer (step + 1; with the chunk count, in the last 16 bytes of the
        // reserved plane) tells cl_finish_f32 whether the buffer really holds step t's partial sums: calls that did not defer leave it
        // alone, and cl_finish_f32 is then a no-op -- the library keeps no host-side state about pending folds.
        float* scratch = a.out_bldg + (long long)CLO_RESERVED * plane;
        const bool deferred = FOLD && a.fused_finish == 2;
        if (deferred) scratch += (long long)(a.t & 1) * a.n_chunks * NQ * a.n_env;
        for (int i = threadIdx.x; i < NQ * TILE; i += blockDim.x) {
            const int q = i / TILE, e = i - q * TILE;
            float s = 0.0f;
            for (int k = 0; k < a.nw; ++k) s += lds[(size_t)k * NQ * TILE + i];
            if (tile_env0 + e < a.n_env) {
                float* dst = scratch + ((long long)by * NQ + q) * a.n_env + tile_env0 + e;
                if (FOLD && a.fused_finish == 1) __hip_atomic_store(dst, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else *dst = s;
            }
        }
        if constexpr (!FOLD) return;                             // cl_finish_kernel folds them (second launch)
        else {
        if (!a.fused_finish) return;                             // cl_tuning.finish = 1: likewise
        // (a launch that does NOT defer clears this step's marker -- here for the in-launch fold, in cl_finish_kernel for the second launch:
        //  a buffer left behind by an earlier deferred step with the same parity must not look current to a later cl_finish_f32)
        if (a.fused_finish == 1 && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
            reinterpret_cast<unsigned*>(a.out_bldg + (long long)(CLO_RESERVED + 1) * plane - 4)[a.t & 1] = 0u;
        if (a.fused_finish == 2) {
            // the previous step's district sums, behind this step's partial-sum stores (the exchange tile was complete at the barrier above)
            fold_finish<TILE>(a, lds_fold, w, lane, bx, by);
            if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
                unsigned* marker = reinterpret_cast<unsigned*>(a.out_bldg + (long long)(CLO_RESERVED + 1) * plane - 4);   // last 16 bytes of the plane
                marker[a.t & 1] = (unsigned)a.t + 1u;
                marker[2] = (unsigned)a.n_chunks;
            }
            return;
        }
        // (the tickets sit at a FIXED place -- the (n_env + 63) / 64 words in front of the marker words at the plane's tail -- whatever the chunk
        //  count: behind the partial-sum rows, where they were until round 5, a chunked cl_rollout_f32 with another chunk geometry wrote its
        //  return rows over them, and a later in-launch fold found non-zero tickets and never folded: round-5 advisor finding)
        unsigned* ticket = reinterpret_cast<unsigned*>(a.out_bldg + (long long)(CLO_RESERVED + 1) * plane) - 4 - (a.n_env + 63) / 64 + bx;
        // this thread's partial sums have left the CU: outside tgsplit mode a workgroup-scope release fence does NOT wait for outstanding
        // vector stores (it only orders LDS), so the wait is spelled out -- s_waitcnt vmcnt(0) expcnt(0) lgkmcnt(0) -- in front of it
        // (round-3 advisor finding: the ticket could otherwise become visible before the write-through partial sums are acknowledged)
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();                                         // ... and so have everybody else's (and nobody reads the wave rows of `lds` any more)
        unsigned* flag = reinterpret_cast<unsigned*>(lds);
        if (threadIdx.x == 0) *flag = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (*flag != (unsigned)a.n_chunks - 1u) return;
        __syncthreads();                                         // (everybody has read the flag: `lds` is reused below)
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        // The fold is one dependent chain per thread -- ticket, loads, adds -- so its cost is memory round trips, not bytes (32 chunks x
        // 4 quantities x 128 envs = 64 KB).  Every thread of the workgroup takes part: output o = (quantity, env) is shared by
        // `rep` = blockDim / (NQ * TILE) threads, each adding a contiguous range of chunks with all its loads in flight at once (sixteen
        // at a time); the ranges are then added in range order through LDS: the same fixed association whoever arrives last.
        const bool marl = rkind == CLR_MARL;
        const int n_out = NQ * TILE;
        const int rep = max(1, (int)blockDim.x / n_out);
        const int cpp = (a.n_chunks + rep - 1) / rep;                       // chunks per range
        float* part = lds;                                                  // [rep][n_out] (and [rep][n_out] district-net parts for MARL behind it)
        for (int i = threadIdx.x; i < rep * n_out; i += blockDim.x) {
            const int o = i % n_out, p = i / n_out;
            const int q = o / TILE, e = o - q * TILE;
            const bool scale = marl && q == CLQ_REWARD;          // the partials carried sign(-net) * 0.01 * net^2: times max(0, district net)
            float s = 0.0f, sn = 0.0f;
            if (tile_env0 + e < a.n_env) {
                const float* src = scratch + (long long)q * a.n_env + tile_env0 + e;
                const float* srcn = scratch + (long long)CLQ_NET * a.n_env + tile_env0 + e;
                const int c_hi = min(a.n_chunks, (p + 1) * cpp);
                for (int c0 = p * cpp; c0 < c_hi; c0 += 16) {
                    float v[16], vn[16];
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const bool in = c0 + j < c_hi;
                        const long long off = (long long)(in ? c0 + j : c0) * NQ * a.n_env;
                        v[j] = __hip_atomic_load(src + off, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        vn[j] = scale ? __hip_atomic_load(srcn + off, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0f;
                        if (!in) { v[j] = 0.0f; vn[j] = 0.0f; }
                    }
#pragma unroll
                    for (int j = 0; j < 16; ++j) { s += v[j]; sn += vn[j]; }
                }
            }
            part[(size_t)p * n_out + o] = s;
            if (marl) part[(size_t)(rep + p) * n_out + o] = sn;
        }
        __syncthreads();
        for (int o = threadIdx.x; o < n_out; o += blockDim.x) {
            const int q = o / TILE, e = o - q * TILE;
            if (tile_env0 + e >= a.n_env) continue;
            float s = 0.0f, sn = 0.0f;
            for (int p = 0; p < rep; ++p) {
                s += part[(size_t)p * n_out + o];
                if (marl) sn += part[(size_t)(rep + p) * n_out + o];
            }
            if (marl && q == CLQ_REWARD) s *= fmaxf(0.0f, sn);
            a.out_env[(long long)q * a.n_env + tile_env0 + e] = s;
        }
        if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next launch
        return;
        }
    }
    for (int i = threadIdx.x; i < NQ * TILE; i += blockDim.x) {
        const int q = i / TILE, e = i - q * TILE;
        float s = 0.0f;
        if constexpr (STRIPS) {
            if (strip_row) s = lds[(size_t)a.nw * NQ * TILE + i];
        }
        for (int k = 0; k < a.nw; ++k) s += lds[(size_t)k * NQ * TILE + i];
        if (coupled && q == CLQ_REWARD) {                      // finished below
            if (FLEX && rkind == CLR_EV) lds[i] = s;           // CLR_EV accumulated sign(-net) * 0.01 * net^2: the district MARL sum / max(0, district net)
            continue;
        }
        if (tile_env0 + e < a.n_env) {
            a.out_env[(long long)q * a.n_env + tile_env0 + e] = s;
            if constexpr (KPIS) {
                if (q == CLQ_NET) {                                                                   // control condition (citylearn.py:1136-1323)
                    if (i == (int)threadIdx.x) kpi_series_apply(a.kpi_env + tile_env0 + e, a.n_env, a.t, s, pre);
                    else kpi_series_update(a.kpi_env + tile_env0 + e, a.n_env, a.t, s);               // (workgroups narrower than their env tile)
                }
            }
        }
        if (coupled && q == CLQ_NET) lds[i] = s;               // wave-0 slot now holds the district net
    }
    if (coupled) {
        // MARL couples every building to the district net (reward_function.py:132-143): second sweep over the
        // nets this same thread wrote a moment ago (L1/L2 hits), then a second LDS reduction for the reward sum.
        __syncthreads();
        float dnet[VEC], dmarl[VEC];
        vload<VEC>(dnet, lds + CLQ_NET * TILE + lane * VEC);
        const bool central_ev = FLEX && rkind == CLR_EV && (a.flags & CLD_CENTRAL_AGENT);
        if (central_ev) {
            vload<VEC>(dmarl, lds + CLQ_REWARD * TILE + lane * VEC);
#pragma unroll
            for (int i = 0; i < VEC; ++i) dmarl[i] *= fmaxf(0.0f, dnet[i]);
        }
        __syncthreads();
        float r_sum[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) r_sum[i] = 0.0f;
        if (live) {
            for (int b = w; b < a.n_bldg; b += stride) {
                const long long off = (long long)b * (FLEX ? a.n_env : a.ld) + env0;
                float n[VEC], rw[VEC];
                vload<VEC>(n, a.out_bldg + CLO_NET * plane + off);
#pragma unroll
                for (int i = 0; i < VEC; ++i) rw[i] = central_ev ? dmarl[i] : cl::marl_reward(n[i], dnet[i]);
                if (FLEX && rkind == CLR_EV) {
                    // Electric_Vehicles_Reward_Function: MARL only scales the charger terms cl_flex_kernel prepared
                    const uint32_t* __restrict__ bp = a.params + (long long)b * CL_NP;
                    const int fbi = (bp[CLP_L_FLAGS] & CLF_FLEX) ? (int)bp[CLP_FLEX_INDEX] : -1;
                    float k0[VEC], kn[VEC], kp[VEC];
                    if (fbi >= 0) {
                        const long long fp = (long long)a.n_flex_bldg * a.n_env, fo = (long long)fbi * a.n_env + env0;
                        vload<VEC>(k0, a.flex_out + CLX_RW_K0 * fp + fo);
                        vload<VEC>(kn, a.flex_out + CLX_RW_KNEG * fp + fo);
                        vload<VEC>(kp, a.flex_out + CLX_RW_KPOS * fp + fo);
                    }
#pragma unroll
                    for (int i = 0; i < VEC; ++i) rw[i] = fbi >= 0 ? cl::ev_reward(true, rw[i], n[i], k0[i], kn[i], kp[i]) : 0.0f;
                    if (fbi >= 0 && a.ev_penalty_coef > 0.0f) {            // reward_function.py:431-434
                        float viol[VEC];
                        vload<VEC>(viol, a.flex_out + CLX_VIOLATION * ((long long)a.n_flex_bldg * a.n_env) + (long long)fbi * a.n_env + env0);
#pragma unroll
                        for (int i = 0; i < VEC; ++i) rw[i] -= viol[i] > 0.0f ? viol[i] * a.ev_penalty_coef : 0.0f;
                    }
                }
#pragma unroll
                for (int i = 0; i < VEC; ++i) r_sum[i] += rw[i];
                pstore<VEC, false>(a.out_bldg + CLO_REWARD * plane + off, rw);
            }
        }
        vstore<VEC>(lds + (size_t)w * TILE + lane * VEC, r_sum);
        __syncthreads();
        for (int e = threadIdx.x; e < TILE; e += blockDim.x) {
            float s = 0.0f;
            for (int k = 0; k < a.nw; ++k) s += lds[(size_t)k * TILE + e];
            if (tile_env0 + e < a.n_env) a.out_env[(long long)CLQ_REWARD * a.n_env + tile_env0 + e] = s;
        }
    }
}

// FLEX: the district has EV chargers / washing machines (cl_flex.h ran just before); a separate instantiation so that
// districts without them keep their register budget.
// PREC: the battery map -- 0 fp32, 1 CLD_F64_MAPS (two more state planes), 2 CLD_F64_CHAIN (cl_unit.h)
// CHECK (CLD_CHECK): the reference's runtime assertions as CLV_* bits, one word per unit, into the reserved plane (never a chunked launch)
template <int VEC, bool FULL, bool DETAIL, bool FLEX = false, int PREC = 0, bool FOLD = false, bool CHECK = false>
__global__ void __launch_bounds__(1024) cl_step_kernel(const StepArgs a) {
    constexpr bool F64 = PREC == 1;
    const int bx = blockIdx.x, by = blockIdx.y;
    extern __shared__ __attribute__((aligned(16))) float lds[];     // [nw][NQ][64*VEC]
    constexpr int TILE = 64 * VEC;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int env0 = bx * TILE + lane * VEC;
    const bool live = env0 < a.n_env;                     // n_env % VEC == 0 is enforced on the host
    // (a row pitch exists for battery + PV districts only: the thermal / flexible-load instantiations never read it -- their scalar
    //  register file is full, one more live word costs them a scratch reservation)
    const int ld = (FULL || FLEX) ? a.n_env : a.ld;
    const long long plane = (long long)a.n_bldg * ld;
    const int rkind = (a.flags & CLD_REWARD_MASK) >> CLD_REWARD_SHIFT;
    const bool quirk = a.flags & CLD_REF_T0_QUIRK;
    constexpr bool detail = DETAIL;

    float q_net[VEC], q_cost[VEC], q_em[VEC], q_rw[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) q_net[i] = q_cost[i] = q_em[i] = q_rw[i] = 0.0f;

    const int b_lo = by * a.b_chunk;
    const int b_hi = min(a.n_bldg, b_lo + a.b_chunk);
    const bool marl_partial = rkind == CLR_MARL && a.n_chunks > 1;
    // table row of this env tile: TILE divides CL_ROW0_BLOCK, so the offset is workgroup-uniform (scalar load)
    const int ts_row = a.t + (a.env_row0 ? a.env_row0[(bx * TILE) / CL_ROW0_BLOCK] : 0);
    // (FOLD, deferred finish) this wave's share of the previous step's chunk sums: the first load of the kernel
    [[maybe_unused]] float fold_prev = 0.0f;
    [[maybe_unused]] bool fold_issued = false, folded = false;
    [[maybe_unused]] float* lds_fold = lds + (size_t)a.nw * NQ * TILE;        // (deferred finish) [64][16] behind the reduction rows
    for (int b = b_lo + w; b < b_hi; b += a.nw) {
        cl::Bp B;
        cl::load_bp<FULL>(B, a.params + (long long)b * CL_NP);
        cl::Row R;
        cl::load_row<FULL>(R, a.ts + ((long long)ts_row * a.n_bldg + b) * CL_NF, B.flags,
                           (FULL && DETAIL) ? a.ts + ((long long)(ts_row - a.t + a.n_steps - 1) * a.n_bldg + b) * CL_NF : nullptr);
        if (live) {
            const long long off = (long long)b * ld + env0;
            float s_soc[VEC], s_eff[VEC], s_deg[VEC], s_cs[VEC], s_hs[VEC], s_ds[VEC];
            [[maybe_unused]] float s_efl[VEC], s_dgl[VEC];                 // CLD_F64_MAPS: low words of efficiency / degraded capacity
            float a_cs[VEC], a_hs[VEC], a_ds[VEC], a_es[VEC], a_cd[VEC], a_hd[VEC];
            const bool batt = B.flags & CLF_BATTERY;
            if (batt) {
                vload<VEC>(s_soc, a.state + CLS_B_SOC * plane + off);
                vload<VEC>(s_eff, a.state + CLS_B_EFF * plane + off);
                vload<VEC>(s_deg, a.state + CLS_B_DEGCAP * plane + off);
                if constexpr (F64) {
                    vload<VEC>(s_efl, a.state + CLS_B_EFF_LO * plane + off);
                    vload<VEC>(s_dgl, a.state + CLS_B_DEGCAP_LO * plane + off);
                }
            }
            load_action<VEC>(a_es, a, B.a_es, env0);
            if constexpr (FULL) {
                if (B.flags & CLF_COOL_STO) vload<VEC>(s_cs, a.state + CLS_CS_SOC * plane + off);
                if (B.flags & CLF_HEAT_STO) vload<VEC>(s_hs, a.state + CLS_HS_SOC * plane + off);
                if (B.flags & CLF_DHW_STO) vload<VEC>(s_ds, a.state + CLS_DS_SOC * plane + off);
                load_action<VEC>(a_cs, a, B.a_cs, env0);
                load_action<VEC>(a_hs, a, B.a_hs, env0);
                load_action<VEC>(a_ds, a, B.a_ds, env0);
                if (B.a_coh >= 0) {
                    float c[VEC];
                    load_action<VEC>(c, a, B.a_coh, env0);
#pragma unroll
                    for (int i = 0; i < VEC; ++i) { a_cd[i] = fabsf(fminf(c[i], 0.0f)); a_hd[i] = fabsf(fmaxf(c[i], 0.0f)); }
                } else {
                    load_action<VEC>(a_cd, a, B.a_cd, env0);
                    load_action<VEC>(a_hd, a, B.a_hd, env0);
                }
            }
            if constexpr (FOLD) {
                // (deferred finish) this wave's share of the previous step's chunk sums: issued BEHIND the first building's plane loads --
                // it crosses XCDs (another workgroup's L2 wrote it) and returns later than they do, and loads return in order
                if (!fold_issued) { fold_prev = fold_prefetch<TILE>(a, w, lane, plane, bx, by); fold_issued = true; }
            }
            float o_net[VEC], o_rw[VEC], o_eb[VEC], o_cd[VEC], o_hd[VEC], o_dd[VEC], o_cc[VEC], o_ch[VEC], o_cw[VEC], o_cn[VEC], o_bn[VEC], o_ex[VEC], o_sv[VEC], o_ws[VEC], o_sc[VEC], o_sh[VEC], o_sd[VEC];
            [[maybe_unused]] float o_viol[VEC];
            // chargers / washing machines of this building, advanced by cl_flex_kernel just before this launch
            const int fbi = (FLEX && (B.flags & CLF_FLEX)) ? (int)B.p[CLP_FLEX_INDEX] : -1;
            float x_load[VEC], x_chg[VEC];
            if (FLEX && fbi >= 0) {
                const long long fp = (long long)a.n_flex_bldg * a.n_env, fo = (long long)fbi * a.n_env + env0;
                vload<VEC>(x_load, a.flex_out + CLX_LOAD * fp + fo);
                if constexpr (DETAIL) vload<VEC>(x_chg, a.flex_out + CLX_CHARGERS * fp + fo);   // only the baseline needs it
                else {
#pragma unroll
                    for (int i = 0; i < VEC; ++i) x_chg[i] = 0.0f;
                }
            }
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                cl::State S;
                S.soc = batt ? s_soc[i] : 0.0f; S.eff = batt ? s_eff[i] : 1.0f; S.degcap = batt ? s_deg[i] : 0.0f;
                S.cs = S.hs = S.ds = 0.0f;
                S.eff_lo = S.deg_lo = 0.0f;
                if constexpr (F64) { S.eff_lo = batt ? s_efl[i] : 0.0f; S.deg_lo = batt ? s_dgl[i] : 0.0f; }
                cl::Act act = {0.0f, 0.0f, 0.0f, a_es[i], 0.0f, 0.0f};
                if constexpr (FULL) {
                    S.cs = (B.flags & CLF_COOL_STO) ? s_cs[i] : 0.0f;
                    S.hs = (B.flags & CLF_HEAT_STO) ? s_hs[i] : 0.0f;
                    S.ds = (B.flags & CLF_DHW_STO) ? s_ds[i] : 0.0f;
                    act = {a_cs[i], a_hs[i], a_ds[i], a_es[i], a_cd[i], a_hd[i]};
                }
                cl::Out O;
                cl::unit_step<FULL, PREC, CHECK>(B, R, a.t, quirk, act, S, O);
                if constexpr (CHECK) o_viol[i] = __uint_as_float(O.viol);
                if (FLEX && fbi >= 0) cl::apply_flex(R.outage, R.price, R.carbon, x_load[i], x_chg[i], O);
                const float rw = cl::unit_reward<FULL>(rkind, B, S, O.net);
                s_soc[i] = S.soc; s_eff[i] = S.eff; s_deg[i] = S.degcap; s_cs[i] = S.cs; s_hs[i] = S.hs; s_ds[i] = S.ds;
                if constexpr (F64) { s_efl[i] = S.eff_lo; s_dgl[i] = S.deg_lo; }
                o_net[i] = O.net; o_rw[i] = rw; o_eb[i] = O.eb; o_cd[i] = O.cool_dem; o_hd[i] = O.heat_dem; o_dd[i] = O.dhw_dem;
                o_cc[i] = O.c_cool; o_ch[i] = O.c_heat; o_cw[i] = O.c_dhw; o_cn[i] = O.c_ns;
                o_bn[i] = O.base_net; o_ex[i] = O.expected; o_sv[i] = O.served; o_ws[i] = O.net_ws;
                o_sc[i] = O.se_cool; o_sh[i] = O.se_heat; o_sd[i] = O.se_dhw;
                // multi-chunk MARL: accumulate sign(-net) * 0.01 * net^2; cl_finish_kernel scales by max(0, district net)
                q_net[i] += O.net; q_cost[i] += O.cost; q_em[i] += O.emission;
                q_rw[i] += (marl_partial || (FLEX && rkind == CLR_EV)) ? cl::marl_reward(O.net, 1.0f) : rw;
            }
            if constexpr (FOLD) {
                // ... and parked in LDS after the LAST building's arithmetic, before its stores: the load crosses XCDs and takes longer than one
                // building's arithmetic (stash before the first of two buildings' stores: + 1.1 us on the thermal shard); the stores of earlier
                // buildings have long been acknowledged by then (a load waited for right behind stores waits for their acknowledgements too)
                if (!folded && b + a.nw >= b_hi) { fold_stash(a, lds_fold, w, lane, fold_prev); folded = true; }
            }
            auto put = [&](auto nt_tag) {
                constexpr bool NT = decltype(nt_tag)::value;
                if (batt) {
                    pstore<VEC, NT>(a.state + CLS_B_SOC * plane + off, s_soc);
                    pstore<VEC, NT>(a.state + CLS_B_EFF * plane + off, s_eff);
                    pstore<VEC, NT>(a.state + CLS_B_DEGCAP * plane + off, s_deg);
                    if constexpr (F64) {
                        pstore<VEC, NT>(a.state + CLS_B_EFF_LO * plane + off, s_efl);
                        pstore<VEC, NT>(a.state + CLS_B_DEGCAP_LO * plane + off, s_dgl);
                    }
                }
                if constexpr (FULL) {
                    if (B.flags & CLF_COOL_STO) pstore<VEC, NT>(a.state + CLS_CS_SOC * plane + off, s_cs);
                    if (B.flags & CLF_HEAT_STO) pstore<VEC, NT>(a.state + CLS_HS_SOC * plane + off, s_hs);
                    if (B.flags & CLF_DHW_STO) pstore<VEC, NT>(a.state + CLS_DS_SOC * plane + off, s_ds);
                }
                pstore<VEC, NT>(a.out_bldg + CLO_NET * plane + off, o_net);
                if (rkind != CLR_MARL && !(FLEX && rkind == CLR_EV)) pstore<VEC, NT>(a.out_bldg + CLO_REWARD * plane + off, o_rw);
                if constexpr (CHECK) pstore<VEC, NT>(a.out_bldg + CLO_RESERVED * plane + off, o_viol);
                if constexpr (FULL && DETAIL) {
                    // what another kernel of the path reads: the KPI pass (baseline, expected, served) and the LSTM stage (delivered demands)
                    pstore<VEC, NT>(a.out_bldg + CLO_COOL_DEM * plane + off, o_cd);
                    pstore<VEC, NT>(a.out_bldg + CLO_HEAT_DEM * plane + off, o_hd);
                    pstore<VEC, NT>(a.out_bldg + CLO_BASE_NET * plane + off, o_bn);
                    pstore<VEC, NT>(a.out_bldg + CLO_EXPECTED * plane + off, o_ex);
                    pstore<VEC, NT>(a.out_bldg + CLO_SERVED * plane + off, o_sv);
                    if (!(a.flags & CLD_DETAIL_MIN)) {                       // the series of evaluate() / the observations / the parity tests
                        pstore<VEC, NT>(a.out_bldg + CLO_B_EB * plane + off, o_eb);
                        pstore<VEC, NT>(a.out_bldg + CLO_DHW_DEM * plane + off, o_dd);
                        pstore<VEC, NT>(a.out_bldg + CLO_C_COOL * plane + off, o_cc);
                        pstore<VEC, NT>(a.out_bldg + CLO_C_HEAT * plane + off, o_ch);
                        pstore<VEC, NT>(a.out_bldg + CLO_C_DHW * plane + off, o_cw);
                        pstore<VEC, NT>(a.out_bldg + CLO_C_NSL * plane + off, o_cn);
                        pstore<VEC, NT>(a.out_bldg + CLO_NET_WS * plane + off, o_ws);
                        pstore<VEC, NT>(a.out_bldg + CLO_SE_COOL * plane + off, o_sc);
                        pstore<VEC, NT>(a.out_bldg + CLO_SE_HEAT * plane + off, o_sh);
                        pstore<VEC, NT>(a.out_bldg + CLO_SE_DHW * plane + off, o_sd);
                    }
                }
            };
            if (a.nt) put(NtOn{}); else put(NtOff{});
        }
    }

    if constexpr (FOLD) {
        if (!folded) {                                              // (waves without a building or beyond the batch)
            if (!fold_issued) fold_prev = fold_prefetch<TILE>(a, w, lane, plane, bx, by);
            fold_stash(a, lds_fold, w, lane, fold_prev);
        }
    }
    district_reduce<VEC, FLEX, FOLD>(a, lds, w, lane, env0, live, plane, rkind, q_net, q_cost, q_em, q_rw, a.nw, lds_fold);
}

// Building-chunked battery + PV districts (BASELINE config 4 with the 2022 device set), latency-ordered (round 5).  cl_step_kernel walks a
// dependent chain per building -- parameter block (scalar loads) -> battery flag / action column -> plane loads -> arithmetic -> stores --
// and a wave of a chunked launch walks it b_chunk / 16 times.  Here a wave issues the plane loads of its FIRST building before it touches a
// parameter and those of its NEXT building before it computes the current one: the addresses depend on the building index only (and on
// CLD_ES_COL_IS_BLDG for the action column; other column maps load the action once the block is there).  The parameter block and the table
// row still arrive by scalar loads (staged in LDS they would sit in 36 vector registers per lane: 44 bytes of scratch at four envs per lane).
// Non-battery buildings' planes are fetched and ignored.  Same arithmetic, same summation order as cl_step_kernel<VEC, false, false>:
// bit-identical planes and sums.
// PREC = 2 (round 6): the battery's soc chain in float64 (CLD_F64_CHAIN, the engine's default precision model) -- the chunked districts' default path
// had been the general kernel plus the second launch.
template <int VEC, bool NT, bool FOLD, int PREC = 0>
__global__ void __launch_bounds__(1024) cl_step_lean_chunk_kernel(const StepArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];     // [nw][NQ][64*VEC] | (FOLD) exchange tile
    constexpr int TILE = 64 * VEC;
    const int bx = blockIdx.x, by = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int env0 = bx * TILE + lane * VEC;
    const bool live = env0 < a.n_env;
    const int ld = a.n_env;                                       // (no row pitch for districts of more than 32 buildings: host)
    const long long plane = (long long)a.n_bldg * ld;
    const int rkind = (a.flags & CLD_REWARD_MASK) >> CLD_REWARD_SHIFT;
    const bool quirk = a.flags & CLD_REF_T0_QUIRK;
    const bool act_by_bldg = (a.flags & CLD_ES_COL_IS_BLDG) && a.act_stride_env == 1;
    const int b_lo = by * a.b_chunk;
    const int b_hi = min(a.n_bldg, b_lo + a.b_chunk);
    const bool marl_partial = rkind == CLR_MARL;                  // (always chunked: cl_finish_kernel scales by the district net)
    const int ts_row = a.t + (a.env_row0 ? a.env_row0[(bx * TILE) / CL_ROW0_BLOCK] : 0);
    [[maybe_unused]] float* lds_fold = lds + (size_t)a.nw * NQ * TILE;
    struct In { float soc[VEC], eff[VEC], deg[VEC], act[VEC]; };
    auto fetch = [&](In& x, int b) {
        const long long off = (long long)b * ld + env0;
        vload<VEC>(x.soc, a.state + CLS_B_SOC * plane + off);
        vload<VEC>(x.eff, a.state + CLS_B_EFF * plane + off);
        vload<VEC>(x.deg, a.state + CLS_B_DEGCAP * plane + off);
        if (act_by_bldg) vload<VEC>(x.act, a.actions + (long long)b * a.act_stride_col + env0);
    };
    In cur;
#pragma unroll
    for (int i = 0; i < VEC; ++i) cur.soc[i] = cur.eff[i] = cur.deg[i] = cur.act[i] = 0.0f;
    int b = b_lo + w;
    if (live && b < b_hi) fetch(cur, b);
    [[maybe_unused]] float fold_prev = 0.0f;
    [[maybe_unused]] bool folded = false;
    if constexpr (FOLD) fold_prev = fold_prefetch<TILE>(a, w, lane, plane, bx, by);      // behind the first building's plane loads (fold_prefetch's note)
    float q_net[VEC], q_cost[VEC], q_em[VEC], q_rw[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) q_net[i] = q_cost[i] = q_em[i] = q_rw[i] = 0.0f;
    for (; b < b_hi; b += a.nw) {
        cl::Bp B;
        cl::load_bp<false>(B, a.params + (long long)b * CL_NP);
        cl::Row R;
        cl::load_row<false>(R, a.ts + ((long long)ts_row * a.n_bldg + b) * CL_NF, B.flags);
        if (live) {
            const long long off = (long long)b * ld + env0;
            const bool batt = B.flags & CLF_BATTERY;
            float a_es[VEC];
            if (act_by_bldg) {
#pragma unroll
                for (int i = 0; i < VEC; ++i) a_es[i] = B.a_es >= 0 ? cur.act[i] : 0.0f;
            } else load_action<VEC>(a_es, a, B.a_es, env0);
            float o_soc[VEC], o_eff[VEC], o_deg[VEC], o_net[VEC], o_rw[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                cl::State S;
                S.soc = batt ? cur.soc[i] : 0.0f; S.eff = batt ? cur.eff[i] : 1.0f; S.degcap = batt ? cur.deg[i] : 0.0f;
                S.cs = S.hs = S.ds = 0.0f; S.eff_lo = S.deg_lo = 0.0f;
                const cl::Act act = {0.0f, 0.0f, 0.0f, a_es[i], 0.0f, 0.0f};
                cl::Out O;
                cl::unit_step<false, PREC>(B, R, a.t, quirk, act, S, O);
                const float rw = cl::unit_reward<false>(rkind, B, S, O.net);
                o_soc[i] = S.soc; o_eff[i] = S.eff; o_deg[i] = S.degcap; o_net[i] = O.net; o_rw[i] = rw;
                q_net[i] += O.net; q_cost[i] += O.cost; q_em[i] += O.emission;
                q_rw[i] += marl_partial ? cl::marl_reward(O.net, 1.0f) : rw;
            }
            if constexpr (FOLD) {
                if (!folded && b + a.nw >= b_hi) { fold_stash(a, lds_fold, w, lane, fold_prev); folded = true; }     // before the LAST building's stores
            }
            // the NEXT building's plane loads, into the registers the arithmetic has just released and IN FRONT of this building's stores: the
            // wait for them at the top of the next iteration then allows the stores to be outstanding (loads and stores share one counter)
            if (b + a.nw < b_hi) fetch(cur, b + a.nw);
            if (batt) {
                pstore<VEC, NT>(a.state + CLS_B_SOC * plane + off, o_soc);
                pstore<VEC, NT>(a.state + CLS_B_EFF * plane + off, o_eff);
                pstore<VEC, NT>(a.state + CLS_B_DEGCAP * plane + off, o_deg);
            }
            pstore<VEC, NT>(a.out_bldg + CLO_NET * plane + off, o_net);
            if (rkind != CLR_MARL) pstore<VEC, NT>(a.out_bldg + CLO_REWARD * plane + off, o_rw);
        }
    }
    if constexpr (FOLD) {
        if (!folded) fold_stash(a, lds_fold, w, lane, fold_prev);      // (waves without a building or beyond the batch)
    }
    district_reduce<VEC, false, FOLD>(a, lds, w, lane, env0, live, plane, rkind, q_net, q_cost, q_em, q_rw, a.nw, lds_fold);
}

// Lean districts (battery + PV + load), at most two buildings per wave, one chunk: the headline shape.  Same arithmetic
// as cl_step_kernel<VEC, false, false>; the memory operations are re-ordered for latency.  A kernel with this launch
// shape and these byte counts but no energy model runs in 5.4 us at 17 x 65 536 (scripts/copy_floor.py) against 8.1 us
// for the generic kernel, whose every wave walks a dependent chain  parameter block (scalar) -> action column ->
// state / action loads -> compute -> stores  once per building.  Here a wave issues the state loads of BOTH its
// buildings (and the action loads, when the column of building b is b: CLD_ES_COL_IS_BLDG) before it touches a parameter.
// (Tried: VEC = 2 compiled for 8 waves per SIMD -- two workgroups per CU, half the per-wave chain: 64 VGPRs with 23 spilled,
// 9.3 us vs 7.9 us for VEC = 4 at 17 x 65 536.  Tried: with 17 = 16 + 1 buildings, sharing the last building's env tile out
// in 64-env strips to four waves at one env per lane instead of giving one wave two buildings -- 5 instead of 8 units on the
// longest wave, 62 instead of 94 VGPRs: 7.89 vs 7.94 us, i.e. the doubled wave is not what bounds the launch.  Tried:
// non-temporal stores for the net / reward planes: 7.87 - 7.91 vs 7.86 - 7.88 us, no effect.  Tried (round 2): plane accesses
// through `float` lvalues instead of float4 ones, so that the parameter block of wave 0's SECOND building -- read after the first
// one's stores, and therefore a uniform *vector* load behind them -- stays a scalar load: 73 instead of 88 VGPRs, and 8.14 vs
// 7.99 us, three alternations on one box: slower.  The same trick is what made the thermal kernel's two-env pack viable
// (cl_full.h); here the vector loads of the 17th building's parameters are issued early enough and the scalar ones are not.
//  Tried again at the end of round 2, with the nt stores and the hoisted unit in place: the 17th building shared out to four waves on
//  four SIMDs as 64-env strips at one env per lane (SIMD loads 4.25 each instead of 5, 4, 4, 4; the strips' district partials in
//  their own LDS row, processed before the wave's main building so that its parameter block stays a scalar load): 7.36 - 7.49 vs
//  7.37 - 7.63 us, alternating on one box -- nothing.  scripts/lean_balance_probe.py: 16 buildings x 65 536 take 6.58 us, 17 take
//  7.39 us, 20 (four waves with two buildings: 5, 5, 5, 5) take 8.22 us = 6.98 us per 17: the cost of the 17th building is that
//  SOME wave walks a second dependent chain behind its first, not the imbalance between the SIMDs.)
// The compact observation of the NEXT row written by the step launch itself (cl_step_observe_f32): every column is an affine map
// of a plane value the wave that stepped the building still holds in registers.
struct ObsFusedArgs {
    float* __restrict__ obs;            // [n_env][pitch]
    const float* __restrict__ table;    // obs_table [n_rows][n_cols]: the offsets of the affine maps
    int n_cols, pitch, row;
    short start[CL_OBS_FUSED_BLDG + 1]; // deps[start[b] .. start[b + 1]) belong to building b
    cl_obs_dep deps[CLOB_MAX_DEPS];     // grouped by building
    int lean_ok;                        // (host) the battery + PV launch can fill it: <= CL_OBS_FUSED_PER_BLDG columns per building, battery / net / reward planes only
};

// UNI (CLD_LEAN_UNIFORM and env-contiguous actions, tested ONCE at the kernel's entry: lean_step_dispatch): every building has a battery driven
// by action column = building index and the reward is -max(net, 0).  What the generic body decides per building at run time -- battery flag,
// `a_es < 0`, action layout, reward kind, exponent -- is a compile-time fact here: the no-battery path, the late action load, the reward switch
// and its two inlined __powf are not in the code a wave fetches, and a building's scalar loads (parameter words, chain constants, table row) form
// ONE group behind the plane loads instead of two dependent ones around the battery-flag test.  Same expressions on the same operands: same bits.
// The plain float64-chain launch only (no FLEX / OBS / KPI epilogue; lean_step_dispatch's note on the fp32 map).
// STORE ACKNOWLEDGEMENTS.  On gfx9 a store counts in vmcnt like a load, so a vmcnt wait behind a wave's plane stores sits out their
// acknowledgement (0.3 - 0.8 us) whatever it was placed for.  The compiler placed three that nothing needed: in front of wave 0's second
// building, in front of the partial sums' LDS writes, behind the reduction's barrier.  The cause is how its wait-count pass joins paths: a
// register holds a "pending load" mark until a wait on the path clears it, and at a join the mark of ANY predecessor survives.  The plane
// loads used to sit in an `if (live)` of their own and each building behind an `if (!own[m])` / `if (!live)` skip: a path "loads requested,
// arithmetic (and its wait) skipped" exists in the flow graph though no wave takes it, the marks reached the join behind the stores, and
// the first instruction there that re-used one of those registers got a vmcnt wait that now counted the stores.  (A wait written out in
// front of the arithmetic does not help: it sits on the side of the skip that was clean already.)  So:
//  - loads, both buildings and their stores form ONE region under `live && own[0]`, and the second building hangs on own[1] alone -- its
//    loads' marks are cleared by the first building's wait on the only path that reaches it;
//  - what the generic body reads behind the first building's stores -- parameter block, table row, chain constants, the reward's capacity
//    word -- comes through the constant address space (scalar loads; as plain reads they were vector loads, real waits behind stores);
//  - actions whose column is a parameter word are requested for both buildings in front of the first one's arithmetic;
//  - the no-battery path, which truly leaves its state rows unread, waits for them itself.
// Left as it was: two waits INSIDE the first building's store burst of the generic body (behind its first and third store; cause not found).
// STRIPS (the uniform body at four envs per lane, a district of ONE building more than waves -- 17 buildings, 16 waves: the headline; the host asks
// for it with CLA_LEAN_STRIPS, cl_tuning.lean_variant & 32 keeps the old mapping).  Wave 0 used to take building nw as a second tile: SIMD 0 then
// holds five tiles of arithmetic and the other three SIMDs four, and all sixteen waves wait at the reduction's barrier for SIMD 0's last wave.  Now
// wave 0 has no second building; the last four waves, nw - 4 + s on SIMD s, each take strip s of building nw -- envs tile + 64 s + lane, one env per
// lane -- BEHIND their main tile.  The strip's four plane dwords are requested first in the load block (the main tile's wait covers them: older
// loads), its parameter block, chain constants and table row are one group of scalar loads, its arithmetic is the tile path's at one env per lane,
// its five planes go out as non-temporal dword stores, and its four district quantities go to LDS row nw (district_reduce: same bits).
// The two round-2 builds of this idea (the notes at the top of this block: 7.89 vs 7.94 and 7.36 - 7.49 vs 7.37 - 7.63 us, "nothing") walked the strips
// BEFORE the main building -- the only order in which the strip's parameter block stayed a scalar load then -- so every strip wave sat out its own
// strip stores' acknowledgements in front of its main tile.  Table reads through cl::as_ctab are scalar loads wherever they stand and no wave waits
// behind its stores any more (STORE ACKNOWLEDGEMENTS), so the strip can follow the main tile with nothing but a store burst nobody waits for in between.
// That alone is still SLOWER than the second tile (7.16 - 7.21 against 7.05 - 7.09 us, twelve alternating rounds in one process): the last four waves
// are the youngest of their SIMDs, the SIMD issues by priority, then age, so they finish their main tile last and walk the strip's latencies alone.
// With `s_setprio 3` at their entry the strip hides under the other waves' arithmetic: 6.82 - 7.00 against 7.24 - 7.30 us (profiles/lean_strips_ab.md).
// A ragged last tile: lane l of the main tile holds envs 4 l .., lane l of strip s env 64 s + l, so a lane can be dead in one and live in the other.
// The region below is entered by lanes live in EITHER; a lane dead in the main tile walks it on the tile's first envs and stores nothing of it (its
// partial sums land in LDS columns of dead envs, which the reducer never writes out); a dead lane of a strip does the same for the strip.
template <int VEC, bool FLEX, bool NT, bool OBS, bool KPI = false, int PREC = 0, bool UNI = false>
CL_DEV void lean_step_body(const StepArgs& a, float* lds, const ObsFusedArgs* of) {     // lds: [nw][NQ][64*VEC] (, then [64*VEC][pitch])
    static_assert(!UNI || (!FLEX && !OBS && !KPI && PREC == 2), "the uniform body is the plain float64-chain launch's");
    constexpr bool F64 = PREC == 1;
    constexpr bool SC = UNI && VEC == 4;                            // the instantiation that carries the strip path (STRIPS, above)
    constexpr int TILE = 64 * VEC;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile_env0 = blockIdx.x * TILE;
    const bool live = tile_env0 + lane * VEC < a.n_env;
    // (SC) a lane whose four envs lie beyond a ragged last tile may still hold a live env of a strip: it walks the main tile with the others, on the
    // tile's first envs (a valid address: n_env is a multiple of four), and stores nothing of it
    const int env0 = SC && !live ? tile_env0 : tile_env0 + lane * VEC;
    const long long plane = (long long)a.n_bldg * a.ld;
    const int rkind = UNI ? (int)CLR_DEFAULT : (int)((a.flags & CLD_REWARD_MASK) >> CLD_REWARD_SHIFT);
    const bool quirk = a.flags & CLD_REF_T0_QUIRK;
    const bool act_by_bldg = UNI || ((a.flags & CLD_ES_COL_IS_BLDG) && a.act_stride_env == 1);
    int row0 = 0;
    if (a.env_row0) {
        if constexpr (UNI) row0 = (int)cl::as_ctab(a.env_row0)[(blockIdx.x * TILE) / CL_ROW0_BLOCK];       // (read-only too: a scalar load)
        else row0 = a.env_row0[(blockIdx.x * TILE) / CL_ROW0_BLOCK];
    }
    const int ts_row = a.t + row0;
    const int bb[2] = {w, w + a.nw};
    // (SC) the strip mapping: one building more than waves, and the host has sized the LDS for the strips' row -- wave-uniform, tested once
    [[maybe_unused]] bool strips = false;
    if constexpr (SC) strips = (a.flags & CLA_LEAN_STRIPS) && a.n_bldg == a.nw + 1;
    const bool own[2] = {bb[0] < a.n_bldg, bb[1] < a.n_bldg && !strips};       // wave-uniform
    // strip s = w - (nw - 4) of building nw: env tile_env0 + 64 s + lane, one per lane
    [[maybe_unused]] const bool strip_w = strips && w >= a.nw - 4;
    [[maybe_unused]] const int x_col = (w - (a.nw - 4)) * 64 + lane;
    [[maybe_unused]] const bool x_live = strip_w && tile_env0 + x_col < a.n_env;
    // The strip waves are the YOUNGEST of their SIMDs, and a SIMD issues by priority, then age: left at priority 0 they finish their main tile last
    // and walk the strip -- a scalar round trip and one dependent float64 chain at one env per lane -- alone, behind everybody else (measured: 7.18
    // against 7.07 us for wave 0's second tile).  Raised, they finish the main tile first and the strip's latencies hide under the other three
    // waves' arithmetic (6.91 against 7.27 us; STRIPS, above).
    if constexpr (SC) {
        if (strip_w) __builtin_amdgcn_s_setprio(3);
    }
    [[maybe_unused]] float x_soc = 0.0f, x_eff = 0.0f, x_deg = 0.0f, x_act = 0.0f;      // the strip's state and action; then its four district quantities
    [[maybe_unused]] float x_net = 0.0f, x_cost = 0.0f, x_em = 0.0f, x_rw = 0.0f;

    float q_net[VEC], q_cost[VEC], q_em[VEC], q_rw[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) q_net[i] = q_cost[i] = q_em[i] = q_rw[i] = 0.0f;
    float s_soc[2][VEC], s_eff[2][VEC], s_deg[2][VEC], a_es[2][VEC];
    [[maybe_unused]] float s_efl[2][VEC], s_dgl[2][VEC];             // CLD_F64_MAPS: low words of efficiency / degraded capacity
    // Non-temporal hint on the plane LOADS (the stores: StepArgs::nt): by instantiation, from alternating A/B builds on one box at 17 buildings
    // (-DCL_LEAN_NT_LOADS=false against the default; profiles/r05_nt_loads/): four envs per lane 65 536 envs 7.52 - 7.56 us with the hint,
    // 6.49 us WITHOUT (49 152: 6.82 / 6.40; 81 920: 11.0 / 10.1) -- the round-2 measurement that introduced the hint (7.32 -> 7.18 us) predates
    // the eight-tensor action ring and the full-year tables; two envs per lane 24 576 / 32 768 envs 4.49 - 4.54 / 4.78 - 4.91 us with, 4.74 - 4.76 /
    // 4.99 - 5.02 without; one env per lane 8 192 / 16 384 envs 3.45 / 4.00 with, 3.34 / 3.78 without; the KPI epilogue's instantiation (four
    // envs per lane) 12.54 us with, 14.78 without.  (With plain STORES the loads' hint is immaterial: 7.29 / 7.31 us.)
    // The flexible-load instantiation (EV districts, behind cl_flex_kernel) keeps it too: 16.2 / 19.7 us per step with, 17.4 / 22.8 without
    // (scripts/ev_step_bench.py, MARL / EV reward, profiles/r05z_ev_step_bench.log against r05w_ev_step_bench.log).
    // The observation epilogue's (cl_step_observe_f32, 65 536 envs): 9.30 - 9.35 us with, 8.84 - 8.85 without (scripts/step_observe_bench.py).
    // (round 6, the HBM-streaming shape 17 x 1 048 576 now that this kernel runs it: the hint on every load, A/B builds in alternating processes --
    //  115.8 - 118.3 us without against 120.0 - 121.3 with on the fp32 map, 120.6 - 123.9 against 113.6 - 121.7 under the chain: nothing; profiles/r06_stream_ntl_ab.log)
    constexpr bool NTL = NT && CL_LEAN_NT_LOADS && (KPI || FLEX || VEC == 2);
    CL_TRACE_DECL;
    CL_TRACE_ENTRY(0);
    CL_TRACE_CYCLES_ENTRY(4);
    if ((live || (SC && x_live)) && own[0]) {
        if constexpr (SC) {
            // The strip's four dwords, requested FIRST: they are the oldest loads of the wave, so the main building's own wait has them too and
            // nothing is left to wait for behind its stores.  (A dead lane of a live strip reads the strip's building at the tile's first env.)
            if (strip_w) {
                const long long xo = (long long)a.nw * a.ld + tile_env0 + (x_live ? x_col : 0);
                const float* xa = a.actions + (long long)a.nw * a.act_stride_col + tile_env0 + (x_live ? x_col : 0);
                float v1[1];
                pload<1, NTL>(v1, a.state + CLS_B_SOC * plane + xo); x_soc = v1[0];
                pload<1, NTL>(v1, a.state + CLS_B_EFF * plane + xo); x_eff = v1[0];
                pload<1, NTL>(v1, a.state + CLS_B_DEGCAP * plane + xo); x_deg = v1[0];
                pload<1, NTL>(v1, xa); x_act = v1[0];
            }
        }
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            if (m && !own[1]) continue;
            const long long off = (long long)bb[m] * a.ld + env0;          // every building has its state rows: no flag test
            pload<VEC, NTL>(s_soc[m], a.state + CLS_B_SOC * plane + off);
            pload<VEC, NTL>(s_eff[m], a.state + CLS_B_EFF * plane + off);
            pload<VEC, NTL>(s_deg[m], a.state + CLS_B_DEGCAP * plane + off);
            if constexpr (F64) {
                pload<VEC, NTL>(s_efl[m], a.state + CLS_B_EFF_LO * plane + off);
                pload<VEC, NTL>(s_dgl[m], a.state + CLS_B_DEGCAP_LO * plane + off);
            }
            if (act_by_bldg) pload<VEC, NTL>(a_es[m], a.actions + (long long)bb[m] * a.act_stride_col + env0);
        }
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            if (m && !own[1]) continue;
            const int b = bb[m];
            cl::Bp B;
            cl::Row R;
            [[maybe_unused]] cl::BattC bc_uni;
            // The building's parameter block and table row through the constant address space (cl_unit.h: the tables are read-only): behind the
            // first building's plane stores a plain read of them is a vector load per lane -- and the wait for it sits out the acknowledgement of
            // those stores as well, since loads and stores count in one counter (STORE ACKNOWLEDGEMENTS, above)
            const cl::cl_ctab pb = cl::as_ctab(a.params + (long long)b * CL_NP);
            const cl::cl_ctab qb = cl::as_ctab(a.ts + ((long long)ts_row * a.n_bldg + b) * CL_NF);
            if constexpr (UNI) {
                // every scalar of the building as ONE group: parameter words, the chain constants (not behind a battery-flag test that needs
                // the words first) and the table row
                B.p = a.params + (long long)b * CL_NP; B.flags = CLF_BATTERY; B.a_es = b; B.rw_exponent = 1.0f;
                B.r = cl::pw(pb, CLP_L_TSR);
                cl::load_battc_from(bc_uni, pb);
            } else cl::load_bp_from<false>(B, a.params + (long long)b * CL_NP, pb);
            R.nsl = cl::pw(qb, CLT_NSL); R.sol = cl::pw(qb, CLT_SOLAR); R.price = cl::pw(qb, CLT_PRICE); R.carbon = cl::pw(qb, CLT_CARBON);
            R.outage = false;
            // (OBS) the building's column descriptors and the offsets of their affine maps, fetched with the parameters: nothing is left to
            // wait for between the arithmetic and the tile writes
            [[maybe_unused]] int od_n = 0, od_col[CL_OBS_FUSED_PER_BLDG], od_src[CL_OBS_FUSED_PER_BLDG];
            [[maybe_unused]] float od_scale[CL_OBS_FUSED_PER_BLDG], od_base[CL_OBS_FUSED_PER_BLDG];
            if constexpr (OBS) {
                const float* __restrict__ trow = of->table + (size_t)(of->row + (ts_row - a.t)) * of->n_cols;
                const int d0 = of->start[b];
                od_n = of->start[b + 1] - d0;
#pragma unroll
                for (int k = 0; k < CL_OBS_FUSED_PER_BLDG; ++k) {
                    const int d = min(d0 + min(k, max(od_n - 1, 0)), CLOB_MAX_DEPS - 1);      // (a building without columns reads a valid, unused entry)
                    od_col[k] = of->deps[d].col; od_src[k] = of->deps[d].src; od_scale[k] = of->deps[d].scale;
                    od_base[k] = trow[od_col[k]];
                }
            }
            const long long off = (long long)b * a.ld + env0;
            const bool batt = UNI || (B.flags & CLF_BATTERY);
            const bool no_es = !UNI && B.a_es < 0;                       // no electrical_storage action: the battery idles
            if constexpr (!UNI) {
                // Actions the top of the kernel could not request (their column is a parameter word): BOTH buildings' here, in front of the
                // first one's arithmetic -- the second one's column word rides in the first one's scalar group.  Requested by the second
                // building itself they would be loads behind the first one's stores.
                if (!act_by_bldg && m == 0) {
                    load_action<VEC>(a_es[0], a, B.a_es, env0);
                    const int col1 = (int)cl::as_ctab(a.params + (long long)bb[own[1] ? 1 : 0] * CL_NP)[CLP_L_ACT_ES];
                    if (own[1]) load_action<VEC>(a_es[1], a, col1, env0);
                }
            }
            CL_TRACE_WAITV(1 + 4 * m, s_deg[m][0]);
            float o_net[VEC], o_rw[VEC];
            [[maybe_unused]] float o_cb[VEC];
            // chargers / washing machines of this building (cl_flex_kernel ran just before this launch)
            const int fbi = (FLEX && (B.flags & CLF_FLEX)) ? (int)B.p[CLP_FLEX_INDEX] : -1;
            float x_load[VEC];
            if (FLEX && fbi >= 0) vload<VEC>(x_load, a.flex_out + (long long)CLX_LOAD * a.n_flex_bldg * a.n_env + (long long)fbi * a.n_env + env0);
            if constexpr (FLEX) {
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    cl::State S;
                    S.soc = batt ? s_soc[m][i] : 0.0f; S.eff = batt ? s_eff[m][i] : 1.0f; S.degcap = batt ? s_deg[m][i] : 0.0f;
                    S.cs = S.hs = S.ds = 0.0f;
                    const cl::Act act = {0.0f, 0.0f, 0.0f, B.a_es >= 0 ? a_es[m][i] : 0.0f, 0.0f, 0.0f};
                    cl::Out O;
                    cl::unit_step<false>(B, R, a.t, quirk, act, S, O);
                    if (FLEX && fbi >= 0) cl::apply_flex(false, R.price, R.carbon, x_load[i], 0.0f, O);
                    const float rw = cl::unit_reward<false>(rkind, B, S, O.net);
                    s_soc[m][i] = S.soc; s_eff[m][i] = S.eff; s_deg[m][i] = S.degcap;
                    o_net[i] = O.net; o_rw[i] = rw;
                    q_net[i] += O.net; q_cost[i] += O.cost; q_em[i] += O.emission;
                    q_rw[i] += (FLEX && rkind == CLR_EV) ? cl::marl_reward(O.net, 1.0f) : rw;
                }
            } else {
                // The lean unit (cl::unit_step<false> + cl::unit_reward<false>, restated with the same expressions) with everything that
                // does not depend on the env taken out of the env loop: the t = 0 booking of the load, the battery's curve parameters
                // (in VGPRs once per building instead of one v_mov per select per env), the has-battery and reward-kind tests.
                // 111 -> 90 VALU instructions per unit (SQ_INSTS_VALU).
                const bool first = quirk && a.t == 0;
                float c_ns = first ? 3.0f * R.nsl : R.nsl;           // booked at reset, by the step and by update_variables
                float sol = R.sol;
                const float cbk = first ? 2.0f : 1.0f;               // c_b = first ? 2 eb : eb
                CL_PIN_V(c_ns); CL_PIN_V(sol);
                if constexpr (UNI) {
                    // The scalar group is complete HERE, at the row's first use, and nothing moves across: left alone, the scheduler sinks the row's
                    // loads behind the battery map (a fresh scalar round trip in the middle of the wave), and the optimiser lifts the actions'
                    // float -> double conversions into the plane-load block (a vector wait between the two buildings' loads, in front of the
                    // scalar group) -- the action stays opaque until this point.  No instruction either way.
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int i = 0; i < VEC; ++i) CL_PIN_V(a_es[m][i]);
                }
                float soc_rw[VEC];
                if (F64 && batt) {
                    // the battery map in float64 on the unrounded parameters (CLD_F64_MAPS, cl_unit.h)
                    if constexpr (F64) {
                        cl::BattP64 B64;
                        cl::load_batt64(B64, B.p);
                        if (B.a_es < 0) {
#pragma unroll
                            for (int i = 0; i < VEC; ++i) a_es[m][i] = 0.0f;
                        }
#pragma unroll
                        for (int i = 0; i < VEC; ++i) {
                            cl::State S = {s_soc[m][i], s_eff[m][i], s_deg[m][i], 0.0f, 0.0f, 0.0f, s_efl[m][i], s_dgl[m][i]};
                            const float eb = cl::battery_charge_ref(B64, (double)a_es[m][i] * B64.pow * B64.dt / B64.r, a.t == 0, S);     // (flexibility = +inf)
                            s_soc[m][i] = S.soc; s_eff[m][i] = S.eff; s_deg[m][i] = S.degcap; s_efl[m][i] = S.eff_lo; s_dgl[m][i] = S.deg_lo;
                            soc_rw[i] = S.soc;
                            o_cb[i] = cbk * eb;
                            o_net[i] = fmaf(c_ns + o_cb[i], B.r, sol);
                        }
                    }
                } else if (PREC == 2 && batt) {
                    // the soc chain in float64, the degraded capacity as the capacity loss (CLD_F64_CHAIN, cl_unit.h)
                    if constexpr (PREC == 2) {
                        cl::BattC bc;
                        if constexpr (UNI) bc = bc_uni;
                        else cl::load_battc_from(bc, pb);
                        if (no_es) {
#pragma unroll
                            for (int i = 0; i < VEC; ++i) a_es[m][i] = 0.0f;
                        }
#pragma unroll
                        for (int i = 0; i < VEC; ++i) {
                            cl::State S = {s_soc[m][i], s_eff[m][i], s_deg[m][i], 0.0f, 0.0f, 0.0f};
                            const float eb = cl::battery_charge_chain(bc, a_es[m][i], INFINITY, S);
                            s_soc[m][i] = S.soc; s_eff[m][i] = S.eff; s_deg[m][i] = S.degcap;
                            soc_rw[i] = S.soc;
                            o_cb[i] = cbk * eb;
                            o_net[i] = fmaf(c_ns + o_cb[i], B.r, sol);
                        }
                    }
                } else if (batt) {
                    cl::BattP Bv = B.batt;
                    CL_PIN_V(Bv.cpc_a0); CL_PIN_V(Bv.cpc_b0); CL_PIN_V(Bv.cpc_a1); CL_PIN_V(Bv.cpc_b1);
                    CL_PIN_V(Bv.pec_a0); CL_PIN_V(Bv.pec_b0); CL_PIN_V(Bv.pec_a1); CL_PIN_V(Bv.pec_b1);
                    CL_PIN_V(Bv.pec_a2); CL_PIN_V(Bv.pec_b2); CL_PIN_V(Bv.pec_a3); CL_PIN_V(Bv.pec_b3);
                    if (no_es) {
#pragma unroll
                        for (int i = 0; i < VEC; ++i) a_es[m][i] = 0.0f;
                    }
#pragma unroll
                    for (int i = 0; i < VEC; ++i) {
                        cl::State S = {s_soc[m][i], s_eff[m][i], s_deg[m][i], 0.0f, 0.0f, 0.0f};
                        // battery_step with flexibility = +inf (no outage in a lean district)
                        const float eb = cl::battery_energy(Bv, a_es[m][i] * Bv.pdt, S);
                        s_soc[m][i] = S.soc; s_eff[m][i] = S.eff; s_deg[m][i] = S.degcap;
                        soc_rw[i] = S.soc;
                        o_cb[i] = cbk * eb;                           // the battery's booked consumption (doubled at t = 0)
                        o_net[i] = fmaf(c_ns + o_cb[i], B.r, sol);
                    }
                } else {
                    // (no battery: nobody reads the state rows requested at the top.  Waited for HERE, on the path that leaves them behind --
                    //  otherwise every wave pays for them at its stores: STORE ACKNOWLEDGEMENTS, above.  s_waitcnt vmcnt(0), the other counters
                    //  open; the first building's covers the second one's rows, and behind a first building WITH a battery they have landed)
                    if (m == 0) __builtin_amdgcn_s_waitcnt(0x0F70);
#pragma unroll
                    for (int i = 0; i < VEC; ++i) { o_net[i] = fmaf(c_ns + 0.0f, B.r, sol); soc_rw[i] = 0.0f; o_cb[i] = 0.0f; }
                }
                if constexpr (UNI) {                                      // lean_rewards' default kind at exponent 1
#pragma unroll
                    for (int i = 0; i < VEC; ++i) o_rw[i] = -fmaxf(o_net[i], 0.0f);
                } else cl::lean_rewards_from<VEC>(rkind, B, pb, soc_rw, o_net, o_rw);
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    q_net[i] += o_net[i]; q_cost[i] += cl::mul_rn(o_net[i], R.price); q_em[i] += fmaxf(0.0f, o_net[i] * R.carbon);
                    q_rw[i] += o_rw[i];
                }
            }
            CL_TRACE_AFTER(2 + 4 * m, o_rw[VEC - 1]);
            // ((SC) the lanes that walk the tile for a strip's sake alone store nothing)
            if (!SC || live) {
                if (batt) {
                    pstore<VEC, NT>(a.state + CLS_B_SOC * plane + off, s_soc[m]);
                    pstore<VEC, NT>(a.state + CLS_B_EFF * plane + off, s_eff[m]);
                    pstore<VEC, NT>(a.state + CLS_B_DEGCAP * plane + off, s_deg[m]);
                    if constexpr (F64) {
                        pstore<VEC, NT>(a.state + CLS_B_EFF_LO * plane + off, s_efl[m]);
                        pstore<VEC, NT>(a.state + CLS_B_DEGCAP_LO * plane + off, s_dgl[m]);
                    }
                }
                pstore<VEC, NT>(a.out_bldg + CLO_NET * plane + off, o_net);
                if (rkind != CLR_MARL && !(FLEX && rkind == CLR_EV)) pstore<VEC, NT>(a.out_bldg + CLO_REWARD * plane + off, o_rw);
            }
            if constexpr (KPI && !FLEX) {
                // The streaming KPI accumulators of this building, updated by the wave that holds its step in registers (cl_kpi_bldg_kernel's
                // arithmetic, citylearn.py:1136-1323).  A lean district has no outage and serves its whole load, so the unserved-energy sums
                // do not move; and its baseline -- the net without the battery (building.py:345-366) = load + solar -- and its expected
                // energy do not depend on the env at all: those five sums are kept ONCE per block of CL_ROW0_BLOCK envs (the envs that share
                // a table row), at the block's first env.  Per (env, building) only the four control sums move: 32 B on top of the step's 37.
                // (the four loads are issued together, before the first store.  Fetching them at the top of the kernel with the state planes was
                //  measured and is slower -- 17.8 vs 15.9 us at 17 x 65 536: 117 instead of 89 VGPRs and 32 more floats per lane in the first burst)
                float k_pos[VEC], k_net[VEC], k_em[VEC], k_cost[VEC];
                float* kp = a.kpi_bldg + off;
                vload<VEC>(k_pos, kp + (long long)CLK_C_POS * plane); vload<VEC>(k_net, kp + (long long)CLK_C_NET * plane);
                vload<VEC>(k_em, kp + (long long)CLK_C_EMISSION * plane); vload<VEC>(k_cost, kp + (long long)CLK_C_COST * plane);
                // ... and, in the same burst, the block's five env-independent sums (lane 0 of the block's first workgroup; they were five
                // `+=` statements behind the stores below: five dependent round trips on every wave's way to the reduction)
                const bool block_sums = lane == 0 && (blockIdx.x * TILE) % CL_ROW0_BLOCK == 0;
                float b_pos = 0.0f, b_net = 0.0f, b_em = 0.0f, b_cost = 0.0f, b_exp = 0.0f;
                if (block_sums) {
                    b_pos = kp[(long long)CLK_B_POS * plane]; b_net = kp[(long long)CLK_B_NET * plane];
                    b_em = kp[(long long)CLK_B_EMISSION * plane]; b_cost = kp[(long long)CLK_B_COST * plane];
                    b_exp = kp[(long long)CLK_EXPECTED_ALL * plane];
                }
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    k_pos[i] += fmaxf(o_net[i], 0.0f); k_net[i] += o_net[i];
                    k_em[i] += fmaxf(o_net[i] * R.carbon, 0.0f); k_cost[i] += fmaxf(o_net[i] * R.price, 0.0f);
                }
                pstore<VEC, NT>(kp + (long long)CLK_C_POS * plane, k_pos); pstore<VEC, NT>(kp + (long long)CLK_C_NET * plane, k_net);
                pstore<VEC, NT>(kp + (long long)CLK_C_EMISSION * plane, k_em); pstore<VEC, NT>(kp + (long long)CLK_C_COST * plane, k_cost);
                const float c_ns0 = (quirk && a.t == 0) ? 3.0f * R.nsl : R.nsl;
                const float base = fmaf(c_ns0, B.r, R.sol);                          // the step's net with the battery term left out
                if (lane == 0) lds[(size_t)a.nw * NQ * TILE + b] = base;               // for the district baseline series (below)
                if (block_sums) {                                                      // (lane 0: kp = this building's row at the block's first env)
                    kp[(long long)CLK_B_POS * plane] = b_pos + fmaxf(base, 0.0f);
                    kp[(long long)CLK_B_NET * plane] = b_net + base;
                    kp[(long long)CLK_B_EMISSION * plane] = b_em + fmaxf(base * R.carbon, 0.0f);
                    kp[(long long)CLK_B_COST * plane] = b_cost + fmaxf(base * R.price, 0.0f);
                    kp[(long long)CLK_EXPECTED_ALL * plane] = b_exp + R.nsl;
                }
            }
            if constexpr (OBS) {
                // this building's observation columns, into the workgroup's [64 * VEC envs][pitch] tile (streamed out below)
                float* tile = lds + (size_t)a.nw * NQ * TILE;
#pragma unroll
                for (int k = 0; k < CL_OBS_FUSED_PER_BLDG; ++k) {
                    if (k >= od_n) break;                                                // wave-uniform
                    const int col = od_col[k], src = od_src[k];
                    const float scale = od_scale[k], base = od_base[k];
                    const bool is_out = (src >> 28) == CLOB_KIND_OUT;
                    const int pl = (src >> 20) & 0xFF;
#pragma unroll
                    for (int i = 0; i < VEC; ++i) {
                        const float v = is_out ? (pl == CLO_NET ? o_net[i] : o_rw[i])
                                               : (pl == CLS_B_SOC ? s_soc[m][i] : pl == CLS_B_EFF ? s_eff[m][i] : s_deg[m][i]);
                        tile[(size_t)(lane * VEC + i) * of->pitch + col] = fmaf(v, scale, base);
                    }
                }
            }
            CL_TRACE_AFTER(3 + 4 * m, q_rw[0]);
        }
        if constexpr (SC) {
            // The strip, BEHIND the main building's store burst: its inputs landed with the main building's (requested first, above), its scalars
            // are one group of scalar loads, so nothing between the two pieces of arithmetic waits for a store.  The tile path's expressions at one env per lane.
            if (strip_w) {
                const int b = a.nw;
                const cl::cl_ctab pb = cl::as_ctab(a.params + (long long)b * CL_NP);
                const cl::cl_ctab qb = cl::as_ctab(a.ts + ((long long)ts_row * a.n_bldg + b) * CL_NF);
                cl::BattC bc;
                const float r = cl::pw(pb, CLP_L_TSR);
                cl::load_battc_from(bc, pb);
                const float nsl = cl::pw(qb, CLT_NSL), price = cl::pw(qb, CLT_PRICE), carbon = cl::pw(qb, CLT_CARBON);
                const bool first = quirk && a.t == 0;
                float c_ns = first ? 3.0f * nsl : nsl;
                float sol = cl::pw(qb, CLT_SOLAR);
                const float cbk = first ? 2.0f : 1.0f;
                CL_PIN_V(c_ns); CL_PIN_V(sol);
                __builtin_amdgcn_sched_barrier(0);                     // (as in the tile path: the scalar group is complete at the row's first use)
                CL_PIN_V(x_act);
                cl::State S = {x_soc, x_eff, x_deg, 0.0f, 0.0f, 0.0f};
                const float eb = cl::battery_charge_chain(bc, x_act, INFINITY, S);
                x_net = fmaf(c_ns + cbk * eb, r, sol);
                x_rw = -fmaxf(x_net, 0.0f);
                x_cost = cl::mul_rn(x_net, price); x_em = fmaxf(0.0f, x_net * carbon);
                if (x_live) {
                    const long long xo = (long long)b * a.ld + tile_env0 + x_col;
                    const float v_soc[1] = {S.soc}, v_eff[1] = {S.eff}, v_deg[1] = {S.degcap}, v_net[1] = {x_net}, v_rw[1] = {x_rw};
                    pstore<1, NT>(a.state + CLS_B_SOC * plane + xo, v_soc);
                    pstore<1, NT>(a.state + CLS_B_EFF * plane + xo, v_eff);
                    pstore<1, NT>(a.state + CLS_B_DEGCAP * plane + xo, v_deg);
                    pstore<1, NT>(a.out_bldg + CLO_NET * plane + xo, v_net);
                    pstore<1, NT>(a.out_bldg + CLO_REWARD * plane + xo, v_rw);
                }
            }
        }
    }
    if constexpr (SC) {
        // building nw's four quantities into the row behind the wave rows, strip s in columns 64 s .. 64 s + 63 (district_reduce, STRIPS)
        if (strip_w) {
            float* xr = lds + (size_t)a.nw * NQ * TILE + x_col;
            xr[0 * TILE] = x_net; xr[1 * TILE] = x_cost; xr[2 * TILE] = x_em; xr[3 * TILE] = x_rw;
        }
    }
    if constexpr (OBS) {
        if (w == 0) {                                                              // pad columns: zeros (like cl_observe_f32)
            float* tile = lds + (size_t)a.nw * NQ * TILE;
            for (int c = of->n_cols; c < of->pitch; ++c) {
#pragma unroll
                for (int i = 0; i < VEC; ++i) tile[(size_t)(lane * VEC + i) * of->pitch + c] = 0.0f;
            }
        }
    }
    CL_TRACE_AFTER(13, q_net[0]);
    [[maybe_unused]] KpiSeries base_pre;
    [[maybe_unused]] const bool base_writer = KPI && !FLEX && threadIdx.x == blockDim.x - 1 && (blockIdx.x * TILE) % CL_ROW0_BLOCK == 0;
    if constexpr (KPI && !FLEX) {
        // (the baseline series' accumulators: fetched before the reduction's barriers, by the workgroup's LAST thread -- the first ones
        //  carry the control series)
        if (base_writer) kpi_series_fetch(base_pre, a.kpi_env + (long long)CLKE_PER_COND * a.n_env + blockIdx.x * TILE, a.n_env);
    }
    district_reduce<VEC, FLEX, false, KPI && !FLEX, false, SC>(a, lds, w, lane, env0, live, plane, rkind, q_net, q_cost, q_em, q_rw, a.nw, nullptr, strips);
    if constexpr (KPI && !FLEX) {
        // baseline condition of the district series: the sum of the buildings' baselines in building order, once per env block
        // (district_reduce's barriers came after every wave's write of its buildings' values)
        if (base_writer) {
            float sum = 0.0f;
            for (int b = 0; b < a.n_bldg; ++b) sum += lds[(size_t)a.nw * NQ * TILE + b];
            kpi_series_apply(a.kpi_env + (long long)CLKE_PER_COND * a.n_env + blockIdx.x * TILE, a.n_env, a.t, sum, base_pre);
        }
    }
    if constexpr (OBS) {
        // (district_reduce's first barrier came after every wave's tile writes.)  The tile's rows are consecutive envs: one contiguous
        // block of the observation matrix, streamed out in 16-byte stores.
        typedef float f4 __attribute__((ext_vector_type(4)));
        const int tile_env0 = blockIdx.x * TILE;
        const int rows = min(TILE, a.n_env - tile_env0);
        const f4* src4 = reinterpret_cast<const f4*>(lds + (size_t)a.nw * NQ * TILE);
        f4* dst4 = reinterpret_cast<f4*>(of->obs + (size_t)tile_env0 * of->pitch);
        const int total4 = rows * of->pitch / 4;
        for (int q = threadIdx.x; q < total4; q += blockDim.x) {
            if constexpr (NT) __builtin_nontemporal_store(src4[q], dst4 + q);
            else dst4[q] = src4[q];
        }
    }
    CL_TRACE_FLUSH();
}

// The plain float64-chain launch -- the engine's default precision model, the launch the headline is timed on -- carries both bodies under its
// one kernel symbol (the names a call reports and a profiler sees stay what they are) and branches ONCE, on two kernel arguments: uniform
// district and env-contiguous actions -> lean_step_body<.., UNI>.  A strided action tensor runs the generic body with the hint set.
// (The fp32 launch cl_step_lean_kernel keeps the generic body alone.  With both it measured 6.39 - 6.45 against 6.54 - 6.56 us at 17 x 65 536,
//  but the second copy of the plane loads takes the kernel past the vector-load count tests/test_isa_guards.py pins for it (37 > 32); and ONE
//  copy of the loads in front of the branch costs registers instead -- 101 VGPRs there, 128 + 20 bytes of scratch under the chain.
//  Since the generic body reads its tables by scalar loads it holds 19 vector loads in 73 VGPRs: a second copy would fit now.  Not measured again.)
template <int VEC, bool NT>
CL_DEV void lean_step_dispatch(const StepArgs& a, float* lds) {
    if ((a.flags & CLD_LEAN_UNIFORM) && a.act_stride_env == 1) lean_step_body<VEC, false, NT, false, false, 2, true>(a, lds, nullptr);
    else lean_step_body<VEC, false, NT, false, false, 2>(a, lds, nullptr);
}

template <int VEC, bool FLEX, bool NT>
__global__ void __launch_bounds__(1024) cl_step_lean_kernel(const StepArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    lean_step_body<VEC, FLEX, NT, false>(a, lds, nullptr);
}

// CLD_F64_MAPS: the lean step with the battery map in the reference's precision model (cl::battery_charge_ref) -- same launch shape, two more state planes
template <int VEC, bool NT>
__global__ void __launch_bounds__(1024) cl_step_lean_f64_kernel(const StepArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    lean_step_body<VEC, false, NT, false, false, 1>(a, lds, nullptr);
}

// CLD_F64_CHAIN: the lean step with the soc chain in float64 (cl::battery_charge_chain) -- same launch shape, same three state planes
template <int VEC, bool NT>
__global__ void __launch_bounds__(1024) cl_step_lean_chain_kernel(const StepArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    lean_step_dispatch<VEC, NT>(a, lds);
}

// ... with the streaming KPI accumulators updated by the step launch (cl_step_lean_kpi_kernel's epilogue), and with the compact observation of
// the next row written by it (cl_step_lean_obs_kernel's): the chain changes the battery map, nothing around it
template <int VEC, bool NT>
__global__ void __launch_bounds__(1024) cl_step_lean_kpi_chain_kernel(const StepArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    lean_step_body<VEC, false, NT, false, true, 2>(a, lds, nullptr);
}

template <int VEC, bool NT>
__global__ void __launch_bounds__(1024) cl_step_lean_obs_chain_kernel(const StepArgs a, const ObsFusedArgs of) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    lean_step_body<VEC, false, NT, true, false, 2>(a, lds, &of);
}

template <int VEC, bool NT>
__global__ void __launch_bounds__(1024) cl_step_lean_kpi_kernel(const StepArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    lean_step_body<VEC, false, NT, false, true>(a, lds, nullptr);
}

template <int VEC, bool NT>
__global__ void __launch_bounds__(1024) cl_step_lean_obs_kernel(const StepArgs a, const ObsFusedArgs of) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    lean_step_body<VEC, false, NT, true>(a, lds, &of);
}

// Lean districts, one wave = 64 envs x ALL buildings ("env-major").  The wave issues every state / action load of its
// envs -- 4 dwords per building -- before the first parameter read, then walks the buildings in order while the data streams
// in, storing as it goes: no LDS, no barrier, no cross-wave reduction (the district sums are formed in registers, in building
// order -- the reference's own summation order, citylearn.py:1909-1918).  With one such wave per SIMD the read stream, the
// arithmetic and the write stream of a CU overlap, which the building-major kernels (one generation of waves in lockstep:
// load, then compute, then store) cannot do.  NB = compile-time bound on the buildings held in flight.
// VEC (round 5): envs per lane.  At one env per lane every plane access is a dword per lane -- 256 B per wave instruction; two envs per
// lane (8-byte accesses, 128-thread workgroups so that the env tile still divides CL_ROW0_BLOCK) halve the number of memory instructions
// and of wave-uniform operations per unit, at twice the registers per wave (two waves per SIMD instead of four, the same bytes in flight).
// The district net of building b is parked in the register that held its state of charge (dead by then): no second array for MARL.
// (Round 5, measured and dropped: the action columns through direct-to-LDS loads -- global_load_lds_dword, no vector register holds them
//  while the state planes stream in: 96 instead of 110 registers, five waves per SIMD instead of four -- 17 x 1 048 576: 127.3 - 129.1 us
//  against 125.2 - 125.4 us, alternating on one box (profiles/r05d_*): every load of the wave then has to land before its first building
//  starts, and a fifth wave per SIMD does not pay for that.)
template <int NB, bool NT, int VEC = 1, int PREC = 0>
__global__ void __launch_bounds__(256 / VEC) cl_step_envmajor_kernel(const StepArgs a) {
    constexpr int THREADS = 256 / VEC, TILE = 256;
    const int env = blockIdx.x * TILE + threadIdx.x * VEC;
    const bool live = env < a.n_env;                  // n_env % 4 == 0 (host): a lane's envs are all live or all dead
    const long long plane = (long long)a.n_bldg * a.ld;
    const int rkind = (a.flags & CLD_REWARD_MASK) >> CLD_REWARD_SHIFT;
    const bool quirk = a.flags & CLD_REF_T0_QUIRK;
    const bool act_by_bldg = (a.flags & CLD_ES_COL_IS_BLDG) && a.act_stride_env == 1;
    const int ts_row = a.t + (a.env_row0 ? a.env_row0[(blockIdx.x * TILE) / CL_ROW0_BLOCK] : 0);
    // the buildings' parameter blocks and time-series rows, staged once per workgroup: a wave walking 17 buildings cannot
    // afford a scalar-load round trip per building (16 us at any batch size), and 17 x 36 SGPRs do not exist
    // (PREC == 2, CLD_F64_CHAIN: the chain's float64 constants -- 2 x CLPC_USED words of the CLP_C_* block -- ride behind them)
    constexpr int PW = CLP_L_LAST - CLP_L_FIRST + 1;          // 32 parameter words
    constexpr int CW = PREC == 2 ? 2 * CLPC_USED : 0;
    __shared__ __attribute__((aligned(8))) uint32_t sp[NB][PW + 4 + CW];
    for (int i = threadIdx.x; i < a.n_bldg * (PW + 4 + CW); i += THREADS) {
        const int b = i / (PW + 4 + CW), k = i - b * (PW + 4 + CW);
        uint32_t v;
        if (k < PW) v = a.params[(long long)b * CL_NP + CLP_L_FIRST + k];
        else if (k >= PW + 4) v = a.params[(long long)b * CL_NP + CLP_C_FIRST + (k - (PW + 4))];
        else {
            const float* q = a.ts + ((long long)ts_row * a.n_bldg + b) * CL_NF;
            v = __float_as_uint(k == PW ? q[CLT_NSL] : k == PW + 1 ? q[CLT_SOLAR] : k == PW + 2 ? q[CLT_PRICE] : q[CLT_CARBON]);
        }
        sp[b][k] = v;
    }
    float s_soc[NB][VEC], s_eff[NB][VEC], s_deg[NB][VEC], a_es[NB][VEC];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) s_soc[b][i] = s_eff[b][i] = s_deg[b][i] = a_es[b][i] = 0.0f;
        if (live && b < a.n_bldg) {               // wave-uniform in b; no `break`: it would push the arrays to scratch
            const long long off = (long long)b * a.ld + env;
            // (non-temporal loads here: no effect between 131 072 and 1 048 576 envs, scripts/stream_floor.py -- the copy-floor pattern
            //  gains 9 % from them at 1 048 576 envs, 120 -> 109 us; this kernel's 4-byte-per-lane loads do not)
            vload<VEC>(s_soc[b], a.state + CLS_B_SOC * plane + off);
            vload<VEC>(s_eff[b], a.state + CLS_B_EFF * plane + off);
            vload<VEC>(s_deg[b], a.state + CLS_B_DEGCAP * plane + off);
            if (act_by_bldg) vload<VEC>(a_es[b], a.actions + (long long)b * a.act_stride_col + env);
        }
    }
    __syncthreads();
    if (!live) return;
    float q_net[VEC], q_cost[VEC], q_em[VEC], q_rw[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) q_net[i] = q_cost[i] = q_em[i] = q_rw[i] = 0.0f;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (b >= a.n_bldg) continue;
        cl::Bp B;
        cl::load_bp<false>(B, &sp[b][0] - CLP_L_FIRST);           // the CLP_L_* block, from LDS (uniform address: a broadcast read)
        cl::Row R;
        R.nsl = __uint_as_float(sp[b][PW]); R.sol = __uint_as_float(sp[b][PW + 1]);
        R.price = __uint_as_float(sp[b][PW + 2]); R.carbon = __uint_as_float(sp[b][PW + 3]);
        R.outage = false;
        const long long off = (long long)b * a.ld + env;
        const bool batt = B.flags & CLF_BATTERY;
        float o_soc[VEC], o_eff[VEC], o_deg[VEC], o_net[VEC], o_rw[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            float act_v = 0.0f;
            if (B.a_es >= 0) act_v = act_by_bldg ? a_es[b][i] : a.actions[(long long)B.a_es * a.act_stride_col + (long long)(env + i) * a.act_stride_env];
            cl::State S;
            S.soc = batt ? s_soc[b][i] : 0.0f; S.eff = batt ? s_eff[b][i] : 1.0f; S.degcap = batt ? s_deg[b][i] : 0.0f;
            S.cs = S.hs = S.ds = 0.0f;
            const cl::Act act = {0.0f, 0.0f, 0.0f, act_v, 0.0f, 0.0f};
            cl::Out O;
            if constexpr (PREC == 2) {
                // the lean unit around cl::battery_charge_chain (same lines as cl::unit_step<false, 2>), its constants read from the LDS copy
                float eb = 0.0f;
                if (batt) {
                    cl::BattC bc;
                    cl::load_battc64(bc, &sp[b][0] + (PW + 4) - CLP_C_FIRST);
                    bc.cap32 = B.batt.cap; bc.omd32 = B.batt.omd; bc.degk = B.batt.degk;       // (the CLP_L_* words: already here)
                    eb = cl::battery_charge_chain(bc, act_v, INFINITY, S);
                }
                const bool first = quirk && a.t == 0;
                const float c_ns = first ? 3.0f * R.nsl : R.nsl, c_b = first ? 2.0f * eb : eb;
                O.net = fmaf(c_ns + c_b, B.r, R.sol); O.cost = cl::mul_rn(O.net, R.price); O.emission = fmaxf(0.0f, O.net * R.carbon);
            } else cl::unit_step<false>(B, R, a.t, quirk, act, S, O);
            o_soc[i] = S.soc; o_eff[i] = S.eff; o_deg[i] = S.degcap; o_net[i] = O.net;
            o_rw[i] = cl::unit_reward<false>(rkind, B, S, O.net);
            s_soc[b][i] = O.net;                                  // (MARL's second sweep reads the nets from here)
            q_net[i] += O.net; q_cost[i] += O.cost; q_em[i] += O.emission; q_rw[i] += o_rw[i];
        }
        if (batt) {
            pstore<VEC, NT>(a.state + CLS_B_SOC * plane + off, o_soc);
            pstore<VEC, NT>(a.state + CLS_B_EFF * plane + off, o_eff);
            pstore<VEC, NT>(a.state + CLS_B_DEGCAP * plane + off, o_deg);
        }
        pstore<VEC, NT>(a.out_bldg + CLO_NET * plane + off, o_net);
        if (rkind != CLR_MARL) pstore<VEC, NT>(a.out_bldg + CLO_REWARD * plane + off, o_rw);
    }
    if (rkind == CLR_MARL) {                      // reward_function.py:132-143: every building against the district net
#pragma unroll
        for (int i = 0; i < VEC; ++i) q_rw[i] = 0.0f;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (b >= a.n_bldg) continue;
            float rw[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) { rw[i] = cl::marl_reward(s_soc[b][i], q_net[i]); q_rw[i] += rw[i]; }
            vstore<VEC>(a.out_bldg + CLO_REWARD * plane + (long long)b * a.ld + env, rw);
        }
    }
    vstore<VEC>(a.out_env + (long long)CLQ_NET * a.n_env + env, q_net);
    vstore<VEC>(a.out_env + (long long)CLQ_COST * a.n_env + env, q_cost);
    vstore<VEC>(a.out_env + (long long)CLQ_EMISSION * a.n_env + env, q_em);
    vstore<VEC>(a.out_env + (long long)CLQ_REWARD * a.n_env + env, q_rw);
}

// (Round 6, measured and dropped -- two attempts at the HBM-streaming shape, 17 x 1 048 576 envs, profiles/r06d_streaming_ab.log:
//  (1) a PERSISTENT, software-pipelined form: 768 workgroups walking several env tiles each, the registers of building b re-filled with the next tile's
//  planes as soon as building b of the current tile is computed, on the theory that the plain kernel's four resident generations run in lockstep -- a
//  164 MB load burst, then arithmetic with the read path idle, four times over.  The 68 loop-carried plane registers + the unit's temporaries need 168
//  registers (three waves per SIMD, still 112 / 160 bytes of scratch in the fp32 / chain instantiation), the compiler's s_waitcnt placement needs a
//  static building count and a branch-free tile loop to keep the prefetches in flight at all, and the result is 155 - 178 us (fp32) / 228 - 271 us
//  (chain) against 124 - 126 / 134 us: a wave that issues four loads per building paces its memory requests by its own arithmetic.
//  (2) narrower workgroups (one or two waves instead of four, so that waves retire and start one at a time): 142 / 158 us against 134 us.
//  What this shape wants is what it has: every load of a wave issued up front, sixteen waves per CU.)
// (Round 5, measured and dropped -- a building-major kernel for the streaming regime: four-wave workgroups over 256 envs at four envs per lane,
//  wave w taking buildings w, w + 4, ..., all plane loads up front like above but 1 KB per wave instruction instead of 256 B, parameters from an
//  LDS copy, 148 VGPRs = three waves per SIMD.  17 x 1 048 576, alternating runs on one box (profiles/r05g_*): 114.9 / 129.1 / 129.2 us against
//  115.9 / 120.4 / 125.8 us for this kernel -- the same range; each PROCESS lands somewhere in it and stays there for thousands of launches (not a
//  function of the planes' virtual addresses: profiles/r05i_placement.log).  17 x 262 144: 30.9 vs 26.0 us.  Wider accesses are not what this shape lacks.)
/* (cl_noslp_tu.hip compiles only what its two kernels need; cl_policy_full.hip keeps cl_full.h without these passes; CL_TU_FINISH: cl_policy_full_chunk.hip
   keeps the first of them, the fold of the chunk partial sums) */
#if (!defined(CL_TU_NOSLP) && !defined(CL_TU_POLICY_FULL)) || defined(CL_TU_FINISH)
// Second pass for building-chunked launches: add the per-chunk partial district sums.  One workgroup = 64 envs x ONE district
// quantity x 16 waves; wave w adds chunks w, w+16, ... (independent loads issued four at a time: one memory round trip for up
// to 64 chunks), then the 16 wave partials are summed in a fixed order through LDS -- deterministic.  (The first version let one
// workgroup walk all four quantities of its 64 envs: 16 workgroups and four dependent rounds at 1024 envs, 4.7 us of a 22 us step.)
// `deferred` (cl_finish_f32): fold buffer t & 1 of the double-buffered scratch rows, and only if its marker says it holds step t's sums.
// `ret_env` (chunked fused rollout, cl_rollout_f32): workgroup row NQ adds the chunks' shares of the K-step return -- one scratch row per
// chunk behind the n_chunks x NQ partial sums -- to ret_env, in the same association.
__global__ void __launch_bounds__(1024) cl_finish_kernel(const StepArgs a, const int deferred, float* __restrict__ ret_env) {
    __shared__ float part[16][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + lane;
    const int q = blockIdx.y;
    const long long plane = (long long)a.n_bldg * a.n_env;
    const float* scratch = a.out_bldg + (long long)CLO_RESERVED * plane;
    int n_chunks = a.n_chunks;
    if (!deferred && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)         // (this step did not defer: see district_reduce)
        reinterpret_cast<unsigned*>(a.out_bldg + (long long)(CLO_RESERVED + 1) * plane - 4)[a.t & 1] = 0u;
    if (deferred) {
        const unsigned* marker = reinterpret_cast<const unsigned*>(a.out_bldg + (long long)(CLO_RESERVED + 1) * plane - 4);
        if (marker[a.t & 1] != (unsigned)a.t + 1u) return;                   // (uniform) step t did not defer its finish: out_env is already final
        n_chunks = (int)marker[2];
        scratch += (long long)(a.t & 1) * n_chunks * NQ * a.n_env;
    }
    const int rkind = (a.flags & CLD_REWARD_MASK) >> CLD_REWARD_SHIFT;
    const bool marl = rkind == CLR_MARL && q == CLQ_REWARD;      // partials carried sign(-net) * 0.01 * net^2: scale by max(0, district net)
    float s = 0.0f, sn = 0.0f;
    if (e < a.n_env) {
        for (int c0 = w; c0 < n_chunks; c0 += 64) {
            float v[4], vn[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = c0 + 16 * j;
                v[j] = c < n_chunks ? scratch[(q < NQ ? (long long)c * NQ + q : (long long)n_chunks * NQ + c) * a.n_env + e] : 0.0f;
                vn[j] = (marl && c < n_chunks) ? scratch[((long long)c * NQ + CLQ_NET) * a.n_env + e] : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) { s += v[j]; sn += vn[j]; }
        }
    }
    part[w][lane] = s;
    __syncthreads();
    float t = 0.0f;
    if (w == 0) {
#pragma unroll
        for (int k = 0; k < 16; ++k) t += part[k][lane];
    }
    if (marl) {                                  // the district net, summed in the same order as the CLQ_NET workgroup does
        __syncthreads();
        part[w][lane] = sn;
        __syncthreads();
        if (w == 0) {
            float n = 0.0f;
#pragma unroll
            for (int k = 0; k < 16; ++k) n += part[k][lane];
            t *= fmaxf(0.0f, n);
        }
    }
    if (w == 0 && e < a.n_env) {
        if (q < NQ) a.out_env[(long long)q * a.n_env + e] = t;
        else ret_env[e] += t;
    }
}

// (host) The fold behind a building-chunked K-step launch -- the last step's district sums and, with `ret_env`, the K-step return: one launch of
// NQ (+ 1) workgroup rows at step t_last.  cl_rollout_f32 and the three chunked policy entries each spelled this as `StepArgs f = a;
// f.t = t0 + k_steps - 1; ...`; this is the one copy.
inline int launch_rollout_finish(const cl_tuning& tun, const StepArgs& a, int t_last, float* ret_env, hipStream_t stream) {
    StepArgs f = a;
    f.t = t_last;
    name_add(tun, "cl_finish_kernel");
    hipLaunchKernelGGL(cl_finish_kernel, dim3((a.n_env + 63) / 64, NQ + (ret_env ? 1 : 0)), dim3(1024), 0, stream, f, 0, ret_env);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_fail(e, "cl_finish_kernel launch");
    return CL_OK;
}
#endif  // cl_finish_kernel

#if !defined(CL_TU_NOSLP) && !defined(CL_TU_POLICY_FULL)
// ---- streaming KPI accumulators (CLD_KPI): two small passes over the detail planes the step kernel just wrote ----
__global__ void cl_kpi_bldg_kernel(const StepArgs a) {
    const long long plane = (long long)a.n_bldg * a.n_env;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= plane) return;
    const int b = (int)(i / a.n_env);
    const int ts_row = a.t + (a.env_row0 ? a.env_row0[(int)(i - (long long)b * a.n_env) / CL_ROW0_BLOCK] : 0);
    const float* q = a.ts + ((long long)ts_row * a.n_bldg + b) * CL_NF;
    const float price = q[CLT_PRICE], carbon = q[CLT_CARBON];
    const bool outage = q[CLT_OUTAGE] != 0.0f;
    const float net = a.out_bldg[CLO_NET * plane + i], base = a.out_bldg[CLO_BASE_NET * plane + i];
    const float ex = a.out_bldg[CLO_EXPECTED * plane + i], sv = a.out_bldg[CLO_SERVED * plane + i];
    float* k = a.kpi_bldg + i;
    k[CLK_C_POS * plane] += fmaxf(net, 0.0f);
    k[CLK_C_NET * plane] += net;
    k[CLK_C_EMISSION * plane] += fmaxf(net * carbon, 0.0f);
    k[CLK_C_COST * plane] += fmaxf(net * price, 0.0f);
    k[CLK_B_POS * plane] += fmaxf(base, 0.0f);
    k[CLK_B_NET * plane] += base;
    k[CLK_B_EMISSION * plane] += fmaxf(base * carbon, 0.0f);
    k[CLK_B_COST * plane] += fmaxf(base * price, 0.0f);
    if (outage) { k[CLK_UNSERVED_OUTAGE * plane] += ex - sv; k[CLK_EXPECTED_OUTAGE * plane] += ex; }
    k[CLK_UNSERVED_ALL * plane] += ex - sv;
    k[CLK_EXPECTED_ALL * plane] += ex;
}

CL_DEV void kpi_series_fetch(KpiSeries& s, const float* __restrict__ k, long long n_env) {
    s.prev = k[CLKE_PREV * n_env]; s.ramp = k[CLKE_RAMP * n_env];
    s.dsum = k[CLKE_DAY_SUM * n_env]; s.dmax = k[CLKE_DAY_MAX * n_env];
    s.msum = k[CLKE_MON_SUM * n_env]; s.mmax = k[CLKE_MON_MAX * n_env];
    s.amax = k[CLKE_ALL_MAX * n_env];
}

CL_DEV void kpi_series_apply(float* __restrict__ k, long long n_env, int t, float v, const KpiSeries& s) {
    // one more sample `v` (index t) of a district series: ramping, 24- and 730-step load factor / peak groups
    if (t > 0) k[CLKE_RAMP * n_env] = s.ramp + fmaxf(v - s.prev, 0.0f);
    k[CLKE_PREV * n_env] = v;
    float dsum = s.dsum, dmax = s.dmax;
    if (t > 0 && t % 24 == 0) {
        k[CLKE_DAY_LF_SUM * n_env] += 1.0f - (dsum * (1.0f / 24.0f)) / dmax;
        k[CLKE_DAY_PEAK_SUM * n_env] += dmax;
        k[CLKE_DAY_N * n_env] += 1.0f;
        dsum = 0.0f; dmax = -INFINITY;
    }
    k[CLKE_DAY_SUM * n_env] = dsum + v; k[CLKE_DAY_MAX * n_env] = fmaxf(dmax, v);
    float msum = s.msum, mmax = s.mmax;
    if (t > 0 && t % 730 == 0) {
        k[CLKE_MON_LF_SUM * n_env] += 1.0f - (msum * (1.0f / 730.0f)) / mmax;
        k[CLKE_MON_N * n_env] += 1.0f;
        msum = 0.0f; mmax = -INFINITY;
    }
    k[CLKE_MON_SUM * n_env] = msum + v; k[CLKE_MON_MAX * n_env] = fmaxf(mmax, v);
    k[CLKE_ALL_MAX * n_env] = fmaxf(s.amax, v);
}

CL_DEV void kpi_series_update(float* __restrict__ k, long long n_env, int t, float v) {
    KpiSeries s;
    kpi_series_fetch(s, k, n_env);
    kpi_series_apply(k, n_env, t, v, s);
}

// District series: control = out_env net; baseline = sum over buildings of the baseline plane (16 waves share the
// building loop, fixed-order LDS sum).
__global__ void __launch_bounds__(1024) cl_kpi_env_kernel(const StepArgs a) {
    __shared__ float part[16][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + lane;
    const long long plane = (long long)a.n_bldg * a.n_env;
    float s = 0.0f;
    if (e < a.n_env)
        for (int b = w; b < a.n_bldg; b += 16) s += a.out_bldg[CLO_BASE_NET * plane + (long long)b * a.n_env + e];
    part[w][lane] = s;
    __syncthreads();
    if (w == 0 && e < a.n_env) {
        float base = 0.0f;
#pragma unroll
        for (int k = 0; k < 16; ++k) base += part[k][lane];
        KpiSeries sc, sb;                       // both series' accumulators first, then the stores (one round trip instead of ten)
        kpi_series_fetch(sc, a.kpi_env + e, a.n_env);
        kpi_series_fetch(sb, a.kpi_env + (long long)CLKE_PER_COND * a.n_env + e, a.n_env);
        const float dnet = a.out_env[(long long)CLQ_NET * a.n_env + e];
        kpi_series_apply(a.kpi_env + e, a.n_env, a.t, dnet, sc);
        kpi_series_apply(a.kpi_env + (long long)CLKE_PER_COND * a.n_env + e, a.n_env, a.t, base, sb);
    }
}

// The two passes above in ONE launch (round 3): a workgroup = 64 envs x every building (16 waves share the building loop); a wave updates
// the per-building accumulators of its buildings from the planes the step just wrote and keeps the baseline partial sum of its envs in a
// register, the 16 partials are added in wave order through LDS (the order cl_kpi_env_kernel used: same bits) and wave 0 feeds the two
// district series.  One launch and one read of the baseline plane less per step.
__global__ void __launch_bounds__(1024) cl_kpi_kernel(const StepArgs a) {
    __shared__ float part[16][64];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int e = blockIdx.x * 64 + lane;
    const bool live = e < a.n_env;
    const long long plane = (long long)a.n_bldg * a.n_env;
    const int ts_row = a.t + (a.env_row0 ? a.env_row0[(blockIdx.x * 64) / CL_ROW0_BLOCK] : 0);      // 64 divides CL_ROW0_BLOCK: workgroup-uniform
    float s = 0.0f;
    for (int b = w; b < a.n_bldg; b += 16) {
        const float* __restrict__ q = a.ts + ((long long)ts_row * a.n_bldg + b) * CL_NF;
        const float price = q[CLT_PRICE], carbon = q[CLT_CARBON];
        const bool outage = q[CLT_OUTAGE] != 0.0f;
        if (!live) continue;
        const long long i = (long long)b * a.n_env + e;
        const float net = a.out_bldg[CLO_NET * plane + i], base = a.out_bldg[CLO_BASE_NET * plane + i];
        const float ex = a.out_bldg[CLO_EXPECTED * plane + i], sv = a.out_bldg[CLO_SERVED * plane + i];
        // every accumulator is LOADED before the first one is stored: `k[p * plane] += x` one after the other is a chain of dependent
        // round trips (a store to k[p * plane] may alias the next load as far as the compiler knows) -- that chain, not the bytes, was
        // the 20 us of the round-2 passes
        float* k = a.kpi_bldg + i;
        float v[CL_NKB];
#pragma unroll
        for (int p = 0; p < CL_NKB; ++p) v[p] = (outage || (p != CLK_UNSERVED_OUTAGE && p != CLK_EXPECTED_OUTAGE)) ? k[p * plane] : 0.0f;
        v[CLK_C_POS] += fmaxf(net, 0.0f);
        v[CLK_C_NET] += net;
        v[CLK_C_EMISSION] += fmaxf(net * carbon, 0.0f);
        v[CLK_C_COST] += fmaxf(net * price, 0.0f);
        v[CLK_B_POS] += fmaxf(base, 0.0f);
        v[CLK_B_NET] += base;
        v[CLK_B_EMISSION] += fmaxf(base * carbon, 0.0f);
        v[CLK_B_COST] += fmaxf(base * price, 0.0f);
        v[CLK_UNSERVED_OUTAGE] += ex - sv; v[CLK_EXPECTED_OUTAGE] += ex;
        v[CLK_UNSERVED_ALL] += ex - sv;
        v[CLK_EXPECTED_ALL] += ex;
#pragma unroll
        for (int p = 0; p < CL_NKB; ++p)
            if (outage || (p != CLK_UNSERVED_OUTAGE && p != CLK_EXPECTED_OUTAGE)) k[p * plane] = v[p];       // (row-uniform: the outage sums are untouched otherwise)
        s += base;
    }
    part[w][lane] = s;
    __syncthreads();
    if (w == 0 && live) {
        float base = 0.0f;
#pragma unroll
        for (int k = 0; k < 16; ++k) base += part[k][lane];
        KpiSeries sc, sb;                       // both series' accumulators first, then the stores (one round trip instead of ten)
        kpi_series_fetch(sc, a.kpi_env + e, a.n_env);
        kpi_series_fetch(sb, a.kpi_env + (long long)CLKE_PER_COND * a.n_env + e, a.n_env);
        const float dnet = a.out_env[(long long)CLQ_NET * a.n_env + e];
        kpi_series_apply(a.kpi_env + e, a.n_env, a.t, dnet, sc);
        kpi_series_apply(a.kpi_env + (long long)CLKE_PER_COND * a.n_env + e, a.n_env, a.t, base, sb);
    }
}

// Third pass, MARL only: per-building rewards need the finished district net.
__global__ void cl_marl_reward_kernel(const StepArgs a) {
    const long long plane = (long long)a.n_bldg * a.n_env;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= plane) return;
    const int e = (int)(i % a.n_env);
    a.out_bldg[CLO_REWARD * plane + i] = cl::marl_reward(a.out_bldg[CLO_NET * plane + i], a.out_env[(long long)CLQ_NET * a.n_env + e]);
}

__global__ void cl_reset_kernel(const uint32_t* __restrict__ params, float* __restrict__ state,
                                float* __restrict__ kpi_bldg, float* __restrict__ kpi_env, int n_env, int n_bldg, uint32_t flags, int ld) {
    // (`ld`: cl_dims.env_pitch -- the pad entries of a row are initialised like its envs; the KPI planes are never pitched: host)
    const long long plane = (long long)n_bldg * ld;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < plane) {
        const int b = (int)(i / ld);
        const uint32_t* p = params + (long long)b * CL_NP;
        if (state) {
            state[CLS_B_SOC * plane + i] = __uint_as_float(p[CLP_L_SOC0]);
            state[CLS_B_EFF * plane + i] = __uint_as_float(p[CLP_L_EFF0]);
            // (CLD_F64_CHAIN: the plane carries the capacity LOSS, capacity - degraded_capacity: nothing lost yet)
            state[CLS_B_DEGCAP * plane + i] = (flags & CLD_F64_CHAIN) ? 0.0f : __uint_as_float(p[CLP_L_CAP]);
            state[CLS_CS_SOC * plane + i] = __uint_as_float(p[CLP_CS_SOC0]);
            state[CLS_HS_SOC * plane + i] = __uint_as_float(p[CLP_HS_SOC0]);
            state[CLS_DS_SOC * plane + i] = __uint_as_float(p[CLP_DS_SOC0]);
            // CLD_F64_MAPS: what the float32 planes above lose of the two float64 start values (Battery.reset, energy_model.py:1237-1242)
            const double eff0 = cl::pd(p, CLPD_EFF0), cap0 = cl::pd(p, CLPD_CAP);
            state[CLS_B_EFF_LO * plane + i] = (float)(eff0 - (double)__uint_as_float(p[CLP_L_EFF0]));
            state[CLS_B_DEGCAP_LO * plane + i] = (float)(cap0 - (double)__uint_as_float(p[CLP_L_CAP]));
        }
        if (kpi_bldg)
            for (int k = 0; k < CL_NKB; ++k) kpi_bldg[k * plane + i] = 0.0f;
    }
    if (kpi_env && i < n_env)
        for (int k = 0; k < CL_NKE; ++k) {
            const int kk = k % CLKE_PER_COND;
            const bool is_max = kk == CLKE_DAY_MAX || kk == CLKE_MON_MAX || kk == CLKE_ALL_MAX;
            kpi_env[(long long)k * n_env + i] = is_max ? -INFINITY : 0.0f;
        }
}
#endif  // CL_TU_NOSLP, CL_TU_POLICY_FULL

}  // namespace

#ifndef CL_TU_NOSLP
#include "cl_full.h"
#endif
#include "cl_rollout.h"

// Two kernels live in a translation unit of their own (cl_noslp_tu.hip = this file with CL_TU_NOSLP, built with -fno-slp-vectorize):
// with several envs per lane the SLP vectoriser packs the envs' identical fp32 operations into v_pk_*_f32, which cost more than the
// plain operations they replace.  Measured with both builds alternating on one box (profiles/r02e_noslp_ab2.log, r02f_noslp_lean_ab.log):
//   fused rollout   17 x 32 768: 2.34 -> 2.14 us per step, 65 536: 4.26 -> 3.88
//   lean step       17 x 65 536 (the headline launch, four envs per lane, 292 packed operations): 7.24 / 6.92 / 7.24 / 7.28 us with,
//                   7.02 / 6.84 / 6.88 / 6.70 us without
// The same switch is a loss for the LSTM kernel (109.8 -> 115.5 us) and the chunked thermal launches (14.75 -> 15.08 us) and within
// the noise for the env-major kernel, hence per translation unit and not for the whole library.  The lean launches with a fused
// epilogue (flexible loads, KPI accumulators, observation tile) were not measured and stay in the main unit.
extern "C" __attribute__((visibility("hidden"))) int cl_tu_launch_rollout(int key, int pin, unsigned grid, unsigned grid_y, unsigned block, size_t lds,
                                                                          void* stream, const void* rollout_args);
extern "C" __attribute__((visibility("hidden"))) int cl_tu_launch_lean(int vec, int nt, unsigned grid_x, unsigned grid_y, unsigned block, size_t lds,
                                                                       void* stream, const void* step_args);

#if defined(CL_TU_POLICY)
// (cl_policy.hip: the helpers and cl_rollout.h above are all it takes from this file -- its kernel, launcher and entry points are its own)
#elif defined(CL_TU_NOSLP)
extern "C" __attribute__((visibility("hidden"))) int cl_tu_launch_rollout(int key, int pin, unsigned grid_x, unsigned grid_y, unsigned block_threads, size_t lds,
                                                                          void* stream, const void* rollout_args) {
    const RolloutArgs& r = *static_cast<const RolloutArgs*>(rollout_args);       // the struct of the including translation unit: same source
    const dim3 block(block_threads), grid(grid_x, grid_y);
    hipStream_t s = (hipStream_t)stream;
    switch (key) {        // (full ? 100 : 0) + 10 * envs per lane + buildings per wave
    case 11: hipLaunchKernelGGL((cl_rollout_kernel<1, false, 1>), grid, block, lds, s, r); break;
    case 12:
        if (pin) hipLaunchKernelGGL((cl_rollout_kernel<1, false, 2>), grid, block, lds, s, r);
        else hipLaunchKernelGGL((cl_rollout_kernel<1, false, 2, false>), grid, block, lds, s, r);      // whole launch resident at once: see PIN
        break;
    case 21: hipLaunchKernelGGL((cl_rollout_kernel<2, false, 1>), grid, block, lds, s, r); break;
    case 22: hipLaunchKernelGGL((cl_rollout_kernel<2, false, 2>), grid, block, lds, s, r); break;
    case 111: hipLaunchKernelGGL((cl_rollout_kernel<1, true, 1>), grid, block, lds, s, r); break;
    // CLD_F64_CHAIN (one env per lane: 2000 + key)
    case 2012: hipLaunchKernelGGL((cl_rollout_kernel<1, false, 2, true, false, 2>), grid, block, lds, s, r); break;
    case 2022: hipLaunchKernelGGL((cl_rollout_kernel<2, false, 2, true, false, 2>), grid, block, lds, s, r); break;
    case 2111: hipLaunchKernelGGL((cl_rollout_kernel<1, true, 1, true, false, 2>), grid, block, lds, s, r); break;
    case 3012: hipLaunchKernelGGL((cl_rollout_kernel<1, false, 2, true, true, 2>), grid, block, lds, s, r); break;
    case 3022: hipLaunchKernelGGL((cl_rollout_kernel<2, false, 2, true, true, 2>), grid, block, lds, s, r); break;
    case 3111: hipLaunchKernelGGL((cl_rollout_kernel<1, true, 1, true, true, 2>), grid, block, lds, s, r); break;
    // building-chunked districts (gridDim.y workgroup rows; cl_rollout.h)
    case 1012: hipLaunchKernelGGL((cl_rollout_kernel<1, false, 2, true, true>), grid, block, lds, s, r); break;
    case 1022: hipLaunchKernelGGL((cl_rollout_kernel<2, false, 2, true, true>), grid, block, lds, s, r); break;
    case 1111: hipLaunchKernelGGL((cl_rollout_kernel<1, true, 1, true, true>), grid, block, lds, s, r); break;
    // with the streaming KPI accumulators (cl_rollout_kpi_kernel; 4000 + 10 * envs per lane + 2, + 2000 under CLD_F64_CHAIN)
#define CL_TU_RKPI(V, P) do { \
        if (lds > 64 * 1024) if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(cl_rollout_kpi_kernel<V, P>), lds); e != hipSuccess) return (int)e; \
        hipLaunchKernelGGL((cl_rollout_kpi_kernel<V, P>), grid, block, lds, s, r); } while (0)
    case 4012: CL_TU_RKPI(1, 0); break;
    case 4022: CL_TU_RKPI(2, 0); break;
    case 6012: CL_TU_RKPI(1, 2); break;
    case 6022: CL_TU_RKPI(2, 2); break;
#undef CL_TU_RKPI
    default: return -1;
    }
    return (int)hipGetLastError();
}

extern "C" __attribute__((visibility("hidden"))) int cl_tu_launch_lean(int vec, int nt, unsigned grid_x, unsigned grid_y, unsigned block_threads,
                                                                       size_t lds, void* stream, const void* step_args) {
    const StepArgs& a = *static_cast<const StepArgs*>(step_args);
    const dim3 grid(grid_x, grid_y), block(block_threads);
    hipStream_t s = (hipStream_t)stream;
#define CL_TU_LEAN(V) case V: \
        if (nt) hipLaunchKernelGGL((cl_step_lean_kernel<V, false, true>), grid, block, lds, s, a); \
        else hipLaunchKernelGGL((cl_step_lean_kernel<V, false, false>), grid, block, lds, s, a); \
        break;
    switch (vec) {
        CL_TU_LEAN(1) CL_TU_LEAN(2) CL_TU_LEAN(4)
    default: return -1;
    }
#undef CL_TU_LEAN
    return (int)hipGetLastError();
}
#else

#include "cl_lstm.h"
#include "cl_observe.h"

namespace {

// Launch-geometry overrides travel with every call (cl_dims.tuning, include/citylearn_amd.h): the library holds no
// mutable state besides the thread-local error string.
const cl_tuning k_default_tuning = {};
const cl_tuning& tuning_of(const cl_dims* d) { return d->tuning ? *d->tuning : k_default_tuning; }

}  // namespace


namespace {
// The rollout policy as planes of actions (same stream as cl_rollout_kernel: a = low + u (high - low),
// u = Philox4x32-10(seed; env, column, t)) -- for districts whose state machines live in HBM between steps.  One Philox
// block holds the draws of four consecutive steps (word t & 3 of block t >> 2), so one launch fills the four planes
// actions[t & 3][column][env] of steps 4 tq .. 4 tq + 3 (one plane per launch measured 19 us at 26 x 65 536: the ten
// rounds of quarter-rate 32-bit multiplies, three of four words thrown away).
__global__ void cl_policy_kernel(float* __restrict__ actions, const float* __restrict__ low, const float* __restrict__ high,
                                 unsigned long long seed, int n_env, int n_cols, int tq, unsigned env_offset) {
    const int env = blockIdx.x * blockDim.x + threadIdx.x, col = blockIdx.y;
    if (env >= n_env) return;
    const float lo = low[col], span = high[col] - lo;
    const cl::U4 blk = cl::philox_block(seed, (uint32_t)env + env_offset, (uint32_t)col, (uint32_t)tq);
#pragma unroll
    for (int w = 0; w < 4; ++w) actions[((long long)w * n_cols + col) * n_env + env] = fmaf(cl::u01(blk.w[w]), span, lo);
}

__global__ void cl_kpi_comfort_reset_kernel(float* k, long long plane) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= plane) return;
    for (int p = 0; p < CL_NKC; ++p) k[p * plane + i] = 0.0f;
    k[CLKC_COLD_MIN * plane + i] = INFINITY; k[CLKC_HOT_MIN * plane + i] = INFINITY;
    k[CLKC_COLD_MAX * plane + i] = -INFINITY; k[CLKC_HOT_MAX * plane + i] = -INFINITY;
}

__global__ void cl_return_kernel(float* __restrict__ ret_env, const float* __restrict__ reward, int n_env) {
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env < n_env) ret_env[env] += reward[env];
}

// The instantiation a plan launches, one switch over the kernel families (plan_name in cl_plan.h spells the same plan fields).  The fp32 lean
// kernel without flexible loads is not here: it lives in the no-SLP unit (cl_tu_launch_lean).
const void* step_kernel_fn(const StepPlan& p) {
#define CL_K(...) reinterpret_cast<const void*>(__VA_ARGS__)
#define CL_NT(K, ...) (p.nt ? CL_K(K<__VA_ARGS__, true>) : CL_K(K<__VA_ARGS__, false>))
#define CL_V124(K) (p.vec == 1 ? CL_NT(K, 1) : p.vec == 2 ? CL_NT(K, 2) : CL_NT(K, 4))
#define CL_LC(V, F, P) (p.nt ? CL_K(cl_step_lean_chunk_kernel<V, true, F, P>) : CL_K(cl_step_lean_chunk_kernel<V, false, F, P>))
#define CL_LC_V(F, P) (p.vec == 1 ? CL_LC(1, F, P) : p.vec == 2 ? CL_LC(2, F, P) : CL_LC(4, F, P))
#define CL_EM(NB, V, P) (p.nt ? CL_K(cl_step_envmajor_kernel<NB, true, V, P>) : CL_K(cl_step_envmajor_kernel<NB, false, V, P>))
    switch (p.kernel) {
    case CLK_STEP:
        if (p.check)
            return p.flex ? CL_K(cl_step_kernel<1, true, true, true, 0, false, true>) : p.prec == 2 ? CL_K(cl_step_kernel<1, true, true, false, 2, false, true>)
                 : p.prec == 1 ? CL_K(cl_step_kernel<1, true, true, false, 1, false, true>) : CL_K(cl_step_kernel<1, true, true, false, 0, false, true>);
        if (p.fold) return p.vec == 1 ? CL_K(cl_step_kernel<1, false, false, false, 0, true>) : CL_K(cl_step_kernel<4, false, false, false, 0, true>);
        if (p.prec == 2)
            return p.full ? (p.det ? CL_K(cl_step_kernel<1, true, true, false, 2>) : CL_K(cl_step_kernel<1, true, false, false, 2>))
                 : p.vec == 1 ? CL_K(cl_step_kernel<1, false, false, false, 2>) : p.vec == 2 ? CL_K(cl_step_kernel<2, false, false, false, 2>)
                 : CL_K(cl_step_kernel<4, false, false, false, 2>);
        if (p.prec == 1)
            return p.full ? (p.det ? CL_K(cl_step_kernel<1, true, true, false, 1>) : CL_K(cl_step_kernel<1, true, false, false, 1>))
                 : p.vec == 1 ? CL_K(cl_step_kernel<1, false, false, false, 1>) : CL_K(cl_step_kernel<2, false, false, false, 1>);
        if (p.flex)
            return p.det ? (p.vec == 1 ? CL_K(cl_step_kernel<1, true, true, true>) : CL_K(cl_step_kernel<2, true, true, true>))
                 : p.full ? (p.vec == 1 ? CL_K(cl_step_kernel<1, true, false, true>) : CL_K(cl_step_kernel<2, true, false, true>))
                 : p.vec == 1 ? CL_K(cl_step_kernel<1, false, false, true>) : CL_K(cl_step_kernel<2, false, false, true>);
        if (p.full)
            return p.det ? (p.vec == 1 ? CL_K(cl_step_kernel<1, true, true>) : CL_K(cl_step_kernel<2, true, true>))
                 : p.vec == 1 ? CL_K(cl_step_kernel<1, true, false>) : CL_K(cl_step_kernel<2, true, false>);
        return p.vec == 1 ? CL_K(cl_step_kernel<1, false, false>) : p.vec == 2 ? CL_K(cl_step_kernel<2, false, false>) : CL_K(cl_step_kernel<4, false, false>);
    case CLK_LEAN_CHUNK:
        return p.prec == 2 ? (p.fold ? CL_LC_V(true, 2) : CL_LC_V(false, 2)) : (p.fold ? CL_LC_V(true, 0) : CL_LC_V(false, 0));
    case CLK_LEAN:
        if (p.prec == 1) return p.vec == 1 ? CL_NT(cl_step_lean_f64_kernel, 1) : CL_NT(cl_step_lean_f64_kernel, 2);
        if (p.prec == 2)
            return p.form == CLF_KPI ? CL_V124(cl_step_lean_kpi_chain_kernel) : p.form == CLF_OBS ? CL_V124(cl_step_lean_obs_chain_kernel) : CL_V124(cl_step_lean_chain_kernel);
        if (p.form == CLF_KPI) return CL_V124(cl_step_lean_kpi_kernel);
        if (p.form == CLF_OBS) return CL_V124(cl_step_lean_obs_kernel);
        return p.vec == 1 ? CL_NT(cl_step_lean_kernel, 1, true) : p.vec == 2 ? CL_NT(cl_step_lean_kernel, 2, true) : CL_NT(cl_step_lean_kernel, 4, true);
    case CLK_ENVMAJOR:
        if (p.prec == 2) return p.nb == 17 ? CL_EM(17, 1, 2) : CL_EM(20, 1, 2);
        return p.nb == 17 ? (p.vec == 2 ? CL_EM(17, 2, 0) : CL_EM(17, 1, 0)) : (p.vec == 2 ? CL_EM(20, 2, 0) : CL_EM(20, 1, 0));
    case CLK_FULL:
        if (p.form == CLF_KPI) return p.nt ? CL_K(cl_step_full_kpi_kernel<true>) : CL_K(cl_step_full_kpi_kernel<false>);
        if (p.form == CLF_OBS) return p.prec == 2 ? CL_NT(cl_step_full_obs_kernel, 2) : CL_NT(cl_step_full_obs_kernel, 0);
        if (p.prec == 2)
            return p.det ? CL_NT(cl_step_full_chain_kernel, 1, true, 1024, 4, false) : p.lp ? CL_NT(cl_step_full_chain_kernel, 1, false, 1024, 4, true)
                 : CL_NT(cl_step_full_chain_kernel, 1, false, 1024, 4, false);
        if (p.det)
            return p.vec == 1 ? CL_NT(cl_step_full_kernel, 1, true, 1024, 4, false) : p.maxt == 576 ? CL_NT(cl_step_full_kernel, 2, true, 576, 3, false)
                 : CL_NT(cl_step_full_kernel, 2, true, 1024, 4, false);
        if (p.lp) return p.vec == 1 ? CL_NT(cl_step_full_kernel, 1, false, 1024, 5, true) : CL_NT(cl_step_full_kernel, 2, false, 1024, 4, true);
        if (p.vec == 1) return CL_NT(cl_step_full_kernel, 1, false, 1024, CL_FULL1_WPE, false);
        return p.maxt == 576 ? CL_NT(cl_step_full_kernel, 2, false, 576, 5, false) : CL_NT(cl_step_full_kernel, 2, false, 1024, 5, false);
    case CLK_FULL_TP:
        if (p.form == CLF_OBS)
            return p.prec == 2 ? CL_NT(cl_step_full_tp_obs_kernel, 1, 2) : p.vec == 2 ? CL_NT(cl_step_full_tp_obs_kernel, 2, 0) : CL_NT(cl_step_full_tp_obs_kernel, 1, 0);
        if (p.prec == 2) return CL_NT(cl_step_full_tp_chain_kernel, 1, 4);
        return p.vec == 2 ? CL_NT(cl_step_full_tp_kernel, 2, 4) : CL_NT(cl_step_full_tp_kernel, 1, 4);
    }
#undef CL_EM
#undef CL_LC_V
#undef CL_LC
#undef CL_V124
#undef CL_NT
#undef CL_K
    return nullptr;
}
}  // namespace

extern "C" {

int cl_abi_version(void) { return CL_ABI_VERSION; }

#ifdef CL_TRACE
// diagnostic build only (scripts/wave_timeline.py): where cl_step_full_kernel parks its per-wave phase stamps
int cl_trace_set(void* buf) { return hipMemcpyToSymbol(HIP_SYMBOL(g_cl_trace), &buf, sizeof(buf)) == hipSuccess ? 0 : -1; }
#endif

const char* cl_last_error(void) { return g_err; }

int cl_reset_f32(const cl_dims* dims, const uint32_t* params, float* state, float* kpi_bldg, float* kpi_env,
                 void* stream) {
    if (int rc = check_dims(dims)) return rc;
    if (int rc = check_ptr(params, "params")) return rc;
    if (int rc = check_ptr(state, "state", false)) return rc;
    if (int rc = check_ptr(kpi_bldg, "kpi_bldg", false)) return rc;
    if (int rc = check_ptr(kpi_env, "kpi_env", false)) return rc;
    const int ld = pitch_of(dims);
    if (ld != dims->n_env && (kpi_bldg || kpi_env)) return fail(CL_EINVAL, "env_pitch=%d: the streaming KPI planes are not pitched", ld);
    const long long n = (long long)ld * dims->n_bldg;
    const int block = 256;
    const unsigned grid = (unsigned)((n + block - 1) / block);
    hipLaunchKernelGGL(cl_reset_kernel, dim3(grid), dim3(block), 0, (hipStream_t)stream, params, state, kpi_bldg,
                       kpi_env, dims->n_env, dims->n_bldg, dims->flags, ld);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_fail(e, "cl_reset_kernel launch");
    return CL_OK;
}

int cl_step_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const float* actions,
                int64_t act_stride_col, int64_t act_stride_env, float* out_bldg, float* out_env, float* kpi_bldg,
                float* kpi_env, int32_t t, void* stream) {
    return cl_step_flex_f32(dims, params, ts, state, actions, act_stride_col, act_stride_env, out_bldg, out_env, kpi_bldg,
                            kpi_env, nullptr, t, stream);
}

static int check_flex(const cl_dims* dims, const cl_flex* f) {
    if (f->n_ev < 0 || f->n_flex_bldg <= 0)
        return fail(CL_EINVAL, "cl_flex: bad counts (ev %d, buildings %d)", f->n_ev, f->n_flex_bldg);
    const int rows = dims->n_ts_rows ? dims->n_ts_rows : dims->n_steps;
    if (f->n_rows < rows) return fail(CL_ERANGE, "cl_flex.n_rows=%d but the step tables have %d rows", f->n_rows, rows);
    if (int rc = check_ptr(f->flex_out, "flex.flex_out")) return rc;
    if (int rc = check_ptr(f->ev_params, "flex.ev_params", f->n_ev > 0)) return rc;
    if (int rc = check_ptr(f->ev_ts, "flex.ev_ts", f->n_ev > 0)) return rc;
    if (int rc = check_ptr(f->ev_state, "flex.ev_state", f->n_ev > 0)) return rc;
    if (int rc = check_ptr(f->charger_params, "flex.charger_params")) return rc;
    if (int rc = check_ptr(f->charger_ts, "flex.charger_ts")) return rc;
    if (int rc = check_ptr(f->wm_params, "flex.wm_params")) return rc;
    if (int rc = check_ptr(f->wm_ts, "flex.wm_ts")) return rc;
    if (int rc = check_ptr(f->wm_state, "flex.wm_state")) return rc;
    return CL_OK;
}

int cl_flex_reset_f32(const cl_dims* dims, const cl_flex* flex, void* stream) {
    if (int rc = check_dims(dims)) return rc;
    if (!flex) return fail(CL_ENULL, "flex is NULL");
    if (int rc = no_pitch(dims, "cl_flex_reset_f32")) return rc;
    if (int rc = check_flex(dims, flex)) return rc;
    const int wm_slots = flex->n_flex_bldg * CL_MAXW;
    const long long n = (long long)dims->n_env * (flex->n_ev > wm_slots ? flex->n_ev : wm_slots);
    if (n > 0) {
        hipLaunchKernelGGL(cl_flex_reset_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *flex,
                           dims->env_row0, dims->n_env);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_fail(e, "cl_flex_reset_kernel launch");
    }
    return CL_OK;
}

// `of` / `fused`: the compact observation to write from inside the step launch (cl_step_observe_f32); *fused tells the caller
// whether the launch that ran could take it (lean district, four envs per lane, one workgroup row) or the observation is still to do.

static int step_impl(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const float* actions,
                     int64_t act_stride_col, int64_t act_stride_env, float* out_bldg, float* out_env, float* kpi_bldg,
                     float* kpi_env, const cl_flex* flex, int32_t t, void* stream, const ObsFusedArgs* of, bool* fused) {
    if (int rc = check_dims(dims)) return rc;
    const cl_tuning& tun = tuning_of(dims);
    name_reset(tun);
    if (int rc = check_ptr(params, "params")) return rc;
    if (int rc = check_ptr(ts, "ts")) return rc;
    if (int rc = check_ptr(state, "state")) return rc;
    if (int rc = check_ptr(actions, "actions", dims->n_act_cols > 0)) return rc;
    if (int rc = check_ptr(out_bldg, "out_bldg")) return rc;
    if (int rc = check_ptr(out_env, "out_env")) return rc;
    if (dims->flags & CLD_KPI) {
        // the per-building accumulators read the detail planes -- except for districts of up to 32 buildings without flexible loads, whose
        // step kernel updates them itself (cl_step_lean_kpi_kernel / cl_step_full_kpi_kernel; plan_step refuses the rest)
        if (!(dims->flags & CLD_WRITE_DETAIL) && (dims->n_bldg > 32 || flex))
            return fail(CL_EINVAL, "CLD_KPI requires CLD_WRITE_DETAIL (except for districts of up to 32 buildings without flexible loads)");
        if (int rc = check_ptr(kpi_bldg, "kpi_bldg")) return rc;
        if (int rc = check_ptr(kpi_env, "kpi_env")) return rc;
    }
    if (t < 0 || t >= dims->n_steps) return fail(CL_ERANGE, "t=%d outside [0, %d)", t, dims->n_steps);
    if (act_stride_env == 1 && (act_stride_col % 4) != 0)
        return fail(CL_EALIGN, "act_stride_col=%lld must be a multiple of 4 floats for the coalesced layout",
                    (long long)act_stride_col);
    const int ld = pitch_of(dims);
    // a pitch is implemented where 2^20-env batches exist: battery + PV districts stepped by the lean / env-major / general lean kernels
    if (ld != dims->n_env && (!(dims->flags & CLD_LEAN) || (dims->flags & (CLD_WRITE_DETAIL | CLD_KPI | CLD_F64_MAPS)) || flex || dims->n_bldg > 32))
        return fail(CL_EINVAL, "env_pitch=%d != n_env=%d is implemented for CLD_LEAN districts of up to 32 buildings without detail planes, streaming KPIs, "
                               "flexible loads or CLD_F64_MAPS", ld, dims->n_env);
    const int rkind_host = (dims->flags & CLD_REWARD_MASK) >> CLD_REWARD_SHIFT;
    if (rkind_host == CLR_EV && !flex) return fail(CL_EINVAL, "reward kind CLR_EV needs the flexible-load tables (cl_step_flex_f32)");
    if (flex)
        if (int rc = check_flex(dims, flex)) return rc;
    StepPlan p;
    if (int rc = plan_step(p, *dims, tun, act_stride_env, flex, of, of && of->lean_ok, of ? of->pitch : 0)) return rc;
    plan_name(p, tun);

    StepArgs a;
    a.params = params; a.ts = ts; a.state = state; a.actions = actions; a.out_bldg = out_bldg; a.out_env = out_env;
    a.kpi_bldg = kpi_bldg; a.kpi_env = kpi_env;
    a.act_stride_col = act_stride_col; a.act_stride_env = act_stride_env;
    a.n_env = dims->n_env; a.n_bldg = dims->n_bldg; a.n_steps = dims->n_steps;
    a.flags = (dims->flags & ~CLA_LEAN_STRIPS) | (p.strips ? CLA_LEAN_STRIPS : 0u); a.t = t; a.env_row0 = dims->env_row0; a.env_offset = (unsigned)dims->env_offset;
    a.ld = ld;
    a.flex_out = nullptr; a.n_flex_bldg = 0; a.ev_penalty_coef = 0.0f;
    a.nw = p.nw; a.b_chunk = p.b_chunk; a.n_chunks = p.n_chunks; a.nt = p.nt; a.fused_finish = p.fused_finish;
    hipStream_t s = (hipStream_t)stream;
    if (flex) {
        FlexArgs fa;
        fa.f = *flex; fa.actions = actions; fa.act_stride_col = act_stride_col; fa.act_stride_env = act_stride_env;
        fa.env_row0 = dims->env_row0; fa.n_env = dims->n_env; fa.n_steps = dims->n_steps; fa.t = t; fa.env_offset = (unsigned)dims->env_offset;
        fa.want_reward = rkind_host == CLR_EV;
        fa.want_chargers = (dims->flags & CLD_WRITE_DETAIL) != 0;
        const dim3 fgrid(p.flex_grid_x, (unsigned)((flex->n_flex_bldg + flex->n_ev + 3) / 4));
#define CL_FLEX_LAUNCH(V) do { \
            if (p.flex_nt) hipLaunchKernelGGL((cl_flex_kernel<V, true>), fgrid, dim3(256), 0, s, fa); \
            else hipLaunchKernelGGL((cl_flex_kernel<V, false>), fgrid, dim3(256), 0, s, fa); } while (0)
        if (p.flex_vec == 4) CL_FLEX_LAUNCH(4); else if (p.flex_vec == 2) CL_FLEX_LAUNCH(2); else CL_FLEX_LAUNCH(1);
#undef CL_FLEX_LAUNCH
        a.flex_out = flex->flex_out; a.n_flex_bldg = flex->n_flex_bldg;
        a.ev_penalty_coef = flex->cons_params ? flex->weights[CLEW_PENALTY_COEFFICIENT] : 0.0f;
    }
    if (p.kernel == CLK_LEAN && p.form == CLF_PLAIN && p.prec == 0 && !p.flex) {
        if (const int rc = cl_tu_launch_lean(p.vec, p.nt, p.grid_x, p.grid_y, p.block, p.lds, stream, &a))
            return hip_fail((hipError_t)rc, "cl_step_lean_kernel launch");
    } else {
        const void* fn = step_kernel_fn(p);
        if (p.lds > (size_t)CL_LDS_PER_CU)
            return fail(CL_EINVAL, "the step launch would need %zu bytes of LDS per workgroup (nw=%d, %d envs per lane): a CU has %d", p.lds, p.nw, p.vec, CL_LDS_PER_CU);
        if (p.lds > 64 * 1024)
            if (hipError_t e = ensure_dynamic_lds(fn, p.lds); e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(step kernel)");
        // kernel arguments: (a), (a, of), (a, tp) or (a, tp, of)
        int tp = p.tp_tiles;
        ObsFusedArgs* obs = const_cast<ObsFusedArgs*>(of);
        void* args[3] = {&a, p.kernel == CLK_FULL_TP ? (void*)&tp : (void*)obs, obs};
        (void)hipLaunchKernel(fn, dim3(p.grid_x, p.grid_y), dim3(p.block), args, p.lds, s);
        if (p.form == CLF_OBS) *fused = true;
    }
    if (p.finish) hipLaunchKernelGGL(cl_finish_kernel, dim3((dims->n_env + 63) / 64, NQ), dim3(1024), 0, s, a, 0, (float*)nullptr);
    const long long n = (long long)dims->n_env * dims->n_bldg;
    if (p.marl) hipLaunchKernelGGL(cl_marl_reward_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    if (p.kpi_passes == 2) {            // the round-1 / round-2 form: two passes (tests, A/B)
        hipLaunchKernelGGL(cl_kpi_bldg_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
        hipLaunchKernelGGL(cl_kpi_env_kernel, dim3((dims->n_env + 63) / 64), dim3(1024), 0, s, a);
    } else if (p.kpi_passes == 1) {
        hipLaunchKernelGGL(cl_kpi_kernel, dim3((dims->n_env + 63) / 64), dim3(1024), 0, s, a);
    }
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_fail(e, "cl_step_kernel launch");
    return CL_OK;
}

int cl_finish_f32(const cl_dims* dims, float* out_bldg, float* out_env, int32_t t, void* stream) {
    if (int rc = check_dims(dims)) return rc;
    if (int rc = check_ptr(out_bldg, "out_bldg")) return rc;
    if (int rc = check_ptr(out_env, "out_env")) return rc;
    if (t < 0 || t >= dims->n_steps) return fail(CL_ERANGE, "t=%d outside [0, %d)", t, dims->n_steps);
    if (dims->n_bldg <= 32) return CL_OK;              // never building-chunked: every step launch finishes its own district sums
    if (int rc = no_pitch(dims, "cl_finish_f32")) return rc;
    StepArgs a = {};
    a.out_bldg = out_bldg; a.out_env = out_env; a.n_env = dims->n_env; a.n_bldg = dims->n_bldg; a.n_steps = dims->n_steps;
    a.flags = dims->flags; a.t = t; a.n_chunks = 0;    // (the kernel reads the chunk count next to the marker)
    hipLaunchKernelGGL(cl_finish_kernel, dim3((dims->n_env + 63) / 64, NQ), dim3(1024), 0, (hipStream_t)stream, a, 1, (float*)nullptr);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_fail(e, "cl_finish_kernel launch");
    return CL_OK;
}

int cl_step_flex_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const float* actions,
                     int64_t act_stride_col, int64_t act_stride_env, float* out_bldg, float* out_env, float* kpi_bldg,
                     float* kpi_env, const cl_flex* flex, int32_t t, void* stream) {
    return step_impl(dims, params, ts, state, actions, act_stride_col, act_stride_env, out_bldg, out_env, kpi_bldg, kpi_env, flex, t, stream,
                     nullptr, nullptr);
}

int cl_step_observe_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const float* actions,
                        int64_t act_stride_col, int64_t act_stride_env, float* out_bldg, float* out_env, float* kpi_bldg, float* kpi_env,
                        int32_t t, const float* obs_table, const int32_t* col_src, const float* col_scale, const cl_obs_dep* deps,
                        int32_t n_deps, float* obs, int32_t n_cols, int32_t obs_pitch, int32_t n_rows, int32_t obs_row, void* stream) {
    if (int rc = check_dims(dims)) return rc;
    if (int rc = check_ptr(obs_table, "obs_table")) return rc;
    if (int rc = check_ptr(obs, "obs")) return rc;
    if (!deps || n_deps != n_cols || n_cols <= 0 || n_cols > CLOB_MAX_DEPS)
        return fail(CL_EINVAL, "cl_step_observe_f32 takes the compact form: every one of the n_cols <= %d columns env-dependent and listed (n_cols=%d, n_deps=%d)",
                    CLOB_MAX_DEPS, n_cols, n_deps);
    if (obs_pitch < n_cols) return fail(CL_EINVAL, "obs_pitch=%d < n_cols=%d", obs_pitch, n_cols);
    if (obs_row < 0 || obs_row >= n_rows) return fail(CL_ERANGE, "obs_row=%d outside [0, %d)", obs_row, n_rows);
    // what the step launch itself can write: columns fed by the planes a lean wave holds in registers, rows padded to 16 bytes
    ObsFusedArgs of;
    bool can = obs_pitch == ((n_cols + 3) & ~3) && dims->n_bldg <= CL_OBS_FUSED_BLDG && tuning_of(dims).obs_variant == 0;
    bool lean_planes = true;                        // only what a battery + PV wave holds: battery state, net, reward
    int n = 0;
    for (int b = 0; b < dims->n_bldg && can; ++b) {
        of.start[b] = (short)n;
        for (int d = 0; d < n_deps; ++d) {
            const int src = deps[d].src, kind = src >> 28, pl = (src >> 20) & 0xFF;
            if (deps[d].col < 0 || deps[d].col >= n_cols || src < 0) return fail(CL_EINVAL, "deps[%d]: col=%d src=%d", d, deps[d].col, src);
            // (under CLD_F64_CHAIN the degraded-capacity plane carries the capacity LOSS: not an observation source -- round-5 advisor)
            if (kind == CLOB_KIND_STATE && pl == CLS_B_DEGCAP && (dims->flags & CLD_F64_CHAIN))
                return fail(CL_EINVAL, "deps[%d]: CLS_B_DEGCAP holds capacity - degraded_capacity under CLD_F64_CHAIN and cannot feed an observation column", d);
            if ((src & 0xFFFFF) != b) continue;
            const bool lean_pl = (kind == CLOB_KIND_STATE && (pl == CLS_B_SOC || pl == CLS_B_EFF || pl == CLS_B_DEGCAP)) ||
                                 (kind == CLOB_KIND_OUT && (pl == CLO_NET || pl == CLO_REWARD));
            lean_planes = lean_planes && lean_pl;
            can = can && (lean_pl || (kind == CLOB_KIND_STATE && (pl == CLS_CS_SOC || pl == CLS_HS_SOC || pl == CLS_DS_SOC)));      // + the tank planes of the thermal kernels
            of.deps[n++] = deps[d];
        }
    }
    can = can && n == n_deps;                       // (a building index beyond n_bldg would have been skipped)
    bool lean_ok = can && lean_planes;
    for (int b = 0; b < dims->n_bldg && lean_ok; ++b) lean_ok = (b + 1 < dims->n_bldg ? of.start[b + 1] : n) - of.start[b] <= CL_OBS_FUSED_PER_BLDG;
    of.lean_ok = lean_ok ? 1 : 0;
    for (int b = dims->n_bldg; b <= CL_OBS_FUSED_BLDG; ++b) of.start[b] = (short)n;
    of.obs = obs; of.table = obs_table; of.n_cols = n_cols; of.pitch = obs_pitch; of.row = obs_row;
    bool fused = false;
    if (int rc = step_impl(dims, params, ts, state, actions, act_stride_col, act_stride_env, out_bldg, out_env, kpi_bldg, kpi_env, nullptr, t,
                           stream, can ? &of : nullptr, &fused)) return rc;
    if (fused) return CL_OK;
    return cl_observe_f32(dims, obs_table, col_src, col_scale, deps, n_deps, state, out_bldg, nullptr, nullptr, 0, obs, n_cols, obs_pitch,
                          n_rows, obs_row, 0u, stream);
}

// cl_rollout_seq_f32 under CLD_ROLLOUT_FUSED: the K steps in ONE fused launch or CL_EINVAL -- never the launch sequence.  (`dims` checked by the caller.)
static int rollout_fused(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const float* actions,
                         int64_t act_stride_step, int64_t act_stride_col, int64_t act_stride_env, const float* act_low,
                         const float* act_high, uint64_t seed, float* out_bldg, float* out_env,
                         float* ret_env, float* kpi_bldg, float* kpi_env, const cl_flex* flex, int32_t t0, int32_t k_steps, void* stream) {
    if (flex) return fail(CL_EINVAL, "CLD_ROLLOUT_FUSED: flex != NULL -- the fused rollout kernels carry no flexible-load state (drop the flag for the launch sequence)");
    if (dims->flags & CLD_F64_MAPS)
        return fail(CL_EINVAL, "CLD_ROLLOUT_FUSED: the fused rollout kernels evaluate the battery map in fp32 or as the float64 chain (CLD_F64_CHAIN), not CLD_F64_MAPS");
    if (!(dims->flags & CLD_KPI))
        return cl_rollout_f32(dims, params, ts, state, actions, act_stride_step, act_stride_col, act_stride_env, act_low, act_high, seed, out_bldg,
                              out_env, ret_env, t0, k_steps, stream);
    if (!(dims->flags & CLD_LEAN))
        return fail(CL_EINVAL, "CLD_ROLLOUT_FUSED with CLD_KPI: only battery + PV districts (CLD_LEAN); a thermal / outage district keeps the launch sequence");
    if (dims->flags & CLD_WRITE_DETAIL) return fail(CL_EINVAL, "CLD_ROLLOUT_FUSED with CLD_KPI: not with the detail planes (CLD_WRITE_DETAIL)");
    if (dims->n_bldg > CL_RKPI_NB)
        return fail(CL_EINVAL, "CLD_ROLLOUT_FUSED with CLD_KPI: n_bldg=%d > %d would be a building-chunked launch, which the fused KPI kernel is not", dims->n_bldg, CL_RKPI_NB);
    if (pitch_of(dims) != dims->n_env)
        return fail(CL_EINVAL, "CLD_ROLLOUT_FUSED with CLD_KPI: env_pitch=%d != n_env=%d -- the streaming KPI planes are not pitched", dims->env_pitch, dims->n_env);
    if (((dims->flags & CLD_REWARD_MASK) >> CLD_REWARD_SHIFT) == CLR_EV)
        return fail(CL_EINVAL, "CLD_ROLLOUT_FUSED: reward kind CLR_EV needs the flexible-load tables");
    const cl_tuning& tun = tuning_of(dims);
    if (int rc = check_ptr(params, "params")) return rc;
    if (int rc = check_ptr(ts, "ts")) return rc;
    if (int rc = check_ptr(state, "state")) return rc;
    if (int rc = check_ptr(out_bldg, "out_bldg")) return rc;
    if (int rc = check_ptr(out_env, "out_env")) return rc;
    if (int rc = check_ptr(kpi_bldg, "kpi_bldg")) return rc;
    if (int rc = check_ptr(kpi_env, "kpi_env")) return rc;
    if (!actions && dims->n_act_cols > 0 && (!act_low || !act_high)) return fail(CL_ENULL, "act_low / act_high are required for the on-device policy");
    if (actions && act_stride_env == 1 && ((act_stride_col % 4) != 0 || (act_stride_step % 4) != 0))
        return fail(CL_EALIGN, "action strides must be multiples of 4 floats for the coalesced layout");

    RolloutArgs r;
    StepArgs& a = r.s;
    a.params = params; a.ts = ts; a.state = state; a.actions = actions; a.out_bldg = out_bldg; a.out_env = out_env;
    a.kpi_bldg = kpi_bldg; a.kpi_env = kpi_env;
    a.act_stride_col = act_stride_col; a.act_stride_env = act_stride_env;
    a.flex_out = nullptr; a.n_flex_bldg = 0; a.ev_penalty_coef = 0.0f;
    a.n_env = dims->n_env; a.n_bldg = dims->n_bldg; a.n_steps = dims->n_steps; a.ld = dims->n_env;
    a.flags = dims->flags; a.t = t0; a.b_chunk = dims->n_bldg; a.n_chunks = 1; a.env_row0 = dims->env_row0; a.env_offset = (unsigned)dims->env_offset;
    a.nt = 0; a.fused_finish = 0;
    r.act_stride_step = act_stride_step; r.act_low = act_low; r.act_high = act_high; r.ret_env = ret_env; r.seed = seed;
    r.t0 = t0; r.k_steps = k_steps;
    // two buildings per wave; envs per lane as cl_rollout_f32 picks them (128-env workgroups in nearly full rounds of one per CU)
    a.nw = tun.nw ? tun.nw : (dims->n_bldg + 1) / 2;
    // (nw > n_bldg: a wave without any building would read its parameter row -- row `w` -- past the end of the table)
    if (a.nw * 2 < dims->n_bldg || a.nw < 1 || a.nw > 16 || a.nw > dims->n_bldg) return fail(CL_EINVAL, "bad nw %d", a.nw);
    const int vec = tun.vec ? tun.vec : (((actions == nullptr || act_stride_env == 1) && full_rounds(dims->n_env, 1)) ? 2 : 1);
    if (vec != 1 && vec != 2) return fail(CL_EINVAL, "no fused KPI rollout kernel at %d envs per lane", vec);
    const int tile = 64 * vec;
    const size_t lds = rollout_kpi_lds_floats(a.nw, tile) * sizeof(float);
    if (lds > CL_LDS_PER_CU) return fail(CL_EINVAL, "the fused KPI rollout would need %zu bytes of LDS per workgroup (nw=%d, %d envs per lane): a CU has %d", lds, a.nw, vec, CL_LDS_PER_CU);
    const bool chain = dims->flags & CLD_F64_CHAIN;
    name_reset(tun);
    name_add(tun, "cl_rollout_kpi_kernel<%d, %d>", vec, chain ? 2 : 0);
    const int rc = cl_tu_launch_rollout(4000 + (chain ? 2000 : 0) + vec * 10 + 2, 1, (unsigned)((dims->n_env + tile - 1) / tile), 1u, 64u * a.nw, lds, stream, &r);
    if (rc) return hip_fail((hipError_t)rc, "cl_rollout_kpi_kernel launch");
    return CL_OK;
}

int cl_rollout_seq_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const float* actions,
                       int64_t act_stride_step, int64_t act_stride_col, int64_t act_stride_env, const float* act_low,
                       const float* act_high, uint64_t seed, float* policy_actions, float* out_bldg, float* out_env,
                       float* ret_env, float* kpi_bldg, float* kpi_env, const cl_flex* flex, int32_t t0, int32_t k_steps, void* stream) {
    if (int rc = check_dims(dims)) return rc;
    if (dims->flags & CLD_ROLLOUT_FUSED) {
        if (int rc = check_ptr(actions, "actions", false)) return rc;
        if (int rc = check_ptr(ret_env, "ret_env", false)) return rc;
        if (k_steps < 0 || t0 < 0 || t0 + k_steps > dims->n_steps)
            return fail(CL_ERANGE, "steps [%d, %d) outside [0, %d)", t0, t0 + k_steps, dims->n_steps);
        return rollout_fused(dims, params, ts, state, actions, act_stride_step, act_stride_col, act_stride_env, act_low, act_high, seed, out_bldg,
                             out_env, ret_env, kpi_bldg, kpi_env, flex, t0, k_steps, stream);
    }
    if (int rc = check_ptr(actions, "actions", false)) return rc;
    if (int rc = check_ptr(ret_env, "ret_env", false)) return rc;
    if (!actions && dims->n_act_cols > 0) {
        if (!act_low || !act_high) return fail(CL_ENULL, "act_low / act_high are required for the on-device policy");
        if (int rc = check_ptr(policy_actions, "policy_actions")) return rc;
        if (dims->n_env % 4) return fail(CL_EALIGN, "the on-device policy needs n_env to be a multiple of 4 (got %d)", dims->n_env);
    }
    if (k_steps < 0 || t0 < 0 || t0 + k_steps > dims->n_steps)
        return fail(CL_ERANGE, "steps [%d, %d) outside [0, %d)", t0, t0 + k_steps, dims->n_steps);
    hipStream_t s = (hipStream_t)stream;
    const unsigned gx = (unsigned)((dims->n_env + 255) / 256);
    for (int k = 0; k < k_steps; ++k) {
        const int t = t0 + k;
        const float* a = actions ? actions + (long long)k * act_stride_step
                                 : policy_actions + (long long)(t & 3) * dims->n_act_cols * dims->n_env;
        if (!actions && dims->n_act_cols > 0 && (k == 0 || (t & 3) == 0))
            hipLaunchKernelGGL(cl_policy_kernel, dim3(gx, (unsigned)dims->n_act_cols), dim3(256), 0, s, policy_actions, act_low, act_high,
                               (unsigned long long)seed, dims->n_env, dims->n_act_cols, t >> 2, (unsigned)dims->env_offset);
        if (int rc = cl_step_flex_f32(dims, params, ts, state, a, actions ? act_stride_col : (int64_t)dims->n_env,
                                      actions ? act_stride_env : (int64_t)1, out_bldg, out_env, kpi_bldg, kpi_env, flex, t, stream))
            return rc;
        if (ret_env) {
            // (a deferred finish -- cl_tuning.finish = 3 -- would leave the previous step's reward here: fold now; a no-op where the step did not defer)
            if (tuning_of(dims).finish == 3)
                if (int rc = cl_finish_f32(dims, out_bldg, out_env, t, stream)) return rc;
            hipLaunchKernelGGL(cl_return_kernel, dim3(gx), dim3(256), 0, s, ret_env, out_env + (long long)CLQ_REWARD * dims->n_env, dims->n_env);
        }
    }
    // end of the sequence: out_env holds the last step's district sums whatever the finish mode
    if (!ret_env && k_steps > 0 && tuning_of(dims).finish == 3)
        if (int rc = cl_finish_f32(dims, out_bldg, out_env, t0 + k_steps - 1, stream)) return rc;
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_fail(e, "cl_rollout_seq_f32 launch");
    return CL_OK;
}

int cl_rollout_f32(const cl_dims* dims, const uint32_t* params, const float* ts, float* state, const float* actions,
                   int64_t act_stride_step, int64_t act_stride_col, int64_t act_stride_env, const float* act_low,
                   const float* act_high, uint64_t seed, float* out_bldg, float* out_env, float* ret_env,
                   int32_t t0, int32_t k_steps, void* stream) {
    if (int rc = check_dims(dims)) return rc;
    const cl_tuning& tun = tuning_of(dims);
    if (int rc = check_ptr(params, "params")) return rc;
    if (int rc = check_ptr(ts, "ts")) return rc;
    if (int rc = check_ptr(state, "state")) return rc;
    if (int rc = check_ptr(out_bldg, "out_bldg")) return rc;
    if (int rc = check_ptr(out_env, "out_env")) return rc;
    if (int rc = check_ptr(actions, "actions", false)) return rc;
    if (int rc = check_ptr(ret_env, "ret_env", false)) return rc;
    if (!actions && dims->n_act_cols > 0) {
        if (!act_low || !act_high) return fail(CL_ENULL, "act_low / act_high are required for the on-device policy");
    }
    if (((dims->flags & CLD_REWARD_MASK) >> CLD_REWARD_SHIFT) == CLR_EV)
        return fail(CL_EINVAL, "reward kind CLR_EV needs the flexible-load tables (cl_rollout_seq_f32)");
    if (dims->flags & CLD_KPI)
        return fail(CL_EINVAL, "cl_rollout_f32 takes no KPI planes: call cl_rollout_seq_f32 with CLD_KPI (launch sequence), or with CLD_KPI | CLD_ROLLOUT_FUSED (one fused launch, battery + PV districts)");
    if (dims->flags & CLD_F64_MAPS) return fail(CL_EINVAL, "the fused rollout evaluates the battery map in fp32 or as the float64 chain (CLD_F64_CHAIN): use cl_rollout_seq_f32 with CLD_F64_MAPS");
    if (k_steps < 0 || t0 < 0 || t0 + k_steps > dims->n_steps)
        return fail(CL_ERANGE, "steps [%d, %d) outside [0, %d)", t0, t0 + k_steps, dims->n_steps);
    if (actions && act_stride_env == 1 && ((act_stride_col % 4) != 0 || (act_stride_step % 4) != 0))
        return fail(CL_EALIGN, "action strides must be multiples of 4 floats for the coalesced layout");

    RolloutArgs r;
    StepArgs& a = r.s;
    a.params = params; a.ts = ts; a.state = state; a.actions = actions; a.out_bldg = out_bldg; a.out_env = out_env;
    a.kpi_bldg = nullptr; a.kpi_env = nullptr;
    a.act_stride_col = act_stride_col; a.act_stride_env = act_stride_env;
    a.n_env = dims->n_env; a.n_bldg = dims->n_bldg; a.n_steps = dims->n_steps;
    a.flags = dims->flags; a.t = t0; a.b_chunk = dims->n_bldg; a.n_chunks = 1; a.env_row0 = dims->env_row0; a.env_offset = (unsigned)dims->env_offset;
    a.nt = 0; a.fused_finish = 0;
    a.ld = pitch_of(dims);
    if (a.ld != a.n_env && (!(dims->flags & CLD_LEAN) || (dims->flags & CLD_WRITE_DETAIL) || dims->n_bldg > 32))
        return fail(CL_EINVAL, "env_pitch=%d != n_env=%d: the fused rollout implements a pitch for CLD_LEAN districts of up to 32 buildings", a.ld, a.n_env);
    r.act_stride_step = act_stride_step; r.act_low = act_low; r.act_high = act_high; r.ret_env = ret_env; r.seed = seed;
    r.t0 = t0; r.k_steps = k_steps;
    const bool full = !(dims->flags & CLD_LEAN) || (dims->flags & CLD_WRITE_DETAIL);
    // a wave keeps the state of MB buildings in registers: two battery + PV buildings, one thermal one.  Districts beyond 16 MB buildings are
    // cut into chunks of `b_chunk` <= 16 MB along gridDim.y (cl_rollout_kernel's note); cl_finish_kernel folds the chunk sums once per launch
    const int mb_max = full ? 1 : 2;
    const bool chunked = dims->n_bldg > 16 * mb_max;
    int mb = full ? 1 : (dims->n_bldg > 16 || (dims->flags & CLD_F64_CHAIN) ? 2 : 1);      // (the one-building chain instantiation reserves scratch memory)
    if (chunked) {
        if (((dims->flags & CLD_REWARD_MASK) >> CLD_REWARD_SHIFT) == CLR_MARL)
            return fail(CL_EINVAL, "the fused rollout of a building-chunked district (n_bldg=%d) cannot couple the buildings inside a step (MARL): use cl_rollout_seq_f32", dims->n_bldg);
        // (the packed thermal kernel: EIGHT buildings = waves per workgroup -- three / two workgroups per CU instead of one sixteen-wave one at its
        //  84 / 97 registers and 50 / 76 KB of LDS: 1024 buildings x 1024 / 2048 / 8192 envs 289 -> 263 / 557 -> 498 / 2173 -> 1873 us per 24 steps
        //  under the float64 chain, 195 -> 183 / 378 -> 336 / 1458 -> 1258 us on the fp32 map; profiles/r06m_*)
        const bool packed_shape = full && !(dims->flags & CLD_WRITE_DETAIL) && tun.full_variant != 1 && dims->n_act_cols <= 65536;
        a.b_chunk = tun.b_chunk > 0 ? tun.b_chunk : packed_shape ? 8 : 16 * mb_max;
        if (a.b_chunk > 16 * mb_max) return fail(CL_EINVAL, "b_chunk=%d: a fused-rollout workgroup holds at most %d buildings of this district", a.b_chunk, 16 * mb_max);
        mb = mb_max;                      // (battery + PV: always two buildings per wave -- the one-building chunked instantiations spill)
        a.n_chunks = (dims->n_bldg + a.b_chunk - 1) / a.b_chunk;
        if (int rc = check_chunk_partials(a.b_chunk, a.n_chunks, dims)) return rc;
    }
    a.nw = tun.nw ? tun.nw : ((chunked ? a.b_chunk : dims->n_bldg) + mb - 1) / mb;
    if (a.nw * mb < (chunked ? a.b_chunk : dims->n_bldg) || a.nw > 16) return fail(CL_EINVAL, "bad nw %d", a.nw);
    // two envs per lane where the 128-env workgroups come in (nearly) full rounds of one per CU (full_rounds)
    const bool chain = dims->flags & CLD_F64_CHAIN;          // (the float64 soc chain: two envs per lane only where one workgroup row holds the district)
    int vec = tun.vec ? tun.vec : ((!full && (actions == nullptr || act_stride_env == 1) && full_rounds(dims->n_env, a.n_chunks)) ? 2 : 1);
    if (chain && (full || vec > 2)) vec = 1;                 // (chunked battery + PV districts keep the two-env pack under the chain too: 1024 x 1024 / x 8192 127.6 -> 107.9 / 932.9 -> 798.9 us per 24 steps, profiles/r06z_*)
    const int tile = 64 * vec;
    const unsigned grid = (unsigned)((dims->n_env + tile - 1) / tile);
    const size_t lds = (size_t)a.nw * NQ * tile * sizeof(float);
    const dim3 block(64 * a.nw);
    name_reset(tun);
    // Thermal / outage districts without detail planes (round 6): the pack-generic unit of cl_full.h inside the K-step loop (cl_rollout_full_kernel),
    // two envs per lane where the battery map is fp32 and the actions are contiguous along the envs; cl_tuning.full_variant = 1 keeps the scalar unit
    const bool packed = full && mb == 1 && !(dims->flags & CLD_WRITE_DETAIL) && tun.full_variant != 1 && dims->n_act_cols <= 65536;      // (column ids travel 16 bits each)
    if (packed) {
        const bool marl = ((dims->flags & CLD_REWARD_MASK) >> CLD_REWARD_SHIFT) == CLR_MARL;      // (never chunked: refused above; one env per lane -- the two-env MARL instantiation parks 36 bytes in scratch)
        const int fvec = (chain || marl || (actions && act_stride_env != 1) || tun.vec == 1) ? 1 : 2;
        const dim3 pgrid((unsigned)((dims->n_env + 64 * fvec - 1) / (64 * fvec)), (unsigned)a.n_chunks);
        // LDS: the reduction rows, or MARL's exchange row + every wave's Philox blocks (cl_rollout_full_kernel's note) -- 100 / 152 KB at 16 waves
        const size_t tile_b = (size_t)64 * fvec * sizeof(float);
        const size_t rows = (size_t)a.nw * NQ * tile_b, rnd = (size_t)a.nw * tile_b + (size_t)a.nw * (fvec == 1 ? CL_ROLLOUT_RND_ROWS<1> : CL_ROLLOUT_RND_ROWS<2>) * tile_b;
        const size_t plds = rows > rnd ? rows : rnd;
        if (plds > CL_LDS_PER_CU) return fail(CL_EINVAL, "the packed fused rollout would need %zu bytes of LDS per workgroup (nw=%d): a CU has %d", plds, a.nw, CL_LDS_PER_CU);
        name_add(tun, "cl_rollout_full_kernel<%d, %s, %d, %s>", fvec, chunked ? "true" : "false", chain ? 2 : 0, marl ? "true" : "false");
#define CL_RFM(V, C, P, M) do { \
            if (plds > 64 * 1024) if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(cl_rollout_full_kernel<V, C, P, M>), plds); e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(cl_rollout_full_kernel)"); \
            hipLaunchKernelGGL((cl_rollout_full_kernel<V, C, P, M>), pgrid, block, plds, (hipStream_t)stream, r); } while (0)
#define CL_RF(V, C, P) do { if (marl && !C) CL_RFM(V, false, P, true); else CL_RFM(V, C, P, false); } while (0)
        if (chain) { if (chunked) CL_RF(1, true, 2); else CL_RF(1, false, 2); }
        else if (fvec == 2) { if (chunked) CL_RFM(2, true, 0, false); else CL_RFM(2, false, 0, false); }
        else { if (chunked) CL_RF(1, true, 0); else CL_RF(1, false, 0); }
#undef CL_RFM
#undef CL_RF
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_fail(e, "cl_rollout_full_kernel launch");
    } else {
    const int key = (full ? 100 : 0) + vec * 10 + mb;
    if ((key != 11 && key != 12 && key != 21 && key != 22 && key != 111) || ((chunked || chain) && key != 12 && key != 22 && key != 111) )
        return fail(CL_EINVAL, "no rollout kernel for vec %d / buildings-per-wave %d / %s", vec, mb, full ? "full" : "lean");
    const bool pin = chunked || chain || (long long)grid * a.nw > 5 * 1024;
    // (spelled as rocprofv3 prints them: every template argument, defaults included)
    name_add(tun, "cl_rollout_kernel<%d, %s, %d, %s, %s, %d>", vec, full ? "true" : "false", mb, (key == 12 && !pin) ? "false" : "true", chunked ? "true" : "false", chain ? 2 : 0);
    const int rc = cl_tu_launch_rollout(key + (chunked ? 1000 : 0) + (chain ? 2000 : 0), pin, grid, (unsigned)a.n_chunks, block.x, lds, stream, &r);
    if (rc) return hip_fail((hipError_t)rc, "cl_rollout_kernel launch");
    }
    // the last step's district sums (and the K-step return): one fold per launch
    if (chunked && k_steps > 0) return launch_rollout_finish(tun, a, t0 + k_steps - 1, ret_env, (hipStream_t)stream);
    return CL_OK;
}

int cl_lstm_reset_f32(const cl_dims* dims, float* hist, float* hidden, float* kpi_comfort, void* stream) {
    if (int rc = check_dims(dims)) return rc;
    if (int rc = no_pitch(dims, "cl_lstm_reset_f32")) return rc;
    if (int rc = check_ptr(hist, "hist")) return rc;
    if (int rc = check_ptr(hidden, "hidden")) return rc;
    const size_t plane = (size_t)dims->n_env * dims->n_bldg * sizeof(float);
    if (hipError_t e = hipMemsetAsync(hist, 0, CL_LSTM_NHIST * plane, (hipStream_t)stream); e != hipSuccess) return hip_fail(e, "memset hist");
    if (hipError_t e = hipMemsetAsync(hidden, 0, CL_LSTM_NHIDDEN * plane, (hipStream_t)stream); e != hipSuccess) return hip_fail(e, "memset hidden");
    if (kpi_comfort) {
        if (int rc = check_ptr(kpi_comfort, "kpi_comfort")) return rc;
        const long long units = (long long)dims->n_env * dims->n_bldg;
        hipLaunchKernelGGL(cl_kpi_comfort_reset_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, (hipStream_t)stream, kpi_comfort, units);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_fail(e, "cl_kpi_comfort_reset_kernel launch");
    }
    return CL_OK;
}

int cl_lstm_step_f32(const cl_dims* dims, const float* lstm_w, const uint16_t* lstm_wb, const float* dyn_pre, const float* cool_dem,
                     const float* heat_dem, float* hist, float* hidden, float* indoor_temp, float* comfort,
                     float* kpi_comfort, int32_t t, void* stream) {
    if (int rc = check_dims(dims)) return rc;
    if (int rc = no_pitch(dims, "cl_lstm_step_f32")) return rc;
    const cl_tuning& tun = tuning_of(dims);
    if (int rc = check_ptr(lstm_w, "lstm_w")) return rc;
    if (int rc = check_ptr(dyn_pre, "dyn_pre")) return rc;
    if (int rc = check_ptr(cool_dem, "cool_dem")) return rc;
    if (int rc = check_ptr(hist, "hist")) return rc;
    if (int rc = check_ptr(hidden, "hidden")) return rc;
    if (int rc = check_ptr(indoor_temp, "indoor_temp")) return rc;
    if (t < 0 || t >= dims->n_steps) return fail(CL_ERANGE, "t=%d outside [0, %d)", t, dims->n_steps);
    LstmArgs a;
    a.lstm_w = lstm_w; a.dyn_pre = dyn_pre; a.cool_dem = cool_dem; a.hist = hist; a.hidden = hidden; a.indoor_temp = indoor_temp;
    a.heat_dem = heat_dem; a.comfort = comfort; a.kpi_comfort = kpi_comfort;
    if (int rc = check_ptr(kpi_comfort, "kpi_comfort", false)) return rc;
    a.n_env = dims->n_env; a.n_bldg = dims->n_bldg; a.t = t; a.env_row0 = dims->env_row0;
    const dim3 grid((dims->n_env + 127) / 128, dims->n_bldg);          // 4 waves x 32 envs per workgroup
    a.lstm_wb = lstm_wb;
    if (int rc = check_ptr(lstm_wb, "lstm_wb", false)) return rc;
    const bool f16 = dims->flags & CLD_LSTM_F16;
    const bool two = dims->flags & CLD_LSTM_TWO_DEMANDS;
    if (two && !heat_dem) return fail(CL_EINVAL, "CLD_LSTM_TWO_DEMANDS needs heat_dem");
    name_reset(tun);
#define CL_LSTM_LAUNCH(DBG, SPLIT) do { if (two) { name_add(tun, "cl_lstm_kernel<" #DBG ", " #SPLIT ", true>"); \
    hipLaunchKernelGGL((cl_lstm_kernel<DBG, SPLIT, true>), grid, dim3(256), 0, (hipStream_t)stream, a); } else { name_add(tun, "cl_lstm_kernel<" #DBG ", " #SPLIT ", false>"); \
    hipLaunchKernelGGL((cl_lstm_kernel<DBG, SPLIT, false>), grid, dim3(256), 0, (hipStream_t)stream, a); } } while (0)
#define CL_LSTM_LAUNCH_WB(DBG) do { if (f16) CL_LSTM_LAUNCH(DBG, 2); else CL_LSTM_LAUNCH(DBG, 1); } while (0)
    switch (tun.lstm_variant) {            // timing experiments (scripts/lstm_check.py); 0 in production
    case 1: CL_LSTM_LAUNCH(1, 0); break;
    case 2: CL_LSTM_LAUNCH(2, 0); break;
    case 3: CL_LSTM_LAUNCH(0, 0); break;                                   // f32 MFMA path
    case 5: if (!lstm_wb) return fail(CL_EINVAL, "lstm_variant 5 needs lstm_wb"); CL_LSTM_LAUNCH_WB(1); break;
    case 6: if (!lstm_wb) return fail(CL_EINVAL, "lstm_variant 6 needs lstm_wb"); CL_LSTM_LAUNCH_WB(2); break;
    case 32: if (!lstm_wb) return fail(CL_EINVAL, "lstm_variant 32 needs lstm_wb"); CL_LSTM_LAUNCH_WB(32); break;   // common-denominator cell update (experiment)
    case 8: if (!lstm_wb || f16) return fail(CL_EINVAL, "lstm_variant 8 needs bf16 lstm_wb"); CL_LSTM_LAUNCH(8, 1); break;   // two-term bf16 split
    default:
        if (lstm_wb) CL_LSTM_LAUNCH_WB(0);
        else CL_LSTM_LAUNCH(0, 0);
    }
#undef CL_LSTM_LAUNCH_WB
#undef CL_LSTM_LAUNCH
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_fail(e, "cl_lstm_kernel launch");
    return CL_OK;
}

int cl_lstm_generic_step_f32(const cl_dims* dims, const float* lstm_w, const float* dyn_pre, const float* gen_w, int64_t gen_w_stride,
                             const float* gen_pre, float* gen_hidden, int32_t gen_h, int32_t gen_layers, const float* cool_dem, const float* heat_dem,
                             float* hist, float* indoor_temp, float* comfort, float* kpi_comfort, int32_t t, void* stream) {
    if (int rc = check_dims(dims)) return rc;
    if (int rc = no_pitch(dims, "cl_lstm_generic_step_f32")) return rc;
    if (int rc = check_ptr(lstm_w, "lstm_w")) return rc;
    if (int rc = check_ptr(dyn_pre, "dyn_pre")) return rc;
    if (int rc = check_ptr(gen_w, "gen_w")) return rc;
    if (int rc = check_ptr(gen_pre, "gen_pre")) return rc;
    if (int rc = check_ptr(gen_hidden, "gen_hidden")) return rc;
    if (int rc = check_ptr(cool_dem, "cool_dem")) return rc;
    if (int rc = check_ptr(hist, "hist")) return rc;
    if (int rc = check_ptr(indoor_temp, "indoor_temp")) return rc;
    if (int rc = check_ptr(kpi_comfort, "kpi_comfort", false)) return rc;
    if (t < 0 || t >= dims->n_steps) return fail(CL_ERANGE, "t=%d outside [0, %d)", t, dims->n_steps);
    if (gen_h < 1 || gen_h > CL_LSTM_GEN_HMAX) return fail(CL_EINVAL, "gen_h=%d outside [1, %d]", gen_h, CL_LSTM_GEN_HMAX);
    if (gen_layers != 1 && gen_layers != 2) return fail(CL_EINVAL, "gen_layers=%d (1 or 2: the deepest model among the generic-kernel buildings)", gen_layers);
    const long long need = (long long)gen_h * 12 + 3ll * gen_h * gen_h * 4 + gen_h * 4 + gen_h;
    if (gen_w_stride < need) return fail(CL_EINVAL, "gen_w_stride=%lld < %lld floats for hidden size %d", (long long)gen_w_stride, need, gen_h);
    LstmGenArgs g;
    LstmArgs& a = g.s;
    a.lstm_w = lstm_w; a.lstm_wb = nullptr; a.dyn_pre = dyn_pre; a.cool_dem = cool_dem; a.hist = hist; a.hidden = nullptr;
    a.indoor_temp = indoor_temp; a.heat_dem = heat_dem; a.comfort = comfort; a.kpi_comfort = kpi_comfort;
    a.n_env = dims->n_env; a.n_bldg = dims->n_bldg; a.t = t; a.env_row0 = dims->env_row0;
    g.gen_w = gen_w; g.gen_pre = gen_pre; g.gen_hidden = gen_hidden; g.H = gen_h; g.gw = gen_w_stride;
    // LDS: hidden states [layers][2][H][64] and, when they fit beside them, the recurrent matrices (WHH0 (, WIH1, WHH1): [H][H][4] each),
    // sized for the deepest model of the district (`gen_layers`)
    const size_t lds_h = (size_t)gen_layers * 2 * gen_h * 64 * sizeof(float), lds_w = (size_t)(gen_layers == 2 ? 3 : 1) * gen_h * gen_h * 4 * sizeof(float);
    const bool staged = lds_h + lds_w <= 150 * 1024;
    const size_t lds = lds_h + (staged ? lds_w : 0);
    const void* fn = staged ? reinterpret_cast<const void*>(cl_lstm_generic_kernel<true>) : reinterpret_cast<const void*>(cl_lstm_generic_kernel<false>);
    if (lds > 64 * 1024) {
        if (hipError_t e = ensure_dynamic_lds(fn, lds); e != hipSuccess)
            return hip_fail(e, "hipFuncSetAttribute(cl_lstm_generic_kernel)");
    }
    const dim3 ggrid((dims->n_env + 63) / 64, dims->n_bldg), gblock(64 * CL_GEN_NWV);
    name_add(tuning_of(dims), staged ? "cl_lstm_generic_kernel<true>" : "cl_lstm_generic_kernel<false>");   // (after cl_lstm_step_f32's entry: no reset)
    if (staged) hipLaunchKernelGGL(cl_lstm_generic_kernel<true>, ggrid, gblock, lds, (hipStream_t)stream, g);
    else hipLaunchKernelGGL(cl_lstm_generic_kernel<false>, ggrid, gblock, lds, (hipStream_t)stream, g);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_fail(e, "cl_lstm_generic_kernel launch");
    return CL_OK;
}

int cl_observe_f32(const cl_dims* dims, const float* obs_table, const int32_t* col_src, const float* col_scale,
                   const cl_obs_dep* deps, int32_t n_deps, const float* state, const float* out_bldg, const float* indoor_temp,
                   const float* extra, int32_t n_extra_rows, float* obs, int32_t n_cols,
                   int32_t obs_pitch, int32_t n_rows, int32_t row, uint32_t flags, void* stream) {
    if (int rc = check_dims(dims)) return rc;
    const cl_tuning& tun = tuning_of(dims);
    if (int rc = check_ptr(obs_table, "obs_table")) return rc;
    if (int rc = check_ptr(obs, "obs")) return rc;
    if (n_cols <= 0 || n_rows <= 0) return fail(CL_EINVAL, "bad observation table shape [%d][%d]", n_rows, n_cols);
    if (obs_pitch < n_cols) return fail(CL_EINVAL, "obs_pitch=%d < n_cols=%d", obs_pitch, n_cols);
    if (row < 0 || row >= n_rows) return fail(CL_ERANGE, "row=%d outside [0, %d)", row, n_rows);
    const bool all_exo = (flags & CLOB_ALL_EXOGENOUS) != 0;
    if (!all_exo) {
        if (int rc = check_ptr(col_src, "col_src")) return rc;
        if (int rc = check_ptr(col_scale, "col_scale")) return rc;
        if (int rc = check_ptr(state, "state")) return rc;
        if (int rc = check_ptr(out_bldg, "out_bldg")) return rc;
        if (int rc = check_ptr(indoor_temp, "indoor_temp", false)) return rc;
    }
    ObsArgs a;
    a.row = obs_table + (size_t)row * n_cols; a.col_src = col_src; a.col_scale = col_scale; a.state = state;
    a.out_bldg = out_bldg; a.indoor_temp = indoor_temp; a.obs = obs; a.extra = extra; a.n_extra_rows = n_extra_rows;
    a.n_env = dims->n_env; a.n_bldg = dims->n_bldg; a.n_cols = n_cols; a.all_exo = all_exo ? 1 : 0;
    a.ld = pitch_of(dims);
    if (a.ld != a.n_env && (indoor_temp || extra)) return fail(CL_EINVAL, "cl_observe_f32: env_pitch=%d != n_env=%d is not implemented with LSTM / flexible-load planes", a.ld, a.n_env);
    a.env_row0 = dims->env_row0;
    const bool vec4 = obs_pitch % 4 == 0;            // 16-byte stores need 16-byte aligned rows
    a.pitch = obs_pitch;
    const int n_seg = (n_cols + OBS_SEG - 1) / OBS_SEG;
    const dim3 grid((dims->n_env + OBS_TILE - 1) / OBS_TILE, n_seg);
    const int padded = obs_pitch < ((n_cols + 3) & ~3) ? obs_pitch : ((n_cols + 3) & ~3);   // columns written per row
    a.padded = padded;
    const bool listed = all_exo || (deps != nullptr && n_deps >= 0 && n_deps <= OBS_DEP_MAX);
    if (listed && !all_exo)
        for (int d = 0; d < n_deps; ++d)
            if (deps[d].col < 0 || deps[d].col >= n_cols || deps[d].src < 0)
                return fail(CL_EINVAL, "deps[%d]: col=%d src=%d", d, deps[d].col, deps[d].src);
    // Kernel choice (measured on MI355X, scripts/observe_bench.py / profiles/):
    //  * narrow vectors (half a wave of 16-byte column groups per row or less): LDS-tile kernel (52 columns: 11 vs 15 us);
    //  * wide vectors when the launch runs in more than ~one round of resident waves (> 96k envs) and the host-side list
    //    leaves no lane with more than OBS_WSLOTS dependent columns: wave-independent kernel -- its waves never
    //    synchronise, so the read latency of starting waves hides behind the stores of running ones
    //    (262 144 x 476: 112 vs 120 us row-wise; 65 536 x 476, a single round: 30 vs 27 us);
    //  * everything else (no list, > 1024 columns, odd pitch, crowded lanes): row-wise kernel.
    ObsTileArgs t;
    if (n_seg == 1 && listed) {
        static_assert(OBS_DEP_MAX == CLOB_MAX_DEPS, "header and kernel disagree");
        t.n_deps = all_exo ? 0 : n_deps;
        for (int d = 0; d < t.n_deps; ++d) t.deps[d] = deps[d];
    }
    const bool narrow = tun.obs_variant == 2 || (tun.obs_variant == 0 && padded <= 128);
    bool wide = n_seg == 1 && listed && vec4 && (tun.obs_variant == 3 || (tun.obs_variant == 0 && !narrow && dims->n_env > 98304));
    if (wide) {
        int owned[256] = {0};
        for (int d = 0; d < t.n_deps && wide; ++d) wide = ++owned[(deps[d].col >> 2) & 63] <= OBS_WSLOTS;
    }
    // every column env-dependent (the compact observation form) and few of them: a plain transpose of the planes
    const bool transpose = !all_exo && n_seg == 1 && listed && vec4 && t.n_deps == n_cols && n_cols <= OBS_TCOLS && obs_pitch <= OBS_TCOLS + 4 &&
                           (tun.obs_variant == 0 || tun.obs_variant == 4);
    // wide vectors in one segment with a host-side list: the one-round-trip row-wise kernel (obs_variant 5 forces it, 1 keeps the round-1 one)
    int row1_slots = 0;                               // most dependent columns any lane owns (lane = 16-byte column group mod 64)
    if (n_seg == 1 && listed) {
        int owned[64] = {0};
        for (int d = 0; d < t.n_deps; ++d) { const int n = ++owned[(deps[d].col >> 2) & 63]; row1_slots = n > row1_slots ? n : row1_slots; }
    }
    // (profiles/r04_observe_bench.log, 65 536 envs, round-1 kernel -> this one: 476 columns 27.6 -> 26.6 us, 527: 32.7 -> 31.5, 272: 26.9 -> 23.4,
    //  245: 19.6 -> 20.6 -- kept on the round-1 kernel --, 262 144 x 476: 122 -> 110 us, where it also beats the wave-independent kernel's 113.5)
    const bool row1 = n_seg == 1 && listed && vec4 && !transpose && row1_slots <= 4 && (tun.obs_variant == 5 || (tun.obs_variant == 0 && !narrow && padded >= 256));
    if (row1) wide = false;
    if (transpose) {
        t.o = a;
        hipLaunchKernelGGL(cl_observe_transpose_kernel, dim3((dims->n_env + OBS_TILE - 1) / OBS_TILE), dim3(OBS_THREADS), 0, (hipStream_t)stream, t);
    } else if (wide) {
        t.o = a;
        const int n_waves = (dims->n_env + OBS_WROWS - 1) / OBS_WROWS, per_wg = OBS_THREADS / 64;
        const dim3 wgrid((n_waves + per_wg - 1) / per_wg);
        if (padded <= 512) hipLaunchKernelGGL(cl_observe_wave_kernel<2>, wgrid, dim3(OBS_THREADS), 0, (hipStream_t)stream, t);
        else hipLaunchKernelGGL(cl_observe_wave_kernel<4>, wgrid, dim3(OBS_THREADS), 0, (hipStream_t)stream, t);
    } else if (row1) {
        t.o = a;
        const dim3 rgrid((dims->n_env + OBS_TILE - 1) / OBS_TILE);
        if (padded <= 512) {
            if (row1_slots <= 2) hipLaunchKernelGGL((cl_observe_row1_kernel<2, 2>), rgrid, dim3(OBS_THREADS), 0, (hipStream_t)stream, t);
            else hipLaunchKernelGGL((cl_observe_row1_kernel<2, 4>), rgrid, dim3(OBS_THREADS), 0, (hipStream_t)stream, t);
        } else hipLaunchKernelGGL((cl_observe_row1_kernel<4, 4>), rgrid, dim3(OBS_THREADS), 0, (hipStream_t)stream, t);
    } else if (n_seg == 1 && padded == obs_pitch && listed && narrow && dims->env_row0 == nullptr) {   // one template row per launch
        int r = tun.obs_rows ? tun.obs_rows : 16;          // 16 envs = one 64-byte line of every dependent plane
        while (r * obs_pitch > OBS_BUF) r >>= 1;       // pitch <= OBS_SEG + 3 -> r >= 4
        a.sub_rows = r;
        t.o = a;
        const int n_blocks = (dims->n_env + r - 1) / r, per_wg = OBS_TILE / r;
        hipLaunchKernelGGL(cl_observe_tile_kernel, dim3((n_blocks + per_wg - 1) / per_wg), dim3(OBS_THREADS), 0, (hipStream_t)stream, t);
    } else if (vec4) hipLaunchKernelGGL(cl_observe_kernel<4>, grid, dim3(OBS_THREADS), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(cl_observe_kernel<1>, grid, dim3(OBS_THREADS), 0, (hipStream_t)stream, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_fail(e, "cl_observe_kernel launch");
    return CL_OK;
}

float cl_philox_uniform(uint64_t seed, uint32_t env, uint32_t col, uint32_t t) {
    return cl::philox_u01(seed, env, col, t);
}

}  // extern "C"
#endif  // CL_TU_NOSLP
