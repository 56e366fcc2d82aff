// cl_policy_full.h -- mode B of a THERMAL district with a CLOSED-LOOP policy: ONE template source, cl_rollout_full_policy_kernel<VEC, PREC, MARL, KPI,
// CHUNK>, for the four per-building thermal policy rollouts.  Its base is the K-step loop of cl_rollout_full_kernel<VEC, false, PREC, MARL>
// (cl_rollout.h: the packed unit clv::unit_step in registers for K steps, one building per wave) whose storage actions of every (env, building, step)
// are the heads of a one-hidden-layer tanh MLP over that building's own observation vector, evaluated inside the loop from the five observations that
// depend on the env -- the unit's four storage socs before the step and its net of the previous step, all in registers already.
//
//     h_j    = tanh(pre[s][r][b][j] + sum_d dep[s][b][d][j] x_d)            x = (soc, cs, hs, ds, net_prev)
//     mean_a = mid_a + half_a tanh(out[s][b][a][H] + sum_j out[s][b][a][j] h_j)       a over the heads (es, cs, hs, ds)
//     act_a  = clamp(mean_a + sigma_a z_a, low_a, high_a)
// The pieces are cl_policy.h's (the hidden unit and the Box-Muller draw literally: cl_policy_common.h): `pre` through the constant address space (s_load_dwordx4 per four units); `dep` / `out` / bounds / sigma staged
// once per launch in the wave's own LDS row and read back as broadcast 16-byte reads; a hidden unit as (1 - e) / (1 + e), e = v_exp_f32 of the
// pre-scaled sum; tanhf for the output units; Box-Muller on the column's Philox stream.  What differs:
//  * Which terms and heads exist is a property of the BUILDING (its CLF_* storage flags, its action columns), hence wave-uniform: per group of four
//    hidden units every term / head sits behind a scalar branch, so a 2020 building pays for its 4 terms and <= 3 heads and not for zeros.
//  * The heads are finished -- tanhf, noise, clamp -- in ONE loop over a = 0 .. 3 that is not unrolled, with the head's accumulator picked by
//    wave-uniform selects: one copy of tanhf and of the Philox block in the code instead of four scheduled into each other
//    (cl_rollout_full_kernel's note on its six inlined block functions).
//  * No Philox cache: the blind kernel's per-wave LDS rows of drawn actions have no counterpart, a noisy head draws its block every step.
//
// Four units instantiate the template, each its own variant only, and report the kernel under the name in the second column:
//     cl_policy_full.hip            <VEC, PREC, MARL, false, false>   cl_rollout_full_policy_kernel<VEC, PREC, MARL>
//     cl_policy_full_kpi.hip        <1, PREC, MARL, true, false>      cl_rollout_full_policy_kpi_kernel<PREC, MARL>
//     cl_policy_full_chunk.hip      <VEC, PREC, false, false, true>   cl_rollout_full_policy_chunk_kernel<VEC, PREC>
//     cl_policy_full_chunk_kpi.hip  <1, PREC, false, true, true>      cl_rollout_full_policy_chunk_kpi_kernel<PREC>
// The statements all four share -- state load / store, the staged row, the hidden groups, the head loop, the per-step re-read of the parameter block,
// the unit, the reward, the record, district_reduce and the return rows -- exist once; what a switch turns on sits under `if constexpr`.  WHERE such a
// statement sits is deliberate: moving one changes the generated code of instantiations it does not even belong to
// (profiles/policy_full_one_source_isa.md has the cases; scripts/isa_compare.py compares the instruction text of two trees).
//
// KPI -- the streaming KPI accumulators inside the launch (one env per lane only: two envs per lane lost for the KPI step kernel, full_step_body's
// note).  Nothing is new arithmetic, and every accumulation keeps the order of the code tests/test_gpu_policy_full_kpi_rollout.py compares it with.
//  * The unit is the DETAIL unit clv::unit_step<F, OUT, true, PREC> with the evaluate()-time COP row, and the last step leaves the five planes a
//    chain engine's KPI pass reads (CLD_WRITE_DETAIL).
//  * From full_step_body<.., KPI> (cl_full.h): the twelve CL_NKB sums per (env, building), its `kv[CLK_*] +=` statements in its order, loaded once
//    before the loop and stored once behind it.  CLK_UNSERVED_OUTAGE / CLK_EXPECTED_OUTAGE move on outage rows only and are stored only if the
//    launch saw one.  WHERE the sums live depends on CHUNK.  One row: in the wave's own LDS rows (the lane's own column `ksum`: read - add - written
//    per step, as full_step_body's QLDS does with the district accumulators) -- with the table reads as vector loads (below) twelve more registers
//    next to the detail values did not fit the 128 of a 1024-thread workgroup (the plain <1, 2, true> has 113), and the sums in registers were not
//    tried again afterwards.  Chunked: in REGISTERS (`kv[]`); the chunk geometry's default of eight waves then keeps its LDS request under 64 KiB
//    -- 43 008 bytes -- where the LDS column would take it to 67 584.
//  * From cl_rollout_kpi_kernel (cl_rollout.h): the ring of S = CL_RKPI_S step slots of wave partials, here for BOTH district series -- slot
//    [s][0][w] holds building w's net of the step, [s][1][w] its baseline net.  One row: folded every S steps and behind the last step through
//    kpi_series_advance on the absolute step index, the buildings in building order (nw <= 16: cl_kpi_kernel's 16-strided association too).  Wave 0
//    folds the control series, the last wave the baseline series; both series are kept PER ENV ([2][12][64] in LDS): a thermal unit's baseline
//    depends on the env (kpi_shared_baseline is false for these engines).  MARL reads the ring slot it just wrote behind ONE barrier per step; the
//    other rewards meet a barrier at the folds only.  Chunked: see CHUNK + KPI.
//  * Every KPI instantiation holds a barrier inside the K loop, behind which the compiler fetches a plain read of the parameter / time-series tables
//    with a vector load per lane (cl_rollout_full_kernel's note; the plain MARL instantiations live with it): that took the one-row chain
//    instantiations to 126 registers and 20 - 28 bytes of scratch.  The two KPI units therefore define CL_TU_CONST_TABLES, under which cl::pw / pc /
//    pd and clv::uword read those READ-ONLY tables through the constant address space -- scalar loads whatever surrounds them: 79 - 96 registers,
//    no scratch.
//
// CHUNK -- a district of MORE THAN 16 buildings in the chunk geometry of cl_rollout_full_kernel<VEC, CHUNK = true, PREC>: the buildings are cut into
// chunks of `b_chunk` <= 16 along gridDim.y, wave w of workgroup row y owns building b = y b_chunk + w, and a workgroup ends with its chunk's partial
// district sums of the last step and its chunk's share of the K-step return in the scratch rows of out_bldg's reserved plane, which ONE
// cl_finish_kernel launch folds per launch (the two chunked units define CL_TU_FINISH).
//  * Everything the one-row kernel indexes by the wave index -- params, ts, state, out_bldg, pre, dep, out, net_reset, the traj planes -- is
//    indexed by the building; the Philox stream stays keyed by (global env, action column, step), so a chunk geometry does not change a draw.
//  * A wave WITHOUT a building (the tail of the last chunk: own = b < min(n_bldg, (y + 1) b_chunk), wave-uniform) reads the parameter words of a
//    clamped, valid row and then loads, stages, computes, records and stores nothing: it meets every barrier and adds zeros to the reductions.
//  * The last step's district sums go through district_reduce's n_chunks > 1 path, the return rows behind them (cl_rollout_full_kernel<CHUNK>'s place).
//  * Without KPI there is no barrier inside the K loop (a wave without a building skips the loop altogether), hence no MARL instantiation (a
//    chunked launch cannot couple the buildings inside a step anyway): the wave-uniform table reads stay scalar.
//
// CHUNK + KPI -- one call is three launches (cl_policy_full_chunk_kpi.h has the second kernel):
//  1. this kernel.  The district series need the DISTRICT net of every step, which no workgroup of a chunked launch sees: every wave parks its
//     building's net and baseline net of step k in slot k % S of the ring, and every S steps and behind the last step the workgroup adds the waves
//     in wave order and writes its CHUNK's partial samples to series_scratch[k][2][blockIdx.y][env].  The series accumulators are not touched here.
//  2. cl_kpi_series_chunk_kernel: both series per env from the n_chunks partials, through kpi_series_advance on the absolute step index.
//  3. cl_finish_kernel: the last step's district sums and the return, as behind the plain chunked kernel.
//  BARRIERS.  The K loop holds two barriers per fold.  Their condition is `slot == S - 1 || last`, a function of k, k_steps and S alone: a wave
//  without a building and a lane past n_env run the same schedule and park zeros -- nothing that depends on `own`, `live`, an outage row or a
//  building flag encloses a barrier.
//
// LDS per workgroup (the four rollout_full_policy*_lds_floats below); above 64 KiB the launch opts in, above the CU's 160 KiB the host refuses:
//     plain, chunked   [nw][NQ][tile] district reduction (MARL's exchange row and the return rows alias it) | policy rows [nw][CLPF_ROW]:
//                      52 KiB at the largest geometry (nw = 16, two envs per lane), 26 KiB at the chunk geometry's default eight waves
//     KPI              ring [S][2][nw][64] | series [2][12][64] | policy rows [nw][CLPF_ROW] | sums [nw][12][64]: 82 176 bytes at nine buildings,
//                      141 312 at sixteen
//     chunked KPI      ring [S][2][nw][64] | policy rows [nw][CLPF_ROW]: 86 016 bytes at sixteen waves
//  With KPI the last step's district reduction ([nw][NQ][64]) and the return rows alias the ring (2 S >= NQ).
#pragma once
#include "cl_policy_common.h"

#ifdef __HIPCC__
namespace {

constexpr int CLPF_GROUP = 4 * (CLPF_ND + CLPF_NA);            // floats of one group of four hidden units: [5 terms | 4 heads][4]
constexpr int CLPF_HEADS = CLPF_GROUP * (CLPF_MAX_HIDDEN / 4);  // where the heads' {bias, mid, half, sigma | low, high, -, -} start
constexpr int CLPF_ROW = CLPF_HEADS + 8 * CLPF_NA;              // floats of one building's staged row

constexpr size_t rollout_full_policy_lds_floats(int nw, int tile) { return (size_t)nw * NQ * tile + (size_t)nw * CLPF_ROW; }
constexpr size_t rollout_full_policy_chunk_lds_floats(int nw, int tile) { return (size_t)nw * NQ * tile + (size_t)nw * CLPF_ROW; }
constexpr size_t rollout_full_policy_kpi_lds_floats(int nw) {
    return (size_t)CL_RKPI_S * 2 * nw * 64 + (size_t)2 * CLKE_PER_COND * 64 + (size_t)nw * CLPF_ROW + (size_t)nw * CL_NKB * 64;
}
constexpr size_t rollout_full_policy_chunk_kpi_lds_floats(int nw) { return (size_t)CL_RKPI_S * 2 * nw * 64 + (size_t)nw * CLPF_ROW; }

// cl_policy_common.h's hidden unit on the packed pair
CL_DEV clv::f2 clpol_unit(clv::f2 z) { clv::f2 r; r.x = clpol_unit(z.x); r.y = clpol_unit(z.y); return r; }

// what the kernel takes by value: each variant keeps the kernarg layout it had (KPI && CHUNK: the launch arguments, then the scratch pointer)
struct FullPolicyChunkKpiArgs : PolicyArgs {
    float* __restrict__ series_scratch;    // [k_steps][2][n_chunks][n_env]: the chunks' partial samples of the two district series
};
template <bool KPI, bool CHUNK> using FullPolicyArgs = std::conditional_t<KPI && CHUNK, FullPolicyChunkKpiArgs, PolicyArgs>;

template <int VEC, int PREC, bool MARL, bool KPI, bool CHUNK>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4))) cl_rollout_full_policy_kernel(const FullPolicyArgs<KPI, CHUNK> p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];     // see the header comment
    static_assert(!KPI || VEC == 1, "the KPI variants run at one env per lane");
    static_assert(!CHUNK || !MARL, "a chunked launch cannot couple the buildings inside a step");
    static_assert(CLKE_PER_COND == 12 && CL_NKB == 12, "the LDS layout and the accounting are written for twelve accumulators per series and per unit");
    static_assert(2 * CL_RKPI_S >= NQ, "the district reduction's rows alias the ring");
    using F = typename Vec<VEC>::type;
    constexpr int TILE = 64 * VEC, RING = CL_RKPI_S;
    const RolloutArgs& r = p.r;
    const StepArgs& a = r.s;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // one row: = the wave's building (host: nw == n_bldg)
    const int tile_env0 = blockIdx.x * TILE;
    const int env0 = tile_env0 + lane * VEC;
    // b: the wave's building; own: it has one (wave-uniform); bi: the building whose tables, state and `pre` it reads
    [[maybe_unused]] int b = w, bi = w;
    [[maybe_unused]] bool own = true;
    if constexpr (CHUNK) {
        const int b_lo = blockIdx.y * a.b_chunk;
        const int b_hi = min(a.n_bldg, b_lo + a.b_chunk);
        b = b_lo + w;
        own = b < b_hi;
        // a wave without a building (only the last chunk has any: b >= n_bldg) reads a valid row, for its flag word only.  (Clamped with ONE min: as
        // `own ? b : min(b_lo, n_bldg - 1)`, cl_rollout_full_kernel's form, every instantiation reserved 20 bytes of scratch memory that no instruction touches.)
        bi = min(b, a.n_bldg - 1);
    }
    const bool live = (!CHUNK || own) && env0 < a.n_env;             // this lane holds a unit
    const long long plane = (long long)a.n_bldg * a.n_env;
    const int rkind = (a.flags & CLD_REWARD_MASK) >> CLD_REWARD_SHIFT;
    const bool quirk = a.flags & CLD_REF_T0_QUIRK;
    const int H = p.n_hidden;
    const int blk = tile_env0 / CL_ROW0_BLOCK;
    const int row0 = a.env_row0 ? a.env_row0[blk] : 0;              // workgroup-uniform
    const int set = p.set_of_block ? p.set_of_block[blk] : 0;       // workgroup-uniform
    // KPI && !CHUNK: control series [12][64], then the baseline series [12][64], behind the ring; `ksum`: the lane's column of its unit's twelve sums
    [[maybe_unused]] float* const ser = lds + (size_t)RING * 2 * a.nw * TILE;
    float* row;
    [[maybe_unused]] float* ksum = nullptr;
    if constexpr (KPI && !CHUNK) {
        row = ser + (size_t)2 * CLKE_PER_COND * TILE + (size_t)w * CLPF_ROW;
        ksum = ser + (size_t)2 * CLKE_PER_COND * TILE + (size_t)a.nw * CLPF_ROW + (size_t)w * CL_NKB * TILE + lane;
    } else if constexpr (KPI) {
        row = ser + (size_t)w * CLPF_ROW;
    } else {
        row = lds + (size_t)a.nw * NQ * TILE + (size_t)w * CLPF_ROW;
    }
    // (KPI && !CHUNK) the district series' accumulators of this lane's env: kept by wave 0 (control) and by the last wave (baseline), which fold them
    [[maybe_unused]] const bool ser_c = w == 0 && live, ser_b = w == a.nw - 1 && live;

    const uint32_t* __restrict__ f = a.params + (long long)bi * CL_NP + CLP_F_FIRST;
    [[maybe_unused]] const uint32_t* __restrict__ grow = PREC == 2 ? a.params + (long long)bi * CL_NP : nullptr;
    const uint32_t flags = clv::uword<false>(f, 0);
    const int c_cs = (int)clv::uword<false>(f, 1), c_hs = (int)clv::uword<false>(f, 2), c_ds = (int)clv::uword<false>(f, 3), c_es = (int)clv::uword<false>(f, 4);
    const long long off = (long long)bi * a.n_env + env0;
    const F zero = (F)(0.0f), one = (F)(1.0f);
    clv::St<F> S = {zero, one, zero, zero, zero, zero};
    // the previous step's net: what the reset observation shows in front of step 0, what the previous launch (or reset) left otherwise
    F last_net = (F)((r.t0 == 0 && p.net_reset) ? p.net_reset[(long long)row0 * a.n_bldg + bi] : 0.0f), last_rw = zero;
    [[maybe_unused]] float kv[CL_NKB];                               // (KPI && CHUNK) the unit's twelve sums
    if constexpr (KPI && CHUNK) {
#pragma unroll
        for (int q = 0; q < CL_NKB; ++q) kv[q] = 0.0f;
    }
    if (live) {
        if (flags & CLF_BATTERY) {
            S.soc = full_load<VEC>(a.state + CLS_B_SOC * plane + off); S.eff = full_load<VEC>(a.state + CLS_B_EFF * plane + off);
            S.degcap = full_load<VEC>(a.state + CLS_B_DEGCAP * plane + off);
        }
        if (flags & CLF_COOL_STO) S.cs = full_load<VEC>(a.state + CLS_CS_SOC * plane + off);
        if (flags & CLF_HEAT_STO) S.hs = full_load<VEC>(a.state + CLS_HS_SOC * plane + off);
        if (flags & CLF_DHW_STO) S.ds = full_load<VEC>(a.state + CLS_DS_SOC * plane + off);
        if (r.t0 != 0) last_net = full_load<VEC>(a.out_bldg + CLO_NET * plane + off);
        if constexpr (KPI && CHUNK) {
            const float* __restrict__ kp = a.kpi_bldg + off;
#pragma unroll
            for (int q = 0; q < CL_NKB; ++q) kv[q] = kp[q * plane];
        }
    }
    if constexpr (KPI && !CHUNK) {
        // the unit's twelve sums: HBM -> the lane's own LDS column
        {
            const float* __restrict__ kp = a.kpi_bldg + off;
#pragma unroll
            for (int q = 0; q < CL_NKB; ++q) ksum[q * TILE] = live ? kp[q * plane] : 0.0f;
        }
        if (ser_c) {
            KpiSeriesAll c;
            kpi_series_get(c, a.kpi_env + env0, a.n_env);
            kpi_series_put(ser + lane, TILE, c);
        }
        if (ser_b) {
            KpiSeriesAll c;
            kpi_series_get(c, a.kpi_env + (long long)CLKE_PER_COND * a.n_env + env0, a.n_env);
            kpi_series_put(ser + (size_t)CLKE_PER_COND * TILE + lane, TILE, c);
        }
    }
    // stage the building's step-independent policy rows (this wave's own LDS row; the barrier below orders them): lane j fetches hidden unit j's
    // nine weights, lane a < 4 head a's bias, bounds and sigma
    if (!CHUNK || own) {
        const long long sb = (long long)set * a.n_bldg + b;
        if (lane < H) {
            float* at = row + (lane >> 2) * CLPF_GROUP + (lane & 3);
#pragma unroll
            for (int d = 0; d < CLPF_ND; ++d) at[4 * d] = p.dep[(sb * CLPF_ND + d) * H + lane];
#pragma unroll
            for (int h = 0; h < CLPF_NA; ++h) at[4 * (CLPF_ND + h)] = p.out[(sb * CLPF_NA + h) * (H + 1) + lane];
        }
        if (lane < CLPF_NA) {
            const int col = lane == CLPF_A_ES ? c_es : lane == CLPF_A_CS ? c_cs : lane == CLPF_A_HS ? c_hs : c_ds;
            float* hp = row + CLPF_HEADS + 8 * lane;
            const bool has = col >= 0;
            const float lo = has ? r.act_low[col] : 0.0f, hi = has ? r.act_high[col] : 0.0f;
            hp[0] = has ? p.out[(sb * CLPF_NA + lane) * (H + 1) + H] : 0.0f;
            hp[1] = 0.5f * (hi + lo); hp[2] = 0.5f * (hi - lo);
            hp[3] = (has && p.sigma) ? p.sigma[col] : 0.0f;
            hp[4] = lo; hp[5] = hi; hp[6] = 0.0f; hp[7] = 0.0f;
        }
    }
    __syncthreads();
    // the `pre` rows of this wave's building in this workgroup's parameter set and episode window (inside the loop: + t n_bldg H)
    const float* __restrict__ pre_w = p.pre + (((long long)set * p.n_rows + row0) * a.n_bldg + bi) * H;
    // (what is zeroed in front of the loop is each variant's own: it is what keeps the chain instantiations free of reserved scratch)
    float ret[VEC], q_net[VEC], q_cost[VEC], q_em[VEC], q_rw[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        ret[i] = 0.0f;
        if constexpr (KPI || CHUNK) q_net[i] = q_cost[i] = q_em[i] = q_rw[i] = 0.0f;
    }
    [[maybe_unused]] bool saw_outage = false;                        // wave-uniform

    // CHUNK alone: no barrier inside, a wave without a building skips the loop altogether.  CHUNK && KPI: EVERY wave and lane of the workgroup runs
    // the loop (its barriers depend on k, k_steps and RING only), the step itself under `own`.
    for (int k = 0; (!CHUNK || KPI || own) && k < r.k_steps; ++k) {
        const int t = r.t0 + k;
        [[maybe_unused]] const int slot = k & (RING - 1);
        // (KPI) the launch's last step.  Chunked: computed here, the fold below needs it outside `if (own)`; one row: in front of the unit -- computed
        // here too, its instantiations come out in another instruction order (profiles/policy_full_one_source_isa.md)
        [[maybe_unused]] bool last = false;
        if constexpr (KPI && CHUNK) last = k == r.k_steps - 1;
        [[maybe_unused]] float smp_net = 0.0f, smp_base = 0.0f;      // (CHUNK && KPI) what this lane parks in the ring: zeros without a unit
        if (!(KPI && CHUNK) || own) {
            float* const tr = p.traj ? p.traj + (long long)k * CLPF_NT * plane + off : nullptr;
#pragma unroll
            for (int i = 0; i < VEC; ++i) q_net[i] = q_cost[i] = q_em[i] = q_rw[i] = 0.0f;

            // ---- the policy: this building's storage actions from (table row, soc, cs, hs, ds, previous net) ----
            clv::Ac<F> act = {zero, zero, zero, zero, zero, zero};
            {
                const clpol_c4ptr pq = (clpol_c4ptr)(const clpol_f4*)(pre_w + (long long)t * a.n_bldg * H);
                F acc_es = zero, acc_cs = zero, acc_hs = zero, acc_ds = zero;
#pragma unroll 1
                for (int g = 0; g < H; g += 4) {
                    const float* grp = row + (g >> 2) * CLPF_GROUP;
                    const clpol_f4 pj = pq[g >> 2];
                    F z[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) z[u] = (F)(pj[u]);
#define CLPF_TERM(d, x) { const clpol_f4 wd = *reinterpret_cast<const clpol_f4*>(grp + 4 * (d)); \
                              _Pragma("unroll") for (int u = 0; u < 4; ++u) z[u] = clv::vfma((F)(wd[u]), x, z[u]); }
                    if (flags & CLF_BATTERY) CLPF_TERM(CLPF_D_SOC, S.soc)
                    if (flags & CLF_COOL_STO) CLPF_TERM(CLPF_D_CS, S.cs)
                    if (flags & CLF_HEAT_STO) CLPF_TERM(CLPF_D_HS, S.hs)
                    if (flags & CLF_DHW_STO) CLPF_TERM(CLPF_D_DS, S.ds)
                    CLPF_TERM(CLPF_D_NET, last_net)
#undef CLPF_TERM
#pragma unroll
                    for (int u = 0; u < 4; ++u) z[u] = clpol_unit(z[u]);
#define CLPF_HEAD(h, acc) { const clpol_f4 wo = *reinterpret_cast<const clpol_f4*>(grp + 4 * (CLPF_ND + (h))); \
                                _Pragma("unroll") for (int u = 0; u < 4; ++u) acc = clv::vfma((F)(wo[u]), z[u], acc); }
                    if (c_es >= 0) CLPF_HEAD(CLPF_A_ES, acc_es)
                    if (c_cs >= 0) CLPF_HEAD(CLPF_A_CS, acc_cs)
                    if (c_hs >= 0) CLPF_HEAD(CLPF_A_HS, acc_hs)
                    if (c_ds >= 0) CLPF_HEAD(CLPF_A_DS, acc_ds)
#undef CLPF_HEAD
                }
#pragma unroll 1
                for (int h = 0; h < CLPF_NA; ++h) {
                    const int col = h == CLPF_A_ES ? c_es : h == CLPF_A_CS ? c_cs : h == CLPF_A_HS ? c_hs : c_ds;
                    if (col < 0) continue;                                   // wave-uniform
                    const clpol_f4 hp = *reinterpret_cast<const clpol_f4*>(row + CLPF_HEADS + 8 * h);      // bias, mid, half, sigma
                    const float lo = row[CLPF_HEADS + 8 * h + 4], hi = row[CLPF_HEADS + 8 * h + 5];
                    const F acc = h == CLPF_A_ES ? acc_es : h == CLPF_A_CS ? acc_cs : h == CLPF_A_HS ? acc_hs : acc_ds;
                    float v[VEC];
                    // (KPI: without the one-trip loop, inside which its instantiations get tanhf as selects instead of a branch)
                    if constexpr (KPI) {
                        v[0] = fmaf(hp[2], tanhf(acc + hp[0]), hp[1]);
                    } else {
#pragma unroll
                        for (int i = 0; i < VEC; ++i) {
                            float s;
                            if constexpr (VEC == 1) s = acc; else s = acc[i];
                            v[i] = fmaf(hp[2], tanhf(s + hp[0]), hp[1]);
                        }
                    }
                    // (through a float local: __builtin_bit_cast on the vector ELEMENT hp[3] copies from the start of the vector -- it read the bias)
                    const float sg_lane = hp[3];
                    const float sg = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, sg_lane)));
                    if (sg != 0.0f) {                                        // wave-uniform
#pragma unroll
                        for (int i = 0; i < VEC; ++i) {                      // (no cache: the block is drawn every step)
                            const cl::U4 bk = cl::philox_block(r.seed, (uint32_t)(env0 + i) + a.env_offset, (uint32_t)col, (uint32_t)t >> 1);
                            v[i] = fmaf(sg, clpol_gauss(bk.w[0], bk.w[1], bk.w[2], bk.w[3], t), v[i]);
                        }
                    }
                    F av;
#pragma unroll
                    for (int i = 0; i < VEC; ++i) {
                        const float c = fminf(fmaxf(v[i], lo), hi);
                        if constexpr (VEC == 1) av = c; else av[i] = c;
                    }
                    if (h == CLPF_A_ES) act.es = av; else if (h == CLPF_A_CS) act.cs = av; else if (h == CLPF_A_HS) act.hs = av; else act.ds = av;
                }
            }

            if constexpr (KPI && !CHUNK) last = k == r.k_steps - 1;      // (see its declaration)
            // ---- the packed thermal unit exactly as in cl_rollout_full_kernel (its note on the per-step re-read of the parameter block); KPI: the
            // DETAIL unit as in full_step_body<.., KPI> ----
            {
                int z;
                asm("s_mov_b32 %0, 0" : "=s"(z) : "s"(k));
                const uint32_t* __restrict__ fz = f + z;
                [[maybe_unused]] const uint32_t* __restrict__ gz = PREC == 2 ? grow + z : nullptr;
                clv::FP B;
                clv::load_fp<false>(B, fz);
                B.f = fz;
                cl::Row R;
                cl::load_row_scalar<true>(R, a.ts + ((long long)(t + row0) * a.n_bldg + bi) * CL_NF, B.flags, nullptr);
                if constexpr (KPI) {
                    // (the evaluate()-time COP row of full_step_body's detail unit: only a dynamics building's baseline reads it)
                    if (B.flags & CLF_DYNAMICS) R.icop_h_eval = cl::pw(reinterpret_cast<const uint32_t*>(a.ts + ((long long)(row0 + a.n_steps - 1) * a.n_bldg + bi) * CL_NF), CLT_ICOP_HEAT);
                }
                clv::Ou<F> O;
                const bool first = quirk && t == 0;
                if (R.outage) clv::unit_step<F, true, KPI, PREC>(B, R, t, first, act, S, O, gz);
                else clv::unit_step<F, false, KPI, PREC>(B, R, t, first, act, S, O, gz);
                const F rw = clv::unit_reward<F>(rkind, B, S, O.net);
                last_net = O.net; last_rw = rw;
                full_accumulate<VEC>(q_net, O.net); full_accumulate<VEC>(q_cost, O.cost); full_accumulate<VEC>(q_em, O.emission); full_accumulate<VEC>(q_rw, rw);
                if constexpr (KPI) {
                    // this building's samples of the two district series
                    if constexpr (CHUNK) {
                        if (live) { smp_net = O.net; smp_base = O.base_net; }
                    } else {
                        lds[((size_t)(slot * 2 + 0) * a.nw + w) * TILE + lane] = O.net;
                        lds[((size_t)(slot * 2 + 1) * a.nw + w) * TILE + lane] = O.base_net;
                    }
                    if (last && live && (a.flags & CLD_WRITE_DETAIL)) {
                        // the planes a chain engine's KPI pass reads (CLD_DETAIL_MIN: host), as K single steps would have left them
                        full_store<1, false>(a.out_bldg + CLO_COOL_DEM * plane + off, O.cool_dem);
                        full_store<1, false>(a.out_bldg + CLO_HEAT_DEM * plane + off, O.heat_dem);
                        full_store<1, false>(a.out_bldg + CLO_BASE_NET * plane + off, O.base_net);
                        full_store<1, false>(a.out_bldg + CLO_EXPECTED * plane + off, O.expected);
                        full_store<1, false>(a.out_bldg + CLO_SERVED * plane + off, O.served);
                    }
                    // full_step_body's `kv[CLK_*] +=` block: in registers when chunked, on the lane's LDS column otherwise
                    {
                        const float net = O.net, base = O.base_net, ex = O.expected, sv = O.served;
#define CLPF_ADD(q, v) { if constexpr (CHUNK) kv[q] += (v); else ksum[(q) * TILE] = ksum[(q) * TILE] + (v); }
                        CLPF_ADD(CLK_C_POS, fmaxf(net, 0.0f))
                        CLPF_ADD(CLK_C_NET, net)
                        CLPF_ADD(CLK_C_EMISSION, fmaxf(net * R.carbon, 0.0f))
                        CLPF_ADD(CLK_C_COST, fmaxf(net * R.price, 0.0f))
                        CLPF_ADD(CLK_B_POS, fmaxf(base, 0.0f))
                        CLPF_ADD(CLK_B_NET, base)
                        CLPF_ADD(CLK_B_EMISSION, fmaxf(base * R.carbon, 0.0f))
                        CLPF_ADD(CLK_B_COST, fmaxf(base * R.price, 0.0f))
                        if (R.outage) {                                          // wave-uniform
                            CLPF_ADD(CLK_UNSERVED_OUTAGE, ex - sv) CLPF_ADD(CLK_EXPECTED_OUTAGE, ex)
                            saw_outage = true;
                        }
                        CLPF_ADD(CLK_UNSERVED_ALL, ex - sv)
                        CLPF_ADD(CLK_EXPECTED_ALL, ex)
#undef CLPF_ADD
                    }
                }
            }
            if (tr && live) {
                full_store<VEC, false>(tr + (long long)(CLPF_T_ACTION + CLPF_A_ES) * plane, act.es);
                full_store<VEC, false>(tr + (long long)(CLPF_T_ACTION + CLPF_A_CS) * plane, act.cs);
                full_store<VEC, false>(tr + (long long)(CLPF_T_ACTION + CLPF_A_HS) * plane, act.hs);
                full_store<VEC, false>(tr + (long long)(CLPF_T_ACTION + CLPF_A_DS) * plane, act.ds);
                full_store<VEC, false>(tr + (long long)CLPF_T_NET * plane, last_net);
                full_store<VEC, false>(tr + (long long)(CLPF_T_SOC + CLPF_D_SOC) * plane, (flags & CLF_BATTERY) ? S.soc : zero);
                full_store<VEC, false>(tr + (long long)(CLPF_T_SOC + CLPF_D_CS) * plane, (flags & CLF_COOL_STO) ? S.cs : zero);
                full_store<VEC, false>(tr + (long long)(CLPF_T_SOC + CLPF_D_HS) * plane, (flags & CLF_HEAT_STO) ? S.hs : zero);
                full_store<VEC, false>(tr + (long long)(CLPF_T_SOC + CLPF_D_DS) * plane, (flags & CLF_DHW_STO) ? S.ds : zero);
                if constexpr (!MARL) full_store<VEC, false>(tr + (long long)CLPF_T_REWARD * plane, last_rw);
            }
            if constexpr (MARL) {
                // the MARL reward couples the buildings through the district net of THIS step: one LDS exchange per step
                if constexpr (KPI) {
                    // the ring slot just written, behind one barrier
                    __syncthreads();
                    float dnet = 0.0f;
                    for (int kk = 0; kk < a.nw; ++kk) dnet += lds[((size_t)(slot * 2) * a.nw + kk) * TILE + lane];
                    last_rw = cl::marl_reward(last_net, dnet);
                    ret[0] += last_rw;
                } else {
                    // an LDS row of its own (it aliases the district reduction's) between two barriers
                    vstore<VEC>(lds + (size_t)w * TILE + lane * VEC, q_net);
                    __syncthreads();
                    float dnet[VEC];
#pragma unroll
                    for (int i = 0; i < VEC; ++i) dnet[i] = 0.0f;
                    for (int kk = 0; kk < a.nw; ++kk) {
                        float part[VEC];
                        vload<VEC>(part, lds + (size_t)kk * TILE + lane * VEC);
#pragma unroll
                        for (int i = 0; i < VEC; ++i) dnet[i] += part[i];
                    }
                    __syncthreads();
#pragma unroll
                    for (int i = 0; i < VEC; ++i) {
                        float n_i, rw_i;
                        if constexpr (VEC == 1) n_i = last_net; else n_i = last_net[i];
                        rw_i = cl::marl_reward(n_i, dnet[i]);
                        if constexpr (VEC == 1) last_rw = rw_i; else last_rw[i] = rw_i;
                        ret[i] += rw_i;
                    }
                }
                if (tr && live) full_store<VEC, false>(tr + (long long)CLPF_T_REWARD * plane, last_rw);
            } else if constexpr (KPI) {
                ret[0] += q_rw[0];                                       // (inside the one-trip loop below this sum comes out with its operands swapped)
            } else {
#pragma unroll
                for (int i = 0; i < VEC; ++i) ret[i] += q_rw[i];
            }
        }
        if constexpr (KPI) {
            if constexpr (CHUNK) {
                // this building's samples of the two district series (a wave without a building, a lane without an env: zeros)
                lds[((size_t)(slot * 2 + 0) * a.nw + w) * TILE + lane] = smp_net;
                lds[((size_t)(slot * 2 + 1) * a.nw + w) * TILE + lane] = smp_base;
            }
            if (slot == RING - 1 || last) {
                if constexpr (!MARL) __syncthreads();                    // (MARL: everybody's slot is behind this step's barrier already)
                if constexpr (CHUNK) {
                    // the chunk's partial samples of steps k - slot .. k: the waves in wave order, to series_scratch[k][2][chunk][env]
                    const int kb = k - slot;
                    for (int i = threadIdx.x; i < (slot + 1) * 2 * TILE; i += blockDim.x) {
                        const int e = i & (TILE - 1), jc = i >> 6;           // jc = 2 j + series
                        float v = 0.0f;
                        for (int kk = 0; kk < a.nw; ++kk) v += lds[((size_t)jc * a.nw + kk) * TILE + e];
                        if (tile_env0 + e < a.n_env)
                            p.series_scratch[(((long long)kb * 2 + jc) * a.n_chunks + blockIdx.y) * a.n_env + tile_env0 + e] = v;
                    }
                } else {
                    // fold the ring's slot + 1 samples (steps t - slot .. t) into the two district series
                    const int tb = t - slot;
                    if (ser_c) {
                        for (int j = 0; j <= slot; ++j) {
                            float v = 0.0f;
                            for (int kk = 0; kk < a.nw; ++kk) v += lds[((size_t)(j * 2) * a.nw + kk) * TILE + lane];
                            kpi_series_advance(ser + lane, TILE, tb + j, v);
                        }
                    }
                    if (ser_b) {
                        for (int j = 0; j <= slot; ++j) {
                            float v = 0.0f;
                            for (int kk = 0; kk < a.nw; ++kk) v += lds[((size_t)(j * 2 + 1) * a.nw + kk) * TILE + lane];
                            kpi_series_advance(ser + (size_t)CLKE_PER_COND * TILE + lane, TILE, tb + j, v);
                        }
                    }
                }
                __syncthreads();                                         // the ring is free again (and, behind the last step, for the reduction rows)
            }
        }
    }

    // ---- write back: carried state, the last step's per-building outputs, the KPI accumulators, district sums (CHUNK: this chunk's partial sums),
    // episode-return partials (CHUNK: this chunk's share) ----
    if (live) {
        if (flags & CLF_BATTERY) {
            full_store<VEC, false>(a.state + CLS_B_SOC * plane + off, S.soc); full_store<VEC, false>(a.state + CLS_B_EFF * plane + off, S.eff);
            full_store<VEC, false>(a.state + CLS_B_DEGCAP * plane + off, S.degcap);
        }
        if (flags & CLF_COOL_STO) full_store<VEC, false>(a.state + CLS_CS_SOC * plane + off, S.cs);
        if (flags & CLF_HEAT_STO) full_store<VEC, false>(a.state + CLS_HS_SOC * plane + off, S.hs);
        if (flags & CLF_DHW_STO) full_store<VEC, false>(a.state + CLS_DS_SOC * plane + off, S.ds);
        if (r.k_steps > 0) {
            full_store<VEC, false>(a.out_bldg + CLO_NET * plane + off, last_net);
            full_store<VEC, false>(a.out_bldg + CLO_REWARD * plane + off, last_rw);
            if constexpr (KPI) {
                float* __restrict__ kp = a.kpi_bldg + off;
#pragma unroll
                for (int q = 0; q < CL_NKB; ++q)
                    if (saw_outage || (q != CLK_UNSERVED_OUTAGE && q != CLK_EXPECTED_OUTAGE)) full_store<1, false>(kp + q * plane, CHUNK ? kv[q] : ksum[q * TILE]);
            }
        }
    }
    if (r.k_steps > 0) {
        if constexpr (KPI && !CHUNK) {
            if (ser_c) {
                KpiSeriesAll c;
                kpi_series_get(c, ser + lane, TILE);
                kpi_series_put(a.kpi_env + env0, a.n_env, c);
            }
            if (ser_b) {
                KpiSeriesAll c;
                kpi_series_get(c, ser + (size_t)CLKE_PER_COND * TILE + lane, TILE);
                kpi_series_put(a.kpi_env + (long long)CLKE_PER_COND * a.n_env + env0, a.n_env, c);
            }
        }
        if constexpr (MARL) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                if constexpr (VEC == 1) q_rw[i] = last_rw; else q_rw[i] = last_rw[i];
            }
        }
        // (CHUNK, n_chunks > 1: the sums of the workgroup's waves go to scratch row (blockIdx.y, quantity) of the reserved plane; cl_finish_kernel adds the chunks)
        district_reduce<VEC>(a, lds, w, lane, env0, live, plane, MARL ? (int)CLR_DEFAULT : rkind, q_net, q_cost, q_em, q_rw, a.nw);
    }
    if (r.ret_env) {
        __syncthreads();
        vstore<VEC>(lds + (size_t)w * TILE + lane * VEC, ret);
        __syncthreads();
        for (int e = threadIdx.x; e < TILE; e += blockDim.x) {
            float s = 0.0f;
            for (int kk = 0; kk < a.nw; ++kk) s += lds[(size_t)kk * TILE + e];
            if (tile_env0 + e < a.n_env) {
                // CHUNK: this workgroup row's share of the return, its scratch row behind the n_chunks x NQ partial sums (cl_rollout_full_kernel<CHUNK>'s)
                if constexpr (CHUNK) a.out_bldg[(long long)CLO_RESERVED * plane + ((long long)a.n_chunks * NQ + blockIdx.y) * a.n_env + tile_env0 + e] = s;
                else r.ret_env[tile_env0 + e] += s;
            }
        }
    }
}

}  // namespace
#endif  // __HIPCC__
