// cl_policy_full_chunk_kpi.h -- mode B of a THERMAL district of MORE THAN 16 buildings with a CLOSED-LOOP policy AND the streaming KPI accumulators:
// cl_rollout_full_policy_chunk_kernel<1, PREC>'s geometry, policy block, Philox keying and record (cl_policy_full_chunk.h) around the DETAIL unit and
// the accounting of cl_rollout_full_policy_kpi_kernel<PREC, false> (cl_policy_full_kpi.h), and cl_kpi_series_chunk_kernel, which feeds the two
// district series from the chunks' partial samples.  Included by cl_policy_full_chunk_kpi.hip only (libcitylearn_amd_policy_full_chunk_kpi.so,
// include/citylearn_amd_policy_full_chunk_kpi.h).
//
// One call is three launches:
//  1. cl_rollout_full_policy_chunk_kpi_kernel<PREC>: the buildings cut into chunks of `b_chunk` <= 16 along gridDim.y, wave w of workgroup row y
//     owns building b = y b_chunk + w, one env per lane.  Per unit the twelve CL_NKB sums of full_step_body<.., KPI> in its order, in REGISTERS
//     (loaded once before the loop, stored once behind it; the chunk geometry's default of eight waves then keeps its LDS request under 64 KiB --
//     43 008 bytes -- where the one-row kernel's LDS column would take it to 67 584); CLK_UNSERVED_OUTAGE / CLK_EXPECTED_OUTAGE move on outage rows
//     only and are stored only if the launch saw one.  The district series need the DISTRICT net of every step, which no workgroup of a chunked
//     launch sees: every wave parks its building's net and baseline net of step k in slot k % S of the LDS ring [S][2][nw][64] (S = CL_RKPI_S),
//     and every S steps and behind the last step the workgroup adds the waves in wave order and writes its CHUNK's partial samples to
//     series_scratch[k][2][blockIdx.y][env].  The series accumulators are not touched here.
//  2. cl_kpi_series_chunk_kernel: per env, both series (2 x 12 rows of kpi_env) through kpi_series_advance on the absolute step index t0 + k, the
//     district sample of step k formed from the n_chunks partials in cl_finish_kernel's association -- sixteen strided partial sums (chunks j,
//     j + 16, ..), then their sum in order -- which depends on n_chunks = f(n_bldg, b_chunk) and on nothing else: not on K, t0, the env block or
//     how a caller cuts K steps into launches.
//  3. cl_finish_kernel: the last step's district sums and the return, as behind cl_rollout_full_policy_chunk_kernel.
//
// BARRIERS.  The K loop of kernel 1 holds two barriers per fold.  Their condition is `slot == S - 1 || last`, a function of k, k_steps and S alone:
// a wave without a building (the tail of the last chunk) and a lane past n_env run the same schedule and park zeros -- nothing that depends on
// `own`, `live`, an outage row or a building flag encloses a barrier.  With barriers inside the loop the table reads must not become vector loads
// (cl_policy_full_kpi.h's note): cl_policy_full_chunk_kpi.hip defines CL_TU_CONST_TABLES.
// LDS per workgroup (rollout_full_policy_chunk_kpi_lds_floats): ring [S][2][nw][64] | policy rows [nw][CLPF_ROW]; the last step's district
// reduction ([nw][NQ][64]) and the return rows alias the ring (2 S >= NQ).  86 016 bytes at sixteen waves: above 64 KiB the launch opts in.
#pragma once
#include "cl_policy_full.h"

#ifdef __HIPCC__
namespace {

constexpr size_t rollout_full_policy_chunk_kpi_lds_floats(int nw) { return (size_t)CL_RKPI_S * 2 * nw * 64 + (size_t)nw * CLPF_ROW; }

template <int PREC>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4))) cl_rollout_full_policy_chunk_kpi_kernel(const PolicyArgs p, float* __restrict__ series_scratch) {
    extern __shared__ __attribute__((aligned(16))) float lds[];     // ring [S][2][nw][64] | rows [nw][CLPF_ROW]
    static_assert(CL_NKB == 12, "the accounting is written for twelve accumulators per unit");
    static_assert(2 * CL_RKPI_S >= NQ, "the district reduction's rows alias the ring");
    using F = float;
    constexpr int TILE = 64, S = CL_RKPI_S;
    const RolloutArgs& r = p.r;
    const StepArgs& a = r.s;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile_env0 = blockIdx.x * TILE;
    const int env0 = tile_env0 + lane;
    const int b_lo = blockIdx.y * a.b_chunk;
    const int b_hi = min(a.n_bldg, b_lo + a.b_chunk);
    const int b = b_lo + w;
    const bool own = b < b_hi;                                       // wave-uniform
    const int bc = min(b, a.n_bldg - 1);                             // (a wave without a building reads a valid row, for its flag word only)
    const bool live = own && env0 < a.n_env;                         // this lane holds a unit
    const long long plane = (long long)a.n_bldg * a.n_env;
    const int rkind = (a.flags & CLD_REWARD_MASK) >> CLD_REWARD_SHIFT;
    const bool quirk = a.flags & CLD_REF_T0_QUIRK;
    const int H = p.n_hidden;
    const int blk = tile_env0 / CL_ROW0_BLOCK;
    const int row0 = a.env_row0 ? a.env_row0[blk] : 0;              // workgroup-uniform
    const int set = p.set_of_block ? p.set_of_block[blk] : 0;       // workgroup-uniform
    float* const row = lds + (size_t)S * 2 * a.nw * TILE + (size_t)w * CLPF_ROW;

    const uint32_t* __restrict__ f = a.params + (long long)bc * CL_NP + CLP_F_FIRST;
    [[maybe_unused]] const uint32_t* __restrict__ grow = PREC == 2 ? a.params + (long long)bc * CL_NP : nullptr;
    const uint32_t flags = clv::uword<false>(f, 0);
    const int c_cs = (int)clv::uword<false>(f, 1), c_hs = (int)clv::uword<false>(f, 2), c_ds = (int)clv::uword<false>(f, 3), c_es = (int)clv::uword<false>(f, 4);
    const long long off = (long long)bc * a.n_env + env0;
    const F zero = 0.0f, one = 1.0f;
    clv::St<F> S_ = {zero, one, zero, zero, zero, zero};
    // the previous step's net: what the reset observation shows in front of step 0, what the previous launch (or reset) left otherwise
    F last_net = (r.t0 == 0 && p.net_reset) ? p.net_reset[(long long)row0 * a.n_bldg + bc] : 0.0f, last_rw = zero;
    float kv[CL_NKB];                                                // the unit's twelve sums
#pragma unroll
    for (int q = 0; q < CL_NKB; ++q) kv[q] = 0.0f;
    if (live) {
        if (flags & CLF_BATTERY) {
            S_.soc = full_load<1>(a.state + CLS_B_SOC * plane + off); S_.eff = full_load<1>(a.state + CLS_B_EFF * plane + off);
            S_.degcap = full_load<1>(a.state + CLS_B_DEGCAP * plane + off);
        }
        if (flags & CLF_COOL_STO) S_.cs = full_load<1>(a.state + CLS_CS_SOC * plane + off);
        if (flags & CLF_HEAT_STO) S_.hs = full_load<1>(a.state + CLS_HS_SOC * plane + off);
        if (flags & CLF_DHW_STO) S_.ds = full_load<1>(a.state + CLS_DS_SOC * plane + off);
        if (r.t0 != 0) last_net = full_load<1>(a.out_bldg + CLO_NET * plane + off);
        const float* __restrict__ kp = a.kpi_bldg + off;
#pragma unroll
        for (int q = 0; q < CL_NKB; ++q) kv[q] = kp[q * plane];
    }
    // stage the building's step-independent policy rows (this wave's own LDS row; the barrier below orders them): cl_rollout_full_policy_chunk_kernel's
    if (own) {
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
    const float* __restrict__ pre_w = p.pre + (((long long)set * p.n_rows + row0) * a.n_bldg + bc) * H;
    float ret[1] = {0.0f}, q_net[1], q_cost[1], q_em[1], q_rw[1];
    q_net[0] = q_cost[0] = q_em[0] = q_rw[0] = 0.0f;
    bool saw_outage = false;                                         // wave-uniform

    // EVERY wave and lane of the workgroup runs this loop: its barriers depend on k, k_steps and S only
    for (int k = 0; k < r.k_steps; ++k) {
        const int t = r.t0 + k;
        const int slot = k & (S - 1);
        const bool last = k == r.k_steps - 1;
        float smp_net = 0.0f, smp_base = 0.0f;                       // what this lane parks in the ring: zeros without a unit
        if (own) {
            float* const tr = p.traj ? p.traj + (long long)k * CLPF_NT * plane + off : nullptr;
            q_net[0] = q_cost[0] = q_em[0] = q_rw[0] = 0.0f;

            // ---- the policy: this building's storage actions from (table row, soc, cs, hs, ds, previous net) -- cl_rollout_full_policy_chunk_kernel's ----
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
                    for (int u = 0; u < 4; ++u) z[u] = pj[u];
#define CLPFCK_TERM(d, x) { const clpol_f4 wd = *reinterpret_cast<const clpol_f4*>(grp + 4 * (d)); \
                            _Pragma("unroll") for (int u = 0; u < 4; ++u) z[u] = clv::vfma((F)(wd[u]), x, z[u]); }
                    if (flags & CLF_BATTERY) CLPFCK_TERM(CLPF_D_SOC, S_.soc)
                    if (flags & CLF_COOL_STO) CLPFCK_TERM(CLPF_D_CS, S_.cs)
                    if (flags & CLF_HEAT_STO) CLPFCK_TERM(CLPF_D_HS, S_.hs)
                    if (flags & CLF_DHW_STO) CLPFCK_TERM(CLPF_D_DS, S_.ds)
                    CLPFCK_TERM(CLPF_D_NET, last_net)
#undef CLPFCK_TERM
#pragma unroll
                    for (int u = 0; u < 4; ++u) z[u] = clpol_unit(z[u]);
#define CLPFCK_HEAD(h, acc) { const clpol_f4 wo = *reinterpret_cast<const clpol_f4*>(grp + 4 * (CLPF_ND + (h))); \
                              _Pragma("unroll") for (int u = 0; u < 4; ++u) acc = clv::vfma((F)(wo[u]), z[u], acc); }
                    if (c_es >= 0) CLPFCK_HEAD(CLPF_A_ES, acc_es)
                    if (c_cs >= 0) CLPFCK_HEAD(CLPF_A_CS, acc_cs)
                    if (c_hs >= 0) CLPFCK_HEAD(CLPF_A_HS, acc_hs)
                    if (c_ds >= 0) CLPFCK_HEAD(CLPF_A_DS, acc_ds)
#undef CLPFCK_HEAD
                }
#pragma unroll 1
                for (int h = 0; h < CLPF_NA; ++h) {
                    const int col = h == CLPF_A_ES ? c_es : h == CLPF_A_CS ? c_cs : h == CLPF_A_HS ? c_hs : c_ds;
                    if (col < 0) continue;                                   // wave-uniform
                    const clpol_f4 hp = *reinterpret_cast<const clpol_f4*>(row + CLPF_HEADS + 8 * h);      // bias, mid, half, sigma
                    const float lo = row[CLPF_HEADS + 8 * h + 4], hi = row[CLPF_HEADS + 8 * h + 5];
                    const F acc = h == CLPF_A_ES ? acc_es : h == CLPF_A_CS ? acc_cs : h == CLPF_A_HS ? acc_hs : acc_ds;
                    float v = fmaf(hp[2], tanhf(acc + hp[0]), hp[1]);
                    // (through a float local: cl_rollout_full_policy_kernel's note)
                    const float sg_lane = hp[3];
                    const float sg = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, sg_lane)));
                    if (sg != 0.0f) {                                        // wave-uniform; (no cache: the block is drawn every step)
                        const cl::U4 bk = cl::philox_block(r.seed, (uint32_t)env0 + a.env_offset, (uint32_t)col, (uint32_t)t >> 1);
                        v = fmaf(sg, clpol_gauss(bk.w[0], bk.w[1], bk.w[2], bk.w[3], t), v);
                    }
                    const F av = fminf(fmaxf(v, lo), hi);
                    if (h == CLPF_A_ES) act.es = av; else if (h == CLPF_A_CS) act.cs = av; else if (h == CLPF_A_HS) act.hs = av; else act.ds = av;
                }
            }

            // ---- the packed thermal DETAIL unit as in cl_rollout_full_policy_kpi_kernel (the per-step re-read of the parameter block: cl_rollout_full_kernel's note) ----
            {
                int z;
                asm("s_mov_b32 %0, 0" : "=s"(z) : "s"(k));
                const uint32_t* __restrict__ fz = f + z;
                [[maybe_unused]] const uint32_t* __restrict__ gz = PREC == 2 ? grow + z : nullptr;
                clv::FP B;
                clv::load_fp<false>(B, fz);
                B.f = fz;
                cl::Row R;
                cl::load_row_scalar<true>(R, a.ts + ((long long)(t + row0) * a.n_bldg + bc) * CL_NF, B.flags, nullptr);
                // (the evaluate()-time COP row of full_step_body's detail unit: only a dynamics building's baseline reads it)
                if (B.flags & CLF_DYNAMICS) R.icop_h_eval = cl::pw(reinterpret_cast<const uint32_t*>(a.ts + ((long long)(row0 + a.n_steps - 1) * a.n_bldg + bc) * CL_NF), CLT_ICOP_HEAT);
                clv::Ou<F> O;
                const bool first = quirk && t == 0;
                if (R.outage) clv::unit_step<F, true, true, PREC>(B, R, t, first, act, S_, O, gz);
                else clv::unit_step<F, false, true, PREC>(B, R, t, first, act, S_, O, gz);
                const F rw = clv::unit_reward<F>(rkind, B, S_, O.net);
                last_net = O.net; last_rw = rw;
                q_net[0] += O.net; q_cost[0] += O.cost; q_em[0] += O.emission; q_rw[0] += rw;
                if (live) { smp_net = O.net; smp_base = O.base_net; }
                if (last && live && (a.flags & CLD_WRITE_DETAIL)) {
                    // the planes a chain engine's KPI pass reads (CLD_DETAIL_MIN: host), as K single steps would have left them
                    full_store<1, false>(a.out_bldg + CLO_COOL_DEM * plane + off, O.cool_dem);
                    full_store<1, false>(a.out_bldg + CLO_HEAT_DEM * plane + off, O.heat_dem);
                    full_store<1, false>(a.out_bldg + CLO_BASE_NET * plane + off, O.base_net);
                    full_store<1, false>(a.out_bldg + CLO_EXPECTED * plane + off, O.expected);
                    full_store<1, false>(a.out_bldg + CLO_SERVED * plane + off, O.served);
                }
                // full_step_body's `kv[CLK_*] +=` block
                {
                    const float net = O.net, base = O.base_net, ex = O.expected, sv = O.served;
                    kv[CLK_C_POS] += fmaxf(net, 0.0f);
                    kv[CLK_C_NET] += net;
                    kv[CLK_C_EMISSION] += fmaxf(net * R.carbon, 0.0f);
                    kv[CLK_C_COST] += fmaxf(net * R.price, 0.0f);
                    kv[CLK_B_POS] += fmaxf(base, 0.0f);
                    kv[CLK_B_NET] += base;
                    kv[CLK_B_EMISSION] += fmaxf(base * R.carbon, 0.0f);
                    kv[CLK_B_COST] += fmaxf(base * R.price, 0.0f);
                    if (R.outage) {                                          // wave-uniform
                        kv[CLK_UNSERVED_OUTAGE] += ex - sv; kv[CLK_EXPECTED_OUTAGE] += ex;
                        saw_outage = true;
                    }
                    kv[CLK_UNSERVED_ALL] += ex - sv;
                    kv[CLK_EXPECTED_ALL] += ex;
                }
            }
            if (tr && live) {
                full_store<1, false>(tr + (long long)(CLPF_T_ACTION + CLPF_A_ES) * plane, act.es);
                full_store<1, false>(tr + (long long)(CLPF_T_ACTION + CLPF_A_CS) * plane, act.cs);
                full_store<1, false>(tr + (long long)(CLPF_T_ACTION + CLPF_A_HS) * plane, act.hs);
                full_store<1, false>(tr + (long long)(CLPF_T_ACTION + CLPF_A_DS) * plane, act.ds);
                full_store<1, false>(tr + (long long)CLPF_T_NET * plane, last_net);
                full_store<1, false>(tr + (long long)(CLPF_T_SOC + CLPF_D_SOC) * plane, (flags & CLF_BATTERY) ? S_.soc : zero);
                full_store<1, false>(tr + (long long)(CLPF_T_SOC + CLPF_D_CS) * plane, (flags & CLF_COOL_STO) ? S_.cs : zero);
                full_store<1, false>(tr + (long long)(CLPF_T_SOC + CLPF_D_HS) * plane, (flags & CLF_HEAT_STO) ? S_.hs : zero);
                full_store<1, false>(tr + (long long)(CLPF_T_SOC + CLPF_D_DS) * plane, (flags & CLF_DHW_STO) ? S_.ds : zero);
                full_store<1, false>(tr + (long long)CLPF_T_REWARD * plane, last_rw);
            }
            ret[0] += q_rw[0];
        }
        // this building's samples of the two district series (a wave without a building, a lane without an env: zeros)
        lds[((size_t)(slot * 2 + 0) * a.nw + w) * TILE + lane] = smp_net;
        lds[((size_t)(slot * 2 + 1) * a.nw + w) * TILE + lane] = smp_base;
        if (slot == S - 1 || last) {
            // the chunk's partial samples of steps k - slot .. k: the waves in wave order, to series_scratch[k][2][chunk][env]
            __syncthreads();
            const int kb = k - slot;
            for (int i = threadIdx.x; i < (slot + 1) * 2 * TILE; i += blockDim.x) {
                const int e = i & (TILE - 1), jc = i >> 6;                   // jc = 2 j + series
                float v = 0.0f;
                for (int kk = 0; kk < a.nw; ++kk) v += lds[((size_t)jc * a.nw + kk) * TILE + e];
                if (tile_env0 + e < a.n_env)
                    series_scratch[(((long long)kb * 2 + jc) * a.n_chunks + blockIdx.y) * a.n_env + tile_env0 + e] = v;
            }
            __syncthreads();                                             // the ring is free again (and, behind the last step, for the reduction rows)
        }
    }

    // ---- write back: carried state, the last step's per-building outputs, the unit's sums, this chunk's partial district sums and its share of the return ----
    if (live) {
        if (flags & CLF_BATTERY) {
            full_store<1, false>(a.state + CLS_B_SOC * plane + off, S_.soc); full_store<1, false>(a.state + CLS_B_EFF * plane + off, S_.eff);
            full_store<1, false>(a.state + CLS_B_DEGCAP * plane + off, S_.degcap);
        }
        if (flags & CLF_COOL_STO) full_store<1, false>(a.state + CLS_CS_SOC * plane + off, S_.cs);
        if (flags & CLF_HEAT_STO) full_store<1, false>(a.state + CLS_HS_SOC * plane + off, S_.hs);
        if (flags & CLF_DHW_STO) full_store<1, false>(a.state + CLS_DS_SOC * plane + off, S_.ds);
        if (r.k_steps > 0) {
            full_store<1, false>(a.out_bldg + CLO_NET * plane + off, last_net);
            full_store<1, false>(a.out_bldg + CLO_REWARD * plane + off, last_rw);
            float* __restrict__ kp = a.kpi_bldg + off;
#pragma unroll
            for (int q = 0; q < CL_NKB; ++q)
                if (saw_outage || (q != CLK_UNSERVED_OUTAGE && q != CLK_EXPECTED_OUTAGE)) full_store<1, false>(kp + q * plane, kv[q]);
        }
    }
    // (n_chunks > 1: the sums of the workgroup's waves go to scratch row (blockIdx.y, quantity) of the reserved plane; cl_finish_kernel adds the chunks)
    if (r.k_steps > 0) district_reduce<1>(a, lds, w, lane, env0, live, plane, rkind, q_net, q_cost, q_em, q_rw, a.nw);
    if (r.ret_env) {
        __syncthreads();
        lds[(size_t)w * TILE + lane] = ret[0];
        __syncthreads();
        // this workgroup row's share of the return: its scratch row behind the n_chunks x NQ partial sums (cl_rollout_full_policy_chunk_kernel's)
        for (int e = threadIdx.x; e < TILE; e += blockDim.x) {
            float s = 0.0f;
            for (int kk = 0; kk < a.nw; ++kk) s += lds[(size_t)kk * TILE + e];
            if (tile_env0 + e < a.n_env)
                a.out_bldg[(long long)CLO_RESERVED * plane + ((long long)a.n_chunks * NQ + blockIdx.y) * a.n_env + tile_env0 + e] = s;
        }
    }
}

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
