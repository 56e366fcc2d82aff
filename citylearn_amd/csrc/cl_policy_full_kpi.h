// cl_policy_full_kpi.h -- mode B of a THERMAL district with a CLOSED-LOOP policy AND the streaming KPI accumulators: the K-step loop of
// cl_rollout_full_policy_kernel<1, PREC, MARL> (cl_policy_full.h) around the DETAIL unit, with the accumulators of full_step_body<.., KPI>
// (cl_full.h) and the district series of cl_rollout_kpi_kernel (cl_rollout.h) kept inside the launch.  Included by cl_policy_full_kpi.hip only
// (libcitylearn_amd_policy_full_kpi.so, include/citylearn_amd_policy_full_kpi.h), behind cl_policy_full.h for the staged-row layout.
//
// Nothing here is new arithmetic, and every accumulation keeps the order of the code tests/test_gpu_policy_full_kpi_rollout.py compares it with.
//  * From cl_rollout_full_policy_kernel, written out again (the policy block as a shared device function is not tried here: the parent's five
//    instantiations are pinned to their register counts, cl_policy.h's clpk_pins): state load / store, the staged `dep` / `out` / bounds row, the
//    hidden groups, the head loop, the per-step re-read of the parameter block, reward, record, district_reduce and the return rows.
//  * From full_step_body<.., KPI>: the twelve CL_NKB sums per (env, building), its `kv[CLK_*] +=` statements in its order, on the values of
//    clv::unit_step<F, OUT, DETAIL = true, PREC>.  They live in the wave's own LDS rows (the lane's own column: read - add - written per step, as
//    full_step_body's QLDS does with the district accumulators), loaded once before the loop and stored once behind it: with the table reads as
//    vector loads (below) twelve more registers next to the detail values did not fit the 128 of a 1024-thread workgroup (the parent's <1, 2, true>
//    has 113), and the sums in registers were not tried again afterwards.  CLK_UNSERVED_OUTAGE / CLK_EXPECTED_OUTAGE move on outage rows only and are
//    stored only if the launch saw one.
//  * From cl_rollout_kpi_kernel: the ring of S = CL_RKPI_S step slots of wave partials, here for BOTH district series -- slot [s][0][w] holds
//    building w's net of the step, [s][1][w] its baseline net -- folded every S steps and behind the last step through kpi_series_advance on the
//    absolute step index, the buildings in building order (nw <= 16: cl_kpi_kernel's 16-strided association too).  Wave 0 folds the control
//    series, the last wave the baseline series; both series are kept PER ENV ([2][12][64] in LDS): a thermal unit's baseline depends on the env
//    (kpi_shared_baseline is false for these engines).  MARL reads the ring slot it just wrote behind ONE barrier per step; the other rewards
//    meet a barrier at the folds only.
// One env per lane only (two envs per lane lost for the KPI step kernel: full_step_body's note), one building per wave, one workgroup row.
// Every instantiation holds a barrier inside the K loop, behind which the compiler fetches a plain read of the parameter / time-series tables with
// a vector load per lane (cl_rollout_full_kernel's note; the parent's MARL instantiations live with it): here that took the chain instantiations to
// 126 registers and 20 - 28 bytes of scratch.  cl_policy_full_kpi.hip therefore defines CL_TU_CONST_TABLES, under which cl::pw / pc / pd and
// clv::uword read those READ-ONLY tables through the constant address space -- scalar loads whatever surrounds them: 79 - 96 registers, no scratch.
// LDS per workgroup (rollout_full_policy_kpi_lds_floats): ring [S][2][nw][64] | series [2][12][64] | policy rows [nw][CLPF_ROW] | sums
// [nw][12][64]: 82 176 bytes at nine buildings, 141 312 at sixteen; above 64 KiB the launch opts in, above the CU's 160 KiB the host refuses.  The
// last step's district reduction ([nw][NQ][64]) and the return rows alias the ring (2 S >= NQ).
#pragma once

#ifdef __HIPCC__
namespace {

constexpr size_t rollout_full_policy_kpi_lds_floats(int nw) {
    return (size_t)CL_RKPI_S * 2 * nw * 64 + (size_t)2 * CLKE_PER_COND * 64 + (size_t)nw * CLPF_ROW + (size_t)nw * CL_NKB * 64;
}

template <int PREC, bool MARL>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4))) cl_rollout_full_policy_kpi_kernel(const PolicyArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];     // ring [S][2][nw][64] | series [2][12][64] | rows [nw][CLPF_ROW] | sums [nw][12][64]
    static_assert(CLKE_PER_COND == 12 && CL_NKB == 12, "the LDS layout is written for twelve accumulators per series and per unit");
    static_assert(2 * CL_RKPI_S >= NQ, "the district reduction's rows alias the ring");
    using F = float;
    constexpr int TILE = 64, S = CL_RKPI_S;
    const RolloutArgs& r = p.r;
    const StepArgs& a = r.s;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // = the wave's building (host: nw == n_bldg)
    const int tile_env0 = blockIdx.x * TILE;
    const int env0 = tile_env0 + lane;
    const bool live = env0 < a.n_env;
    const long long plane = (long long)a.n_bldg * a.n_env;
    const int rkind = (a.flags & CLD_REWARD_MASK) >> CLD_REWARD_SHIFT;
    const bool quirk = a.flags & CLD_REF_T0_QUIRK;
    const int H = p.n_hidden;
    const int blk = tile_env0 / CL_ROW0_BLOCK;
    const int row0 = a.env_row0 ? a.env_row0[blk] : 0;              // workgroup-uniform
    const int set = p.set_of_block ? p.set_of_block[blk] : 0;       // workgroup-uniform
    float* const ser = lds + (size_t)S * 2 * a.nw * TILE;           // control series [12][64], then the baseline series [12][64]
    float* const row = ser + (size_t)2 * CLKE_PER_COND * TILE + (size_t)w * CLPF_ROW;
    float* const ksum = ser + (size_t)2 * CLKE_PER_COND * TILE + (size_t)a.nw * CLPF_ROW + (size_t)w * CL_NKB * TILE + lane;
    // the district series' accumulators of this lane's env: kept by wave 0 (control) and by the last wave (baseline), which fold them
    const bool ser_c = w == 0 && live, ser_b = w == a.nw - 1 && live;

    const uint32_t* __restrict__ f = a.params + (long long)w * CL_NP + CLP_F_FIRST;
    [[maybe_unused]] const uint32_t* __restrict__ grow = PREC == 2 ? a.params + (long long)w * CL_NP : nullptr;
    const uint32_t flags = clv::uword<false>(f, 0);
    const int c_cs = (int)clv::uword<false>(f, 1), c_hs = (int)clv::uword<false>(f, 2), c_ds = (int)clv::uword<false>(f, 3), c_es = (int)clv::uword<false>(f, 4);
    const long long off = (long long)w * a.n_env + env0;
    const F zero = 0.0f, one = 1.0f;
    clv::St<F> S_ = {zero, one, zero, zero, zero, zero};
    // the previous step's net: what the reset observation shows in front of step 0, what the previous launch (or reset) left otherwise
    F last_net = (r.t0 == 0 && p.net_reset) ? p.net_reset[(long long)row0 * a.n_bldg + w] : 0.0f, last_rw = zero;
    if (live) {
        if (flags & CLF_BATTERY) {
            S_.soc = full_load<1>(a.state + CLS_B_SOC * plane + off); S_.eff = full_load<1>(a.state + CLS_B_EFF * plane + off);
            S_.degcap = full_load<1>(a.state + CLS_B_DEGCAP * plane + off);
        }
        if (flags & CLF_COOL_STO) S_.cs = full_load<1>(a.state + CLS_CS_SOC * plane + off);
        if (flags & CLF_HEAT_STO) S_.hs = full_load<1>(a.state + CLS_HS_SOC * plane + off);
        if (flags & CLF_DHW_STO) S_.ds = full_load<1>(a.state + CLS_DS_SOC * plane + off);
        if (r.t0 != 0) last_net = full_load<1>(a.out_bldg + CLO_NET * plane + off);
    }
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
    // stage the building's step-independent policy rows (this wave's own LDS row; the barrier below orders them): cl_rollout_full_policy_kernel's
    {
        const long long sb = (long long)set * a.n_bldg + w;
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
    const float* __restrict__ pre_w = p.pre + (((long long)set * p.n_rows + row0) * a.n_bldg + w) * H;
    float ret[1] = {0.0f}, q_net[1], q_cost[1], q_em[1], q_rw[1];
    q_net[0] = q_cost[0] = q_em[0] = q_rw[0] = 0.0f;
    bool saw_outage = false;                                         // wave-uniform

    for (int k = 0; k < r.k_steps; ++k) {
        const int t = r.t0 + k;
        const int slot = k & (S - 1);
        float* const tr = p.traj ? p.traj + (long long)k * CLPF_NT * plane + off : nullptr;
        q_net[0] = q_cost[0] = q_em[0] = q_rw[0] = 0.0f;

        // ---- the policy: this building's storage actions from (table row, soc, cs, hs, ds, previous net) -- cl_rollout_full_policy_kernel's ----
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
#define CLPFK_TERM(d, x) { const clpol_f4 wd = *reinterpret_cast<const clpol_f4*>(grp + 4 * (d)); \
                           _Pragma("unroll") for (int u = 0; u < 4; ++u) z[u] = clv::vfma((F)(wd[u]), x, z[u]); }
                if (flags & CLF_BATTERY) CLPFK_TERM(CLPF_D_SOC, S_.soc)
                if (flags & CLF_COOL_STO) CLPFK_TERM(CLPF_D_CS, S_.cs)
                if (flags & CLF_HEAT_STO) CLPFK_TERM(CLPF_D_HS, S_.hs)
                if (flags & CLF_DHW_STO) CLPFK_TERM(CLPF_D_DS, S_.ds)
                CLPFK_TERM(CLPF_D_NET, last_net)
#undef CLPFK_TERM
#pragma unroll
                for (int u = 0; u < 4; ++u) z[u] = clpol_unit(z[u]);
#define CLPFK_HEAD(h, acc) { const clpol_f4 wo = *reinterpret_cast<const clpol_f4*>(grp + 4 * (CLPF_ND + (h))); \
                             _Pragma("unroll") for (int u = 0; u < 4; ++u) acc = clv::vfma((F)(wo[u]), z[u], acc); }
                if (c_es >= 0) CLPFK_HEAD(CLPF_A_ES, acc_es)
                if (c_cs >= 0) CLPFK_HEAD(CLPF_A_CS, acc_cs)
                if (c_hs >= 0) CLPFK_HEAD(CLPF_A_HS, acc_hs)
                if (c_ds >= 0) CLPFK_HEAD(CLPF_A_DS, acc_ds)
#undef CLPFK_HEAD
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

        // ---- the packed thermal DETAIL unit as in full_step_body<.., KPI> (the per-step re-read of the parameter block: cl_rollout_full_kernel's note) ----
        const bool last = k == r.k_steps - 1;
        {
            int z;
            asm("s_mov_b32 %0, 0" : "=s"(z) : "s"(k));
            const uint32_t* __restrict__ fz = f + z;
            [[maybe_unused]] const uint32_t* __restrict__ gz = PREC == 2 ? grow + z : nullptr;
            clv::FP B;
            clv::load_fp<false>(B, fz);
            B.f = fz;
            cl::Row R;
            cl::load_row_scalar<true>(R, a.ts + ((long long)(t + row0) * a.n_bldg + w) * CL_NF, B.flags, nullptr);
            // (the evaluate()-time COP row of full_step_body's detail unit: only a dynamics building's baseline reads it)
            if (B.flags & CLF_DYNAMICS) R.icop_h_eval = cl::pw(reinterpret_cast<const uint32_t*>(a.ts + ((long long)(row0 + a.n_steps - 1) * a.n_bldg + w) * CL_NF), CLT_ICOP_HEAT);
            clv::Ou<F> O;
            const bool first = quirk && t == 0;
            if (R.outage) clv::unit_step<F, true, true, PREC>(B, R, t, first, act, S_, O, gz);
            else clv::unit_step<F, false, true, PREC>(B, R, t, first, act, S_, O, gz);
            const F rw = clv::unit_reward<F>(rkind, B, S_, O.net);
            last_net = O.net; last_rw = rw;
            q_net[0] += O.net; q_cost[0] += O.cost; q_em[0] += O.emission; q_rw[0] += rw;
            // this building's samples of the two district series
            lds[((size_t)(slot * 2 + 0) * a.nw + w) * TILE + lane] = O.net;
            lds[((size_t)(slot * 2 + 1) * a.nw + w) * TILE + lane] = O.base_net;
            if (last && live && (a.flags & CLD_WRITE_DETAIL)) {
                // the planes a chain engine's KPI pass reads (CLD_DETAIL_MIN: host), as K single steps would have left them
                full_store<1, false>(a.out_bldg + CLO_COOL_DEM * plane + off, O.cool_dem);
                full_store<1, false>(a.out_bldg + CLO_HEAT_DEM * plane + off, O.heat_dem);
                full_store<1, false>(a.out_bldg + CLO_BASE_NET * plane + off, O.base_net);
                full_store<1, false>(a.out_bldg + CLO_EXPECTED * plane + off, O.expected);
                full_store<1, false>(a.out_bldg + CLO_SERVED * plane + off, O.served);
            }
            // full_step_body's `kv[CLK_*] +=` block on the lane's LDS column
            {
                const float net = O.net, base = O.base_net, ex = O.expected, sv = O.served;
#define CLPFK_ADD(q, v) ksum[(q) * TILE] = ksum[(q) * TILE] + (v)
                CLPFK_ADD(CLK_C_POS, fmaxf(net, 0.0f));
                CLPFK_ADD(CLK_C_NET, net);
                CLPFK_ADD(CLK_C_EMISSION, fmaxf(net * R.carbon, 0.0f));
                CLPFK_ADD(CLK_C_COST, fmaxf(net * R.price, 0.0f));
                CLPFK_ADD(CLK_B_POS, fmaxf(base, 0.0f));
                CLPFK_ADD(CLK_B_NET, base);
                CLPFK_ADD(CLK_B_EMISSION, fmaxf(base * R.carbon, 0.0f));
                CLPFK_ADD(CLK_B_COST, fmaxf(base * R.price, 0.0f));
                if (R.outage) {                                          // wave-uniform
                    CLPFK_ADD(CLK_UNSERVED_OUTAGE, ex - sv); CLPFK_ADD(CLK_EXPECTED_OUTAGE, ex);
                    saw_outage = true;
                }
                CLPFK_ADD(CLK_UNSERVED_ALL, ex - sv);
                CLPFK_ADD(CLK_EXPECTED_ALL, ex);
#undef CLPFK_ADD
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
            if constexpr (!MARL) full_store<1, false>(tr + (long long)CLPF_T_REWARD * plane, last_rw);
        }
        if constexpr (MARL) {
            // the MARL reward couples the buildings through the district net of THIS step: the ring slot just written, behind one barrier
            __syncthreads();
            float dnet = 0.0f;
            for (int kk = 0; kk < a.nw; ++kk) dnet += lds[((size_t)(slot * 2) * a.nw + kk) * TILE + lane];
            last_rw = cl::marl_reward(last_net, dnet);
            ret[0] += last_rw;
            if (tr && live) full_store<1, false>(tr + (long long)CLPF_T_REWARD * plane, last_rw);
        } else {
            ret[0] += q_rw[0];
        }
        if (slot == S - 1 || last) {
            // fold the ring's slot + 1 samples (steps t - slot .. t) into the two district series
            if constexpr (!MARL) __syncthreads();                        // (MARL: everybody's slot is behind this step's barrier already)
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
            __syncthreads();                                             // the ring is free again (and, behind the last step, for the reduction rows)
        }
    }

    // ---- write back: carried state, the last step's per-building outputs, the KPI accumulators, district sums, episode-return partials ----
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
                if (saw_outage || (q != CLK_UNSERVED_OUTAGE && q != CLK_EXPECTED_OUTAGE)) full_store<1, false>(kp + q * plane, ksum[q * TILE]);
        }
    }
    if (r.k_steps > 0) {
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
        if constexpr (MARL) q_rw[0] = last_rw;
        district_reduce<1>(a, lds, w, lane, env0, live, plane, MARL ? (int)CLR_DEFAULT : rkind, q_net, q_cost, q_em, q_rw, a.nw);
    }
    if (r.ret_env) {
        __syncthreads();
        lds[(size_t)w * TILE + lane] = ret[0];
        __syncthreads();
        for (int e = threadIdx.x; e < TILE; e += blockDim.x) {
            float s = 0.0f;
            for (int kk = 0; kk < a.nw; ++kk) s += lds[(size_t)kk * TILE + e];
            if (tile_env0 + e < a.n_env) r.ret_env[tile_env0 + e] += s;
        }
    }
}

}  // namespace
#endif  // __HIPCC__
