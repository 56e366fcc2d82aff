// cl_policy_full_chunk.h -- mode B of a THERMAL district of MORE THAN 16 buildings with a CLOSED-LOOP policy: the K loop of
// cl_rollout_full_policy_kernel<VEC, PREC, false> (cl_policy_full.h: the storage heads of a one-hidden-layer tanh MLP evaluated inside the loop from
// the unit's four socs and its previous net, then the packed thermal unit clv::unit_step) in the chunk geometry of
// cl_rollout_full_kernel<VEC, CHUNK = true, PREC> (cl_rollout.h): the buildings are cut into chunks of `b_chunk` <= 16 along gridDim.y, wave w of
// workgroup row y owns building b = y b_chunk + w, and a workgroup ends with its chunk's partial district sums of the last step and its chunk's share
// of the K-step return in the scratch rows of out_bldg's reserved plane, which ONE cl_finish_kernel launch folds per launch.  Included by
// cl_policy_full_chunk.hip only (libcitylearn_amd_policy_full_chunk.so, include/citylearn_amd_policy_full_chunk.h).
//
// What differs from the one-row kernel:
//  * everything it indexes by the wave index -- params, ts, state, out_bldg, pre, dep, out, net_reset, the traj planes -- is indexed by b here; the
//    Philox stream stays keyed by (global env, action column, step), so a chunk geometry does not change a draw;
//  * a wave WITHOUT a building (the tail of the last chunk: own = b < min(n_bldg, (y + 1) b_chunk), wave-uniform) reads the parameter words of a
//    clamped, valid row and then loads, stages, computes, records and stores nothing: it meets every barrier and adds zeros to the reductions;
//  * the last step's district sums go through district_reduce's n_chunks > 1 path, the return rows behind them (cl_rollout_full_kernel<CHUNK>'s place);
//  * no barrier inside the K loop, hence no MARL instantiation (a chunked launch cannot couple the buildings inside a step anyway): the
//    wave-uniform table reads stay scalar (cl_rollout_full_kernel's note on its MARL instantiations).
// The policy block is written out again (as cl_policy_full_kpi.h does): shared functions changed the parents' generated code before
// (profiles/policy_refactor_isa.md), and one template source for the thermal kernels (profiles/policy_one_source_isa.md has the rule) is not
// attempted.  LDS per workgroup: cl_policy_full.h's formula, [nw][NQ][tile] reduction rows (the return rows alias them) +
// nw x CLPF_ROW floats -- 26 KiB at the default eight waves and two envs per lane, 52 KiB at sixteen.
#pragma once
#include "cl_policy_full.h"

#ifdef __HIPCC__
namespace {

constexpr size_t rollout_full_policy_chunk_lds_floats(int nw, int tile) { return (size_t)nw * NQ * tile + (size_t)nw * CLPF_ROW; }

template <int VEC, int PREC>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4))) cl_rollout_full_policy_chunk_kernel(const PolicyArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];     // [nw][NQ][64*VEC] | [nw][CLPF_ROW]
    using F = typename Vec<VEC>::type;
    const RolloutArgs& r = p.r;
    const StepArgs& a = r.s;
    constexpr int TILE = 64 * VEC;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile_env0 = blockIdx.x * TILE;
    const int env0 = tile_env0 + lane * VEC;
    const int b_lo = blockIdx.y * a.b_chunk;
    const int b_hi = min(a.n_bldg, b_lo + a.b_chunk);
    const int b = b_lo + w;
    const bool own = b < b_hi;                                       // wave-uniform
    // a wave without a building (only the last chunk has any: b >= n_bldg) reads a valid row, for its flag word only.  (Clamped with ONE min: as
    // `own ? b : min(b_lo, n_bldg - 1)`, cl_rollout_full_kernel's form, every instantiation reserved 20 bytes of scratch memory that no instruction touches.)
    const int bc = min(b, a.n_bldg - 1);
    const bool live = own && env0 < a.n_env;                         // this lane holds a unit
    const long long plane = (long long)a.n_bldg * a.n_env;
    const int rkind = (a.flags & CLD_REWARD_MASK) >> CLD_REWARD_SHIFT;
    const bool quirk = a.flags & CLD_REF_T0_QUIRK;
    const int H = p.n_hidden;
    const int blk = tile_env0 / CL_ROW0_BLOCK;
    const int row0 = a.env_row0 ? a.env_row0[blk] : 0;              // workgroup-uniform
    const int set = p.set_of_block ? p.set_of_block[blk] : 0;       // workgroup-uniform
    float* const row = lds + (size_t)a.nw * NQ * TILE + (size_t)w * CLPF_ROW;

    const uint32_t* __restrict__ f = a.params + (long long)bc * CL_NP + CLP_F_FIRST;
    [[maybe_unused]] const uint32_t* __restrict__ grow = PREC == 2 ? a.params + (long long)bc * CL_NP : nullptr;
    const uint32_t flags = clv::uword<false>(f, 0);
    const int c_cs = (int)clv::uword<false>(f, 1), c_hs = (int)clv::uword<false>(f, 2), c_ds = (int)clv::uword<false>(f, 3), c_es = (int)clv::uword<false>(f, 4);
    const long long off = (long long)bc * a.n_env + env0;
    const F zero = (F)(0.0f), one = (F)(1.0f);
    clv::St<F> S = {zero, one, zero, zero, zero, zero};
    // the previous step's net: what the reset observation shows in front of step 0, what the previous launch (or reset) left otherwise
    F last_net = (F)((r.t0 == 0 && p.net_reset) ? p.net_reset[(long long)row0 * a.n_bldg + bc] : 0.0f), last_rw = zero;
    if (live) {
        if (flags & CLF_BATTERY) {
            S.soc = full_load<VEC>(a.state + CLS_B_SOC * plane + off); S.eff = full_load<VEC>(a.state + CLS_B_EFF * plane + off);
            S.degcap = full_load<VEC>(a.state + CLS_B_DEGCAP * plane + off);
        }
        if (flags & CLF_COOL_STO) S.cs = full_load<VEC>(a.state + CLS_CS_SOC * plane + off);
        if (flags & CLF_HEAT_STO) S.hs = full_load<VEC>(a.state + CLS_HS_SOC * plane + off);
        if (flags & CLF_DHW_STO) S.ds = full_load<VEC>(a.state + CLS_DS_SOC * plane + off);
        if (r.t0 != 0) last_net = full_load<VEC>(a.out_bldg + CLO_NET * plane + off);
    }
    // stage the building's step-independent policy rows (this wave's own LDS row; the barrier below orders them): lane j fetches hidden unit j's
    // nine weights, lane a < 4 head a's bias, bounds and sigma
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
    float ret[VEC], q_net[VEC], q_cost[VEC], q_em[VEC], q_rw[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) ret[i] = q_net[i] = q_cost[i] = q_em[i] = q_rw[i] = 0.0f;

    // (no barrier inside: a wave without a building skips the loop altogether)
    for (int k = 0; own && k < r.k_steps; ++k) {
        const int t = r.t0 + k;
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
#define CLPFC_TERM(d, x) { const clpol_f4 wd = *reinterpret_cast<const clpol_f4*>(grp + 4 * (d)); \
                           _Pragma("unroll") for (int u = 0; u < 4; ++u) z[u] = clv::vfma((F)(wd[u]), x, z[u]); }
                if (flags & CLF_BATTERY) CLPFC_TERM(CLPF_D_SOC, S.soc)
                if (flags & CLF_COOL_STO) CLPFC_TERM(CLPF_D_CS, S.cs)
                if (flags & CLF_HEAT_STO) CLPFC_TERM(CLPF_D_HS, S.hs)
                if (flags & CLF_DHW_STO) CLPFC_TERM(CLPF_D_DS, S.ds)
                CLPFC_TERM(CLPF_D_NET, last_net)
#undef CLPFC_TERM
#pragma unroll
                for (int u = 0; u < 4; ++u) z[u] = clpol_unit(z[u]);
#define CLPFC_HEAD(h, acc) { const clpol_f4 wo = *reinterpret_cast<const clpol_f4*>(grp + 4 * (CLPF_ND + (h))); \
                             _Pragma("unroll") for (int u = 0; u < 4; ++u) acc = clv::vfma((F)(wo[u]), z[u], acc); }
                if (c_es >= 0) CLPFC_HEAD(CLPF_A_ES, acc_es)
                if (c_cs >= 0) CLPFC_HEAD(CLPF_A_CS, acc_cs)
                if (c_hs >= 0) CLPFC_HEAD(CLPF_A_HS, acc_hs)
                if (c_ds >= 0) CLPFC_HEAD(CLPF_A_DS, acc_ds)
#undef CLPFC_HEAD
            }
#pragma unroll 1
            for (int h = 0; h < CLPF_NA; ++h) {
                const int col = h == CLPF_A_ES ? c_es : h == CLPF_A_CS ? c_cs : h == CLPF_A_HS ? c_hs : c_ds;
                if (col < 0) continue;                                   // wave-uniform
                const clpol_f4 hp = *reinterpret_cast<const clpol_f4*>(row + CLPF_HEADS + 8 * h);      // bias, mid, half, sigma
                const float lo = row[CLPF_HEADS + 8 * h + 4], hi = row[CLPF_HEADS + 8 * h + 5];
                const F acc = h == CLPF_A_ES ? acc_es : h == CLPF_A_CS ? acc_cs : h == CLPF_A_HS ? acc_hs : acc_ds;
                float v[VEC];
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    float s;
                    if constexpr (VEC == 1) s = acc; else s = acc[i];
                    v[i] = fmaf(hp[2], tanhf(s + hp[0]), hp[1]);
                }
                // (through a float local: cl_rollout_full_policy_kernel's note on __builtin_bit_cast of a vector element)
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

        // ---- the packed thermal unit exactly as in cl_rollout_full_kernel (its note on the per-step re-read of the parameter block) ----
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
            clv::Ou<F> O;
            const bool first = quirk && t == 0;
            if (R.outage) clv::unit_step<F, true, false, PREC>(B, R, t, first, act, S, O, gz);
            else clv::unit_step<F, false, false, PREC>(B, R, t, first, act, S, O, gz);
            const F rw = clv::unit_reward<F>(rkind, B, S, O.net);
            last_net = O.net; last_rw = rw;
            full_accumulate<VEC>(q_net, O.net); full_accumulate<VEC>(q_cost, O.cost); full_accumulate<VEC>(q_em, O.emission); full_accumulate<VEC>(q_rw, rw);
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
            full_store<VEC, false>(tr + (long long)CLPF_T_REWARD * plane, last_rw);
        }
#pragma unroll
        for (int i = 0; i < VEC; ++i) ret[i] += q_rw[i];
    }

    // ---- write back: carried state, the last step's per-building outputs, this chunk's partial district sums and its share of the return ----
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
        }
    }
    // (n_chunks > 1: the sums of the workgroup's waves go to scratch row (blockIdx.y, quantity) of the reserved plane; cl_finish_kernel adds the chunks)
    if (r.k_steps > 0) district_reduce<VEC>(a, lds, w, lane, env0, live, plane, rkind, q_net, q_cost, q_em, q_rw, a.nw);
    if (r.ret_env) {
        __syncthreads();
        vstore<VEC>(lds + (size_t)w * TILE + lane * VEC, ret);
        __syncthreads();
        // this workgroup row's share of the return: its scratch row behind the n_chunks x NQ partial sums (cl_rollout_full_kernel<CHUNK>'s)
        for (int e = threadIdx.x; e < TILE; e += blockDim.x) {
            float s = 0.0f;
            for (int kk = 0; kk < a.nw; ++kk) s += lds[(size_t)kk * TILE + e];
            if (tile_env0 + e < a.n_env)
                a.out_bldg[(long long)CLO_RESERVED * plane + ((long long)a.n_chunks * NQ + blockIdx.y) * a.n_env + tile_env0 + e] = s;
        }
    }
}

}  // namespace
#endif  // __HIPCC__
