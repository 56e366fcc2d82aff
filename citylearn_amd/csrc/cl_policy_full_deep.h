// cl_policy_full_deep.h -- cl_rollout_full_policy_kernel<1, PREC, MARL> (cl_policy_full.h) with a policy of TWO hidden tanh layers: the thermal K-step
// loop whose storage actions of every (env, building, step) are
//     h1_j   = tanh(pre[s][r][b][j] + sum_d dep[s][b][d][j] x_d)                             j < H1, x = (soc, cs, hs, ds, net_prev)
//     h2_i   = tanh(l2[s][b][H1][i] + sum_j l2[s][b][j][i] h1_j)                             i < H2
//     act_a  = clamp(mid_a + half_a tanh(out[s][b][a][H2] + sum_i out[s][b][a][i] h2_i) + sigma_a z_a, low_a, high_a)      a over the heads (es, cs, hs, ds)
// Included by cl_policy_full_deep.hip only (libcitylearn_amd_policy_full_deep.so, include/citylearn_amd_policy_full_deep.h) behind cl_kernels.hip's
// helpers and cl_policy_common.h.  One env per lane, one building per wave (host: nw == n_bldg <= 16).  Everything outside the policy block is
// cl_rollout_full_policy_kernel<1, PREC, MARL>'s statements written out again (as functions they change the generated code,
// profiles/policy_refactor_isa.md; one template source with cl_policy_full.h, profiles/policy_one_source_isa.md, is not attempted): the prologue, the
// packed unit with its outage branch, the record, MARL's exchange, the write-back, district_reduce and the return rows; the row staging and the
// policy block are this file's.  The policy block runs BEFORE the unit step, so its registers are free again when unit_step starts.
//
// MMA = 0, layer 2 in exact fp32 (cl_policy_deep.h's scheme with cl_policy_full.h's terms and heads).  The H1 units of layer 1 are produced four
// at a time, each of the five terms behind the building's wave-uniform CLF_* branch, and each unit is consumed at once by H2 fused multiply-adds
// into z2[H2] in registers -- z2_i = fmaf(l2[j][i], h1_j, z2_i), bias row first, j ascending -- from the wave's own staged LDS row as broadcast
// ds_read_b128.  H2 is a template parameter of the block behind a wave-uniform switch.  Then h2_i = clpol_unit(z2_i) once, in place, and up to
// four head sums over it, each behind its scalar c_* >= 0 branch.  One building's row:
//     [H1 / 4][5 terms x 4] | l2 [H1 + 1][H2] | w3 [4][H2] | 4 x {bias, mid, half, sigma, low, high, -, -}
// = 5 H1 + (H1 + 1) H2 + 4 H2 + 32 floats, 5504 bytes at 32 x 32.
//
// MMA = 1, layer 2 on the f16 matrix cores: clpd_hidden_mma's scheme (cl_policy_deep.h has the layouts, the scaled two-term splits and why no
// f16 term may be subnormal; the scales here are its scales, the packed table its table).  Two passes of 32 envs, lanes n and n + 32 on the same
// env -- FIVE ds_bpermute for the inputs -- each lane computes the first-layer units of its own k-slots (all five terms: the weights of a term the
// building lacks are 0), six MFMAs, then up to four partial w3_a . h2 sums, each meeting its other half by one ds_bpermute; lane l keeps pass
// l >> 5.  One building's row, the same size at every H1, H2 and -- by coincidence of 5 x 32 + 32 + 4 x 32 + 32 -- the exact family's at 32 x 32:
//     w [5][32] | b2' [32] | w3 [4][32] | 4 x {bias, mid, half, sigma, low, high, -, -} (head 0's last two: inv, 2^-11 inv) | fragments [1024]
// = 1376 floats.
//
// The heads are finished in cl_policy_full.h's one not-unrolled loop (tanhf, Philox + Box-Muller drawn every step, clamp) in both families.
// LDS per workgroup: the district reduction's [nw][NQ][64] rows (MARL's exchange row and the return rows alias them) + nw rows: 104 448 bytes at
// sixteen buildings and 32 x 32 -- opted in above 64 KiB (CL_POLICY_LAUNCH), below the CU's 160 KiB at every accepted geometry.
#pragma once
#include "cl_policy_common.h"

#ifdef __HIPCC__
namespace {

constexpr int CLPFD_MAX_H = 32;
constexpr int CLPFD_TAILS = 8 * CLPF_NA;                     // 4 x {bias, mid, half, sigma, low, high, -, -}
constexpr int CLPFD_GROUP = 4 * CLPF_ND;                     // floats of one group of four first-layer units: [5 terms][4]

// floats of one building's staged row in the exact-fp32 family
constexpr int clpfd_row_floats(int h1, int h2) { return CLPF_ND * h1 + (h1 + 1) * h2 + CLPF_NA * h2 + CLPFD_TAILS; }

// the matrix-core family's row
constexpr int CLPFD_M_B2 = CLPF_ND * 32, CLPFD_M_W3 = CLPFD_M_B2 + 32, CLPFD_M_TAIL = CLPFD_M_W3 + CLPF_NA * 32, CLPFD_M_FRAG = CLPFD_M_TAIL + CLPFD_TAILS;
constexpr int CLPFD_M_FRAG_FLOATS = 2 * 2 * 64 * 4;                                  // 1024: [kk][term][lane][8 x f16]
constexpr int CLPFD_M_ROW = CLPFD_M_FRAG + CLPFD_M_FRAG_FLOATS;                      // 1376 floats
constexpr int CLPFD_M_L2 = CLPFD_M_FRAG_FLOATS + CLPFD_MAX_H + 4;                    // the packed table per building (cl_policy_deep.h's CLPD_M_L2)
static_assert(CLPFD_M_ROW == clpfd_row_floats(32, 32) && CLPFD_M_FRAG % 4 == 0, "both families' rows at 32 x 32");

constexpr size_t rollout_full_policy_deep_lds_floats(int nw, int h1, int h2, bool mma) {
    return (size_t)nw * NQ * 64 + (size_t)nw * (mma ? CLPFD_M_ROW : clpfd_row_floats(h1, h2));
}

struct DeepFullPolicyArgs {
    PolicyArgs p;                          // p.n_hidden = H1, p.out: [n_sets][n_bldg][CLPF_NA][H2 + 1]
    const float* __restrict__ l2;          // MMA = 0: [n_sets][n_bldg][H1 + 1][H2];  MMA = 1: [n_sets][n_bldg][CLPFD_M_L2]
    int n_hidden2;
};

// what the policy block needs of its building, all wave-uniform
struct DeepFullHeads { uint32_t flags; int c_es, c_cs, c_hs, c_ds; };

// ---- MMA = 0 ----
// Both hidden layers and the four output sums (without their biases) of one building for this lane's env: `row` the building's staged row, `pq`
// its `pre` row of the step.
template <int H2>
CL_DEV void clpfd_hidden(const float* row, const clpol_c4ptr pq, int H1, const DeepFullHeads& hd, float soc, float cs, float hs, float ds, float net,
                         float& acc_es, float& acc_cs, float& acc_hs, float& acc_ds) {
    const float* const l2 = row + CLPF_ND * H1;
    float z2[H2];
#pragma unroll
    for (int g2 = 0; g2 < H2; g2 += 4) {
        const clpol_f4 b = *reinterpret_cast<const clpol_f4*>(l2 + H1 * H2 + g2);
#pragma unroll
        for (int v = 0; v < 4; ++v) z2[g2 + v] = b[v];
    }
#pragma unroll 1
    for (int g = 0; g < H1; g += 4) {
        const float* grp = row + (g >> 2) * CLPFD_GROUP;
        const clpol_f4 pj = pq[g >> 2];
        float z[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) z[u] = pj[u];
#define CLPFD_TERM(d, x) { const clpol_f4 wd = *reinterpret_cast<const clpol_f4*>(grp + 4 * (d)); \
                           _Pragma("unroll") for (int u = 0; u < 4; ++u) z[u] = fmaf(wd[u], x, z[u]); }
        if (hd.flags & CLF_BATTERY) CLPFD_TERM(CLPF_D_SOC, soc)
        if (hd.flags & CLF_COOL_STO) CLPFD_TERM(CLPF_D_CS, cs)
        if (hd.flags & CLF_HEAT_STO) CLPFD_TERM(CLPF_D_HS, hs)
        if (hd.flags & CLF_DHW_STO) CLPFD_TERM(CLPF_D_DS, ds)
        CLPFD_TERM(CLPF_D_NET, net)
#undef CLPFD_TERM
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float h1 = clpol_unit(z[u]);
            const float* const wr = l2 + (g + u) * H2;
#pragma unroll
            for (int g2 = 0; g2 < H2; g2 += 4) {
                const clpol_f4 wv = *reinterpret_cast<const clpol_f4*>(wr + g2);
#pragma unroll
                for (int v = 0; v < 4; ++v) z2[g2 + v] = fmaf(wv[v], h1, z2[g2 + v]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < H2; ++i) z2[i] = clpol_unit(z2[i]);             // h2, once for all heads
    const float* const w3 = l2 + (H1 + 1) * H2;
#define CLPFD_HEAD(h, acc) { _Pragma("unroll") for (int g2 = 0; g2 < H2; g2 += 4) { \
                                 const clpol_f4 wo = *reinterpret_cast<const clpol_f4*>(w3 + (h) * H2 + g2); \
                                 _Pragma("unroll") for (int v = 0; v < 4; ++v) acc = fmaf(wo[v], z2[g2 + v], acc); } }
    if (hd.c_es >= 0) CLPFD_HEAD(CLPF_A_ES, acc_es)
    if (hd.c_cs >= 0) CLPFD_HEAD(CLPF_A_CS, acc_cs)
    if (hd.c_hs >= 0) CLPFD_HEAD(CLPF_A_HS, acc_hs)
    if (hd.c_ds >= 0) CLPFD_HEAD(CLPF_A_DS, acc_ds)
#undef CLPFD_HEAD
}

// ---- MMA = 1 ----
// (cl_lstm.h and cl_policy_deep.h are not part of this unit: the two vector types, the split and the cross-lane read, restated)
typedef _Float16 clpfd_f16x8 __attribute__((ext_vector_type(8)));
typedef float clpfd_f32x16 __attribute__((ext_vector_type(16)));

// 2^12 h = t0 + 2^-11 t1 + r with two round-to-nearest-even f16 terms, |r| <= 2^-22 |2^12 h|: both scalings are exact, and so is the residual
CL_DEV void clpfd_split(const float (&h)[8], clpfd_f16x8 (&t)[2]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float x = h[j] * 4096.0f;
        const _Float16 q = (_Float16)x;
        t[0][j] = q;
        t[1][j] = (_Float16)((x - (float)q) * 2048.0f);
    }
}

CL_DEV float clpfd_bperm(int src_lane, float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src_lane * 4, __builtin_bit_cast(int, v)));
}

// both hidden layers and the four output sums (without their biases) of one building for this lane's env; the whole wave must be active
CL_DEV void clpfd_hidden_mma(const float* row, const float* __restrict__ pre_b, int H1, const DeepFullHeads& hd, float soc, float cs, float hs, float ds,
                             float net, int lane, float& acc_es, float& acc_cs, float& acc_hs, float& acc_ds) {
    const int n = lane & 31, hh = lane >> 5;
    const clpfd_f16x8* const frag = reinterpret_cast<const clpfd_f16x8*>(row + CLPFD_M_FRAG);      // [kk][term][lane]
#pragma unroll 1
    for (int ps = 0; ps < 2; ++ps) {
        // every staged word below is the same for all K steps and both passes: without this the compiler keeps them in registers across the K loop
        // (nothing writes LDS inside it) and spills (cl_policy_deep.h's note); they are re-read from LDS instead, a few ds_read_b128 per pass
        asm volatile("" ::: "memory");
        const float inv = row[CLPFD_M_TAIL + 6], inv_res = row[CLPFD_M_TAIL + 7];
        const int src = 32 * ps + n;
        const float x_p[CLPF_ND] = {clpfd_bperm(src, soc), clpfd_bperm(src, cs), clpfd_bperm(src, hs), clpfd_bperm(src, ds), clpfd_bperm(src, net)};
        clpfd_f16x8 Bt[2][2];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            float h1[8];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int u0 = 16 * kk + 8 * hh + 4 * c;
                clpol_f4 z = {0.0f, 0.0f, 0.0f, 0.0f};
                if (u0 < H1) z = *reinterpret_cast<const clpol_f4*>(pre_b + u0);      // (per lane half: `pre` has H1 floats only)
#pragma unroll
                for (int d = 0; d < CLPF_ND; ++d) {
                    const clpol_f4 wd = *reinterpret_cast<const clpol_f4*>(row + 32 * d + u0);
#pragma unroll
                    for (int v = 0; v < 4; ++v) z[v] = fmaf(wd[v], x_p[d], z[v]);
                }
#pragma unroll
                for (int v = 0; v < 4; ++v) h1[4 * c + v] = clpol_unit(z[v]);
            }
            clpfd_split(h1, Bt[kk]);
        }
        clpfd_f32x16 acc;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const clpol_f4 b = *reinterpret_cast<const clpol_f4*>(row + CLPFD_M_B2 + 8 * g + 4 * hh);
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[4 * g + v] = b[v];
        }
        clpfd_f32x16 res = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#define CLPFD_MMA(C, KK, I, J) C = __builtin_amdgcn_mfma_f32_32x32x16_f16(frag[((KK) * 2 + (I)) * 64 + lane], Bt[KK][J], C, 0, 0, 0);
        CLPFD_MMA(res, 0, 1, 0) CLPFD_MMA(acc, 0, 0, 0) CLPFD_MMA(res, 1, 1, 0) CLPFD_MMA(acc, 1, 0, 0) CLPFD_MMA(res, 0, 0, 1) CLPFD_MMA(res, 1, 0, 1)
#undef CLPFD_MMA
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = clpol_unit(fmaf(res[i], inv_res, acc[i] * inv));      // h2 of this half's sixteen units, once for all heads
        // (the partial sums of the two halves meet by one ds_bpermute: the same value in both halves, the sum commutes)
#define CLPFD_HEAD(h, out) { float part = 0.0f; \
                             _Pragma("unroll") for (int g = 0; g < 4; ++g) { \
                                 const clpol_f4 wo = *reinterpret_cast<const clpol_f4*>(row + CLPFD_M_W3 + 32 * (h) + 8 * g + 4 * hh); \
                                 _Pragma("unroll") for (int v = 0; v < 4; ++v) part = fmaf(wo[v], acc[4 * g + v], part); } \
                             const float z3 = part + clpfd_bperm(lane ^ 32, part); \
                             out = hh == ps ? z3 : out; }
        if (hd.c_es >= 0) CLPFD_HEAD(CLPF_A_ES, acc_es)
        if (hd.c_cs >= 0) CLPFD_HEAD(CLPF_A_CS, acc_cs)
        if (hd.c_hs >= 0) CLPFD_HEAD(CLPF_A_HS, acc_hs)
        if (hd.c_ds >= 0) CLPFD_HEAD(CLPF_A_DS, acc_ds)
#undef CLPFD_HEAD
    }
}

template <int PREC, int MMA, bool MARL>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4))) cl_rollout_full_policy_deep_kernel(const DeepFullPolicyArgs d) {
    extern __shared__ __attribute__((aligned(16))) float lds[];     // [nw][NQ][64] | [nw][clpfd_row_floats(H1, H2) | CLPFD_M_ROW]
    constexpr int VEC = 1, TILE = 64;
    using F = float;
    const PolicyArgs& p = d.p;
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
    const int H = p.n_hidden, H2 = d.n_hidden2;
    const int ROWF = MMA ? CLPFD_M_ROW : clpfd_row_floats(H, H2), TAIL = MMA ? CLPFD_M_TAIL : ROWF - CLPFD_TAILS;
    const int blk = tile_env0 / CL_ROW0_BLOCK;
    const int row0 = a.env_row0 ? a.env_row0[blk] : 0;              // workgroup-uniform
    const int set = p.set_of_block ? p.set_of_block[blk] : 0;       // workgroup-uniform
    float* const row = lds + (size_t)a.nw * NQ * TILE + (size_t)w * ROWF;

    const uint32_t* __restrict__ f = a.params + (long long)w * CL_NP + CLP_F_FIRST;
    [[maybe_unused]] const uint32_t* __restrict__ grow = PREC == 2 ? a.params + (long long)w * CL_NP : nullptr;
    const uint32_t flags = clv::uword<false>(f, 0);
    const int c_cs = (int)clv::uword<false>(f, 1), c_hs = (int)clv::uword<false>(f, 2), c_ds = (int)clv::uword<false>(f, 3), c_es = (int)clv::uword<false>(f, 4);
    const DeepFullHeads hd = {flags, c_es, c_cs, c_hs, c_ds};
    const long long off = (long long)w * a.n_env + env0;
    const F zero = (F)(0.0f), one = (F)(1.0f);
    clv::St<F> S = {zero, one, zero, zero, zero, zero};
    // the previous step's net: what the reset observation shows in front of step 0, what the previous launch (or reset) left otherwise
    F last_net = (F)((r.t0 == 0 && p.net_reset) ? p.net_reset[(long long)row0 * a.n_bldg + w] : 0.0f), last_rw = zero;
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
    // stage the building's step-independent policy rows (this wave's own LDS row; the barrier below orders them)
    {
        const long long sb = (long long)set * a.n_bldg + w;
        if constexpr (MMA) {
            if (lane < CLPFD_MAX_H) {                                    // zero-padded to 32 units
#pragma unroll
                for (int t = 0; t < CLPF_ND; ++t) row[32 * t + lane] = lane < H ? p.dep[(sb * CLPF_ND + t) * H + lane] : 0.0f;
                row[CLPFD_M_B2 + lane] = d.l2[sb * CLPFD_M_L2 + CLPFD_M_FRAG_FLOATS + lane];
#pragma unroll
                for (int h = 0; h < CLPF_NA; ++h) row[CLPFD_M_W3 + 32 * h + lane] = lane < H2 ? p.out[(sb * CLPF_NA + h) * (H2 + 1) + lane] : 0.0f;
            }
            for (int i = lane; i < CLPFD_M_FRAG_FLOATS; i += 64) row[CLPFD_M_FRAG + i] = d.l2[sb * CLPFD_M_L2 + i];
        } else {
            if (lane < H) {
                float* at = row + (lane >> 2) * CLPFD_GROUP + (lane & 3);
#pragma unroll
                for (int t = 0; t < CLPF_ND; ++t) at[4 * t] = p.dep[(sb * CLPF_ND + t) * H + lane];
            }
            const int n2 = (H + 1) * H2;
            for (int i = lane; i < n2; i += 64) row[CLPF_ND * H + i] = d.l2[sb * n2 + i];
            if (lane < H2) {
#pragma unroll
                for (int h = 0; h < CLPF_NA; ++h) row[CLPF_ND * H + n2 + h * H2 + lane] = p.out[(sb * CLPF_NA + h) * (H2 + 1) + lane];
            }
        }
        if (lane < CLPF_NA) {
            const int col = lane == CLPF_A_ES ? c_es : lane == CLPF_A_CS ? c_cs : lane == CLPF_A_HS ? c_hs : c_ds;
            float* hp = row + TAIL + 8 * lane;
            const bool has = col >= 0;
            const float lo = has ? r.act_low[col] : 0.0f, hi = has ? r.act_high[col] : 0.0f;
            hp[0] = has ? p.out[(sb * CLPF_NA + lane) * (H2 + 1) + H2] : 0.0f;
            hp[1] = 0.5f * (hi + lo); hp[2] = 0.5f * (hi - lo);
            hp[3] = (has && p.sigma) ? p.sigma[col] : 0.0f;
            hp[4] = lo; hp[5] = hi;
            float inv = 0.0f;
            if constexpr (MMA) inv = lane == 0 ? d.l2[sb * CLPFD_M_L2 + CLPFD_M_FRAG_FLOATS + CLPFD_MAX_H] : 0.0f;
            hp[6] = inv; hp[7] = inv * 0x1p-11f;
        }
    }
    __syncthreads();
    // the `pre` rows of this wave's building in this workgroup's parameter set and episode window (inside the loop: + t n_bldg H)
    const float* __restrict__ pre_w = p.pre + (((long long)set * p.n_rows + row0) * a.n_bldg + w) * H;
    float ret[VEC], q_net[VEC], q_cost[VEC], q_em[VEC], q_rw[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) ret[i] = 0.0f;

    for (int k = 0; k < r.k_steps; ++k) {
        const int t = r.t0 + k;
        float* const tr = p.traj ? p.traj + (long long)k * CLPF_NT * plane + off : nullptr;
#pragma unroll
        for (int i = 0; i < VEC; ++i) q_net[i] = q_cost[i] = q_em[i] = q_rw[i] = 0.0f;

        // ---- the policy: this building's storage actions from (table row, soc, cs, hs, ds, previous net) through both hidden layers ----
        clv::Ac<F> act = {zero, zero, zero, zero, zero, zero};
        {
            const float* const pre_b = pre_w + (long long)t * a.n_bldg * H;
            float acc_es = 0.0f, acc_cs = 0.0f, acc_hs = 0.0f, acc_ds = 0.0f;
            if constexpr (MMA) {
                clpfd_hidden_mma(row, pre_b, H, hd, S.soc, S.cs, S.hs, S.ds, last_net, lane, acc_es, acc_cs, acc_hs, acc_ds);
            } else {
                const clpol_c4ptr pq = (clpol_c4ptr)(const clpol_f4*)pre_b;
#define CLPFD_CASE(N) clpfd_hidden<N>(row, pq, H, hd, S.soc, S.cs, S.hs, S.ds, last_net, acc_es, acc_cs, acc_hs, acc_ds); break;
                switch (H2 >> 2) {                                       // wave-uniform
                case 1: CLPFD_CASE(4)
                case 2: CLPFD_CASE(8)
                case 3: CLPFD_CASE(12)
                case 4: CLPFD_CASE(16)
                case 5: CLPFD_CASE(20)
                case 6: CLPFD_CASE(24)
                case 7: CLPFD_CASE(28)
                default: CLPFD_CASE(32)
                }
#undef CLPFD_CASE
            }
#pragma unroll 1
            for (int h = 0; h < CLPF_NA; ++h) {
                const int col = h == CLPF_A_ES ? c_es : h == CLPF_A_CS ? c_cs : h == CLPF_A_HS ? c_hs : c_ds;
                if (col < 0) continue;                                   // wave-uniform
                const clpol_f4 hp = *reinterpret_cast<const clpol_f4*>(row + TAIL + 8 * h);      // bias, mid, half, sigma
                const float lo = row[TAIL + 8 * h + 4], hi = row[TAIL + 8 * h + 5];
                const float acc = h == CLPF_A_ES ? acc_es : h == CLPF_A_CS ? acc_cs : h == CLPF_A_HS ? acc_hs : acc_ds;
                float v = fmaf(hp[2], tanhf(acc + hp[0]), hp[1]);
                // (through a float local: __builtin_bit_cast on the vector ELEMENT hp[3] copies from the start of the vector -- cl_policy_full.h)
                const float sg_lane = hp[3];
                const float sg = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, sg_lane)));
                if (sg != 0.0f) {                                        // wave-uniform (no cache: the block is drawn every step)
                    const cl::U4 bk = cl::philox_block(r.seed, (uint32_t)env0 + a.env_offset, (uint32_t)col, (uint32_t)t >> 1);
                    v = fmaf(sg, clpol_gauss(bk.w[0], bk.w[1], bk.w[2], bk.w[3], t), v);
                }
                const F av = fminf(fmaxf(v, lo), hi);
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
            cl::load_row_scalar<true>(R, a.ts + ((long long)(t + row0) * a.n_bldg + w) * CL_NF, B.flags, nullptr);
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
            if constexpr (!MARL) full_store<VEC, false>(tr + (long long)CLPF_T_REWARD * plane, last_rw);
        }
        if constexpr (MARL) {
            // the MARL reward couples the buildings through the district net of THIS step: one LDS exchange per step
            vstore<VEC>(lds + (size_t)w * TILE + lane * VEC, q_net);
            __syncthreads();
            float dnet = 0.0f;
            for (int kk = 0; kk < a.nw; ++kk) {
                float part[VEC];
                vload<VEC>(part, lds + (size_t)kk * TILE + lane * VEC);
                dnet += part[0];
            }
            __syncthreads();
            last_rw = cl::marl_reward(last_net, dnet);
            ret[0] += last_rw;
            if (tr && live) full_store<VEC, false>(tr + (long long)CLPF_T_REWARD * plane, last_rw);
        } else {
            ret[0] += q_rw[0];
        }
    }

    // ---- write back: carried state, the last step's per-building outputs, district sums, episode-return partials (cl_rollout_full_kernel's) ----
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
    if (r.k_steps > 0) {
        if constexpr (MARL) q_rw[0] = last_rw;
        district_reduce<VEC>(a, lds, w, lane, env0, live, plane, MARL ? (int)CLR_DEFAULT : rkind, q_net, q_cost, q_em, q_rw, a.nw);
    }
    if (r.ret_env) {
        __syncthreads();
        vstore<VEC>(lds + (size_t)w * TILE + lane * VEC, ret);
        __syncthreads();
        for (int e = threadIdx.x; e < TILE; e += blockDim.x) {
            float s = 0.0f;
            for (int kk = 0; kk < a.nw; ++kk) s += lds[(size_t)kk * TILE + e];
            if (tile_env0 + e < a.n_env) r.ret_env[tile_env0 + e] += s;
        }
    }
}

// ---- host ----
// the struct of a deep thermal policy (check_thermal_policy_mlp's counterpart for clpfd_mlp, in its order, then the second layer's words)
inline int check_deep_thermal_policy_mlp(const char* entry, const cl_dims* dims, const clpfd_mlp* mlp) {
    if (dims->n_act_cols > 65536) return fail(CL_EINVAL, "%s: n_act_cols=%d > 65536", entry, dims->n_act_cols);
    if (!mlp) return fail(CL_ENULL, "mlp is NULL");
    if (mlp->n_device_cols != 0)
        return fail(CL_EINVAL, "%s: n_device_cols=%d: a building with a cooling / heating / combined device action column is not covered "
                               "(the policy has storage heads only)", entry, mlp->n_device_cols);
    if (int rc = check_policy_sizes(*mlp, CLPFD_MAX_HIDDEN)) return rc;
    if (mlp->n_hidden2 < 4 || mlp->n_hidden2 > CLPFD_MAX_HIDDEN || mlp->n_hidden2 % 4)
        return fail(CL_EINVAL, "n_hidden2=%d: the deep thermal policy kernel takes 4, 8, .. %d units in its second hidden layer", mlp->n_hidden2, CLPFD_MAX_HIDDEN);
    if ((mlp->flags & ~CLPFD_MATRIX_CORES) || mlp->reserved) return fail(CL_EINVAL, "clpfd_mlp.flags takes CLPFD_MATRIX_CORES only, .reserved must be 0");
    return CL_OK;
}

}  // namespace
#endif  // __HIPCC__
