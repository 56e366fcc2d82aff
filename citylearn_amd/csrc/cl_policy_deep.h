// cl_policy_deep.h -- cl_rollout_policy_kernel (cl_policy.h) with a policy of TWO hidden tanh layers: the battery + PV K-step loop whose
// electrical-storage action of every (env, building, step) is
//     h1_j = tanh(pre[s][r][b][j] + dep[s][b][0][j] soc + dep[s][b][1][j] net_prev)                   j < H1   (cl_policy.h's split first layer)
//     h2_i = tanh(l2[s][b][H1][i] + sum_j l2[s][b][j][i] h1_j)                                        i < H2
//     a    = clamp(mid + half tanh(out[s][b][H2] + sum_i out[s][b][i] h2_i) + sigma z, low, high)
// Included by cl_policy_deep.hip (libcitylearn_amd_policy_deep.so, include/citylearn_amd_policy_deep.h) behind cl_kernels.hip's helpers and
// cl_policy_common.h.  The body is cl_rollout_policy_kernel's written out again (as functions the shared pieces change the generated code,
// profiles/policy_refactor_isa.md; one template source with cl_policy.h, profiles/policy_one_source_isa.md, has not been tried): the prologue, the
// Philox cache, the lean unit, the record, the write-back, district_reduce and the return rows are its statements; MARL's exchange is left out
// (the host refuses CLR_MARL: no barrier in this K loop), the row staging and the policy block are this file's.
//
// Layer 2 in exact fp32, lane = env.  The H1 units of layer 1 are produced four at a time, as in cl_policy.h, and each is consumed at once by H2
// fused multiply-adds into the layer-2 sums z2[H2], which live in registers: z2_i = fmaf(l2[j][i], h1_j, z2_i) for j ascending, starting from
// the bias row -- per unit i that is the dot product in fixed j order.  So no h1 vector is kept, and the inner loop's weights are the H2
// CONSECUTIVE floats of row j: the packer hands layer 2 over transposed, scaled by -2 log2 e like `pre` / `dep` (clpol_unit takes the scaled sum).
// H2 is a template parameter of the policy block (eight copies, chosen by a wave-uniform switch): z2 is indexed by constants only and the inner
// loop has no branches.
//
// Where layer 2 is read from: the wave's own staged LDS rows, as broadcast ds_read_b128 per four units -- not the constant address space.  `l2`
// is the same for all K steps, like `dep` / `out`, and cl_policy.h's reason holds: the scalar register file of these kernels is full, and a
// 32-float row through s_load would need 32 more SGPRs in flight per h1 unit.  One building's row:
//     [H1 / 4][ws x 4 | wn x 4] | l2 [H1 + 1][H2] | w3 [H2] | bias, mid, half, sigma, low, high, pad x 2
// = 2 H1 + (H1 + 1) H2 + H2 + 8 floats, 4640 bytes at 32 x 32.  LDS per workgroup: the district reduction's [nw][NQ][tile] rows (the return rows
// alias them) + nw x 2 rows; the host refuses what exceeds the CU's 160 KiB (16 waves at 32 x 32: 164 864 bytes).
//
// Instantiated at one env per lane only: at two, z2 alone is 64 registers of the 128 a 1024-thread workgroup leaves a lane, and the
// instantiation spills to scratch memory (136 bytes) -- dropped, the host refuses cl_tuning.vec = 2.  The second family (MMA = 1, below) runs the
// same layer on the f16 matrix cores; this one is its arithmetic reference and what `matrix_cores=None` picks for small layers (policy.py).
#pragma once
#include "cl_policy_common.h"

#ifdef __HIPCC__
namespace {

constexpr int CLPD_MAX_H = 32;
constexpr int CLPD_TAIL = 8;                          // bias, mid, half, sigma, low, high, pad x 2

// floats of one building's staged row
constexpr int clpd_row_floats(int h1, int h2) { return 2 * h1 + (h1 + 1) * h2 + h2 + CLPD_TAIL; }

struct DeepPolicyArgs {
    PolicyArgs p;                          // p.n_hidden = H1, p.out: [n_sets][n_bldg][H2 + 1]
    const float* __restrict__ l2;          // MMA = 0: [n_sets][n_bldg][H1 + 1][H2];  MMA = 1: [n_sets][n_bldg][CLPD_M_L2]
    int n_hidden2;
};

// ---- MMA = 1: layer 2 on the f16 matrix cores ----
// Z2[32 units x 32 envs] = W2[32 x 32] . H1[32 x 32 envs] as v_mfma_f32_32x32x16_f16 with both operands split into two f16 terms and the three
// partial products i + j <= 1 (cl_lstm.h's LstmSplit<2>, lstm_split and association: smallest terms first), b2 as the C operand of the first
// product; two MFMAs (kk = 0, 1) cover K = 32.  The 64-env tile is evaluated in two passes of 32 envs: in pass p lanes n and n + 32 both hold
// env 32 p + n (one ds_bpermute per input) and k-slot j of lane half hh in MFMA kk IS first-layer unit 16 kk + 8 hh + j, which that lane computes
// itself -- the B operand needs no cross-lane traffic.  The D layout (row = (reg & 3) + 8 (reg >> 2) + 4 hh, column = n) leaves each half with
// sixteen of the h2 units; the two partial w3 . h2 sums meet by one ds_bpermute, and lane l keeps the action of pass l >> 5.  Everything outside
// the policy block stays in the lane = env layout.  H1 / H2 below 32 are zero-padded: a padded unit's sum is 0, its tanh 0, its weights 0.
//
// NO f16 TERM MAY BE SUBNORMAL.  The residual of a value in [-1, 1] is below 2^-12, mostly under f16's smallest normal 2^-14; plain
// residual terms put the action 5e-5 off on the MI355X, which is what flushing them to zero gives (LAB_NOTES 6.16).
// So every term is scaled by a power of two into the normal range and the scale taken out of the fp32 sums:
//     weights   W' = sw W (sw: the power of two that puts the building's largest |W| into [2^13, 2^14), chosen by the packer),
//               A0 = f16(W'), A1 = f16(2^11 (W' - A0))
//     h1        h' = 2^12 h, B0 = f16(h'), B1 = f16(2^11 (h' - B0))
//     sums      main = 2^12 sw b2 + sum A0 B0,   res = sum A1 B0 + sum A0 B1 (C = 0),   z2 = inv (main + 2^-11 res),  inv = 2^-12 / sw
// The packer hands over the bias row already multiplied by 2^12 sw, and inv.  A term is then subnormal only where its value is below 2^-27 of the
// building's largest weight, or |h1| < 2^-26 (tests/policy_deep_util.py `split_sum_bound` has the bound that follows).
// One building's staged row (the same size at every H1, H2):
//     ws [32] | wn [32] | b2' [32] | w3 [32] | bias, mid, half, sigma, low, high, inv, 2^-11 inv | fragments [kk][term][lane][8 x f16]
// The fragments are the A operands in lane order: [lane][j] = term of W'[lane & 31][16 kk + 8 (lane >> 5) + j], W = -2 log2 e W2.
constexpr int CLPD_M_WN = 32, CLPD_M_B2 = 64, CLPD_M_W3 = 96, CLPD_M_TAIL = 128, CLPD_M_FRAG = 136;
constexpr int CLPD_M_FRAG_FLOATS = 2 * 2 * 64 * 4;                                   // 1024
constexpr int CLPD_M_ROW = CLPD_M_FRAG + CLPD_M_FRAG_FLOATS;                         // 1160 floats
constexpr int CLPD_M_L2 = CLPD_M_FRAG_FLOATS + CLPD_MAX_H + 4;                       // the packed table per building: fragments | b2' [32] | inv, pad x 3

// (cl_lstm.h is not part of the policy units: its two vector types and LstmSplit<2>'s lstm_split, restated)
typedef _Float16 clpd_f16x8 __attribute__((ext_vector_type(8)));
typedef float clpd_f32x16 __attribute__((ext_vector_type(16)));

// 2^12 h = t0 + 2^-11 t1 + r with two round-to-nearest-even f16 terms, |r| <= 2^-22 |2^12 h|: both scalings are exact, and so is the residual
CL_DEV void clpd_split(const float (&h)[8], clpd_f16x8 (&t)[2]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float x = h[j] * 4096.0f;
        const _Float16 q = (_Float16)x;
        t[0][j] = q;
        t[1][j] = (_Float16)((x - (float)q) * 2048.0f);
    }
}

CL_DEV float clpd_bperm(int src_lane, float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src_lane * 4, __builtin_bit_cast(int, v)));
}

// both hidden layers and the output sum of one building for this lane's env (the whole wave must be active): returns the argument of the output tanh
CL_DEV float clpd_hidden_mma(const float* row, const float* __restrict__ pre_b, int H1, float soc, float net, int lane) {
    const int n = lane & 31, hh = lane >> 5;
    const clpd_f16x8* const frag = reinterpret_cast<const clpd_f16x8*>(row + CLPD_M_FRAG);      // [kk][term][lane]
    const float bias = row[CLPD_M_TAIL], inv = row[CLPD_M_TAIL + 6], inv_res = row[CLPD_M_TAIL + 7];
    float arg = 0.0f;
#pragma unroll 1
    for (int ps = 0; ps < 2; ++ps) {
        // every staged word below is the same for all K steps and both passes: without this the compiler keeps them all in registers across the
        // K loop (nothing writes LDS inside it) and spills; they are re-read from LDS instead, a few ds_read_b128 per pass
        asm volatile("" ::: "memory");
        const float soc_p = clpd_bperm(32 * ps + n, soc), net_p = clpd_bperm(32 * ps + n, net);
        clpd_f16x8 Bt[2][2];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            float h1[8];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int u0 = 16 * kk + 8 * hh + 4 * c;
                clpol_f4 pj = {0.0f, 0.0f, 0.0f, 0.0f};
                if (u0 < H1) pj = *reinterpret_cast<const clpol_f4*>(pre_b + u0);     // (per lane half: `pre` has H1 floats only)
                const clpol_f4 ws = *reinterpret_cast<const clpol_f4*>(row + u0);
                const clpol_f4 wn = *reinterpret_cast<const clpol_f4*>(row + CLPD_M_WN + u0);
#pragma unroll
                for (int v = 0; v < 4; ++v) h1[4 * c + v] = clpol_unit(fmaf(wn[v], net_p, fmaf(ws[v], soc_p, pj[v])));
            }
            clpd_split(h1, Bt[kk]);
        }
        clpd_f32x16 acc;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const clpol_f4 b = *reinterpret_cast<const clpol_f4*>(row + CLPD_M_B2 + 8 * g + 4 * hh);
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[4 * g + v] = b[v];
        }
        clpd_f32x16 res = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#define CLPD_MMA(C, KK, I, J) C = __builtin_amdgcn_mfma_f32_32x32x16_f16(frag[((KK) * 2 + (I)) * 64 + lane], Bt[KK][J], C, 0, 0, 0);
        CLPD_MMA(res, 0, 1, 0) CLPD_MMA(acc, 0, 0, 0) CLPD_MMA(res, 1, 1, 0) CLPD_MMA(acc, 1, 0, 0) CLPD_MMA(res, 0, 0, 1) CLPD_MMA(res, 1, 0, 1)
#undef CLPD_MMA
        float part = 0.0f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const clpol_f4 wo = *reinterpret_cast<const clpol_f4*>(row + CLPD_M_W3 + 8 * g + 4 * hh);
#pragma unroll
            for (int v = 0; v < 4; ++v) part = fmaf(wo[v], clpol_unit(fmaf(res[4 * g + v], inv_res, acc[4 * g + v] * inv)), part);
        }
        const float z3 = (part + clpd_bperm(lane ^ 32, part)) + bias;                 // (the same value in both halves: the sum commutes)
        arg = hh == ps ? z3 : arg;
    }
    return arg;
}

// The two hidden layers and the output sum of one building for this lane's envs: `row` the building's staged row, `pq` its `pre` row of the step.
// Returns in acc the argument of the output tanh.
template <int H2, int VEC>
CL_DEV void clpd_hidden(const float* row, const clpol_c4ptr pq, int H1, const float (&soc)[VEC], const float (&net)[VEC], float (&acc)[VEC]) {
    const float* const l2 = row + 2 * H1;
    float z2[H2][VEC];
#pragma unroll
    for (int g2 = 0; g2 < H2; g2 += 4) {
        const clpol_f4 b = *reinterpret_cast<const clpol_f4*>(l2 + H1 * H2 + g2);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) z2[g2 + v][i] = b[v];
        }
    }
#pragma unroll 1
    for (int g = 0; g < H1; g += 4) {
        const clpol_f4 pj = pq[g >> 2];
        const clpol_f4 ws = *reinterpret_cast<const clpol_f4*>(row + g * 2);
        const clpol_f4 wn = *reinterpret_cast<const clpol_f4*>(row + g * 2 + 4);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float h1[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) h1[i] = clpol_unit(fmaf(wn[u], net[i], fmaf(ws[u], soc[i], pj[u])));
            const float* const wr = l2 + (g + u) * H2;
#pragma unroll
            for (int g2 = 0; g2 < H2; g2 += 4) {
                const clpol_f4 wv = *reinterpret_cast<const clpol_f4*>(wr + g2);
#pragma unroll
                for (int v = 0; v < 4; ++v) {
#pragma unroll
                    for (int i = 0; i < VEC; ++i) z2[g2 + v][i] = fmaf(wv[v], h1[i], z2[g2 + v][i]);
                }
            }
        }
    }
    const float* const w3 = l2 + (H1 + 1) * H2;
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = w3[H2];
#pragma unroll
    for (int g2 = 0; g2 < H2; g2 += 4) {
        const clpol_f4 wo = *reinterpret_cast<const clpol_f4*>(w3 + g2);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = fmaf(wo[v], clpol_unit(z2[g2 + v][i]), acc[i]);
        }
    }
}

template <int VEC, int PREC, int MMA>
__global__ void __launch_bounds__(1024) cl_rollout_policy_deep_kernel(const DeepPolicyArgs d) {
    static_assert(!MMA || VEC == 1, "the matrix-core policy block maps lane = env");
    extern __shared__ __attribute__((aligned(16))) float lds[];     // [nw][NQ][64*VEC] | [nw][2][clpd_row_floats(H1, H2) | CLPD_M_ROW]
    constexpr int MB = 2, TILE = 64 * VEC;
    const PolicyArgs& p = d.p;
    const RolloutArgs& r = p.r;
    const StepArgs& a = r.s;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile_env0 = blockIdx.x * TILE;
    const int env0 = tile_env0 + lane * VEC;
    const bool live = env0 < a.n_env;
    const long long plane = (long long)a.n_bldg * a.n_env;         // (no row pitch: host)
    const int rkind = (a.flags & CLD_REWARD_MASK) >> CLD_REWARD_SHIFT;
    const bool quirk = a.flags & CLD_REF_T0_QUIRK;
    const int H = p.n_hidden, H2 = d.n_hidden2;
    const int ROWF = MMA ? CLPD_M_ROW : clpd_row_floats(H, H2), TAIL = MMA ? CLPD_M_TAIL : ROWF - CLPD_TAIL;
    const int blk = tile_env0 / CL_ROW0_BLOCK;
    const int row0 = a.env_row0 ? a.env_row0[blk] : 0;              // workgroup-uniform
    const int set = p.set_of_block ? p.set_of_block[blk] : 0;       // workgroup-uniform
    float* const pol = lds + (size_t)a.nw * NQ * TILE + (size_t)w * MB * ROWF;

    const float* __restrict__ ts_w = a.ts + (long long)w * CL_NF;
    // the `pre` rows of this wave's first building in this workgroup's parameter set and episode window (inside the loop: + (t n_bldg + m nw) H)
    const float* __restrict__ pre_w = p.pre + (((long long)set * p.n_rows + row0) * a.n_bldg + w) * H;
    cl::Bp B[MB];
    cl::State St[MB][VEC];
    bool own[MB];
    long long off[MB];
    float last_net[MB][VEC], last_rw[MB][VEC];
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        const int b = w + m * a.nw;
        own[m] = b < a.n_bldg;
        const int bc = own[m] ? b : w;
        off[m] = (long long)bc * a.n_env + env0;
        cl::load_bp<false>(B[m], a.params + (long long)bc * CL_NP);
        // the previous step's net: what the reset observation shows in front of step 0, what the previous launch (or reset) left otherwise
        const float net0 = (r.t0 == 0 && p.net_reset) ? p.net_reset[(long long)row0 * a.n_bldg + bc] : 0.0f;
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            St[m][i] = {0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            last_net[m][i] = net0; last_rw[m][i] = 0.0f;
        }
        if (live && own[m]) {
            float v[VEC];
#define CL_GET(dst, base, plane_id)                                    \
    vload<VEC>(v, base + (long long)(plane_id) * plane + off[m]);      \
    _Pragma("unroll") for (int i = 0; i < VEC; ++i) dst = v[i];
            CL_GET(St[m][i].soc, a.state, CLS_B_SOC) CL_GET(St[m][i].eff, a.state, CLS_B_EFF) CL_GET(St[m][i].degcap, a.state, CLS_B_DEGCAP)
            if (r.t0 != 0) { CL_GET(last_net[m][i], a.out_bldg, CLO_NET) }
#undef CL_GET
        }
        // stage the building's step-independent policy rows (this wave's own LDS rows; the barrier below orders them)
        if (own[m] && B[m].a_es >= 0) {
            float* row = pol + m * ROWF;
            const long long sb = (long long)set * a.n_bldg + bc;
            if constexpr (MMA) {
                if (lane < CLPD_MAX_H) {                                 // zero-padded to 32 units
                    row[lane] = lane < H ? p.dep[(sb * 2 + 0) * H + lane] : 0.0f;
                    row[CLPD_M_WN + lane] = lane < H ? p.dep[(sb * 2 + 1) * H + lane] : 0.0f;
                    row[CLPD_M_B2 + lane] = d.l2[sb * CLPD_M_L2 + CLPD_M_FRAG_FLOATS + lane];
                    row[CLPD_M_W3 + lane] = lane < H2 ? p.out[sb * (H2 + 1) + lane] : 0.0f;
                }
                for (int i = lane; i < CLPD_M_FRAG_FLOATS; i += 64) row[CLPD_M_FRAG + i] = d.l2[sb * CLPD_M_L2 + i];
            } else {
                if (lane < H) {
                    const int at = (lane >> 2) * 8 + (lane & 3);
                    row[at] = p.dep[(sb * 2 + 0) * H + lane];
                    row[at + 4] = p.dep[(sb * 2 + 1) * H + lane];
                }
                const int n2 = (H + 1) * H2;
                for (int i = lane; i < n2; i += 64) row[2 * H + i] = d.l2[sb * n2 + i];
                if (lane < H2) row[2 * H + n2 + lane] = p.out[sb * (H2 + 1) + lane];
            }
            if constexpr (MMA) {
                if (lane == 1) {
                    const float inv = d.l2[sb * CLPD_M_L2 + CLPD_M_FRAG_FLOATS + CLPD_MAX_H];
                    row[TAIL + 6] = inv;
                    row[TAIL + 7] = inv * 0x1p-11f;
                }
            }
            if (lane == 0) {
                const float lo = r.act_low[B[m].a_es], hi = r.act_high[B[m].a_es];
                row[TAIL + 0] = p.out[sb * (H2 + 1) + H2];
                row[TAIL + 1] = 0.5f * (hi + lo);
                row[TAIL + 2] = 0.5f * (hi - lo);
                row[TAIL + 3] = p.sigma ? p.sigma[B[m].a_es] : 0.0f;
                row[TAIL + 4] = lo;
                row[TAIL + 5] = hi;
            }
        }
    }
    __syncthreads();
    cl::BattP Bv[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        Bv[m] = B[m].batt;
        // the curve parameters pinned in VGPRs for all K steps (cl_rollout_kernel's PIN) -- not at two envs per lane on the fp32 map, where the
        // loop's registers leave no room for them under a 1024-thread workgroup's 128 (cl_rollout_kpi_kernel's note)
        // -- and not in the matrix-core family, whose accumulator, fragments and split operands need the room
        if constexpr ((VEC == 2 && PREC == 0) || MMA) continue;
        CL_PIN_V(Bv[m].cpc_a0); CL_PIN_V(Bv[m].cpc_b0); CL_PIN_V(Bv[m].cpc_a1); CL_PIN_V(Bv[m].cpc_b1);
        CL_PIN_V(Bv[m].pec_a0); CL_PIN_V(Bv[m].pec_b0); CL_PIN_V(Bv[m].pec_a1); CL_PIN_V(Bv[m].pec_b1);
        CL_PIN_V(Bv[m].pec_a2); CL_PIN_V(Bv[m].pec_b2); CL_PIN_V(Bv[m].pec_a3); CL_PIN_V(Bv[m].pec_b3);
    }
    float ret[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) ret[i] = 0.0f;
    float q_net[VEC], q_cost[VEC], q_em[VEC], q_rw[VEC];
    PhiloxCache rnd[MB][VEC];

    for (int k = 0; k < r.k_steps; ++k) {
        const int t = r.t0 + k;
        float* const tr = p.traj ? p.traj + (long long)k * CLPOL_NT * plane : nullptr;
#pragma unroll
        for (int i = 0; i < VEC; ++i) q_net[i] = q_cost[i] = q_em[i] = q_rw[i] = 0.0f;
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            if (!own[m]) continue;                                       // wave-uniform
            cl::Row R;
            const cl_cptr q = as_const(ts_w + ((long long)(t + row0) * a.n_bldg + m * a.nw) * CL_NF);
            R.nsl = cw(q, CLT_NSL); R.sol = cw(q, CLT_SOLAR); R.price = cw(q, CLT_PRICE); R.carbon = cw(q, CLT_CARBON);

            // ---- the policy: this building's storage action from (table row, soc, previous net) through both hidden layers ----
            float a_es[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) a_es[i] = 0.0f;
            if (B[m].a_es >= 0) {
                const float* row = pol + m * ROWF;
                const clpol_c4ptr pq = (clpol_c4ptr)(const clpol_f4*)(pre_w + ((long long)t * a.n_bldg + m * a.nw) * H);
                float acc[VEC], socs0[VEC];
#pragma unroll
                for (int i = 0; i < VEC; ++i) socs0[i] = St[m][i].soc;
                if constexpr (MMA) {
                    acc[0] = clpd_hidden_mma(row, pre_w + ((long long)t * a.n_bldg + m * a.nw) * H, H, socs0[0], last_net[m][0], lane);
                } else switch (H2 >> 2) {                                // wave-uniform
                case 1: clpd_hidden<4, VEC>(row, pq, H, socs0, last_net[m], acc); break;
                case 2: clpd_hidden<8, VEC>(row, pq, H, socs0, last_net[m], acc); break;
                case 3: clpd_hidden<12, VEC>(row, pq, H, socs0, last_net[m], acc); break;
                case 4: clpd_hidden<16, VEC>(row, pq, H, socs0, last_net[m], acc); break;
                case 5: clpd_hidden<20, VEC>(row, pq, H, socs0, last_net[m], acc); break;
                case 6: clpd_hidden<24, VEC>(row, pq, H, socs0, last_net[m], acc); break;
                case 7: clpd_hidden<28, VEC>(row, pq, H, socs0, last_net[m], acc); break;
                default: clpd_hidden<32, VEC>(row, pq, H, socs0, last_net[m], acc); break;
                }
                const float mid = row[TAIL + 1], half = row[TAIL + 2], lo = row[TAIL + 4], hi = row[TAIL + 5];
                const float sg = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, row[TAIL + 3])));
#pragma unroll
                for (int i = 0; i < VEC; ++i) a_es[i] = fmaf(half, tanhf(acc[i]), mid);
                if (sg != 0.0f) {                                        // wave-uniform
                    // Box-Muller on two draws of the column's stream: counters 2t and 2t + 1 = words (0, 1) or (2, 3) of block t >> 1
                    if (k == 0 || (t & 1) == 0) {
#pragma unroll
                        for (int i = 0; i < VEC; ++i) {
                            const cl::U4 bk = cl::philox_block(r.seed, (uint32_t)(env0 + i) + a.env_offset, (uint32_t)B[m].a_es, (uint32_t)t >> 1);
                            rnd[m][i].w0 = bk.w[0]; rnd[m][i].w1 = bk.w[1]; rnd[m][i].w2 = bk.w[2]; rnd[m][i].w3 = bk.w[3];
                        }
                    }
#pragma unroll
                    for (int i = 0; i < VEC; ++i) {
                        a_es[i] = fmaf(sg, clpol_gauss(rnd[m][i].w0, rnd[m][i].w1, rnd[m][i].w2, rnd[m][i].w3, t), a_es[i]);
                    }
                }
#pragma unroll
                for (int i = 0; i < VEC; ++i) a_es[i] = fminf(fmaxf(a_es[i], lo), hi);
            }

            // ---- the lean unit exactly as in cl_rollout_kernel ----
            const bool first = quirk && t == 0;
            float c_ns = first ? 3.0f * R.nsl : R.nsl, sol = R.sol;
            const float cbk = first ? 2.0f : 1.0f;
            if constexpr (VEC > 1) { CL_PIN_V(c_ns); CL_PIN_V(sol); }
            const bool batt = B[m].flags & CLF_BATTERY;
            float nets[VEC], socs[VEC], rws[VEC];
            [[maybe_unused]] cl::BattC bc;
            if constexpr (PREC == 2) {
                if (batt) load_battc_const(bc, as_const(B[m].p));       // (scalar loads every step, as in cl_rollout_kernel)
            }
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                float eb = 0.0f;
                if constexpr (PREC == 2) {
                    if (batt) eb = cl::battery_charge_chain(bc, a_es[i], INFINITY, St[m][i]);
                } else if (batt) eb = cl::battery_energy(Bv[m], a_es[i] * Bv[m].pdt, St[m][i]);
                nets[i] = fmaf(c_ns + cbk * eb, B[m].r, sol);
                socs[i] = St[m][i].soc;
            }
            cl::lean_rewards<VEC>(rkind, B[m], socs, nets, rws);
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                last_net[m][i] = nets[i]; last_rw[m][i] = rws[i];
                q_net[i] += nets[i]; q_cost[i] += cl::mul_rn(nets[i], R.price); q_em[i] += fmaxf(0.0f, nets[i] * R.carbon); q_rw[i] += rws[i];
            }
            if (tr && live) {
                float* const tb = tr + off[m];
                vstore<VEC>(tb + (long long)CLPOL_T_ACTION * plane, a_es);
                vstore<VEC>(tb + (long long)CLPOL_T_NET * plane, nets);
                vstore<VEC>(tb + (long long)CLPOL_T_SOC * plane, socs);
                vstore<VEC>(tb + (long long)CLPOL_T_REWARD * plane, rws);
            }
        }
#pragma unroll
        for (int i = 0; i < VEC; ++i) ret[i] += q_rw[i];
    }

    // ---- write back: carried state, the last step's per-building outputs, district sums, episode-return partials (cl_rollout_kernel's) ----
    if (live) {
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            if (!own[m]) continue;
            float v[VEC];
#define CL_PUT(base, plane_id, expr)                                   \
    _Pragma("unroll") for (int i = 0; i < VEC; ++i) v[i] = (expr);      \
    vstore<VEC>(base + (long long)(plane_id) * plane + off[m], v);
            if (B[m].flags & CLF_BATTERY) {
                CL_PUT(a.state, CLS_B_SOC, St[m][i].soc) CL_PUT(a.state, CLS_B_EFF, St[m][i].eff) CL_PUT(a.state, CLS_B_DEGCAP, St[m][i].degcap)
            }
            if (r.k_steps > 0) {
                CL_PUT(a.out_bldg, CLO_NET, last_net[m][i])
                CL_PUT(a.out_bldg, CLO_REWARD, last_rw[m][i])
            }
#undef CL_PUT
        }
    }
    if (r.k_steps > 0) {
        // district sums of the last step
        district_reduce<VEC>(a, lds, w, lane, env0, live, plane, rkind, q_net, q_cost, q_em, q_rw, a.nw);
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
constexpr size_t rollout_policy_deep_lds_floats(int nw, int tile, int h1, int h2, bool mma) {
    return (size_t)nw * NQ * tile + (size_t)nw * 2 * (mma ? CLPD_M_ROW : clpd_row_floats(h1, h2));
}

// the struct of a deep battery + PV policy (check_lean_policy_mlp's counterpart)
inline int check_deep_policy_mlp(const clpd_mlp* mlp) {
    if (!mlp) return fail(CL_ENULL, "mlp is NULL");
    if (int rc = check_policy_sizes(*mlp, CLPD_MAX_HIDDEN)) return rc;
    if (mlp->n_hidden2 < 4 || mlp->n_hidden2 > CLPD_MAX_HIDDEN || mlp->n_hidden2 % 4)
        return fail(CL_EINVAL, "n_hidden2=%d: the deep policy kernel takes 4, 8, .. %d units in its second hidden layer", mlp->n_hidden2, CLPD_MAX_HIDDEN);
    if ((mlp->flags & ~CLPD_MATRIX_CORES) || mlp->reserved || mlp->reserved2)
        return fail(CL_EINVAL, "clpd_mlp.flags takes CLPD_MATRIX_CORES only, .reserved / .reserved2 must be 0");
    return CL_OK;
}

// The geometry: two buildings per wave as cl_rollout_policy_kernel (lean_policy_geometry's nw rule), ONE env per lane
inline int deep_policy_geometry(const cl_dims* dims, const cl_tuning& tun, int& nw, int& vec) {
    nw = tun.nw ? tun.nw : (dims->n_bldg + 1) / 2;
    // (nw > n_bldg: a wave without any building would read its parameter row -- row `w` -- past the end of the table)
    if (nw * 2 < dims->n_bldg || nw < 1 || nw > 16 || nw > dims->n_bldg) return fail(CL_EINVAL, "bad nw %d", nw);
    vec = 1;
    return one_env_per_lane_only(tun, "deep policy");
}

}  // namespace
#endif  // __HIPCC__
