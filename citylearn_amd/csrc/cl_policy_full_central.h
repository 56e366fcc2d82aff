// cl_policy_full_central.h -- the THERMAL K-step loop of cl_rollout_full_policy_kernel (cl_policy_full.h: the packed unit clv::unit_step in registers
// for K steps, one building per wave) under a CENTRAL-AGENT policy: one tanh MLP over the district's observation vector returns every building's
// storage actions, up to four heads per building.  ONE kernel template, cl_rollout_full_policy_central_kernel<PREC, MARL, DEEP>, for the policy
// with one hidden layer (DEEP = false) and for the one of the shape of a SAC / PPO actor trained with central_agent=True on the 2020 / 2021
// schemas, with two (DEEP = true):
//     h1_j   = tanh(pre[s][r][j] + sum_b sum_d dep[s][j / 4][b][d][j % 4] x_d[b])                      j < H   (b ascending, d in CLPF_D_* order)
//     h2_i   = tanh(l2[s][H][i] + sum_j l2[s][j][i] h1_j)                                              i < H2  (j ascending; DEEP only)
//     mean_a = mid_a + half_a tanh(out[s][b][a][HO] + sum_i out[s][b][a][i] h_i)                       a over the heads (es, cs, hs, ds) of building b,
//              over the last hidden layer h: h1 at width HO = H, or h2 at width HO = H2
//     act_a  = clamp(mean_a + sigma_a z_a, low_a, high_a)
// Included by cl_policy_full_central.hip (DEEP = false: libcitylearn_amd_policy_full_central.so, include/citylearn_amd_policy_full_central.h) and by
// cl_policy_full_central_deep.hip (DEEP = true: libcitylearn_amd_policy_full_central_deep.so, include/citylearn_amd_policy_full_central_deep.h),
// each behind cl_kernels.hip's helpers and cl_policy_common.h; each unit instantiates its own variant only and keeps the kernarg layout it had
// (PolicyArgs, or PolicyArgs + l2 + n_hidden2).  What only the second layer needs sits under `if constexpr (DEEP)`, as in cl_policy_central.h, so
// each instantiation is the code of the kernel it was when the two were separate sources (profiles/policy_full_central_one_source_isa.md).  The
// geometry is the thermal policy kernel's: ONE building per wave (nw == n_bldg <= 16), lane = env, one env per lane only; the prologue, the packed
// unit with its outage branch and per-step parameter re-read, the record, the write-back, district_reduce and the return rows are
// cl_rollout_full_policy_kernel's statements written out again (as functions they change the generated code, profiles/policy_refactor_isa.md; one
// template source with cl_policy_full.h, profiles/policy_one_source_isa.md, is not attempted), the hidden phases are
// cl_rollout_policy_central_kernel's (cl_policy_central.h), the first over five terms instead of two, the second statement for statement:
//   publish   (prologue, then the end of every action phase) every wave writes its building's soc, cs, hs, ds and previous net into
//             X[5][n_bldg][64]; 0 where the building has no such storage -- the values the record's planes CLPF_T_SOC + d / CLPF_T_NET hold.
//   hidden 1  the H units are dealt to the waves in groups of four, group g to wave g mod nw.  The owner walks the buildings in ascending order
//             and per building the five terms in CLPF_D_* order with ONE fused-multiply-add chain per unit starting from 0, and writes
//             h = clpol_unit(pre + z) to Hh[H][64]: `pre` enters LAST (cl_policy_central.h's header: 4.4 x against inside the gate).
//   barrier A (Hh complete, every read of X done)
//   hidden 2  (DEEP) the H2 units dealt to the waves the same way.  The owner of group g walks j = 0 .. H - 1 ascending with four chains from 0:
//             per j ONE ds_read_b32 of Hh[j][lane] and ONE ds_read_b128 of the staged l2[j][4 g .. 4 g + 3], the same address in every lane -- a
//             broadcast, no bank conflict.  The bias row l2[H] is added last, then clpol_unit, into Hh2[H2][64].  One H x H2 product per ENV
//             (not per building): exact fp32, no matrix-core family.
//   barrier A2 (DEEP: Hh2 complete, every read of Hh done)
//   action    every wave, for its own building: the heads it has over the last hidden layer at width HO -- i ascending from 0, the bias last --,
//             then tanhf, noise and clamp in cl_policy_full.h's single non-unrolled head loop; the packed thermal unit; the record; the five
//             new values into X.
//   barrier B (orders X, Hh and Hh2 for the next step's hidden phases)
// MARL rides on barrier B: the district net of the step is X's net row summed in building order by every lane for its own env -- the order and
// the operands of cl_rollout_full_policy_kernel's exchange row.  ALL waves and ALL lanes execute every barrier of every step: a wave without a
// group in either layer (sixteen buildings at H2 = 4: fifteen of sixteen waves in layer 2), lanes past n_env (they compute on the reset values
// and never store to memory).  No sum that feeds an action depends on nw.
//
// A term a building lacks has weight 0 (the packer) and plane 0 (the publish): fma(0, 0, z) is z, so the owner RUNS all five terms of every
// building instead of branching on another building's flags -- no per-building flag table in the hidden phase, one loop body, the same bits.
//
// Where the K-invariant weights are read from: STAGED LDS, once per launch, as in cl_policy_central.h -- `dep` as it is packed,
// [H / 4][n_bldg][5][4], five broadcast ds_read_b128 per (group, building) next to the five ds_read_b32 of X; `l2` as it is packed,
// [H + 1][H2] (DEEP); each wave's own head row [HO / 4][4 heads][4] + the 4 x 8 head parameters of cl_policy_full.h.  `pre` changes every step:
// four consecutive floats per group through the constant address space.  The building's parameter block is re-read every step exactly as in
// cl_rollout_full_policy_kernel (whose MARL instantiation has two barriers per step as well).
// Decided from the generated code (gfx950, with SLP vectorisation: the translation units' headers), <PREC, MARL> at DEEP = false: <0, false> 70
// VGPRs, <0, true> and <2, false> 106, <2, true> 121; no scratch memory in any; all four number 100 of a wave's 102 scalar registers and keep
// 91 / 29 / 73 / 31 more scalars in VGPR lanes -- cl_rollout_full_policy_kernel's own figures at one env per lane are 60 / 98 / 92 / 113 VGPRs and
// 74 / 25 / 55 / 18 such scalars.  The MARL = false instantiations keep the parameter block on the scalar route with both barriers in the loop
// (52 / 58 s_load, 18 / 48 global_load in the whole kernel, the latter the prologue's state planes and the float64 chain's words); the MARL = true
// ones read it as cl_rollout_full_policy_kernel<1, PREC, true> does (30 s_load, 57 / 75 global_load: 25 - 39 and 61 / 79 there).  Hence MARL
// stays a template parameter -- a run-time branch would hand the MARL form to every reward kind -- and nothing is staged in LDS: no
// instantiation spills.
// At DEEP = true: 80 / 109 / 110 / 125 VGPRs, no scratch memory in any; all four number 100 of a wave's 102 scalar registers and keep 102 / 60 /
// 92 / 61 more scalars in VGPR lanes (distinct v_writelane_b32 destinations).  Without SLP vectorisation 69 / 109 / 110 / 125 and no scratch
// either: the limit of a 1024-thread workgroup (128) does not depend on the flag.  With it the second hidden phase's loop pairs its four chains
// into two v_pk_fma_f32 per j next to one ds_read_b128 of l2 (the reads of Hh[j] merge into ds_read2st64_b32 at the loop's unroll of four).
// Nothing of the phase is live across barrier A2 but the addresses the action phase uses anyway.
//
// LDS per workgroup, in floats (the public headers' formulas, _lib.policy_full_central_lds_bytes / _lib.policy_full_central_deep_lds_bytes):
//     [nw][NQ][64] reduction rows (the return rows alias them) | X [5][n_bldg][64] | Hh [H][64] | Hh2 [H2][64] (DEEP) | dep [H / 4][n_bldg][5][4] |
//     l2 [H + 1][H2] (DEEP) | head rows [nw][CLPFC_ROW]
// At sixteen buildings: 92 160 bytes at 64 units, 125 184 bytes at 64 x 64 (DEEP); above 64 KiB the launch opts in (CL_POLICY_LAUNCH).  Every
// region starts on a multiple of four floats (H, H2 are multiples of four), which the ds_read_b128 of dep, l2 and the head rows need.
#pragma once
#include "cl_policy_common.h"

#ifdef __HIPCC__
namespace {

constexpr int CLPFC_MAX_HIDDEN = 64;                           // CLPFCA_MAX_HIDDEN and CLPFCD_MAX_HIDDEN (each unit asserts its own)
constexpr int CLPFC_HEADS = CLPF_NA * CLPFC_MAX_HIDDEN;         // where the heads' {bias, mid, half, sigma | low, high, -, -} start
constexpr int CLPFC_ROW = CLPFC_HEADS + 8 * CLPF_NA;            // floats of one building's staged head row: [HO / 4][4 heads][4] | 4 x 8

// PolicyArgs (its n_hidden is H1; its `out` rows have H2 + 1 floats) + the second layer
struct CentralDeepFullPolicyArgs {
    PolicyArgs p;
    const float* __restrict__ l2;          // [n_sets][H1 + 1][H2]
    int n_hidden2;
};
// what the kernel takes by value: each variant keeps the kernarg layout it had
template <bool DEEP> using CentralFullPolicyArgs = std::conditional_t<DEEP, CentralDeepFullPolicyArgs, PolicyArgs>;
CL_DEV const PolicyArgs& central_full_policy_args(const PolicyArgs& p) { return p; }
CL_DEV const PolicyArgs& central_full_policy_args(const CentralDeepFullPolicyArgs& d) { return d.p; }
// how the kernel names its PolicyArgs: a copy of the argument (DEEP = false) or a reference into it (DEEP = true).  Per variant because the
// generated code is: a reference costs the DEEP = false instantiations 4 - 7 instructions, a copy changes the DEEP = true ones by 6 - 7
// (profiles/policy_full_central_one_source_isa.md)
template <bool DEEP> using CentralFullPolicyView = std::conditional_t<DEEP, const PolicyArgs&, const PolicyArgs>;

constexpr size_t rollout_full_policy_central_lds_floats(int nw, int n_bldg, int h) {
    return (size_t)nw * NQ * 64 + (size_t)CLPF_ND * n_bldg * 64 + (size_t)h * 64 + (size_t)CLPF_ND * h * n_bldg + (size_t)nw * CLPFC_ROW;
}
constexpr size_t rollout_full_policy_central_deep_lds_floats(int nw, int n_bldg, int h1, int h2) {
    return (size_t)nw * NQ * 64 + (size_t)CLPF_ND * n_bldg * 64 + (size_t)h1 * 64 + (size_t)h2 * 64 + (size_t)CLPF_ND * h1 * n_bldg + (size_t)(h1 + 1) * h2
           + (size_t)nw * CLPFC_ROW;
}

template <int PREC, bool MARL, bool DEEP>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4))) cl_rollout_full_policy_central_kernel(const CentralFullPolicyArgs<DEEP> d) {
    extern __shared__ __attribute__((aligned(16))) float lds[];     // see the header comment
    constexpr int VEC = 1, TILE = 64;
    using F = float;
    CentralFullPolicyView<DEEP> p = central_full_policy_args(d);
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
    const int H = p.n_hidden, NB = a.n_bldg;
    int H2 = 0;                                                     // (DEEP only)
    if constexpr (DEEP) H2 = d.n_hidden2;
    const int HO = DEEP ? H2 : H;                                   // the width of the layer under the heads
    const int blk = tile_env0 / CL_ROW0_BLOCK;
    const int row0 = a.env_row0 ? a.env_row0[blk] : 0;              // workgroup-uniform
    const int set = p.set_of_block ? p.set_of_block[blk] : 0;       // workgroup-uniform
    float* const X = lds + (size_t)a.nw * NQ * TILE;                // [5][NB][64]: soc, cs, hs, ds, previous net
    float* const Hh = X + (size_t)CLPF_ND * NB * TILE;              // [H][64]: hidden layer 1
    float* const Hh2 = Hh + (size_t)H * TILE;                       // [H2][64]: hidden layer 2 (DEEP only: no floats otherwise)
    float* const depl = Hh2 + (size_t)H2 * TILE;                    // [H / 4][NB][5][4]
    float* const l2l = depl + (size_t)CLPF_ND * H * NB;             // [H + 1][H2] (DEEP only)
    float* const row = l2l + (DEEP ? (size_t)(H + 1) * H2 : 0) + (size_t)w * CLPFC_ROW;
    const float* const Ho = DEEP ? Hh2 : Hh;                        // what the heads read

    const uint32_t* __restrict__ f = a.params + (long long)w * CL_NP + CLP_F_FIRST;
    [[maybe_unused]] const uint32_t* __restrict__ grow = PREC == 2 ? a.params + (long long)w * CL_NP : nullptr;
    const uint32_t flags = clv::uword<false>(f, 0);
    const int c_cs = (int)clv::uword<false>(f, 1), c_hs = (int)clv::uword<false>(f, 2), c_ds = (int)clv::uword<false>(f, 3), c_es = (int)clv::uword<false>(f, 4);
    const long long off = (long long)w * a.n_env + env0;
    const F zero = 0.0f, one = 1.0f;
    clv::St<F> S = {zero, one, zero, zero, zero, zero};
    // the previous step's net: what the reset observation shows in front of step 0, what the previous launch (or reset) left otherwise
    F last_net = (r.t0 == 0 && p.net_reset) ? p.net_reset[(long long)row0 * a.n_bldg + w] : 0.0f, last_rw = zero;
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
    // stage `dep` of this workgroup's parameter set as it is packed (all threads; the barrier below orders it)
    {
        const float* __restrict__ src = p.dep + (long long)set * CLPF_ND * H * NB;
        for (int i = threadIdx.x; i < CLPF_ND * H * NB; i += blockDim.x) depl[i] = src[i];
        if constexpr (DEEP) {
            // ... and layer 2, bias row included
            const float* __restrict__ src2 = d.l2 + (long long)set * (H + 1) * H2;
            for (int i = threadIdx.x; i < (H + 1) * H2; i += blockDim.x) l2l[i] = src2[i];
        }
    }
    // publish: what the first step's hidden phase reads of this building
#define CLPFC_PUBLISH() do { \
        float* const xb = X + (size_t)w * TILE + lane; \
        xb[(size_t)CLPF_D_SOC * NB * TILE] = (flags & CLF_BATTERY) ? S.soc : zero; xb[(size_t)CLPF_D_CS * NB * TILE] = (flags & CLF_COOL_STO) ? S.cs : zero; \
        xb[(size_t)CLPF_D_HS * NB * TILE] = (flags & CLF_HEAT_STO) ? S.hs : zero; xb[(size_t)CLPF_D_DS * NB * TILE] = (flags & CLF_DHW_STO) ? S.ds : zero; \
        xb[(size_t)CLPF_D_NET * NB * TILE] = last_net; } while (0)
    CLPFC_PUBLISH();
    // stage the building's step-independent head rows (this wave's own LDS row; the barrier below orders them): lane j fetches unit j of the
    // last hidden layer's four head weights, lane a < 4 head a's bias, bounds and sigma
    {
        const long long sb = (long long)set * a.n_bldg + w;
        if (lane < HO) {
            float* at = row + (lane >> 2) * (4 * CLPF_NA) + (lane & 3);
#pragma unroll
            for (int h = 0; h < CLPF_NA; ++h) at[4 * h] = p.out[(sb * CLPF_NA + h) * (HO + 1) + lane];
        }
        if (lane < CLPF_NA) {
            const int col = lane == CLPF_A_ES ? c_es : lane == CLPF_A_CS ? c_cs : lane == CLPF_A_HS ? c_hs : c_ds;
            float* hp = row + CLPFC_HEADS + 8 * lane;
            const bool has = col >= 0;
            const float lo = has ? r.act_low[col] : 0.0f, hi = has ? r.act_high[col] : 0.0f;
            hp[0] = has ? p.out[(sb * CLPF_NA + lane) * (HO + 1) + HO] : 0.0f;
            hp[1] = 0.5f * (hi + lo); hp[2] = 0.5f * (hi - lo);
            hp[3] = (has && p.sigma) ? p.sigma[col] : 0.0f;
            hp[4] = lo; hp[5] = hi; hp[6] = 0.0f; hp[7] = 0.0f;
        }
    }
    __syncthreads();
    // the `pre` row of this workgroup's parameter set at the first row of its episode window (inside the loop: + t H)
    const float* __restrict__ pre_w = p.pre + ((long long)set * p.n_rows + row0) * H;
    float ret[VEC], q_net[VEC], q_cost[VEC], q_em[VEC], q_rw[VEC];
    ret[0] = 0.0f;

    for (int k = 0; k < r.k_steps; ++k) {
        const int t = r.t0 + k;
        float* const tr = p.traj ? p.traj + (long long)k * CLPF_NT * plane + off : nullptr;
        q_net[0] = q_cost[0] = q_em[0] = q_rw[0] = 0.0f;

        // ---- hidden phase 1: this wave's groups of four units over ALL buildings and terms, in fixed order ----
        {
            const clpol_c4ptr pq = (clpol_c4ptr)(const clpol_f4*)(pre_w + (long long)t * H);
#pragma unroll 1
            for (int g = w; g < (H >> 2); g += a.nw) {                   // wave-uniform
                const clpol_f4 pj = pq[g];
                float p0 = pj[0], p1 = pj[1], p2 = pj[2], p3 = pj[3];
                CL_PIN_V(p0); CL_PIN_V(p1); CL_PIN_V(p2); CL_PIN_V(p3);
                float z0 = 0.0f, z1 = 0.0f, z2 = 0.0f, z3 = 0.0f;
                const float* wg = depl + (size_t)g * NB * (4 * CLPF_ND);
#pragma unroll 1
                for (int b = 0; b < NB; ++b) {
                    const float* xb = X + (size_t)b * TILE + lane;
                    const float* wb = wg + b * (4 * CLPF_ND);
#pragma unroll
                    for (int dd = 0; dd < CLPF_ND; ++dd) {
                        const float x = xb[(size_t)dd * NB * TILE];
                        const clpol_f4 wd = *reinterpret_cast<const clpol_f4*>(wb + 4 * dd);
                        z0 = fmaf(wd[0], x, z0); z1 = fmaf(wd[1], x, z1); z2 = fmaf(wd[2], x, z2); z3 = fmaf(wd[3], x, z3);
                    }
                }
                float* hg = Hh + (size_t)(4 * g) * TILE + lane;
                hg[0 * TILE] = clpol_unit(p0 + z0); hg[1 * TILE] = clpol_unit(p1 + z1);
                hg[2 * TILE] = clpol_unit(p2 + z2); hg[3 * TILE] = clpol_unit(p3 + z3);
            }
        }
        __syncthreads();                                                 // barrier A: Hh complete, every read of X done

        if constexpr (DEEP) {
            // ---- hidden phase 2: this wave's groups of four layer-2 units over ALL layer-1 units, in fixed order (cl_policy_central.h's) ----
#pragma unroll 1
            for (int g = w; g < (H2 >> 2); g += a.nw) {                  // wave-uniform
                float z0 = 0.0f, z1 = 0.0f, z2 = 0.0f, z3 = 0.0f;
                const float* wg = l2l + 4 * g;
                const float* hj = Hh + lane;
#pragma unroll 4
                for (int j = 0; j < H; ++j) {
                    const float h = hj[(size_t)j * TILE];
                    const clpol_f4 wj = *reinterpret_cast<const clpol_f4*>(wg + j * H2);      // the same address in every lane: a broadcast
                    z0 = fmaf(wj[0], h, z0); z1 = fmaf(wj[1], h, z1); z2 = fmaf(wj[2], h, z2); z3 = fmaf(wj[3], h, z3);
                }
                const clpol_f4 bj = *reinterpret_cast<const clpol_f4*>(wg + H * H2);          // the bias row, added last
                float* hg = Hh2 + (size_t)(4 * g) * TILE + lane;
                hg[0 * TILE] = clpol_unit(bj[0] + z0); hg[1 * TILE] = clpol_unit(bj[1] + z1);
                hg[2 * TILE] = clpol_unit(bj[2] + z2); hg[3 * TILE] = clpol_unit(bj[3] + z3);
            }
            __syncthreads();                                             // barrier A2: Hh2 complete, every read of Hh done
        }

        // ---- action phase: this building's heads over the shared (last) hidden layer ----
        clv::Ac<F> act = {zero, zero, zero, zero, zero, zero};
        {
            F acc_es = zero, acc_cs = zero, acc_hs = zero, acc_ds = zero;
#pragma unroll 1
            for (int g = 0; g < HO; g += 4) {
                const float* grp = row + (g >> 2) * (4 * CLPF_NA);
                const float* hg = Ho + (size_t)g * TILE + lane;
                const float h0 = hg[0 * TILE], h1 = hg[1 * TILE], h2 = hg[2 * TILE], h3 = hg[3 * TILE];
#define CLPFC_HEAD(h, acc) { const clpol_f4 wo = *reinterpret_cast<const clpol_f4*>(grp + 4 * (h)); \
                              acc = fmaf(wo[3], h3, fmaf(wo[2], h2, fmaf(wo[1], h1, fmaf(wo[0], h0, acc)))); }
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
                const clpol_f4 hp = *reinterpret_cast<const clpol_f4*>(row + CLPFC_HEADS + 8 * h);      // bias, mid, half, sigma
                const float lo = row[CLPFC_HEADS + 8 * h + 4], hi = row[CLPFC_HEADS + 8 * h + 5];
                const F acc = h == CLPF_A_ES ? acc_es : h == CLPF_A_CS ? acc_cs : h == CLPF_A_HS ? acc_hs : acc_ds;
                float v = fmaf(hp[2], tanhf(acc + hp[0]), hp[1]);
                // (through a float local: __builtin_bit_cast on the vector ELEMENT hp[3] copies from the start of the vector)
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

        // ---- the packed thermal unit exactly as in cl_rollout_full_policy_kernel (cl_rollout_full_kernel's note on the per-step re-read) ----
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
        // publish for the next step's hidden phase (and this step's MARL sum): all waves are past their reads of X (barrier A)
        CLPFC_PUBLISH();
        __syncthreads();                                                 // barrier B: X complete, every read of Hh / Hh2 done
        if constexpr (MARL) {
            // the MARL reward couples the buildings through the district net of THIS step: X's net row, summed in building order
            float dnet = 0.0f;
            const float* xn = X + (size_t)CLPF_D_NET * NB * TILE + lane;
            for (int b = 0; b < NB; ++b) dnet += xn[(size_t)b * TILE];
            last_rw = cl::marl_reward(last_net, dnet);
            ret[0] += last_rw;
            if (tr && live) full_store<VEC, false>(tr + (long long)CLPF_T_REWARD * plane, last_rw);
        } else {
            ret[0] += q_rw[0];
        }
    }
#undef CLPFC_PUBLISH

    // ---- write back: carried state, the last step's per-building outputs, district sums, episode-return partials (cl_rollout_full_policy_kernel's) ----
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
// the struct of a central-agent thermal policy (check_thermal_policy_mlp's counterpart, in its order) and of one with two hidden layers (H1 in
// front of H2 as in check_central_deep_policy_mlp); each where the unit has included the public header that declares the struct, as in
// cl_policy_central.h
#ifdef CITYLEARN_AMD_POLICY_FULL_CENTRAL_H
inline int check_central_thermal_policy_mlp(const char* entry, const cl_dims* dims, const clpfca_mlp* mlp) {
    if (dims->n_act_cols > 65536) return fail(CL_EINVAL, "%s: n_act_cols=%d > 65536", entry, dims->n_act_cols);
    if (!mlp) return fail(CL_ENULL, "mlp is NULL");
    if (mlp->n_device_cols != 0)
        return fail(CL_EINVAL, "%s: n_device_cols=%d: a building with a cooling / heating / combined device action column is not covered "
                               "(the policy has storage heads only)", entry, mlp->n_device_cols);
    if (int rc = check_policy_sizes(*mlp, CLPFCA_MAX_HIDDEN)) return rc;
    if (mlp->reserved) return fail(CL_EINVAL, "clpfca_mlp.reserved must be 0");
    return CL_OK;
}
#endif
#ifdef CITYLEARN_AMD_POLICY_FULL_CENTRAL_DEEP_H
inline int check_central_deep_thermal_policy_mlp(const char* entry, const cl_dims* dims, const clpfcd_mlp* mlp) {
    if (dims->n_act_cols > 65536) return fail(CL_EINVAL, "%s: n_act_cols=%d > 65536", entry, dims->n_act_cols);
    if (!mlp) return fail(CL_ENULL, "mlp is NULL");
    if (mlp->n_device_cols != 0)
        return fail(CL_EINVAL, "%s: n_device_cols=%d: a building with a cooling / heating / combined device action column is not covered "
                               "(the policy has storage heads only)", entry, mlp->n_device_cols);
    if (int rc = check_policy_sizes(*mlp, CLPFCD_MAX_HIDDEN)) return rc;
    if (mlp->n_hidden2 < 4 || mlp->n_hidden2 > CLPFCD_MAX_HIDDEN || mlp->n_hidden2 % 4)
        return fail(CL_EINVAL, "n_hidden2=%d: the deep central thermal policy kernel takes 4, 8, .. %d units in its second hidden layer", mlp->n_hidden2,
                    CLPFCD_MAX_HIDDEN);
    if (mlp->flags || mlp->reserved) return fail(CL_EINVAL, "clpfcd_mlp.flags / .reserved must be 0");
    return CL_OK;
}
#endif

}  // namespace
#endif  // __HIPCC__
