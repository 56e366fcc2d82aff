// cl_policy_central.h -- the battery + PV K-step loop of cl_rollout_policy_kernel (cl_policy.h) under a CENTRAL-AGENT policy: one tanh MLP over the
// district's observation vector returns every building's electrical-storage action.  ONE kernel template, cl_rollout_policy_central_kernel<PREC, DEEP>,
// for the policy with one hidden layer (DEEP = false) and for the one of the shape of a SAC / PPO actor with two (DEEP = true):
//     h1_j = tanh(pre[s][r][j] + sum_b (ws[b][j] soc_b + wn[b][j] net_prev_b))                         j < H   (b ascending, soc then net)
//     h2_i = tanh(l2[s][H][i] + sum_j l2[s][j][i] h1_j)                                                i < H2  (j ascending; DEEP only)
//     a_b  = clamp(mid_b + half_b tanh(out[s][b][HO] + sum_i out[s][b][i] h_i) + sigma_b z, low_b, high_b)   for every building b with a storage column,
//            over the last hidden layer h: h1 at width HO = H, or h2 at width HO = H2
// Included by cl_policy_central.hip (DEEP = false: libcitylearn_amd_policy_central.so, include/citylearn_amd_policy_central.h) and by
// cl_policy_central_deep.hip (DEEP = true: libcitylearn_amd_policy_central_deep.so, include/citylearn_amd_policy_central_deep.h), each behind
// cl_kernels.hip's helpers and cl_policy_common.h; each unit instantiates its own variant only and keeps the kernarg layout it had (PolicyArgs, or
// PolicyArgs + l2 + n_hidden2).  What only the second layer needs sits under `if constexpr (DEEP)`, so each instantiation is the code of the kernel
// it was when the two were separate sources (profiles/policy_one_source_isa.md).  The geometry is the lean kernels': two buildings per wave,
// lane = env, `nw` waves; the prologue, the Philox cache, the lean unit, the record, the write-back, district_reduce and the return rows are
// cl_rollout_policy_kernel's statements written out again (as functions they change the generated code, profiles/policy_refactor_isa.md; one
// template source with cl_policy.h has not been tried).  One env per lane only.
//
// A hidden layer is a sum over ALL buildings (or all units of the layer below), so a step has two or three phases with a workgroup barrier behind each:
//   publish   (prologue, then the end of every action phase) every wave writes its buildings' soc and previous net into X[2][n_bldg][64];
//   hidden 1  the H units are dealt to the waves in groups of four, group g to wave g mod nw.  The owner walks the buildings in ascending order
//             with ONE fused-multiply-add chain per unit -- z = fma(wn, net_b, fma(ws, soc_b, z)) starting from 0 -- and writes
//             h = clpol_unit(pre + z) to Hh[H][64].  The order does not depend on nw: action, net and soc are bit-identical under every cl_tuning.nw.
//   barrier A (Hh complete, every read of X done)
//   hidden 2  (DEEP) the H2 units dealt to the waves the same way.  The owner of group g walks j = 0 .. H - 1 ascending with four chains from 0:
//             per j ONE ds_read_b32 of Hh[j][lane] and ONE ds_read_b128 of l2[j][4 g .. 4 g + 3], the same address in every lane -- a
//             broadcast, no bank conflict.  The bias row l2[H] is added last, then clpol_unit, into Hh2[H2][64].  One product per ENV: 1 / n_bldg
//             of the per-building deep kernel's layer 2 (cl_policy_deep.h), which is why it stays exact fp32 here.
//   barrier A2 (DEEP: Hh2 complete, every read of Hh done)
//   action    every wave, for its own driven buildings: (sum_i out[i] h_i[lane], i ascending from 0) + out[HO], the output tanh, the noise, the clamp;
//             then the lean unit for all its buildings, the record, and the new soc / net into X (all waves are past their reads of X: barrier A).
//   barrier B (orders X, Hh and Hh2 for the next step)
// MARL rides on barrier B: the district net of the step is X's net row summed in building order by every lane for its own env.  No sum that
// feeds an action depends on nw.
// `pre` and every bias enter their sums LAST.  They are an order of magnitude larger than the terms they are added to (a 2 B-term sum of
// single weights times a normalised input; H products of a head weight and a tanh), and a chain that starts from them rounds every partial sum at
// THEIR magnitude: measured on the MI355X with the chains started from pre / the bias, the action lay 4.4 x a float32 torch evaluation's deviation
// from float64 at H = 32 (torch adds its biases behind the matrix products too); in this order it stays inside the project's 4 x gate
// (profiles/policy_central_parity.md).
// ALL waves execute every barrier of every step -- a wave without a hidden group in either layer (b32 at H2 = 4: fifteen of sixteen), a wave
// without a second building, lanes past n_env (they compute on the reset values and never store to memory).
//
// Where the K-invariant weights are read from: STAGED LDS, once per launch -- `dep` as it is packed, [H / 4][n_bldg][ws x 4 | wn x 4], read back as
// two broadcast ds_read_b128 per (group, building) next to the two ds_read_b32 of X; `l2` [H + 1][H2] as it is packed (DEEP); each wave's own
// out rows [2][CLPC_ROW] as in cl_policy.h.
// Decided from the generated code: both DEEP = false instantiations already number 100 of a wave's 102 scalar registers and keep 109 / 129
// more scalars in VGPR lanes (the lean unit's parameters of two buildings fill the file, as in cl_policy.h, whose instantiations keep 83 - 118
// there; 98 / 74 VGPRs, no scratch), and the scalar route -- s_load_dwordx8 per (group, building) through the constant address space -- needs
// eight more per building in flight, sixteen at the loop's unroll of two.  The staged form needs none and its reads queue with X's; for the same
// reason l2 does not go through scalar loads.  The two routes were not timed against each other on the device.
// `pre` changes every step: four consecutive floats per group through the constant address space, as in cl_policy.h.
//
// LDS per workgroup, in floats (the public headers' formulas, _lib.policy_central_lds_bytes / _lib.policy_central_deep_lds_bytes):
//     [nw][NQ][64] reduction rows (the return rows alias them) | X [2][n_bldg][64] | Hh [H][64] | Hh2 [H2][64] (DEEP) | dep [H / 4][n_bldg][8] |
//     l2 [H + 1][H2] (DEEP) | out rows [nw][2][CLPC_ROW]
// At sixteen waves and 32 buildings: 74 752 bytes at 64 units, 107 776 bytes at 64 x 64 (DEEP); above 64 KiB the launch opts in
// (CL_POLICY_LAUNCH).  Every region starts on a multiple of four floats (H, H2 are multiples of four), which the ds_read_b128 of dep, l2 and the
// out rows need.
#pragma once
#include "cl_policy_common.h"

#ifdef __HIPCC__
namespace {

constexpr int CLPC_MAX_HIDDEN = 64;                  // CLPCA_MAX_HIDDEN and CLPCD_MAX_HIDDEN (each unit asserts its own)
constexpr int CLPC_ROW = CLPC_MAX_HIDDEN + 8;        // floats of one building's staged out row: head weights [CLPC_MAX_HIDDEN] | bias, mid, half, sigma, low, high, pad x 2

// PolicyArgs (its n_hidden is H1; its `out` rows have H2 + 1 floats) + the second layer
struct CentralDeepPolicyArgs {
    PolicyArgs p;
    const float* __restrict__ l2;          // [n_sets][H1 + 1][H2]
    int n_hidden2;
};
// what the kernel takes by value: each variant keeps the kernarg layout it had
template <bool DEEP> using CentralPolicyArgs = std::conditional_t<DEEP, CentralDeepPolicyArgs, PolicyArgs>;
CL_DEV const PolicyArgs& central_policy_args(const PolicyArgs& p) { return p; }
CL_DEV const PolicyArgs& central_policy_args(const CentralDeepPolicyArgs& d) { return d.p; }

constexpr size_t rollout_policy_central_lds_floats(int nw, int n_bldg, int h) {
    return (size_t)nw * NQ * 64 + (size_t)2 * n_bldg * 64 + (size_t)h * 64 + (size_t)2 * h * n_bldg + (size_t)nw * 2 * CLPC_ROW;
}
constexpr size_t rollout_policy_central_deep_lds_floats(int nw, int n_bldg, int h1, int h2) {
    return (size_t)nw * NQ * 64 + (size_t)2 * n_bldg * 64 + (size_t)h1 * 64 + (size_t)h2 * 64 + (size_t)2 * h1 * n_bldg + (size_t)(h1 + 1) * h2
           + (size_t)nw * 2 * CLPC_ROW;
}

template <int PREC, bool DEEP>
__global__ void __launch_bounds__(1024) cl_rollout_policy_central_kernel(const CentralPolicyArgs<DEEP> d) {
    extern __shared__ __attribute__((aligned(16))) float lds[];     // see the header comment
    constexpr int MB = 2, VEC = 1, TILE = 64;
    const PolicyArgs& p = central_policy_args(d);
    const RolloutArgs& r = p.r;
    const StepArgs& a = r.s;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile_env0 = blockIdx.x * TILE;
    const int env0 = tile_env0 + lane;
    const bool live = env0 < a.n_env;
    const long long plane = (long long)a.n_bldg * a.n_env;         // (no row pitch: host)
    const int rkind = (a.flags & CLD_REWARD_MASK) >> CLD_REWARD_SHIFT;
    const bool quirk = a.flags & CLD_REF_T0_QUIRK;
    const int H = p.n_hidden, NB = a.n_bldg;
    int H2 = 0;                                                     // (DEEP only)
    if constexpr (DEEP) H2 = d.n_hidden2;
    const int HO = DEEP ? H2 : H;                                   // the width of the layer under the head
    const int blk = tile_env0 / CL_ROW0_BLOCK;
    const int row0 = a.env_row0 ? a.env_row0[blk] : 0;              // workgroup-uniform
    const int set = p.set_of_block ? p.set_of_block[blk] : 0;       // workgroup-uniform
    float* const X = lds + (size_t)a.nw * NQ * TILE;                // [2][NB][64]: soc, previous net
    float* const Hh = X + (size_t)2 * NB * TILE;                    // [H][64]: hidden layer 1
    float* const Hh2 = Hh + (size_t)H * TILE;                       // [H2][64]: hidden layer 2 (DEEP only: no floats otherwise)
    float* const depl = Hh2 + (size_t)H2 * TILE;                    // [H / 4][NB][8]
    float* const l2l = depl + (size_t)2 * H * NB;                   // [H + 1][H2] (DEEP only)
    float* const pol = l2l + (DEEP ? (size_t)(H + 1) * H2 : 0) + (size_t)w * MB * CLPC_ROW;
    const float* const Ho = DEEP ? Hh2 : Hh;                        // what the head reads

    const float* __restrict__ ts_w = a.ts + (long long)w * CL_NF;
    // the `pre` row of this workgroup's parameter set at the first row of its episode window (inside the loop: + t H)
    const float* __restrict__ pre_w = p.pre + ((long long)set * p.n_rows + row0) * H;
    cl::Bp B[MB];
    cl::State St[MB][VEC];
    bool own[MB];
    long long off[MB];
    int bidx[MB];
    float last_net[MB][VEC], last_rw[MB][VEC];
    // stage `dep` of this workgroup's parameter set as it is packed (all threads; the barrier below orders it)
    {
        const float* __restrict__ src = p.dep + (long long)set * 2 * H * NB;
        for (int i = threadIdx.x; i < 2 * H * NB; i += blockDim.x) depl[i] = src[i];
        if constexpr (DEEP) {
            // ... and layer 2, bias row included
            const float* __restrict__ src2 = d.l2 + (long long)set * (H + 1) * H2;
            for (int i = threadIdx.x; i < (H + 1) * H2; i += blockDim.x) l2l[i] = src2[i];
        }
    }
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        const int b = w + m * a.nw;
        own[m] = b < a.n_bldg;
        const int bc = own[m] ? b : w;
        bidx[m] = bc;
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
        if (own[m]) {
            // publish: what the first step's hidden phase reads of this building
            X[(size_t)bc * TILE + lane] = St[m][0].soc;
            X[(size_t)(NB + bc) * TILE + lane] = last_net[m][0];
        }
        // stage the building's step-independent out row (this wave's own LDS rows; the barrier below orders them)
        if (own[m] && B[m].a_es >= 0) {
            float* row = pol + m * CLPC_ROW;
            const long long sb = (long long)set * a.n_bldg + bc;
            if (lane < HO) row[lane] = p.out[sb * (HO + 1) + lane];
            if (lane == 0) {
                const float lo = r.act_low[B[m].a_es], hi = r.act_high[B[m].a_es];
                row[CLPC_MAX_HIDDEN + 0] = p.out[sb * (HO + 1) + HO];
                row[CLPC_MAX_HIDDEN + 1] = 0.5f * (hi + lo);
                row[CLPC_MAX_HIDDEN + 2] = 0.5f * (hi - lo);
                row[CLPC_MAX_HIDDEN + 3] = p.sigma ? p.sigma[B[m].a_es] : 0.0f;
                row[CLPC_MAX_HIDDEN + 4] = lo;
                row[CLPC_MAX_HIDDEN + 5] = hi;
            }
        }
    }
    __syncthreads();
    cl::BattP Bv[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        Bv[m] = B[m].batt;
        // the curve parameters pinned in VGPRs for all K steps (cl_rollout_kernel's PIN)
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

        // ---- hidden phase: this wave's groups of four units over ALL buildings, in fixed order ----
        {
            const clpol_c4ptr pq = (clpol_c4ptr)(const clpol_f4*)(pre_w + (long long)t * H);
#pragma unroll 1
            for (int g = w; g < (H >> 2); g += a.nw) {                   // wave-uniform
                const clpol_f4 pj = pq[g];
                // (held in VGPRs across the loop over the buildings: the scalar register file is full)
                float p0 = pj[0], p1 = pj[1], p2 = pj[2], p3 = pj[3];
                CL_PIN_V(p0); CL_PIN_V(p1); CL_PIN_V(p2); CL_PIN_V(p3);
                float z0 = 0.0f, z1 = 0.0f, z2 = 0.0f, z3 = 0.0f;
                const float* wg = depl + (size_t)g * NB * 8;
#pragma unroll 2
                for (int b = 0; b < NB; ++b) {
                    const float soc = X[(size_t)b * TILE + lane], net = X[(size_t)(NB + b) * TILE + lane];
                    const clpol_f4 ws = *reinterpret_cast<const clpol_f4*>(wg + b * 8);
                    const clpol_f4 wn = *reinterpret_cast<const clpol_f4*>(wg + b * 8 + 4);
                    z0 = fmaf(wn[0], net, fmaf(ws[0], soc, z0));
                    z1 = fmaf(wn[1], net, fmaf(ws[1], soc, z1));
                    z2 = fmaf(wn[2], net, fmaf(ws[2], soc, z2));
                    z3 = fmaf(wn[3], net, fmaf(ws[3], soc, z3));
                }
                float* hg = Hh + (size_t)(4 * g) * TILE + lane;
                hg[0 * TILE] = clpol_unit(p0 + z0); hg[1 * TILE] = clpol_unit(p1 + z1);
                hg[2 * TILE] = clpol_unit(p2 + z2); hg[3 * TILE] = clpol_unit(p3 + z3);
            }
        }
        __syncthreads();                                                 // barrier A: Hh complete, every read of X done

        if constexpr (DEEP) {
            // ---- hidden phase 2: this wave's groups of four layer-2 units over ALL layer-1 units, in fixed order ----
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

        // ---- action phase ----
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            if (!own[m]) continue;                                       // wave-uniform (the barriers are outside this loop)
            cl::Row R;
            const cl_cptr q = as_const(ts_w + ((long long)(t + row0) * a.n_bldg + m * a.nw) * CL_NF);
            R.nsl = cw(q, CLT_NSL); R.sol = cw(q, CLT_SOLAR); R.price = cw(q, CLT_PRICE); R.carbon = cw(q, CLT_CARBON);

            // ---- the policy's head of this building over the shared (last) hidden layer ----
            float a_es[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) a_es[i] = 0.0f;
            if (B[m].a_es >= 0) {
                const float* row = pol + m * CLPC_ROW;
                float acc = 0.0f;
#pragma unroll 1
                for (int g = 0; g < HO; g += 4) {
                    const clpol_f4 wo = *reinterpret_cast<const clpol_f4*>(row + g);
                    const float* hg = Ho + (size_t)g * TILE + lane;
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc = fmaf(wo[u], hg[u * TILE], acc);
                }
                const float mid = row[CLPC_MAX_HIDDEN + 1], half = row[CLPC_MAX_HIDDEN + 2], lo = row[CLPC_MAX_HIDDEN + 4], hi = row[CLPC_MAX_HIDDEN + 5];
                const float sg = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, row[CLPC_MAX_HIDDEN + 3])));
                a_es[0] = fmaf(half, tanhf(acc + row[CLPC_MAX_HIDDEN + 0]), mid);
                if (sg != 0.0f) {                                        // wave-uniform
                    // Box-Muller on two draws of the column's stream: counters 2t and 2t + 1 = words (0, 1) or (2, 3) of block t >> 1
                    if (k == 0 || (t & 1) == 0) {
                        const cl::U4 bk = cl::philox_block(r.seed, (uint32_t)env0 + a.env_offset, (uint32_t)B[m].a_es, (uint32_t)t >> 1);
                        rnd[m][0].w0 = bk.w[0]; rnd[m][0].w1 = bk.w[1]; rnd[m][0].w2 = bk.w[2]; rnd[m][0].w3 = bk.w[3];
                    }
                    a_es[0] = fmaf(sg, clpol_gauss(rnd[m][0].w0, rnd[m][0].w1, rnd[m][0].w2, rnd[m][0].w3, t), a_es[0]);
                }
                a_es[0] = fminf(fmaxf(a_es[0], lo), hi);
            }

            // ---- the lean unit exactly as in cl_rollout_kernel ----
            const bool first = quirk && t == 0;
            float c_ns = first ? 3.0f * R.nsl : R.nsl, sol = R.sol;
            const float cbk = first ? 2.0f : 1.0f;
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
            // publish for the next step's hidden phase (and this step's MARL sum)
            X[(size_t)bidx[m] * TILE + lane] = socs[0];
            X[(size_t)(NB + bidx[m]) * TILE + lane] = nets[0];
            if (tr && live) {
                float* const tb = tr + off[m];
                vstore<VEC>(tb + (long long)CLPOL_T_ACTION * plane, a_es);
                vstore<VEC>(tb + (long long)CLPOL_T_NET * plane, nets);
                vstore<VEC>(tb + (long long)CLPOL_T_SOC * plane, socs);
                if (rkind != CLR_MARL) vstore<VEC>(tb + (long long)CLPOL_T_REWARD * plane, rws);
            }
        }
        __syncthreads();                                                 // barrier B: X complete, every read of Hh / Hh2 done
        if (rkind == CLR_MARL) {
            // the MARL reward couples the buildings through the district net of THIS step: X's net row, summed in building order
            float dnet = 0.0f;
            for (int b = 0; b < NB; ++b) dnet += X[(size_t)(NB + b) * TILE + lane];
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                if (!own[m]) continue;
                last_rw[m][0] = cl::marl_reward(last_net[m][0], dnet); ret[0] += last_rw[m][0];
                if (tr && live) vstore<VEC>(tr + off[m] + (long long)CLPOL_T_REWARD * plane, last_rw[m]);
            }
        } else {
            ret[0] += q_rw[0];
        }
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
        if (rkind == CLR_MARL) {
            q_rw[0] = 0.0f;
#pragma unroll
            for (int m = 0; m < MB; ++m) q_rw[0] += own[m] ? last_rw[m][0] : 0.0f;
        }
        // district sums of the last step (for MARL the reward plane / sum were finished above: pass kind DEFAULT)
        district_reduce<VEC>(a, lds, w, lane, env0, live, plane, rkind == CLR_MARL ? (int)CLR_DEFAULT : rkind, q_net, q_cost, q_em, q_rw, a.nw);
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
// the struct of a central-agent policy (check_lean_policy_mlp's counterpart) and of one with two hidden layers (check_deep_policy_mlp's); each
// where the unit has included the public header that declares the struct, as in cl_policy_common.h
#ifdef CITYLEARN_AMD_POLICY_CENTRAL_H
inline int check_central_policy_mlp(const clpca_mlp* mlp) {
    if (!mlp) return fail(CL_ENULL, "mlp is NULL");
    if (int rc = check_policy_sizes(*mlp, CLPCA_MAX_HIDDEN)) return rc;
    if (mlp->flags || mlp->reserved) return fail(CL_EINVAL, "clpca_mlp.flags / .reserved must be 0");
    return CL_OK;
}
#endif
#ifdef CITYLEARN_AMD_POLICY_CENTRAL_DEEP_H
inline int check_central_deep_policy_mlp(const clpcd_mlp* mlp) {
    if (!mlp) return fail(CL_ENULL, "mlp is NULL");
    if (int rc = check_policy_sizes(*mlp, CLPCD_MAX_HIDDEN)) return rc;
    if (mlp->n_hidden2 < 4 || mlp->n_hidden2 > CLPCD_MAX_HIDDEN || mlp->n_hidden2 % 4)
        return fail(CL_EINVAL, "n_hidden2=%d: the deep central policy kernel takes 4, 8, .. %d units in its second hidden layer", mlp->n_hidden2, CLPCD_MAX_HIDDEN);
    if (mlp->flags || mlp->reserved || mlp->reserved2) return fail(CL_EINVAL, "clpcd_mlp.flags / .reserved / .reserved2 must be 0");
    return CL_OK;
}
#endif

// The geometry: two buildings per wave as cl_rollout_policy_kernel (lean_policy_geometry's nw rule), ONE env per lane.  `what`: "central policy"
// or "deep central policy", for the refusal
inline int central_policy_geometry(const cl_dims* dims, const cl_tuning& tun, const char* what, int& nw) {
    nw = tun.nw ? tun.nw : (dims->n_bldg + 1) / 2;
    // (nw > n_bldg: a wave without any building would read its parameter row -- row `w` -- past the end of the table)
    if (nw * 2 < dims->n_bldg || nw < 1 || nw > 16 || nw > dims->n_bldg) return fail(CL_EINVAL, "bad nw %d", nw);
    return one_env_per_lane_only(tun, what);
}

}  // namespace
#endif  // __HIPCC__
