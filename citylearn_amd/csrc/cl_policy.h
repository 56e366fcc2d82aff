// cl_policy.h -- mode B with a CLOSED-LOOP policy: the battery + PV K-step loop of cl_rollout_kernel<VEC, false, 2> (cl_rollout.h) whose
// electrical-storage action of every (env, building, step) is a one-hidden-layer tanh MLP over that building's own observation vector, evaluated
// inside the loop from the two observations that depend on the env -- the unit's soc before the step and its net of the previous step, both in
// registers already.  ONE kernel template, cl_rollout_policy_kernel<VEC, PREC, KPI, CHUNK>, for the three lean units, each of which instantiates
// its own variant only:
//   cl_policy.hip        <.., false, false>  libcitylearn_amd_policy.so, include/citylearn_amd_policy.h
//   cl_policy_kpi.hip    <.., true, false>   libcitylearn_amd_policy_kpi.so, include/citylearn_amd_policy_kpi.h: with the streaming KPI accumulators (below)
//   cl_policy_chunk.hip  <.., false, true>   libcitylearn_amd_policy_chunk.so, include/citylearn_amd_policy_chunk.h: districts of more than 32 buildings as
//                                            a building-chunked launch (cl_policy_chunk.h says what CHUNK switches)
// behind cl_kernels.hip's helpers.  The libraries report them as cl_rollout_policy_kernel / _kpi_kernel / _chunk_kernel<VEC, PREC>.  PolicyArgs, the
// hidden unit and the Box-Muller draw are cl_policy_common.h's, shared with the thermal policy kernel too.
//
// The split (cl_lstm.h's `dyn_pre`, for an MLP): a building's observation is obs[c] = table[row][c] + col_scale[c] * plane[c] with a plane for two
// columns only, so  W1 obs + b1 = pre[row] + ws * soc + wn * net_prev  with `pre` one H-vector per (parameter set, table row, building) the host
// computes once (citylearn_amd/policy.py) -- three FMAs and one tanh per hidden unit instead of n_obs FMAs:
//     h_j  = tanh(pre[s][r][b][j] + dep[s][b][0][j] soc + dep[s][b][1][j] net_prev)
//     mean = low + (high - low) (1 + tanh(out[s][b][H] + sum_j out[s][b][j] h_j)) / 2
//     a    = clamp(mean + sigma z, low, high),   z = sqrt(-2 ln(u1 + 2^-25)) cos(2 pi u2)  (nothing drawn where sigma == 0)
// A hidden unit's tanh is (1 - e) / (1 + e) with e = 2^(-2 log2(e) x): the packer multiplies `pre` / `dep` by -2 log2 e, so a unit is fma, fma, min,
// v_exp_f32, sub, add, v_rcp_f32, mul, fma.  (The cheaper 2 / (1 + e) - 1 with the "2 q - 1" folded into the output weights was emulated in
// float32 on the CPU before anything ran: it cancels where tanh is small and put the action 3 - 9 x (an emulation's figure, not a device measurement) a float32 torch evaluation's error away from
// float64; this form stays within 2 - 3 x.  The min keeps e finite: (1 - inf) * 0 is a NaN.)  The ONE output unit per building and step uses the
// library's tanhf on the unscaled sum: a = mid + half tanh(.) is what the caller's torch code computes, and its error goes straight to the action.
//
// Where the tables are read from.  Everything is wave-uniform (the building is, the parameter set and the table row are workgroup-uniform):
//  * `pre` changes every step: H consecutive floats through the constant address space (s_load_dwordx4 per four units) -- cl_rollout_kpi_kernel's
//    route for tables read inside a loop that holds MARL's barriers;
//  * `dep` / `out` / the column's bounds and sigma are the same for all K steps.  The scalar register file of these kernels is full
//    (cl_rollout_kernel's notes), so each wave stages them once per launch in its own LDS rows -- per building [H / 4][ws x 4 | wn x 4 | out x 4]
//    + {bias, mid, half, sigma, low, high} -- and reads them back as three broadcast ds_read_b128 per four hidden units.
// LDS per workgroup: the district reduction's [nw][NQ][tile] rows (MARL's exchange row and the return rows alias them) + nw x 2 x CLPOL_ROW floats:
// 49 KiB at the largest geometry (nw = 16, two envs per lane); the host refuses anything beyond the CU's 160 KiB.
//
// KPI = true is the K-step loop of cl_rollout_kpi_kernel (cl_rollout.h) with this action source; what it adds sits under `if constexpr (KPI)`, so
// each instantiation is the code of the kernel it was when the two were separate sources (profiles/policy_one_source_isa.md).  Nothing in it is
// new arithmetic, and every accumulation keeps the order of the two kernels that tests/test_gpu_policy_kpi_rollout.py compares it with.  From
// cl_rollout_kpi_kernel: the four control sums per unit in registers; the control / baseline district series in LDS (kpi_series_get / _put /
// _advance); the S = 8 ring of wave partial nets folded in wave order; the env block's `brow` / `bsum` baseline rows kept by its head workgroup;
// MARL reading the ring slot it just wrote behind ONE barrier per step (without the KPIs: slot 0, and a second barrier before it is written
// again); tables through the constant address space.
// Its LDS per workgroup: cl_rollout_kpi_kernel's region (rollout_kpi_lds_floats) followed by nw x 2 x CLPOL_ROW floats (rollout_policy_kpi_lds_floats):
// 55 296 bytes at 17 buildings (nw = 9) and two envs per lane, 89 792 at the largest geometry (nw = 16, two envs per lane); above 64 KiB -- from
// nw = 12 at two envs per lane -- the launch opts in, above the CU's 160 KiB the host refuses.
// Its registers: the sixteen control sums and the MLP loop's live values together; which curve parameters stay pinned per instantiation: clpk_pins.
#pragma once
#include "cl_policy_common.h"

#ifdef __HIPCC__
namespace {

constexpr int CLPOL_MAX_H = 32;
constexpr int CLPOL_ROW = 3 * CLPOL_MAX_H + 8;       // floats of one building's staged row: [H/4][3][4] weights | bias, mid, half, sigma, low, high, pad x 2

constexpr size_t rollout_policy_lds_floats(int nw, int tile) { return (size_t)nw * NQ * tile + (size_t)nw * 2 * CLPOL_ROW; }
constexpr size_t rollout_policy_kpi_lds_floats(int nw, int tile) { return rollout_kpi_lds_floats(nw, tile) + (size_t)nw * 2 * CLPOL_ROW; }

// The curve parameters pinned in VGPRs for all K steps (cl_rollout_kernel's PIN): only where the 128 registers of a 1024-thread workgroup have room
// for them.  With the KPIs, next to the control sums and the policy's inputs, that is one env per lane (DESIGN section 5 has the figures of every
// instantiation); without them, everywhere but two envs per lane on the fp32 map (cl_rollout_kpi_kernel's note).
constexpr bool clpk_pins(bool kpi, int vec, int prec) { return kpi ? vec == 1 : !(vec == 2 && prec == 0); }

template <int VEC, int PREC, bool KPI, bool CHUNK>
__global__ void __launch_bounds__(1024) cl_rollout_policy_kernel(const PolicyArgs p) {
    static_assert(!(KPI && CHUNK), "no building-chunked launch keeps the streaming KPIs");
    // KPI:  ring [S][nw][64*VEC] | control series [12][64*VEC] | baseline series [16] | rows [S][4][32] | baseline sums [5][32] | policy rows [nw][2][CLPOL_ROW]
    // else: [nw][NQ][64*VEC] | [nw][2][CLPOL_ROW]
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int MB = 2, TILE = 64 * VEC, S = CL_RKPI_S;
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
    const int H = p.n_hidden;
    const int blk = tile_env0 / CL_ROW0_BLOCK;
    const int row0 = a.env_row0 ? a.env_row0[blk] : 0;              // workgroup-uniform
    const int set = p.set_of_block ? p.set_of_block[blk] : 0;       // workgroup-uniform
    // KPI only (as in cl_rollout_kpi_kernel) -- the head workgroup of an env block keeps the block's env-independent sums
    [[maybe_unused]] const bool head = tile_env0 % CL_ROW0_BLOCK == 0;               // workgroup-uniform
    [[maybe_unused]] const bool base_owner = head && threadIdx.x == blockDim.x - 1;
    [[maybe_unused]] float* const ser = lds + (size_t)S * a.nw * TILE;
    [[maybe_unused]] float* const bser = ser + (size_t)CLKE_PER_COND * TILE;
    [[maybe_unused]] float* const brow = bser + 16;                 // per ring slot and building: baseline net, carbon intensity, price, load
    [[maybe_unused]] float* const bsum = brow + S * 4 * CL_RKPI_NB; // CLK_B_POS, _NET, _EMISSION, _COST, CLK_EXPECTED_ALL of the env block
    // the env block's per-building sums: lane b of the head workgroup's LAST wave keeps building b's five
    [[maybe_unused]] const bool bsum_owner = head && w == a.nw - 1 && lane < a.n_bldg;
    // the staged policy rows: behind the KPI region, or behind the reduction rows
    float* const pol = (KPI ? bsum + 5 * CL_RKPI_NB : lds + (size_t)a.nw * NQ * TILE) + (size_t)w * MB * CLPOL_ROW;

    if constexpr (KPI) {
        // the district series' accumulators: HBM -> LDS, by the thread that folds them (nobody else touches the column)
        for (int e = threadIdx.x; e < TILE; e += blockDim.x) {
            if (tile_env0 + e >= a.n_env) continue;
            KpiSeriesAll c;
            kpi_series_get(c, a.kpi_env + tile_env0 + e, a.n_env);
            kpi_series_put(ser + e, TILE, c);
        }
        if (base_owner) {
            KpiSeriesAll c;
            kpi_series_get(c, a.kpi_env + (long long)CLKE_PER_COND * a.n_env + tile_env0, a.n_env);
            kpi_series_put(bser, 1, c);
        }
        if (bsum_owner) {
            const float* kp = a.kpi_bldg + (long long)lane * a.n_env + tile_env0;      // building `lane` at the block's first env
            bsum[0 * CL_RKPI_NB + lane] = kp[(long long)CLK_B_POS * plane]; bsum[1 * CL_RKPI_NB + lane] = kp[(long long)CLK_B_NET * plane];
            bsum[2 * CL_RKPI_NB + lane] = kp[(long long)CLK_B_EMISSION * plane]; bsum[3 * CL_RKPI_NB + lane] = kp[(long long)CLK_B_COST * plane];
            bsum[4 * CL_RKPI_NB + lane] = kp[(long long)CLK_EXPECTED_ALL * plane];
        }
    }

    // CHUNK: the first building of this workgroup row's chunk (gridDim.y rows of a.b_chunk buildings)
    const int b_lo = CHUNK ? blockIdx.y * a.b_chunk : 0;
    // the table rows of this wave's first building ...
    const float* __restrict__ ts_w;
    // ... and its `pre` rows in this workgroup's parameter set and episode window (inside the loop: + (t n_bldg + m nw) H)
    const float* __restrict__ pre_w;
    if constexpr (!CHUNK) {
        ts_w = a.ts + (long long)w * CL_NF;
        pre_w = p.pre + (((long long)set * p.n_rows + row0) * a.n_bldg + w) * H;
    }
    cl::Bp B[MB];
    cl::State St[MB][VEC];
    bool own[MB];
    long long off[MB];
    [[maybe_unused]] float k_pos[MB][VEC], k_net[MB][VEC], k_em[MB][VEC], k_cost[MB][VEC];      // KPI: cl_step_lean_kpi_kernel's four control sums
    float last_net[MB][VEC], last_rw[MB][VEC];
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        const int b = b_lo + w + m * a.nw;
        // CHUNK: b < b_hi = min(n_bldg, b_lo + b_chunk), wave-uniform.  (The scalar register file of this kernel is full -- numbered_sgpr = 100 in
        // every instantiation -- and what its allocation spills decides whether a 16-byte spill slot and the 4-byte scavenging slot stay reserved
        // as scratch memory that no instruction touches.  With b_hi as a value of its own <2, 0> reserved those 20 bytes; see also the pointers
        // behind the barrier and the arguments re-read behind the K loop.)
        own[m] = CHUNK ? (w + m * a.nw < a.b_chunk) && b < a.n_bldg : b < a.n_bldg;
        // a seat without a building reads a valid parameter row, for its flag words only (CHUNK: ONE min, cl_policy_full.h's note)
        const int bc = CHUNK ? min(b, a.n_bldg - 1) : own[m] ? b : w;
        off[m] = (long long)bc * a.n_env + env0;
        cl::load_bp<false>(B[m], a.params + (long long)bc * CL_NP);
        // the previous step's net: what the reset observation shows in front of step 0, what the previous launch (or reset) left otherwise
        const float net0 = (r.t0 == 0 && p.net_reset) ? p.net_reset[(long long)row0 * a.n_bldg + bc] : 0.0f;
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            St[m][i] = {0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            if constexpr (KPI) k_pos[m][i] = k_net[m][i] = k_em[m][i] = k_cost[m][i] = 0.0f;
            last_net[m][i] = net0; last_rw[m][i] = 0.0f;
        }
        if (live && own[m]) {
            float v[VEC];
#define CL_GET(dst, base, plane_id)                                    \
    vload<VEC>(v, base + (long long)(plane_id) * plane + off[m]);      \
    _Pragma("unroll") for (int i = 0; i < VEC; ++i) dst = v[i];
            CL_GET(St[m][i].soc, a.state, CLS_B_SOC) CL_GET(St[m][i].eff, a.state, CLS_B_EFF) CL_GET(St[m][i].degcap, a.state, CLS_B_DEGCAP)
            if constexpr (KPI) {
                CL_GET(k_pos[m][i], a.kpi_bldg, CLK_C_POS) CL_GET(k_net[m][i], a.kpi_bldg, CLK_C_NET)
                CL_GET(k_em[m][i], a.kpi_bldg, CLK_C_EMISSION) CL_GET(k_cost[m][i], a.kpi_bldg, CLK_C_COST)
            }
            if (r.t0 != 0) { CL_GET(last_net[m][i], a.out_bldg, CLO_NET) }
#undef CL_GET
        }
        // stage the building's step-independent policy rows (this wave's own LDS rows; the barrier below orders them)
        if (own[m] && B[m].a_es >= 0) {
            float* row = pol + m * CLPOL_ROW;
            const long long sb = (long long)set * a.n_bldg + bc;
            if (lane < H) {
                const int at = (lane >> 2) * 12 + (lane & 3);
                row[at] = p.dep[(sb * 2 + 0) * H + lane];
                row[at + 4] = p.dep[(sb * 2 + 1) * H + lane];
                row[at + 8] = p.out[sb * (H + 1) + lane];
            }
            if (lane == 0) {
                const float lo = r.act_low[B[m].a_es], hi = r.act_high[B[m].a_es];
                row[3 * CLPOL_MAX_H + 0] = p.out[sb * (H + 1) + H];
                row[3 * CLPOL_MAX_H + 1] = 0.5f * (hi + lo);
                row[3 * CLPOL_MAX_H + 2] = 0.5f * (hi - lo);
                row[3 * CLPOL_MAX_H + 3] = p.sigma ? p.sigma[B[m].a_es] : 0.0f;
                row[3 * CLPOL_MAX_H + 4] = lo;
                row[3 * CLPOL_MAX_H + 5] = hi;
            }
        }
    }
    __syncthreads();
    if constexpr (CHUNK) {
        // inside the K loop neither the chunk nor the wave index is needed for a row address (read only by a seat that has a building; computed
        // behind the prologue, whose scalar loads of two parameter blocks need the registers)
        ts_w = a.ts + (long long)(b_lo + w) * CL_NF;
        pre_w = p.pre + (((long long)set * p.n_rows + row0) * a.n_bldg + b_lo + w) * H;
    }
    cl::BattP Bv[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        Bv[m] = B[m].batt;
        if constexpr (!clpk_pins(KPI, VEC, PREC)) continue;
        CL_PIN_V(Bv[m].cpc_a0); CL_PIN_V(Bv[m].cpc_b0); CL_PIN_V(Bv[m].cpc_a1); CL_PIN_V(Bv[m].cpc_b1);
        CL_PIN_V(Bv[m].pec_a0); CL_PIN_V(Bv[m].pec_b0); CL_PIN_V(Bv[m].pec_a1); CL_PIN_V(Bv[m].pec_b1);
        CL_PIN_V(Bv[m].pec_a2); CL_PIN_V(Bv[m].pec_b2); CL_PIN_V(Bv[m].pec_a3); CL_PIN_V(Bv[m].pec_b3);
    }
    float ret[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) ret[i] = 0.0f;
    float q_net[VEC], q_cost[VEC], q_em[VEC], q_rw[VEC];
    if constexpr (CHUNK) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) q_net[i] = q_cost[i] = q_em[i] = q_rw[i] = 0.0f;
    }
    PhiloxCache rnd[MB][VEC];

    // (CHUNK: no barrier inside, hence no MARL -- a wave without a building runs the K loop's frame and nothing in it)

    for (int k = 0; k < r.k_steps; ++k) {
        const int t = r.t0 + k;
        const int slot = KPI ? k & (S - 1) : 0;                          // KPI: the ring slot of this step's wave partial nets
        float* const tr = p.traj ? p.traj + (long long)k * CLPOL_NT * plane : nullptr;
#pragma unroll
        for (int i = 0; i < VEC; ++i) q_net[i] = q_cost[i] = q_em[i] = q_rw[i] = 0.0f;
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            if (!own[m]) continue;                                       // wave-uniform
            cl::Row R;
            const cl_cptr q = as_const(ts_w + ((long long)(t + row0) * a.n_bldg + m * a.nw) * CL_NF);
            R.nsl = cw(q, CLT_NSL); R.sol = cw(q, CLT_SOLAR); R.price = cw(q, CLT_PRICE); R.carbon = cw(q, CLT_CARBON);

            // ---- the policy: this building's storage action from (table row, soc, previous net) ----
            float a_es[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) a_es[i] = 0.0f;
            if (B[m].a_es >= 0) {
                const float* row = pol + m * CLPOL_ROW;
                const clpol_c4ptr pq = (clpol_c4ptr)(const clpol_f4*)(pre_w + ((long long)t * a.n_bldg + m * a.nw) * H);
                float acc[VEC];
#pragma unroll
                for (int i = 0; i < VEC; ++i) acc[i] = row[3 * CLPOL_MAX_H + 0];
#pragma unroll 1
                for (int g = 0; g < H; g += 4) {
                    const clpol_f4 pj = pq[g >> 2];
                    const clpol_f4 ws = *reinterpret_cast<const clpol_f4*>(row + g * 3);
                    const clpol_f4 wn = *reinterpret_cast<const clpol_f4*>(row + g * 3 + 4);
                    const clpol_f4 wo = *reinterpret_cast<const clpol_f4*>(row + g * 3 + 8);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
#pragma unroll
                        for (int i = 0; i < VEC; ++i) {
                            acc[i] = fmaf(wo[u], clpol_unit(fmaf(wn[u], last_net[m][i], fmaf(ws[u], St[m][i].soc, pj[u]))), acc[i]);
                        }
                    }
                }
                const float mid = row[3 * CLPOL_MAX_H + 1], half = row[3 * CLPOL_MAX_H + 2], lo = row[3 * CLPOL_MAX_H + 4], hi = row[3 * CLPOL_MAX_H + 5];
                const float sg = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, row[3 * CLPOL_MAX_H + 3])));
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
            if (KPI && head && lane == 0) {
                // the step's net with the battery term left out (and what prices it): for the env block's baseline sums and baseline district series
                float* brw = brow + (size_t)slot * 4 * CL_RKPI_NB + w + m * a.nw;
                brw[0 * CL_RKPI_NB] = fmaf(c_ns, B[m].r, sol); brw[1 * CL_RKPI_NB] = R.carbon; brw[2 * CL_RKPI_NB] = R.price; brw[3 * CL_RKPI_NB] = R.nsl;
            }
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
                if constexpr (KPI) {
                    // cl_step_lean_kpi_kernel's four control sums
                    k_pos[m][i] += fmaxf(nets[i], 0.0f); k_net[m][i] += nets[i];
                    k_em[m][i] += fmaxf(nets[i] * R.carbon, 0.0f); k_cost[m][i] += fmaxf(nets[i] * R.price, 0.0f);
                }
            }
            if (tr && live) {
                float* const tb = tr + off[m];
                vstore<VEC>(tb + (long long)CLPOL_T_ACTION * plane, a_es);
                vstore<VEC>(tb + (long long)CLPOL_T_NET * plane, nets);
                vstore<VEC>(tb + (long long)CLPOL_T_SOC * plane, socs);
                if (CHUNK || rkind != CLR_MARL) vstore<VEC>(tb + (long long)CLPOL_T_REWARD * plane, rws);
            }
        }
        // the wave's partial net into the ring slot (KPI: every step, for the district series; else: MARL's exchange row, slot 0)
        if (KPI || (!CHUNK && rkind == CLR_MARL)) vstore<VEC>(lds + ((size_t)slot * a.nw + w) * TILE + lane * VEC, q_net);
        if (!CHUNK && rkind == CLR_MARL) {
            // the MARL reward couples the buildings through the district net of THIS step: one LDS exchange per step
            __syncthreads();
            float dnet[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) dnet[i] = 0.0f;
            for (int kk = 0; kk < a.nw; ++kk) {
                float part[VEC];
                vload<VEC>(part, lds + ((size_t)slot * a.nw + kk) * TILE + lane * VEC);
#pragma unroll
                for (int i = 0; i < VEC; ++i) dnet[i] += part[i];
            }
            if constexpr (!KPI) __syncthreads();                         // (KPI: the slot is not written again before the fold's barrier)
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                if (!own[m]) continue;
#pragma unroll
                for (int i = 0; i < VEC; ++i) { last_rw[m][i] = cl::marl_reward(last_net[m][i], dnet[i]); ret[i] += last_rw[m][i]; }
                if (tr && live) vstore<VEC>(tr + off[m] + (long long)CLPOL_T_REWARD * plane, last_rw[m]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < VEC; ++i) ret[i] += q_rw[i];
        }
        if (KPI && (slot == S - 1 || k == r.k_steps - 1)) {
            // fold the ring's slot + 1 samples (steps t - slot .. t) into the district series
            if (rkind != CLR_MARL) __syncthreads();                      // (MARL: everybody's slot is behind this step's barrier already)
            const int tb = t - slot;
            for (int e = threadIdx.x; e < TILE; e += blockDim.x) {
                if (tile_env0 + e >= a.n_env) continue;
                for (int j = 0; j <= slot; ++j) {
                    float v = 0.0f;
                    for (int kk = 0; kk < a.nw; ++kk) v += lds[((size_t)j * a.nw + kk) * TILE + e];
                    kpi_series_advance(ser + e, TILE, tb + j, v);
                }
            }
            if (bsum_owner) {
                // cl_step_lean_kpi_kernel's `block_sums`, step by step
                float p_pos = bsum[0 * CL_RKPI_NB + lane], p_net = bsum[1 * CL_RKPI_NB + lane], p_em = bsum[2 * CL_RKPI_NB + lane],
                      p_cost = bsum[3 * CL_RKPI_NB + lane], p_exp = bsum[4 * CL_RKPI_NB + lane];
                for (int j = 0; j <= slot; ++j) {
                    const float* brw = brow + (size_t)j * 4 * CL_RKPI_NB + lane;
                    const float base = brw[0 * CL_RKPI_NB], carbon = brw[1 * CL_RKPI_NB], price = brw[2 * CL_RKPI_NB];
                    p_pos += fmaxf(base, 0.0f); p_net += base;
                    p_em += fmaxf(base * carbon, 0.0f); p_cost += fmaxf(base * price, 0.0f);
                    p_exp += brw[3 * CL_RKPI_NB];
                }
                bsum[0 * CL_RKPI_NB + lane] = p_pos; bsum[1 * CL_RKPI_NB + lane] = p_net; bsum[2 * CL_RKPI_NB + lane] = p_em;
                bsum[3 * CL_RKPI_NB + lane] = p_cost; bsum[4 * CL_RKPI_NB + lane] = p_exp;
            }
            if (base_owner) {
                // the baseline district series: the buildings' baselines in building order (cl_step_lean_kpi_kernel's `base_writer`)
                for (int j = 0; j <= slot; ++j) {
                    float v = 0.0f;
                    for (int b = 0; b < a.n_bldg; ++b) v += brow[(size_t)j * 4 * CL_RKPI_NB + b];
                    kpi_series_advance(bser, 1, tb + j, v);
                }
            }
            __syncthreads();                                             // the ring is free again (and, behind the last step, for the reduction rows)
        }
    }

    // ---- write back: carried state, the last step's per-building outputs, the KPI accumulators, district sums, episode-return partials
    // (cl_rollout_kernel's / cl_rollout_kpi_kernel's).  The loop nest is each variant's own -- `live` outside the buildings without the KPIs,
    // inside with them: either nest for both changes the other variant's generated code (profiles/policy_one_source_isa.md) ----
    // CHUNK: the launch arguments the epilogue needs -- the plane pointers, n_env, n_chunks, ret_env -- are read AGAIN here, from the
    // kernel-argument segment at an offset the compiler cannot see is zero (cl_rollout_full_kernel's device for its per-step parameter re-read):
    // taken from `p` they stay in scalar registers across the whole K loop, and the float64-chain instantiations, whose loop holds a building's
    // 19 doubles beside both parameter blocks, then reserve the 20 bytes of scratch memory of the note above.  PolicyArgs is the kernel's only argument.
    const PolicyArgs* pep = &p;
    if constexpr (CHUNK) {
        int z;
        asm("s_mov_b32 %0, 0" : "=s"(z) : "s"(r.k_steps));
        pep = (const PolicyArgs*)((const char*)__builtin_amdgcn_kernarg_segment_ptr() + z);      // (C casts: out of the constant address space)
    }
    const RolloutArgs& re = pep->r;
    const StepArgs& ae = re.s;
#define CL_PUT(base, plane_id, expr)                                   \
    _Pragma("unroll") for (int i = 0; i < VEC; ++i) v[i] = (expr);      \
    vstore<VEC>(base + (long long)(plane_id) * plane + off[m], v);
#define CL_PUT_UNIT                                                                                                                            \
    float v[VEC];                                                                                                                              \
    if (B[m].flags & CLF_BATTERY) {                                                                                                            \
        CL_PUT(ae.state, CLS_B_SOC, St[m][i].soc) CL_PUT(ae.state, CLS_B_EFF, St[m][i].eff) CL_PUT(ae.state, CLS_B_DEGCAP, St[m][i].degcap)    \
    }                                                                                                                                          \
    if (r.k_steps > 0) {                                                                                                                       \
        CL_PUT(ae.out_bldg, CLO_NET, last_net[m][i])                                                                                           \
        CL_PUT(ae.out_bldg, CLO_REWARD, last_rw[m][i])                                                                                         \
        if constexpr (KPI) {                                                                                                                   \
            CL_PUT(a.kpi_bldg, CLK_C_POS, k_pos[m][i]) CL_PUT(a.kpi_bldg, CLK_C_NET, k_net[m][i])                                              \
            CL_PUT(a.kpi_bldg, CLK_C_EMISSION, k_em[m][i]) CL_PUT(a.kpi_bldg, CLK_C_COST, k_cost[m][i])                                        \
        }                                                                                                                                      \
    }
    if constexpr (KPI) {
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            if (!own[m]) continue;
            if (live) { CL_PUT_UNIT }
        }
    } else if (live) {
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            if (!own[m]) continue;
            CL_PUT_UNIT
        }
    }
#undef CL_PUT_UNIT
#undef CL_PUT
    if (r.k_steps > 0) {
        if constexpr (KPI) {
            if (bsum_owner) {
                float* kp = a.kpi_bldg + (long long)lane * a.n_env + tile_env0;
                kp[(long long)CLK_B_POS * plane] = bsum[0 * CL_RKPI_NB + lane]; kp[(long long)CLK_B_NET * plane] = bsum[1 * CL_RKPI_NB + lane];
                kp[(long long)CLK_B_EMISSION * plane] = bsum[2 * CL_RKPI_NB + lane]; kp[(long long)CLK_B_COST * plane] = bsum[3 * CL_RKPI_NB + lane];
                kp[(long long)CLK_EXPECTED_ALL * plane] = bsum[4 * CL_RKPI_NB + lane];
            }
            for (int e = threadIdx.x; e < TILE; e += blockDim.x) {
                if (tile_env0 + e >= a.n_env) continue;
                KpiSeriesAll c;
                kpi_series_get(c, ser + e, TILE);
                kpi_series_put(a.kpi_env + tile_env0 + e, a.n_env, c);
            }
            if (base_owner) {
                KpiSeriesAll c;
                kpi_series_get(c, bser, 1);
                kpi_series_put(a.kpi_env + (long long)CLKE_PER_COND * a.n_env + tile_env0, a.n_env, c);
            }
        }
        if (!CHUNK && rkind == CLR_MARL) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                q_rw[i] = 0.0f;
#pragma unroll
                for (int m = 0; m < MB; ++m) q_rw[i] += own[m] ? last_rw[m][i] : 0.0f;
            }
        }
        // district sums of the last step (for MARL the reward plane / sum were finished above: pass kind DEFAULT).  CHUNK (n_chunks > 1): the sums of
        // the workgroup's waves go to scratch row (blockIdx.y, quantity) of the reserved plane; cl_finish_kernel adds the chunks
        district_reduce<VEC>(ae, lds, w, lane, env0, live, plane, !CHUNK && rkind == CLR_MARL ? (int)CLR_DEFAULT : rkind, q_net, q_cost, q_em, q_rw, ae.nw);
    }
    if (re.ret_env) {
        __syncthreads();
        vstore<VEC>(lds + (size_t)w * TILE + lane * VEC, ret);
        __syncthreads();
        for (int e = threadIdx.x; e < TILE; e += blockDim.x) {
            float s = 0.0f;
            for (int kk = 0; kk < ae.nw; ++kk) s += lds[(size_t)kk * TILE + e];
            if (tile_env0 + e >= ae.n_env) continue;
            // CHUNK: this workgroup row's share of the return, in its scratch row behind the n_chunks x NQ partial sums (cl_rollout_kernel<CHUNK>'s),
            // for cl_finish_kernel to add to ret_env
            if constexpr (CHUNK) ae.out_bldg[(long long)CLO_RESERVED * plane + ((long long)ae.n_chunks * NQ + blockIdx.y) * ae.n_env + tile_env0 + e] = s;
            else re.ret_env[tile_env0 + e] += s;
        }
    }
}

// ---- host: what clpol_rollout_mlp_f32 and clpk_rollout_mlp_kpi_f32 share beyond cl_policy_common.h ----
// The one-row lean rollout's geometry: two buildings per wave, two envs per lane where the 128-env workgroups come in (nearly) full rounds of one
// per CU (full_rounds, cl_kernels.hip).  `what`: "policy" or "policy KPI", for the refusal
int lean_policy_geometry(const cl_dims* dims, const cl_tuning& tun, const char* what, int& nw, int& vec) {
    nw = tun.nw ? tun.nw : (dims->n_bldg + 1) / 2;
    // (nw > n_bldg: a wave without any building would read its parameter row -- row `w` -- past the end of the table)
    if (nw * 2 < dims->n_bldg || nw < 1 || nw > 16 || nw > dims->n_bldg) return fail(CL_EINVAL, "bad nw %d", nw);
    vec = tun.vec ? tun.vec : (full_rounds(dims->n_env, 1) ? 2 : 1);
    if (vec != 1 && vec != 2) return fail(CL_EINVAL, "no %s rollout kernel at %d envs per lane", what, vec);
    return CL_OK;
}

}  // namespace
#endif  // __HIPCC__
