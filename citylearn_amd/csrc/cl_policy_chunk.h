// cl_policy_chunk.h -- mode B of a battery + PV district of MORE THAN 32 buildings with a CLOSED-LOOP policy: the K loop of
// cl_rollout_policy_kernel<VEC, PREC> (cl_policy.h: two buildings per wave, each one's storage action a one-hidden-layer tanh MLP evaluated inside
// the loop from its soc and its previous net, then the lean unit) in the chunk geometry of cl_rollout_kernel<.., CHUNK = true, ..> (cl_rollout.h):
// the buildings are cut into chunks of `b_chunk` <= 32 along gridDim.y, wave w of workgroup row y owns buildings y b_chunk + w and y b_chunk + w + nw,
// and a workgroup ends with its chunk's partial district sums of the last step and its chunk's share of the K-step return in the scratch rows of
// out_bldg's reserved plane, which ONE cl_finish_kernel launch folds per launch.  Included by cl_policy_chunk.hip only
// (libcitylearn_amd_policy_chunk.so, include/citylearn_amd_policy_chunk.h).
//
// What differs from the one-row kernel:
//  * everything it indexes by w + m nw -- params, ts, state, out_bldg, pre, dep, out, net_reset, the traj planes -- is indexed by the global
//    building b = y b_chunk + w + m nw here; the Philox stream stays keyed by (global env, action column, step) and keeps its two-step block cache,
//    so a chunk geometry does not change a draw;
//  * a SEAT without a building (own[m] = b < min(n_bldg, (y + 1) b_chunk), wave-uniform) loads, stages, computes, records and stores nothing and
//    adds zeros to the reductions.  A wave with NEITHER seat filled (the tail of the last chunk: 33 buildings cut 32 + 1 leave fifteen) reads the
//    parameter row of one clamped, valid building -- ONE min, cl_policy_full_chunk.h's note -- and touches nothing else; it meets the barrier behind
//    the row staging, district_reduce's and the return rows';
//  * the last step's district sums go through district_reduce's n_chunks > 1 path, the return rows behind them (cl_rollout_kernel<CHUNK>'s place);
//    ret_env is cl_finish_kernel's to add to;
//  * NO barrier inside the K loop, hence no MARL (a chunked launch cannot couple the buildings inside a step anyway): the wave-uniform table reads
//    stay scalar (cl_rollout_full_kernel's note on its MARL instantiations).
// The policy block is written out again (as cl_policy_kpi.h does): shared functions changed the parents' generated code before
// (profiles/policy_refactor_isa.md).  LDS per workgroup: cl_policy.h's formula, [nw][NQ][tile] reduction rows (the return rows alias them) +
// nw x 2 x CLPOL_ROW floats -- 29 KiB at the default sixteen waves and one env per lane, 45 KiB at two.
#pragma once
#include "cl_policy.h"

#ifdef __HIPCC__
namespace {

constexpr size_t rollout_policy_chunk_lds_floats(int nw, int tile) { return (size_t)nw * NQ * tile + (size_t)nw * 2 * CLPOL_ROW; }

template <int VEC, int PREC>
__global__ void __launch_bounds__(1024) cl_rollout_policy_chunk_kernel(const PolicyArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];     // [nw][NQ][64*VEC] | [nw][2][CLPOL_ROW]
    constexpr int MB = 2, TILE = 64 * VEC;
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
    float* const pol = lds + (size_t)a.nw * NQ * TILE + (size_t)w * MB * CLPOL_ROW;

    const int b_lo = blockIdx.y * a.b_chunk;
    cl::Bp B[MB];
    cl::State St[MB][VEC];
    bool own[MB];
    long long off[MB];
    float last_net[MB][VEC], last_rw[MB][VEC];
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        const int b = b_lo + w + m * a.nw;
        // b < b_hi = min(n_bldg, b_lo + b_chunk), wave-uniform.  (The scalar register file of this kernel is full -- numbered_sgpr = 100 in every
        // instantiation -- and what its allocation spills decides whether a 16-byte spill slot and the 4-byte scavenging slot stay reserved as
        // scratch memory that no instruction touches.  With b_hi as a value of its own <2, 0> reserved those 20 bytes; see also the pointers behind
        // the barrier and the arguments re-read behind the K loop.)
        own[m] = (w + m * a.nw < a.b_chunk) && b < a.n_bldg;
        // a seat without a building reads a valid parameter row, for its flag words only (ONE min: cl_policy_full_chunk.h's note)
        const int bc = min(b, a.n_bldg - 1);
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
    // the table rows of this wave's first seat: inside the K loop neither the chunk nor the wave index is needed for a row address (read only
    // by a seat that has a building; computed behind the prologue, whose scalar loads of two parameter blocks need the registers)
    const float* __restrict__ ts_w = a.ts + (long long)(b_lo + w) * CL_NF;
    // ... and its `pre` rows in this workgroup's parameter set and episode window (inside the loop: + (t n_bldg + m nw) H)
    const float* __restrict__ pre_w = p.pre + (((long long)set * p.n_rows + row0) * a.n_bldg + b_lo + w) * H;
    cl::BattP Bv[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        Bv[m] = B[m].batt;
        // the curve parameters pinned in VGPRs for all K steps (cl_rollout_kernel's PIN) -- not at two envs per lane on the fp32 map, where the
        // loop's registers leave no room for them under a 1024-thread workgroup's 128 (cl_rollout_kpi_kernel's note)
        if constexpr (VEC == 2 && PREC == 0) continue;
        CL_PIN_V(Bv[m].cpc_a0); CL_PIN_V(Bv[m].cpc_b0); CL_PIN_V(Bv[m].cpc_a1); CL_PIN_V(Bv[m].cpc_b1);
        CL_PIN_V(Bv[m].pec_a0); CL_PIN_V(Bv[m].pec_b0); CL_PIN_V(Bv[m].pec_a1); CL_PIN_V(Bv[m].pec_b1);
        CL_PIN_V(Bv[m].pec_a2); CL_PIN_V(Bv[m].pec_b2); CL_PIN_V(Bv[m].pec_a3); CL_PIN_V(Bv[m].pec_b3);
    }
    float ret[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) ret[i] = 0.0f;
    float q_net[VEC], q_cost[VEC], q_em[VEC], q_rw[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) q_net[i] = q_cost[i] = q_em[i] = q_rw[i] = 0.0f;
    PhiloxCache rnd[MB][VEC];

    // (no barrier inside: a wave without a building runs the K loop's frame and nothing in it)
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

    // ---- write back: carried state, the last step's per-building outputs, this chunk's partial district sums and its share of the return ----
    // The launch arguments the epilogue needs -- the plane pointers, n_env, n_chunks, ret_env -- are read AGAIN here, from the kernel-argument
    // segment at an offset the compiler cannot see is zero (cl_rollout_full_kernel's device for its per-step parameter re-read): taken from `p`
    // they stay in scalar registers across the whole K loop, and the float64-chain instantiations, whose loop holds a building's 19 doubles
    // beside both parameter blocks, then reserve the 20 bytes of scratch memory of the note above.  PolicyArgs is the kernel's only argument.
    int z;
    asm("s_mov_b32 %0, 0" : "=s"(z) : "s"(r.k_steps));
    const PolicyArgs& pe = *(const PolicyArgs*)((const char*)__builtin_amdgcn_kernarg_segment_ptr() + z);      // (C casts: out of the constant address space)
    const RolloutArgs& re = pe.r;
    const StepArgs& ae = re.s;
    if (live) {
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            if (!own[m]) continue;
            float v[VEC];
#define CL_PUT(base, plane_id, expr)                                   \
    _Pragma("unroll") for (int i = 0; i < VEC; ++i) v[i] = (expr);      \
    vstore<VEC>(base + (long long)(plane_id) * plane + off[m], v);
            if (B[m].flags & CLF_BATTERY) {
                CL_PUT(ae.state, CLS_B_SOC, St[m][i].soc) CL_PUT(ae.state, CLS_B_EFF, St[m][i].eff) CL_PUT(ae.state, CLS_B_DEGCAP, St[m][i].degcap)
            }
            if (r.k_steps > 0) {
                CL_PUT(ae.out_bldg, CLO_NET, last_net[m][i])
                CL_PUT(ae.out_bldg, CLO_REWARD, last_rw[m][i])
            }
#undef CL_PUT
        }
    }
    // (n_chunks > 1: the sums of the workgroup's waves go to scratch row (blockIdx.y, quantity) of the reserved plane; cl_finish_kernel adds the chunks)
    if (r.k_steps > 0) district_reduce<VEC>(ae, lds, w, lane, env0, live, plane, rkind, q_net, q_cost, q_em, q_rw, ae.nw);
    if (re.ret_env) {
        __syncthreads();
        vstore<VEC>(lds + (size_t)w * TILE + lane * VEC, ret);
        __syncthreads();
        // this workgroup row's share of the return: its scratch row behind the n_chunks x NQ partial sums (cl_rollout_kernel<CHUNK>'s)
        for (int e = threadIdx.x; e < TILE; e += blockDim.x) {
            float s = 0.0f;
            for (int kk = 0; kk < ae.nw; ++kk) s += lds[(size_t)kk * TILE + e];
            if (tile_env0 + e < ae.n_env)
                ae.out_bldg[(long long)CLO_RESERVED * plane + ((long long)ae.n_chunks * NQ + blockIdx.y) * ae.n_env + tile_env0 + e] = s;
        }
    }
}

}  // namespace
#endif  // __HIPCC__
