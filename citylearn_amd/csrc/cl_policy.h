// cl_policy.h -- mode B with a CLOSED-LOOP policy: the battery + PV K-step loop of cl_rollout_kernel<VEC, false, 2> (cl_rollout.h) whose
// electrical-storage action of every (env, building, step) is a one-hidden-layer tanh MLP over that building's own observation vector, evaluated
// inside the loop from the two observations that depend on the env -- the unit's soc before the step and its net of the previous step, both in
// registers already.  Included by cl_policy.hip (libcitylearn_amd_policy.so, include/citylearn_amd_policy.h) and, for the staged-row layout and the two lean
// entry points' shared host checks, by cl_policy_kpi.hip; behind cl_kernels.hip's helpers.  PolicyArgs, the hidden unit and the Box-Muller draw are
// cl_policy_common.h's, shared with the thermal policy kernel too.
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
#pragma once
#include "cl_policy_common.h"

#ifdef __HIPCC__
namespace {

constexpr int CLPOL_MAX_H = 32;
constexpr int CLPOL_ROW = 3 * CLPOL_MAX_H + 8;       // floats of one building's staged row: [H/4][3][4] weights | bias, mid, half, sigma, low, high, pad x 2

constexpr size_t rollout_policy_lds_floats(int nw, int tile) { return (size_t)nw * NQ * tile + (size_t)nw * 2 * CLPOL_ROW; }

template <int VEC, int PREC>
__global__ void __launch_bounds__(1024) cl_rollout_policy_kernel(const PolicyArgs p) {
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
                if (rkind != CLR_MARL) vstore<VEC>(tb + (long long)CLPOL_T_REWARD * plane, rws);
            }
        }
        if (rkind == CLR_MARL) {
            // the MARL reward couples the buildings through the district net of THIS step: one LDS exchange per step
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
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                q_rw[i] = 0.0f;
#pragma unroll
                for (int m = 0; m < MB; ++m) q_rw[i] += own[m] ? last_rw[m][i] : 0.0f;
            }
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
