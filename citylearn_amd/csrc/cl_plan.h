// cl_plan.h -- which kernels one call of cl_step_f32 / cl_step_flex_f32 / cl_step_observe_f32 launches, as plain values (StepPlan),
// and the kernel_name string of that plan.  Host code only: no HIP header, no device code -- tests/host_shim/step_plan_host.cpp compiles
// it with g++ and checks the selection on a machine without a GPU; cl_kernels.hip (step_impl) launches what plan_step decides.
#pragma once

#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/citylearn_amd.h"

namespace {

thread_local char g_err[512] = {0};

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// The entry points' argument checks (`inline`: not every unit that includes this header calls them).
// cl_dims as every entry point checks it.  `pitch` = false leaves env_pitch to the caller: the policy libraries' entry points take none and
// say so in words of their own, behind their other refusals.
inline int check_dims(const cl_dims* d, bool pitch = true) {
    if (!d) return fail(CL_ENULL, "dims is NULL");
    if (d->n_env <= 0 || d->n_bldg <= 0 || d->n_steps <= 0 || d->n_act_cols < 0)
        return fail(CL_EINVAL, "bad dims: n_env=%d n_bldg=%d n_steps=%d n_act_cols=%d", d->n_env, d->n_bldg,
                    d->n_steps, d->n_act_cols);
    if (d->n_env % 4 != 0) return fail(CL_EALIGN, "n_env=%d must be a multiple of 4 (pad the env batch)", d->n_env);
    if (d->n_ts_rows != 0 && d->n_ts_rows < d->n_steps)
        return fail(CL_EINVAL, "n_ts_rows=%d < n_steps=%d", d->n_ts_rows, d->n_steps);
    if (reinterpret_cast<uintptr_t>(d->env_row0) & 3) return fail(CL_EALIGN, "env_row0 is not 4-byte aligned");
    if (pitch && d->env_pitch != 0 && (d->env_pitch < d->n_env || d->env_pitch % 4 != 0))
        return fail(CL_EINVAL, "env_pitch=%d must be 0 or a multiple of 4 >= n_env=%d", d->env_pitch, d->n_env);
    const uint32_t rk = (d->flags & CLD_REWARD_MASK) >> CLD_REWARD_SHIFT;
    if (rk > CLR_EV) return fail(CL_EINVAL, "unknown reward kind %u", rk);
    // the Philox counter word of the random streams is env_offset + env (32 bits): shards must not alias
    if (d->env_offset < 0 || d->env_offset + (int64_t)d->n_env > (int64_t)1 << 32)
        return fail(CL_ERANGE, "env_offset=%lld with n_env=%d leaves the 32-bit env index of the random streams", (long long)d->env_offset, d->n_env);
    return CL_OK;
}

// cl_dims.env_pitch (0 = n_env); entry points that do not implement a pitch refuse one
inline int pitch_of(const cl_dims* d) { return d->env_pitch ? d->env_pitch : d->n_env; }
inline int no_pitch(const cl_dims* d, const char* who) {
    if (pitch_of(d) != d->n_env) return fail(CL_EINVAL, "%s: env_pitch=%d != n_env=%d is not implemented for this call", who, d->env_pitch, d->n_env);
    return CL_OK;
}

inline int check_ptr(const void* p, const char* name, bool required = true) {
    if (!p) return required ? fail(CL_ENULL, "%s is NULL", name) : CL_OK;
    if (reinterpret_cast<uintptr_t>(p) & 15) return fail(CL_EALIGN, "%s is not 16-byte aligned", name);
    return CL_OK;
}

constexpr int CL_OBS_FUSED_BLDG = 32;          // buildings a fused observation list can address (= the lean kernel's 2 x 16)
// largest launch (env x building units) whose plane stores carry the non-temporal hint (see pstore)
constexpr long long CL_NT_MAX_UNITS = 3ll << 20;
constexpr long long CL_NT_STREAM_UNITS = 16ll << 20;      // ... and the smallest streaming-regime launch that takes it again
constexpr int CL_LP_WORDS = (CLP_F_LAST - CLP_F_FIRST + 1) + CL_NF;      // 64 + 16 staged words per building (cl_full.h LP)
#ifdef CL_TRACE                  // the stamps need a few registers: five waves per SIMD (what the 9-building launch holds) instead of six
constexpr int CL_FULL1_WPE = 5;
#else
constexpr int CL_FULL1_WPE = 6;  // waves per SIMD of the one-env-per-lane thermal kernel (cl_step_full_kernel<1, false, 1024, WPE, false>)
#endif

// Launch geometry.  Measured on MI355X (scripts/tune.py, profiles/): at ~1M units per launch the 16-wave
// workgroup with 16-byte accesses (1 workgroup per CU, every wave one memory round trip) is fastest; the
// full (thermal) kernel needs too many registers for VEC > 1.
int pick_nw(int n_bldg, int /*vec*/) {
    const int rounds = (n_bldg + 15) / 16;
    int nw = (n_bldg + rounds - 1) / rounds;
    if (n_bldg > 16 && n_bldg <= 32) nw = 16;            // e.g. 17 buildings: 16 waves, wave 0 takes two
    return nw;
}

// envs per lane: wide (16 B) accesses once the batch is large enough to still give every CU a workgroup
int pick_vec(int n_env, int n_bldg, bool unit_stride) {
    if (!unit_stride) return 1;
    // the narrowest pack that still gives at most one workgroup per CU (the lean kernels' launch shape): 49 152 envs at two envs per
    // lane were 384 workgroups -- the general kernel, 9.8 us -- and are 192 latency-ordered ones at four (scripts/step_observe_bench.py)
    if (n_env > 256 * 128) return 4;
    if (n_env > 256 * 64) return 2;
    (void)n_bldg;
    return 1;
}

// The step kernel families; each name below is the kernel of that family for the plan's precision and form.
enum StepKernel {
    CLK_STEP,          // cl_step_kernel<VEC, FULL, DETAIL, FLEX, PREC, FOLD[, CHECK]>
    CLK_LEAN_CHUNK,    // cl_step_lean_chunk_kernel<VEC, NT, FOLD, PREC>
    CLK_LEAN,          // cl_step_lean[_kpi | _obs][_f64 | _chain]_kernel<VEC, [FLEX, ]NT>
    CLK_ENVMAJOR,      // cl_step_envmajor_kernel<NB, NT, VEC, PREC>
    CLK_FULL,          // cl_step_full[_chain]_kernel<VEC, DETAIL, MAXT, WPE, LP, NT>, cl_step_full_obs_kernel<PREC, NT>, cl_step_full_kpi_kernel<NT>
    CLK_FULL_TP,       // cl_step_full_tp[_chain]_kernel<VEC, WPE, NT>, cl_step_full_tp_obs_kernel<VEC, PREC, NT>  (extra argument: tp_tiles)
};
enum StepForm { CLF_PLAIN, CLF_OBS, CLF_KPI };     // OBS: the launch writes the compact observation (ObsFusedArgs); KPI: the streaming KPI accumulators

struct StepPlan {
    StepKernel kernel;
    StepForm form;
    int vec;                          // VEC (envs per lane)
    int nt;                           // NT: non-temporal plane stores (StepArgs.nt)
    int prec;                         // PREC: 0 = fp32 map, 1 = CLD_F64_MAPS, 2 = CLD_F64_CHAIN
    bool full, det, flex, fold, check;          // cl_step_kernel: FULL, DETAIL, FLEX, FOLD, CHECK (det: also cl_step_full*; fold: also the lean chunk kernel)
    bool lp;                          // cl_step_full*_kernel: parameter blocks staged in LDS
    int maxt, wpe;                    // cl_step_full*_kernel: MAXT, WPE (the multi-tile kernels: WPE)
    int nb;                           // cl_step_envmajor_kernel: NB
    bool strips;                      // cl_step_lean_chain_kernel<4, ..>, uniform body: the building beyond the waves goes to the last four waves as 64-env strips
    unsigned grid_x, grid_y, block;   // launch shape (block: threads)
    size_t lds;                       // dynamic LDS bytes
    int nw, b_chunk, n_chunks, fused_finish;    // the StepArgs fields the selection sets
    int tp_tiles;                     // CLK_FULL_TP: env tiles per workgroup
    int flex_vec, flex_nt;            // cl_flex_kernel<VEC, NT> ahead of the step launch (flex_vec = 0: no flexible loads) ...
    unsigned flex_grid_x;             // ... over flex_grid_x env tiles
    bool finish;                      // follow-ups: cl_finish_kernel (chunk sums not folded by the step launch),
    bool marl;                        //   cl_marl_reward_kernel (building-chunked MARL),
    int kpi_passes;                   //   0 = none, 1 = cl_kpi_kernel, 2 = cl_kpi_bldg_kernel + cl_kpi_env_kernel
};

// The step path's kernel selection.  `flex`: flexible-load tables are present (cl_step_flex_f32); `obs`: cl_step_observe_f32 asks for the compact
// observation (`obs_lean_ok`: the battery + PV launch can fill it, `obs_pitch`: its row pitch).  Returns CL_OK or the refusal (cl_last_error).
int plan_step(StepPlan& p, const cl_dims& d, const cl_tuning& tun, int64_t act_stride_env, bool flex, bool obs, bool obs_lean_ok, int obs_pitch) {
    // (`obs`: the compact observation the step launch may write itself -- the battery + PV kernels under their own limits (`obs_lean_ok`), the thermal
    //  kernels of cl_full.h for any listed battery / tank / net / reward column)
    const bool of = obs && obs_lean_ok;
    p = StepPlan{};
    const int rkind_host = (d.flags & CLD_REWARD_MASK) >> CLD_REWARD_SHIFT;
    // non-temporal plane stores while the launch's footprint (~40 - 60 B per (env, building) unit) stays inside the Infinity Cache
    // ... and again once it is several times that cache (17 x 1 048 576: 125 -> 115 us, 17 x 1 572 864: 196 -> 170 us): nothing of a step
    // survives in the cache until the next one anyway, and the hint keeps the stores from displacing what the step still reads.  In
    // between (footprint of the order of the cache: 17 x 262 144 +10 %, 17 x 524 288 +-4 %) plain stores win.
    const long long nt_units = (long long)d.n_env * d.n_bldg;
    p.nt = tun.nt_stores == 1 || (tun.nt_stores == 0 && (nt_units <= CL_NT_MAX_UNITS || nt_units >= CL_NT_STREAM_UNITS));
    if (flex) {
        // four envs per lane once there are enough envs to fill the chip that way (and plane rows stay 16-byte aligned)
        const int fvec = tun.flex_vec ? tun.flex_vec : d.n_env >= 16384 ? 4 : 1;
        p.flex_grid_x = (unsigned)((d.n_env + 64 * fvec - 1) / (64 * fvec));
        p.flex_vec = fvec == 4 || fvec == 2 ? fvec : 1;
        p.flex_nt = p.nt;
    }
    if ((tun.lean_variant >> 2) & 1) return fail(CL_EINVAL, "cl_tuning.lean_variant = %d: bit 4 (lean districts through the thermal kernel) is not implemented", tun.lean_variant);
    const bool full = !(d.flags & CLD_LEAN) || (d.flags & CLD_WRITE_DETAIL);
    p.nw = tun.nw ? tun.nw : pick_nw(d.n_bldg, 1);
    // general kernel: two buildings per wave measured fastest for the 6..16-building thermal schemas (fewer, longer waves)
    if (!tun.nw && full && d.n_bldg >= 6 && d.n_bldg <= 16) p.nw = (d.n_bldg + 1) / 2;
    const bool will_chunk = d.n_bldg > 32 && !tun.no_chunks;
    int vec = full ? 1 : pick_vec(d.n_env, d.n_bldg, act_stride_env == 1);
    if (will_chunk && act_stride_env == 1) {               // few envs, many buildings: width from the unit count
        const long long units = (long long)d.n_env * d.n_bldg;
        // (under the float64 chain the four-env pack pays off one octave later -- scripts/r06_cliffs.py, profiles/r06c_cliffs_chain.jsonl: 33 x 16 384 and
        //  128 x 4 096, both 2^19 units, 13.8 / 12.6 us at four envs per lane against 12.2 / 9.8 us at one)
        const long long lean4 = (d.flags & CLD_F64_CHAIN) ? (1ll << 20) : (1ll << 19);
        vec = full ? (units >= (1ll << 19) && d.n_env >= 256 ? 2 : 1) : (units >= lean4 && d.n_env >= 512 ? 4 : 1);
        // (chain, districts just beyond the 32-building limit of the one-row kernels on batches of >= 2048 one-env tiles: two rows of ~17 buildings at four
        //  envs per lane leave every wave one or two buildings behind a long load chain -- 33 x 262 144: 117.5 us against 74 us for the UNCHUNKED general
        //  kernel at one env per lane, which the grid rule below selects by itself once the tile count reaches 2048; profiles/r06d_cliffs_chain.jsonl)
        if (!full && (d.flags & CLD_F64_CHAIN) && d.n_bldg <= 40 && d.n_env >= 131072) vec = 1;
    }
    if (tun.vec) vec = tun.vec;
    // CLD_F64_MAPS: the battery map in float64 -- general and lean step kernels at one or two envs per lane (a double is two VGPRs)
    const bool f64 = d.flags & CLD_F64_MAPS;
    // CLD_F64_CHAIN: the soc chain in float64 on the default three state planes (cl_unit.h battery_charge_chain) -- lean, env-major, general and
    // thermal-specialised step kernels
    const bool chain = d.flags & CLD_F64_CHAIN;
    if (chain) {
        if (f64) return fail(CL_EINVAL, "CLD_F64_CHAIN and CLD_F64_MAPS are two precision models of the same map: pick one");
        if (flex) return fail(CL_EINVAL, "CLD_F64_CHAIN is not implemented for districts with flexible loads (the EV batteries of cl_flex_kernel are fp32)");
        // (streaming KPIs without the detail planes: the lean step launch updates them itself under the chain too; a thermal district needs the planes)
        if ((d.flags & CLD_KPI) && !(d.flags & CLD_WRITE_DETAIL) && (full || d.n_bldg > 32))
            return fail(CL_EINVAL, "CLD_F64_CHAIN with CLD_KPI needs CLD_WRITE_DETAIL (except for battery + PV districts of up to 32 buildings)");
        if (full) vec = 1;                     // (the thermal unit around the float64 chain spills at two envs per lane)
    }
    if (f64) {
        if (flex) return fail(CL_EINVAL, "CLD_F64_MAPS is not implemented for districts with flexible loads (the EV batteries of cl_flex_kernel are fp32)");
        if ((d.flags & CLD_KPI) && !(d.flags & CLD_WRITE_DETAIL)) return fail(CL_EINVAL, "CLD_F64_MAPS with CLD_KPI needs CLD_WRITE_DETAIL");
        vec = full ? 1 : (vec > 2 ? 2 : vec);          // (the thermal unit with a float64 battery spills at two envs per lane)
    }
    if (flex && vec > 2 && !(!full && d.n_bldg <= 2 * p.nw && !will_chunk && (d.n_env + 64 * vec - 1) / (64 * vec) <= 256 && !(tun.lean_variant & 1)))
        vec = 2;                             // general-kernel FLEX instantiations exist for 1 and 2 envs per lane
    const int tile = 64 * vec;
    const unsigned grid_x = (unsigned)((d.n_env + tile - 1) / tile);
    // Large districts (e.g. 1024 buildings x 1024 envs per GPU): a 1-D grid over env tiles would leave most CUs idle, so
    // the buildings are cut into chunks along gridDim.y and the district sums are finished by a second tiny kernel.
    p.b_chunk = d.n_bldg; p.n_chunks = 1;
    if (d.n_bldg > 32 && grid_x < 2048 && !tun.no_chunks) {
        long long r = ((long long)d.n_bldg * grid_x) / (16ll * 2048);
        if (r < 1) r = 1;
        // about one 16-wave workgroup per CU when the launch is small: the 1024 x 1024 thermal shard at two envs per lane then gives
        // every wave two buildings (32 chunks x 8 env tiles = 256 workgroups, all resident at once): 16.0 vs 18.0 us with one
        // building per wave in two generations (scripts/c4_sweep.py, profiles/r02_c4_chunk_sweep.log)
        const long long per_cu = ((long long)d.n_bldg * grid_x + 2048) / 4096;
        if (per_cu >= 2 && r < 2) r = 2;
        // (round 5) the thermal kernel with staged parameter blocks (cl_full.h LP) on batches of several workgroup generations: FEWER, LARGER
        // chunks -- one or two workgroups per CU, each wave walking 8 - 16 buildings -- instead of eight generations of two buildings per
        // wave.  1024 buildings (scripts/gpurun/r05_call12.sh, profiles/r05m_*): x 8192 envs 103.0 / 95.3 / 91.4 / 91.6 us with chunks of
        // 32 / 64 / 128 / 256; x 4096: 55.0 / 50.9 / 48.7 / 78.4 (128 workgroups leave half the CUs idle); x 2048: 26.6 / 30.1 / 36.4 / 61.0
        // and x 1024: 13.2 / 21.5 / 34.5 / 60.2 -- those stay at 32.  (Battery + PV districts, cl_step_kernel: 32 stays best, 8192 envs:
        // 63.8 / 60.3 / 64.9 / 67.4 us with 24 / 32 / 48 / 64.)
        const bool lp_shape = !(d.flags & CLD_LEAN) && !flex && !(d.flags & (CLD_WRITE_DETAIL | CLD_F64_MAPS)) && vec == 2 &&
                              tun.full_variant != 1 && tun.full_variant != 3;
        if (lp_shape && d.n_bldg >= 256 && (long long)d.n_bldg * grid_x >= 32ll * 1024) {     // (measured on 1024 buildings; smaller districts keep the rule above)
            long long want = ((long long)d.n_bldg * grid_x + 255) / 256;          // buildings per chunk for 256 workgroups ...
            r = 2; while (16 * r < want && r < 8) r *= 2;                            // ... as a power of two, 128 at most (40 KB of staged blocks)
        }
        // (round 6) the thermal kernel around the float64 chain (one env per lane, parameter blocks through the constant cache): ONE workgroup per CU --
        // 256 workgroups, chunks of up to 256 buildings.  1024 buildings x 1024 / 2048 / 4096 / 8192 envs with chunks of 32 / 64 / 128 / 256:
        // 20.2 / 17.7 / 27.4 / 47.6, 37.4 / 33.5 / 31.3 / 48.8, 71.3 / 68.7 / 67.5 / 65.8, 149.7 / 137.3 / 129.5 / 125.4 us
        // (scripts/gpurun/r06_call15.sh, profiles/r06o_*).
        const bool chain_full_shape = chain && !(d.flags & CLD_LEAN) && !flex && !(d.flags & (CLD_WRITE_DETAIL | CLD_F64_MAPS)) && tun.full_variant != 1;
        // 128 .. 1024 buildings x 1024 .. 65 536 envs (scripts/r06_chunk_sweep.py, profiles/r06p_chunks_*.jsonl): the rule is within 3 % of the best chunk size
        // of every cell -- 128 x 16 384 36.4 -> 25.6 us, 256 x 16 384 66.9 -> 49.2, 512 x 16 384 153 -> 126, 1024 x 16 384 317 -> 249 (chunks as large as
        // the district = one workgroup row, no second launch)
        if (chain_full_shape && d.n_bldg >= 128 && (long long)d.n_bldg * grid_x >= 16ll * 1024) {
            const long long want = ((long long)d.n_bldg * grid_x + 255) / 256;
            r = 2; while (16 * r < want && r < 16) r *= 2;
        }
        // (fp32 map, same sweep: up to 256 buildings x 65 536 envs in ONE workgroup row -- 128 buildings 113 -> 98 us, 256 buildings 204 -> 182 us; at
        //  16 384 envs the chunked launch stays ahead, 29.0 vs 32.4 and 49.0 vs 59.1 us)
        if (lp_shape && d.n_bldg <= 256 && grid_x >= 512) r = 16;
        // ... whose plane stores take the non-temporal hint at every batch size (the footprint rule above is the battery + PV kernels': 1024 x
        // 8192 envs 101.2 -> 100.0 us, x 4096 54.3 -> 53.3 us, chunks of 128: 91.4 -> 89.1 us; profiles/r05l_*, r05m_*)
        if (lp_shape && tun.nt_stores == 0) p.nt = 1;
        p.b_chunk = tun.b_chunk > 0 ? tun.b_chunk : (int)(16 * r);
        p.n_chunks = (d.n_bldg + p.b_chunk - 1) / p.b_chunk;
        if (tun.b_chunk <= 0 && p.n_chunks > 1) {
            // balanced chunks (round 6): 33 buildings were cut 16 + 16 + 1 -- a third workgroup row per env tile for one building; now round(33 / 16) = 2
            // rows of 17 (one wave of the sixteen walks two buildings).  Districts that divide evenly (1024 / 32) keep their geometry.
            const int nc = (int)((2ll * d.n_bldg + p.b_chunk) / (2ll * p.b_chunk));       // round(n_bldg / b_chunk)
            if (nc >= 2) { p.n_chunks = nc; p.b_chunk = (d.n_bldg + nc - 1) / nc; p.n_chunks = (d.n_bldg + p.b_chunk - 1) / p.b_chunk; }
        }
        if (p.n_chunks == 1) p.b_chunk = d.n_bldg;
        else p.nw = (tun.b_chunk > 0 && tun.nw > 0) ? tun.nw : 16;
        // the reserved plane holds the chunk partial sums (twice under the deferred finish), the tickets of the in-launch fold and, in its
        // last 16 bytes, the marker words EVERY chunked launch touches (a non-deferring one clears its step's marker)
        // (the second buffer only where the launch can defer at all: finish = 3 on a launch that keeps the second cl_finish launch needs one)
        const long long scratch_words = (long long)p.n_chunks * CL_NQ * d.n_env + (d.n_env + 63) / 64 + 4;
        if (scratch_words > (long long)d.n_bldg * d.n_env)
            return fail(CL_EINVAL, "b_chunk=%d leaves no room for the %d chunk partial sums, their tickets and the marker words", p.b_chunk, p.n_chunks);
    }
    if (p.n_chunks > 1 && rkind_host == CLR_EV)
        return fail(CL_EINVAL, "reward kind CLR_EV is not implemented for building-chunked launches (n_bldg=%d)", d.n_bldg);
    // Deferred finish (cl_tuning.finish = 3): the launch folds the PREVIOUS step's chunk sums and leaves its own for the next launch or for
    // cl_finish_f32 (district_reduce).  Only where nothing of the path reads out_env inside the step: no coupled reward (MARL's per-building
    // rewards need the district net of the same step, reward_function.py:132-143; the EV reward likewise), no streaming KPIs, no flexible
    // loads, and the kernels that carry the fold (the FOLD instantiations below); a 16-wave workgroup folds at most 64 district sums of at most 64 chunks, 1024 partial sums in all,
    // and the reserved plane has to hold both buffers and the marker words.  Anything else keeps the second launch.
    const int fold_per_row = p.n_chunks > 1 ? (CL_NQ * tile + p.n_chunks - 1) / p.n_chunks : 0;
    // (battery + PV districts keep the 16-sum limit: where more sums per row would be needed -- 1024 x 4096 / 8192 envs at four envs per lane --
    //  the folding instantiation's 107 registers cost more than the second launch: 32.8 vs 32.0 us, 65.2 vs 61.3 us, profiles/r05n_*)
    const int fold_w = fold_per_row <= 16 ? 16 : fold_per_row <= 32 ? 32 : 64;          // row width of the exchange tile (fold_shift)
    const bool can_defer = p.n_chunks > 1 && tun.finish == 3 && rkind_host != CLR_MARL && rkind_host != CLR_EV && !flex &&
                           !(d.flags & (CLD_KPI | CLD_F64_MAPS | CLD_WRITE_DETAIL)) && (!chain || !full) &&      // (the float64 chain: the battery + PV chunk kernel carries the fold; the thermal chain kernel does not)
                           fold_per_row <= (full ? 64 : 16) && p.n_chunks * fold_w <= 1024 &&
                           p.nw == 16 && p.n_chunks <= 64 &&
                           2ll * p.n_chunks * CL_NQ * d.n_env + (d.n_env + 63) / 64 + 4 <= (long long)d.n_bldg * d.n_env;
    const bool det = d.flags & CLD_WRITE_DETAIL;
    // streaming KPIs of thermal / outage districts (and of any district stepped with detail planes) inside the step launch:
    // cl_step_full_kpi_kernel (cl_full.h); cl_tuning.kpi_passes = 1 keeps the separate cl_kpi_kernel pass (A/B), 2 the two round-1 passes
    // (up to 128 buildings: their baselines of one env tile sit in LDS, 256 B per building)
    const bool kpi_full = (d.flags & CLD_KPI) && full && !flex && !f64 && !chain && p.n_chunks == 1 && vec == 1 && tun.full_variant != 1 && tun.kpi_passes == 0 &&
                          d.n_bldg <= 128;
    // ... whose waves should all be resident at once (16 per CU at its 119 registers): as many waves per workgroup as that allows, at least
    // two (9 x 65 536: four waves 18.8 us, the step-only default of five -- two generations -- 23.6 us; profiles/r03_kpi_in_step_probe.log)
    if (kpi_full && !tun.nw) {
        const long long fit = (16ll * 256) / grid_x;
        p.nw = (int)(fit < 2 ? 2 : fit > 16 ? 16 : fit);
        if (p.nw > d.n_bldg) p.nw = d.n_bldg;
    }
    // thermal kernel with the parameter blocks of the workgroup's buildings staged in LDS
    // (for the building-chunked launches only -- a workgroup of the 9 x 65 536 launch would wait for the staging round trip before it
    //  can issue its plane loads, while its scalar reads hit the constant cache: 10.7 vs 8.7 us; full_variant = 2 forces it, 3 forbids it)
    // (not under the float64 chain unless forced: its one-env-per-lane thermal kernel reads the blocks through the constant cache faster -- chunked 1024-,
    //  512-, 256-building districts 1.06 - 1.21 x, profiles/r06c_cliffs_chain.jsonl -- and a 512-building chunk's 160 KB of staged blocks do not exist)
    const bool lp = full && !flex && !det && !f64 && tun.full_variant != 1 && tun.full_variant != 3 && vec <= 2 &&
                    ((p.n_chunks > 1 && !chain) || tun.full_variant == 2) && (size_t)p.b_chunk * CL_LP_WORDS * sizeof(uint32_t) <= 96 * 1024;
    const size_t lds = (size_t)p.nw * CL_NQ * tile * sizeof(float) + (lp ? (size_t)p.b_chunk * CL_LP_WORDS * sizeof(uint32_t) : 0) +
                       (can_defer ? 1024 * sizeof(float) : 0);          // (+ the [chunks][16 / 32 / 64 sums] exchange tile of the deferred fold)
    // Thermal districts whose batch can be cut into ONE 16-wave workgroup per CU: a workgroup takes `tiles` 128-env tiles (two envs per
    // lane) and deals its tiles x B (tile, building) items to the 16 waves in order (cl_step_full_tp_kernel) -- the items divide over
    // the four SIMDs where the B buildings of one tile do not, and the whole launch is resident at once.  scripts/tp_sweep.py,
    // scripts/tp_sweep2.py (profiles/r02_tp_sweep*.log), one-tile kernel -> this one: 9 x 65 536 8.5 -> 7.7 us, 9 x 131 072 17.3 -> 14.3,
    // 9 x 262 144 29.4 -> 28.0, 12 x 65 536 11.8 -> 9.2, 16 x 65 536 13.4 -> 11.7, 6 x 65 536 7.0 -> 6.6, 3 x 262 144 11.9 -> 10.7; with
    // fewer than ~12 items per workgroup (3 x 65 536) or with more / fewer workgroups than CUs the one-tile kernel wins and stays.
    // full_variant: 5 forces it (tun.vec = envs per lane, tun.nw = waves, tun.b_chunk = tiles), 3 forbids it.
    const bool tp_forced = tun.full_variant == 5;
    // small batches (193 .. 256 one-env-per-lane tiles, i.e. up to 16 384 envs): one tile per workgroup, one WAVE per building --
    // 9 x 16 384 5.62 -> 5.01 us, 6 x 16 384 5.50 -> 4.41, 12 x 16 384 6.15 -> 5.25, 16 x 16 384 6.26 -> 5.84 (scripts/tp_small_probe.py)
    const unsigned tiles1 = (unsigned)((d.n_env + 63) / 64);
    const bool tp_small = !tp_forced && tiles1 > 192 && tiles1 <= 256 && d.n_bldg >= 6 && d.n_bldg <= 16;
    const int tp_vec = (tp_forced && tun.vec == 1) || tp_small || chain ? 1 : 2;       // (the float64 chain spills at two envs per lane)
    const int tp_auto_tiles = tp_small ? 1 : (int)((d.n_env + 256 * 64 * tp_vec - 1) / (256 * 64 * tp_vec));      // one workgroup per CU
    // (chain, round 6: where one workgroup per CU would need more tiles than LDS holds -- 17 / 20 thermal buildings x 262 144 envs -- four tiles per
    //  workgroup in several generations still beat the one-tile kernel 1.36 x / 1.16 x: profiles/r06c_cliffs_chain.jsonl)
    const size_t tp_tile_bytes = ((size_t)d.n_bldg * CL_NQ + 1) * 64 * tp_vec * sizeof(float);
    const bool tp_capped = chain && !tp_forced && !tp_small && (size_t)tp_auto_tiles * tp_tile_bytes > 150 * 1024 && 4 * tp_tile_bytes <= 150 * 1024 && d.n_bldg >= 6;
    const int tp_tiles = tp_forced ? (tun.b_chunk > 0 ? tun.b_chunk : CL_ROW0_BLOCK / (64 * tp_vec)) : tp_capped ? 4 : tp_auto_tiles;
    const int tp_nw = tp_forced && tun.nw ? tun.nw : (tp_small ? d.n_bldg : 16);
    const unsigned tp_grid = (unsigned)((d.n_env + tp_tiles * 64 * tp_vec - 1) / (tp_tiles * 64 * tp_vec));
    const size_t tp_lds = ((size_t)tp_tiles * d.n_bldg * CL_NQ + tp_tiles) * 64 * tp_vec * sizeof(float);
    bool tp_kernel = full && !flex && !(d.flags & CLD_WRITE_DETAIL) && !kpi_full && p.n_chunks == 1 && d.n_bldg <= 32 && tp_lds <= 150 * 1024 &&
                     (!d.env_row0 || CL_ROW0_BLOCK % (tp_tiles * 64 * tp_vec) == 0);    // one episode offset per workgroup: no workgroup straddles two blocks
    if (tp_forced) {
        if (!tp_kernel || tp_nw > 16)
            return fail(CL_EINVAL, "full_variant = 5: %d tiles x %d envs per lane x %d waves is not a launch of cl_step_full_tp_kernel for this district", tp_tiles, tp_vec, tp_nw);
    } else tp_kernel = tp_kernel && tun.full_variant == 0 && !tun.vec && !tun.nw && (tp_small || tp_tiles * d.n_bldg >= 12) && ((tp_grid > 192 && tp_grid <= 256) || tp_capped);
    // (up to 480 workgroups -- two 9-wave workgroups per CU are resident at once, so up to 512 the launch is still ONE generation: re-measured
    //  at the end of round 5, after the latency-ordered kernel lost the non-temporal hint on its loads (scripts/gpurun/r05_call24.sh,
    //  profiles/r05_nt_loads/r05y.log), 17 buildings x 98 304 / 106 496 / 114 688 / 131 072 / 163 840 / 196 608 / 262 144 envs: 10.6 / 11.0 /
    //  11.8 / 15.5 / 19.2 / 22.6 / 31.7 us against 13.2 / 13.2 / 13.5 / 15.6 / 19.2 / 21.3 / 26.2 us for the env-major kernel -- the old rule
    //  (352 workgroups, env-major from 106 496 envs) had the general kernel at 98 304 envs, 13.0 us)
    // streaming KPIs without the detail planes: the lean kernel updates the per-building accumulators itself, at any grid size
    const bool kpi_lean = (d.flags & CLD_KPI) && !(d.flags & CLD_WRITE_DETAIL) && !kpi_full;
    // cl_step_observe_f32 on a thermal / outage district: the step launch fills the compact observation itself (cl_full.h OBS) where it is one
    // workgroup row of the one-env-per-lane kernel or the multi-tile kernel, without detail planes / KPIs / a coupled reward
    const bool obs_full = obs && full && !flex && !det && !f64 && !(d.flags & CLD_KPI) && p.n_chunks == 1 && rkind_host != CLR_MARL && tun.obs_variant == 0;
    // Env-major or building-major above one wave generation?  Re-measured in round 6, both kernels alternating in ONE process (scripts/r06_lean_vs_envmajor.py,
    // profiles/r06_lean_vs_envmajor*.log; a process lands in a +- 4 % band, which is what hid this in round 5):
    //  * the env-major kernel wins where the step's footprint is of the order of the Infinity Cache -- 17 x 262 144: 25.8 / 30.7 us (fp32 / chain) against 27.9 /
    //    32.2 for the latency-ordered building-major kernel at four envs per lane; 9 x 262 144: 16.1 / 18.8 against 19.2 / 21.4;
    //  * far beyond the cache the building-major kernel's 16-byte accesses win again: 17 x 1 048 576 -- the HBM-true shape of the bench line -- 104.6 - 111.8 us
    //    against 113.5 - 127.6 us (fp32) and 113.5 - 120.4 against 125.6 - 134.4 (chain) in three processes, 17 x 2 097 152 222 - 224 / 236 against 225 - 247 /
    //    245 - 261, 20 x 1 048 576 (fp32) 126 - 129 against 133 - 140;
    //  * under the float64 chain the building-major kernel holds on longer below: 17 x 147 456 / 163 840 / 180 224 20.5 / 21.8 / 22.8 us against 23.4 / 24.2 /
    //    25.2 (196 608: 24.4 - 25.6 against 25.8 - 26.5; 229 376: even); 9 and 6 buildings: 131 072 envs 10.1 / 7.6 against 11.1 / 8.6, even or behind from 147 456.
    //  * (scripts/r06_stream_map.py, 6 .. 20 buildings x 393 216 .. 2 097 152 envs, five variants side by side, medians of three rounds; profiles/r06_stream_map*.jsonl)
    //    from 12 buildings and 8 Mi units the building-major kernel WITH non-temporal stores is the best or within 3 % of it in 25 of 30 cells -- 12 x 786 432 /
    //    1 048 576: 57.0 / 75.0 us against 62.8 / 84.3 (fp32), 57.0 / 75.0 against 68.9 / 94.0 (chain); 20 x 524 288 / 786 432 (fp32): 61.2 / 93.2 against 72.8 / 106.9;
    //    6 and 9 buildings are mixed and keep the env-major kernel.
    const bool stream_lean = d.n_bldg >= 12 && (long long)d.n_bldg * d.n_env >= (8ll << 20);
    const int em_min = !chain ? 122880 : d.n_bldg >= 16 ? 196608 : 131072;
    const bool em_auto = d.n_env > em_min && !(chain && d.n_bldg > 17) && !stream_lean;
    const bool lean_beyond = tun.envmajor == 0 && !full && d.n_bldg <= 20 && d.n_env > 122880 && !em_auto;      // (what the env-major rule no longer takes)
    const bool lean_shape = p.n_chunks == 1 && d.n_bldg <= 2 * p.nw && (grid_x <= 480 || (tun.lean_variant & 2) || kpi_lean || lean_beyond) &&
                            !((tun.lean_variant & 1) && !kpi_lean);
    if (lean_beyond && stream_lean && lean_shape && tun.nt_stores == 0) p.nt = 1;      // (8 .. 16 Mi units: the footprint rule above says plain stores -- measured on the env-major kernel)
    // without the detail planes only cl_step_lean_kpi_kernel updates the per-building accumulators (and writes the baseline plane
    // cl_kpi_env_kernel sums): a launch shape that cannot take it must not silently leave them stale
    if (kpi_lean && (full || flex || !lean_shape))
        return fail(CL_EINVAL, "CLD_KPI without CLD_WRITE_DETAIL needs a step launch that updates the accumulators itself (battery + PV: n_bldg=%d <= 2 x nw=%d "
                               "waves, no chunks; thermal: one env per lane, no chunks, no flexible loads, no CLD_F64_MAPS): drop the cl_tuning override or set CLD_WRITE_DETAIL",
                    d.n_bldg, p.nw);
    // (chain: the 20-building instantiation holds 140 registers -- three waves per SIMD -- and loses to the building-major kernel, 41.6 vs 33.6 us at
    //  20 x 262 144: only districts of up to 17 buildings go env-major by themselves; profiles/r06c_cliffs_chain.jsonl)
    const bool envmajor_shape = !full && p.n_chunks == 1 && d.n_bldg <= 20 && !kpi_lean &&
                                (tun.envmajor == 1 || (tun.envmajor == 0 && em_auto));

    // the launch: defaults of the common shape, then the kernel family
    p.prec = chain ? 2 : f64 ? 1 : 0;
    p.vec = vec; p.full = full; p.det = full && det; p.flex = flex;
    p.grid_x = grid_x; p.grid_y = (unsigned)p.n_chunks; p.block = 64 * p.nw; p.lds = lds;
    const bool lean_obs = of && rkind_host != CLR_MARL;      // (MARL's reward plane is finished after the sweep the tile is filled in)
    auto set_lean = [&](int lean_vec) -> int {       // the latency-ordered battery + PV kernels (two buildings per wave at most)
        if (lean_vec != 1 && lean_vec != 2 && lean_vec != 4) return fail(CL_EINVAL, "bad vec %d", lean_vec);
        p.kernel = CLK_LEAN; p.vec = lean_vec;
        p.form = kpi_lean ? CLF_KPI : lean_obs ? CLF_OBS : CLF_PLAIN;
        // + one baseline value per building / the observation tile
        p.lds = lds + (kpi_lean ? CL_OBS_FUSED_BLDG * sizeof(float) : lean_obs ? (size_t)tile * obs_pitch * sizeof(float) : 0);
        // One building more than waves under the uniform body of the plain chain launch at four envs per lane (17 buildings, 16 waves: the headline):
        // the last four waves -- one per SIMD -- take the extra building as four 64-env strips instead of wave 0 taking a second tile
        // (csrc/cl_kernels.hip lean_step_body, STRIPS).  Their district partials go to one more LDS row: 17 x 4 x 256 x 4 = 69 632 bytes at 16 waves,
        // beyond the 64 KB a kernel gets without opting in (the launcher opts in and refuses a request beyond a CU's LDS).
        // cl_tuning.lean_variant & 32 keeps wave 0's second tile (tests, A/B).
        p.strips = chain && p.form == CLF_PLAIN && lean_vec == 4 && (d.flags & CLD_LEAN_UNIFORM) && act_stride_env == 1 && p.nw >= 4 &&
                   d.n_bldg == p.nw + 1 && !(tun.lean_variant & 32);
        if (p.strips) p.lds += (size_t)CL_NQ * 64 * lean_vec * sizeof(float);
        return CL_OK;
    };
    auto set_full = [&](int maxt, int wpe, bool lp_k) { p.kernel = CLK_FULL; p.maxt = maxt; p.wpe = wpe; p.lp = lp_k; };
    auto set_full_obs = [&] {                         // the thermal kernels that write the compact observation themselves (cl_full.h OBS)
        p.kernel = CLK_FULL; p.form = CLF_OBS; p.lds = lds + (size_t)64 * obs_pitch * sizeof(float);
    };
    // thermal districts, several env tiles per workgroup (cl_step_full_tp_kernel's launch shape); forced: tun.vec = envs per lane, tun.nw = waves,
    // tun.b_chunk = tiles.  The observation tile joins the launch where it fits (a tile that does not fit: the two launches)
    auto set_tp = [&] {
        p.kernel = CLK_FULL_TP; p.vec = tp_vec; p.wpe = 4; p.nw = tp_nw; p.tp_tiles = tp_tiles;
        p.grid_x = tp_grid; p.grid_y = 1; p.block = 64 * tp_nw; p.lds = tp_lds;
        const size_t obs_lds = (size_t)tp_tiles * 64 * tp_vec * obs_pitch * sizeof(float);
        if (obs_full && tp_lds + obs_lds <= 150 * 1024) { p.form = CLF_OBS; p.lds += obs_lds; }
    };
    auto set_lean_chunk = [&] {                       // building-chunked battery + PV districts: the latency-ordered chunk kernel (deferred fold where it applies)
        p.kernel = CLK_LEAN_CHUNK; p.fold = can_defer; p.fused_finish = can_defer ? 2 : 0;
    };
    // (lean_variant & 16 keeps cl_step_kernel: tests, A/B)
    const bool lean_chunk = !full && p.n_chunks > 1 && tun.finish != 2 && (vec == 1 || vec == 2 || vec == 4) && !(tun.lean_variant & 16);
    if (d.flags & CLD_CHECK) {
        // debug mode: the general kernel with the reference's assertions compiled in, one env per lane (include/citylearn_amd.h CLD_CHECK)
        if (!det || (d.flags & CLD_DETAIL_MIN) || p.n_chunks > 1 || kpi_full)
            return fail(CL_EINVAL, "CLD_CHECK needs CLD_WRITE_DETAIL (all planes), a district of up to 32 buildings (the violation words use the reserved plane) "
                                   "and, with CLD_KPI, the separate KPI launch (cl_tuning.kpi_passes = 1)");
        p.kernel = CLK_STEP; p.check = true; p.vec = 1; p.full = true; p.det = true;
        p.grid_x = (unsigned)((d.n_env + 63) / 64); p.lds = (size_t)p.nw * CL_NQ * 64 * sizeof(float);
    } else if (chain) {
        if (envmajor_shape) {
            p.kernel = CLK_ENVMAJOR; p.nb = d.n_bldg <= 17 ? 17 : 20; p.vec = 1;
            p.grid_x = (unsigned)((d.n_env + 255) / 256); p.block = 256; p.lds = 0;
        } else if (!full && lean_shape) {
            if (int rc = set_lean(vec)) return rc;
        } else if (lean_chunk) {
            set_lean_chunk();
        } else if (tp_kernel) {
            set_tp();
        } else if (full && tun.full_variant != 1) {
            // thermal / outage districts: the pack-generic kernel of cl_full.h at one env per lane (parameter blocks staged in LDS where chunked)
            if (det) set_full(1024, 4, false);
            else if (obs_full && !lp) set_full_obs();
            else set_full(1024, 4, lp);
        } else p.kernel = CLK_STEP;
    } else if (f64) {
        if (!full && lean_shape) { p.kernel = CLK_LEAN; p.vec = vec == 1 ? 1 : 2; }
        else p.kernel = CLK_STEP;
    } else if (flex && !full && lean_shape) {
        if (int rc = set_lean(vec)) return rc;
        p.form = CLF_PLAIN; p.lds = lds;
    } else if (flex) {
        // districts with chargers / washing machines: the FLEX instantiations of the general kernel
        if (vec > 2) return fail(CL_EINVAL, "bad vec %d for the flexible-load step", vec);
        p.kernel = CLK_STEP;
    } else if (tp_kernel) {
        set_tp();
    } else if (full && tun.full_variant != 1 && vec <= 2) {
        // thermal / outage districts: the pack-generic kernel of cl_full.h
        const bool small = p.block <= 576;
        if (kpi_full) {
            p.kernel = CLK_FULL; p.form = CLF_KPI; p.lds = lds + (size_t)d.n_bldg * tile * sizeof(float);      // + the per-building baselines of the tile
        } else if (det) {
            if (vec == 1) set_full(1024, 4, false);
            else if (small) set_full(576, 3, false);
            else set_full(1024, 4, false);
        } else if (lp) {
            // parameter blocks staged in LDS (cl_full.h); full_variant = 3 keeps them in SGPRs (tests, A/B)
            p.fused_finish = (p.n_chunks > 1 && vec == 2 && !small) ? (tun.finish == 2 ? 1 : can_defer ? 2 : 0) : 0;
            // (chunks of 128 buildings: 40 KB of staged blocks + 32 KB of reduction rows + the exchange tile -- more dynamic LDS than a
            //  kernel gets without opting in where the runtime enforces the 64 KB default)
            if (vec == 1) set_full(1024, 5, true);
            else if (!small) set_full(1024, 4, true);
            else set_full(576, 5, false);      // (96 VGPRs do not hold the staged operands: 61 scratch accesses)
        } else {
            if (vec == 1 && obs_full) set_full_obs();
            else if (vec == 1) set_full(1024, CL_FULL1_WPE, false);
            else if (small) set_full(576, 5, false);
            else set_full(1024, 5, false);
        }
    } else if (full) {
        // (four envs per lane is not instantiated for the thermal unit: 92 bytes of scratch per lane, never selected by the library)
        if (vec != 1 && vec != 2) return fail(CL_EINVAL, "bad vec %d", vec);
        p.kernel = CLK_STEP;
    } else if (envmajor_shape) {
        // two or more waves per SIMD: the env-major kernel (bench.py --envs-per-gpu: 17 x 131 072 17.0 vs 18.5 us,
        // 17 x 262 144 28.2 vs 32.5 us, 17 x 1 048 576 136 vs 157 us; at 17 x 65 536 -- one wave per SIMD, nothing to hide the
        // per-building dependency chain behind -- 13.1 vs 8.0 us)
        // envs per lane (cl_tuning.vec: 1 or 2) and the compile-time bound on the buildings held in flight (17 = the 2022 challenge's
        // district: three fewer register quadruples than the general 20)
        p.kernel = CLK_ENVMAJOR;
        p.vec = tun.vec == 2 && act_stride_env == 1 ? 2 : 1;
        p.nb = d.n_bldg <= 17 && tun.lean_variant != 8 ? 17 : 20;
        p.grid_x = (unsigned)((d.n_env + 255) / 256); p.block = 256 / p.vec; p.lds = 0;
    } else if (lean_shape) {
        // one workgroup per CU at most: with more rounds the generic kernel's smaller register file (52 vs 88 VGPRs, two
        // workgroups per CU) wins again -- 17 x 262 144: 30.8 us vs 33.0 us
        if (int rc = set_lean(vec)) return rc;
    } else if (lean_chunk) {
        set_lean_chunk();
    } else if (p.n_chunks > 1 && (tun.finish == 2 || can_defer) && (vec == 1 || vec == 4)) {
        // building-chunked battery + PV districts (C4 with the 2022 device set): the instantiations that fold the chunk sums themselves
        // (finish = 2: their own, inside the launch; finish = 3: the previous step's, deferred)
        // (four envs per lane x 16 waves: 64 KB of reduction rows + the 4 KB exchange tile of the deferred fold -- more dynamic LDS than a
        //  kernel gets without opting in where the runtime enforces the 64 KB default; gfx950's 160 KB hold it)
        p.kernel = CLK_STEP; p.fold = true; p.fused_finish = tun.finish == 2 ? 1 : 2;
    } else {
        if (vec != 1 && vec != 2 && vec != 4) return fail(CL_EINVAL, "bad vec %d", vec);
        p.kernel = CLK_STEP;
    }
    p.finish = p.n_chunks > 1 && !p.fused_finish;
    p.marl = p.n_chunks > 1 && rkind_host == CLR_MARL;
    // (without the detail planes -- lean districts -- and under cl_step_full_kpi_kernel the step launch has updated every accumulator itself)
    p.kpi_passes = (d.flags & CLD_KPI) && !kpi_full && det ? (tun.kpi_passes == 2 ? 2 : 1) : 0;
    return CL_OK;
}

// cl_tuning.kernel_name (diagnostics): the instantiations a call launched, '+'-separated, spelled as rocprofv3 prints them
void name_reset(const cl_tuning& tun) { if (tun.kernel_name) tun.kernel_name[0] = 0; }
void name_add(const cl_tuning& tun, const char* fmt, ...) {
    if (!tun.kernel_name) return;
    size_t n = strnlen(tun.kernel_name, CL_KERNEL_NAME_LEN - 1);
    if (n && n + 2 < CL_KERNEL_NAME_LEN) { tun.kernel_name[n++] = '+'; tun.kernel_name[n] = 0; }
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(tun.kernel_name + n, CL_KERNEL_NAME_LEN - n, fmt, ap);
    va_end(ap);
}

// The kernel_name of a plan (the instantiations the launcher picks from the same fields).  Formats only where the caller asked for a name.
void plan_name(const StepPlan& p, const cl_tuning& tun) {
    name_reset(tun);
    if (!tun.kernel_name) return;
    auto tf = [](bool b) { return b ? "true" : "false"; };
    const char* nt = tf(p.nt);
    if (p.flex_vec) name_add(tun, "cl_flex_kernel<%d, %s>", p.flex_vec, tf(p.flex_nt));
    const char* chain = p.prec == 2 ? "_chain" : "";
    switch (p.kernel) {
    case CLK_STEP:
        name_add(tun, "cl_step_kernel<%d, %s, %s, %s, %d, %s%s>", p.vec, tf(p.full), tf(p.det), tf(p.flex), p.prec, tf(p.fold), p.check ? ", true" : "");
        break;
    case CLK_LEAN_CHUNK: name_add(tun, "cl_step_lean_chunk_kernel<%d, %s, %s, %d>", p.vec, nt, tf(p.fold), p.prec); break;
    case CLK_LEAN:
        if (p.form == CLF_PLAIN && p.prec == 0) name_add(tun, "cl_step_lean_kernel<%d, %s, %s>", p.vec, tf(p.flex), nt);
        else name_add(tun, "cl_step_lean%s%s_kernel<%d, %s>", p.form == CLF_KPI ? "_kpi" : p.form == CLF_OBS ? "_obs" : "",
                      p.prec == 2 ? "_chain" : p.prec == 1 ? "_f64" : "", p.vec, nt);
        break;
    case CLK_ENVMAJOR: name_add(tun, "cl_step_envmajor_kernel<%d, %s, %d, %d>", p.nb, nt, p.vec, p.prec); break;
    case CLK_FULL:
        if (p.form == CLF_KPI) name_add(tun, "cl_step_full_kpi_kernel<%s>", nt);
        else if (p.form == CLF_OBS) name_add(tun, "cl_step_full_obs_kernel<%d, %s>", p.prec, nt);
        else name_add(tun, "cl_step_full%s_kernel<%d, %s, %d, %d, %s, %s>", chain, p.vec, tf(p.det), p.maxt, p.wpe, tf(p.lp), nt);
        break;
    case CLK_FULL_TP:
        if (p.form == CLF_OBS) name_add(tun, "cl_step_full_tp_obs_kernel<%d, %d, %s>", p.vec, p.prec, nt);
        else name_add(tun, "cl_step_full_tp%s_kernel<%d, %d, %s>", chain, p.vec, p.wpe, nt);
        break;
    }
    if (p.finish) name_add(tun, "cl_finish_kernel");
    if (p.marl) name_add(tun, "cl_marl_reward_kernel");
    if (p.kpi_passes == 2) name_add(tun, "cl_kpi_bldg_kernel+cl_kpi_env_kernel");
    else if (p.kpi_passes == 1) name_add(tun, "cl_kpi_kernel");
}

}  // namespace
