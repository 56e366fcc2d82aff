// cl_policy_chunk.h -- mode B of a battery + PV district of MORE THAN 32 buildings with a CLOSED-LOOP policy: cl_policy.h's kernel template at
// CHUNK = true, cl_rollout_policy_kernel<VEC, PREC, KPI = false, CHUNK = true> (two buildings per wave, each one's storage action a one-hidden-layer
// tanh MLP evaluated inside the loop from its soc and its previous net, then the lean unit; reported as cl_rollout_policy_chunk_kernel<VEC, PREC>)
// in the chunk geometry of cl_rollout_kernel<.., CHUNK = true, ..> (cl_rollout.h):
// the buildings are cut into chunks of `b_chunk` <= 32 along gridDim.y, wave w of workgroup row y owns buildings y b_chunk + w and y b_chunk + w + nw,
// and a workgroup ends with its chunk's partial district sums of the last step and its chunk's share of the K-step return in the scratch rows of
// out_bldg's reserved plane, which ONE cl_finish_kernel launch folds per launch.  Included by cl_policy_chunk.hip only
// (libcitylearn_amd_policy_chunk.so, include/citylearn_amd_policy_chunk.h), which instantiates no other variant of the template.
//
// What `CHUNK` switches in the kernel, against the one-row launch:
//  * everything it indexes by w + m nw -- params, ts, state, out_bldg, pre, dep, out, net_reset, the traj planes -- is indexed by the global
//    building b = y b_chunk + w + m nw here; the Philox stream stays keyed by (global env, action column, step) and keeps its two-step block cache,
//    so a chunk geometry does not change a draw;
//  * a SEAT without a building (own[m] = b < min(n_bldg, (y + 1) b_chunk), wave-uniform) loads, stages, computes, records and stores nothing and
//    adds zeros to the reductions.  A wave with NEITHER seat filled (the tail of the last chunk: 33 buildings cut 32 + 1 leave fifteen) reads the
//    parameter row of one clamped, valid building -- ONE min, cl_policy_full.h's note -- and touches nothing else; it meets the barrier behind
//    the row staging, district_reduce's and the return rows';
//  * the last step's district sums go through district_reduce's n_chunks > 1 path, the return rows behind them (cl_rollout_kernel<CHUNK>'s place);
//    ret_env is cl_finish_kernel's to add to;
//  * NO barrier inside the K loop, hence no MARL (a chunked launch cannot couple the buildings inside a step anyway): the wave-uniform table reads
//    stay scalar (cl_rollout_full_kernel's note on its MARL instantiations).
// These sit under `if constexpr (CHUNK)` (or `CHUNK ?` / `CHUNK ||` in a condition) in the one source, so each instantiation is the code of the
// kernel it was when this file held a kernel of its own (profiles/policy_one_source_isa.md).  LDS per workgroup: cl_policy.h's formula,
// [nw][NQ][tile] reduction rows (the return rows alias them) + nw x 2 x CLPOL_ROW floats -- 29 KiB at the default sixteen waves and one env per lane, 45 KiB at two.
#pragma once
#include "cl_policy.h"

#ifdef __HIPCC__
namespace {

constexpr size_t rollout_policy_chunk_lds_floats(int nw, int tile) { return (size_t)nw * NQ * tile + (size_t)nw * 2 * CLPOL_ROW; }

}  // namespace
#endif  // __HIPCC__
