"""us per env step of the building-chunked closed-loop policy rollout of a thermal district WITH the streaming KPIs
(cl_rollout_full_policy_chunk_kpi_kernel + cl_kpi_series_chunk_kernel + cl_finish_kernel) against what it replaces, on BASELINE config 4's
district -- the 2020 climate-zone-1 device set tiled to 1024 buildings -- x 1024 envs, K = 24, H = 16, sigma = 0, float64 chain and fp32 map, one
process, the variants alternating round by round (medians of the rounds), resets outside the timed region.
  (a) the chunked KPI rollout on a kpi=True engine, no record
  (b) the route without it: the chunked rollout WITH the record (K x 10 x n_bldg x n_env floats), the recorded head planes scattered to action
      columns, and those fed through `step_many` to a second, kpi=True engine
  (c) the chunked rollout without KPIs and without the record
    python scripts/policy_full_chunk_kpi_probe.py [--rounds 7] [--envs 1024] [--buildings 1024] > profiles/policy_full_chunk_kpi_probe.log"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from citylearn_amd import load_district, policy as P       # noqa: E402
from citylearn_amd.data import sample_schema                # noqa: E402
from citylearn_amd.observations import ObservationLayout    # noqa: E402
from citylearn_amd.synthetic import tile_district           # noqa: E402
from citylearn_amd.vector_env import VectorCityLearnEnv     # noqa: E402
from policy_full_chunk_probe import K, make_policy          # noqa: E402


def timed(fn, resets):
    for reset in resets:
        reset()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--envs', type=int, default=1024)
    ap.add_argument('--buildings', type=int, default=1024)
    args = ap.parse_args()
    E = args.envs
    spec = tile_district(load_district(sample_schema('citylearn_challenge_2020_climate_zone_1_744h')), args.buildings)
    for f64 in ('chain', False):
        plain = VectorCityLearnEnv(spec, E, f64_maps=f64)
        kenv = VectorCityLearnEnv(spec, E, f64_maps=f64, kpi=True)
        e, ke = plain.engine, kenv.engine
        e.trace_kernels(); ke.trace_kernels()
        dev = plain.device
        ret = torch.zeros(E, device=dev)
        traj = torch.empty((K, P.CLPF_NT, e.n_bldg, E), device=dev)
        acts = torch.zeros((K, e.n_act_cols, E), device=dev)
        layout = ObservationLayout(plain.spec, 'current', False, plain.reference_quirks)
        pol = make_policy(layout)
        pt = pol.pack(layout, plain.tables, device=dev)
        b, h = np.nonzero(pt.cols >= 0)
        cols, hh, bb = (torch.as_tensor(x, device=dev) for x in (pt.cols[b, h], h, b))

        def replay_route():
            e.rollout_policy(K, pt, seed=1, ret_env=ret, traj=traj, t0=0, chunked=True)
            acts[:, cols] = traj[:, P.CLPF_T_ACTION + hh, bb]
            ke.step_many(acts, t0=0)

        variants = {'(a) chunked policy KPI rollout, traj=0': (lambda: ke.rollout_policy(K, pt, seed=1, ret_env=ret, traj=None, t0=0, kpi=True, chunked=True), (ke.reset,)),
                    '(b) chunked policy traj=1 + scatter + step_many(kpi=True)': (replay_route, (e.reset, ke.reset)),
                    '(c) chunked policy, no KPIs, traj=0': (lambda: e.rollout_policy(K, pt, seed=1, ret_env=ret, traj=None, t0=0, chunked=True), (e.reset,))}
        times = {k: [] for k in variants}
        for r in range(args.rounds + 1):
            for name, (fn, resets) in variants.items():
                t = timed(fn, resets)
                if r:                                           # round 0 warms up
                    times[name].append(t)
        kern = {}
        e.reset(); ke.reset(); replay_route(); kern['(b)'] = e.last_kernels + ' ; ' + ke.last_kernels
        kpi_ref, env_ref = ke.kpi_bldg.clone(), ke.kpi_env.clone()
        ke.reset(); variants['(a) chunked policy KPI rollout, traj=0'][0](); kern['(a)'] = ke.last_kernels
        e.reset(); variants['(c) chunked policy, no KPIs, traj=0'][0](); kern['(c)'] = e.last_kernels
        fin = torch.isfinite(env_ref)
        close = bool(torch.allclose(ke.kpi_bldg, kpi_ref, rtol=1e-4, atol=1e-3)) and bool(torch.allclose(ke.kpi_env[fin], env_ref[fin], rtol=1e-4, atol=1e-2))
        med = {}
        for name, ts in times.items():
            med[name] = statistics.median(ts)
            print(json.dumps({'n_bldg': e.n_bldg, 'n_env': E, 'f64_maps': f64, 'variant': name, 'us_per_step_median': round(med[name], 3),
                              'min': round(min(ts), 3), 'max': round(max(ts), 3), 'rounds': len(ts)}), flush=True)
        a_, b_, c_ = (med[k] for k in variants)
        print(json.dumps({'n_bldg': e.n_bldg, 'n_env': E, 'f64_maps': f64, 'kernels': kern, 'kpi_planes_of_both_routes_close': close,
                          'series_scratch_MB': round(ke._series_scratch.numel() * 4 / 1e6, 1),
                          'replay_over_kpi (b)/(a)': round(b_ / a_, 3), 'kpi_over_plain (a)/(c)': round(a_ / c_, 3), 'a_faster_than_b': bool(a_ < b_)}), flush=True)
        variants.clear()
        del plain, kenv, e, ke, traj, acts, pt
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
