"""us per env step of the closed-loop policy rollout of a thermal district WITH the streaming KPIs (cl_rollout_full_policy_kpi_kernel) against
what it replaces: the 2020 climate-zone-1 district, 9 buildings x 32 768 / 65 536 envs, K = 24, H = 16, sigma = 0, float64 chain and fp32 map,
one process, the variants alternating round by round (medians of the rounds), resets outside the timed region.
  (i)   cl_rollout_full_policy_kernel without the record (no KPIs at all)
  (ii)  cl_rollout_full_policy_kpi_kernel on a kpi=True engine, no record
  (iii) the route without the kernel: the policy rollout WITH the record, the recorded head planes scattered to action columns, and those fed
        through `step_many` to a second, kpi=True engine
    python scripts/policy_full_kpi_probe.py [--rounds 7] [--sizes 32768,65536] > profiles/policy_full_kpi_probe.log"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from citylearn_amd import policy as P                      # noqa: E402
from citylearn_amd.data import sample_schema                # noqa: E402
from citylearn_amd.vector_env import VectorCityLearnEnv     # noqa: E402
from policy_full_probe import K, make_policy                # noqa: E402


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
    ap.add_argument('--sizes', default='32768,65536')
    args = ap.parse_args()
    schema = sample_schema('citylearn_challenge_2020_climate_zone_1_744h')
    for E in (int(x) for x in args.sizes.split(',')):
        for f64 in ('chain', False):
            plain = VectorCityLearnEnv(schema, E, f64_maps=f64)
            kenv = VectorCityLearnEnv(schema, E, f64_maps=f64, kpi=True)
            e, ke = plain.engine, kenv.engine
            e.trace_kernels(); ke.trace_kernels()
            dev = plain.device
            ret = torch.zeros(E, device=dev)
            traj = torch.empty((K, P.CLPF_NT, e.n_bldg, E), device=dev)
            acts = torch.zeros((K, e.n_act_cols, E), device=dev)
            from citylearn_amd.observations import ObservationLayout
            layout = ObservationLayout(plain.spec, 'current', False, plain.reference_quirks)
            pol = make_policy(layout)
            pt = pol.pack(layout, plain.tables, device=dev)
            b, h = np.nonzero(pt.cols >= 0)
            cols, hh, bb = (torch.as_tensor(x, device=dev) for x in (pt.cols[b, h], h, b))

            def replay_route():
                e.rollout_policy(K, pt, seed=1, ret_env=ret, traj=traj, t0=0)
                acts[:, cols] = traj[:, P.CLPF_T_ACTION + hh, bb]
                ke.step_many(acts, t0=0)

            variants = {'(i) policy, no KPIs, traj=0': (lambda: e.rollout_policy(K, pt, seed=1, ret_env=ret, traj=None, t0=0), (e.reset,)),
                        '(ii) policy KPI kernel, traj=0': (lambda: ke.rollout_policy(K, pt, seed=1, ret_env=ret, traj=None, t0=0, kpi=True), (ke.reset,)),
                        '(iii) policy traj=1 + scatter + step_many(kpi=True)': (replay_route, (e.reset, ke.reset))}
            times = {k: [] for k in variants}
            for r in range(args.rounds + 1):
                for name, (fn, resets) in variants.items():
                    t = timed(fn, resets)
                    if r:                                           # round 0 warms up
                        times[name].append(t)
            kern = {}
            e.reset(); ke.reset(); replay_route(); kern['(iii)'] = e.last_kernels + ' ; ' + ke.last_kernels
            kpi_ref = ke.kpi_bldg.clone()
            ke.reset(); variants['(ii) policy KPI kernel, traj=0'][0](); kern['(ii)'] = ke.last_kernels
            close = bool(torch.allclose(ke.kpi_bldg, kpi_ref, rtol=1e-4, atol=1e-3))        # both routes scored the same controllers
            med = {}
            for name, ts in times.items():
                med[name] = statistics.median(ts)
                print(json.dumps({'n_env': E, 'f64_maps': f64, 'variant': name, 'us_per_step_median': round(med[name], 3),
                                  'min': round(min(ts), 3), 'max': round(max(ts), 3), 'rounds': len(ts)}), flush=True)
            i, ii, iii = (med[k] for k in variants)
            print(json.dumps({'n_env': E, 'f64_maps': f64, 'kernels': kern, 'kpi_bldg_of_both_routes_close': close,
                              'kpi_over_plain (ii)/(i)': round(ii / i, 3), 'replay_over_kpi (iii)/(ii)': round(iii / ii, 3),
                              'ii_faster_than_iii_by_more_than_4_percent': bool(ii < iii / 1.04)}), flush=True)
            del plain, kenv, e, ke


if __name__ == '__main__':
    main()
