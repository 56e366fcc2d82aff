"""us per env step of the building-chunked closed-loop policy rollout of a battery + PV district (cl_rollout_policy_chunk_kernel +
cl_finish_kernel) on the packaged citylearn_challenge_2022_phase_all_720h district tiled to 1024 buildings, against (i) the blind chunked fused
rollout (cl_rollout_kernel<.., CHUNK = true, ..>, uniform random policy) and (iii) `capture_rollout` with the equivalent torch MLP, the route it
replaces: 1024 buildings x 1024 / 8192 envs, K = 24, H = 16, sigma = 0, float64 chain and fp32 map, one process, the variants alternating round
by round (medians of the rounds), resets outside the timed region.  (ii) runs without the record at the default chunking (32 x 32 buildings) and
at b_chunk = 16 (64 chunks of eight waves); with the record (0.4 GB at x 1024) and (iii) only at x 1024.
THE ONE CONDITION: (ii) with the record is faster than (iii) by more than the project's +-4 % process band, under both precision models --
the last line says whether it is met.  The ratios (ii) / (i) and b_chunk = 16 / default are recorded, not gated.
    python scripts/policy_chunk_probe.py [--rounds 7] [--sizes 1024,8192] [--buildings 1024] > profiles/policy_chunk_probe.log"""
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
from citylearn_amd.synthetic import tile_district           # noqa: E402
from citylearn_amd.vector_env import VectorCityLearnEnv     # noqa: E402

K, H = 24, 16
RECORD_MAX_ENVS = 1024          # the record is K x 4 x n_bldg x n_env floats
BAND = 1.04                     # the project's +-4 % process band


def make_policy(layout):
    n_obs, nb = max(len(n) for n in layout.building_names), len(layout.building_names)
    rng = np.random.RandomState(H)
    return P.MLPPolicy(rng.uniform(-1, 1, (1, nb, H, n_obs)) * 0.25 / np.sqrt(n_obs), rng.uniform(-0.5, 0.5, (1, nb, H)),
                       rng.uniform(-1, 1, (1, nb, H)) * 0.5 / np.sqrt(H), rng.uniform(-0.2, 0.2, (1, nb)))


def timed(fn, reset):
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
    ap.add_argument('--sizes', default='1024,8192')
    ap.add_argument('--buildings', type=int, default=1024)
    args = ap.parse_args()
    spec = tile_district(load_district(sample_schema('citylearn_challenge_2022_phase_all_720h')), args.buildings)
    met = []
    for E in (int(x) for x in args.sizes.split(',')):
        for f64 in ('chain', False):
            env = VectorCityLearnEnv(spec, E, observations='tensor', normalize_observations=True, f64_maps=f64)
            e = env.engine
            e.trace_kernels()
            e.set_action_limits(env.action_low.cpu().numpy(), env.action_high.cpu().numpy())
            ret = torch.zeros(E, device=env.device)
            record = E <= RECORD_MAX_ENVS
            traj = torch.empty((K, P.CLPOL_NT, e.n_bldg, E), device=env.device) if record else None
            pol = make_policy(env.layout)
            pt = pol.pack(env.layout, env.tables, device=env.device)

            def chunked(b_chunk, tr):
                def run():
                    e.tuning.b_chunk = b_chunk              # (the tuning block travels with every call: set for this call only)
                    try:
                        e.rollout_policy(K, pt, seed=1, ret_env=ret, traj=tr, t0=0, chunked=True)
                    finally:
                        e.tuning.b_chunk = 0
                return run
            variants = {'(i) blind chunked fused rollout': lambda: e.rollout(K, seed=1, ret_env=ret, t0=0, fused=True),
                        '(ii) policy traj=0 default chunks': chunked(0, None),
                        '(ii) policy traj=0 b_chunk=16': chunked(16, None)}
            if record:
                variants['(ii) policy traj=1 default chunks'] = chunked(0, traj)
                cap = env.capture_rollout(pol.torch_policy(env.layout, env.tables, env.device), K)
                env.reset()
                cap.run()                                              # capture + first replay
                variants['(iii) capture_rollout torch MLP'] = cap.run                  # (env.reset() outside the timed region, like the other variants' reset)
            times = {k: [] for k in variants}
            for r in range(args.rounds + 1):
                for name, fn in variants.items():
                    t = timed(fn, e.reset if not name.startswith('(iii)') else env.reset)
                    if r:                                           # round 0 warms up
                        times[name].append(t)
            kern = {}
            e.reset(); variants['(ii) policy traj=0 default chunks'](); kern['policy'] = e.last_kernels
            e.reset(); variants['(ii) policy traj=0 b_chunk=16'](); kern['policy b_chunk=16'] = e.last_kernels
            e.reset(); variants['(i) blind chunked fused rollout'](); kern['blind'] = e.last_kernels
            med = {}
            for name, ts in times.items():
                med[name] = statistics.median(ts)
                print(json.dumps({'n_bldg': e.n_bldg, 'n_env': E, 'f64_maps': f64, 'variant': name, 'us_per_step_median': round(med[name], 3),
                                  'min': round(min(ts), 3), 'max': round(max(ts), 3), 'rounds': len(ts)}), flush=True)
            summary = {'n_bldg': e.n_bldg, 'n_env': E, 'f64_maps': f64, 'kernels': kern,
                       'policy_over_blind': round(med['(ii) policy traj=0 default chunks'] / med['(i) blind chunked fused rollout'], 3),
                       'b_chunk16_over_default': round(med['(ii) policy traj=0 b_chunk=16'] / med['(ii) policy traj=0 default chunks'], 3)}
            if record:
                ratio = med['(iii) capture_rollout torch MLP'] / med['(ii) policy traj=1 default chunks']
                summary['capture_over_policy_traj1'] = round(ratio, 2)
                met.append(ratio > BAND)
            print(json.dumps(summary), flush=True)
            variants.clear()
            del env, e, traj, pt
            torch.cuda.empty_cache()
    print(json.dumps({'condition': '(ii) with the record faster than (iii) by more than the +-4 % band under both precision models',
                      'met': bool(met) and all(met), 'cases': len(met)}), flush=True)


if __name__ == '__main__':
    main()
