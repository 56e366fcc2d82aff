"""us per env step of the closed-loop policy rollout (cl_rollout_policy_kernel) against (1) the random-policy fused rollout and (3)
`capture_rollout` with the equivalent torch MLP: 17 buildings x 32 768 / 65 536 envs, K = 24, float64 chain and fp32 map, one process, the
variants alternating round by round (medians of the rounds).  Kernel times: run this script under `rocprofv3 --kernel-trace --stats`.
    python scripts/policy_rollout_probe.py [--rounds 7] [--sizes 32768,65536]"""
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

K = 24


def make_policy(layout, H, sigma):
    n_obs, nb = max(len(n) for n in layout.building_names), len(layout.building_names)
    rng = np.random.RandomState(H)
    return P.MLPPolicy(rng.uniform(-1, 1, (1, nb, H, n_obs)) * 0.25 / np.sqrt(n_obs), rng.uniform(-0.5, 0.5, (1, nb, H)),
                       rng.uniform(-1, 1, (1, nb, H)) * 0.5 / np.sqrt(H), rng.uniform(-0.2, 0.2, (1, nb)), sigma=sigma)


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
    ap.add_argument('--sizes', default='32768,65536')
    args = ap.parse_args()
    schema = sample_schema('citylearn_challenge_2022_phase_all_720h')
    for E in (int(x) for x in args.sizes.split(',')):
        for f64 in ('chain', False):
            env = VectorCityLearnEnv(schema, E, observations='tensor', normalize_observations=True, f64_maps=f64)
            e = env.engine
            e.trace_kernels()
            e.set_action_limits(env.action_low.cpu().numpy(), env.action_high.cpu().numpy())
            ret = torch.zeros(E, device=env.device)
            traj = torch.empty((K, P.CLPOL_NT, e.n_bldg, E), device=env.device)
            variants = {'random': lambda: e.rollout(K, seed=1, ret_env=ret, t0=0)}
            for H in (8, 16, 32):
                for sigma in (None, 0.1):
                    pt = make_policy(env.layout, H, sigma).pack(env.layout, env.tables, device=env.device)
                    for rec in (False, True):
                        variants[f'policy H={H} sigma={sigma or 0} traj={int(rec)}'] = \
                            (lambda pt=pt, rec=rec: e.rollout_policy(K, pt, seed=1, ret_env=ret, traj=traj if rec else None, t0=0))
            f = make_policy(env.layout, 16, None).torch_policy(env.layout, env.tables, env.device)
            cap = env.capture_rollout(f, K)
            env.reset()
            cap.run()                                              # capture + first replay
            variants['capture_rollout torch MLP H=16'] = lambda: (env.reset(), cap.run())
            times = {k: [] for k in variants}
            for r in range(args.rounds + 1):
                for name, fn in variants.items():
                    t = timed(fn, e.reset if not name.startswith('capture') else (lambda: None))
                    if r:                                           # round 0 warms up
                        times[name].append(t)
            kern = {}
            e.reset(); variants['policy H=16 sigma=0 traj=1'](); kern['policy'] = e.last_kernels
            e.reset(); variants['random'](); kern['random'] = e.last_kernels
            for name, ts in times.items():
                print(json.dumps({'n_env': E, 'f64_maps': f64, 'variant': name, 'us_per_step_median': round(statistics.median(ts), 3),
                                  'min': round(min(ts), 3), 'max': round(max(ts), 3), 'rounds': len(ts)}), flush=True)
            print(json.dumps({'n_env': E, 'f64_maps': f64, 'kernels': kern}), flush=True)
            del cap, env, e


if __name__ == '__main__':
    main()
