"""us per env step of the closed-loop rollout of a THERMAL district under a CENTRAL-AGENT policy with TWO hidden layers
(cl_rollout_full_policy_central_deep_kernel: csrc/cl_policy_full_central.h at DEEP = true) at (H1, H2) = (16, 16), (32, 32), (64, 64) and (64, 4), against the one-hidden-layer central thermal
kernel (cl_rollout_full_policy_central_kernel: the same template at DEEP = false) at H = H1 -- what the second layer, its LDS and its barrier add -- and against `capture_rollout`
with the same two-layer MLP in torch -- the only way to run such an actor on such a district without the kernel: the 2020 schema's 9 buildings x
32 768 envs, K = 24, with the record, float64 chain and fp32 map.  The protocol of scripts/policy_full_central_probe.py: one process, the legs
alternating round by round, round 0 discarded; every timed window is `--launches` rollouts between two device events.  Prints one JSON line per
leg (median, min, max over the rounds) and, per case, both comparisons with whether the difference exceeds the sum of the two spreads
(max - min): no figure is fixed in advance, every case is reported either way.  The committed log is profiles/policy_full_central_deep_probe.log.
    python scripts/policy_full_central_deep_probe.py [--rounds 7] [--launches 4] [--sizes 32768] [--log profiles/policy_full_central_deep_probe.log]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from citylearn_amd import policy as P                      # noqa: E402
from citylearn_amd.data import sample_schema                # noqa: E402
from citylearn_amd.vector_env import VectorCityLearnEnv     # noqa: E402

K = 24
SHAPES = ((16, 16), (32, 32), (64, 64), (64, 4))
SCHEMA = 'citylearn_challenge_2020_climate_zone_1_744h'


def make_central_policy(layout, H):
    n_cols, nb = layout.n_cols, len(layout.building_names)
    rng = np.random.RandomState(500 + H)
    return P.CentralStorageMLPPolicy(rng.uniform(-1, 1, (1, H, n_cols)) * 0.125 / np.sqrt(n_cols), rng.uniform(-0.5, 0.5, (1, H)),
                                     rng.uniform(-1, 1, (1, nb, P.CLPF_NA, H)) * 0.125 / np.sqrt(H), rng.uniform(-0.05, 0.05, (1, nb, P.CLPF_NA)))


def make_deep_central_policy(layout, H1, H2):
    n_cols, nb = layout.n_cols, len(layout.building_names)
    rng = np.random.RandomState(700 + 100 * H1 + H2)
    return P.DeepCentralStorageMLPPolicy(rng.uniform(-1, 1, (1, H1, n_cols)) * 0.125 / np.sqrt(n_cols), rng.uniform(-0.5, 0.5, (1, H1)),
                                         rng.uniform(-1, 1, (1, H2, H1)) / np.sqrt(H1), rng.uniform(-0.5, 0.5, (1, H2)),
                                         rng.uniform(-1, 1, (1, nb, P.CLPF_NA, H2)) * 0.125 / np.sqrt(H2), rng.uniform(-0.05, 0.05, (1, nb, P.CLPF_NA)))


def timed(fn, launches):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (K * launches)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--launches', type=int, default=4)
    ap.add_argument('--sizes', default='32768')
    ap.add_argument('--log', default=str(ROOT / 'profiles' / 'policy_full_central_deep_probe.log'))
    args = ap.parse_args()
    log = open(args.log, 'w') if args.log else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if log:
            log.write(line + '\n')
            log.flush()

    emit({'device': torch.cuda.get_device_name(0), 'k_steps': K, 'rounds': args.rounds, 'launches_per_window': args.launches,
          'unit': 'us per env step (all 9 buildings, all envs), record on'})
    schema = sample_schema(SCHEMA)
    beyond = []
    for E in (int(x) for x in args.sizes.split(',')):
        for f64 in ('chain', False):
            env = VectorCityLearnEnv(schema, E, observations='tensor', normalize_observations=True, f64_maps=f64, central_agent=True)
            e = env.engine
            e.trace_kernels()
            ret = torch.zeros(E, device=env.device)
            traj = torch.empty((K, P.CLPF_NT, e.n_bldg, E), device=env.device)
            legs, kernels = {}, {}

            def add(name, pt):
                legs[name] = (lambda pt=pt: e.rollout_policy(K, pt, seed=1, ret_env=ret, traj=traj, t0=0))
                e.rollout_policy(K, pt, seed=1, ret_env=ret, t0=0)
                kernels[name] = e.last_kernels
            for H1, H2 in SHAPES:
                add(f'deep central {H1}x{H2}', make_deep_central_policy(env.layout, H1, H2).pack(env.layout, env.tables, device=env.device))
            for H in sorted({h1 for h1, _ in SHAPES}):
                add(f'central H={H}', make_central_policy(env.layout, H).pack(env.layout, env.tables, device=env.device))
            caps = []
            for H1, H2 in SHAPES:
                f = make_deep_central_policy(env.layout, H1, H2).torch_policy(env.layout, env.tables, env.device)
                env.reset()
                cap = env.capture_rollout(f, K)
                cap.run()                                          # capture + first replay
                caps.append(cap)
                legs[f'capture_rollout torch deep central MLP {H1}x{H2}'] = (lambda cap=cap: (env.reset(), cap.run()))
            times = {k: [] for k in legs}
            for r in range(args.rounds + 1):
                for name, fn in legs.items():
                    t = timed(fn, 1 if name.startswith('capture') else args.launches)
                    if r:                                          # round 0 warms up
                        times[name].append(t)
            stat = {}
            for name, ts in times.items():
                stat[name] = (statistics.median(ts), min(ts), max(ts))
                emit({'n_env': E, 'f64_maps': f64, 'leg': name, 'us_per_step_median': round(stat[name][0], 3), 'min': round(min(ts), 3),
                      'max': round(max(ts), 3), 'rounds': len(ts)})
            emit({'n_env': E, 'f64_maps': f64, 'kernels': kernels})
            spread = lambda s: s[2] - s[1]
            for H1, H2 in SHAPES:
                deep, one = stat[f'deep central {H1}x{H2}'], stat[f'central H={H1}']
                cap = stat[f'capture_rollout torch deep central MLP {H1}x{H2}']
                faster = deep[0] < cap[0] - (spread(deep) + spread(cap))
                differs = abs(deep[0] - one[0]) > spread(deep) + spread(one)
                beyond.append(faster)
                emit({'n_env': E, 'f64_maps': f64, 'H1': H1, 'H2': H2, 'deep_us': round(deep[0], 3), 'one_hidden_layer_us': round(one[0], 3),
                      'deep_over_one_hidden_layer': round(deep[0] / one[0], 2), 'differs_beyond_both_spreads': bool(differs),
                      'capture_rollout_us': round(cap[0], 3), 'capture_over_deep': round(cap[0] / deep[0], 2),
                      'deep_faster_than_capture_beyond_both_spreads': bool(faster)})
            del caps, cap, env, e
    emit({'deep_faster_than_capture_beyond_both_spreads': f'{sum(beyond)} of {len(beyond)} cases'})
    if log:
        log.close()


if __name__ == '__main__':
    main()
