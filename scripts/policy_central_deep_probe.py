"""us per env step of the closed-loop rollout under a CENTRAL-AGENT policy with TWO hidden layers (cl_rollout_policy_central_deep_kernel) at
(H1, H2) = (16, 16), (32, 32), (64, 64) and (64, 4), against cl_rollout_policy_central_kernel (one hidden layer) at H = H1 -- what the second
layer costs -- and against `capture_rollout` with the same two-layer central MLP in torch, the only way to run such an actor without the kernel:
17 buildings x 32 768 envs, K = 24, with the record, float64 chain and fp32 map.  One process, the legs alternating round by round, round 0
discarded; every timed window is `--launches` rollouts between two device events.  Prints one JSON line per leg (median, min, max over the
rounds); per case whether the fused launch beats `capture_rollout` by more than the sum of the two spreads (max - min), and its cost over the
one-hidden-layer kernel; and per map the (64, 64) - (64, 4) difference: sixty of layer 2's sixty-four units, the share of a step the new phase
costs at that width.  The committed log is profiles/policy_central_deep_probe.log.
    python scripts/policy_central_deep_probe.py [--rounds 7] [--launches 4] [--sizes 32768] [--log profiles/policy_central_deep_probe.log]"""
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


def make_central_policy(layout, H):
    n_cols, nb = layout.n_cols, len(layout.building_names)
    rng = np.random.RandomState(500 + H)
    return P.CentralMLPPolicy(rng.uniform(-1, 1, (1, H, n_cols)) * 0.125 / np.sqrt(n_cols), rng.uniform(-0.5, 0.5, (1, H)),
                              rng.uniform(-1, 1, (1, nb, H)) * 0.125 / np.sqrt(H), rng.uniform(-0.2, 0.2, (1, nb)))


def make_deep_central_policy(layout, H1, H2):
    n_cols, nb = layout.n_cols, len(layout.building_names)
    rng = np.random.RandomState(700 + 64 * H1 + H2)
    return P.DeepCentralMLPPolicy(rng.uniform(-1, 1, (1, H1, n_cols)) * 0.125 / np.sqrt(n_cols), rng.uniform(-0.5, 0.5, (1, H1)),
                                  rng.uniform(-1, 1, (1, H2, H1)) / np.sqrt(H1), rng.uniform(-0.5, 0.5, (1, H2)),
                                  rng.uniform(-1, 1, (1, nb, H2)) * 0.125 / np.sqrt(H2), rng.uniform(-0.2, 0.2, (1, nb)))


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
    ap.add_argument('--log', default=str(ROOT / 'profiles' / 'policy_central_deep_probe.log'))
    args = ap.parse_args()
    log = open(args.log, 'w') if args.log else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if log:
            log.write(line + '\n')
            log.flush()

    emit({'device': torch.cuda.get_device_name(0), 'k_steps': K, 'rounds': args.rounds, 'launches_per_window': args.launches,
          'unit': 'us per env step (all 17 buildings, all envs), record on'})
    schema = sample_schema('citylearn_challenge_2022_phase_all_720h')
    wins = []
    for E in (int(x) for x in args.sizes.split(',')):
        for f64 in ('chain', False):
            env = VectorCityLearnEnv(schema, E, observations='tensor', normalize_observations=True, f64_maps=f64, central_agent=True)
            e = env.engine
            e.trace_kernels()
            ret = torch.zeros(E, device=env.device)
            traj = torch.empty((K, P.CLPOL_NT, e.n_bldg, E), device=env.device)
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
            for H1, H2 in SHAPES:
                fused, cap, one = stat[f'deep central {H1}x{H2}'], stat[f'capture_rollout torch deep central MLP {H1}x{H2}'], stat[f'central H={H1}']
                ok = fused[0] < cap[0] - ((fused[2] - fused[1]) + (cap[2] - cap[1]))
                wins.append(ok)
                emit({'n_env': E, 'f64_maps': f64, 'H1': H1, 'H2': H2, 'fused_us': round(fused[0], 3), 'capture_rollout_us': round(cap[0], 3),
                      'ratio': round(cap[0] / fused[0], 2), 'fused_faster_beyond_both_spreads': bool(ok),
                      'one_hidden_layer_us': round(one[0], 3), 'over_one_hidden_layer_us': round(fused[0] - one[0], 3)})
            wide, narrow = stat['deep central 64x64'], stat['deep central 64x4']
            emit({'n_env': E, 'f64_maps': f64, 'layer2_64x64_minus_64x4_us': round(wide[0] - narrow[0], 3),
                  'share_of_the_64x64_step': round((wide[0] - narrow[0]) / wide[0], 3),
                  'spreads_us': [round(wide[2] - wide[1], 3), round(narrow[2] - narrow[1], 3)]})
            del caps, cap, env, e
    emit({'fused_faster_beyond_both_spreads': f'{sum(wins)} of {len(wins)} cases', 'accepted': all(wins)})
    if log:
        log.close()


if __name__ == '__main__':
    main()
