"""us per env step of the closed-loop rollout of a THERMAL district under a policy with TWO hidden layers (cl_rollout_full_policy_deep_kernel),
both kernel families -- layer 2 in exact fp32 (MMA 0) and on the f16 matrix cores with split operands (MMA 1) -- at (H1, H2) = (16, 16) and
(32, 32) and the further shapes the `matrix_cores=None` rule is drawn from, against cl_rollout_full_policy_kernel (ONE hidden layer: what the
second layer costs) at H = 16 / 32 and `capture_rollout` with the same deep MLP in torch (the only other route for this policy): g2020_cz1's nine
buildings x 32 768 / 65 536 envs, K = 24, record off and on, float64 chain and fp32 map.  One process, the legs alternating round by round,
round 0 discarded; every timed window is `--launches` rollouts between two device events.  Prints one JSON line per leg (median, min, max over
the rounds); per (H1, H2), which family `policy.default_thermal_matrix_cores` may name: MMA 1 only where its median is below MMA 0's by more
than the spread (max - min) of its own rounds in EVERY measured case; and whether the fused launch beats `capture_rollout` by more than both
spreads in every case.  The committed log is profiles/policy_full_deep_probe.log.
    python scripts/policy_full_deep_probe.py [--rounds 7] [--launches 4] [--sizes 32768,65536] [--shapes 16x16,32x32,..] [--log FILE]"""
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
SHAPES = ((16, 16), (32, 32), (8, 8), (16, 32), (32, 16), (24, 24))
CAPTURED = ((16, 16), (32, 32))             # the shapes that also run through capture_rollout


def make_policy(layout, H):
    n_obs, nb = max(len(n) for n in layout.building_names), len(layout.building_names)
    rng = np.random.RandomState(H)
    return P.StorageMLPPolicy(rng.uniform(-1, 1, (1, nb, H, n_obs)) * 0.25 / np.sqrt(n_obs), rng.uniform(-0.5, 0.5, (1, nb, H)),
                              rng.uniform(-1, 1, (1, nb, 4, H)) * 0.125 / np.sqrt(H), rng.uniform(-0.05, 0.05, (1, nb, 4)))


def make_deep_policy(layout, H1, H2):
    n_obs, nb = max(len(n) for n in layout.building_names), len(layout.building_names)
    rng = np.random.RandomState(100 * H1 + H2)
    return P.DeepStorageMLPPolicy(rng.uniform(-1, 1, (1, nb, H1, n_obs)) * 0.25 / np.sqrt(n_obs), rng.uniform(-0.5, 0.5, (1, nb, H1)),
                                  rng.uniform(-1, 1, (1, nb, H2, H1)) / np.sqrt(H1), rng.uniform(-0.5, 0.5, (1, nb, H2)),
                                  rng.uniform(-1, 1, (1, nb, 4, H2)) * 0.125 / np.sqrt(H2), rng.uniform(-0.05, 0.05, (1, nb, 4)))


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
    ap.add_argument('--sizes', default='32768,65536')
    ap.add_argument('--log', default=None)
    ap.add_argument('--shapes', default=','.join(f'{a}x{b}' for a, b in SHAPES))
    args = ap.parse_args()
    shapes = tuple(tuple(int(v) for v in x.split('x')) for x in args.shapes.split(','))
    log = open(args.log, 'w') if args.log else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if log:
            log.write(line + '\n')
            log.flush()

    emit({'device': torch.cuda.get_device_name(0), 'k_steps': K, 'rounds': args.rounds, 'launches_per_window': args.launches,
          'unit': 'us per env step (all 9 buildings, all envs)'})
    schema = sample_schema('citylearn_challenge_2020_climate_zone_1_744h')
    faster = {}                                                    # (H1, H2) -> [MMA 1 faster than MMA 0 by more than its spread, per case]
    beats = []                                                     # [the fused launch faster than capture_rollout by more than both spreads, per case]
    for E in (int(x) for x in args.sizes.split(',')):
        for f64 in ('chain', False):
            env = VectorCityLearnEnv(schema, E, observations='tensor', normalize_observations=True, f64_maps=f64)
            e = env.engine
            e.trace_kernels()
            ret = torch.zeros(E, device=env.device)
            traj = torch.empty((K, P.CLPF_NT, e.n_bldg, E), device=env.device)
            legs, kernels = {}, {}

            def add(name, pt):
                for rec in (0, 1):
                    legs[f'{name} traj={rec}'] = (lambda pt=pt, rec=rec: e.rollout_policy(K, pt, seed=1, ret_env=ret, traj=traj if rec else None, t0=0))
                e.rollout_policy(K, pt, seed=1, ret_env=ret, t0=0)
                kernels[name] = e.last_kernels
            for H1, H2 in shapes:
                pol = make_deep_policy(env.layout, H1, H2)
                for mma in (0, 1):
                    add(f'deep ({H1}, {H2}) MMA={mma}', pol.pack(env.layout, env.tables, device=env.device, matrix_cores=bool(mma)))
            for H in (16, 32):
                add(f'one hidden layer H={H}', make_policy(env.layout, H).pack(env.layout, env.tables, device=env.device))
            caps, cap = [], None
            for H1, H2 in [x for x in shapes if x in CAPTURED]:
                f = make_deep_policy(env.layout, H1, H2).torch_policy(env.layout, env.tables, env.device)
                env.reset()
                cap = env.capture_rollout(f, K)
                cap.run()                                          # capture + first replay
                caps.append(cap)
                legs[f'capture_rollout torch deep MLP ({H1}, {H2})'] = (lambda cap=cap: (env.reset(), cap.run()))
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
            for H1, H2 in shapes:
                for rec in (0, 1):
                    m0, m1 = stat[f'deep ({H1}, {H2}) MMA=0 traj={rec}'], stat[f'deep ({H1}, {H2}) MMA=1 traj={rec}']
                    faster.setdefault((H1, H2), []).append(m1[0] < m0[0] - (m1[2] - m1[1]))
                cname = f'capture_rollout torch deep MLP ({H1}, {H2})'
                if cname in stat:                                  # (capture_rollout hands out what a record holds: against the legs with the record)
                    c = stat[cname]
                    for mma in (0, 1):
                        m = stat[f'deep ({H1}, {H2}) MMA={mma} traj=1']
                        beats.append(m[0] < c[0] - (m[2] - m[1]) - (c[2] - c[1]))
                        emit({'n_env': E, 'f64_maps': f64, 'shape': [H1, H2], 'MMA': mma, 'capture_rollout_over_fused': round(c[0] / m[0], 2),
                              'faster_beyond_both_spreads': beats[-1]})
            del caps, cap, env, e
    for (H1, H2), wins in faster.items():
        emit({'shape': [H1, H2], 'matrix_cores_faster_beyond_its_spread': f'{sum(wins)} of {len(wins)} cases', 'default_thermal_matrix_cores': all(wins)})
    emit({'fused_faster_than_capture_rollout_beyond_both_spreads': f'{sum(beats)} of {len(beats)} cases'})
    if log:
        log.close()


if __name__ == '__main__':
    main()
