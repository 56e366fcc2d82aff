"""us per env step of the closed-loop policy rollout that keeps the streaming KPIs (cl_rollout_policy_kpi_kernel) against what it replaces and
against its floor: 17 buildings x 32 768 / 65 536 envs, K = 24, H = 16, sigma = 0, float64 chain and fp32 map, one process, the variants
alternating round by round (medians of the rounds):
  (a) `rollout_policy(kpi=True)` without a record: the new launch;
  (b) `rollout_policy(record=True)` on an env without KPIs + the fused KPI replay of the recorded action plane on a second `kpi=True` env;
  (c) `rollout_policy` without KPIs and without a record: the floor.
    python scripts/policy_kpi_probe.py [--rounds 7] [--sizes 32768,65536] [--out profiles/policy_kpi_probe.log]
Without --worker the script starts one child per (size, precision model), each under its own `timeout`, and stops at the first that fails."""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

K, H = 24, 16


def worker(E, f64, rounds):
    import torch
    from citylearn_amd import policy as P
    from citylearn_amd.data import sample_schema
    from citylearn_amd.vector_env import VectorCityLearnEnv
    from policy_rollout_probe import make_policy, timed

    schema = sample_schema('citylearn_challenge_2022_phase_all_720h')
    mk = lambda kpi: VectorCityLearnEnv(schema, E, observations='tensor', normalize_observations=True, f64_maps=f64, kpi=kpi)
    kenv, penv = mk(True), mk(False)
    ke, pe = kenv.engine, penv.engine
    ke.trace_kernels()
    pt = make_policy(kenv.layout, H, None).pack(kenv.layout, kenv.tables, device=kenv.device)
    ret = torch.zeros(E, device=kenv.device)
    traj = torch.empty((K, P.CLPOL_NT, ke.n_bldg, E), device=kenv.device)

    def replaced():
        pe.rollout_policy(K, pt, seed=1, ret_env=ret, traj=traj, t0=0)
        ke.rollout(K, actions=traj[:, P.CLPOL_T_ACTION], fused=True, t0=0)      # (a strided view of the record: no copy)

    def both():
        ke.reset(); pe.reset()
    variants = {'a: rollout_policy(kpi=True)': (lambda: ke.rollout_policy(K, pt, seed=1, ret_env=ret, t0=0, kpi=True), ke.reset),
                'b: rollout_policy(record=True) + fused KPI replay': (replaced, both),
                'c: rollout_policy, no KPIs': (lambda: pe.rollout_policy(K, pt, seed=1, ret_env=ret, t0=0), pe.reset)}
    times = {k: [] for k in variants}
    for r in range(rounds + 1):
        for name, (fn, reset) in variants.items():
            t = timed(fn, reset)
            if r:                                                   # round 0 warms up
                times[name].append(t)
    ke.reset(); variants['a: rollout_policy(kpi=True)'][0]()
    kern = ke.last_kernels
    for name, ts in times.items():
        print(json.dumps({'n_env': E, 'f64_maps': f64, 'variant': name, 'us_per_step_median': round(statistics.median(ts), 3),
                          'min': round(min(ts), 3), 'max': round(max(ts), 3), 'rounds': len(ts)}), flush=True)
    print(json.dumps({'n_env': E, 'f64_maps': f64, 'kernel': kern, 'record_MB_per_launch': round(traj.numel() * 4 / 1e6, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--sizes', default='32768,65536')
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'policy_kpi_probe.log'))
    ap.add_argument('--step-timeout', type=int, default=240, help='seconds one (size, precision model) child may take')
    ap.add_argument('--worker', nargs=2, metavar=('N_ENV', 'F64'), help='internal: measure one (size, precision model) in this process')
    args = ap.parse_args()
    if args.worker:
        sys.path.insert(0, str(Path(__file__).resolve().parent))
        worker(int(args.worker[0]), 'chain' if args.worker[1] == 'chain' else False, args.rounds)
        return
    lines = []
    for E in args.sizes.split(','):
        for f64 in ('chain', 'fp32'):
            cmd = ['timeout', '-k', '10', str(args.step_timeout), sys.executable, __file__, '--rounds', str(args.rounds), '--worker', E, f64]
            p = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(p.stdout)
            sys.stdout.flush()
            lines.append(p.stdout)
            if p.returncode:                                        # nothing more on the GPU after a failure
                sys.stderr.write(p.stderr[-4000:])
                Path(args.out).write_text(''.join(lines) + f'FAILED: {" ".join(cmd)} -> exit {p.returncode}\n')
                sys.exit(p.returncode)
    Path(args.out).write_text(''.join(lines))


if __name__ == '__main__':
    main()
