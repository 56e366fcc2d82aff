"""In-process A/B of the headline step's strip mapping (csrc/cl_kernels.hip: lean_step_body, STRIPS): two engines at 17 buildings x 65 536 envs
under the float64 chain -- the default (the 17th building as four 64-env strips behind the last four waves' main tile) and `cl_tuning.lean_variant`
= 32 (wave 0 takes it as a second tile) -- each captured once into a hipGraph of `steps` step launches, replayed alternately round by round.
us per step and round, then min / median per variant.  Usage: lean_strips_ab.py [envs] [rounds] [buildings]"""
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from citylearn_amd import load_district                 # noqa: E402
from citylearn_amd.data import sample_schema            # noqa: E402
from citylearn_amd.engine import StepEngine             # noqa: E402
from citylearn_amd.synthetic import tile_district       # noqa: E402

STEPS, REPS = 200, 5


def capture(eng, acts, stream):
    with torch.cuda.stream(stream):
        for t in range(3):
            eng.step(acts[t % 2], 1 + t)
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            for t in range(STEPS):
                eng.step(acts[t % 2], 1 + t % 600)
        g.replay()
        stream.synchronize()
    return g


def timed(g, stream):
    with torch.cuda.stream(stream):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        for _ in range(REPS):
            g.replay()
        ev1.record(stream)
        stream.synchronize()
    return ev0.elapsed_time(ev1) / (STEPS * REPS) * 1e3


if __name__ == '__main__':
    E = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 12
    B = int(sys.argv[3]) if len(sys.argv) > 3 else 17
    spec = load_district(sample_schema('citylearn_challenge_2022_phase_all_720h'))
    if B != 17:
        spec = tile_district(spec, B, jitter=0.0)
    tab = spec.episode_tables(0)
    low, high = spec.action_limits()
    lo, hi = torch.from_numpy(low).cuda(), torch.from_numpy(high).cuda()
    acts = [lo[:, None] + torch.rand((len(low), E), device='cuda') * (hi - lo)[:, None] for _ in range(2)]
    stream = torch.cuda.Stream()
    variants = {'strips': {}, 'second_tile': dict(lean_variant=32)}
    engines = {k: StepEngine(tab, E, f64_maps='chain', tuning=v) for k, v in variants.items()}
    graphs = {}
    for k, e in engines.items():
        e.trace_kernels()
        graphs[k] = capture(e, acts, stream)
        print(f'{k}: {e.last_kernels}', flush=True)
    us = {k: [] for k in engines}
    for r in range(rounds):
        for k in (list(engines) if r % 2 == 0 else list(engines)[::-1]):
            us[k].append(timed(graphs[k], stream))
        print(f'round {r:2d}: ' + '  '.join(f'{k} {us[k][-1]:.3f} us' for k in engines), flush=True)
    for k, v in us.items():
        print(f'{k}: min {min(v):.3f}  median {statistics.median(v):.3f}  max {max(v):.3f} us  (B={B}, E={E}, {rounds} rounds)', flush=True)
