"""Mode B with streaming KPIs: what K = 24 steps of the on-device policy cost per step (GPU box), one process, the variants alternating
launch by launch:
  (a) rollout(kpi=True)              -- the launch sequence cl_rollout_seq_f32 (policy, cl_step_lean_kpi*_kernel, return per step)
  (b) rollout(kpi=True, fused=True)  -- ONE launch, cl_rollout_kpi_kernel keeps the accumulators
  (c) rollout() of an engine without KPIs -- the fused rollout as it was (cl_rollout_kernel)
at 17 x 32 768 and 17 x 65 536, default precision (the float64 chain) and the fp32 map.  Device events around every call; medians over
ROUNDS rounds of a / b / c / a / b / c ...  Usage: python scripts/rollout_kpi_probe.py [rounds [envs ...]]"""
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / 'tests'))
from golden_util import golden
from citylearn_amd.engine import StepEngine

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
K = 24
g = golden('g2022_all'); spec = g.spec(); tab = spec.episode_tables(0)
low, high = spec.action_limits()

for E in ([int(x) for x in sys.argv[2:]] or [32768, 65536]):
    for f64 in (None, False):
        eng = {'a': StepEngine(tab, E, kpi=True, f64_maps=f64), 'b': StepEngine(tab, E, kpi=True, f64_maps=f64), 'c': StepEngine(tab, E, f64_maps=f64)}
        fused = {'a': None, 'b': True, 'c': None}
        ret = torch.zeros(E, device='cuda')
        names = {}
        for v, e in eng.items():
            e.set_action_limits(low, high)
            e.trace_kernels()
            for i in range(3):                                   # warm-up: code objects, the policy scratch planes
                e.rollout(K, seed=i, ret_env=ret, t0=1, fused=fused[v])
            names[v] = e.last_kernels
        torch.cuda.synchronize()
        times = {v: [] for v in eng}
        for i in range(ROUNDS):
            for v, e in eng.items():
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                for j in range(4):                               # 4 x 24 steps per sample
                    e.rollout(K, seed=i, ret_env=ret, t0=1 + ((4 * i + j) * K) % 600, fused=fused[v])
                ev1.record()
                torch.cuda.synchronize()
                times[v].append(ev0.elapsed_time(ev1) / (4 * K) * 1e3)
        med = {v: statistics.median(t) for v, t in times.items()}
        lo = {v: min(t) for v, t in times.items()}
        hi = {v: max(t) for v, t in times.items()}
        prec = 'chain' if eng['a'].f64_chain else 'fp32'
        print(f'17 x {E}, K = {K}, {prec}: ' + ' | '.join(f'({v}) {med[v]:.2f} us/step [{lo[v]:.2f} .. {hi[v]:.2f}]' for v in 'abc')
              + f' | a/b = {med["a"] / med["b"]:.2f}, b/c = {med["b"] / med["c"]:.2f}', flush=True)
        for v in 'abc':
            print(f'    ({v}) {names[v]}', flush=True)
        del eng
