"""profiles/fused_rollout_geometry_parity.md from the `CL_PARITY_REPORT` file of one run of tests/test_gpu_rollout_geometry.py:

    CL_PARITY_REPORT=parity.jsonl python -m pytest tests/test_gpu_rollout_geometry.py -q
    python scripts/geometry_parity_table.py parity.jsonl > profiles/fused_rollout_geometry_parity.md

Every reading is the worst |got - ref| / (1e-4 + 1e-4 |ref|) of a quantity (the plain bar), except the teacher-forced action deviations, which
are absolute.  Rows are the worst over the reward kinds (and batch sizes) of a (district, precision model, envs per lane) cell."""
import json
import re
import sys
from collections import defaultdict

PREC = {'chain': 'float64 chain', 'False': 'fp32'}
ORDER = ['b1', 'b2', 'b16', 'b31', 'b32', 'het17']


def table(rows, pattern, keys, quantities, title, head):
    """Group the records whose label matches `pattern` by the named groups `keys`; per group the worst of every quantity."""
    cells = defaultdict(lambda: defaultdict(float))
    n = 0
    for r in rows:
        m = re.fullmatch(pattern, r.get('label') or '')
        if not m:
            continue
        n += 1
        cell = cells[tuple(m.group(k) for k in keys)]
        for q, v in r['worst'].items():
            cell[q] = max(cell[q], v)
    if not cells:
        return
    print(f'## {title}\n\n{head}  {n} checks.\n')
    print('| ' + ' | '.join(k.replace('f64', 'battery map').replace('vec', 'envs per lane').replace('name', 'district') for k in keys) + ' | '
          + ' | '.join(quantities) + ' | worst |')
    print('|' + '---|' * (len(keys) + len(quantities) + 1))
    worst_all = 0.0
    for key in sorted(cells, key=lambda k: (ORDER.index(k[0]) if k[0] in ORDER else 99, k[1:])):
        c = cells[key]
        shown = [PREC.get(v, v) if k == 'f64' else v for k, v in zip(keys, key)]
        worst_all = max(worst_all, max(c.values()))
        print('| ' + ' | '.join(shown) + ' | ' + ' | '.join(f'{c[q]:.4f}' if q in c else '' for q in quantities) + f' | **{max(c.values()):.4f}** |')
    print(f'\nWorst reading of the section: {worst_all:.4f} x the plain bar.\n')


def main():
    rows = [json.loads(line) for line in open(sys.argv[1]) if line.strip()]
    rows = [r for r in rows if 'test_gpu_rollout_geometry' in r.get('test', '')]
    print('# Fused rollouts at the geometry edges: parity on MI355X\n')
    print('`tests/test_gpu_rollout_geometry.py` over the districts of `tests/district_util.py` (1, 2, 16, 31, 32 buildings and the heterogeneous '
          '`het17`), one suite run with `CL_PARITY_REPORT` set, summarised by `scripts/geometry_parity_table.py`.  Readings are in units of the plain '
          'bar `1e-4 + 1e-4 |ref|`; a row is the worst over the reward kinds (and batch sizes) of its cell.  The comparisons against single steps are '
          'GATED at the tolerances of `_compare_step_outputs` / `_compare_kpi_planes` (tests/test_gpu_rollout_kpi.py), not at the bar: the bar reading '
          'is recorded beside them.\n')
    table(rows, r'single steps (?P<name>\w+) (?P<kind>\w+) f64_maps=(?P<f64>\w+)', ['name', 'f64'],
          ['soc', 'net', 'reward', 'd_net', 'district_reward'], 'The reference side: `StepEngine.step` against the float64 CPU oracle',
          'K = 48 random actions per env, teacher-forced, E = 68, four reward kinds; gate: the plain bar.')
    table(rows, r'kpi rollout vs single steps (?P<name>\w+) (?P<kind>\w+) E=(?P<E>\d+) f64_maps=(?P<f64>\w+) vec=(?P<vec>\d)', ['name', 'f64', 'vec'],
          ['state', 'net', 'reward', 'out_env', 'return', 'kpi_bldg', 'kpi_env'], '`cl_rollout_kpi_kernel` against single steps',
          'Launches of 30 + 27 open-loop steps from t0 = 0, E = 260 and 64; recorded.')
    table(rows, r'kpi rollout, on-device policy \+ windows (?P<name>\w+) f64_maps=(?P<f64>\w+)', ['name', 'f64'], ['state', 'kpi_bldg', 'kpi_env'],
          '`cl_rollout_kpi_kernel`, Philox policy and three episode windows against the launch sequence', 'E = 640, K = 30; recorded.')
    table(rows, r'policy rollout vs single steps (?P<name>\w+) (?P<kind>\w+) f64_maps=(?P<f64>\w+) vec=(?P<vec>\d)', ['name', 'f64', 'vec'],
          ['soc', 'net', 'reward', 'state', 'out_env', 'return'], '`cl_rollout_policy_kernel` replayed through `step()`',
          'K = 30, E = 260, sigma = 0.1, MARL and RewardFunction; recorded.')
    table(rows, r'policy rollout free-running (?P<name>\w+) (?P<kind>\w+) f64_maps=(?P<f64>\w+) vec=(?P<vec>\d)', ['name', 'f64', 'vec'],
          ['soc', 'net', 'reward', 'district_net', 'degraded_capacity'], '`cl_rollout_policy_kernel` free-running against the CPU oracle',
          'K = 48 from reset, E = 64, H = 16, RewardFunction and MARL; gate: the plain bar.')
    tf = [(re.fullmatch(r'teacher-forced (\w+) f64_maps=(\w+) vec=(\d) H=(\d+) sigma=(\S+)', r.get('label') or ''), r) for r in rows]
    tf = [(m, r) for m, r in tf if m]
    if tf:
        print(f'## Teacher-forced actions of `cl_rollout_policy_kernel`\n\nWorst absolute deviation from the float64 MLP on the recorded inputs, beside a '
              f'float32 torch evaluation\'s (K = 24, E = 260); gate: kernel <= 4 x float32 torch.  {len(tf)} checks.\n')
        print('| district | battery map | envs per lane | H | sigma | kernel | float32 torch | ratio |')
        print('|---|---|---|---|---|---|---|---|')
        for m, r in sorted(tf, key=lambda x: (ORDER.index(x[0].group(1)), x[0].groups()[1:])):
            w = r['worst']
            print(f"| {m.group(1)} | {PREC[m.group(2)]} | {m.group(3)} | {m.group(4)} | {0 if m.group(5) == 'None' else m.group(5)} | {w['kernel']:.3e} | "
                  f"{w['float32_torch']:.3e} | {w['ratio']:.2f} |")
        print(f"\nWorst ratio: {max(r['worst']['ratio'] for _, r in tf):.2f}.\n")

    # the LDS request of the largest launches, from the kernel's own formula and constants (what the host passes as the dynamic LDS size)
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    text = (root / 'citylearn_amd' / 'csrc' / 'cl_rollout.h').read_text()
    s, nb = (int(re.search(rf'constexpr int {k} = (\d+);', text).group(1)) for k in ('CL_RKPI_S', 'CL_RKPI_NB'))
    sys.path.insert(0, str(root))
    from citylearn_amd import abi
    per_cond = abi.CLKE_PER_COND
    lds = lambda nw, tile: 4 * (s * nw * tile + per_cond * tile + 16 + s * 4 * nb + 5 * nb)
    ran = sorted({m.group(1) for r in rows for m in [re.fullmatch(r'kpi rollout vs single steps (b31|b32) \w+ E=\d+ f64_maps=\w+ vec=2', r.get('label') or '')] if m})
    print('## LDS request of `cl_rollout_kpi_kernel`\n')
    print(f'`rollout_kpi_lds_floats(nw, tile) * 4`, the dynamic LDS size the host passes to the launch (not read back from a profiler): '
          f'**{lds(16, 128)} bytes** at nw = 16 and two envs per lane ({", ".join(ran) or "no district"} at `vec = 2` in this run: '
          f'`last_kernels` named `cl_rollout_kpi_kernel<2, ..>` and the cases passed -- the launches that go through the opt-in above 65 536 bytes), '
          f'{lds(16, 64)} at nw = 16 and one env per lane, {lds(9, 128)} at 17 buildings (nw = 9) and two envs per lane, '
          f'{lds(13, 128)} / {lds(14, 128)} at nw = 13 / 14: the opt-in starts at 27 buildings.')


if __name__ == '__main__':
    main()
