"""profiles/policy_kpi_parity.md from the `CL_PARITY_REPORT` file of one run of tests/test_gpu_policy_kpi_rollout.py:

    CL_PARITY_REPORT=parity.jsonl python -m pytest tests/test_gpu_policy_kpi_rollout.py -q
    python scripts/policy_kpi_parity_table.py parity.jsonl > profiles/policy_kpi_parity.md

Readings are the worst |got - ref| / (1e-4 + 1e-4 |ref|) of a quantity (the plain bar), except the teacher-forced action deviations, which are
absolute.  A row is the worst over the reward kinds and batch sizes of its cell."""
import json
import re
import sys
from collections import defaultdict

PREC = {'chain': 'float64 chain', 'False': 'fp32'}


def main():
    rows = [json.loads(line) for line in open(sys.argv[1]) if line.strip()]
    rows = [r for r in rows if 'test_gpu_policy_kpi_rollout' in r.get('test', '')]
    print('# The closed-loop policy rollout with streaming KPIs: parity on MI355X\n')
    print('`tests/test_gpu_policy_kpi_rollout.py`, one run with `CL_PARITY_REPORT` set, summarised by `scripts/policy_kpi_parity_table.py`.  Readings '
          'are in units of the plain bar `1e-4 + 1e-4 |ref|`.  The comparisons against single steps are GATED at the tolerances of '
          '`_compare_step_outputs` / `_compare_kpi_planes` / `_finalised_close` (tests/test_gpu_rollout_kpi.py), not at the bar: the bar reading is '
          'recorded beside them.\n')
    cells, n = defaultdict(lambda: defaultdict(float)), 0
    for r in rows:
        m = re.fullmatch(r'policy kpi rollout vs single steps (\w+) (\w+) E=(\d+) f64_maps=(\w+) vec=(\w+)', r.get('label') or '')
        if m:
            n += 1
            for q, v in r['worst'].items():
                key = (m.group(1), PREC[m.group(4)], m.group(5).replace('None', 'default'))
                cells[key][q] = max(cells[key][q], v)
    qs = ['soc', 'net', 'reward', 'state', 'out_env', 'return', 'kpi_bldg', 'kpi_env']
    print(f'## Check 2: `cl_rollout_policy_kpi_kernel` against single steps fed the recorded actions\n\nK = 30, sigma = 0.1, E = 64 / 260 / 4096.  {n} checks.\n')
    print('| district | battery map | envs per lane | ' + ' | '.join(qs) + ' | worst |\n|' + '---|' * (len(qs) + 4))
    for key in sorted(cells):
        c = cells[key]
        print('| ' + ' | '.join(key) + ' | ' + ' | '.join(f'{c[q]:.4f}' if q in c else '' for q in qs) + f' | **{max(c.values()):.4f}** |')
    for r in rows:
        if (r.get('label') or '').endswith('month boundary'):
            print('\nMonth boundary (720 + 20 steps, g2022_p1_year): ' + ', '.join(f'{k} {v:.4f}' for k, v in r['worst'].items()) + '.')
    fin = [(re.fullmatch(r'policy kpi finalised (\w+) f64_maps=(\w+)', r.get('label') or ''), r) for r in rows]
    fin = [(m, r) for m, r in fin if m]
    print(f'\n## Check 3: finalised KPIs of `evaluate()` after 57 steps against an env stepping the recorded actions\n\n{len(fin)} checks.\n')
    print('| district | battery map | building KPIs | district KPIs |\n|---|---|---|---|')
    for m, r in fin:
        print(f"| {m.group(1)} | {PREC[m.group(2)]} | {r['worst']['building']:.4f} | {r['worst']['district']:.4f} |")
    tf = [(re.fullmatch(r'policy kpi teacher-forced f64_maps=(\w+) vec=(\d) H=(\d+) sigma=(\S+)', r.get('label') or ''), r) for r in rows]
    tf = [(m, r) for m, r in tf if m]
    print(f'\n## Check 4: teacher-forced actions\n\nWorst absolute deviation from the float64 MLP on the recorded inputs, beside a float32 torch '
          f"evaluation's (K = 24, E = 260, g2022_all); gate: kernel <= 4 x float32 torch.  {len(tf)} checks.\n")
    print('| battery map | envs per lane | H | sigma | kernel | float32 torch | ratio |\n|---|---|---|---|---|---|---|')
    for m, r in sorted(tf, key=lambda x: x[0].groups()):
        w = r['worst']
        print(f"| {PREC[m.group(1)]} | {m.group(2)} | {m.group(3)} | {0 if m.group(4) == 'None' else m.group(4)} | {w['kernel']:.3e} | {w['float32_torch']:.3e} | {w['ratio']:.2f} |")
    if tf:
        print(f"\nWorst ratio: {max(r['worst']['ratio'] for _, r in tf):.2f}.")
    fr = [(re.fullmatch(r'policy kpi free-running (\w+) f64_maps=(\w+)', r.get('label') or ''), r) for r in rows]
    fr = [(m, r) for m, r in fr if m]
    print('\nFree-running against the CPU oracle\'s closed loop (K = 48 from reset, E = 64, H = 16; gate: the plain bar):\n')
    print('| reward | battery map | soc | net | reward | district_net | degraded_capacity |\n|---|---|---|---|---|---|---|')
    for m, r in fr:
        w = r['worst']
        print(f"| {m.group(1)} | {PREC[m.group(2)]} | " + ' | '.join(f'{w[k]:.4f}' for k in ('soc', 'net', 'reward', 'district_net', 'degraded_capacity')) + ' |')


if __name__ == '__main__':
    main()
