"""profiles/policy_full_kpi_parity.md from the `CL_PARITY_REPORT` file of one run of tests/test_gpu_policy_full_kpi_rollout.py:

    CL_PARITY_REPORT=parity.jsonl python -m pytest tests/test_gpu_policy_full_kpi_rollout.py -q
    python scripts/policy_full_kpi_parity_table.py parity.jsonl > profiles/policy_full_kpi_parity.md

Readings are the worst |got - ref| / (1e-4 + 1e-4 |ref|) of a quantity (the plain bar), except the teacher-forced action deviations, which are
absolute.  A row is the worst over the reward kinds and batch sizes of its cell."""
import json
import re
import sys
from collections import defaultdict

PREC = {'chain': 'float64 chain', 'False': 'fp32'}


def main():
    rows = [json.loads(line) for line in open(sys.argv[1]) if line.strip()]
    rows = [r for r in rows if 'test_gpu_policy_full_kpi_rollout' in r.get('test', '')]
    print('# The closed-loop policy rollout of thermal districts with streaming KPIs: parity on MI355X\n')
    print('`tests/test_gpu_policy_full_kpi_rollout.py`, one run with `CL_PARITY_REPORT` set, summarised by `scripts/policy_full_kpi_parity_table.py`.  '
          'Readings are in units of the plain bar `1e-4 + 1e-4 |ref|`.  The comparisons against single steps are GATED at the two-paths tolerances of '
          'the test file (`_replay`, `_compare_kpi`, `_finalised_close`), not at the bar: the bar reading is recorded beside them.  A reading of 0.0000 '
          'is bit-equality.\n')
    cells, n = defaultdict(lambda: defaultdict(float)), 0
    for r in rows:
        m = re.fullmatch(r'thermal policy kpi rollout vs single steps (\w+) (\w+) E=(\d+) f64_maps=(\w+)', r.get('label') or '')
        if m:
            n += 1
            for q, v in r['worst'].items():
                key = (m.group(1), PREC[m.group(4)])
                cells[key][q] = max(cells[key][q], v)
    qs = ['soc', 'net', 'reward', 'state', 'out_env', 'return', 'kpi_bldg', 'kpi_env', 'detail']
    print(f'## Check 2: `cl_rollout_full_policy_kpi_kernel` against single steps fed the recorded actions\n\nK = 30, sigma = 0.1, E = 64 / 260.  {n} checks.  '
          '`detail`: the five `CLD_DETAIL_MIN` planes of the last step (chain engines only).\n')
    print('| district | battery map | ' + ' | '.join(qs) + ' | worst |\n|' + '---|' * (len(qs) + 3))
    for key in sorted(cells):
        c = cells[key]
        print('| ' + ' | '.join(key) + ' | ' + ' | '.join(f'{c[q]:.4f}' if q in c else '' for q in qs) + f' | **{max(c.values()):.4f}** |')
    for r in rows:
        if (r.get('label') or '').endswith('month boundary'):
            print('\nMonth boundary (720 + 20 steps, g2020_cz1, float64 chain): ' + ', '.join(f'{k} {v:.4f}' for k, v in r['worst'].items()) + '.')
    fin = [(re.fullmatch(r'thermal policy kpi finalised (\w+) f64_maps=(\w+)', r.get('label') or ''), r) for r in rows]
    fin = [(m, r) for m, r in fin if m]
    print(f'\n## Check 3: finalised KPIs of `evaluate()` after 57 steps against an env stepping the recorded actions\n\n{len(fin)} checks.\n')
    print('| district | battery map | building KPIs | district KPIs |\n|---|---|---|---|')
    for m, r in fin:
        print(f"| {m.group(1)} | {PREC[m.group(2)]} | {r['worst']['building']:.4f} | {r['worst']['district']:.4f} |")
    tf = [(re.fullmatch(r'thermal policy kpi teacher-forced f64_maps=(\w+) H=(\d+) sigma=(\S+)', r.get('label') or ''), r) for r in rows]
    tf = [(m, r) for m, r in tf if m]
    print(f'\n## Check 4: teacher-forced actions\n\nWorst absolute deviation from the float64 MLP on the recorded inputs, beside a float32 torch '
          f"evaluation's (K = 24, E = 260, g2020_cz1); gate: kernel <= 4 x float32 torch.  {len(tf)} checks.\n")
    print('| battery map | H | sigma | kernel | float32 torch | ratio |\n|---|---|---|---|---|---|')
    for m, r in sorted(tf, key=lambda x: x[0].groups()):
        w = r['worst']
        print(f"| {PREC[m.group(1)]} | {m.group(2)} | {0 if m.group(3) == 'None' else m.group(3)} | {w['kernel']:.3e} | {w['float32_torch']:.3e} | {w['ratio']:.2f} |")
    if tf:
        print(f"\nWorst ratio: {max(r['worst']['ratio'] for _, r in tf):.2f}.")
    fr = [r for r in rows if (r.get('label') or '').startswith('thermal policy kpi free-running')]
    print('\nFree-running against the CPU oracle\'s closed loop (K = 48 from reset, E = 64, H = 16, float64 chain; gate: the plain bar):\n')
    for r in fr:
        print(', '.join(f'{k} {v:.4f}' for k, v in r['worst'].items()) + '.')


if __name__ == '__main__':
    main()
