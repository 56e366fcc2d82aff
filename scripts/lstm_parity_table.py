"""profiles/lstm_parity.md from the `CL_PARITY_REPORT` file of one run of tests/test_gpu_lstm_synthetic.py:

    CL_PARITY_REPORT=parity.jsonl python -m pytest tests/test_gpu_lstm_synthetic.py -q -m gpu
    python scripts/lstm_parity_table.py parity.jsonl > profiles/lstm_parity.md

Teacher-forced rows: worst absolute deviation from the float64 reference of tests/lstm_ref_util.py over every (step, building, env) of a case,
the kernel's beside the same-precision numpy evaluation's, and their ratio (gate: 4).  Free-running rows: worst |T - T_ref| / (1e-4 + 1e-4 |T_ref|)."""
import json
import sys

CASES = {'a': 'trained models, distinct envs', 'b': 'matrix-core kernel, synthetic two-layer models', 'c': 'common-denominator cell update at its bound',
         'd': 'generic kernel, shapes', 'e': 'mixed districts', 'g': 'with the comfort KPI accumulators'}


def main():
    rows = [json.loads(line) for line in open(sys.argv[1]) if line.strip()]
    rows = [r for r in rows if 'test_gpu_lstm_synthetic' in r.get('test', '')]
    forced = [r for r in rows if 'ratio_temp' in r['worst']]
    free = [r for r in rows if r['label'].startswith('f ')]
    print('# LSTM temperature stage per env: parity on MI355X\n')
    print('`tests/test_gpu_lstm_synthetic.py` at 132 envs with a different delivered demand in every (step, building, env), one run with '
          '`CL_PARITY_REPORT` set, summarised by `scripts/lstm_parity_table.py`.  Reference: `tests/lstm_ref_util.py`, float64 from the raw state '
          'dicts.\n')
    print(f'## Teacher-forced: one env step from the carried rings and state\n\n36 steps (12 of warm-up); worst absolute deviation from float64 of the '
          f'kernel and of the evaluation at the kernel\'s own precision (float32 numpy; split 16-bit operands where the kernel splits) on the same inputs.  '
          f'Temperature in C, y = the normalised temperature ring row, state = h and c of every real unit.  Gate: ratio <= 4.  {len(forced)} cases.\n')
    print('| case | temperature: kernel | float32 | ratio | y: kernel | float32 | ratio | state: kernel | float32 | ratio | ComfortReward / bar |')
    print('|---|---|---|---|---|---|---|---|---|---|---|')
    for r in forced:
        w = r['worst']
        print(f"| {r['label']} | " + ' | '.join(f"{w[q + '_kernel']:.2e} | {w[q + '_f32']:.2e} | {w['ratio_' + q]:.2f}" for q in ('temp', 'y', 'state'))
              + f" | {w['reward']:.4f} |")
    print(f"\nWorst ratio: {max(max(r['worst']['ratio_' + q] for q in ('temp', 'y', 'state')) for r in forced):.2f}.  "
          'Case letters: ' + '; '.join(f'{k} = {v}' for k, v in CASES.items()) + '.\n')
    print(f'## Free-running: 60 steps from reset against `run_ref` in float64\n\nWorst reading per building in units of the plain bar '
          f'1e-4 + 1e-4 |T_ref| (gate: 1).  {len(free)} cases.\n')
    print('| case | building 0 | building 1 | building 2 | worst |')
    print('|---|---|---|---|---|')
    for r in free:
        w = r['worst']
        print(f"| {r['label'][2:]} | " + ' | '.join(f"{w[f'temp_{b}']:.4f}" if f'temp_{b}' in w else 'no dynamics' for b in range(3)) + f" | **{max(w.values()):.4f}** |")
    print(f"\nWorst reading: {max(max(r['worst'].values()) for r in free):.4f} x the bar.")


if __name__ == '__main__':
    main()
