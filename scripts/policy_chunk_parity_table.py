"""The parity record of tests/test_gpu_policy_chunk_rollout.py as markdown: `CL_PARITY_REPORT=<file> pytest tests/test_gpu_policy_chunk_rollout.py`
appends one JSON line per check (tests/golden_util.py `record_worst` / `check_worst`); this prints one table per check of the file.

    python scripts/policy_chunk_parity_table.py parity.jsonl > profiles/policy_chunk_parity.md"""
import json
import sys

SECTIONS = [('test_1', 'Check 1: `cl_rollout_policy_chunk_kernel` against `cl_rollout_policy_kernel` on districts one workgroup row holds',
             'K = 30, sigma = 0.1, E = 260.  `bit_equal` = 1: record, the three battery state planes and `out_bldg[:2]` equal bit for bit (recorded, not gated); '
             '`district_sums`: `out_env` in units of the plain bar, its sums associated per chunk first; `return`: worst absolute difference.'),
            ('test_2', 'Check 2: replayed through `step()` of a second engine',
             'K = 30, sigma = 0.1.  Units of the plain bar `1e-4 + 1e-4 |ref|`; `return_dev_kernel` / `return_dev_steps`: absolute deviation of either '
             "path's float32 return from the float64 sum of the recorded reward plane."),
            ('test_3', 'Check 3: teacher-forced actions', 'E = 260, K = 24, sigma = 0.1.  Worst |action - float64 MLP|; gate: `ratio` <= 4.'),
            ('test_4', 'Check 4: free-running against the CPU oracle loop', 'K = 48, E = 64, H = 16.  Units of the plain bar; gate 1.0.'),
            ('test_8', 'Check 8: env level against `capture_rollout` with `torch_policy`', '33 buildings x 256 envs, K = 24: worst |action difference| and its tolerance.')]


def main():
    rows = [json.loads(line) for line in open(sys.argv[1]) if line.strip()]
    print('# The building-chunked closed-loop policy rollout of battery + PV districts: parity on MI355X\n')
    print('`tests/test_gpu_policy_chunk_rollout.py`, one run with `CL_PARITY_REPORT` set, summarised by `scripts/policy_chunk_parity_table.py`.  '
          'A reading of 0.0000 in units of the bar is bit-equality.\n')
    for prefix, title, note in SECTIONS:
        sel = [r for r in rows if r['test'].split('::')[-1].startswith(prefix)]
        if not sel:
            continue
        keys = list(dict.fromkeys(k for r in sel for k in r['worst']))
        print(f'## {title}\n\n{note}  {len(sel)} checks.\n')
        print('| case | ' + ' | '.join(keys) + ' |')
        print('|---|' + '---|' * len(keys))
        for r in sel:
            fmt = lambda v: '' if v is None else (f'{v:.2e}' if 0 < abs(v) < 1e-3 else f'{v:.4f}')
            print(f"| {r.get('label', '')} | " + ' | '.join(fmt(r['worst'].get(k)) for k in keys) + ' |')
        if prefix == 'test_1':
            print(f"\nBit-equal in {sum(int(r['worst']['bit_equal']) for r in sel)} of {len(sel)} cases.")
        print()


if __name__ == '__main__':
    main()
