"""profiles/policy_full_chunk_parity.md from the `CL_PARITY_REPORT` file of one run of tests/test_gpu_policy_full_chunk_rollout.py:

    CL_PARITY_REPORT=parity.jsonl python -m pytest tests/test_gpu_policy_full_chunk_rollout.py -q
    python scripts/policy_full_chunk_parity_table.py parity.jsonl > profiles/policy_full_chunk_parity.md

Readings are the worst |got - ref| / (1e-4 + 1e-4 |ref|) of a quantity (the plain bar), except the teacher-forced action deviations and the
return differences, which are absolute."""
import json
import re
import sys

PREC = {'chain': 'float64 chain', 'False': 'fp32'}


def main():
    rows = [json.loads(line) for line in open(sys.argv[1]) if line.strip()]
    rows = [r for r in rows if 'test_gpu_policy_full_chunk_rollout' in r.get('test', '')]
    print('# The building-chunked closed-loop policy rollout of thermal districts: parity on MI355X\n')
    print('`tests/test_gpu_policy_full_chunk_rollout.py`, one run with `CL_PARITY_REPORT` set, summarised by `scripts/policy_full_chunk_parity_table.py`.  '
          'Readings are in units of the plain bar `1e-4 + 1e-4 |ref|` unless marked; a reading of 0.0000 is bit-equality.\n')
    one = [(re.fullmatch(r'chunked thermal policy rollout vs one-row kernel t16 b_chunk=(\d+) (\w+) f64_maps=(\w+) vec=(\d)', r['label']), r) for r in rows]
    one = [(m, r) for m, r in one if m]
    print(f'## Check 1: `cl_rollout_full_policy_chunk_kernel` against `cl_rollout_full_policy_kernel` on sixteen buildings\n\nK = 30, sigma = 0.1, E = 260.  '
          f'{len(one)} checks.  `bit-equal`: record, six state planes and `out_bldg[:2]` equal bit for bit (recorded, not gated); `district sums`: `out_env`, '
          'whose sums are associated per chunk first; `return`: worst absolute difference.\n')
    print('| chunks | battery map | envs per lane | reward | bit-equal | district sums | return (abs) |\n|---|---|---|---|---|---|---|')
    for m, r in one:
        w = r['worst']
        print(f"| {'8 + 8' if m.group(1) == '8' else '6 + 6 + 4'} | {PREC[m.group(3)]} | {m.group(4)} | {m.group(2)} | {'yes' if w['bit_equal'] else 'NO'} | {w['district_sums']:.4f} | {w['return']:.2e} |")
    print(f"\nBit-equal in {sum(1 for _, r in one if r['worst']['bit_equal'])} of {len(one)} cases.")
    rep = [r for r in rows if r['label'].startswith('thermal policy rollout vs single steps under an outage')]
    worst = {}
    for r in rep:
        for k, v in r['worst'].items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f'\n## Check 2: replay through single steps\n\nGated at `_replay`\'s two-paths tolerances (72 cases: 17 buildings as 6 + 6 + 5, 8 + 8 + 1 and 16 + 1, 24 as '
          f'8 + 8 + 8, 33 as 7 + 7 + 7 + 7 + 5, the 17-building outage district; E = 64 / 260, both battery maps, three rewards; and 1024 buildings as 128 x 8 at E = 64).  `_replay` records the plain-bar reading on the '
          f'outage district only: worst over its {len(rep)} cases ' + ', '.join(f'{k} {v:.4f}' for k, v in worst.items()) + '.')
    tf = [(re.fullmatch(r'chunked thermal policy teacher-forced t17 f64_maps=(\w+) vec=(\d) H=(\d+)', r['label']), r) for r in rows]
    tf = [(m, r) for m, r in tf if m]
    print(f'\n## Check 3: teacher-forced actions\n\nWorst absolute deviation from the float64 MLP on the recorded inputs, beside a float32 torch evaluation\'s '
          f'(17 buildings, K = 24, E = 260, sigma = 0.1); gate: kernel <= 4 x float32 torch.  {len(tf)} checks.\n')
    print('| battery map | envs per lane | H | kernel | float32 torch | ratio |\n|---|---|---|---|---|---|')
    for m, r in tf:
        w = r['worst']
        print(f"| {PREC[m.group(1)]} | {m.group(2)} | {m.group(3)} | {w['kernel']:.3e} | {w['float32_torch']:.3e} | {w['ratio']:.2f} |")
    if tf:
        print(f"\nWorst ratio: {max(r['worst']['ratio'] for _, r in tf):.2f}.")
    fr = [(re.fullmatch(r'chunked thermal policy rollout (\w+) f64=(\w+)', r['label']), r) for r in rows]
    fr = [(m, r) for m, r in fr if m]
    qs = ['soc', 'cs', 'ds', 'net', 'reward', 'district_net', 'district_net_of_record', 'degraded_capacity']
    print('\n## Check 4: free-running against the CPU oracle\'s closed loop\n\nK = 48 from reset, E = 64, H = 16; gate: the plain bar.  `district_net`: the folded '
          '`out_env` of the last step; `district_net_of_record`: the recorded nets summed over the buildings, every step.\n')
    print('| district | battery map | ' + ' | '.join(qs) + ' | worst |\n|' + '---|' * (len(qs) + 3))
    for m, r in fr:
        w = r['worst']
        print(f'| {m.group(1)} | {PREC[m.group(2)]} | ' + ' | '.join(f'{w[q]:.4f}' for q in qs) + f' | **{max(w.values()):.4f}** |')
    print('\nChecks 5 - 7 (split launches and checkpoint, env blocks, the accumulated return) are bit-for-bit comparisons and record nothing.')


if __name__ == '__main__':
    main()
