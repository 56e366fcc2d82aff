#!/usr/bin/env python
"""Compare the generated gfx950 code of every closed-loop policy unit between two trees of this repository.

    python scripts/isa_compare.py <parent-tree> <this-tree> [--unit NAME ...] [--map OLD=NEW ...] [--markdown]

`<parent-tree>` is a checkout of the commit to compare with (`git worktree add <dir> <commit>`).  For every `_Extension` of `<this-tree>`'s
`citylearn_amd/_lib.py` the unit's `.hip` of both trees is compiled to assembly with that unit's flags through `tests/test_isa_guards._asm`, the
kernels are paired by their template arguments, and per instantiation the tool prints whether the instruction streams are the same text (the
`.LBB` labels renamed in order of appearance, a kernel's own symbol replaced by a placeholder), the instruction counts (the length of `_asm`'s list,
label entries included -- behind a unit's last kernel that list runs on into the metadata, which is counted but not compared), the VGPRs and
the scratch bytes.  It compares instruction text and nothing else.  No GPU; exit status 1 if any
instantiation differs or has no partner.

A kernel whose name differs between the trees is paired through `--map`: `OLD=NEW` pairs `OLD<args>` with `NEW<args>`, and
`OLD=NEW<*, true>` pairs `OLD<args>` with `NEW<args, true>` (`NEW<1, *, true>`: with `NEW<1, args, true>`).  DEFAULT_MAP holds the renames of the
latest one-source change, the two thermal central-agent rollouts in one template (profiles/policy_full_central_one_source_isa.md); the maps of
the changes before it are written down in profiles/policy_full_one_source_isa.md and profiles/policy_one_source_isa.md as the `--map` arguments
that make those notes again."""
import argparse
import importlib.util
import re
import subprocess
import sys
import tempfile
from pathlib import Path

# parent name -> name in this tree (`*`: the parent's template arguments)
DEFAULT_MAP = {
    'cl_rollout_full_policy_central_kernel': 'cl_rollout_full_policy_central_kernel<*, false>',
    'cl_rollout_full_policy_central_deep_kernel': 'cl_rollout_full_policy_central_kernel<*, true>',
}


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Tmp:
    """What `_asm` needs of pytest's tmp_path_factory"""

    def __init__(self, root):
        self.root, self.n = Path(root), 0

    def mktemp(self, name):
        self.n += 1
        d = self.root / f'{name}{self.n}'
        d.mkdir()
        return d


def _demangle(names):
    out = subprocess.run(['/opt/rocm/llvm/bin/llvm-cxxfilt' if Path('/opt/rocm/llvm/bin/llvm-cxxfilt').exists() else 'c++filt', *names],
                         check=True, capture_output=True, text=True).stdout.split('\n')
    return dict(zip(names, out))


def _key(demangled):
    """`(anonymous namespace)::name<1, 0>(Args)` -> ('name', '1, 0') ('' for a kernel that is no template)"""
    m = re.match(r'^(?:void )?(?:\(anonymous namespace\)::)*(\w+)(?:<(.*?)>)?\(', demangled)
    return (m.group(1), m.group(2) or '') if m else None


def _normal(ins, symbol):
    labels = {}
    # (behind the unit's last kernel `_asm`'s list runs on into the metadata, which names the kernels: the stream ends at the last s_endpgm)
    ins = ins[:len(ins) - [i.split()[0] for i in reversed(ins)].index('s_endpgm')]

    def rename(m):
        return labels.setdefault(m.group(0), f'.L{len(labels)}')
    return [re.sub(r'\.LBB\d+_\d+', rename, i.replace(symbol, 'KERNEL')) for i in ins]


def _kernels(asm, src, flags, tmp):
    kernels, meta = asm(src, flags, tmp)
    pretty = _demangle(list(kernels))
    out = {}
    for sym, ins in kernels.items():
        key = _key(pretty[sym])
        if key is not None:
            out[key] = (_normal(ins, sym), dict(meta.get(sym, {}), n=len(ins)))
    return out


def _mapped(key, name_map):
    name, args = key
    new = name_map.get(name)
    if new is None:
        return key
    m = re.match(r'^(\w+)(?:<(.*)>)?$', new)
    return (m.group(1), m.group(2).replace('*', args) if m.group(2) else args)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('parent', type=Path)
    ap.add_argument('this', type=Path)
    ap.add_argument('--map', action='append', default=[], metavar='OLD=NEW', help='pair a renamed kernel (besides DEFAULT_MAP)')
    ap.add_argument('--unit', action='append', default=[], metavar='NAME', help='only the unit csrc/cl_NAME.hip (default: every policy unit)')
    ap.add_argument('--markdown', action='store_true', help='print table rows in the form of profiles/policy_one_source_isa.md')
    a = ap.parse_args()
    name_map = dict(DEFAULT_MAP, **dict(m.split('=', 1) for m in a.map))

    this = a.this.resolve()
    sys.path.insert(0, str(this))
    from citylearn_amd import _lib
    asm = _load(this / 'tests' / 'test_isa_guards.py', 'isa_guards')._asm
    units = [v for v in vars(_lib).values() if isinstance(v, _lib._Extension)]
    if a.unit:
        units = [u for u in units if Path(u.sources[0][0] if isinstance(u.sources[0], tuple) else u.sources[0]).stem[3:] in a.unit]
    bad = 0
    with tempfile.TemporaryDirectory() as d:
        tmp = _Tmp(d)
        for ext in units:
            src, flags = ext.sources[0] if isinstance(ext.sources[0], tuple) else (ext.sources[0], [])
            before = _kernels(asm, a.parent.resolve() / src.relative_to(this), flags, tmp)
            after = _kernels(asm, src, flags, tmp)
            print(f'## {src.name} {" ".join(flags)}'.rstrip())
            for key, (ins0, meta0) in before.items():
                new = _mapped(key, name_map)
                old_name, new_name = f'{key[0]}<{key[1]}>', f'{new[0]}<{new[1]}>'
                if new not in after:
                    print(f'{old_name}: NO PARTNER {new_name}')
                    bad += 1
                    continue
                ins1, meta1 = after.pop(new)
                same, n0, n1 = ins0 == ins1, meta0['n'], meta1['n']
                bad += not same
                cells = (f'{n0} / {n1}', f'{meta0.get("num_vgpr")} / {meta1.get("num_vgpr")}',
                         f'{meta0.get("private_seg_size")} / {meta1.get("private_seg_size")}')
                if a.markdown:
                    print(f'| `{old_name}` | `{new_name}` | {"yes" if same else "NO"} | {" | ".join(cells)} |')
                else:
                    print(f'{"identical" if same else "CHANGED  "}  {old_name} -> {new_name}: instructions {cells[0]}, VGPRs {cells[1]}, scratch bytes {cells[2]}')
            for key in after:
                print(f'{key[0]}<{key[1]}>: NO PARTNER in the parent')
                bad += 1
    print(f'{bad} instantiation(s) changed or unpaired' if bad else 'every instantiation identical')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
