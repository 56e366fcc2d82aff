"""Static guard on the generated gfx950 code of the two headline lean step kernels (no GPU: hipcc cross-compiles to assembly, like
tests/test_isa_guards.py): no wave sits out the acknowledgement of its own plane stores.  On gfx9 a store counts in `vmcnt` like a load, so
ANY `s_waitcnt vmcnt(n)` behind a burst of stores waits for stores -- whatever the compiler placed it for (csrc/cl_kernels.hip, STORE
ACKNOWLEDGEMENTS; profiles/store_ack_waits.md holds the counts of the commit before, where every check below fails).

A building's plane stores are a burst of five `global_store_dwordx4 .. nt` (three state planes, net, reward) with address arithmetic in
between; bursts are hundreds of instructions apart (a building's arithmetic).  `cl_step_lean_chain_kernel<4, true>` holds four bursts -- two
buildings of the generic body, then, behind the first `sched_barrier` marker, two of the uniform body -- and `cl_step_lean_kernel<4, false,
true>` two."""
import os
import re
import subprocess

import pytest

from citylearn_amd import _lib

CHAIN = r'cl_step_lean_chain_kernelILi4ELb1EE'
FP32 = r'cl_step_lean_kernelILi4ELb0ELb1EE'
BURST_GAP = 64              # instructions: more than between two stores of a building, far fewer than a building's arithmetic


def _asm(src, extra, tmp_path_factory):
    """{kernel: instruction list} with 'SCHED_BARRIER' entries where the assembly prints the marker, and the kernels' register / scratch figures."""
    out = tmp_path_factory.mktemp('isa_waits') / (src.stem + '.s')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    flags = [f for f in _lib.HIPCC_FLAGS if f not in ('-shared', '-fPIC')]
    subprocess.run([hipcc, *flags, *extra, '-S', '--cuda-device-only', str(src), '-o', str(out)], check=True, capture_output=True)
    return parse(out.read_text())


def parse(text):
    kernels, meta, cur = {}, {}, None
    for line in text.splitlines():
        m = re.match(r'^(_Z\w+):', line)
        if m:
            cur = m.group(1); kernels[cur] = []
            continue
        m = re.match(r'\s*\.set (_Z\w+)\.(num_vgpr|private_seg_size), (\d+)', line)
        if m:
            meta.setdefault(m.group(1), {})[m.group(2)] = int(m.group(3))
            continue
        t = line.split()
        if cur is None or not t:
            continue
        if t[0] == ';' and 'sched_barrier' in line:
            kernels[cur].append('SCHED_BARRIER')
        elif not t[0].startswith(('.', ';')):
            kernels[cur].append(line.strip())
    return kernels, meta


def _is_plane_store(x):
    return x.startswith('global_store_dwordx4') and x.endswith(' nt')


def _is_f64(x):
    return re.match(r'v_\w+_f64', x) is not None


def _has_vmcnt(x):
    return x.startswith('s_waitcnt') and 'vmcnt(' in x


def bursts(ins):
    """[(first, last)] instruction indices of the bursts of plane stores"""
    out = []
    for i, x in enumerate(ins):
        if not _is_plane_store(x):
            continue
        if out and i - out[-1][1] <= BURST_GAP:
            out[-1][1] = i
        else:
            out.append([i, i])
    return [tuple(b) for b in out]


def waits_behind_bursts(ins):
    """For every burst: the `s_waitcnt` with a vmcnt field between its last store and the next s_barrier / float64 instruction (first hit only)."""
    hits = []
    for _, last in bursts(ins):
        hit = None
        for k in range(last + 1, len(ins)):
            if ins[k].startswith(('s_barrier', 's_endpgm')) or _is_f64(ins[k]):
                break
            if _has_vmcnt(ins[k]):
                hit = (k, ins[k])
                break
        hits.append(hit)
    return hits


def waits_inside_bursts(ins):
    return [[(k, ins[k]) for k in range(first, last) if _has_vmcnt(ins[k])] for first, last in bursts(ins)]


def waits_behind_barrier(ins, start):
    """`s_waitcnt .. vmcnt(0)` between the first s_barrier behind instruction `start` and the first `global_store_dword` (out_env) behind it"""
    b = next(k for k in range(start, len(ins)) if ins[k].startswith('s_barrier'))
    hits = []
    for k in range(b + 1, len(ins)):
        if re.match(r'global_store_dword\s', ins[k]) or ins[k].startswith('s_endpgm'):
            break
        if ins[k].startswith('s_waitcnt') and 'vmcnt(0)' in ins[k]:
            hits.append((k, ins[k]))
    return hits


def bodies(ins):
    """The bursts of the kernel grouped by body: two buildings each; the uniform body's are the ones behind the first sched_barrier marker."""
    bs = bursts(ins)
    marker = ins.index('SCHED_BARRIER') if 'SCHED_BARRIER' in ins else len(ins)
    return [b for b in bs if b[0] < marker], [b for b in bs if b[0] > marker]


def report(kernels, meta, pattern):
    """The figures profiles/store_ack_waits.md tabulates (also for a tree that fails the assertions)."""
    k = _one(kernels, pattern)
    ins = kernels[k]
    generic, uniform = bodies(ins)
    return {'kernel': k, 'bursts': (len(generic), len(uniform)), 'stores_per_burst': [sum(_is_plane_store(x) for x in ins[a:b + 1]) for a, b in bursts(ins)],
            'behind_bursts': [h[1] if h else None for h in waits_behind_bursts(ins)],
            'inside_bursts': [[h[1] for h in w] for w in waits_inside_bursts(ins)],
            'behind_barrier': [[h[1] for h in waits_behind_barrier(ins, body[-1][1])] for body in (generic, uniform) if body],
            'num_vgpr': meta[k].get('num_vgpr'), 'private_seg_size': meta[k].get('private_seg_size')}


@pytest.fixture(scope='module')
def units(tmp_path_factory):
    (main, _), (noslp, noslp_flags) = [(u, []) if not isinstance(u, tuple) else u for u in _lib.LIB_SOURCES]
    return _asm(main, [], tmp_path_factory), _asm(noslp, noslp_flags, tmp_path_factory)


def _one(kernels, pattern):
    names = [k for k in kernels if re.search(pattern, k)]
    assert len(names) == 1, (pattern, names)
    return names[0]


def _kernel(units, pattern):
    (main, main_meta), (noslp, noslp_meta) = units
    kernels, meta = (main, main_meta) if pattern == CHAIN else (noslp, noslp_meta)
    k = _one(kernels, pattern)
    return kernels[k], meta[k]


@pytest.mark.parametrize('pattern,n_generic,n_uniform', [(CHAIN, 2, 2), (FP32, 2, 0)])
def test_no_wait_for_store_acknowledgements_behind_a_buildings_stores(units, pattern, n_generic, n_uniform):
    """(a) nothing between wave 0's first building's stores and its second building's arithmetic, (b) nothing between a wave's last store and
    the LDS writes of its partial sums / the barrier -- in the generic and in the uniform body."""
    ins, _ = _kernel(units, pattern)
    generic, uniform = bodies(ins)
    assert (len(generic), len(uniform)) == (n_generic, n_uniform), (generic, uniform)
    assert all(sum(_is_plane_store(x) for x in ins[a:b + 1]) == 5 for a, b in generic + uniform)
    hits = waits_behind_bursts(ins)
    assert hits == [None] * (n_generic + n_uniform), hits
    # the uniform body's bursts are straight-line: no wait inside them either
    inside = waits_inside_bursts(ins)[n_generic:]
    assert inside == [[]] * n_uniform, inside


@pytest.mark.parametrize('pattern', [CHAIN, FP32])
def test_no_full_vector_wait_between_the_barrier_and_the_district_sums(units, pattern):
    """(c) behind the reduction's first barrier a wave adds up the wave rows and stores out_env: no `vmcnt(0)` in front of that."""
    ins, _ = _kernel(units, pattern)
    for body in bodies(ins):
        if body:
            assert waits_behind_barrier(ins, body[-1][1]) == [], body


def test_register_budgets(units):
    chain, chain_meta = _kernel(units, CHAIN)
    fp32, fp32_meta = _kernel(units, FP32)
    assert chain_meta['private_seg_size'] == 0 and fp32_meta['private_seg_size'] == 0
    assert chain_meta['num_vgpr'] <= 128
    assert fp32_meta['num_vgpr'] <= 96                    # (tests/test_isa_guards.py::test_headline_lean_kernel's budget)
    assert not [x for x in chain + fp32 if x.startswith('scratch_')]
