"""One-off: the four central-agent policy classes of this tree (`policy._CentralBase`) against the policy.py of the tree before them, bit for bit:
every tensor and array of `pack`, `_full`, `actions_host` in every calling form, `torch_policy` on the CPU in float32 and float64, and `update`, on the
districts of the four central host tests, two parameter sets with and without `set_of_block`, sigma None / scalar / per column, (H1, H2) = (4, 64) and
(24, 40).  No GPU.

    python scripts/policy_central_base_compare.py <parent-tree>          (from the repository root; the parent as a `git worktree`)"""
import importlib.util
import itertools
import sys
from pathlib import Path
import numpy as np
import torch
sys.path[:0] = [str(Path.cwd()), str(Path.cwd() / 'tests')]
from citylearn_amd import policy as new
spec_ = importlib.util.spec_from_file_location('citylearn_amd.policy_parent', Path(sys.argv[1]) / 'citylearn_amd' / 'policy.py')
old = importlib.util.module_from_spec(spec_)
sys.modules[spec_.name] = old
spec_.loader.exec_module(old)
assert old.__file__ != new.__file__ and not hasattr(old, '_CentralBase') and hasattr(new, '_CentralBase')
from district_util import district
from policy_full_util import thermal_district
from policy_central_util import central_layout

def same(a, b, path):
    if isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b) and a.is_contiguous() == b.is_contiguous(), path
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b), path
    else:
        assert type(a) is type(b) and a == b, (path, a, b)
    return 1

n_cmp = n_case = 0
rng = np.random.RandomState(0)
for thermal, names in ((False, ('g2022_all', 'het17')), (True, ('g2020_cz1', 't2', 't2_outage'))):
    for name, normalize in itertools.product(names, (True, False)):
        sp = thermal_district(name) if thermal else district(name)
        tab = sp.episode_tables(0)
        layout = central_layout(sp, normalize)
        B, N = len(sp.buildings), layout.n_cols
        hs = (4,) if thermal else ()
        n_act = len(layout.spec.action_limits()[0])
        for deep, (H1, H2), sig in itertools.product((False, True), ((4, 64), (24, 40)), ('none', 'scalar', 'column')):
            u = lambda a, *shape: rng.uniform(-a, a, shape)
            w = [u(0.2, 2, H1, N), u(0.5, 2, H1)]
            if deep:
                w += [u(0.3, 1, H2, H1), u(0.5, 2, H2)]              # (a leading 1 broadcasts)
            HO = H2 if deep else H1
            w += [u(0.3, 2, B, *hs, HO), u(0.4, 1, B, *hs)]
            sigma = {'none': None, 'scalar': 0.1, 'column': np.linspace(0.0, 0.3, n_act)}[sig]
            cls = ('Deep' if deep else '') + ('CentralStorageMLPPolicy' if thermal else 'CentralMLPPolicy')
            po, pn = getattr(old, cls)(*w, sigma=sigma), getattr(new, cls)(*w, sigma=sigma)
            for sob in (None, [1, 0]):
                to, tn = po.pack(layout, tab, set_of_block=sob), pn.pack(layout, tab, set_of_block=sob)
                assert type(to).__name__ == type(tn).__name__ and sorted(vars(to)) == sorted(vars(tn)), cls
                n_cmp += sum(same(vars(to)[k], vars(tn)[k], (cls, name, k)) for k in vars(to))
            for a, b in zip(po._full(B), pn._full(B)):
                n_cmp += same(np.array(a), np.array(b), (cls, '_full'))
            E = 5
            x = rng.uniform(-1, 2, (E, N))
            z = rng.standard_normal((E, B) + hs)
            for s in (0, 1):
                if thermal:
                    calls = [dict(noise=None), dict(noise=z)]
                    ao, an = [po.actions_host(x, to, set_index=s, **kw) for kw in calls], [pn.actions_host(x, tn, set_index=s, **kw) for kw in calls]
                else:
                    calls = [dict(), dict(tables=to), dict(noise=z, tables=to), dict(noise=z, low=to.low_bldg, high=to.high_bldg, sigma_bldg=to.sigma_bldg)]
                    if sig != 'column':
                        calls.append(dict(noise=z))
                    ao, an = [po.actions_host(x, set_index=s, **kw) for kw in calls], [pn.actions_host(x, set_index=s, **kw) for kw in calls]
                for a, b in zip(ao, an):
                    n_cmp += same(a, b, (cls, name, 'actions_host'))
                for dt in (torch.float32, torch.float64):
                    xo = torch.from_numpy(x).to(dt)
                    fo, fn = po.torch_policy(layout, tab, 'cpu', dtype=dt, set_index=s), pn.torch_policy(layout, tab, 'cpu', dtype=dt, set_index=s)
                    n_cmp += same(fo(xo), fn(xo), (cls, name, 'torch_policy', dt))
            # the learner's step
            for p in (po, pn):
                p.update(w1=-p.w1, sigma=0.05)
            assert po.version == pn.version == 1
            n_cmp += same(po.actions_host(x, to) if thermal else po.actions_host(x), pn.actions_host(x, tn) if thermal else pn.actions_host(x), (cls, 'update'))
            n_case += 1
print(f'{n_case} cases, {n_cmp} comparisons: every one bit-equal')
