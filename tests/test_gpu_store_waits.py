"""The lean step kernels after their plane loads, buildings and stores became one region per wave (csrc/cl_kernels.hip, STORE ACKNOWLEDGEMENTS:
no wave waits for the acknowledgement of its own stores any more) against a twin engine forced onto the general `cl_step_kernel`, the reference
of tests/test_gpu_parity.py::test_lean_kernel_variants_are_bit_identical: equal BITS on every state plane, net, reward and district sum.  GPU only.

Six consecutive steps from t = 0 (the first one books the load three times), enqueued without a host synchronisation in between: the outputs of
every step are cloned on the device and compared at the end.  Geometry forced through `tuning` as in tests/test_gpu_lean_uniform.py.

Shapes: 17 buildings (wave 0 owns two), 16 (no wave owns two), 3, 1 (one wave); 256 envs and 1 000 (a ragged last env tile at one, two and four
envs per lane: dead lanes and, at four, a workgroup with dead WAVES' worth of lanes); the float64 chain (uniform body), the fp32 map and the
float64 maps (generic body).  het17 (tests/district_util.py) puts a battery-less building first in its wave and an undriven one second: the
generic body's no-battery path and the action columns that are parameter words."""
from functools import lru_cache

import pytest
import torch

from district_util import district
from uniform_util import tables_2022
from citylearn_amd import abi
from citylearn_amd.engine import StepEngine

pytestmark = pytest.mark.gpu

STEPS = 6
PRECISIONS = {'chain': 'chain', 'fp32': False, 'f64': True}
LEAN_KERNEL = {'chain': 'cl_step_lean_chain_kernel<', 'fp32': 'cl_step_lean_kernel<', 'f64': 'cl_step_lean_f64_kernel<'}
REWARDS = ('RewardFunction', 'MARL', 'IndependentSACReward', 'SolarPenaltyReward')


@lru_cache(maxsize=None)
def _tables(name):
    return tables_2022(3) if name == 'b3' else district(name).episode_tables(0)


def _bits(x):
    return x.contiguous().view(torch.int32)


def _check(tab, E, vec, prec, reward='RewardFunction', strided=False, seed=0, **kwargs):
    """Lean launch (`lean_variant` 2) and general kernel (1) side by side for STEPS steps; returns the lean engine."""
    lean, general = (StepEngine(tab, E, reward=reward, f64_maps=PRECISIONS[prec], tuning=dict(vec=vec, lean_variant=v), **kwargs) for v in (2, 1))
    lean.trace_kernels()
    general.trace_kernels()
    gen = torch.Generator(device='cuda').manual_seed(seed)
    snaps = []
    for t in range(STEPS):
        if strided:
            a = (torch.rand((E, lean.n_act_cols), device='cuda', generator=gen) * 2 - 1).T
            assert a.stride(1) != 1
        else:
            a = torch.rand((lean.n_act_cols, E), device='cuda', generator=gen) * 2 - 1
        lean.step(a, t)
        general.step(a, t)
        snaps.append([(e.state.clone(), e.out_bldg[:2].clone(), e.out_env.clone()) for e in (lean, general)])
    for t, (got, ref) in enumerate(snaps):
        for what, g, r in zip(('state', 'net / reward', 'district sums'), got, ref):
            assert torch.equal(_bits(g), _bits(r)), (t, what, E, vec, prec, reward)
    assert LEAN_KERNEL[prec] in lean.last_kernels and 'cl_step_kernel<' in general.last_kernels, (lean.last_kernels, general.last_kernels)
    if prec != 'f64':                                     # (the float64 maps run at one or two envs per lane)
        assert f'<{vec},' in lean.last_kernels, lean.last_kernels
    assert bool((lean.soc != 0).any()) or lean.n_bldg == 1
    return lean


@pytest.mark.parametrize('prec', list(PRECISIONS))
@pytest.mark.parametrize('name', ['g2022_all', 'b16', 'b3', 'b1'])
def test_lean_launch_equals_the_general_kernel_bit_for_bit(name, prec):
    for E in (256, 1000):
        for vec in (1, 2, 4):
            lean = _check(_tables(name), E, vec, prec, seed=100 * E + vec)
            if prec == 'chain':
                assert lean.dims.flags & abi.CLD_LEAN_UNIFORM          # the uniform body


@pytest.mark.parametrize('prec', list(PRECISIONS))
@pytest.mark.parametrize('reward', REWARDS)
def test_reward_kinds(reward, prec):
    """MARL takes district_reduce's coupled path: a thread re-reads the nets it stored itself, behind the barrier that no longer waits for them."""
    for E, vec in ((1000, 4), (256, 1)):
        _check(_tables('g2022_all'), E, vec, prec, reward=reward, seed=7)


@pytest.mark.parametrize('prec', list(PRECISIONS))
def test_strided_actions_take_the_generic_body_with_the_hint_set(prec):
    for vec in (1, 4):
        lean = _check(_tables('g2022_all'), 1000, vec, prec, strided=True, seed=11)
        assert lean.dims.flags & abi.CLD_LEAN_UNIFORM


@pytest.mark.parametrize('prec', list(PRECISIONS))
def test_episode_windows(prec):
    E = 1000
    row0 = [0, 37, 500, 680][:-(-E // abi.CL_ROW0_BLOCK)]
    for vec in (1, 4):
        lean = _check(_tables('g2022_all'), E, vec, prec, seed=13, n_steps=40, env_row0=row0)
        assert not torch.equal(lean.net[:, :abi.CL_ROW0_BLOCK], lean.net[:, abi.CL_ROW0_BLOCK:2 * abi.CL_ROW0_BLOCK])      # (the windows differ)


@pytest.mark.parametrize('prec', list(PRECISIONS))
@pytest.mark.parametrize('reward', ['RewardFunction', 'SolarPenaltyReward'])
def test_heterogeneous_district(reward, prec):
    """No battery on a wave's first building, an undriven battery on a second one: action columns that are not the building index."""
    for E, vec, nw in ((1000, 4, 9), (256, 2, 9), (1000, 1, 0)):
        tab = _tables('het17')
        lean, general = (StepEngine(tab, E, reward=reward, f64_maps=PRECISIONS[prec], tuning=dict(vec=vec, nw=nw, lean_variant=v)) for v in (2, 1))
        assert not lean.dims.flags & abi.CLD_LEAN_UNIFORM and not lean.dims.flags & abi.CLD_ES_COL_IS_BLDG
        lean.trace_kernels()
        gen = torch.Generator(device='cuda').manual_seed(17)
        snaps = []
        for t in range(STEPS):
            a = torch.rand((lean.n_act_cols, E), device='cuda', generator=gen) * 2 - 1
            lean.step(a, t)
            general.step(a, t)
            snaps.append([(e.state.clone(), e.out_bldg[:2].clone(), e.out_env.clone()) for e in (lean, general)])
        for t, (got, ref) in enumerate(snaps):
            for g, r in zip(got, ref):
                assert torch.equal(_bits(g), _bits(r)), (t, E, vec, prec, reward)
        assert LEAN_KERNEL[prec] in lean.last_kernels, lean.last_kernels
