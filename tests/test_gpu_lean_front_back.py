"""The front and the back of a wave of the plain float64-chain step launch's uniform body (csrc/cl_kernels.hip): its plane addresses, and the
one-sum-per-thread reducer of a sixteen-wave workgroup (district_reduce, STRIPS: address in front of the barrier, seventeen LDS rows read back to back,
the adds in the loop's order).  Neither may change a bit: held to (a) the same launch with the old mapping of the extra building forced
(`cl_tuning.lean_variant` bit 32: no strip row, two-tile waves) and (b) the general `cl_step_kernel` (bit 1) -- every state plane, net, reward and the four
`out_env` rows after each of six consecutive steps enqueued without a host synchronisation in between (snapshots are device-side copies; the comparison
comes after the last step).  GPU only.

Cases (all under the chain, `tuning vec=4`): 17 buildings x 256 envs (one tile of sixteen waves: the straight-line reducer with the strip row), x 1 000
(a ragged last tile: threads of the reducer whose env lies beyond the batch), x 64 (strips 1 - 3 dead, 48 lanes of every wave outside the batch), x 1 000
with per-block episode windows, x 1 000 with a padded row pitch (out_env's rows stay n_env apart, the planes' do not); 16 and 18 buildings (sixteen waves,
no strip row); 9 buildings at `nw = 8` (strips, the reducer's loop: eight waves); a 17th building without a battery and a strided action tensor (both: the
generic body and the reducer's loop); and the first step (t = 0 is step one of every case) with and without `CLD_REF_T0_QUIRK`."""
import pytest
import torch

from golden_util import golden
from uniform_util import tables_2022, tables_last_without_battery
from citylearn_amd import abi
from citylearn_amd.engine import StepEngine
from citylearn_amd.synthetic import tile_district

pytestmark = pytest.mark.gpu

STEPS = 6
NAME = 'cl_step_lean_chain_kernel<4, true>'
OLD_MAPPING = 32            # cl_tuning.lean_variant: wave 0 takes the extra building as a second tile
GENERAL = 1                 # ... the general step kernel


def _tables_18():
    return tile_district(golden('g2022_all').spec(), 18, jitter=0.0).episode_tables(0)


# tables, envs, cl_tuning fields, StepEngine arguments, whether the district gets the uniform hint
CASES = {
    'b17_e256': (lambda: tables_2022(17), 256, {}, {}, True),
    'b17_e1000_ragged': (lambda: tables_2022(17), 1000, {}, {}, True),
    'b17_e64': (lambda: tables_2022(17), 64, {}, {}, True),
    'b17_e1000_windows': (lambda: tables_2022(17), 1000, {}, dict(n_steps=40, env_row0=[0, 37, 500, 680]), True),
    'b17_e1000_pitch': (lambda: tables_2022(17), 1000, {}, dict(env_pitch=1000 + 256), True),
    'b16_e256': (lambda: tables_2022(16), 256, {}, {}, True),
    'b18_e256': (_tables_18, 256, {}, {}, True),
    'b9_nw8_e1000': (lambda: tables_2022(9), 1000, dict(nw=8), {}, True),
    'het17_e256': (tables_last_without_battery, 256, {}, {}, False),
    'b17_e256_no_t0_quirk': (lambda: tables_2022(17), 256, {}, dict(t0_quirk=False), True),
}


def _snapshot(e):
    return e.state.clone(), e.out_bldg[:2].clone(), e.out_env.clone()


def _run(engines, actions):
    """Six steps of every engine from t = 0, back to back on the stream; [engine][step] snapshots, compared by the caller afterwards."""
    snaps = [[] for _ in engines]
    for t in range(STEPS):
        for k, e in enumerate(engines):
            e.step(actions[k][t], t)
            snaps[k].append(_snapshot(e))
    return snaps


def _same(snaps):
    for other in snaps[1:]:
        for t, (got, ref) in enumerate(zip(snaps[0], other)):
            for plane, (x, y) in zip(('state', 'net / reward', 'out_env'), zip(got, ref)):
                assert torch.equal(x, y), (plane, t)


@pytest.mark.parametrize('case', list(CASES))
def test_same_bits_as_the_old_mapping_and_the_general_kernel(case):
    tables, E, tun, kwargs, uniform = CASES[case]
    tab = tables()
    if 'env_row0' in kwargs:
        kwargs = dict(kwargs, env_row0=kwargs['env_row0'][:-(-E // abi.CL_ROW0_BLOCK)])
    engines = [StepEngine(tab, E, f64_maps='chain', tuning=dict(vec=4, lean_variant=v, **tun), **kwargs) for v in (0, OLD_MAPPING, GENERAL)]
    assert all(bool(e.dims.flags & abi.CLD_LEAN_UNIFORM) == uniform for e in engines)
    assert all(bool(e.dims.flags & abi.CLD_REF_T0_QUIRK) == kwargs.get('t0_quirk', True) for e in engines)
    for e in engines:
        e.trace_kernels()
    gen = torch.Generator(device='cuda').manual_seed(23)
    acts = [torch.rand((engines[0].n_act_cols, E), device='cuda', generator=gen) * 2 - 1 for _ in range(STEPS)]
    snaps = _run(engines, [acts] * 3)
    _same(snaps)
    assert engines[0].last_kernels == NAME and engines[1].last_kernels == NAME, (engines[0].last_kernels, engines[1].last_kernels)
    assert engines[2].last_kernels.startswith('cl_step_kernel<4, false, false, false, 2'), engines[2].last_kernels
    soc = [s[0][abi.CLS_B_SOC] for s in snaps[0]]
    assert bool((soc[-1] != soc[0]).any())                           # (the batteries moved)
    if 'env_pitch' in kwargs:
        assert engines[0].dims.env_pitch == kwargs['env_pitch'] != E


def test_strided_actions_keep_the_generic_body():
    """`[n_env, n_cols].T`: the entry test takes the generic body, whose district sums go through the reducer's loop -- same bits with and without the
    off switch, as the general kernel on the same view, and as the uniform body with the straight-line reducer on a contiguous copy."""
    E = 256
    engines = [StepEngine(tables_2022(17), E, f64_maps='chain', tuning=dict(vec=4, lean_variant=v)) for v in (0, OLD_MAPPING, GENERAL, 0)]
    for e in engines:
        e.trace_kernels()
    gen = torch.Generator(device='cuda').manual_seed(29)
    strided = [(torch.rand((E, engines[0].n_act_cols), device='cuda', generator=gen) * 2 - 1).T for _ in range(STEPS)]
    assert strided[0].stride(1) != 1
    packed = [a.contiguous() for a in strided]
    _same(_run(engines, [strided, strided, strided, packed]))
    assert engines[0].last_kernels == NAME and engines[3].last_kernels == NAME
