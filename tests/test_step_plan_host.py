"""The step path's kernel selection on the CPU: csrc/cl_plan.h (`plan_step` + `plan_name`) compiled with g++ (tests/host_shim, a test
harness -- the library launches the plan on the GPU).  The kernel names pinned here are the ones the GPU tests read back from
`cl_tuning.kernel_name` after a real launch (tests/test_gpu_config_sizes.py test_kernel_selection_map / test_kernel_selection_by_batch_size,
tests/test_gpu_parity.py CHAIN_CASES, tests/test_gpu_observe.py), so a rule change shows up here without a GPU."""
import ctypes
import json
import subprocess
from pathlib import Path

import pytest

from citylearn_amd import abi
from citylearn_amd._lib import Dims, Tuning

HERE = Path(__file__).resolve().parent


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    out = tmp_path_factory.mktemp('plan') / 'libstep_plan_host.so'
    subprocess.run(['g++', '-std=c++17', '-O1', '-shared', '-fPIC', '-Wall', '-Werror', str(HERE / 'host_shim' / 'step_plan_host.cpp'), '-o', str(out)],
                   check=True)
    lib = ctypes.CDLL(str(out))
    lib.host_plan_step.argtypes = [ctypes.POINTER(Dims), ctypes.POINTER(Tuning), ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_longlong)]
    lib.host_plan_step.restype = ctypes.c_int

    def run(B, E, flags=0, tuning=None, flex=False, obs=False, obs_lean_ok=False, obs_pitch=0, act_stride_env=1):
        """(rc, kernel_name, cl_last_error, geometry) of one step call on a B-building x E-env district."""
        dims = Dims(E, B, 24, B, flags, 0, None, None, 0, 0, 0)
        tun = Tuning(**(tuning or {}))
        name, err, geom = ctypes.create_string_buffer(abi.CL_KERNEL_NAME_LEN), ctypes.create_string_buffer(512), (ctypes.c_longlong * 8)()
        rc = lib.host_plan_step(ctypes.byref(dims), ctypes.byref(tun), act_stride_env, int(flex), int(obs), int(obs_lean_ok), obs_pitch, name, err, geom)
        return rc, name.value.decode(), err.value.decode(), list(geom)
    return run


def _flags(lean, precision='chain', detail=False, kpi=False, reward=abi.CLR_DEFAULT, check=False):
    f = reward << abi.CLD_REWARD_SHIFT
    f |= abi.CLD_LEAN if lean else 0
    f |= {'chain': abi.CLD_F64_CHAIN, 'f64': abi.CLD_F64_MAPS, 'fp32': 0}[precision]
    f |= abi.CLD_WRITE_DETAIL if detail else 0
    f |= abi.CLD_KPI if kpi else 0
    f |= abi.CLD_CHECK if check else 0
    return f


def _selection_map():
    return json.loads((HERE / 'golden' / 'kernel_selection_r06.json').read_text())


@pytest.mark.parametrize('cell', _selection_map(), ids=lambda c: f"{c['kind']}-{c['B']}x{c['E']}")
def test_selection_map(plan, cell):
    """Every cell of the map test_kernel_selection_map pins on the GPU (the default precision model, RewardFunction, finish = 3 above 32 buildings)."""
    B, E = cell['B'], cell['E']
    rc, name, err, _ = plan(B, E, _flags(cell['kind'] == 'lean'), tuning={'finish': 3} if B > 32 else None)
    assert rc == abi.CL_OK, err
    assert name == cell['kernel'], (cell, name)


@pytest.mark.parametrize('E,expect', [(16384, 'cl_step_lean_kernel<1, '), (32768, 'cl_step_lean_kernel<2, '), (65536, 'cl_step_lean_kernel<4, '),
                                       (98304, 'cl_step_lean_kernel<4, '), (122880, 'cl_step_lean_kernel<4, '), (122884, 'cl_step_envmajor_kernel<17, '),
                                       (196608, 'cl_step_envmajor_kernel<17, '), (196612, 'cl_step_envmajor_kernel<17, '), (262144, 'cl_step_envmajor_kernel<17, '),
                                       (524288, 'cl_step_lean_kernel<4, false, true>'), (1048576, 'cl_step_lean_kernel<4, ')])
@pytest.mark.parametrize('precision', ['chain', 'fp32'])
def test_selection_by_batch_size(plan, E, expect, precision):
    """The 17-building battery + PV district (test_kernel_selection_by_batch_size), and its reference launch through the general kernel."""
    if precision == 'chain':
        if E in (122884, 196608):
            expect = 'cl_step_lean_kernel<4, '
        expect = expect.replace('cl_step_lean_kernel<4, false, true>', 'cl_step_lean_kernel<4, true>').replace('cl_step_lean_kernel<', 'cl_step_lean_chain_kernel<')
    rc, name, err, _ = plan(17, E, _flags(True, precision))
    assert rc == abi.CL_OK and name.startswith(expect), (name, err)
    rc, name, err, _ = plan(17, E, _flags(True, precision), tuning=dict(lean_variant=1, envmajor=2))
    assert rc == abi.CL_OK and name.startswith('cl_step_kernel<'), (name, err)


@pytest.mark.parametrize('lean,B,vec,tuning,detail,kernel', [
    (True, 17, 1, None, False, 'cl_step_lean_chain_kernel<1'), (True, 17, 2, None, False, 'cl_step_lean_chain_kernel<2'),
    (True, 17, 4, None, False, 'cl_step_lean_chain_kernel<4'), (True, 17, 0, dict(envmajor=1), False, 'cl_step_envmajor_kernel<17, true, 1, 2>'),
    (True, 17, 2, dict(lean_variant=1), False, 'cl_step_kernel<2, false, false, false, 2, false>'),
    (False, 9, 0, None, False, 'cl_step_full_chain_kernel<1, false, 1024, 4, false'), (False, 9, 0, dict(full_variant=5), False, 'cl_step_full_tp_chain_kernel<1, 4'),
    (False, 9, 1, dict(full_variant=1), False, 'cl_step_kernel<1, true, false, false, 2, false>'), (False, 9, 0, None, True, 'cl_step_full_chain_kernel<1, true')])
def test_chain_kernels(plan, lean, B, vec, tuning, detail, kernel):
    """CLD_F64_CHAIN at 64 envs (tests/test_gpu_parity.py CHAIN_CASES)."""
    rc, name, err, _ = plan(B, 64, _flags(lean, 'chain', detail=detail), tuning=dict(vec=vec, **(tuning or {})))
    assert rc == abi.CL_OK and kernel in name, (name, err)


@pytest.mark.parametrize('lean,B,E,kernel', [(True, 17, 65536, 'cl_step_lean_kernel<4'), (False, 9, 65536, 'cl_step_full_tp_kernel'),
                                             (True, 17, 262144, 'cl_step_envmajor_kernel')])
def test_fp32_and_f64_kernels(plan, lean, B, E, kernel):
    """The fp32 map (tests/test_gpu_config_sizes.py) and CLD_F64_MAPS: the lean float64 kernel or PREC = 1 of the general kernel."""
    rc, name, err, _ = plan(B, E, _flags(lean, 'fp32'))
    assert rc == abi.CL_OK and kernel in name, (name, err)
    rc, name, err, _ = plan(B, E, _flags(lean, 'f64'))
    assert rc == abi.CL_OK and ('cl_step_lean_f64_kernel' in name or ', 1, false>' in name), (name, err)


@pytest.mark.parametrize('precision', ['chain', 'fp32'])
@pytest.mark.parametrize('B,E,tuning,kernel', [(9, 65536, None, 'cl_step_full_tp_obs_kernel<'), (9, 4996, dict(full_variant=5), 'cl_step_full_tp_obs_kernel<'),
                                               (9, 772, None, 'cl_step_full_obs_kernel<')])
def test_fused_observation(plan, B, E, tuning, kernel, precision):
    """cl_step_observe_f32: the thermal kernels write the compact observation themselves in one launch (tests/test_gpu_observe.py), the lean
    kernels likewise where the battery + PV launch can fill it."""
    rc, name, err, _ = plan(B, E, _flags(False, precision), tuning=tuning, obs=True, obs_pitch=32)
    assert rc == abi.CL_OK and name.startswith(kernel) and '+' not in name, (name, err)
    rc, name, err, _ = plan(17, 65536, _flags(True, precision), obs=True, obs_lean_ok=True, obs_pitch=32)
    assert rc == abi.CL_OK and name == {'chain': 'cl_step_lean_obs_chain_kernel<4, true>', 'fp32': 'cl_step_lean_obs_kernel<4, true>'}[precision], (name, err)


@pytest.mark.parametrize('E,tuning,kernel', [(65536, None, 'cl_step_lean_kpi_kernel<4, true>'), (516, None, 'cl_step_lean_kpi_kernel<1, true>'),
                                             (132, dict(vec=4, lean_variant=2), 'cl_step_lean_kpi_kernel<4, true>')])
def test_streaming_kpis_in_the_lean_step(plan, E, tuning, kernel):
    """CLD_KPI without the detail planes (tests/test_gpu_config_sizes.py test_kpi_accumulators_updated_by_the_lean_step_kernel): one launch."""
    rc, name, err, _ = plan(17, E, _flags(True, 'fp32', kpi=True), tuning=tuning)
    assert rc == abi.CL_OK and name == kernel, (name, err)


def test_check_names_the_launched_instantiation(plan):
    """CLD_CHECK launches cl_step_kernel<1, true, true, FLEX, PREC, false, true>: the name spells the arguments actually launched."""
    for precision, flex, prec in (('chain', False, 2), ('f64', False, 1), ('fp32', False, 0), ('fp32', True, 0)):
        rc, name, err, _ = plan(9, 1024, _flags(False, precision, detail=True, check=True), flex=flex)
        assert rc == abi.CL_OK, err
        assert name.endswith(f'cl_step_kernel<1, true, true, {"true" if flex else "false"}, {prec}, false, true>'), name


def test_follow_up_launches(plan):
    """Building-chunked districts: the second launch that folds the chunk sums unless the step defers it; MARL's reward pass; the KPI passes."""
    rc, name, _, geom = plan(1024, 8192, _flags(False, 'fp32'))
    assert rc == abi.CL_OK and name.endswith('+cl_finish_kernel') and geom[1] > 1, (name, geom)
    rc, name, _, _ = plan(1024, 8192, _flags(False, 'fp32', reward=abi.CLR_MARL))
    assert name.endswith('+cl_finish_kernel+cl_marl_reward_kernel'), name
    rc, name, _, _ = plan(9, 4096, _flags(False, 'fp32', detail=True, kpi=True), tuning=dict(kpi_passes=2))
    assert name.endswith('+cl_kpi_bldg_kernel+cl_kpi_env_kernel'), name
    rc, name, _, _ = plan(9, 4096, _flags(False, 'fp32', detail=True, kpi=True), tuning=dict(kpi_passes=1))
    assert name.endswith('+cl_kpi_kernel'), name
    rc, name, _, _ = plan(9, 65536, _flags(False, 'fp32', kpi=True))
    assert name.startswith('cl_step_full_kpi_kernel<') and '+' not in name, name
    rc, name, _, _ = plan(17, 4096, _flags(True, 'fp32'), flex=True)
    assert name.startswith('cl_flex_kernel<1, true>+cl_step_'), name


@pytest.mark.parametrize('B,E,flags,tuning,flex,message', [
    (64, 1024, _flags(False, 'fp32', detail=True, check=True), None, False, 'CLD_CHECK needs CLD_WRITE_DETAIL'),
    (17, 1024, _flags(True, 'fp32', check=True), None, False, 'CLD_CHECK needs CLD_WRITE_DETAIL'),
    (17, 65536, _flags(True, 'fp32', kpi=True), dict(nw=4), False, 'CLD_KPI without CLD_WRITE_DETAIL needs a step launch'),
    (9, 65536, _flags(False, 'chain', kpi=True), None, False, 'CLD_F64_CHAIN with CLD_KPI needs CLD_WRITE_DETAIL'),
    (64, 65536, _flags(False, 'fp32'), dict(full_variant=5), False, 'full_variant = 5'),
    (17, 4096, _flags(True, 'chain'), dict(lean_variant=4), False, 'lean_variant = 4'),
    (17, 4096, _flags(True, 'chain'), None, True, 'CLD_F64_CHAIN is not implemented for districts with flexible loads'),
    (17, 4096, _flags(True, 'f64', kpi=True), None, False, 'CLD_F64_MAPS with CLD_KPI needs CLD_WRITE_DETAIL'),
    (9, 4096, _flags(False, 'fp32'), dict(full_variant=1, vec=4), False, 'bad vec 4'),
    (64, 4096, _flags(True, 'fp32', reward=abi.CLR_EV), None, True, 'reward kind CLR_EV is not implemented for building-chunked launches')])
def test_refusals(plan, B, E, flags, tuning, flex, message):
    """Launch overrides and flag combinations that do not fit come back as CL_EINVAL with the message cl_last_error gives on the GPU."""
    rc, name, err, _ = plan(B, E, flags, tuning=tuning, flex=flex)
    assert rc == abi.CL_EINVAL and message in err, (rc, err, name)
