"""The single-step path of a THERMAL district under a power outage (`StepEngine.step` on tests/policy_full_util.py's nine-building outage
district: battery, cooling tank and DHW tank in one building, no LSTM stage) against the C oracle -- what the closed-loop policy rollout tests
(tests/test_gpu_policy_full_rollout.py, tests/test_gpu_policy_full_kpi_rollout.py) replay through.  Before this module the only GPU outage
coverage was on the 2023 buildings (battery + DHW tank): `cl_step_full_kernel`'s outage unit had never stepped a cooling tank.  The oracle
itself is pinned on this district by tests/test_policy_full_host.py::test_c_and_python_oracles_agree_under_a_thermal_outage.  GPU only."""
import numpy as np
import pytest
import torch

from golden_util import check_worst
from citylearn_amd import abi
from citylearn_amd.engine import StepEngine
from policy_full_util import outage_mask, thermal_district
from test_gpu_config_sizes import _kpi_step_waves
from test_gpu_parity import _err, _teach

pytestmark = pytest.mark.gpu

KINDS = ['RewardFunction', 'MARL', 'IndependentSACReward', 'SolarPenaltyReward']
OUTAGE = [abi.CLK_UNSERVED_OUTAGE, abi.CLK_EXPECTED_OUTAGE]
K = 48


@pytest.mark.parametrize('kpi', [False, True])
@pytest.mark.parametrize('f64', ['chain', False])
@pytest.mark.parametrize('E', [64, 260])
@pytest.mark.parametrize('kind', KINDS)
def test_single_steps_under_a_thermal_outage_against_the_c_oracle(kind, E, f64, kpi):
    """Steps 0 .. 47, every env its own actions (a column of zeros, one at the lower and one at the upper bounds), each step teacher-forced from
    the oracle's state (tests/test_gpu_config_sizes.py::test_config_sizes_with_distinct_actions_against_the_c_oracle's pattern): every state
    plane, net, reward and the four district sums at the plain bar; net exactly 0 on the outage (row, building) pairs and only there.
    `kpi=True`: the same through the launch that keeps the streaming KPIs -- on the fp32 map both routes (`cl_step_full_kpi_kernel`, and the
    step with the `CLD_DETAIL_MIN` planes + `cl_kpi_kernel`) with bit-equal outage sums, under the float64 chain the second one; the two outage
    sums move for some env of every building with outage rows, stay at their reset value for buildings 2, 5 and 8, and unserved <= expected.
    Their VALUES against a sum of the oracle's own quantities, independent of every kernel: oracle/oracle.py (equal to the C oracle bit for bit
    from reset, asserted here on net) steps envs 0 .. 2 -- no action, every storage at its lower and at its upper bound -- and on the outage
    (row, building) pairs its demands (cooling + heating + DHW + non-shiftable load: expected) and what devices, discharging storages and the
    load actually got (served) are added up in float64, the reference's unserved-energy terms (building.py `unserved_energy`).  Expected energy
    at the plain bar; unserved = sum(expected - served) cancels, so its bar is the plain one on the two sums it is the difference of:
    1e-4 + 1e-4 (sum expected + sum served)."""
    from oracle.c_oracle import COracle, OS, OO
    from oracle.oracle import DistrictOracle
    spec = thermal_district('g2020_cz1_outage')
    tab = spec.episode_tables(0)
    m = outage_mask(tab, K)
    engines = [StepEngine(tab, E, reward=kind, f64_maps=f64, kpi=kpi)]
    if kpi and not f64:
        engines.append(StepEngine(tab, E, reward=kind, f64_maps=f64, kpi=True, tuning=dict(kpi_passes=1, nw=_kpi_step_waves(E, 9))))
    for eng in engines:
        assert not eng.lean and eng.n_bldg == 9 and eng.f64_chain == (f64 == 'chain')
        eng.trace_kernels()
    reset_outage = engines[0].kpi_bldg[OUTAGE].clone() if kpi else None
    ora = COracle(spec, tab, E, reward=kind)
    NP = 3
    po, want, served = (DistrictOracle(spec, tab, NP, reward=kind), np.zeros((2, 9, NP)), np.zeros((9, NP))) if kpi else (None, None, None)
    if kpi:
        po.reset()
    low, high = spec.action_limits()
    rng = np.random.RandomState(E + len(kind))
    planes = ((abi.CLS_B_SOC, 'SOC'), (abi.CLS_B_EFF, 'EFF'), (abi.CLS_B_DEGCAP, 'DEGCAP'), (abi.CLS_CS_SOC, 'CS'), (abi.CLS_HS_SOC, 'HS'), (abi.CLS_DS_SOC, 'DS'))
    worst = {}
    for t in range(K):
        a = rng.uniform(low[:, None], high[:, None], size=(len(low), E)).astype(np.float32)
        a[:, 0] = 0.0
        a[:, 1], a[:, 2] = low, high
        for eng in engines:
            _teach(eng, ora, OS)
            eng.step(torch.from_numpy(a).cuda(), t)
        out, oe = ora.step(a, t)
        for eng in engines:
            got_state = {pl: (eng.degraded_capacity if pl == abi.CLS_B_DEGCAP else eng.state[pl]).cpu().numpy() for pl, _ in planes}
            checks = [(key.lower(), got_state[pl], ora.state[:, :, OS[key]].T) for pl, key in planes]
            checks += [('net', eng.net.cpu().numpy(), out[:, :, OO['NET']].T), ('reward', eng.reward_bldg.cpu().numpy(), out[:, :, OO['REWARD']].T),
                       ('d_net', eng.district_net.cpu().numpy(), oe[:, 0]), ('d_cost', eng.out_env[abi.CLQ_COST].cpu().numpy(), oe[:, 1]),
                       ('d_emission', eng.out_env[abi.CLQ_EMISSION].cpu().numpy(), oe[:, 2]), ('d_reward', eng.district_reward.cpu().numpy(), oe[:, 3])]
            for key, got, ref in checks:
                worst[key] = max(worst.get(key, 0.0), _err(got, ref, 1e-4, 1e-4))
            zero = (eng.net == 0).cpu().numpy()
            assert np.array_equal(zero, np.broadcast_to(m[t][:, None], zero.shape)), t
        assert not out[:, m[t], OO['NET']].any()
        if kpi:
            assert np.array_equal(po.step(a[:, :NP])['net'], out[:NP, :, OO['NET']].T.astype(np.float32)), t
            for e, env in enumerate(po.units):
                for b in np.nonzero(m[t])[0]:
                    u = env[b]
                    ex = float(u.cool_dem) + float(u.heat_dem) + float(u.dhw_dem[t]) + float(u.nsl[t])
                    sv = float(u.e_cool_dev) + float(u.e_heat_dev) + float(u.e_dhw_dev) + float(u.e_ns) \
                        + sum(max(-float(k.eb), 0.0) for k in (u.cs, u.hs, u.ds))
                    want[0, b, e] += ex - sv
                    want[1, b, e] += ex
                    served[b, e] += sv
    names = [eng.last_kernels for eng in engines]
    print(kind, E, f64, kpi, names, {k: round(v, 4) for k, v in worst.items()})
    if not kpi:
        assert names[0].startswith('cl_step_full_chain_kernel<' if f64 == 'chain' else 'cl_step_full_kernel<') and '+' not in names[0], names
    elif f64 == 'chain':
        assert names[0].startswith('cl_step_full_chain_kernel<') and names[0].endswith('+cl_kpi_kernel'), names
    else:
        assert names[0].startswith('cl_step_full_kpi_kernel<') and '+' not in names[0], names
        assert names[1].startswith('cl_step_full_kernel<') and names[1].endswith('+cl_kpi_kernel'), names
    if kpi:
        has = torch.as_tensor(m.any(axis=0), device='cuda')
        assert has.tolist() == [i % 3 != 2 for i in range(9)]
        for eng in engines:
            un, ex = eng.kpi_bldg[abi.CLK_UNSERVED_OUTAGE], eng.kpi_bldg[abi.CLK_EXPECTED_OUTAGE]
            assert torch.equal(eng.kpi_bldg[OUTAGE][:, ~has], reset_outage[:, ~has])
            assert bool((ex[has] > 0).all()) and bool((un[has] > 0).any(dim=1).all())
            assert bool((un >= 0).all()) and bool((un <= ex).all())
            assert bool((eng.kpi_bldg[abi.CLK_UNSERVED_ALL] <= eng.kpi_bldg[abi.CLK_EXPECTED_ALL]).all())
            got = (eng.kpi_bldg[OUTAGE].double() - reset_outage.double())[:, :, :NP].cpu().numpy()
            worst['kpi_expected_outage'] = max(worst.get('kpi_expected_outage', 0.0), _err(got[1], want[1], 1e-4, 1e-4))
            worst['kpi_unserved_outage'] = max(worst.get('kpi_unserved_outage', 0.0),
                                               float((np.abs(got[0] - want[0]) / (1e-4 + 1e-4 * (want[1] + served))).max()))
            print('outage sums against the oracle:', {k: round(worst[k], 4) for k in ('kpi_expected_outage', 'kpi_unserved_outage')},
                  'largest unserved', round(float(want[0].max()), 3), 'of expected', round(float(want[1].max()), 3))
            assert want[0].max() > 1.0 and np.all(want[1][m.any(axis=0)] > 1.0)
        if len(engines) == 2:
            assert torch.equal(engines[0].kpi_bldg[OUTAGE], engines[1].kpi_bldg[OUTAGE])
            assert torch.equal(engines[0].state, engines[1].state) and torch.equal(engines[0].out_bldg[:2], engines[1].out_bldg[:2])
    check_worst(worst, f'thermal outage single steps {kind} E={E} f64_maps={f64} kpi={kpi}')
