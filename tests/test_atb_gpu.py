"""GPU tests (-m gpu) of the weight-gradient GEMMs (tests/atb_common.py) on a real MI355X: the simulator file's cases -
every body of k_atb, fp32 and bf16, at the 64-row chunk edges, three and more chunks per workgroup, the planner's launch
splits, EQD_ATB_WGS / EQD_ATB_XCD_ALIGN - against float64, every many-unit case twice from the same buffers with equal
bits, the 40-unit calls of 10 769 rows that the simulator leaves out, and the model's ride-along tails on against off.

Only this file covers what the simulator cannot: the barrier that atb_fast_bf leaves out between chunks (workgroups that
walk three and four chunks over its two LDS buffers), and the tail job's descriptor read from the kernarg segment at a
computed offset (the simulator copies it from the argument, #ifdef EQD_HOSTSIM in k_atb)."""
import pytest
import torch

from tests import atb_common as ac

pytestmark = pytest.mark.gpu
MEASURE = {}


@pytest.fixture(scope='module')
def dev():
    from equidock_public_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.unload_for_testing()
    _lib.load_library()
    assert not _lib.is_simulator()
    yield torch.device('cuda:0')
    _lib.reload_tunables()
    print('\n' + ac.report(MEASURE))


MANY = ac.many_unit_cases(gpu=True)


@pytest.mark.parametrize('group', ac.EDGE_GROUPS)
def test_atb_row_edges(dev, group, monkeypatch):
    ac.apply_env(monkeypatch, {})
    cases = ac.edge_cases((group,))
    assert cases
    for case in cases:
        ac.check_case(dev, case, measure=MEASURE)


@pytest.mark.parametrize('case', MANY, ids=[c['id'] for c in MANY])
def test_atb_many_units(dev, case, monkeypatch):
    ac.apply_env(monkeypatch, case.get('env', {}))
    ac.check_case(dev, case, measure=MEASURE, twice=True)


def test_atb_planner(dev, monkeypatch):
    ac.apply_env(monkeypatch, {})
    for case in ac.planner_cases():
        ac.check_case(dev, case, measure=MEASURE, twice=len(case['jobs']) > 1)


def test_atb_contract_errors(dev, monkeypatch):
    ac.apply_env(monkeypatch, {})
    ac.check_contract_errors(dev)


def test_atb_bodies_agree(dev, monkeypatch):
    ac.apply_env(monkeypatch, {})
    for name, base, va, vb, bits in ac.AGREE:
        ac.check_bodies_agree(dev, name, base, va, vb, bits)


@pytest.mark.parametrize('name', list(ac.TAIL_CONFIGS))
def test_atb_tails_on_against_off(dev, name, monkeypatch):
    """the linear job riding in k_atb reads its descriptor from the kernarg segment behind the 128 units and the
    partial pointer: a wrong offset shows as a d h[0] - and so an embedding gradient - that differs from the separate
    k_linear launch's"""
    ac.check_tails(dev, monkeypatch, name)
