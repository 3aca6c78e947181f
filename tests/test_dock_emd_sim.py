"""CPU tests of the batched exact transport solver on the device: csrc_dock/ compiled for x86 against the host simulator
and driven through equidock_public_amd.dock, as on the GPU (the shared checks live in tests/dock_emd_common.py)."""
import pytest
import torch

from equidock_public_amd import dock as DK
from tests import dock_common as dc
from tests import dock_emd_common as ec

DEV = torch.device('cpu')


@pytest.fixture(scope='module', autouse=True)
def simulator():
    DK.load_dock_library_for_testing(dc.build_sim())
    assert DK._dock_is_sim
    yield
    DK.unload_dock_for_testing()


def test_abi():
    lib = DK.load_dock_library()
    assert lib.eqd_dock_emd_abi() == DK.DOCK_EMD_ABI == 1 and lib.eqd_dock_abi_version() == 1
    assert DK.EMD_MAX_NODES >= 2048


@pytest.mark.parametrize('resident', [True, False], ids=['resident', 'general'])
def test_plans_are_the_host_solvers_k50(resident):
    ec.check_against_host(DEV, 'k50', resident)


@pytest.mark.parametrize('resident', [True, False], ids=['resident', 'general'])
@pytest.mark.parametrize('K', ec.N40_COLS)
def test_plans_are_the_host_solvers_n40(K, resident):
    ec.check_against_host(DEV, f'n40_{K}', resident)


@pytest.mark.parametrize('resident', [True, False], ids=['resident', 'general'])
@pytest.mark.parametrize('size', ec.TIE_SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_ties_settle_in_the_host_solvers_order(size, resident):
    ec.check_against_host(DEV, f'tie_{size[0]}x{size[1]}', resident)


def test_plans_against_the_lp_oracle():
    ec.check_lp_oracle(DEV)


def test_bits_alone_first_last_permuted_and_run_to_run():
    ec.check_bits(DEV)


def test_status_of_a_nan_problem():
    ec.check_status(DEV)


def test_validation_errors():
    ec.check_validation_errors(DEV)


def test_resident_switch_from_the_environment(monkeypatch):
    monkeypatch.setenv('EQD_DOCK_EMD_RESIDENT', '0')
    assert not DK.emd_resident_enabled()
    ec.check_against_host(DEV, 'tie_12x12', None, alone=False)
    monkeypatch.delenv('EQD_DOCK_EMD_RESIDENT')
    assert DK.emd_resident_enabled()


@pytest.fixture
def model_simulator():
    from equidock_public_amd import _lib
    from tests.hostsim import build as hs
    _lib.load_library_for_testing(hs.build())
    yield
    _lib.unload_for_testing()


def test_pocket_ot_loss_on_the_device_solver(model_simulator, monkeypatch):
    ec.check_pocket_ot_loss(DEV, monkeypatch)


def test_train_step_on_the_device_solver(model_simulator):
    ec.check_train_step(DEV)
