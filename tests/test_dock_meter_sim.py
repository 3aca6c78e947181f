"""CPU tests of the batched RMSD meter: csrc_dock/ compiled for x86 against the host simulator and driven through
equidock_public_amd.dock, as on the GPU (the shared checks live in tests/dock_meter_common.py)."""
import pytest
import torch

from equidock_public_amd import dock as DK
from tests import dock_common as dc
from tests import dock_meter_common as mc

DEV = torch.device('cpu')


@pytest.fixture(scope='module', autouse=True)
def simulator():
    DK.load_dock_library_for_testing(dc.build_sim())
    assert DK._dock_is_sim
    yield
    DK.unload_dock_for_testing()


def test_abi():
    lib = DK.load_dock_library()
    assert lib.eqd_dock_meter_abi() == DK.DOCK_METER_ABI == 1 and lib.eqd_dock_abi_version() == 1


def test_golden_inputs_in_one_batch():
    mc.check_golden(DEV)


def test_tile_and_chunk_edges():
    mc.check_edges(DEV)


def test_degenerate_sets():
    mc.check_degenerate(DEV)


def test_bits_alone_first_last_permuted_and_run_to_run():
    mc.check_bits(DEV)


def test_rec_pred_given_against_null():
    mc.check_rec_pred(DEV)


def test_device_meter_against_the_host_meter():
    mc.check_device_meter(DEV)


def test_validation_errors():
    mc.check_validation_errors(DEV)


@pytest.fixture
def model_simulator():
    from equidock_public_amd import _lib
    from tests.hostsim import build as hs
    _lib.load_library_for_testing(hs.build())
    yield
    _lib.unload_for_testing()


def test_train_step_with_a_meter(model_simulator):
    mc.check_train_step_meter(DEV)


def test_dock_complexes_with_ground_truth(model_simulator):
    mc.check_dock_complexes_ground_truth(DEV, ('graph_case', 'graph_case_tiny'), max_it=5, check_every=2)
