"""CPU tests (host simulator): the resident-weights body of the forward node chain computes the bits of k_rowchain.  The
simulator checks addressing - the swizzled LDS image, the per-wave ownership of weight rows, ragged tiles, the epilogue -
from the same source; the waits of the asynchronous copies are only exercised on the GPU (tests/test_chain_resident_gpu.py)."""
import pytest
import torch

from equidock_public_amd import _lib
from tests import chain_resident_common as cr

DEV = torch.device('cpu')


@pytest.fixture(scope='module', autouse=True)
def simulator():
    from tests.hostsim import build as hs
    lib = hs.build()
    _lib.load_library_for_testing(lib)
    assert _lib.is_simulator()
    yield
    _lib.unload_for_testing()


@pytest.mark.parametrize('name', ['B_b3_dips8', 'D_degraded3'])
def test_golden_cases_bit_equal(name, monkeypatch):
    cr.check_golden_case(DEV, monkeypatch, name)


def test_ragged_last_tile_bit_equal(monkeypatch):
    cr.check_ragged_tiles(DEV, monkeypatch)


def test_workload_b_batch_bit_equal(monkeypatch):
    cr.check_workload_b(DEV, monkeypatch)
