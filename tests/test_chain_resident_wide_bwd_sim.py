"""CPU tests (host simulator): the wide resident body of the first layer's backward node chain (k_rowchain_res_bwd_wide,
csrc/eqd_chainres_bwd_wide_inl.h) computes the bits of k_rowchain's general body, and is selected for exactly the six-job
list of the 69-wide layer.  The simulator checks addressing - the per-wave slabs, the two-piece images of output block 4,
the image of the rows k = 64 .. 68 and their zero padding, ragged tiles, the stores of 69- and 80-float rows - from the same
source; the waits of the asynchronous copies are only exercised on the GPU (tests/test_chain_resident_wide_bwd_gpu.py)."""
import pytest
import torch

from equidock_public_amd import _lib
from tests import chain_resident_wide_bwd_common as cwb

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
    cwb.check_golden_case(DEV, monkeypatch, name)


# every row count and every depth once, with and without dropout in turn (the GPU file runs the whole product)
@pytest.mark.parametrize('sizes,layers,dropout', list(zip(cwb.SIZES, (2, 3, 2, 3, 2), (0.0, 0.25, 0.25, 0.0, 0.25))),
                         ids=lambda v: '%d_rows' % sum(a + b for a, b in v) if isinstance(v, list) else str(v))
def test_sizes_and_depths_bit_equal(sizes, layers, dropout, monkeypatch):
    cwb.check_sizes(DEV, monkeypatch, sizes, layers, dropouts=(dropout,))


def test_counters(monkeypatch):
    cwb.check_counted(DEV, monkeypatch)


def test_not_eligible_stays_on_the_general_bodies(monkeypatch):
    cwb.check_not_eligible(DEV, monkeypatch, many_tiles=False)      # (4 112 rows: the GPU file)


def test_guard_rows_and_float64_formulas(monkeypatch):
    cwb.check_guard_rows(DEV, monkeypatch)
