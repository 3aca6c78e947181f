"""CPU tests (host simulator): the wide resident body of the first layer's forward node chain (k_rowchain_res_fwd_wide,
csrc/eqd_chainres_wide_inl.h) computes the bits of k_rowchain's general body, and is selected for exactly the two-job list
of the 69-wide layer.  The simulator checks addressing - the 80-row swizzled chunk images, the two-piece remainder images
and their zero padding, ragged tiles, the element-wise stores of 69-float rows - from the same source; the waits of the
asynchronous copies are only exercised on the GPU (tests/test_chain_resident_wide_gpu.py)."""
import pytest
import torch

from equidock_public_amd import _lib
from tests import chain_resident_wide_common as crw

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
    crw.check_golden_case(DEV, monkeypatch, name)


# every row count and every depth once (the GPU file runs the whole product: the wide body is layer 0's forward chain, the
# same launch at every depth - what changes with the depth is what the older counters must report around it)
@pytest.mark.parametrize('sizes,layers', list(zip(crw.SIZES, (1, 2, 3, 2, 1))),
                         ids=lambda v: '%d_rows' % sum(a + b for a, b in v) if isinstance(v, list) else '%d_layers' % v)
def test_sizes_and_depths_bit_equal(sizes, layers, monkeypatch):
    crw.check_sizes(DEV, monkeypatch, sizes, layers)


def test_not_eligible_stays_on_the_general_bodies(monkeypatch):
    crw.check_not_eligible(DEV, monkeypatch)


def test_guard_rows_and_clamped_source_rows(monkeypatch):
    crw.check_guard_rows(DEV, monkeypatch)
