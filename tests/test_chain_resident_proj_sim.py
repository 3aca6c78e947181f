"""CPU tests (host simulator): the carrying forms of the resident forward node chain (k_rowchain_res_fwd<5> / <1>,
csrc/eqd_chainres_inl.h) compute the bits of the two-job body followed by the projections' own launches, and are selected
for exactly the lists the model driver builds for 64-wide fp32 layers with cross messages.  The simulator checks addressing
- the refilled weight slots, the tile of h[l+1] in LDS, ragged tiles, the held-back stores, the epilogues - from the same
source; the waits of the asynchronous copies are only exercised on the GPU (tests/test_chain_resident_proj_gpu.py)."""
import pytest
import torch

from equidock_public_amd import _lib
from tests import chain_resident_proj_common as crp

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
    # (with dropout only: the simulator takes a minute per step of these batches; the GPU file runs both)
    crp.check_golden_case(DEV, monkeypatch, name, dropouts=(0.25,))


@pytest.mark.parametrize('layers', crp.LAYERS)
@pytest.mark.parametrize('sizes', crp.SIZES, ids=lambda s: '%d_rows' % crp.rows_of(s))
def test_sizes_and_depths_bit_equal(sizes, layers, monkeypatch):
    crp.check_sizes(DEV, monkeypatch, sizes, layers)


def test_carrying_forms_are_counted_and_replace_k_linear_launches(monkeypatch):
    crp.check_forms_counted(DEV, monkeypatch)


def test_not_eligible_keeps_the_separate_launches(monkeypatch):
    crp.check_not_eligible(DEV, monkeypatch, many_tiles='forward')


def test_guard_rows_and_clamped_source_rows(monkeypatch):
    crp.check_guard_rows(DEV, monkeypatch)
