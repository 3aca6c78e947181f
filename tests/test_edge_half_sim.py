"""CPU tests (host simulator): the half-tile edge-forward body of the fused small-batch launch (k_edge_attn_fwd_half,
csrc/eqd_edge_fwd_half_inl.h: 1 024-thread workgroups, a pair of waves per 32-edge tile) computes the bytes of the
whole-tile body and is selected for exactly the fused fp32 launches of the 64-wide layers.  The simulator runs the same
source - the split of a tile's edges and of the means' column blocks, the two feature regions, the barrier that idle
pairs and empty halves must reach - one fiber per thread; what it cannot show is timing between the two waves of a pair
(tests/test_edge_half_gpu.py runs the same checks on the GPU, and replays)."""
import pytest
import torch

from equidock_public_amd import _lib
from tests import edge_half_common as eh

DEV = torch.device('cpu')


@pytest.fixture(scope='module', autouse=True)
def simulator():
    from tests.hostsim import build as hs
    lib = hs.build()
    _lib.load_library_for_testing(lib)
    assert _lib.is_simulator()
    yield
    _lib.unload_for_testing()


@pytest.mark.parametrize('drop', (False, True), ids=('plain', 'dropout'))
@pytest.mark.parametrize('name', sorted(eh.GRAPHS))
def test_tile_shapes_byte_equal(name, drop, monkeypatch):
    eh.check_graph(DEV, monkeypatch, name, drop)


def test_not_eligible_stays_on_the_whole_tile_kernels(monkeypatch):
    eh.check_not_eligible(DEV, monkeypatch, many_tiles=False)      # (2 060 tiles: the GPU file)


@pytest.mark.parametrize('name,dropout', [('B_b3_dips8', 0.0), ('D_degraded3', 0.25)])
def test_golden_cases_bit_equal(name, dropout, monkeypatch):
    eh.check_golden_case(DEV, monkeypatch, name, dropouts=(dropout,))      # (both dropouts of both cases: the GPU file)
