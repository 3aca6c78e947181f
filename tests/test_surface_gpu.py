"""GPU tests (-m gpu) of the surface-function kernels (tests/surface_common.py) on a real MI355X: one exact clash-removal
step of k_dock_* (alone and all cases in one batch) and of k_clash_* at every shape around their tile and chunk edges,
from zero and from non-zero angles, and the pair losses on a ragged batch crossing 256-row and 1 024-partner edges,
against float64."""
import pytest
import torch

from tests import surface_common as sc

pytestmark = pytest.mark.gpu

STATES = ('zero', 'angles', 'pitch90')


@pytest.fixture(scope='module')
def dev():
    from equidock_public_amd import _lib, dock as DK
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.unload_for_testing()
    _lib.load_library()
    DK.unload_dock_for_testing()
    DK.load_dock_library()
    assert not DK._dock_is_sim and not _lib.is_simulator()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def dock_cases():
    return sc.clash_cases(sc.DOCK_SHAPES, STATES, 256, 512)


def test_dock_one_step_alone(dev, dock_cases):
    worst = [0.0, 0.0]
    for case in dock_cases:
        worst = [max(w, e) for w, e in zip(worst, sc.dock_steps(dev, [case]))]
    print('dock alone: loss / gradient error of the scale: %.2e %.2e' % tuple(worst))


def test_dock_one_step_batched(dev, dock_cases):
    print('dock batch: loss / gradient error of the scale: %.2e %.2e' % tuple(sc.dock_steps(dev, dock_cases)))


def test_single_complex_one_step(dev):
    worst = [0.0, 0.0]
    for case in sc.clash_cases(sc.SINGLE_SHAPES, STATES, 256, 1024):
        worst = [max(w, e) for w, e in zip(worst, sc.single_step(dev, case))]
    print('single complex: loss / gradient error of the scale: %.2e %.2e' % tuple(worst))


@pytest.mark.parametrize('sigma,ct', [(25.0, 10.0), (8.0, 8.0)])
def test_pair_losses_at_chunk_edges(dev, sigma, ct):
    e = sc.pair_losses_at_edges(dev, sc.pair_batch(dev), sc.PAIR_SIZES, sigma, ct)
    print('pair losses sigma %g: forward / backward error of the scale: %.2e %.2e' % ((sigma,) + e))
