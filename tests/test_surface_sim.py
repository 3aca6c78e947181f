"""CPU tests of the surface-function kernels (tests/surface_common.py) on the x86 simulator builds of both libraries:
one exact clash-removal step of k_dock_* and k_clash_* and the pair losses, against float64 at tile and chunk edges.
The shapes of tests/test_surface_gpu.py; the start state with pitch near pi/2 only in the batch."""
import numpy as np
import pytest
import torch

from equidock_public_amd import _lib, dock as DK
from tests import dock_common as dc, surface_common as sc

DEV = torch.device('cpu')


@pytest.fixture(scope='module', autouse=True)
def simulators():
    from tests.hostsim import build as hs
    _lib.load_library_for_testing(hs.build())
    DK.load_dock_library_for_testing(dc.build_sim())
    assert _lib.is_simulator() and DK._dock_is_sim
    yield
    DK.unload_dock_for_testing()
    _lib.unload_for_testing()


def test_rot_mat_matches_the_reference():
    """the tests' own R = RZ(yaw) RY(pitch) RX(roll) reproduces the reference's get_rot_mat output"""
    z = np.load(sc.GOLDEN + '/inference_case.npz')
    R = sc.rot_mat(torch.from_numpy(z['rot_euler']).double())
    assert float((R - torch.from_numpy(z['rot_mat']).double()).abs().max()) <= 1e-6


@pytest.mark.parametrize('shape', sc.DOCK_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_dock_one_step_alone(shape):
    """k_dock_eval / _grad / _step: one complex, from zero and from non-zero angles"""
    for case in sc.clash_cases([shape], ('zero', 'angles'), 256, 512):
        print(case['what'], 'loss / gradient error of the scale: %.2e %.2e' % tuple(sc.dock_steps(DEV, [case])))


def test_dock_one_step_batched():
    """the same kernels with every shape and start state in one batch"""
    cases = sc.clash_cases(sc.DOCK_SHAPES, ('zero', 'angles', 'pitch90'), 256, 512)
    print('batch: loss / gradient error of the scale: %.2e %.2e' % tuple(sc.dock_steps(DEV, cases)))


@pytest.mark.parametrize('shape', sc.SINGLE_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_single_complex_one_step(shape):
    """k_clash_lig / _rec / _grad / _step (eqd_clash_iterations)"""
    for case in sc.clash_cases([shape], ('zero', 'angles'), 256, 1024):
        print(case['what'], 'loss / gradient error of the scale: %.2e %.2e' % tuple(sc.single_step(DEV, case)))


@pytest.mark.parametrize('sigma,ct', [(25.0, 10.0), (8.0, 8.0)])
def test_pair_losses_at_chunk_edges(sigma, ct):
    """k_pair_losses_fwd / _bwd on one ragged batch whose pairs cross 256-row and 1 024-partner edges on both sides"""
    e = sc.pair_losses_at_edges(DEV, sc.pair_batch(DEV), sc.PAIR_SIZES, sigma, ct)
    print('pair losses forward / backward error of the scale: %.2e %.2e' % e)
