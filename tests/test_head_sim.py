"""CPU tests of the keypoint / Kabsch head (tests/head_common.py) on the x86 simulator build: eqd_kabsch_fwd / _bwd over
K = 1 .. 128 and through every guard path, keypoint pooling past 64 heads, and the model at num_att_heads 64 .. 128 with
ligands either side of the fused apply's 64-row stride, against float64."""
import pytest
import torch

from equidock_public_amd import _lib
from tests import head_common as hc, parity_common as pc

DEV = torch.device('cpu')
KS = [1, 2, 3, 4, 16, 50, 63, 64, 65, 100, 127, 128]


@pytest.fixture(scope='module', autouse=True)
def simulator():
    from tests.hostsim import build as hs
    _lib.load_library_for_testing(hs.build())
    assert _lib.is_simulator()
    yield
    _lib.unload_for_testing()


def _report(what, worst):
    print(what + ': ' + ', '.join(f'{k} {v:.2e}' for k, v in worst.items()))


@pytest.mark.parametrize('K', KS)
def test_kabsch_keypoint_counts(K):
    """six pairs per call, spreads 1 - 100 A at PDB offsets, both det signs, two near-degenerate pairs (K <= 3: guard pairs,
    1 .. 10 iterations); T absolute, b of |mean_r| + |mean_l|, dY of the pair's largest |dY|"""
    worst, signs = hc.check_kabsch_batch(DEV, hc.kabsch_batch(K, seed=100 + K), seed=K)
    assert K <= 3 or signs == {-1, 1}, signs
    _report(f'Kabsch K={K}', worst)


GUARDS = [('planar', 64, (1, 3, 10)), ('planar', 100, (2, 1, 7)), ('planar', 128, (10, 1, 4)),
          ('collapsed', 16, (1, 2, 10)), ('collapsed', 65, (1, 6, 3)), ('collapsed', 127, (4, 10, 1))]


@pytest.mark.parametrize('kind,K,its', GUARDS, ids=[f'{k}-{K}' for k, K, _ in GUARDS])
def test_kabsch_guard(kind, K, its):
    """the guard through explicit draws: status = the reference's iteration count (10 included), T, b, A_out, dY through
    the guarded A, T orthonormal with det T = sign det A"""
    batch = hc.guard_batch(kind, K, its, seed=K + len(kind))
    worst, _ = hc.check_kabsch_batch(DEV, batch, seed=K)
    _report(f'guard {kind} K={K}', worst)


def test_kabsch_unstable_exit():
    """status 11 after ten ineffective draws: A = 0 at K = 1 (finite T, b and backward), and planar keypoints whose zero
    column the draws never touch (the rank-deficient completion of U)"""
    hc.check_status_11(DEV)
    print('planar, status 11: |T T^T - I|, |T v - u| %.2e' % hc.check_planar_unstable(DEV))


@pytest.mark.parametrize('K', [2, 64, 128])
def test_kabsch_seeded_draws(K):
    print('seeded draws, status', hc.check_seeded_draws(DEV, K))


def test_kabsch_limit():
    hc.check_kabsch_limit(DEV)


@pytest.mark.parametrize('K', [64, 65, 100, 127, 128])
@pytest.mark.parametrize('mm', ['0', '1'])
def test_keypoint_pool_head_counts(K, mm, monkeypatch):
    """segments of 1 node and of 1 030 nodes, under both kernel forms"""
    monkeypatch.setenv('EQD_KEYPOINT_MM', mm)
    print('keypoint pool K=%d MM=%s: keypoints %.2e, gradients %.2e' % ((K, mm) + hc.check_keypoint_pool(DEV, K)))


@pytest.mark.parametrize('K', [64, 65, 100, 128])
def test_model_head_counts(K):
    hc.check_model(DEV, K)
    pc.check_head_backward(DEV, hc.HEAD_SIZES, layers=2, num_att_heads=K, what=f'num_att_heads={K}')
    print('fused apply K=%d: forward %.2e, backward %.2e' % ((K,) + hc.check_fused_apply(DEV, K)))


def test_head_backward_bf16_100_heads():
    pc.check_head_backward(DEV, hc.HEAD_SIZES, layers=2, bf16=True, num_att_heads=100, what='num_att_heads=100 bf16')


def test_model_head_limit():
    hc.check_model_limit(DEV)
