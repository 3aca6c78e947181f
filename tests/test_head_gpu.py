"""GPU tests (-m gpu) of the keypoint / Kabsch head (tests/head_common.py) on a real MI355X: eqd_kabsch_fwd / _bwd over
K = 1 .. 128 and through every guard path, keypoint pooling past 64 heads under both kernel forms, and the model at
num_att_heads 64 .. 128 with ligands either side of the fused apply's 64-row stride, against float64."""
import pytest
import torch

from tests import head_common as hc, parity_common as pc

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 4, 16, 50, 63, 64, 65, 100, 127, 128]
GUARDS = [('planar', 64, (1, 3, 10)), ('planar', 100, (2, 1, 7)), ('planar', 128, (10, 1, 4)),
          ('collapsed', 16, (1, 2, 10)), ('collapsed', 65, (1, 6, 3)), ('collapsed', 127, (4, 10, 1))]


@pytest.fixture(scope='module')
def dev():
    from equidock_public_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.unload_for_testing()
    _lib.load_library()
    assert not _lib.is_simulator()
    return torch.device('cuda:0')


def _merge(worst, more):
    for k, v in more.items():
        worst[k] = max(worst.get(k, 0.0), v)


def test_kabsch_operators(dev):
    worst, signs = {}, set()
    for K in KS:
        w, s = hc.check_kabsch_batch(dev, hc.kabsch_batch(K, seed=100 + K), seed=K)
        _merge(worst, w)
        signs |= s
    for kind, K, its in GUARDS:
        _merge(worst, hc.check_kabsch_batch(dev, hc.guard_batch(kind, K, its, seed=K + len(kind)), seed=K)[0])
    assert signs == {-1, 1}
    print('Kabsch: ' + ', '.join(f'{k} {v:.2e}' for k, v in sorted(worst.items())))


def test_kabsch_exits_seeds_and_limit(dev):
    hc.check_status_11(dev)
    print('planar, status 11: %.2e' % hc.check_planar_unstable(dev))
    for K in (2, 64, 128):
        hc.check_seeded_draws(dev, K)
    hc.check_kabsch_limit(dev)


@pytest.mark.parametrize('mm', ['0', '1'])
def test_keypoint_pool_head_counts(dev, mm, monkeypatch):
    monkeypatch.setenv('EQD_KEYPOINT_MM', mm)
    worst = [0.0, 0.0]
    for K in (64, 65, 100, 127, 128):
        worst = [max(a, b) for a, b in zip(worst, hc.check_keypoint_pool(dev, K))]
    print('keypoint pool MM=%s: keypoints %.2e, gradients %.2e' % ((mm,) + tuple(worst)))


@pytest.mark.parametrize('K', [64, 65, 100, 128])
def test_model_head_counts(dev, K):
    hc.check_model(dev, K)
    pc.check_head_backward(dev, hc.HEAD_SIZES, layers=2, num_att_heads=K, what=f'num_att_heads={K}')
    print('fused apply K=%d: forward %.2e, backward %.2e' % ((K,) + hc.check_fused_apply(dev, K)))


def test_head_backward_bf16_100_heads(dev):
    pc.check_head_backward(dev, hc.HEAD_SIZES, layers=2, bf16=True, num_att_heads=100, what='num_att_heads=100 bf16')


def test_model_head_limit(dev):
    hc.check_model_limit(dev)
