"""GPU tests (-m gpu) of the batched exact transport solver on the device: libequidock_dock.so on a real MI355X through
equidock_public_amd.dock (the shared checks live in tests/dock_emd_common.py), losses.pocket_ot_loss(solver='device') and
train_step.TrainStep(ot_solver='device').  Every loop of the kernel has a bound computed from the problem's sizes, so each
of these ends on any input."""
import pytest
import torch

from tests import dock_emd_common as ec

pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize('resident', [True, False], ids=['resident', 'general'])
def test_plans_are_the_host_solvers_k50(dev, resident):
    ec.check_against_host(dev, 'k50', resident)


@pytest.mark.parametrize('resident', [True, False], ids=['resident', 'general'])
@pytest.mark.parametrize('K', ec.N40_COLS)
def test_plans_are_the_host_solvers_n40(dev, K, resident):
    ec.check_against_host(dev, f'n40_{K}', resident)


@pytest.mark.parametrize('resident', [True, False], ids=['resident', 'general'])
@pytest.mark.parametrize('size', ec.TIE_SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_ties_settle_in_the_host_solvers_order(dev, size, resident):
    ec.check_against_host(dev, f'tie_{size[0]}x{size[1]}', resident)


def test_plans_against_the_lp_oracle(dev):
    ec.check_lp_oracle(dev)


def test_bits_alone_first_last_permuted_and_run_to_run(dev):
    ec.check_bits(dev)


def test_status_of_a_nan_problem(dev):
    ec.check_status(dev)


def test_validation_errors(dev):
    ec.check_validation_errors(dev)


def test_pocket_ot_loss_on_the_device_solver(dev):
    ec.check_pocket_ot_loss(dev)


def test_pocket_ot_loss_neither_synchronises_nor_downloads(dev, monkeypatch):
    """pocket_ot_loss(solver='device') on a prepared EmdPlan, forward and backward: no Tensor.cpu, no synchronisation"""
    from equidock_public_amd import dock as DK, losses
    pls, prs, Yl, Yr, w = ec.pocket_inputs()
    pls, prs, w = [t.to(dev) for t in pls], [t.to(dev) for t in prs], w.to(dev)
    a, b = Yl.to(dev).requires_grad_(True), Yr.to(dev).requires_grad_(True)
    ep = DK.EmdPlan(list(ec.OT_COUNTS), ec.OT_K, dev)
    calls = {'cpu': 0, 'sync': 0}
    real_cpu, real_ssync, real_sync = torch.Tensor.cpu, torch.cuda.Stream.synchronize, torch.cuda.synchronize

    def cpu(self, *args, **kw):
        calls['cpu'] += int(self.is_cuda)
        return real_cpu(self, *args, **kw)

    def ssync(self):
        calls['sync'] += 1
        return real_ssync(self)

    def sync(*args, **kw):
        calls['sync'] += 1
        return real_sync(*args, **kw)

    monkeypatch.setattr(torch.Tensor, 'cpu', cpu)
    monkeypatch.setattr(torch.cuda.Stream, 'synchronize', ssync)
    monkeypatch.setattr(torch.cuda, 'synchronize', sync)
    ot = losses.pocket_ot_loss(a, b, pls, prs, solver='device', emd_plan=ep)
    (ot * w).sum().backward()
    assert calls == {'cpu': 0, 'sync': 0}, calls
    monkeypatch.undo()
    assert ep.failed() == [] and bool(torch.isfinite(a.grad).all())


def test_train_step_one_graph_three_replays(dev):
    ec.check_train_step(dev)


@pytest.mark.parametrize('variant', ['meter', 'bf16', 'dropout'])
def test_train_step_variants(dev, variant):
    ec.check_train_step(dev, meter=variant == 'meter', bf16=variant == 'bf16', dropout=0.25 if variant == 'dropout' else 0.0,
                        replays=1)
