"""GPU tests (-m gpu) of the batched RMSD meter: libequidock_dock.so on a real MI355X through equidock_public_amd.dock
(the shared checks live in tests/dock_meter_common.py), dock_complexes(ground_truth=...), the command line's
--device-metrics and TrainStep(meter=...)."""
import re
import subprocess
import sys

import pytest
import torch

from tests import dock_common as dc
from tests import dock_meter_common as mc

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


def test_golden_inputs_in_one_batch(dev):
    mc.check_golden(dev)


def test_tile_and_chunk_edges(dev):
    mc.check_edges(dev)


def test_degenerate_sets(dev):
    mc.check_degenerate(dev)


def test_bits_alone_first_last_permuted_and_run_to_run(dev):
    mc.check_bits(dev)


def test_rec_pred_given_against_null(dev):
    mc.check_rec_pred(dev)


def test_device_meter_against_the_host_meter(dev):
    mc.check_device_meter(dev)


def test_device_meter_downloads_once_and_never_synchronises(dev, monkeypatch):
    """two update_batch calls (2 and 5 complexes): no Tensor.cpu, no stream synchronisation; summarize: one download"""
    from equidock_public_amd import dock as DK
    cases = [mc.all_cases()[n] for n in ('1AVX', 'edge_2x2', '1H1V', 'edge_256x512', '1HCF', 'edge_1x3', 'no_pair')]
    dev_cases = [[mc._t(c[0], dev), mc._t(c[3], dev), mc._t(c[2], dev), mc._t(c[3], dev)] for c in cases]
    calls = {'cpu': 0, 'sync': 0}
    real_cpu, real_sync = torch.Tensor.cpu, torch.cuda.Stream.synchronize

    def cpu(self, *a, **k):
        calls['cpu'] += int(self.is_cuda)
        return real_cpu(self, *a, **k)

    def sync(self):
        calls['sync'] += 1
        return real_sync(self)

    meter = DK.DeviceMeter(interface=True)
    monkeypatch.setattr(torch.Tensor, 'cpu', cpu)
    monkeypatch.setattr(torch.cuda.Stream, 'synchronize', sync)
    for part in (dev_cases[:2], dev_cases[2:]):
        meter.update_batch([c[0] for c in part], None, [c[2] for c in part], [c[3] for c in part])
    assert calls == {'cpu': 0, 'sync': 0}, calls
    meter.summarize('mean')
    assert calls == {'cpu': 1, 'sync': 0}, calls
    meter.summarize_with_std('median')
    assert calls == {'cpu': 2, 'sync': 0}, calls
    monkeypatch.undo()
    assert len(meter) == 7 and meter.rows().shape == (7, 8)


def test_validation_errors(dev):
    mc.check_validation_errors(dev)


def test_dock_complexes_with_ground_truth(dev):
    mc.check_dock_complexes_ground_truth(dev, dc.REAL, max_it=20, check_every=10)


LINE = re.compile(r'^(\w+): \d+ ligand atoms, \d+ receptor atoms -> \S+  clash iterations \d+, loss [-\d.]+'
                  r'  CRMSD ([\d.]+)  IRMSD ([\d.]+)$')


def test_command_line_device_metrics(dev, tmp_path):
    """the command line with and without --device-metrics on the files test_command_line writes: the per-complex CRMSD /
    IRMSD of the two runs differ by at most 1e-3 A (the file path reads coordinates rounded to 3 decimals: <= 5e-4 per
    axis, and the RMSD is 1-Lipschitz in the RMS displacement: <= 8.7e-4), same line format, same summary lines"""
    net, args, sd = dc.seeded_net(dev)
    ckpt = tmp_path / 'db5_model_best.pth'
    torch.save({'args': dict(args, device=torch.device('cpu'), graph_cutoff=30.0, graph_max_neighbor=10,
                             pocket_cutoff=8.0, intersection_loss_weight=10.0), 'state_dict': sd}, ckpt)
    inp, gt = tmp_path / 'in', tmp_path / 'gt'
    inp.mkdir()
    gt.mkdir()
    names = ['GCAS', 'P300', 'BIGL']
    for nm, fx in zip(names, dc.REAL):
        lig, rec = dc.fixture_residues(fx)
        dc.write_pdb(lig, inp / f'{nm}_l_b.pdb')
        dc.write_pdb(lig, gt / f'{nm}_l_b_COMPLEX.pdb')
        dc.write_pdb(rec, gt / f'{nm}_r_b_COMPLEX.pdb')
    got = {}
    for flag in ((), ('--device-metrics',)):
        cmd = [sys.executable, '-m', 'equidock_public_amd.dock', '--checkpoint', str(ckpt), '--input-dir', str(inp),
               '--gt-dir', str(gt), '--out-dir', str(tmp_path / ('out' + str(len(flag)))), '--remove-clashes', '--batch', '2',
               '--max-it', '20'] + list(flag)
        p = subprocess.run(cmd, cwd=dc.ROOT, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        lines = p.stdout.strip().splitlines()
        assert len(lines) == 6, p.stdout
        ms = [LINE.match(ln) for ln in lines[:3]]
        assert all(ms), p.stdout
        assert lines[3].startswith('Mean runtime:') and lines[4].startswith('CRMSD median/mean/std: ') \
            and lines[5].startswith('IRMSD median/mean/std: '), p.stdout
        got[flag] = {m.group(1): (float(m.group(2)), float(m.group(3))) for m in ms}
    host, device = got[()], got[('--device-metrics',)]
    assert sorted(host) == sorted(device) == sorted(names)
    for nm in names:
        for a, b in zip(host[nm], device[nm]):
            print(f'{nm}: host files {a:.3f}  device {b:.3f}')
            assert abs(a - b) <= 1e-3 + 1e-9, (nm, host[nm], device[nm])
    # a missing ground truth is an error with the flag
    (gt / 'BIGL_l_b_COMPLEX.pdb').unlink()
    p = subprocess.run(cmd, cwd=dc.ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and 'BIGL_l_b_COMPLEX.pdb' in p.stderr


def test_train_step_with_a_meter(dev):
    mc.check_train_step_meter(dev)
