"""GPU tests (-m gpu) of the batched docking quality (fnat, LRMSD, backbone iRMSD, DockQ, clashes): libequidock_dock.so on
a real MI355X through equidock_public_amd.dock (the shared checks live in tests/dock_quality_common.py),
dock_complexes(quality=True) and the command line's --dockq."""
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import dock_common as dc
from tests import dock_quality_common as qc

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


def test_abi(dev):
    from equidock_public_amd import dock as DK
    assert DK.load_dock_library().eqd_dock_quality_abi() == DK.DOCK_QUALITY_ABI == 1


def test_real_complexes_in_one_batch(dev):
    qc.check_real(dev)


def test_near_native_poses(dev):
    qc.check_near_native(dev)


def test_tile_chunk_and_staging_edges(dev):
    qc.check_edges(dev)


def test_degenerate_sets(dev):
    qc.check_degenerate(dev)


def test_bits_alone_first_last_permuted_and_run_to_run(dev):
    qc.check_bits(dev)


def test_pruning_changes_no_other_column(dev, monkeypatch):
    qc.check_pruning(dev, monkeypatch)


def test_validation_errors(dev):
    qc.check_validation_errors(dev)


def test_pose_quality_batch_never_synchronises_or_downloads(dev, monkeypatch):
    """8. with a plan (its init has copied the item table): no Tensor.cpu, no stream or device synchronisation inside
    pose_quality_batch; without one, the only wait is the init's own, inside the library"""
    from equidock_public_amd import dock as DK
    cases = [qc.all_cases()[n] for n in ('1AVX_NO_CLASHES', 'edge_1x1', 'edge_17x65', 'no_native_contact')]
    args = ([qc._t(c[0], dev) for c in cases], [qc._t(c[2], dev) for c in cases], [qc._t(c[3], dev) for c in cases])
    tables = ([c[4] for c in cases], [c[5] for c in cases], [c[6] for c in cases], [c[7] for c in cases])
    plan = DK.QualityPlan(*tables, dev)
    calls = {'cpu': 0, 'sync': 0}
    real_cpu, real_sync, real_dsync = torch.Tensor.cpu, torch.cuda.Stream.synchronize, torch.cuda.synchronize

    def cpu(self, *a, **k):
        calls['cpu'] += int(self.is_cuda)
        return real_cpu(self, *a, **k)

    def sync(self):
        calls['sync'] += 1
        return real_sync(self)

    def dsync(*a, **k):
        calls['sync'] += 1
        return real_dsync(*a, **k)

    monkeypatch.setattr(torch.Tensor, 'cpu', cpu)
    monkeypatch.setattr(torch.cuda.Stream, 'synchronize', sync)
    monkeypatch.setattr(torch.cuda, 'synchronize', dsync)
    with_plan = DK.pose_quality_batch(*args, plan=plan)
    again = DK.pose_quality_batch(*args, plan=plan)
    fresh = DK.pose_quality_batch(*args, *tables)
    assert calls == {'cpu': 0, 'sync': 0}, calls
    monkeypatch.undo()
    assert with_plan['plan'] is plan and fresh['plan'] is not plan
    rows = with_plan['quality'].cpu().numpy()
    assert rows.tobytes() == again['quality'].cpu().numpy().tobytes() == fresh['quality'].cpu().numpy().tobytes()
    assert rows.tobytes() == qc.run(dev, cases).tobytes()


def test_quality_pass_is_capturable(dev):
    """eval neither synchronises, allocates nor copies: captured into a graph and replayed on new coordinates, it gives the
    bits of the host-enqueued pass"""
    from equidock_public_amd import dock as DK
    cases = [qc.all_cases()[n] for n in ('1HCF_NO_CLASHES', 'edge_9x33')]
    plan = DK.QualityPlan([c[4] for c in cases], [c[5] for c in cases], [c[6] for c in cases], [c[7] for c in cases], dev)
    lp, lt, rt = (torch.cat([qc._t(c[k], dev) for c in cases]) for k in (0, 2, 3))
    out = torch.zeros(2, DK.QUALITY_COLS, dtype=torch.float64, device=dev)
    want = plan.eval(lp, None, lt, rt, torch.empty_like(out)).cpu().numpy()
    buf = lt.clone()                                   # (captured with the exact prediction, replayed with the model)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        plan.eval(buf, None, lt, rt, out)
    torch.cuda.current_stream(dev).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.eval(buf, None, lt, rt, out)
    buf.copy_(lp)
    g.replay()
    torch.cuda.synchronize(dev)
    assert out.cpu().numpy().tobytes() == want.tobytes()


def test_dock_complexes_with_quality(dev):
    qc.check_dock_complexes_quality(dev, dc.REAL, max_it=20, check_every=10)


LINE = re.compile(r'^(\w+): \d+ ligand atoms, \d+ receptor atoms -> \S+  clash iterations \d+, loss [-\d.]+'
                  r'  CRMSD ([\d.]+)  IRMSD ([\d.]+)$')
DOCKQ = re.compile(r'^(.*?)  DockQ ([\d.]+|nan)  fnat ([\d.]+|nan)  LRMSD ([\d.]+|nan)  iRMSD\(bb\) ([\d.]+|nan)  clashes (\d+)$')


def test_command_line_dockq(dev, tmp_path):
    """10. the command line with and without --dockq on written files: without the flag the lines match the existing LINE
    pattern exactly; with it the line is that line plus the appended fields, which equal the in-process values of
    dock_complexes(quality=True) on the same files to the printed digits, followed by the two summary lines"""
    from equidock_public_amd import dock as DK
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
    order = sorted(names)
    complexes = [(str(inp / f'{nm}_l_b.pdb'), str(gt / f'{nm}_r_b_COMPLEX.pdb')) for nm in order]
    truths = [str(gt / f'{nm}_l_b_COMPLEX.pdb') for nm in order]
    want = {}
    for b0 in (0, 2):                                  # (--batch 2)
        for nm, r in zip(order[b0:b0 + 2], DK.dock_complexes(net, complexes[b0:b0 + 2], remove_clashes=True, max_it=20,
                                                             device=dev, ground_truth=truths[b0:b0 + 2], quality=True)):
            want[nm] = r
    got = {}
    for flag in ((), ('--dockq',)):
        cmd = [sys.executable, '-m', 'equidock_public_amd.dock', '--checkpoint', str(ckpt), '--input-dir', str(inp),
               '--gt-dir', str(gt), '--out-dir', str(tmp_path / ('out' + str(len(flag)))), '--remove-clashes', '--batch', '2',
               '--max-it', '20'] + list(flag)
        p = subprocess.run(cmd, cwd=dc.ROOT, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        got[flag] = p.stdout.strip().splitlines()
    plain, with_q = got[()], got[('--dockq',)]
    assert len(plain) == 6 and all(LINE.match(ln) for ln in plain[:3]), plain
    assert plain[3].startswith('Mean runtime:') and plain[4].startswith('CRMSD median/mean/std: ') \
        and plain[5].startswith('IRMSD median/mean/std: ')
    assert len(with_q) == 8, with_q
    dq = []
    for ln, base in zip(with_q[:3], plain[:3]):
        m = DOCKQ.match(ln)
        # the line as it is today (the two runs write to out1 and out0), plus the appended fields
        assert m and m.group(1).replace(str(tmp_path / 'out1'), str(tmp_path / 'out0')) == base, (ln, base)
        r = want[LINE.match(base).group(1)]
        assert m.group(2) == f"{r['dockq']:.3f}" and m.group(3) == f"{r['fnat']:.3f}" and m.group(4) == f"{r['lrmsd']:.3f}" \
            and m.group(5) == f"{r['irmsd_backbone']:.3f}" and int(m.group(6)) == r['clashes'], (ln, r)
        dq.append(r['dockq'])
    assert with_q[3].startswith('Mean runtime:') and with_q[4:6] == plain[4:6]
    dq = np.asarray(dq)
    assert with_q[6] == "DockQ median/mean/std: %.3f / %.3f / %.3f" % (np.median(dq), np.mean(dq), np.std(dq)), with_q[6]
    assert with_q[7] == "CAPRI classes (DockQ): incorrect %d  acceptable %d  medium %d  high %d" % (
        (dq < 0.23).sum(), ((dq >= 0.23) & (dq < 0.49)).sum(), ((dq >= 0.49) & (dq < 0.80)).sum(), (dq >= 0.80).sum()), with_q[7]
    # a missing ground truth is an error with the flag
    (gt / 'BIGL_l_b_COMPLEX.pdb').unlink()
    p = subprocess.run(cmd, cwd=dc.ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and 'BIGL_l_b_COMPLEX.pdb' in p.stderr
