"""GPU tests (-m gpu) of batched docking inference: libequidock_dock.so on a real MI355X through
equidock_public_amd.dock - reference trajectories, batch invariance, agreement with the single-complex clash removal,
dock_complexes against the single-complex pipeline, and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import dock_common as dc

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


def test_reference_trajectories_in_one_batch(dev):
    """inference_case a, b, c with per-complex caps, plus the atoms of two real complexes (graph_case, 240 x 836;
    graph_case_pair300, 2 060 x 2 305) in the same batch"""
    extra = [dc.fixture_atoms('graph_case') + (60,), dc.fixture_atoms('graph_case_pair300') + (60,)]
    dc.check_reference_trajectories(dev, extra=extra)


def test_batch_invariance_and_run_to_run_bits(dev):
    z = np.load(os.path.join(dc.GOLDEN, 'inference_case.npz'))
    complexes = [(z['b_lig'], z['b_rec']), dc.fixture_atoms('graph_case_pair300'), dc.fixture_atoms('graph_case_big'),
                 (z['a_lig'], z['a_rec']), dc.fixture_atoms('graph_case')]
    out = dc.check_batch_invariance(dev, complexes, caps=[1300, 40, 30, 300, 50], runs=2)
    assert out[0]['iterations'] < 1300          # b converges and stops on its own while the others run on


def test_agrees_with_single_complex_remove_clashes(dev):
    """the same 300 iterations as inference.remove_clashes (eqd_clash_iterations) on the atoms of the real complexes:
    reordered sums, positions within 1e-4 of the largest coordinate (loss_stop = -1: every complex runs all 300)"""
    from equidock_public_amd import dock as DK, inference as INF
    ligs, recs = [], []
    for name in dc.REAL:
        lig, rec = dc.fixture_atoms(name)
        ligs.append(torch.from_numpy(lig).to(dev))
        recs.append(torch.from_numpy(rec).to(dev))
    batch = DK.remove_clashes_batch(ligs, recs, loss_stop=-1.0, max_it=300, check_every=100)
    for name, lig, rec, b in zip(dc.REAL, ligs, recs, batch):
        s = INF.remove_clashes(lig, rec, loss_stop=-1.0, max_it=300, check_every=100)
        assert b['iterations'] == s['iterations'] == 300
        dc.close(b['positions'], s['positions'], 1e-4, f'{name}: batched vs single-complex clash removal')
        assert abs(b['loss'] - s['loss']) <= 1e-4 * max(1.0, abs(s['loss'])), (name, b['loss'], s['loss'])


def test_dock_complexes_matches_the_single_complex_pipeline(dev):
    from equidock_public_amd import dock as DK, inference as INF
    from equidock_public_amd import featurize as FZ
    net, _, _ = dc.seeded_net(dev)
    residues = [dc.fixture_residues(n) for n in dc.REAL]
    res = DK.dock_complexes(net, residues, remove_clashes=True, max_it=20, check_every=10)
    assert len(res) == 3 and res[0]['batch_seconds']['n_complexes'] == 3
    status = net.iegmn_original.last_svd_status                 # the scaled keypoint projections: the guard stays silent
    assert int(status.abs().sum()) == 0, status
    for name, (lig_res, rec_res), r in zip(dc.REAL, residues, res):
        R, t = dc.single_complex_pipeline(net, lig_res, rec_res, dev)
        dc.close(r['rotation'], R, 1e-4, f'{name}: rotation, batched vs single forward')
        dc.close(r['translation'], t, 1e-4, f'{name}: translation, batched vs single forward')
        atoms = torch.from_numpy(FZ.atoms_ragged(lig_res)[0]).to(dev)
        dc.close(r['ligand_atoms_docked'], INF.apply_rigid(torch.from_numpy(r['rotation']), torch.from_numpy(r['translation']),
                                                           atoms), 1e-5, f'{name}: docked ligand atoms vs apply_rigid')
        assert 1 <= r['clash_iterations'] <= 20 and r['ligand_atoms'].shape == atoms.shape
        assert torch.isfinite(r['ligand_atoms']).all()


def test_command_line(dev, tmp_path):
    """python -m equidock_public_amd.dock on PDB files written from the fixtures, with a torch.save'd {'args',
    'state_dict'} checkpoint: outputs named as the reference names them, coordinates = the API's within PDB rounding,
    the summary lines"""
    from equidock_public_amd import dock as DK, inference as INF
    net, args, sd = dc.seeded_net(dev)
    ckpt = tmp_path / 'db5_model_best.pth'
    torch.save({'args': dict(args, device=torch.device('cpu'), graph_cutoff=30.0, graph_max_neighbor=10,
                             pocket_cutoff=8.0, intersection_loss_weight=10.0), 'state_dict': sd}, ckpt)
    inp, gt, out = tmp_path / 'in', tmp_path / 'gt', tmp_path / 'out'
    inp.mkdir()
    gt.mkdir()
    names = ['GCAS', 'P300', 'BIGL']
    for nm, fx in zip(names, dc.REAL):
        lig, rec = dc.fixture_residues(fx)
        dc.write_pdb(lig, inp / f'{nm}_l_b.pdb')
        dc.write_pdb(lig, gt / f'{nm}_l_b_COMPLEX.pdb')
        dc.write_pdb(rec, gt / f'{nm}_r_b_COMPLEX.pdb')
    cmd = [sys.executable, '-m', 'equidock_public_amd.dock', '--checkpoint', str(ckpt), '--input-dir', str(inp),
           '--gt-dir', str(gt), '--out-dir', str(out), '--remove-clashes', '--batch', '2', '--max-it', '20']
    p = subprocess.run(cmd, cwd=dc.ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert 'Mean runtime:' in p.stdout and 'CRMSD median/mean/std' in p.stdout and 'IRMSD median/mean/std' in p.stdout, p.stdout
    api = DK.dock_complexes(DK.load_checkpoint(str(ckpt), dev),
                            [(str(inp / f'{nm}_l_b.pdb'), str(gt / f'{nm}_r_b_COMPLEX.pdb')) for nm in sorted(names)],
                            max_complexes_per_batch=2, max_it=20)
    for nm, r in zip(sorted(names), api):
        f = out / f'{nm}_l_b_EQUIDOCK_NO_CLASHES.pdb'
        assert f.is_file(), sorted(os.listdir(out))
        got = INF.read_pdb_atoms(str(f))
        assert got.shape == tuple(r['ligand_atoms'].shape)
        assert float(np.abs(got - r['ligand_atoms'].cpu().numpy()).max()) <= 1e-3, nm
    # a missing receptor is an error: non-zero exit
    os.remove(gt / 'BIGL_r_b_COMPLEX.pdb')
    p = subprocess.run(cmd, cwd=dc.ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and 'BIGL_r_b_COMPLEX.pdb' in p.stderr
