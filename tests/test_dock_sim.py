"""CPU tests of batched clash removal: csrc_dock/ compiled for x86 against the host simulator (tests/dock_common.py
builds it into a library of its own) and driven through equidock_public_amd.dock, as on the GPU."""
import numpy as np
import pytest
import torch

from equidock_public_amd import dock as DK
from tests import dock_common as dc

DEV = torch.device('cpu')


@pytest.fixture(scope='module', autouse=True)
def simulator():
    DK.load_dock_library_for_testing(dc.build_sim())
    assert DK._dock_is_sim
    yield
    DK.unload_dock_for_testing()


def test_reference_trajectories_in_one_batch():
    """inference_case a, b, c batched with per-complex caps against the reference's own trajectories"""
    dc.check_reference_trajectories(DEV)


def test_batch_invariance_bits():
    """alone vs batched vs reversed: bit-identical; one complex has > 256 ligand and > 1 024 receptor atoms (several row
    tiles and partner chunks on both sides)"""
    z = np.load(dc.GOLDEN + '/inference_case.npz')
    lig3, rec3 = dc.fixture_atoms('graph_case_pair300')                  # 2 060 x 2 305
    complexes = [(z['b_lig'], z['b_rec']), (lig3, rec3), (z['a_lig'], z['a_rec'])]
    out = dc.check_batch_invariance(DEV, complexes, caps=[40, 2, 25])
    assert [r['iterations'] for r in out] == [40, 2, 25]


def test_host_side_validation():
    dc.check_validation_errors(DEV)


def test_dock_complexes_on_the_simulators():
    """dock_complexes end to end with both libraries' simulator builds (two small real complexes): one batched forward
    gives each complex the (R, t) of its own single-complex forward, the docked atoms are apply_rigid of them"""
    from equidock_public_amd import _lib, featurize as FZ, inference as INF
    from tests.hostsim import build as hs
    _lib.load_library_for_testing(hs.build())
    try:
        net, _, _ = dc.seeded_net(DEV)
        names = ('graph_case', 'graph_case_tiny')
        residues = [dc.fixture_residues(n) for n in names]
        res = DK.dock_complexes(net, residues, remove_clashes=True, max_it=5, check_every=2, device=DEV)
        for name, (lig_res, rec_res), r in zip(names, residues, res):
            R, t = dc.single_complex_pipeline(net, lig_res, rec_res, DEV)
            dc.close(r['rotation'], R, 1e-4, f'{name}: rotation')
            dc.close(r['translation'], t, 1e-4, f'{name}: translation')
            atoms = torch.from_numpy(FZ.atoms_ragged(lig_res)[0])
            dc.close(r['ligand_atoms_docked'], INF.apply_rigid(torch.from_numpy(r['rotation']),
                                                               torch.from_numpy(r['translation']), atoms), 1e-5, name)
            assert 1 <= r['clash_iterations'] <= 5 and r['ligand_atoms'].shape == atoms.shape
    finally:
        _lib.unload_for_testing()
