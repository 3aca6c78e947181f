"""GPU tests (-m gpu) of batched graph construction: eqd_dock_graph_* of libequidock_dock.so on a real MI355X through
equidock_public_amd.dock.protein_graphs_batch / dock_complexes, against the reference's recorded graphs and, bit for
bit, against the per-protein path (featurize.protein_graph, libequidock_hip.so)."""
import pytest
import torch

from tests import dock_graph_common as gc

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


def test_reference_graphs_in_one_batch(dev):
    out = gc.check_reference_graphs(dev, gc.GPU_CASES)
    assert all(g[k].is_cuda for g in out for k in gc.KEYS)


def test_bit_equal_to_the_per_protein_path(dev):
    gc.check_against_per_protein(dev, gc.GPU_CASES)


def test_composition_and_run_to_run_bits(dev):
    gc.check_composition(dev, gc.GPU_CASES)
    gc.check_composition(dev, gc.GPU_CASES, target='graph_case_big/rec')


@pytest.mark.parametrize('name, expect_pruned', [('graph_case_pair300', True), ('graph_case_big', True),
                                                 ('graph_case_tiny', False)])
def test_pruning_changes_no_bit(dev, name, expect_pruned, monkeypatch):
    gc.check_pruning(dev, name, expect_pruned, monkeypatch)


def test_residue_of_more_than_64_atoms(dev):
    assert gc.check_long_residue(dev) > 64


def test_errors(dev):
    from equidock_public_amd import _lib
    gc.check_errors(dev)
    lig = gc.fixture_proteins(['graph_case'])[0]
    with pytest.raises(_lib.EquidockHipError, match='is on cpu'):
        gc.batch_of([lig], torch.device('cpu'))


def test_two_synchronisations_whatever_the_batch(dev, monkeypatch):
    """the call reads the device twice: the counts (Tensor.cpu) and the outputs (one stream synchronise behind the
    non-blocking copies into pinned host buffers) - for 2 proteins as for 8"""
    prots = gc.fixture_proteins(gc.GPU_CASES)
    calls = {'cpu': 0, 'sync': 0}
    real_cpu, real_sync = torch.Tensor.cpu, torch.cuda.Stream.synchronize

    def cpu(self, *a, **k):
        calls['cpu'] += int(self.is_cuda)
        return real_cpu(self, *a, **k)

    def sync(self):
        calls['sync'] += 1
        return real_sync(self)

    for batch in (prots[:2], prots):
        gc.batch_of(batch, dev)          # warm: pinned blocks, workspace
        monkeypatch.setattr(torch.Tensor, 'cpu', cpu)
        monkeypatch.setattr(torch.cuda.Stream, 'synchronize', sync)
        calls.update(cpu=0, sync=0)
        out = gc.batch_of(batch, dev)
        monkeypatch.undo()
        assert calls == {'cpu': 1, 'sync': 1}, (len(batch), calls)
        assert all(out[0]['host'][k].flags['C_CONTIGUOUS'] or out[0]['host'][k].size == 0 for k in gc.KEYS)


def test_dock_complexes_batched_and_looped_graphs_agree(dev):
    from tests import dock_common as dc
    res = gc.check_pipeline(dev, dc.REAL, max_it=20, check_every=10)
    assert res[0]['batch_seconds']['n_complexes'] == 3
