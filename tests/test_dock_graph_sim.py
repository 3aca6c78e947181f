"""CPU tests of batched graph construction: csrc_dock/ and csrc/ compiled for x86 against the host simulator and driven
through equidock_public_amd.dock.protein_graphs_batch / dock_complexes, as on the GPU; plus the resource check of the
shipped gfx950 code object."""
import pytest
import torch

from equidock_public_amd import _lib, dock as DK
from tests import dock_common as dc, dock_graph_common as gc

DEV = torch.device('cpu')


@pytest.fixture(scope='module', autouse=True)
def simulators():
    from tests.hostsim import build as hs
    DK.load_dock_library_for_testing(dc.build_sim())
    _lib.load_library_for_testing(hs.build())
    assert DK._dock_is_sim and _lib.is_simulator()
    yield
    _lib.unload_for_testing()
    DK.unload_dock_for_testing()


def test_reference_graphs_in_one_batch():
    gc.check_reference_graphs(DEV, gc.SIM_CASES)


def test_bit_equal_to_the_per_protein_path():
    gc.check_against_per_protein(DEV, gc.SIM_CASES)


def test_composition_and_run_to_run_bits():
    gc.check_composition(DEV, gc.SIM_CASES)


@pytest.mark.parametrize('name, expect_pruned', [('graph_case_pair300', True), ('graph_case_tiny', False)])
def test_pruning_changes_no_bit(name, expect_pruned, monkeypatch):
    gc.check_pruning(DEV, name, expect_pruned, monkeypatch)


def test_residue_of_more_than_64_atoms():
    assert gc.check_long_residue(DEV) > 64


def test_errors():
    gc.check_errors(DEV)


def test_dock_complexes_batched_and_looped_graphs_agree():
    gc.check_pipeline(DEV, ('graph_case', 'graph_case_tiny'))


def test_command_line_flag():
    """--no-batched-graphs parses; without it the batched path is the default (checked without running a model)"""
    import inspect
    assert inspect.signature(DK.dock_complexes).parameters['batched_graphs'].default is True
    assert DK.main(['--checkpoint', '/nonexistent.pth', '--input-dir', '/nonexistent', '--gt-dir', '/nonexistent',
                    '--out-dir', '/nonexistent', '--no-batched-graphs']) == 1      # reaches the missing input directory


def test_graph_kernels_use_no_scratch():
    """8. the new kernels in the shipped libequidock_dock.so report zero scratch"""
    from equidock_public_amd import build as hip_build
    from tests.test_abi_and_graph import _gfx950_kernel_notes
    notes = [(n, f) for n, f in _gfx950_kernel_notes(hip_build.build_dock(verbose=False)) if 'k_dg_' in n]
    found = {k for k in ('k_dg_centroids', 'k_dg_distances', 'k_dg_select', 'k_dg_scan', 'k_dg_edges') if any(k in n for n, _ in notes)}
    assert len(found) == 5, found
    bad = [(n, f['private_segment_fixed_size']) for n, f in notes
           if int(f['private_segment_fixed_size']) != 0 or f.get('uses_dynamic_stack') == 'true']
    assert not bad, bad
