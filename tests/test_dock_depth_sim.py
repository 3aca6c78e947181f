"""CPU tests of the batched residue depth: csrc_dock/ compiled for x86 against the host simulator and driven through
equidock_public_amd.dock, as on the GPU (the shared checks live in tests/dock_depth_common.py)."""
import pytest
import torch

from equidock_public_amd import dock as DK
from tests import dock_common as dc
from tests import dock_depth_common as pc

DEV = torch.device('cpu')


@pytest.fixture(scope='module', autouse=True)
def simulator():
    DK.load_dock_library_for_testing(dc.build_sim())
    assert DK._dock_is_sim
    yield
    DK.unload_dock_for_testing()


def test_abi_and_validation_errors():
    pc.check_validation_errors(DEV)


def test_yardstick_reproduces_the_recorded_figures():
    pc.check_yardstick_reproduces_the_issue()


def test_real_poses_in_one_batch():
    pc.check_real(DEV)


def test_tile_word_and_residue_edges():
    pc.check_edges(DEV)


def test_degenerate_sets():
    pc.check_degenerate(DEV)


def test_pruning_switch_changes_only_the_skipped_count(monkeypatch):
    pc.check_pruning_switch(DEV, monkeypatch)


def test_bits_alone_first_last_permuted_and_run_to_run():
    pc.check_bits(DEV)


def test_spearman():
    pc.check_spearman()


def test_command_line_flag():
    """--depth parses (checked without running a model): the call reaches the missing input directory"""
    assert DK.main(['--checkpoint', '/nonexistent.pth', '--input-dir', '/nonexistent', '--gt-dir', '/nonexistent',
                    '--out-dir', '/nonexistent', '--depth']) == 1


def test_depth_kernels_use_no_scratch():
    """the new kernels in the shipped libequidock_dock.so report zero scratch and no dynamic stack"""
    from equidock_public_amd import build as hip_build
    from tests.test_abi_and_graph import _gfx950_kernel_notes
    notes = [(n, f) for n, f in _gfx950_kernel_notes(hip_build.build_dock(verbose=False)) if 'k_dp_' in n]
    kernels = ('k_dp_masks', 'k_dp_tiles', 'k_dp_search', 'k_dp_residues', 'k_dp_finish')
    found = {k for k in kernels if any(k in n for n, _ in notes)}
    assert len(found) == len(kernels), found
    bad = [(n, f['private_segment_fixed_size']) for n, f in notes
           if int(f['private_segment_fixed_size']) != 0 or f.get('uses_dynamic_stack') == 'true']
    assert not bad, bad


def test_surface_feature_analysis():
    pc.check_surface_feature_analysis(DEV)


def test_surface_analysis_command_line(tmp_path, capsys):
    pc.check_surface_analysis_command_line(DEV, tmp_path, capsys)


@pytest.fixture
def model_simulator():
    from equidock_public_amd import _lib
    from tests.hostsim import build as hs
    _lib.load_library_for_testing(hs.build())
    yield
    _lib.unload_for_testing()


def test_dock_complexes_with_depth(model_simulator):
    pc.check_dock_complexes_depth(DEV, ('graph_case', 'graph_case_tiny'), max_it=5, check_every=2)


def test_command_line_depth(model_simulator, tmp_path, capsys):
    pc.check_command_line(DEV, tmp_path, capsys, ('graph_case', 'graph_case_tiny'))
