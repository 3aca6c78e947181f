"""CPU tests of the batched lDDT and interface lDDT: csrc_dock/ compiled for x86 against the host simulator and driven
through equidock_public_amd.dock, as on the GPU (the shared checks live in tests/dock_lddt_common.py)."""
import pytest
import torch

from equidock_public_amd import dock as DK
from tests import dock_common as dc
from tests import dock_lddt_common as lc

DEV = torch.device('cpu')


@pytest.fixture(scope='module', autouse=True)
def simulator():
    DK.load_dock_library_for_testing(dc.build_sim())
    assert DK._dock_is_sim
    yield
    DK.unload_dock_for_testing()


def test_abi_and_validation_errors():
    lc.check_validation_errors(DEV)


def test_yardstick_reproduces_the_recorded_table():
    lc.check_yardstick_reproduces_the_table()


def test_real_poses_in_one_batch():
    lc.check_real(DEV)


def test_block_stage_and_residue_edges():
    lc.check_edges(DEV)


def test_degenerate_sets():
    lc.check_degenerate(DEV)


def test_pruning_switch_changes_only_the_skipped_count(monkeypatch):
    lc.check_pruning_switch(DEV, monkeypatch)


def test_bits_alone_first_last_permuted_and_run_to_run():
    lc.check_bits(DEV)


def test_command_line_flag():
    """--lddt parses (checked without running a model): the call reaches the missing input directory"""
    assert DK.main(['--checkpoint', '/nonexistent.pth', '--input-dir', '/nonexistent', '--gt-dir', '/nonexistent',
                    '--out-dir', '/nonexistent', '--lddt']) == 1


def test_lddt_kernels_use_no_scratch():
    """the new kernels in the shipped libequidock_dock.so report zero scratch"""
    from equidock_public_amd import build as hip_build
    from tests.test_abi_and_graph import _gfx950_kernel_notes
    notes = [(n, f) for n, f in _gfx950_kernel_notes(hip_build.build_dock(verbose=False)) if 'k_ld_' in n]
    kernels = ('k_ld_bounds', 'k_ld_pairs', 'k_ld_residues', 'k_ld_finish')
    found = {k for k in kernels if any(k in n for n, _ in notes)}
    assert len(found) == len(kernels), found
    bad = [(n, f['private_segment_fixed_size']) for n, f in notes
           if int(f['private_segment_fixed_size']) != 0 or f.get('uses_dynamic_stack') == 'true']
    assert not bad, bad


@pytest.fixture
def model_simulator():
    from equidock_public_amd import _lib
    from tests.hostsim import build as hs
    _lib.load_library_for_testing(hs.build())
    yield
    _lib.unload_for_testing()


def test_dock_complexes_with_lddt(model_simulator):
    lc.check_dock_complexes_lddt(DEV, ('graph_case', 'graph_case_tiny'), max_it=5, check_every=2)


def test_command_line_lddt(model_simulator, tmp_path, capsys):
    lc.check_command_line(DEV, tmp_path, capsys, ('graph_case', 'graph_case_tiny'))
