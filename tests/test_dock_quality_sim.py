"""CPU tests of the batched docking quality (fnat, LRMSD, backbone iRMSD, DockQ, clashes): csrc_dock/ compiled for x86
against the host simulator and driven through equidock_public_amd.dock, as on the GPU (the shared checks live in
tests/dock_quality_common.py)."""
import pytest
import torch

from equidock_public_amd import dock as DK
from tests import dock_common as dc
from tests import dock_quality_common as qc

DEV = torch.device('cpu')


@pytest.fixture(scope='module', autouse=True)
def simulator():
    DK.load_dock_library_for_testing(dc.build_sim())
    assert DK._dock_is_sim
    yield
    DK.unload_dock_for_testing()


def test_abi():
    lib = DK.load_dock_library()
    assert lib.eqd_dock_quality_abi() == DK.DOCK_QUALITY_ABI == 1 and DK.QUALITY_COLS == 16
    assert lib.eqd_dock_abi_version() == 1 and lib.eqd_dock_meter_abi() == 1 and lib.eqd_dock_graph_abi() == 1


def test_yardstick_reproduces_the_recorded_table():
    qc.check_yardstick_reproduces_the_table()


def test_atom_table(tmp_path):
    qc.check_atom_table(tmp_path)


def test_real_complexes_in_one_batch():
    qc.check_real(DEV)


def test_near_native_poses():
    qc.check_near_native(DEV)


def test_tile_chunk_and_staging_edges():
    qc.check_edges(DEV)


def test_degenerate_sets():
    qc.check_degenerate(DEV)


def test_bits_alone_first_last_permuted_and_run_to_run():
    qc.check_bits(DEV)


def test_pruning_changes_no_other_column(monkeypatch):
    qc.check_pruning(DEV, monkeypatch)


def test_validation_errors():
    qc.check_validation_errors(DEV)


def test_command_line_flag():
    """--dockq parses (checked without running a model): the call reaches the missing input directory"""
    assert DK.main(['--checkpoint', '/nonexistent.pth', '--input-dir', '/nonexistent', '--gt-dir', '/nonexistent',
                    '--out-dir', '/nonexistent', '--dockq']) == 1


def test_quality_kernels_use_no_scratch():
    """11. the new kernels in the shipped libequidock_dock.so report zero scratch"""
    from equidock_public_amd import build as hip_build
    from tests.test_abi_and_graph import _gfx950_kernel_notes
    notes = [(n, f) for n, f in _gfx950_kernel_notes(hip_build.build_dock(verbose=False)) if 'k_dq_' in n]
    kernels = ('k_dq_bounds', 'k_dq_pairs', 'k_dq_moments', 'k_dq_solve', 'k_dq_residuals', 'k_dq_finish')
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


def test_dock_complexes_with_quality(model_simulator):
    qc.check_dock_complexes_quality(DEV, ('graph_case', 'graph_case_tiny'), max_it=5, check_every=2)
