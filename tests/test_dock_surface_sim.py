"""CPU tests of the batched solvent-accessible surface (SASA, buried surface area, buried atoms and residues): csrc_dock/
compiled for x86 against the host simulator and driven through equidock_public_amd.dock, as on the GPU (the shared checks
live in tests/dock_surface_common.py)."""
import pytest
import torch

from equidock_public_amd import dock as DK
from tests import dock_common as dc
from tests import dock_surface_common as sc

DEV = torch.device('cpu')


@pytest.fixture(scope='module', autouse=True)
def simulator():
    DK.load_dock_library_for_testing(dc.build_sim())
    assert DK._dock_is_sim
    yield
    DK.unload_dock_for_testing()


def test_abi_and_validation_errors():
    sc.check_validation_errors(DEV)


def test_yardstick_reproduces_the_recorded_table():
    sc.check_yardstick_reproduces_the_table()


def test_sphere_points_and_atom_radii(tmp_path):
    sc.check_sphere_and_radii(tmp_path)


def test_real_complexes_in_one_batch():
    sc.check_real(DEV)


def test_tile_chunk_segment_and_point_count_edges():
    sc.check_edges(DEV)


def test_degenerate_sets():
    sc.check_degenerate(DEV)


def test_all_partners_switch_gives_the_same_bits(monkeypatch):
    sc.check_all_partners_switch(DEV, monkeypatch)


def test_bits_alone_first_last_permuted_and_run_to_run():
    sc.check_bits(DEV)


def test_command_line_flag():
    """--surface parses (checked without running a model): the call reaches the missing input directory"""
    assert DK.main(['--checkpoint', '/nonexistent.pth', '--input-dir', '/nonexistent', '--gt-dir', '/nonexistent',
                    '--out-dir', '/nonexistent', '--surface']) == 1


def test_surface_kernels_use_no_scratch():
    """10. the new kernels in the shipped libequidock_dock.so report zero scratch"""
    from equidock_public_amd import build as hip_build
    from tests.test_abi_and_graph import _gfx950_kernel_notes
    notes = [(n, f) for n, f in _gfx950_kernel_notes(hip_build.build_dock(verbose=False)) if 'k_sa_' in n]
    kernels = ('k_sa_lists', 'k_sa_points', 'k_sa_residues', 'k_sa_finish')
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


def test_dock_complexes_with_surface(model_simulator):
    sc.check_dock_complexes_surface(DEV, ('graph_case', 'graph_case_tiny'), max_it=5, check_every=2)


def test_command_line_surface(model_simulator, tmp_path, capsys):
    sc.check_command_line(DEV, tmp_path, capsys, ('graph_case', 'graph_case_tiny'))
