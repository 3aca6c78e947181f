"""GPU tests (-m gpu) of the batched solvent-accessible surface (SASA, buried surface area, buried atoms and residues):
libequidock_dock.so on a real MI355X through equidock_public_amd.dock (the shared checks live in
tests/dock_surface_common.py), dock_complexes(surface=True) and the command line's --surface."""
import numpy as np
import pytest
import torch

from tests import dock_common as dc
from tests import dock_surface_common as sc

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


def test_abi_and_validation_errors(dev):
    sc.check_validation_errors(dev)


def test_real_complexes_in_one_batch(dev):
    sc.check_real(dev)


def test_tile_chunk_segment_and_point_count_edges(dev):
    sc.check_edges(dev)


def test_degenerate_sets(dev):
    sc.check_degenerate(dev)


def test_all_partners_switch_gives_the_same_bits(dev, monkeypatch):
    sc.check_all_partners_switch(dev, monkeypatch)


def test_bits_alone_first_last_permuted_and_run_to_run(dev):
    sc.check_bits(dev)


def _plan_and_inputs(dev, names):
    from equidock_public_amd import dock as DK
    cases = [sc.all_cases()[n] for n in names]
    plan = DK.SurfacePlan([c[4] for c in cases], [c[5] for c in cases], [c[2] for c in cases], [c[3] for c in cases], dev)
    return cases, plan, [sc._t(c[0], dev) for c in cases], [sc._t(c[1], dev) for c in cases]


def test_surface_area_batch_never_synchronises_or_downloads(dev, monkeypatch):
    """8. with a plan (its init has copied the item table): no Tensor.cpu, no stream or device synchronisation inside
    surface_area_batch; without one, the only wait is the init's own, inside the library"""
    from equidock_public_amd import dock as DK
    cases, plan, ligs, recs = _plan_and_inputs(dev, ('1HCF_native', 'edge_1x1', 'edge_65x257', 'far_ligand'))
    tables = ([c[2] for c in cases], [c[3] for c in cases], [c[4] for c in cases], [c[5] for c in cases])
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
    with_plan = DK.surface_area_batch(ligs, recs, plan=plan)
    again = DK.surface_area_batch(ligs, recs, plan=plan)
    fresh = DK.surface_area_batch(ligs, recs, *tables)
    assert calls == {'cpu': 0, 'sync': 0}, calls
    monkeypatch.undo()
    assert with_plan['plan'] is plan and fresh['plan'] is not plan
    for k in ('rows', 'lig_points', 'rec_points', 'lig_res_area', 'rec_res_area'):
        a = with_plan[k].cpu().numpy().tobytes()
        assert a == again[k].cpu().numpy().tobytes() == fresh[k].cpu().numpy().tobytes(), k
    for got, c in zip(sc.run(dev, cases), range(len(cases))):
        assert got['row'].tobytes() == with_plan['rows'][c].cpu().numpy().tobytes()


def test_surface_pass_is_capturable(dev):
    """8. eval neither synchronises, allocates nor copies: ONE capture on a single stream and one replay on new coordinates
    give the bits of the host-enqueued pass"""
    cases, plan, ligs, recs = _plan_and_inputs(dev, ('1AVX_EQUIDOCK', 'edge_63x255'))
    lig, rec = torch.cat(ligs), torch.cat(recs)
    native = torch.cat([sc._t(sc.all_cases()['1AVX_native'][0], dev), ligs[1]])
    want = plan.outputs()
    plan.eval(lig, rec, *want)
    out = plan.outputs()
    for t in out:
        t.zero_()
    buf = native.clone()                                # (captured on the native ligand, replayed on the docked one)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        plan.eval(buf, rec, *out)
    torch.cuda.current_stream(dev).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.eval(buf, rec, *out)
    buf.copy_(lig)
    g.replay()
    torch.cuda.synchronize(dev)
    for a, b in zip(out, want):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert float(want[2][0, 3]) > 0.0


def test_dock_complexes_with_surface(dev):
    sc.check_dock_complexes_surface(dev, ('graph_case', 'graph_case_pair300'), max_it=20, check_every=10)


def test_command_line_surface(dev, tmp_path, capsys):
    sc.check_command_line(dev, tmp_path, capsys, ('graph_case', 'graph_case_tiny'), max_it=20)
