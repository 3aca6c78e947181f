"""GPU tests (-m gpu) of the batched residue depth: libequidock_dock.so on a real MI355X through
equidock_public_amd.dock (the shared checks live in tests/dock_depth_common.py), surface_feature_analysis,
dock_complexes(depth=True) and the command line's --depth."""
import pytest
import torch

from tests import dock_depth_common as pc

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
    pc.check_validation_errors(dev)


def test_real_poses_in_one_batch(dev):
    pc.check_real(dev)


def test_tile_word_and_residue_edges(dev):
    pc.check_edges(dev)


def test_degenerate_sets(dev):
    pc.check_degenerate(dev)


def test_pruning_switch_changes_only_the_skipped_count(dev, monkeypatch):
    pc.check_pruning_switch(dev, monkeypatch)


def test_bits_alone_first_last_permuted_and_run_to_run(dev):
    pc.check_bits(dev)


def _plan_and_inputs(dev, names):
    from equidock_public_amd import dock as DK
    cases = [pc.all_cases()[n] for n in names]
    plan = DK.DepthPlan([c[4] for c in cases], [c[5] for c in cases], [c[2] for c in cases], [c[3] for c in cases], dev,
                        lig_names=[c[6] for c in cases], rec_names=[c[7] for c in cases])
    return cases, plan, [pc._t(c[0], dev) for c in cases], [pc._t(c[1], dev) for c in cases]


def test_depth_batch_never_synchronises_or_downloads(dev, monkeypatch):
    """with a plan (its init has copied the tile table): no Tensor.cpu, no stream or device synchronisation inside
    residue_depth_batch; without one, the only wait is the init's own, inside the library"""
    from equidock_public_amd import dock as DK
    cases, plan, ligs, recs = _plan_and_inputs(dev, ('1HCF_EQUIDOCK', 'edge_1x1', 'edge_65x257', 'far_sides'))
    tables = dict(lig_radii=[c[2] for c in cases], rec_radii=[c[3] for c in cases], lig_res_offsets=[c[4] for c in cases],
                  rec_res_offsets=[c[5] for c in cases], lig_names=[c[6] for c in cases], rec_names=[c[7] for c in cases])
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
    with_plan = DK.residue_depth_batch(ligs, recs, plan=plan)
    again = DK.residue_depth_batch(ligs, recs, plan=plan)
    fresh = DK.residue_depth_batch(ligs, recs, **tables)
    assert calls == {'cpu': 0, 'sync': 0}, calls
    monkeypatch.undo()
    assert with_plan['plan'] is plan and fresh['plan'] is not plan
    for k in ('rows', 'lig_depth', 'rec_depth', 'lig_res_depth', 'rec_res_depth'):
        a = with_plan[k].cpu().numpy().tobytes()
        assert a == again[k].cpu().numpy().tobytes() == fresh[k].cpu().numpy().tobytes(), k
    for c, got in enumerate(pc.run(dev, cases)):
        assert got['row'].tobytes() == with_plan['rows'][c].cpu().numpy().tobytes()


def test_depth_pass_is_capturable(dev):
    """eval neither synchronises, allocates nor copies: ONE capture on a side stream and one replay on new coordinates
    give the bytes of the host-enqueued pass"""
    cases, plan, ligs, recs = _plan_and_inputs(dev, ('1AVX_EQUIDOCK', 'edge_63x255'))
    native = pc.all_cases()['1AVX_native']
    lig, rec = torch.cat(ligs), torch.cat(recs)
    want = plan.outputs()
    plan.eval(lig, rec, *want)
    out = plan.outputs()
    for t in out:
        t.zero_()
    buf = torch.cat([pc._t(native[0], dev), ligs[1]])   # (captured on the native pose, replayed on the docked one)
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
    assert float(want[2][0, 8]) > 0 and float(want[2][0, 13]) > 0


def test_surface_feature_analysis(dev):
    pc.check_surface_feature_analysis(dev)


def test_surface_analysis_command_line(dev, tmp_path, capsys):
    pc.check_surface_analysis_command_line(dev, tmp_path, capsys)


def test_dock_complexes_with_depth(dev):
    pc.check_dock_complexes_depth(dev, ('graph_case', 'graph_case_pair300'), max_it=20, check_every=10)


def test_command_line_depth(dev, tmp_path, capsys):
    pc.check_command_line(dev, tmp_path, capsys, ('graph_case', 'graph_case_tiny'), max_it=20)
