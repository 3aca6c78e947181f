"""GPU tests (-m gpu) of the batched lDDT and interface lDDT: libequidock_dock.so on a real MI355X through
equidock_public_amd.dock (the shared checks live in tests/dock_lddt_common.py), dock_complexes(lddt=True) and the command
line's --lddt."""
import pytest
import torch

from tests import dock_lddt_common as lc

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
    lc.check_validation_errors(dev)


def test_real_poses_in_one_batch(dev):
    lc.check_yardstick_reproduces_the_table()
    lc.check_real(dev)


def test_block_stage_and_residue_edges(dev):
    lc.check_edges(dev)


def test_degenerate_sets(dev):
    lc.check_degenerate(dev)


def test_pruning_switch_changes_only_the_skipped_count(dev, monkeypatch):
    lc.check_pruning_switch(dev, monkeypatch)


def test_bits_alone_first_last_permuted_and_run_to_run(dev):
    lc.check_bits(dev)


def _plan_and_inputs(dev, names):
    from equidock_public_amd import dock as DK
    cases = [lc.all_cases()[n] for n in names]
    plan = DK.LddtPlan([c[4] for c in cases], [c[5] for c in cases], dev)
    return (cases, plan, [lc._t(c[0], dev) for c in cases], [lc._t(c[2], dev) for c in cases],
            [lc._t(c[3], dev) for c in cases])


def test_lddt_batch_never_synchronises_or_downloads(dev, monkeypatch):
    """with a plan (its init has copied the item table): no Tensor.cpu, no stream or device synchronisation inside
    lddt_batch; without one, the only wait is the init's own, inside the library"""
    from equidock_public_amd import dock as DK
    cases, plan, ligs_p, ligs_t, recs_t = _plan_and_inputs(dev, ('1HCF EquiDock', 'edge_1x1', 'edge_65x513', 'far_sides'))
    tables = ([c[4] for c in cases], [c[5] for c in cases])
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
    with_plan = DK.lddt_batch(ligs_p, ligs_t, recs_t, plan=plan)
    again = DK.lddt_batch(ligs_p, ligs_t, recs_t, plan=plan)
    fresh = DK.lddt_batch(ligs_p, ligs_t, recs_t, *tables)
    assert calls == {'cpu': 0, 'sync': 0}, calls
    monkeypatch.undo()
    assert with_plan['plan'] is plan and fresh['plan'] is not plan
    for k in ('rows', 'lig_counts', 'rec_counts', 'lig_res_lddt', 'rec_res_lddt'):
        a = with_plan[k].cpu().numpy().tobytes()
        assert a == again[k].cpu().numpy().tobytes() == fresh[k].cpu().numpy().tobytes(), k
    for c, got in enumerate(lc.run(dev, cases)):
        assert got['row'].tobytes() == with_plan['rows'][c].cpu().numpy().tobytes()


def test_lddt_pass_is_capturable(dev):
    """eval neither synchronises, allocates nor copies: ONE capture on a side stream and one replay on new coordinates
    give the bits of the host-enqueued pass"""
    cases, plan, ligs_p, ligs_t, recs_t = _plan_and_inputs(dev, ('1AVX EquiDock', 'edge_63x511'))
    lig_p, lig_t, rec_t = torch.cat(ligs_p), torch.cat(ligs_t), torch.cat(recs_t)
    want = plan.outputs()
    plan.eval(lig_p, None, lig_t, rec_t, *want)
    out = plan.outputs()
    for t in out:
        t.zero_()
    buf = lig_t.clone()                                 # (captured on the native as model, replayed on the docked pose)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        plan.eval(buf, None, lig_t, rec_t, *out)
    torch.cuda.current_stream(dev).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.eval(buf, None, lig_t, rec_t, *out)
    buf.copy_(lig_p)
    g.replay()
    torch.cuda.synchronize(dev)
    for a, b in zip(out, want):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert 0.0 < float(want[2][0, 1]) < 1.0


def test_dock_complexes_with_lddt(dev):
    lc.check_dock_complexes_lddt(dev, ('graph_case', 'graph_case_pair300'), max_it=20, check_every=10)


def test_command_line_lddt(dev, tmp_path, capsys):
    lc.check_command_line(dev, tmp_path, capsys, ('graph_case', 'graph_case_tiny'), max_it=20)
