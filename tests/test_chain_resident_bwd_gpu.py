"""GPU tests (-m gpu): the resident-weights body of the backward node chain (k_rowchain_res_bwd,
csrc/eqd_chainres_bwd_inl.h) computes the bits of k_rowchain on an MI355X, and computes the same bits every time.  Its
weights and rows arrive by asynchronous LDS copies - four slabs are refilled while the chain runs - that only counted waits
order against the fragment reads: a missing or too-small wait reads stale LDS - bits that differ from k_rowchain's, or
from one replay of a step to the next.  Both are compared here."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from equidock_public_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.unload_for_testing()
    _lib.load_library()
    assert not _lib.is_simulator(), "GPU tests must run the real gfx950 library"
    return torch.device('cuda:0')


@pytest.mark.parametrize('name', ['B_b3_dips8', 'D_degraded3'])
def test_golden_cases_bit_equal(dev, name, monkeypatch):
    from tests import chain_resident_bwd_common as crb
    crb.check_golden_case(dev, monkeypatch, name)


def _ids(s):
    return '%d_rows' % sum(a + b for a, b in s)


@pytest.mark.parametrize('sizes', [[(33, 32)], [(40, 39)], [(17, 20), (30, 30)], [(7, 8)], [(24, 24)]], ids=_ids)
def test_three_layers_bit_equal(dev, sizes, monkeypatch):
    from tests import chain_resident_bwd_common as crb
    assert sizes in list(crb.SIZES)
    crb.check_sizes(dev, monkeypatch, sizes)


def test_five_and_six_job_forms_are_counted(dev, monkeypatch):
    from tests import chain_resident_bwd_common as crb
    crb.check_forms_counted(dev, monkeypatch)


def test_not_eligible_stays_on_the_general_bodies(dev, monkeypatch):
    from tests import chain_resident_bwd_common as crb
    crb.check_not_eligible(dev, monkeypatch)


def test_guard_rows_and_clamped_source_rows(dev, monkeypatch):
    from tests import chain_resident_bwd_common as crb
    crb.check_guard_rows(dev, monkeypatch)


def test_training_step_run_to_run_bits(dev, monkeypatch):
    """five runs of the same seeded fp32 training step at the DB5.5 batch size with dropout 0.25, resident bodies on"""
    from tests import chain_resident_bwd_common as crb
    from tests import parity_common as pc
    monkeypatch.delenv('EQD_CHAIN_RESIDENT', raising=False)
    crb.set_switch(monkeypatch, crb.SWITCH, '1')
    before = crb.bwd_launches()
    pc.check_run_to_run_bits(dev, cases=((False, 0.25, 8, 8, 200),), runs=5)
    assert crb.bwd_launches() - before == 5 * 7
    crb.set_switch(monkeypatch, crb.SWITCH, None)


def test_replays_of_a_captured_step_are_bit_equal(dev, monkeypatch):
    """workload B's step captured into a hipGraph as bench.py captures it; five replays give the same outputs and the same
    flat gradient, and those are the bits of the EQD_CHAIN_RESIDENT_BWD=0 capture of the same graph"""
    from equidock_public_amd import graph, losses, model, parallel
    from tests import chain_resident_bwd_common as crb
    from tests import chain_resident_common as cr
    monkeypatch.delenv('EQD_CHAIN_RESIDENT', raising=False)
    args, sd, pairs = cr.workload_b(dev)
    got = {}
    for mode in ('0', '1'):
        crb.set_switch(monkeypatch, crb.SWITCH, mode)
        net = model.Rigid_Body_Docking_Net(args).to(dev)
        net.load_state_dict(sd)
        net.train(True)
        g = graph.batch_pairs(pairs).to(dev)
        packed = g.pack()
        reducer = parallel.FlatGradAllReduce(net)
        scalar_loss = losses.ScalarLoss(packed, args['num_att_heads'])
        last = {}

        def compute():
            reducer.zero()
            lig, Yl, Yr, T, b = net.forward_batched(g)
            loss, grads = scalar_loss(lig, Yl, Yr)
            torch.autograd.backward([lig, Yl, Yr], list(grads))
            last.update(loss=loss, lig=lig, Yl=Yl, Yr=Yr, T=T, b=b)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                compute()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        before = crb.bwd_launches()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, capture_error_mode='thread_local'):
            compute()
        assert crb.bwd_launches() - before == (7 if mode == '1' else 0)      # layers 7 .. 1 of the eight
        runs = []
        for _ in range(5):
            gr.replay()
            torch.cuda.synchronize()
            runs.append({k: v.detach().clone() for k, v in last.items()} | {'grad': reducer.flat.clone()})
        assert float(runs[0]['grad'].abs().max()) > 0
        for r, run in enumerate(runs[1:], 1):
            for k in run:
                assert torch.equal(run[k], runs[0][k]), f'{crb.SWITCH}={mode}: replay {r} differs from replay 0 in {k}'
        got[mode] = runs[0]
        del gr
    crb.set_switch(monkeypatch, crb.SWITCH, None)
    for k in got['0']:
        assert torch.equal(got['0'][k], got['1'][k]), f'{k}: the two bodies differ (max {float((got["0"][k] - got["1"][k]).abs().max()):.3e})'
