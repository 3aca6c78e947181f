"""GPU tests (-m gpu): the carrying forms of the resident forward node chain (k_rowchain_res_fwd<5> / <1>,
csrc/eqd_chainres_inl.h) compute the bits of the two-job body followed by the projections' own launches on an MI355X, and
compute the same bits every time.  The carried jobs' weights arrive by asynchronous LDS copies into slots the wave has just
read, ordered against the fragment reads by counted waits only, and every global store of the launch is held back behind
the last of those waits: a missing or too-small wait reads stale LDS - bits that differ from the separate launches', or from
one replay of a step to the next.  Both are compared here."""
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
    from tests import chain_resident_proj_common as crp
    crp.check_golden_case(dev, monkeypatch, name)


def _ids(s):
    return '%d_rows' % sum(a + b for a, b in s)


@pytest.mark.parametrize('layers', [2, 3, 4])
@pytest.mark.parametrize('sizes', [[(7, 8)], [(24, 24)], [(33, 32)], [(40, 39)], [(17, 20), (30, 30)]], ids=_ids)
def test_sizes_and_depths_bit_equal(dev, sizes, layers, monkeypatch):
    from tests import chain_resident_proj_common as crp
    assert sizes in list(crp.SIZES) and layers in crp.LAYERS
    crp.check_sizes(dev, monkeypatch, sizes, layers)


def test_carrying_forms_are_counted_and_replace_k_linear_launches(dev, monkeypatch):
    from tests import chain_resident_proj_common as crp
    crp.check_forms_counted(dev, monkeypatch)


def test_not_eligible_keeps_the_separate_launches(dev, monkeypatch):
    from tests import chain_resident_proj_common as crp
    crp.check_not_eligible(dev, monkeypatch)


def test_guard_rows_and_clamped_source_rows(dev, monkeypatch):
    from tests import chain_resident_proj_common as crp
    crp.check_guard_rows(dev, monkeypatch)


def test_training_step_run_to_run_bits(dev, monkeypatch):
    """five eager runs of the same seeded fp32 training step at the DB5.5 batch size with dropout 0.25, carrying forms on"""
    from tests import chain_resident_proj_common as crp
    from tests import parity_common as pc
    monkeypatch.delenv('EQD_CHAIN_RESIDENT', raising=False)
    crp.set_switch(monkeypatch, crp.SWITCH, '1')
    before = crp.proj_launches()
    pc.check_run_to_run_bits(dev, cases=((False, 0.25, 8, 8, 200),), runs=5)
    assert crp.proj_launches() - before == 5 * 7      # layers 1 .. 7 of the eight, per forward
    crp.set_switch(monkeypatch, crp.SWITCH, None)


def _capture_and_replay(dev, monkeypatch, training):
    """workload B captured into a hipGraph as bench.py captures it (training: the step; else the forward alone, no state
    kept); five replays give the same bits, and those are the bits of the EQD_CHAIN_RESIDENT_PROJ=0 capture"""
    from equidock_public_amd import graph, losses, model, parallel
    from tests import chain_resident_common as cr
    from tests import chain_resident_proj_common as crp
    monkeypatch.delenv('EQD_CHAIN_RESIDENT', raising=False)
    args, sd, pairs = cr.workload_b(dev)
    got = {}
    for mode in ('0', '1'):
        crp.set_switch(monkeypatch, crp.SWITCH, mode)
        net = model.Rigid_Body_Docking_Net(args).to(dev)
        net.load_state_dict(sd)
        net.train(training)
        g = graph.batch_pairs(pairs).to(dev)
        packed = g.pack()
        reducer = parallel.FlatGradAllReduce(net) if training else None
        scalar_loss = losses.ScalarLoss(packed, args['num_att_heads']) if training else None
        last = {}

        def compute():
            if training:
                reducer.zero()
                lig, Yl, Yr, T, b = net.forward_batched(g)
                loss, grads = scalar_loss(lig, Yl, Yr)
                torch.autograd.backward([lig, Yl, Yr], list(grads))
                last.update(loss=loss, lig=lig, Yl=Yl, Yr=Yr, T=T, b=b)
            else:
                with torch.no_grad():
                    lig, Yl, Yr, T, b = net.forward_batched(g)
                last.update(lig=lig, Yl=Yl, Yr=Yr, T=T, b=b)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                compute()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        before = crp.proj_launches()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, capture_error_mode='thread_local'):
            compute()
        assert crp.proj_launches() - before == (7 if mode == '1' else 0)      # layers 1 .. 7 of the eight
        runs = []
        for _ in range(5):
            gr.replay()
            torch.cuda.synchronize()
            runs.append({k: v.detach().clone() for k, v in last.items()} | ({'grad': reducer.flat.clone()} if training else {}))
        if training:
            assert float(runs[0]['grad'].abs().max()) > 0
        for r, run in enumerate(runs[1:], 1):
            for k in run:
                assert torch.equal(run[k], runs[0][k]), f'{crp.SWITCH}={mode}: replay {r} differs from replay 0 in {k}'
        got[mode] = runs[0]
        del gr
    crp.set_switch(monkeypatch, crp.SWITCH, None)
    for k in got['0']:
        assert torch.equal(got['0'][k], got['1'][k]), f'{k}: the two forms differ (max {float((got["0"][k] - got["1"][k]).abs().max()):.3e})'


def test_replays_of_a_captured_step_are_bit_equal(dev, monkeypatch):
    _capture_and_replay(dev, monkeypatch, True)


def test_replays_of_a_captured_inference_forward_are_bit_equal(dev, monkeypatch):
    _capture_and_replay(dev, monkeypatch, False)
