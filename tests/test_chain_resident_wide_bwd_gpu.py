"""GPU tests (-m gpu): the wide resident body of the first layer's backward node chain (k_rowchain_res_bwd_wide,
csrc/eqd_chainres_bwd_wide_inl.h) computes the bits of k_rowchain's general body on an MI355X, and computes the same bits
every time.  Its operands arrive by 49 asynchronous LDS copies per wave that only counted waits order against the fragment
reads: a missing or too-small wait reads stale LDS - bits that differ from k_rowchain's, or from one replay of a step to
the next.  Both are compared here."""
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
    from tests import chain_resident_wide_bwd_common as cwb
    cwb.check_golden_case(dev, monkeypatch, name)


def _ids(s):
    return '%d_rows' % sum(a + b for a, b in s)


@pytest.mark.parametrize('layers', (2, 3))
@pytest.mark.parametrize('sizes', [[(7, 8)], [(24, 24)], [(33, 32)], [(40, 39)], [(17, 20), (30, 30)]], ids=_ids)
def test_sizes_and_depths_bit_equal(dev, sizes, layers, monkeypatch):
    from tests import chain_resident_wide_bwd_common as cwb
    assert sizes in list(cwb.SIZES) and layers in cwb.LAYERS
    cwb.check_sizes(dev, monkeypatch, sizes, layers)      # dropout 0 and 0.25


def test_counters(dev, monkeypatch):
    from tests import chain_resident_wide_bwd_common as cwb
    cwb.check_counted(dev, monkeypatch)


def test_not_eligible_stays_on_the_general_bodies(dev, monkeypatch):
    from tests import chain_resident_wide_bwd_common as cwb
    cwb.check_not_eligible(dev, monkeypatch)


def test_guard_rows_and_float64_formulas(dev, monkeypatch):
    from tests import chain_resident_wide_bwd_common as cwb
    cwb.check_guard_rows(dev, monkeypatch)


def test_replays_of_a_captured_step_are_bit_equal(dev, monkeypatch):
    """a training step of one pair (40, 39) - 79 rows, 15 in the last tile - three layers, captured into a hipGraph as
    bench.py captures it; five replays give the same outputs and the same flat gradient, and those are the bits of the
    eager EQD_CHAIN_RESIDENT_WIDE_BWD=0 run of the same step"""
    from equidock_public_amd import graph, losses, model, parallel, synthetic
    from tests import chain_resident_wide_bwd_common as cwb
    monkeypatch.delenv('EQD_CHAIN_RESIDENT', raising=False)
    args, sd = cwb.model_of(dev, 3)
    pairs = synthetic.make_pairs([(40, 39)], 13)
    got = {}
    for mode in ('0', None):
        cwb.set_switch(monkeypatch, cwb.SWITCH, mode)
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

        def snapshot():
            return {k: v.detach().clone() for k, v in last.items()} | {'grad': reducer.flat.clone()}
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        before = cwb.wide_bwd_launches()
        with torch.cuda.stream(side):
            for _ in range(3):
                compute()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        assert cwb.wide_bwd_launches() - before == (0 if mode == '0' else 3)
        if mode == '0':      # the eager run on the general body
            got[mode] = snapshot()
            continue
        before = cwb.wide_bwd_launches()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, capture_error_mode='thread_local'):
            compute()
        assert cwb.wide_bwd_launches() - before == 1
        runs = []
        for _ in range(5):
            gr.replay()
            torch.cuda.synchronize()
            runs.append(snapshot())
        assert float(runs[0]['grad'].abs().max()) > 0
        for r, run in enumerate(runs[1:], 1):
            for k in run:
                assert torch.equal(run[k], runs[0][k]), f'replay {r} differs from replay 0 in {k}'
        got[mode] = runs[0]
        del gr
    cwb.set_switch(monkeypatch, cwb.SWITCH, None)
    for k in got['0']:
        assert torch.equal(got['0'][k], got[None][k]), f'{k}: the two bodies differ (max {float((got["0"][k] - got[None][k]).abs().max()):.3e})'
