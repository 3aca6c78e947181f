"""GPU tests (-m gpu): the half-tile edge-forward body of the fused small-batch launch (k_edge_attn_fwd_half,
csrc/eqd_edge_fwd_half_inl.h) computes the bytes of the whole-tile body on an MI355X, and the same bytes every time.  The
two waves of a pair meet at one workgroup barrier between their message rows and the membership product; a half that read
the other's rows too early, or a feature tile overwritten while its owner still reads it, shows as bytes that differ from
k_edge_attn_fwd's or from one replay to the next.  Both are compared here."""
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


@pytest.mark.parametrize('drop', (False, True), ids=('plain', 'dropout'))
@pytest.mark.parametrize('name', ['full_tile', 'mixed', 'single_tile'])
def test_tile_shapes_byte_equal(dev, name, drop, monkeypatch):
    from tests import edge_half_common as eh
    assert sorted(eh.GRAPHS) == ['full_tile', 'mixed', 'single_tile']
    eh.check_graph(dev, monkeypatch, name, drop)


def test_not_eligible_stays_on_the_whole_tile_kernels(dev, monkeypatch):
    from tests import edge_half_common as eh
    eh.check_not_eligible(dev, monkeypatch)


@pytest.mark.parametrize('name', ['B_b3_dips8', 'D_degraded3'])
def test_golden_cases_bit_equal(dev, name, monkeypatch):
    from tests import edge_half_common as eh
    eh.check_golden_case(dev, monkeypatch, name)


def test_counters(dev, monkeypatch):
    from tests import edge_half_common as eh
    eh.check_counted(dev, monkeypatch)


def test_ten_replays_of_a_captured_launch_are_byte_equal(dev, monkeypatch):
    """the launch on the `mixed` graph with dropout masks, captured into a hipGraph: ten replays into re-poisoned buffers give
    the bytes of the eager EQD_EDGE_FWD_HALF=0 launch"""
    import ctypes as C
    from equidock_public_amd import _lib as L
    from tests import edge_half_common as eh
    from tests import parity_common as pc
    monkeypatch.delenv('EQD_FUSE_FWD', raising=False)
    g, pk, gs = eh.graph_of(dev, 'mixed')
    host, d, ep, fz, fc = eh.edge_inputs(dev, pk, drop=True)
    eh.set_switch(monkeypatch, eh.SWITCH, '0')
    ref, n = eh.run_launch(dev, gs, pk, d, ep)
    assert n == 0
    eh.set_switch(monkeypatch, eh.SWITCH, None)
    N = pk.n_nodes
    bufs = {k: eh.framed(N * w, dev) for k, w in zip(eh.OUTPUTS, (64, 3, 64, 1))}
    fn = pc.lib().eqd_selftest_edge_attn_fwd
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] * 7 + [C.c_int] + [C.c_void_p] * 6
    P = pc.P

    def launch():
        L.check(fn(C.byref(gs), C.byref(ep), P(d['Pn']), P(d['Qn']), P(d['x']), P(bufs['aggr_msg'][1]), P(bufs['x_new'][1]), 64,
                   P(d['q']), P(d['k']), P(d['v']), P(bufs['att_out'][1]), P(bufs['lse'][1]), pc.st(dev)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    before = eh.launches()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, capture_error_mode='thread_local'):
        launch()
    assert eh.launches() - before == 1
    for r in range(10):
        for whole, body in bufs.values():
            body.fill_(float('nan'))
        gr.replay()
        torch.cuda.synchronize()
        got = {}
        for k, (whole, body) in bufs.items():
            assert bool((whole[:eh.GUARD] == eh.SENTINEL).all()) and bool((whole[-eh.GUARD:] == eh.SENTINEL).all()), k
            got[k] = body
        eh.same_bytes(ref, got, f'replay {r}')
    del gr
