"""Bit comparison of the two bodies of the backward node chain: k_rowchain (EQD_CHAIN_RESIDENT_BWD=0) and the
resident-weights body k_rowchain_res_bwd (unset / 1; csrc/eqd_chainres_bwd_inl.h), the forward resident body on in both.
The resident body runs the same MFMA sequence per output element, the same source and chunk order, the same epilogue
expressions and chain_lnbwd64's LayerNorm backward, so every output, every saved layer state and the flat gradient must be
EQUAL, not close.  Shared by tests/test_chain_resident_bwd_sim.py and tests/test_chain_resident_bwd_gpu.py.

Which chains: eqd_model_backward launches one chain per layer.  With cross messages and the published widths (layer 0 is
69 wide, every later layer 64) the last layer's chain is the five-job form, layers L-2 .. 1 are the six-job form and layer
0's chain is not eligible: a model of L layers launches the new body L - 1 times per backward - 0 for one layer, 1 (the
five-job form alone) for two, 2 (the six-job form added) for three.

What the simulator cannot see: it copies at issue time, so a missing or too-small vmcnt wait shows up only on the GPU - as
bits that differ from k_rowchain's or between replays (the GPU file compares replays of one captured step as well)."""
import ctypes as C

import torch

from equidock_public_amd import _lib as L
from equidock_public_amd import graph as G
from equidock_public_amd import synthetic
from oracle import iegmn_port as port
from tests import chain_resident_common as cr
from tests import node_chain_common as nc
from tests import parity_common as pc
from tests.util import load_case, pairs_from_raw, state_dict_for

SWITCH = 'EQD_CHAIN_RESIDENT_BWD'


def bwd_launches():
    fn = pc.lib().eqd_chain_resident_bwd_launches
    fn.restype = C.c_longlong
    fn.argtypes = []
    return int(fn())


def expected_launches(args):
    """launches of the new body in one backward of the model `args` describes, at a batch of no more tiles than CUs"""
    if not args['cross_msgs'] or args.get('hip_storage_dtype') == 'bf16':
        return 0
    return int(args['iegmn_n_lays']) - (1 if args['use_mean_node_features'] else 0)


def one_step(dev, args, sd, pairs, dropout):
    """chain_resident_common.one_step plus the new body's launches of the step"""
    before = bwd_launches()
    outs, states, flat, fwd = cr.one_step(dev, args, sd, pairs, dropout)
    return outs, states, flat, fwd, bwd_launches() - before


def launches_of_a_step(dev, args, sd, pairs):
    """the new body's launches of one training step, without reading the layer states (bf16 storage does not keep them)"""
    net = pc.build_model(args, sd, dev)
    net.train(True)
    g = G.batch_pairs(pairs).to(dev)
    before = bwd_launches()
    port.scalar_loss(net(g, epoch=0)).backward()
    pc.sync(dev)
    return bwd_launches() - before


def set_switch(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)
    L.reload_tunables()


def check_bodies_agree(dev, monkeypatch, args, sd, pairs, what, dropouts=(0.0, 0.25)):
    monkeypatch.delenv('EQD_CHAIN_RESIDENT', raising=False)
    want = expected_launches(args)
    assert want > 0, f'{what}: no eligible chain in this model'
    for dropout in dropouts:
        res = {}
        for mode in ('0', '1'):
            set_switch(monkeypatch, SWITCH, mode)
            res[mode] = one_step(dev, args, sd, pairs, dropout)
        set_switch(monkeypatch, SWITCH, None)
        w = f'{what}, dropout {dropout}'
        assert res['0'][3] > 0 and res['0'][3] == res['1'][3], f'{w}: the forward resident body ran {res["0"][3]} / {res["1"][3]} times'
        assert res['0'][4] == 0, f'{w}: {SWITCH}=0 launched the resident body {res["0"][4]} times'
        # every 64-wide layer's chain (five jobs: the last layer, six jobs: the others) and never layer 0's 69-wide one
        assert res['1'][4] == want, f'{w}: the resident body ran {res["1"][4]} times, expected {want}'
        for a, b in zip(res['0'][0], res['1'][0]):
            assert torch.equal(a, b), f'{w}: outputs differ (max {float((a - b).abs().max()):.3e})'
        for l, ((h0, x0), (h1, x1)) in enumerate(zip(res['0'][1], res['1'][1])):
            assert torch.equal(h0, h1), f'{w}: h after layer {l} differs (max {float((h0 - h1).abs().max()):.3e})'
            assert torch.equal(x0, x1), f'{w}: x after layer {l} differs'
        g0, g1 = res['0'][2], res['1'][2]
        assert torch.equal(g0, g1), f'{w}: gradients differ (max {float((g0 - g1).abs().max()):.3e} of {float(g0.abs().max()):.3e})'


def check_golden_case(dev, monkeypatch, name):
    z, meta, args, raw = load_case(name)
    check_bodies_agree(dev, monkeypatch, args, state_dict_for(meta, args), pairs_from_raw(raw), name)


def three_layers(dev):
    args = port.default_args(iegmn_n_lays=3, skip_weight_h=0.75, device=torch.device(dev))
    return args, port.init_state_dict(args, seed=4, rot_scale=10.0)


# rows: 65, 79, 97 (n % 16 in {1, 15}: chain_resident_common.check_ragged_tiles), 15 (less than one tile), 48 (whole tiles)
SIZES = ([(33, 32)], [(40, 39)], [(17, 20), (30, 30)], [(7, 8)], [(24, 24)])


def check_sizes(dev, monkeypatch, sizes):
    args, sd = three_layers(dev)
    n = sum(a + b for a, b in sizes)
    check_bodies_agree(dev, monkeypatch, args, sd, synthetic.make_pairs(sizes, 13), f'{n} rows')


def check_forms_counted(dev, monkeypatch):
    """one layer: no eligible chain; two: the five-job form alone; three: the six-job form as well"""
    monkeypatch.delenv('EQD_CHAIN_RESIDENT', raising=False)
    set_switch(monkeypatch, SWITCH, None)
    pairs = synthetic.make_pairs([(21, 20)], 13)
    for layers in (1, 2, 3):
        args = port.default_args(iegmn_n_lays=layers, skip_weight_h=0.75, device=torch.device(dev))
        got = launches_of_a_step(dev, args, port.init_state_dict(args, seed=4, rot_scale=10.0), pairs)
        assert got == layers - 1 == expected_launches(args), (layers, got)


def check_not_eligible(dev, monkeypatch, many_tiles=True):
    """every condition that keeps a backward chain on k_rowchain (or k_rowres): the new counter does not move.
    many_tiles: include the batch of more tiles than CUs (a minute on the simulator for a comparison of two host integers
    that is the same code in both builds: the GPU file runs it)"""
    monkeypatch.delenv('EQD_CHAIN_RESIDENT', raising=False)
    set_switch(monkeypatch, SWITCH, None)
    small = synthetic.make_pairs([(21, 20), (30, 18)], 13)

    def launches(over, pairs, env=None):
        for k, v in (env or {}).items():
            set_switch(monkeypatch, k, v)
        args = port.default_args(**dict(dict(iegmn_n_lays=3, skip_weight_h=0.75, device=torch.device(dev)), **over))
        n = launches_of_a_step(dev, args, port.init_state_dict(args, seed=4, rot_scale=10.0), pairs)
        for k in (env or {}):
            set_switch(monkeypatch, k, None)
        return n
    assert launches({}, small) == 2      # (the same model and batch with nothing in the way)
    assert launches(dict(cross_msgs=False), small) == 0
    assert launches(dict(hip_storage_dtype='bf16'), small) == 0
    # 4 112 rows: 257 tiles on 256 CUs (two layers and short receptors: the smallest step that has an eligible list there)
    if many_tiles:
        many = synthetic.make_pairs([(250, 7)] * 16, 13)
        assert launches(dict(iegmn_n_lays=2), many) == 0
    assert launches({}, small, {'EQD_ROW_TILES': '2'}) == 0
    assert launches({}, small, {'EQD_ROWCHAIN_OCC': '1'}) == 0
    # the operator entry point at 64 x 64: four column blocks (d_h0 at full width, d_h last, with the skip residual) - with
    # and without cross messages (without: a five-job list, but its blocks are not adjacent and the last has a residual)
    for cross in (True, False):
        cfg = dict(d=64, d0=64, ldc=64, cross=cross, s=0.75)
        before = bwd_launches()
        nc.run_kernels(dev, nc.make_case(cfg, 50), False)
        assert bwd_launches() == before, f'eqd_node_update_bwd (cross={cross}) selected the resident backward body'


# ---- one chain on guarded buffers (eqd_selftest_node_chain_bwd) ----------------------------------------------------------


class EqdNodeChainBwdTest(C.Structure):
    _fields_ = [('rows', C.c_int32), ('with_dh', C.c_int32), ('d0', C.c_int32), ('skip_weight_h', C.c_float),
                ('slope', C.c_float), ('ln_eps', C.c_float), ('dh_X', C.c_void_p * 6), ('dh_W', C.c_void_p * 6),
                ('dh_wcs', C.c_int32 * 6), ('dH_above', C.c_void_p), ('dH', C.c_void_p), ('Wn2', C.c_void_p),
                ('Wn1', C.c_void_p), ('y_act', C.c_void_p), ('ln_g', C.c_void_p), ('drop_mul', C.c_void_p),
                ('dz', C.c_void_p), ('ln_part', C.c_void_p), ('d_aggr_msg', C.c_void_p), ('d_aggr_cross', C.c_void_p),
                ('dh0acc', C.c_void_p)]


def run_guarded_chain(dev, with_dh, rows=37, d0=69, seed=7):
    """One chain of the model driver's list on NaN-filled outputs with sentinel rows behind every buffer.  Returns the
    outputs (bodies only) after the guards, the untouched parts and the written parts have been checked."""
    gen = torch.Generator().manual_seed(seed)
    nan, tiles, ldn = float('nan'), (rows + 15) // 16, d0 + 192

    def src(cols, scale=0.5):      # a source: read up to the clamped last row, never written; sentinel rows behind it
        t = nc._guarded(dev, rows, cols, 0.0)
        t[:rows] = (torch.randn(rows, cols, generator=gen) * scale).to(dev)
        return t
    mk = lambda *sh: (torch.randn(*sh, generator=gen) * 0.3).to(dev).contiguous()      # noqa: E731
    X = [src(64) for _ in range(6)]
    # the weights as the model holds them: Wn1 [64][ldn], W1 [64][128] (two sources), Wq / Wk / Wv [64][64]
    Wn1, W1, Wq, Wk, Wv, Wn2 = mk(64, ldn), mk(64, 128), mk(64, 64), mk(64, 64), mk(64, 64), mk(64, 64)
    dh_W = [(Wn1, 0, ldn), (W1, 0, 128), (W1, 64, 128), (Wq, 0, 64), (Wk, 0, 64), (Wv, 0, 64)]
    above, y_act = src(64), src(64, 1.0)
    mul = nc._guarded(dev, rows, 64, 0.0)
    mul[:rows] = ((torch.rand(rows, 64, generator=gen) >= 0.25).float() / 0.75).to(dev)
    mul[rows - 1] = 0.0      # a row whose dropout factors are all zero, inside the ragged tile
    ln_g = (1.0 + 0.2 * torch.randn(64, generator=gen)).to(dev)
    acc0 = (torch.randn(rows, 64, generator=gen) * 0.5).to(dev)
    out = dict(dH=nc._guarded(dev, rows, 64, nan), dz=nc._guarded(dev, rows, 64, nan), ln_part=nc._guarded(dev, tiles, 256, nan),
               d_aggr_msg=nc._guarded(dev, rows, 64, nan), d_aggr_cross=nc._guarded(dev, rows, 64, nan),
               dh0acc=nc._guarded(dev, rows, d0, nan))
    if with_dh:
        out['dh0acc'][:rows, :64] = acc0      # the accumulator of the layers above
    inputs = X + [above, y_act, mul]
    before = [t.clone() for t in inputs]
    t = EqdNodeChainBwdTest()
    t.rows, t.with_dh, t.d0, t.skip_weight_h, t.slope, t.ln_eps = rows, int(with_dh), d0, 0.75, nc.SLOPE, nc.EPS
    for s in range(6):
        t.dh_X[s] = X[s].data_ptr()
        t.dh_W[s] = dh_W[s][0].data_ptr() + 4 * dh_W[s][1]
        t.dh_wcs[s] = dh_W[s][2]
    t.dH_above, t.dH, t.Wn2, t.Wn1 = above.data_ptr(), out['dH'].data_ptr(), Wn2.data_ptr(), Wn1.data_ptr()
    t.y_act, t.ln_g, t.drop_mul = y_act.data_ptr(), ln_g.data_ptr(), mul.data_ptr()
    for k in ('dz', 'ln_part', 'd_aggr_msg', 'd_aggr_cross', 'dh0acc'):
        setattr(t, k, out[k].data_ptr())
    nb = C.c_int(0)
    fn = pc.lib().eqd_selftest_node_chain_bwd
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.check(fn(C.byref(t), C.byref(nb), pc.st(dev)))
    pc.sync(dev)
    assert nb.value == tiles, (nb.value, tiles)
    for a, b in zip(inputs, before):
        assert torch.equal(a, b), 'a source buffer (or the guard behind it) was written'
    got = {}
    for k, v in out.items():
        n = tiles if k == 'ln_part' else rows
        assert bool((v[n:] == nc.SENTINEL).all()), f'{k}: the guard rows behind the buffer were written'
        got[k] = v[:n].cpu()
    for k in ('dz', 'd_aggr_msg', 'd_aggr_cross') + (('dH',) if with_dh else ()):
        assert bool(torch.isfinite(got[k]).all()), f'{k}: not every element was written'
    if not with_dh:
        assert bool(torch.isnan(got['dH']).all()), 'dH was written by the five-job chain'
    assert bool(torch.isfinite(got['dh0acc'][:, :64]).all()) and bool(torch.isnan(got['dh0acc'][:, 64:]).all()), \
        'dh0acc: the 64 embedding columns are written, the trailing feature columns are not'
    lp = got['ln_part']
    assert bool(torch.isfinite(lp[:, :64]).all()) and bool(torch.isfinite(lp[:, 128:192]).all()), 'ln_part: d gamma / d beta not written'
    assert bool(torch.isnan(lp[:, 64:128]).all()) and bool(torch.isnan(lp[:, 192:]).all()), 'ln_part: columns beyond 64 features written'
    assert bool((got['dz'][rows - 1] == 0).all()), 'dz of the row with all-zero dropout factors'
    return got


def check_guard_rows(dev, monkeypatch):
    monkeypatch.delenv('EQD_CHAIN_RESIDENT', raising=False)
    for with_dh in (True, False):
        res = {}
        for mode in ('0', '1'):
            set_switch(monkeypatch, SWITCH, mode)
            before = bwd_launches()
            res[mode] = run_guarded_chain(dev, with_dh)
            assert bwd_launches() - before == int(mode), f'{SWITCH}={mode}, with_dh={with_dh}: which body ran'
        set_switch(monkeypatch, SWITCH, None)
        for k in res['0']:
            a, b = res['0'][k], res['1'][k]
            same = torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0))
            assert same, f'with_dh={with_dh}: {k} differs between the bodies'
