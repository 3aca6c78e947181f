"""Bit comparison of the two bodies of the FIRST layer's backward node chain: k_rowchain's general body
(EQD_CHAIN_RESIDENT_WIDE_BWD=0) and the wide resident body k_rowchain_res_bwd_wide (unset / 1;
csrc/eqd_chainres_bwd_wide_inl.h), every other resident body on in both.  The wide body runs, per output element, the MFMA
sequence of the path each of the six jobs takes in k_rowchain (the lean path for the 64-wide outputs, the general path for
the 69-wide ones: the full chunk, then the zero-padded 16-deep step), its accumulator sets and epilogue expressions, and
chain_lnbwd<1>'s LayerNorm backward in its reduction order: every output, every saved layer state and the flat gradient
must be EQUAL, not close.  Shared by tests/test_chain_resident_wide_bwd_sim.py and tests/test_chain_resident_wide_bwd_gpu.py.

Which chains: layer 0's backward chain of a model with >= 2 layers, cross messages, fp32, one 16-row tile per workgroup and
no more tiles than CUs: one launch per training step.  A one-layer model (the five-job form) stays on k_rowchain.  The four
older counters move as before.

What the simulator cannot see: it copies at issue time, so a missing or too-small vmcnt wait shows up only on the GPU - as
bits that differ or that change between replays (the GPU file compares replays of one captured step as well)."""
import ctypes as C

import torch

from equidock_public_amd import _lib as L
from equidock_public_amd import synthetic
from tests import chain_resident_proj_common as crp
from tests import chain_resident_wide_common as crw
from tests import node_chain_common as nc
from tests import parity_common as pc
from tests.util import load_case, pairs_from_raw, state_dict_for

SWITCH = 'EQD_CHAIN_RESIDENT_WIDE_BWD'
set_switch = crp.set_switch
model_of = crp.model_of
# rows: 15 (less than one tile), 48 (whole tiles), 65, 79 (1 and 15 rows in the last tile), 97 (two segments, ragged)
SIZES = crp.SIZES
LAYERS = (2, 3)


def wide_bwd_launches():
    fn = pc.lib().eqd_chain_resident_wide_bwd_launches
    fn.restype = C.c_longlong
    fn.argtypes = []
    return int(fn())


def counters():
    """(the new counter, then the four older ones: wide forward, resident forward, carrying forms, 64-wide backward)"""
    return (wide_bwd_launches(),) + crw.counters()


def expected(args):
    """launches of the new body in one training step of the model `args` describes, at a batch of no more tiles than CUs"""
    if not args['cross_msgs'] or args.get('hip_storage_dtype') == 'bf16':
        return 0
    return 1 if int(args['iegmn_n_lays']) >= 2 else 0


def one_step(dev, args, sd, pairs, dropout):
    """chain_resident_proj_common.one_step plus what the five counters moved by during the whole step"""
    before = counters()
    res = crp.one_step(dev, args, sd, pairs, dropout)
    res['counters'] = tuple(a - b for a, b in zip(counters(), before))
    return res


def check_bodies_agree(dev, monkeypatch, args, sd, pairs, what, dropouts=(0.0, 0.25), formula=False):
    monkeypatch.delenv('EQD_CHAIN_RESIDENT', raising=False)
    for dropout in dropouts:
        res = {}
        for mode in ('0', None):
            set_switch(monkeypatch, SWITCH, mode)
            res[mode] = one_step(dev, args, sd, pairs, dropout)
        set_switch(monkeypatch, SWITCH, None)
        w = f'{what}, dropout {dropout}'
        assert res['0']['counters'][0] == 0, f'{w}: {SWITCH}=0 launched the wide backward body {res["0"]["counters"][0]} times'
        assert res[None]['counters'][0] == expected(args), f'{w}: the wide backward body ran {res[None]["counters"][0]} times'
        assert res['0']['counters'][1:] == res[None]['counters'][1:], f'{w}: {res["0"]["counters"]} / {res[None]["counters"]}'
        if formula:
            assert res[None]['counters'][1:] == (1,) + crw.old_counters(args), f'{w}: the older counters moved by {res[None]["counters"][1:]}'
        crp.assert_same_bits(res['0'], res[None], w)


def check_golden_case(dev, monkeypatch, name):
    z, meta, args, raw = load_case(name)
    check_bodies_agree(dev, monkeypatch, args, state_dict_for(meta, args), pairs_from_raw(raw), name)


def check_sizes(dev, monkeypatch, sizes, layers, dropouts=(0.0, 0.25)):
    args, sd = model_of(dev, layers)
    assert expected(args) == 1
    check_bodies_agree(dev, monkeypatch, args, sd, synthetic.make_pairs(sizes, 13), f'{crp.rows_of(sizes)} rows, {layers} layers',
                       dropouts, formula=True)


def check_counted(dev, monkeypatch):
    """+ 1 per training step for L >= 2, 0 for one layer (the five-job form) and 0 with the switch at 0"""
    monkeypatch.delenv('EQD_CHAIN_RESIDENT', raising=False)
    pairs = synthetic.make_pairs([(21, 20)], 13)
    for layers in (1, 2, 3):
        args, sd = model_of(dev, layers)
        got = {}
        for mode in ('0', None):
            set_switch(monkeypatch, SWITCH, mode)
            got[mode] = one_step(dev, args, sd, pairs, 0.0)['counters']
        set_switch(monkeypatch, SWITCH, None)
        assert got['0'][0] == 0 and got[None][0] == (1 if layers >= 2 else 0) == expected(args), (layers, got)
        assert got['0'][1:] == got[None][1:] == (1,) + crw.old_counters(args), (layers, got)


def check_not_eligible(dev, monkeypatch, many_tiles=True):
    """every condition that keeps layer 0's backward chain on k_rowchain (or hands it to another kernel): the new counter
    stays put and the step's bits are those of the switch-off run"""
    monkeypatch.delenv('EQD_CHAIN_RESIDENT', raising=False)
    small = synthetic.make_pairs([(21, 20), (30, 18)], 13)

    def run(over, pairs, env, layers):
        args, sd = model_of(dev, layers, **over)
        for k, v in env.items():
            set_switch(monkeypatch, k, v)
        res = one_step(dev, args, sd, pairs, 0.0)
        for k in env:
            set_switch(monkeypatch, k, None)
        return res

    def stays(over, pairs, env, layers=3):
        on = run(over, pairs, env, layers)
        assert on['counters'][0] == 0, f'{over} {env}: the wide backward body ran {on["counters"][0]} times'
        off = run(over, pairs, dict(env, **{SWITCH: '0'}), layers)
        assert off['counters'] == on['counters'], (over, env, off['counters'], on['counters'])
        crp.assert_same_bits(off, on, f'{over} {env}')
    assert run({}, small, {}, 3)['counters'][0] == 1      # (the same model and batch with nothing in the way)
    stays({}, small, {'EQD_CHAIN_RESIDENT': '0'})
    stays(dict(cross_msgs=False), small, {})
    stays(dict(hip_storage_dtype='bf16'), small, {})
    stays({}, small, {'EQD_ROW_TILES': '2'})
    stays({}, small, {'EQD_ROWCHAIN_OCC': '1'})
    stays({}, small, {'EQD_ROWWAVE': '1'})
    stays({}, small, {}, layers=1)
    if many_tiles:      # 4 112 rows: 257 tiles on 256 CUs
        stays({}, synthetic.make_pairs([(250, 7)] * 16, 13), {}, layers=2)
    # the operator entry point at 69 x 69 with cross messages: six jobs too, but no dh job in front and a d_h job last
    case = nc.make_case(nc.CONFIGS['69x69'], 37)
    got = {}
    for mode in ('0', None):
        set_switch(monkeypatch, SWITCH, mode)
        before = wide_bwd_launches()
        got[mode] = nc.run_kernels(dev, case, False)[0]
        assert wide_bwd_launches() == before, f'eqd_node_update_bwd selected the wide backward body ({SWITCH}={mode})'
    set_switch(monkeypatch, SWITCH, None)
    for k in nc.NAMES_ROW + nc.NAMES_W:
        assert torch.equal(got['0'][k], got[None][k]), f'eqd_node_update_bwd: {k} differs'


# ---- one chain on guarded buffers (eqd_selftest_node_chain_bwd_wide) -----------------------------------------------------

D, DA, DH, LDN = 69, 80, 64, 271
OUTPUTS = ('dH', 'dz', 'ln_part', 'd_aggr_msg', 'd_aggr_cross', 'dh0acc')


class EqdNodeChainBwdWideTest(C.Structure):
    _fields_ = [('rows', C.c_int32), ('skip_weight_h', C.c_float), ('slope', C.c_float), ('ln_eps', C.c_float),
                ('dh_X', C.c_void_p * 6), ('dh_W', C.c_void_p * 6), ('dh_wcs', C.c_int32 * 6)] + \
               [(k, C.c_void_p) for k in ('dH_above', 'dH', 'Wn2', 'Wn1', 'y_act', 'ln_g', 'drop_mul', 'dz', 'ln_part',
                                          'd_aggr_msg', 'd_aggr_cross', 'dh0acc')]


_CASES = {}


def guarded_case(rows, drop, seed=7):
    """the chain's inputs on the host (made once per size and shared, never changed)"""
    key = (rows, drop, seed)
    if key not in _CASES:
        gen = torch.Generator().manual_seed(seed)
        rnd = lambda *sh, scale=0.5: torch.randn(*sh, generator=gen) * scale      # noqa: E731
        c = dict(rows=rows, X=[rnd(rows, DH) for _ in range(6)], above=rnd(rows, DH), y_act=rnd(rows, D, scale=1.0),
                 acc0=rnd(rows, DH), ln_g=1.0 + 0.2 * torch.randn(D, generator=gen))
        # the weights as layer 1 / layer 0 hold them, element (m, k) of a transposed source at W[k][offset + m]:
        # layer 1's Wn1 [64][261], W1 [64][128] (two sources), Wq / Wk / Wv [64][64]; layer 0's Wn2 [64][69], Wn1 [69][271]
        c['dh_W'] = [(rnd(64, 261, scale=0.3), 0), None, None, (rnd(64, 64, scale=0.3), 0), (rnd(64, 64, scale=0.3), 0),
                     (rnd(64, 64, scale=0.3), 0)]
        W1 = rnd(64, 128, scale=0.3)
        c['dh_W'][1], c['dh_W'][2] = (W1, 0), (W1, 64)
        c['Wn2'], c['Wn1'] = rnd(DH, D, scale=0.3), rnd(D, LDN, scale=0.3)
        c['mul'] = None
        if drop:
            c['mul'] = (torch.rand(rows, D, generator=gen) >= 0.25).float() / 0.75
            c['mul'][rows - 1] = 0.0      # a row whose dropout factors are all zero, inside the last (ragged) tile
        _CASES[key] = c
    return _CASES[key]


def chain_formulas(c, dtype):
    """the six jobs of the chain written out in torch, evaluated in `dtype` on copies of the float32 inputs"""
    t = lambda x: x.to(dtype)      # noqa: E731
    rows, s = c['rows'], 0.75
    dH = (1.0 - s) * t(c['above'])
    for X, (W, off) in zip(c['X'], c['dh_W']):
        dH = dH + t(X) @ t(W)[:, off:off + DH]
    da = dH @ t(c['Wn2'])
    y = t(c['y_act'])
    cen = y - y.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt((cen * cen).mean(1, keepdim=True) + nc.EPS)
    xh = cen * rstd
    dx = da * t(c['ln_g'])
    z = rstd * (dx - dx.mean(1, keepdim=True) - xh * (dx * xh).mean(1, keepdim=True))
    z = z * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, nc.SLOPE))
    if c['mul'] is not None:
        z = z * t(c['mul'])
    tiles = (rows + 15) // 16
    lnp = torch.zeros(tiles, 256, dtype=dtype)
    for i in range(tiles):
        sl = slice(16 * i, min(16 * i + 16, rows))
        lnp[i, :D] = (da[sl] * xh[sl]).sum(0)
        lnp[i, 128:128 + D] = da[sl].sum(0)
    Wn1 = t(c['Wn1'])
    cross = torch.zeros(rows, DA, dtype=dtype)
    cross[:, :D] = z @ Wn1[:, D + 64:2 * D + 64]
    return dict(dH=dH, dz=z, ln_part=lnp, d_aggr_msg=z @ Wn1[:, D:D + 64], d_aggr_cross=cross,
                dh0acc=t(c['acc0']) + z @ Wn1[:, 2 * D + 64:2 * D + 128])


def run_guarded_chain(dev, c):
    """The six-job chain on NaN-filled outputs with sentinel rows behind every buffer, sources with sentinel rows behind them
    (a ragged tile's copies clamp to the last row) and NaN behind every weight matrix.  Returns the outputs after the guards,
    the untouched parts and the written parts have been checked."""
    rows, nan, tiles = c['rows'], float('nan'), (c['rows'] + 15) // 16

    def src(x):
        t = nc._guarded(dev, rows, x.shape[1], 0.0)
        t[:rows] = x.to(dev)
        return t

    def weight(w):      # NaN behind the last row: a piece that ran past the end of the matrix would poison an output
        t = torch.full((w.numel() + 64,), nan, dtype=torch.float32, device=dev)
        t[:w.numel()] = w.reshape(-1).to(dev)
        return t
    X = [src(x) for x in c['X']]
    above, y_act = src(c['above']), src(c['y_act'])
    mul = None if c['mul'] is None else src(c['mul'])
    wbuf = {id(w): weight(w) for w, _ in c['dh_W']}
    Wn2, Wn1, ln_g = weight(c['Wn2']), weight(c['Wn1']), c['ln_g'].to(dev)
    out = dict(dH=nc._guarded(dev, rows, DH, nan), dz=nc._guarded(dev, rows, D, nan), ln_part=nc._guarded(dev, tiles, 256, nan),
               d_aggr_msg=nc._guarded(dev, rows, 64, nan), d_aggr_cross=nc._guarded(dev, rows, DA, nan),
               dh0acc=nc._guarded(dev, rows, D, nan))
    out['dh0acc'][:rows, :64] = c['acc0'].to(dev)      # the accumulator of the layers above
    inputs = X + [above, y_act, Wn2, Wn1, ln_g] + list(wbuf.values()) + ([] if mul is None else [mul])
    before = [t.clone() for t in inputs]
    t = EqdNodeChainBwdWideTest()
    t.rows, t.skip_weight_h, t.slope, t.ln_eps = rows, 0.75, nc.SLOPE, nc.EPS
    for s in range(6):
        w, off = c['dh_W'][s]
        t.dh_X[s] = X[s].data_ptr()
        t.dh_W[s] = wbuf[id(w)].data_ptr() + 4 * off
        t.dh_wcs[s] = w.shape[1]
    t.dH_above, t.Wn2, t.Wn1 = above.data_ptr(), Wn2.data_ptr(), Wn1.data_ptr()
    t.y_act, t.ln_g, t.drop_mul = y_act.data_ptr(), ln_g.data_ptr(), None if mul is None else mul.data_ptr()
    for k in OUTPUTS:
        setattr(t, k, out[k].data_ptr())
    nb = C.c_int(0)
    fn = pc.lib().eqd_selftest_node_chain_bwd_wide
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.check(fn(C.byref(t), C.byref(nb), pc.st(dev)))
    pc.sync(dev)
    assert nb.value == tiles, (nb.value, tiles)
    for a, b in zip(inputs, before):
        assert torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0)), 'a source buffer (or its guard) was written'
    got = {}
    for k, v in out.items():
        n = tiles if k == 'ln_part' else rows
        assert bool((v[n:] == nc.SENTINEL).all()), f'{k}: the guard rows behind the buffer were written'
        got[k] = v[:n].cpu()
    for k in ('dH', 'dz', 'ln_part', 'd_aggr_msg', 'd_aggr_cross'):      # (dz: columns 0 .. 68, the whole row)
        assert bool(torch.isfinite(got[k]).all()), f'{k}: not every element was written'
    assert bool((got['d_aggr_cross'][:, D:] == 0).all()), 'd aggr_cross: the padding columns 69 .. 79 are zeros'
    assert bool(torch.isfinite(got['dh0acc'][:, :64]).all()) and bool(torch.isnan(got['dh0acc'][:, 64:]).all()), \
        'dh0acc: the 64 embedding columns are written, the trailing feature columns are not'
    lp = got['ln_part']      # the general body writes all 256 floats of the row: sums of features >= 69 are zeros
    assert bool((lp[:, D:128] == 0).all()) and bool((lp[:, 128 + D:] == 0).all()), 'ln_part: columns of features beyond 69'
    if mul is not None:
        assert bool((got['dz'][rows - 1] == 0).all()), 'dz of the row with all-zero dropout factors'
    return got


def check_guard_rows(dev, monkeypatch, measure=None):
    """37 rows (5 in the last tile) with dropout factors, 16 rows without: both bodies write the same bits, and both meet
    the float64 evaluation of the chain's formulas within 8 x the float32 evaluation's own distance from it (the rule of
    tests/atb_common.py: the yardstick's error, never the kernels')"""
    monkeypatch.delenv('EQD_CHAIN_RESIDENT', raising=False)
    for rows, drop in ((37, True), (16, False)):
        c = guarded_case(rows, drop)
        ref, f32 = chain_formulas(c, torch.float64), chain_formulas(c, torch.float32)
        res = {}
        for mode in ('0', None):
            set_switch(monkeypatch, SWITCH, mode)
            before = wide_bwd_launches()
            res[mode] = run_guarded_chain(dev, c)
            assert wide_bwd_launches() - before == (0 if mode == '0' else 1), f'{SWITCH}={mode}, {rows} rows: which body ran'
        set_switch(monkeypatch, SWITCH, None)
        for k in OUTPUTS:
            a, b = res['0'][k], res[None][k]
            assert torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0)), f'{rows} rows: {k} differs between the bodies'
        for k in OUTPUTS:
            cols = slice(0, 64) if k == 'dh0acc' else slice(None)
            yard = nc.rel_max(f32[k][:, cols], ref[k][:, cols])
            dist = {m: nc.rel_max(res[m][k][:, cols], ref[k][:, cols]) for m in ('0', None)}
            print(f'rows {rows} {k}: float32 evaluation {yard:.3e}, k_rowchain {dist["0"]:.3e}, wide body {dist[None]:.3e}')
            if measure is not None:
                measure[(rows, k)] = (yard, dist['0'], dist[None])
            assert yard > 0
            assert dist['0'] <= 8.0 * yard, f'{rows} rows, {k}: the general body misses the bound - the yardstick is wrong'
            assert dist[None] <= 8.0 * yard, f'{rows} rows, {k}: {dist[None]:.3e} > 8 x {yard:.3e}'
