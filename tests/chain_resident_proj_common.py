"""Bit comparison of the carrying forms of the resident forward node chain (k_rowchain_res_fwd<5> / <1>,
csrc/eqd_chainres_inl.h; EQD_CHAIN_RESIDENT_PROJ unset / 1) with the two-job body plus the projections' own launches
(EQD_CHAIN_RESIDENT_PROJ=0: k_linear_simple for P, Q, q, k, v of the next layer, k_linear for the head's mlp_h_mean_ROT).
A carried job is one cr_mma-ordered 64-deep chunk and linear_tile_lean's epilogue expressions on the tile of h[l+1] that
node_mlp.4 left in LDS - the MFMA sequence and the expressions of the separate launch - so every output, every saved node
tensor (P, Q, q, k, v, a1n, hm, h, x) and the flat gradient must be EQUAL, not close.  Shared by
tests/test_chain_resident_proj_sim.py and tests/test_chain_resident_proj_gpu.py.

Which chains: layer 0 is 69 wide and never eligible; every later layer's chain carries the next layer's five projections
(<5>), the last layer's carries the head's job (<1>): a model of L layers launches L - 1 carrying chains per forward, one of
them the <1> form.

What the simulator cannot see: it copies at issue time, so a missing or too-small vmcnt wait shows up only on the GPU - as
bits that differ or that change between replays (the GPU file compares replays of one captured step as well)."""
import ctypes as C

import torch

from equidock_public_amd import _lib as L
from equidock_public_amd import graph as G
from equidock_public_amd import synthetic
from oracle import iegmn_port as port
from tests import chain_resident_common as cr
from tests import node_chain_common as nc
from tests import parity_common as pc
from tests.util import cat_out, load_case, pairs_from_raw, state_dict_for

SWITCH = 'EQD_CHAIN_RESIDENT_PROJ'
NODE_TENSORS = ('P', 'Q', 'q', 'k', 'v', 'a1n', 'hm')


def proj_launches():
    fn = pc.lib().eqd_chain_resident_proj_launches
    fn.restype = C.c_longlong
    fn.argtypes = []
    return int(fn())


def expected_forms(args):
    """(+1 launches, +5 launches) of one forward of the model `args` describes, at a batch of no more tiles than CUs"""
    if not args['cross_msgs'] or args.get('hip_storage_dtype') == 'bf16' or not args['use_mean_node_features']:
        return 0, 0
    layers = int(args['iegmn_n_lays'])
    return (1, layers - 2) if layers >= 2 else (0, 0)


def set_switch(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)
    L.reload_tunables()


def node_state(net, g, layer):
    """{name: tensor} of NODE_TENSORS for `layer` of the last forward that kept its state (eqd_model_node_state)"""
    m = net.iegmn_original
    packed = g.pack()
    saved, sb = packed._last_saved[0], packed._last_saved[1]
    desc, gs = m._desc(), packed.c_struct()
    ptrs, d_in, d_att = (C.c_void_p * 7)(), C.c_int(0), C.c_int(0)
    fn = pc.lib().eqd_model_node_state
    fn.restype = C.c_int
    L.check(fn(C.byref(desc), C.byref(gs), L.ptr(saved), C.c_size_t(sb), int(layer), ptrs, C.byref(d_in), C.byref(d_att)))
    n, base = packed.n_nodes, saved.data_ptr()
    f = saved.view(torch.float32) if saved.numel() % 4 == 0 else saved[:saved.numel() // 4 * 4].view(torch.float32)
    widths = (64, 64, d_att.value, d_att.value, d_att.value, d_in.value, 64)
    out = {}
    for name, p, w in zip(NODE_TENSORS, ptrs, widths):
        if p:
            at = (p - base) // 4
            out[name] = f[at:at + n * w].view(n, w).clone()
    return out


def one_step(dev, args, sd, pairs, dropout):
    """One seeded training step -> outputs, (h, x) per layer, node tensors per layer, flat gradient, launches of the resident
    forward body and of its carrying forms"""
    args = dict(args)
    if dropout > 0:
        args = dict(args, dropout=dropout, hip_dropout_masks='library')
    net = pc.build_model(args, sd, dev)
    net.train(True)
    flat = net.iegmn_original.enable_flat_grads()
    g = G.batch_pairs(pairs).to(dev)
    flat.zero_()
    torch.manual_seed(99)
    before = cr.resident_launches(), proj_launches()
    outs = net(g, epoch=0)
    n_lays = int(args['iegmn_n_lays'])
    bf16 = args.get('hip_storage_dtype') == 'bf16'      # (bf16 storage keeps no fp32 form of the middle layers' state)
    states = [net.iegmn_original.layer_state(g, l) for l in ((0, n_lays) if bf16 else range(n_lays + 1))]
    nodes = [] if bf16 else [node_state(net, g, l) for l in range(n_lays)]
    launched = cr.resident_launches() - before[0], proj_launches() - before[1]
    port.scalar_loss(outs).backward()
    pc.sync(dev)
    assert float(flat.abs().max()) > 0
    return dict(outs=[cat_out(list(o)).detach().clone() for o in outs], states=states, nodes=nodes, grad=flat.clone(),
                resident=launched[0], carrying=launched[1])


def assert_same_bits(a, b, w):
    for x, y in zip(a['outs'], b['outs']):
        assert torch.equal(x, y), f'{w}: outputs differ (max {float((x - y).abs().max()):.3e})'
    for l, ((h0, x0), (h1, x1)) in enumerate(zip(a['states'], b['states'])):
        assert torch.equal(h0, h1), f'{w}: h after layer {l} differs (max {float((h0 - h1).abs().max()):.3e})'
        assert torch.equal(x0, x1), f'{w}: x after layer {l} differs'
    assert len(a['nodes']) == len(b['nodes'])
    for l, (n0, n1) in enumerate(zip(a['nodes'], b['nodes'])):
        assert set(n0) == set(n1)
        for k in n0:
            assert torch.equal(n0[k], n1[k]), f'{w}: {k} of layer {l} differs (max {float((n0[k] - n1[k]).abs().max()):.3e})'
    g0, g1 = a['grad'], b['grad']
    assert torch.equal(g0, g1), f'{w}: gradients differ (max {float((g0 - g1).abs().max()):.3e} of {float(g0.abs().max()):.3e})'


def check_forms_agree(dev, monkeypatch, args, sd, pairs, what, dropouts=(0.0, 0.25)):
    monkeypatch.delenv('EQD_CHAIN_RESIDENT', raising=False)
    want = sum(expected_forms(args))
    assert want > 0, f'{what}: no carrying chain in this model'
    for dropout in dropouts:
        res = {}
        for mode in ('0', '1'):
            set_switch(monkeypatch, SWITCH, mode)
            res[mode] = one_step(dev, args, sd, pairs, dropout)
        set_switch(monkeypatch, SWITCH, None)
        w = f'{what}, dropout {dropout}'
        assert res['0']['resident'] == res['1']['resident'] == want, \
            f'{w}: the resident forward body ran {res["0"]["resident"]} / {res["1"]["resident"]} times, expected {want}'
        assert res['0']['carrying'] == 0, f'{w}: {SWITCH}=0 launched a carrying form {res["0"]["carrying"]} times'
        assert res['1']['carrying'] == want, f'{w}: {res["1"]["carrying"]} carrying launches, expected {want}'
        assert_same_bits(res['0'], res['1'], w)


def check_golden_case(dev, monkeypatch, name, dropouts=(0.0, 0.25)):
    z, meta, args, raw = load_case(name)
    check_forms_agree(dev, monkeypatch, args, state_dict_for(meta, args), pairs_from_raw(raw), name, dropouts)


def model_of(dev, layers, **over):
    args = port.default_args(**dict(dict(iegmn_n_lays=layers, skip_weight_h=0.75, device=torch.device(dev)), **over))
    return args, port.init_state_dict(args, seed=4, rot_scale=10.0)


# rows: 15 (less than one tile), 48 (whole tiles), 65, 79 (n % 16 in {1, 15}), 97 (a ragged last tile of two segments): the
# clamped rows of the last tile are computed and must not be stored
SIZES = ([(7, 8)], [(24, 24)], [(33, 32)], [(40, 39)], [(17, 20), (30, 30)])
LAYERS = (2, 3, 4)


def rows_of(sizes):
    return sum(a + b for a, b in sizes)


def check_sizes(dev, monkeypatch, sizes, layers):
    args, sd = model_of(dev, layers)
    check_forms_agree(dev, monkeypatch, args, sd, synthetic.make_pairs(sizes, 13), f'{rows_of(sizes)} rows, {layers} layers')


def forward_counts(dev, args, sd, pairs):
    """launch names (eqd_profile_*) and the counters' increments of one forward that keeps its state"""
    net = pc.build_model(args, sd, dev)
    net.train(True)
    g = G.batch_pairs(pairs).to(dev)
    before = cr.resident_launches(), proj_launches()
    keep = {}
    names = pc.launch_names(dev, lambda: keep.update(outs=net(g, epoch=0)))
    pc.sync(dev)
    outs = [cat_out(list(o)).detach().clone() for o in keep['outs']]
    return names, cr.resident_launches() - before[0], proj_launches() - before[1], outs


def check_forms_counted(dev, monkeypatch):
    """layers 1 .. 4: (+1, +5) launches = (0, 0), (1, 0), (1, 1), (1, 2) - never layer 0's chain; with the switch at 0 the
    counter does not move and the forward's launches are the parent's: 2 L + ... k_linear entries, L for the projections and
    one for the head"""
    monkeypatch.delenv('EQD_CHAIN_RESIDENT', raising=False)
    pairs = synthetic.make_pairs([(21, 20)], 13)
    for layers, (one, five) in zip((1, 2, 3, 4), ((0, 0), (1, 0), (1, 1), (1, 2))):
        args, sd = model_of(dev, layers)
        assert expected_forms(args) == (one, five)
        set_switch(monkeypatch, SWITCH, None)
        names1, res1, car1, outs1 = forward_counts(dev, args, sd, pairs)
        set_switch(monkeypatch, SWITCH, '0')
        names0, res0, car0, outs0 = forward_counts(dev, args, sd, pairs)
        set_switch(monkeypatch, SWITCH, None)
        assert car1 == one + five and car0 == 0, (layers, car1, car0)
        assert res1 == res0 == layers - 1, (layers, res1, res0)      # every 64-wide layer's chain, in both settings
        lin0, lin1 = names0.count('k_linear'), names1.count('k_linear')
        assert lin0 == layers + 1, (layers, names0)                   # the parent's: one per layer and the head's
        assert lin1 == lin0 - (one + five), (layers, names1)          # a carrying launch replaces exactly one of them
        assert names0.count('k_rowchain') == names1.count('k_rowchain') == layers
        assert len(names0) - len(names1) == one + five
        for a, b in zip(outs0, outs1):
            assert torch.equal(a, b)


def check_not_eligible(dev, monkeypatch, many_tiles=True):
    """every condition that keeps the two-job chain and the projections' own launches: the carrying counter does not move,
    and the bits are those of EQD_CHAIN_RESIDENT_PROJ=0"""
    monkeypatch.delenv('EQD_CHAIN_RESIDENT', raising=False)
    small = synthetic.make_pairs([(21, 20), (30, 18)], 13)

    def run(over, pairs, env=None, layers=3):
        args, sd = model_of(dev, layers, **over)
        res = {}
        for mode in (None, '0'):
            for k, v in (env or {}).items():
                set_switch(monkeypatch, k, v)
            set_switch(monkeypatch, SWITCH, mode)
            res[mode] = one_step(dev, args, sd, pairs, 0.0)
            for k in (env or {}):
                set_switch(monkeypatch, k, None)
        set_switch(monkeypatch, SWITCH, None)
        assert_same_bits(res['0'], res[None], f'{over} {env}')
        assert res['0']['carrying'] == 0
        return res[None]['carrying'], res[None]['resident']
    assert run({}, small) == (2, 2)      # (the same model and batch with nothing in the way)
    assert run(dict(cross_msgs=False), small) == (0, 2)      # two projections per layer, no attention: the two-job body
    assert run(dict(hip_storage_dtype='bf16'), small) == (0, 0)
    assert run({}, small, {'EQD_CHAIN_RESIDENT': '0'}) == (0, 0)
    assert run({}, small, {'EQD_ROW_TILES': '2'}) == (0, 0)
    assert run({}, small, {'EQD_ROWCHAIN_OCC': '1'}) == (0, 0)
    assert run({}, small, {'EQD_ROWWAVE': '1'})[0] == 0      # a forced k_rowwave takes the chains first
    # 4 112 rows: 257 tiles on 256 CUs (the simulator's device has 256 as well).  many_tiles = 'forward': the forward alone -
    # which is where the forms are chosen - and its outputs; a training step of this batch takes the simulator minutes
    many = synthetic.make_pairs([(250, 7)] * 16, 13)
    if many_tiles == 'forward':
        args, sd = model_of(dev, 2)
        res = {}
        for mode in (None, '0'):
            set_switch(monkeypatch, SWITCH, mode)
            res[mode] = forward_counts(dev, args, sd, many)
        set_switch(monkeypatch, SWITCH, None)
        assert res[None][1:3] == res['0'][1:3] == (0, 0) and res[None][0] == res['0'][0]
        for a, b in zip(res[None][3], res['0'][3]):
            assert torch.equal(a, b)
    elif many_tiles:
        assert run({}, many, layers=2) == (0, 0)


# ---- one carrying chain on guarded buffers (eqd_selftest_node_chain_fwd) -------------------------------------------------


class EqdNodeChainFwdTest(C.Structure):
    _fields_ = [('rows', C.c_int32), ('d0', C.c_int32), ('form', C.c_int32), ('skip_weight_h', C.c_float),
                ('slope', C.c_float), ('ln_eps', C.c_float)] + \
               [(k, C.c_void_p) for k in ('h', 'aggr_msg', 'aggr_cross', 'h0', 'Wn1', 'Bn1', 'ln_g', 'ln_b', 'Wn2', 'Bn2',
                                          'drop_mul', 'a1n', 'y_act', 'h_out', 'W1', 'B1', 'WQ', 'WK', 'WV', 'P', 'Q', 'qa',
                                          'ka', 'va', 'WM', 'BM', 'head_mul', 'hm')]


OUTPUTS = {5: ('a1n', 'y_act', 'h_out', 'P', 'Q', 'qa', 'ka', 'va'), 1: ('a1n', 'y_act', 'h_out', 'hm')}


def run_guarded_chain(dev, form, rows=37, d0=69, seed=7):
    """One chain of the model driver's list: NaN-filled outputs with sentinel rows behind every buffer, sources with sentinel
    rows behind them (the copies of a ragged tile clamp to the last row).  Returns the outputs after the guards, the sources
    and the written rows have been checked."""
    gen = torch.Generator().manual_seed(seed)
    nan, ldn = float('nan'), d0 + 192

    def src(cols, scale=0.5):
        t = nc._guarded(dev, rows, cols, nan)
        t[:rows] = (torch.randn(rows, cols, generator=gen) * scale).to(dev)
        return t
    mk = lambda *sh: (torch.randn(*sh, generator=gen) * 0.3).to(dev).contiguous()      # noqa: E731
    X = dict(h=src(64), aggr_msg=src(64), aggr_cross=src(64), h0=src(d0))
    mul, hmul = src(64), src(64)
    mul[:rows] = ((torch.rand(rows, 64, generator=gen) >= 0.25).float() / 0.75).to(dev)
    hmul[:rows] = ((torch.rand(rows, 64, generator=gen) >= 0.25).float() / 0.75).to(dev)
    hmul[rows - 1] = 0.0      # a row whose dropout factors are all zero, inside the ragged tile
    Wt = dict(Wn1=mk(64, ldn), Bn1=mk(64), ln_g=1.0 + mk(64), ln_b=mk(64), Wn2=mk(64, 64), Bn2=mk(64), W1=mk(64, 128),
              B1=mk(64), WQ=mk(64, 64), WK=mk(64, 64), WV=mk(64, 64), WM=mk(64, 64), BM=mk(64))
    out = {k: nc._guarded(dev, rows, 64, nan) for k in OUTPUTS[form]}
    inputs = list(X.values()) + [mul, hmul]
    before = [t.clone() for t in inputs]
    t = EqdNodeChainFwdTest()
    t.rows, t.d0, t.form, t.skip_weight_h, t.slope, t.ln_eps = rows, d0, form, 0.75, nc.SLOPE, nc.EPS
    for k, v in list(X.items()) + list(Wt.items()) + list(out.items()):
        setattr(t, k, v.data_ptr())
    t.drop_mul, t.head_mul = mul.data_ptr(), hmul.data_ptr()
    fn = pc.lib().eqd_selftest_node_chain_fwd
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p]
    L.check(fn(C.byref(t), pc.st(dev)))
    pc.sync(dev)
    for a, b in zip(inputs, before):
        assert torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0)), 'a source buffer (or its guard) was written'
    got = {}
    for k, v in out.items():
        assert bool((v[rows:] == nc.SENTINEL).all()), f'{k}: the guard rows behind the buffer were written'
        got[k] = v[:rows].cpu()
        assert bool(torch.isfinite(got[k]).all()), f'{k}: a NaN below row {rows}: not every element was written, or a guard row was read'
    if form == 1:
        assert bool((got['hm'][rows - 1] == 0).all()), 'hm of the row with all-zero dropout factors'
    return got


def check_guard_rows(dev, monkeypatch):
    monkeypatch.delenv('EQD_CHAIN_RESIDENT', raising=False)
    for form in (5, 1):
        res = {}
        for mode in ('0', '1'):
            set_switch(monkeypatch, SWITCH, mode)
            before = proj_launches()
            res[mode] = run_guarded_chain(dev, form)
            assert proj_launches() - before == int(mode), f'{SWITCH}={mode}, form {form}: which body ran'
        set_switch(monkeypatch, SWITCH, None)
        for k in res['0']:
            assert torch.equal(res['0'][k], res['1'][k]), f'form {form}: {k} differs between the bodies'
