"""Byte comparison of the two edge-forward bodies of the fused small-batch launch of a 64-wide layer: edge_fwd_body on whole
32-edge tiles (k_edge_attn_fwd, EQD_EDGE_FWD_HALF=0) and edge_fwd_half_body on 16-edge half tiles, a pair of waves per tile
(k_edge_attn_fwd_half, unset / 1; csrc/eqd_edge_fwd_half_inl.h).  Every per-edge value of a half is the value the whole-tile
wave computes for that edge (a column of an MFMA product depends on its own column of the B operand only), and every
column block of the per-node means sees the same eight steps in the same order: aggr_msg, x_new, the attention output and
lse must be EQUAL byte for byte, not close.  Shared by tests/test_edge_half_sim.py and tests/test_edge_half_gpu.py.

The launch is called through eqd_selftest_edge_attn_fwd on sentinel-framed, NaN-filled buffers; the graphs are synthetic
pairs whose in-degrees are pruned to the patterns below, so that the greedy node-aligned tiling produces the tile shapes at
which a split by halves can go wrong (check_shapes asserts that it did)."""
import ctypes as C

import numpy as np
import torch

from equidock_public_amd import _lib as L
from equidock_public_amd import graph as G
from equidock_public_amd import synthetic
from tests import chain_resident_proj_common as crp
from tests import parity_common as pc
from tests.util import load_case, pairs_from_raw, state_dict_for

SWITCH = 'EQD_EDGE_FWD_HALF'
set_switch = crp.set_switch
OUTPUTS = ('aggr_msg', 'x_new', 'att_out', 'lse')
GUARD = 64
SENTINEL = -7.25

# In-degree patterns (ligand, receptor); the tiling is greedy over the nodes in order (<= 32 edges, <= 32 nodes per tile):
#   [17] | [16, 16] | [10, 10, 10, 2] | [1] * 20 | [13, 0, 0, 3] | [17] ...
#   17 edges in one node that straddles positions 15 / 16 | 32 edges split exactly at 16 | 32 edges, the second node
#   (edges 10 .. 19) straddles 15 / 16 | 20 nodes (> 16: two node blocks in the means) | 16 edges (empty second half),
#   nodes of degree 0 | ...
MIXED = ([17, 16, 16, 10, 10, 10, 2] + [1] * 20 + [13, 0, 0, 3, 17, 9, 0, 12, 11, 5, 16],
         [20, 3, 0, 0, 0, 15, 1, 1, 1, 14, 7, 7, 7, 7, 4, 18, 2, 19, 13, 0, 6, 6, 20, 12, 1])
# one tile of 14 edges on 8 nodes, two of them of degree 0: a single-tile graph, its second half empty
SINGLE = ([3, 2, 0, 3], [2, 0, 3, 1])
# one tile of exactly 32 edges on 24 nodes; the second node (edges 11 .. 20) straddles positions 15 / 16
FULL = ([11, 10], [11])
GRAPHS = {'mixed': MIXED, 'single_tile': SINGLE, 'full_tile': FULL}


def launches():
    fn = pc.lib().eqd_edge_fwd_half_launches
    fn.restype = C.c_longlong
    fn.argtypes = []
    return int(fn())


def pruned_pair(degs, seed=21):
    """one synthetic pair whose node i keeps the first degs[i] of its in-edges"""
    dl, dr = degs
    k = max(max(dl), max(dr))
    n = [max(len(d), k + 1) for d in (dl, dr)]      # (enough nodes for the largest degree; the extra nodes keep no edge)
    lig, rec = synthetic.make_pairs([tuple(n)], seed, k=k, cutoff=1e9)[0]
    for p, d in ((lig, dl), (rec, dr)):
        want = np.zeros(len(p['x']), np.int64)
        want[:len(d)] = d
        dst = p['dst'].astype(np.int64)
        first = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=len(want)))])[dst]
        keep = (np.arange(len(dst)) - first) < want[dst]
        for key in ('src', 'dst', 'he'):
            p[key] = p[key][keep]
        assert np.array_equal(np.bincount(p['dst'], minlength=len(want)), want)
    return lig, rec


def tiles_of(pk):
    """[(first edge, edges, nodes, row pointers relative to the first edge)] per tile"""
    tn, rp = pk.tile_node.cpu().numpy(), pk.rowptr.cpu().numpy()
    return [(int(rp[a]), int(rp[b] - rp[a]), int(b - a), (rp[a:b + 1] - rp[a]).tolist()) for a, b in zip(tn[:-1], tn[1:])]


def check_shapes(pk, name):
    """the graph `name` does hold the tile shapes it is there for"""
    t = tiles_of(pk)
    ne = [x[1] for x in t]
    straddle = [any(lo < 16 < hi for lo, hi in zip(x[3][:-1], x[3][1:])) for x in t]
    deg0 = [any(lo == hi for lo, hi in zip(x[3][:-1], x[3][1:])) for x in t]
    if name == 'mixed':
        assert 17 in ne and 32 in ne and any(0 < e <= 16 for e in ne), ne
        assert any(straddle) and any(deg0), (straddle, deg0)
        assert any(x[2] > 16 for x in t), [x[2] for x in t]
        assert len(t) % 8 != 0 and len(t) > 8, len(t)      # idle pairs in the last workgroup, more than one workgroup
    elif name == 'single_tile':
        assert len(t) == 1 and ne[0] <= 16 and deg0[0], t
    elif name == 'full_tile':
        assert len(t) == 1 and ne[0] == 32, t


def graph_of(dev, name):
    g = G.batch_pairs([pruned_pair(GRAPHS[name])]).to(dev)
    pk = g.pack()
    check_shapes(pk, name)
    return g, pk, L.graph_struct(pk)


def framed(n, dev):
    """a NaN-filled buffer of n floats between two sentinel guards -> (whole, body)"""
    whole = torch.full((n + 2 * GUARD,), SENTINEL, device=dev)
    body = whole[GUARD:GUARD + n]
    body.fill_(float('nan'))
    return whole, body


def edge_inputs(dev, pk, d_att=64, drop=False, bf16=False, seed=2):
    torch.manual_seed(seed)
    N, E, d_in = pk.n_nodes, pk.n_edges, 64
    ldw1 = 2 * d_in + 42
    host = dict(W1=torch.randn(64, ldw1) * 0.2, lng=torch.randn(64) * 0.5 + 1, lnb=torch.randn(64) * 0.1,
                W2=torch.randn(64, 64) * 0.2, b2=torch.randn(64) * 0.1, Wc1=torch.randn(64, 64) * 0.2,
                bc1=torch.randn(64) * 0.1, wc2=torch.randn(1, 64) * 0.2, bc2=torch.randn(1) * 0.1,
                Pn=torch.randn(N, 64), Qn=torch.randn(N, 64), x=pk.x0.cpu() + 0.1 * torch.randn(N, 3),
                q=torch.randn(N, d_att) * 0.5, k=torch.randn(N, d_att) * 0.5, v=torch.randn(N, d_att))
    d = {k: v.to(dev).contiguous() for k, v in host.items()}
    ep = L.EqdEdgeParams()
    ep.W1, ep.ldw1, ep.d_in, ep.ln_g, ep.ln_b = d['W1'].data_ptr(), ldw1, d_in, d['lng'].data_ptr(), d['lnb'].data_ptr()
    ep.W2, ep.b2, ep.Wc1, ep.bc1 = (d[k].data_ptr() for k in ('W2', 'b2', 'Wc1', 'bc1'))
    ep.wc2, ep.bc2 = d['wc2'].data_ptr(), d['bc2'].data_ptr()
    ep.slope, ep.ln_eps, ep.eta, ep.use_dist, ep.use_he = 0.01, 1e-5, 0.25, 1, 1
    ep.bf16 = int(bf16)
    fz = fc = None
    if drop:
        pdrop = 0.25
        kz, kc = torch.rand(E, 64) >= pdrop, torch.rand(E, 64) >= pdrop
        fz, fc = kz.float() / (1 - pdrop), kc.float() / (1 - pdrop)
        d['bz'], d['bc'] = pc.pack_keep_bits(kz).to(dev), pc.pack_keep_bits(kc).to(dev)
        ep.drop_z1, ep.drop_ch, ep.drop_scale = d['bz'].data_ptr(), d['bc'].data_ptr(), 1.0 / (1 - pdrop)
    return host, d, ep, fz, fc


def run_launch(dev, gs, pk, d, ep, d_att=64):
    """eqd_selftest_edge_attn_fwd on framed buffers -> ({name: body clone}, increment of the half-tile counter)"""
    N = pk.n_nodes
    bufs = {k: framed(N * w, dev) for k, w in zip(OUTPUTS, (64, 3, d_att, 1))}
    fn = pc.lib().eqd_selftest_edge_attn_fwd
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] * 7 + [C.c_int] + [C.c_void_p] * 6
    before = launches()
    P = pc.P
    L.check(fn(C.byref(gs), C.byref(ep), P(d['Pn']), P(d['Qn']), P(d['x']), P(bufs['aggr_msg'][1]), P(bufs['x_new'][1]),
               d_att, P(d['q']), P(d['k']), P(d['v']), P(bufs['att_out'][1]), P(bufs['lse'][1]), pc.st(dev)))
    pc.sync(dev)
    out = {}
    for k, (whole, body) in bufs.items():
        assert bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all()), f'{k}: guard overwritten'
        assert not bool(torch.isnan(body).any()), f'{k}: an element was left unwritten'
        out[k] = body.clone()
    return out, launches() - before


def same_bytes(a, b, what):
    for k in OUTPUTS:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), \
            f'{what}: {k} differs (max {float((a[k] - b[k]).abs().max()):.3e})'


def check_graph(dev, monkeypatch, name, drop=False):
    """the two bodies on the graph `name`: which one ran, equal bytes, and - without dropout masks in the way of a plain
    restatement they are covered by tests/parity_common.py - the torch formulas of the edge op and of the attention"""
    monkeypatch.delenv('EQD_FUSE_FWD', raising=False)
    g, pk, gs = graph_of(dev, name)
    host, d, ep, fz, fc = edge_inputs(dev, pk, drop=drop)
    got = {}
    for mode in ('0', None):
        set_switch(monkeypatch, SWITCH, mode)
        got[mode], n = run_launch(dev, gs, pk, d, ep)
        assert n == (0 if mode == '0' else 1), f'{name}: {SWITCH}={mode}: the half-tile kernel ran {n} times'
    set_switch(monkeypatch, SWITCH, None)
    same_bytes(got['0'], got[None], f'{name}, dropout {drop}')
    am, xn = pc._edge_ref(pk, 0.25, host['Pn'], host['Qn'], host['x'], host['W1'][:, 128:].contiguous(), host['lng'], host['lnb'],
                          host['W2'], host['b2'], host['Wc1'], host['bc1'], host['wc2'], host['bc2'], fz=fz, fc=fc)
    pc.close(got[None]['aggr_msg'].view(-1, 64), am, what=f'{name}: aggr_msg')
    pc.close(got[None]['x_new'].view(-1, 3), xn, what=f'{name}: x_new')
    pc.close(got[None]['att_out'].view(-1, 64), pc._attn_ref(pk, host['q'], host['k'], host['v']), what=f'{name}: attention')


def check_not_eligible(dev, monkeypatch, many_tiles=True):
    """bf16 (never fused), the 80-wide attention of the first layer (k_edge_attn_fwd80) and a fused launch of more tiles than
    wave pairs (two tiles per wave of k_edge_attn_fwd) stay on today's kernels: the counter stays put, equal bytes"""
    monkeypatch.delenv('EQD_FUSE_FWD', raising=False)

    def stays(g3, what, **kw):
        g, pk, gs = g3
        host, d, ep, fz, fc = edge_inputs(dev, pk, **kw)
        got = {}
        for mode in ('0', None):
            set_switch(monkeypatch, SWITCH, mode)
            got[mode], n = run_launch(dev, gs, pk, d, ep, d_att=kw.get('d_att', 64))
            assert n == 0, f'{what}: {SWITCH}={mode}: the half-tile kernel ran {n} times'
        set_switch(monkeypatch, SWITCH, None)
        same_bytes(got['0'], got[None], what)
    stays(graph_of(dev, 'mixed'), 'bf16', bf16=True)
    stays(graph_of(dev, 'mixed'), 'd_att = 80', d_att=80)
    if many_tiles:
        # 2 060 nodes of in-degree 32: one tile each, 129 edge workgroups of two tiles per wave beside 72 attention items
        g = G.batch_pairs(synthetic.make_pairs([(1030, 1030)], 5, k=32, cutoff=1e9)).to(dev)
        pk = g.pack()
        assert pk.n_tiles == 2060 and pk.n_att_items == 72, (pk.n_tiles, pk.n_att_items)
        stays((g, pk, L.graph_struct(pk)), 'more tiles than wave pairs')


# ---- through the model ---------------------------------------------------------------------------------------------------

def expected(args):
    """half-tile launches per forward: the fused launches of the 64-wide layers 1 .. L - 1 of an fp32 model"""
    if not args['cross_msgs'] or args.get('hip_storage_dtype') == 'bf16':
        return 0
    return int(args['iegmn_n_lays']) - 1


def one_step(dev, args, sd, pairs, dropout):
    before = launches()
    res = crp.one_step(dev, args, sd, pairs, dropout)
    res['half'] = launches() - before
    return res


def check_model(dev, monkeypatch, args, sd, pairs, what, dropouts=(0.0, 0.25)):
    monkeypatch.delenv('EQD_FUSE_FWD', raising=False)
    for dropout in dropouts:
        res = {}
        for mode in ('0', None):
            set_switch(monkeypatch, SWITCH, mode)
            res[mode] = one_step(dev, args, sd, pairs, dropout)
        set_switch(monkeypatch, SWITCH, None)
        w = f'{what}, dropout {dropout}'
        assert res['0']['half'] == 0, f'{w}: {SWITCH}=0 launched the half-tile kernel {res["0"]["half"]} times'
        assert res[None]['half'] == expected(args), f'{w}: the half-tile kernel ran {res[None]["half"]} times'
        crp.assert_same_bits(res['0'], res[None], w)


def check_golden_case(dev, monkeypatch, name, dropouts=(0.0, 0.25)):
    z, meta, args, raw = load_case(name)
    check_model(dev, monkeypatch, args, state_dict_for(meta, args), pairs_from_raw(raw), name, dropouts)


def check_counted(dev, monkeypatch):
    """+ 7 per forward of an 8-layer model (layer 0 runs k_edge_attn_fwd80), 0 with the switch at 0, 0 unfused"""
    args, sd = crp.model_of(dev, 8)
    pairs = synthetic.make_pairs([(21, 20)], 13)
    for env, want in (({}, 7), ({SWITCH: '0'}, 0), ({'EQD_FUSE_FWD': '0'}, 0)):
        for k, v in env.items():
            set_switch(monkeypatch, k, v)
        got = one_step(dev, args, sd, pairs, 0.0)['half']
        for k in env:
            set_switch(monkeypatch, k, None)
        assert got == want == (expected(args) if not env else 0), (env, got)
