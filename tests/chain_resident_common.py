"""Bit comparison of the two bodies of the forward node chain: k_rowchain (EQD_CHAIN_RESIDENT=0) and the resident-weights
body k_rowchain_res_fwd (unset / 1; csrc/eqd_chainres_inl.h).  The resident body runs the same MFMA sequence per output
element, the same chunk order and the same epilogue expressions, so every output, every saved layer state and the flat
gradient must be EQUAL, not close.  Shared by tests/test_chain_resident_sim.py and tests/test_chain_resident_gpu.py.

What the simulator cannot see: it copies at issue time, so a missing or too-small vmcnt wait shows up only on the GPU - as
bits that differ from k_rowchain's or between replays (the GPU file compares replays of one captured step as well)."""
import ctypes as C

import torch

from equidock_public_amd import _lib as L
from equidock_public_amd import config
from equidock_public_amd import graph as G
from equidock_public_amd import synthetic
from oracle import iegmn_port as port
from tests import parity_common as pc
from tests.util import cat_out, load_case, pairs_from_raw, state_dict_for


def resident_launches():
    fn = pc.lib().eqd_chain_resident_launches
    fn.restype = C.c_longlong
    fn.argtypes = []
    return int(fn())


def one_step(dev, args, sd, pairs, dropout):
    """One seeded training step -> (outputs, layer states, flat gradient, resident-body launches of this step)"""
    args = dict(args)
    if dropout > 0:
        args = dict(args, dropout=dropout, hip_dropout_masks='library')
    net = pc.build_model(args, sd, dev)
    net.train(True)
    flat = net.iegmn_original.enable_flat_grads()
    g = G.batch_pairs(pairs).to(dev)
    flat.zero_()
    torch.manual_seed(99)
    before = resident_launches()
    outs = net(g, epoch=0)
    n_lays = int(args['iegmn_n_lays'])
    states = [net.iegmn_original.layer_state(g, l) for l in range(n_lays + 1)]
    port.scalar_loss(outs).backward()
    pc.sync(dev)
    launched = resident_launches() - before
    assert float(flat.abs().max()) > 0
    return [cat_out(list(o)).detach().clone() for o in outs], states, flat.clone(), launched


def check_bodies_agree(dev, monkeypatch, args, sd, pairs, what, dropouts=(0.0, 0.25)):
    for dropout in dropouts:
        res = {}
        for mode in ('0', '1'):
            monkeypatch.setenv('EQD_CHAIN_RESIDENT', mode)
            L.reload_tunables()
            res[mode] = one_step(dev, args, sd, pairs, dropout)
        monkeypatch.delenv('EQD_CHAIN_RESIDENT')
        L.reload_tunables()
        w = f'{what}, dropout {dropout}'
        assert res['0'][3] == 0, f'{w}: EQD_CHAIN_RESIDENT=0 launched the resident body {res["0"][3]} times'
        assert res['1'][3] > 0, f'{w}: the resident body was never launched'
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


def workload_b(dev):
    """the model, weights and batch bench.py runs as workload B (8 pairs x (200, 200), 8 layers, seeds 0 / 1000)"""
    args = config.published_args(iegmn_n_lays=8, shared_layers=False, skip_weight_h=0.75, device=torch.device(dev))
    return args, config.seeded_state_dict(args, seed=0), synthetic.make_pairs([(200, 200)] * 8, seed=1000)


def check_workload_b(dev, monkeypatch):
    args, sd, pairs = workload_b(dev)
    check_bodies_agree(dev, monkeypatch, args, sd, pairs, 'workload B')


def check_ragged_tiles(dev, monkeypatch):
    """row counts that leave 1 and 15 rows in the last 16-row tile (the clamped source rows of the copies)"""
    args = port.default_args(iegmn_n_lays=3, skip_weight_h=0.75, device=torch.device(dev))
    sd = port.init_state_dict(args, seed=4, rot_scale=10.0)
    for sizes in ([(33, 32)], [(40, 39)], [(17, 20), (30, 30)], [(31, 16), (40, 24)]):
        n = sum(a + b for a, b in sizes)
        assert n % 16 in (1, 15), n
        check_bodies_agree(dev, monkeypatch, args, sd, synthetic.make_pairs(sizes, 13), f'{n} rows')
