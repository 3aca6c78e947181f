"""Bit comparison of the two bodies of the FIRST layer's forward node chain: k_rowchain's general body
(EQD_CHAIN_RESIDENT_WIDE=0) and the wide resident body k_rowchain_res_fwd_wide (unset / 1; csrc/eqd_chainres_wide_inl.h),
every other resident body on in both.  The wide body runs the general body's MFMA sequence per output element - source by
source, the full chunk and then the 5-column remainder as a zero-padded 16-deep step - its accumulator sets, its LayerNorm
exchange order over 69 features and its epilogue expressions, and linear_tile_lean's for node_mlp.4 with K = 69: every
output, every saved layer state, every saved node tensor (layer 0's a1n among them) and the flat gradient (which reads layer
0's y_act) must be EQUAL, not close.  Shared by tests/test_chain_resident_wide_sim.py and
tests/test_chain_resident_wide_gpu.py.

Which chains: layer 0's forward chain with cross messages, fp32, one 16-row tile per workgroup and no more tiles than CUs:
one launch per forward at every depth.  The three older counters keep counting 64-wide layers only.  Layer 0's BACKWARD
chain has no resident form and stays on k_rowchain.

What the simulator cannot see: it copies at issue time, so a missing or too-small vmcnt wait shows up only on the GPU - as
bits that differ or that change between replays (the GPU file compares replays of one captured step as well)."""
import ctypes as C

import torch

from equidock_public_amd import synthetic
from tests import chain_resident_bwd_common as crb
from tests import chain_resident_common as cr
from tests import chain_resident_proj_common as crp
from tests import node_chain_common as nc
from tests import parity_common as pc
from tests.util import load_case, pairs_from_raw, state_dict_for

SWITCH = 'EQD_CHAIN_RESIDENT_WIDE'
set_switch = crp.set_switch
model_of = crp.model_of
# rows: 15 (less than one tile), 48 (whole tiles), 65, 79 (1 and 15 rows in the last tile), 97 (two segments, ragged)
SIZES = crp.SIZES
LAYERS = (1, 2, 3)


def wide_launches():
    fn = pc.lib().eqd_chain_resident_wide_launches
    fn.restype = C.c_longlong
    fn.argtypes = []
    return int(fn())


def counters():
    return wide_launches(), cr.resident_launches(), crp.proj_launches(), crb.bwd_launches()


def one_step(dev, args, sd, pairs, dropout):
    """chain_resident_proj_common.one_step plus what the four counters moved by during the whole step"""
    before = counters()
    res = crp.one_step(dev, args, sd, pairs, dropout)
    res['counters'] = tuple(a - b for a, b in zip(counters(), before))
    return res


def old_counters(args):
    """what one training step moves the three older counters by (64-wide layers only)"""
    return (int(args['iegmn_n_lays']) - 1, sum(crp.expected_forms(args)), crb.expected_launches(args))


def check_bodies_agree(dev, monkeypatch, args, sd, pairs, what, dropouts=(0.0, 0.25), formula=False):
    monkeypatch.delenv('EQD_CHAIN_RESIDENT', raising=False)
    for dropout in dropouts:
        res = {}
        for mode in ('0', None):
            set_switch(monkeypatch, SWITCH, mode)
            res[mode] = one_step(dev, args, sd, pairs, dropout)
        set_switch(monkeypatch, SWITCH, None)
        w = f'{what}, dropout {dropout}'
        # one launch of the new body per step (the forward; the backward has none), the three older counters as before
        assert res['0']['counters'][0] == 0, f'{w}: {SWITCH}=0 launched the wide body {res["0"]["counters"][0]} times'
        assert res[None]['counters'][0] == 1, f'{w}: the wide body ran {res[None]["counters"][0]} times'
        assert res['0']['counters'][1:] == res[None]['counters'][1:], f'{w}: {res["0"]["counters"]} / {res[None]["counters"]}'
        if formula:
            assert res[None]['counters'][1:] == old_counters(args), f'{w}: the older counters moved by {res[None]["counters"][1:]}'
        crp.assert_same_bits(res['0'], res[None], w)


def check_golden_case(dev, monkeypatch, name):
    z, meta, args, raw = load_case(name)
    check_bodies_agree(dev, monkeypatch, args, state_dict_for(meta, args), pairs_from_raw(raw), name)


def check_sizes(dev, monkeypatch, sizes, layers):
    args, sd = model_of(dev, layers)
    check_bodies_agree(dev, monkeypatch, args, sd, synthetic.make_pairs(sizes, 13), f'{crp.rows_of(sizes)} rows, {layers} layers',
                       formula=True)


def check_not_eligible(dev, monkeypatch, many_tiles=True):
    """every condition that keeps layer 0's forward chain on k_rowchain (or hands it to another kernel): the new counter stays
    put and the outputs are the bits of the switch-off run"""
    monkeypatch.delenv('EQD_CHAIN_RESIDENT', raising=False)
    small = synthetic.make_pairs([(21, 20), (30, 18)], 13)

    def run(over, pairs, env, layers=3):
        args, sd = model_of(dev, layers, **over)
        for k, v in env.items():
            set_switch(monkeypatch, k, v)
        before = wide_launches()
        names, _, _, outs = crp.forward_counts(dev, args, sd, pairs)
        moved = wide_launches() - before
        for k in env:
            set_switch(monkeypatch, k, None)
        return moved, outs, names

    def stays(over, pairs, env, layers=3):
        moved, outs, names = run(over, pairs, env, layers)
        assert moved == 0, f'{over} {env}: the wide body ran {moved} times'
        moved0, outs0, names0 = run(over, pairs, dict(env, **{SWITCH: '0'}), layers)
        assert moved0 == 0 and names0 == names, (over, env)
        for a, b in zip(outs0, outs):
            assert torch.equal(a, b), f'{over} {env}: bits differ from the {SWITCH}=0 run'
    moved, _, names = run({}, small, {})
    assert moved == 1 and names.count('k_rowchain') == 3      # (the same model and batch with nothing in the way)
    stays({}, small, {'EQD_CHAIN_RESIDENT': '0'})
    stays(dict(cross_msgs=False), small, {})
    stays(dict(hip_storage_dtype='bf16'), small, {})
    stays({}, small, {'EQD_ROW_TILES': '2'})
    stays({}, small, {'EQD_ROWCHAIN_OCC': '1'})
    stays({}, small, {'EQD_ROWWAVE': '1'})
    if many_tiles:      # 4 112 rows: 257 tiles on 256 CUs
        stays({}, synthetic.make_pairs([(250, 7)] * 16, 13), {}, layers=1)


def check_guard_rows(dev, monkeypatch):
    """eqd_node_update_fwd at (d_in, d0) = (69, 69) with cross messages builds layer 0's forward list: on NaN-filled outputs
    with sentinel rows behind them (node_chain_common.run_kernels checks the guards and that every element is written - the
    float64 comparison of tests/test_node_chain_*.py needs it finite), at 37 rows - 5 in the last tile - with dropout
    factors and one all-zero row of them, both bodies write the same bits.  Without aggr_cross (three sources) and at 64
    outputs the list is not the wide body's."""
    monkeypatch.delenv('EQD_CHAIN_RESIDENT', raising=False)
    for cfg_id, rows, drop, want in (('69x69', 37, True, 1), ('69x69', 16, False, 1), ('69x69-nocross', 37, True, 0),
                                     ('64x69', 37, True, 0)):
        case = nc.make_case(nc.CONFIGS[cfg_id], rows, drop=drop)
        res = {}
        for mode in ('0', None):
            set_switch(monkeypatch, SWITCH, mode)
            before = wide_launches()
            got, names_f, _, _ = nc.run_kernels(dev, case, False)
            assert names_f == ['k_rowchain'], names_f
            assert wide_launches() - before == (0 if mode == '0' else want), f'{cfg_id}, {SWITCH}={mode}: which body ran'
            res[mode] = got
        set_switch(monkeypatch, SWITCH, None)
        for k in nc.NAMES_FWD:
            assert bool(torch.isfinite(res[None][k]).all()), f'{cfg_id}: {k} not written everywhere'
            assert torch.equal(res['0'][k], res[None][k]), f'{cfg_id}: {k} differs between the bodies'
        if drop:
            assert bool((res[None]['y_act'][nc.zero_row(case)] == 0).all()), 'y_act of the row with all-zero dropout factors'
