"""Checks of the batched exact transport solver on the device (equidock_public_amd.dock.EmdPlan / emd_uniform_batch,
libequidock_dock.so: eqd_dock_emd_*) and of what is built on it (losses.pocket_ot_loss(solver='device'),
train_step.TrainStep(ot_solver='device')), shared by the simulator tests (tests/test_dock_emd_sim.py) and the GPU tests
(tests/test_dock_emd_gpu.py).  The yardstick of every plan is the host solver losses.emd_uniform_host, bit for bit; one
check goes to the independent LP oracle (oracle/ot_port.py)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from equidock_public_amd import dock as DK, losses

K50_ROWS = (1, 2, 23, 25, 37, 49, 50, 63, 64, 65, 100, 127, 128, 129, 150)      # n with K = 50
N40_COLS = (1, 7, 63, 64, 65, 128)                                              # K with n = 40
TIE_SIZES = ((12, 12), (30, 50), (64, 64))
OT_COUNTS, OT_K = (23, 1, 50, 64, 37), 50                                       # parity_common.check_pocket_ot


def host_build():
    from equidock_public_amd import build as B
    B.build_host(verbose=False)                    # the yardstick: libequidock_host.so


def seeded_cost(n, K, seed):
    """sq_dist(pocket_lig, Y_lig) + sq_dist(pocket_rec, Y_rec) with the scales of parity_common.check_pocket_ot"""
    gen = torch.Generator().manual_seed(seed)
    pl, pr = torch.randn(n, 3, generator=gen) * 9, torch.randn(n, 3, generator=gen) * 9 + 2
    yl, yr = torch.randn(K, 3, generator=gen) * 8, torch.randn(K, 3, generator=gen) * 8

    def sq(a, b):
        return ((a.view(n, 1, 3) - b.view(1, K, 3)) ** 2).sum(dim=2)
    return (sq(pl, yl) + sq(pr, yr)).to(torch.float32).contiguous()


def grid_cost(n, K, seed):
    """integer coordinates on a small grid: integer-valued costs, many reduced costs exactly equal"""
    gen = torch.Generator().manual_seed(seed)
    pl, pr = (torch.randint(0, 4, (n, 3), generator=gen).float() for _ in range(2))
    yl, yr = (torch.randint(0, 4, (K, 3), generator=gen).float() for _ in range(2))

    def sq(a, b):
        return ((a.view(n, 1, 3) - b.view(1, K, 3)) ** 2).sum(dim=2)
    return (sq(pl, yl) + sq(pr, yr)).to(torch.float32).contiguous()


def budget_rows(K):
    """the last n whose n x K problem fits the resident body's budget"""
    return DK.EMD_RESIDENT_CELLS // K


@functools.lru_cache(maxsize=None)
def case(name):
    """(counts, K, cost [sum counts, K], the host solver's plans) of a named batch; computed once, never changed"""
    host_build()
    if name == 'k50':                               # K = 50, a problem of 0 rows in mid-batch, the budget's two sides
        nb = budget_rows(50)
        counts = list(K50_ROWS[:7]) + [0] + list(K50_ROWS[7:]) + [nb, nb + 1]
        K = 50
        mats = [seeded_cost(n, K, 100 + i) for i, n in enumerate(counts)]
    elif name.startswith('n40_'):
        K = int(name[4:])
        counts = [40, 40]
        mats = [seeded_cost(40, K, 200 + K), seeded_cost(40, K, 300 + K)]
    elif name.startswith('tie_'):
        n, K = (int(v) for v in name[4:].split('x'))
        counts = [n, n]
        mats = [grid_cost(n, K, 400 + n), grid_cost(n, K, 500 + n)]
    elif name == 'ot':
        counts, K = list(OT_COUNTS), OT_K
        mats = [seeded_cost(n, K, 600 + i) for i, n in enumerate(counts)]
    else:
        raise KeyError(name)
    cost = torch.cat(mats).contiguous()
    plan, _ = losses.emd_uniform_host(cost, counts)
    return counts, K, cost, plan


def _blocks(t, counts):
    off = np.concatenate([[0], np.cumsum(counts)])
    return [t[off[i]:off[i + 1]] for i in range(len(counts))]


def solve(dev, cost, counts, resident):
    plan, status = DK.emd_uniform_batch(cost.to(dev), counts, resident=resident)
    return plan.cpu(), status.cpu().tolist()


def check_against_host(dev, name, resident, alone=True):
    """the batch's plans, and each problem's alone, are the host solver's bit for bit"""
    counts, K, cost, ref = case(name)
    plan, status = solve(dev, cost, counts, resident)
    assert status == [0] * len(counts), status
    for p, (a, b) in enumerate(zip(_blocks(plan, counts), _blocks(ref, counts))):
        assert torch.equal(a, b), f'{name} resident={resident}: problem {p} ({counts[p]} x {K}) differs from the host solver in the batch'
    assert torch.equal(plan, ref)
    if not alone:
        return
    for p, (c, b) in enumerate(zip(_blocks(cost, counts), _blocks(ref, counts))):
        if counts[p] == 0:
            continue
        a, st = solve(dev, c.contiguous(), [counts[p]], resident)
        assert st == [0] and torch.equal(a, b), f'{name} resident={resident}: problem {p} ({counts[p]} x {K}) differs alone'


def check_lp_oracle(dev):
    """the five problems of check_pocket_ot: the plan is within 1e-7 of the LP oracle's (that check's own bound, through
    its `close`: absolute against max(1, |ref|)), row sums within 1e-6 relative of 1 / n, column sums of 1 / K"""
    from oracle import ot_port
    from tests.dock_common import close
    counts, K, cost, _ = case('ot')
    for resident in (True, False):
        plan, status = solve(dev, cost, counts, resident)
        assert status == [0] * len(counts)
        for p, (a, c) in enumerate(zip(_blocks(plan, counts), _blocks(cost, counts))):
            n = counts[p]
            lp = ot_port.emd_lp(np.ones(n) / n, np.ones(K) / K, c.numpy())
            close(a, lp, 1e-7, f'plan of problem {p} against the LP oracle')
            rows, cols = a.double().sum(1).numpy(), a.double().sum(0).numpy()
            assert np.abs(rows - 1.0 / n).max() <= 1e-6 / n, (p, np.abs(rows * n - 1).max())
            assert np.abs(cols - 1.0 / K).max() <= 1e-6 / K, (p, np.abs(cols * K - 1).max())


def check_bits(dev):
    """a problem's plan is identical alone, first, last, in a permuted batch and from run to run"""
    counts, K, cost, ref = case('ot')
    cb, rb = _blocks(cost, counts), _blocks(ref, counts)
    q = 3                                              # the 64 x 50 problem
    orders = ([q], [q, 0, 1, 2, 4], [0, 1, 2, 4, q], [4, 2, q, 0, 1], [4, 2, q, 0, 1])
    for resident in (True, False):
        for order in orders:
            cs = [counts[i] for i in order]
            plan, status = solve(dev, torch.cat([cb[i] for i in order]).contiguous(), cs, resident)
            assert status == [0] * len(order)
            for i, a in zip(order, _blocks(plan, cs)):
                assert torch.equal(a, rb[i]), (resident, order, i)


def check_status(dev):
    """one all-NaN matrix in mid-batch: status 1 and a NaN plan for it, the others unchanged; EmdPlan.failed() names it"""
    counts, K, cost, ref = case('ot')
    off = np.concatenate([[0], np.cumsum(counts)])
    bad = cost.clone()
    bad[off[2]:off[3]] = float('nan')
    for resident in (True, False):
        ep = DK.EmdPlan(counts, K, dev)
        plan = torch.full_like(bad, 7.0).to(dev)
        ep.solve(bad.to(dev), plan, resident=resident)
        assert ep.failed() == [2]
        assert ep.status.cpu().tolist() == [0, 0, 1, 0, 0]
        plan = plan.cpu()
        assert bool(torch.isnan(plan[off[2]:off[3]]).all())
        for p in (0, 1, 3, 4):
            assert torch.equal(plan[off[p]:off[p + 1]], ref[off[p]:off[p + 1]]), p
        ep.solve(cost.to(dev), plan.to(dev), resident=resident)          # the status is rewritten by every solve
        assert ep.failed() == []


def check_validation_errors(dev):
    """the C ABI's validation: each error returns its code and message, and nothing is launched (buffers untouched)"""
    lib = DK.load_dock_library()

    def offs(v):
        return np.ascontiguousarray(np.asarray(v, dtype=np.int32))

    def vp(a):
        return a.ctypes.data_as(C.c_void_p)

    good = offs([0, 4, 4, 9])
    wsb = lib.eqd_dock_emd_workspace_bytes(3, vp(good), 5)
    assert wsb > 0
    for bad_off, P, m, msg in ((offs([1, 4, 9, 9]), 3, 5, b'src_off[0] = 1'), (offs([0, 6, 4, 9]), 3, 5, b'problem 1 has -2 rows'),
                               (good, 3, 0, b'n_snk = 0'), (good, 0, 5, b'n_problems = 0'),
                               (offs([0, 4, DK.EMD_MAX_NODES]), 2, 5, b'EQD_DOCK_EMD_MAX_NODES')):
        assert lib.eqd_dock_emd_workspace_bytes(P, vp(bad_off), m) == 0
        assert msg in lib.eqd_dock_last_error(), lib.eqd_dock_last_error()
    assert lib.eqd_dock_emd_workspace_bytes(3, None, 5) == 0 and b'NULL offsets' in lib.eqd_dock_last_error()
    # the largest problem the library takes: n + m == EQD_DOCK_EMD_MAX_NODES
    assert lib.eqd_dock_emd_workspace_bytes(1, vp(offs([0, DK.EMD_MAX_NODES - 5])), 5) > 0
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    cost = torch.ones(9, 5, device=dev)
    plan = torch.full((9, 5), 7.0, device=dev)
    status = torch.full((3,), 3, dtype=torch.int32, device=dev)
    st = DK._stream(dev)
    p = lambda t: C.c_void_p(t.data_ptr())

    def init(o, P, m, w, size):
        return lib.eqd_dock_emd_init(P, vp(o) if o is not None else None, m, w, C.c_size_t(size), st)

    def run(o, P, m, c, pl, s, w, size):
        return lib.eqd_dock_emd_solve(P, vp(o) if o is not None else None, m, c, pl, s, 1, w, C.c_size_t(size), st)

    assert init(None, 3, 5, p(ws), wsb) == 1
    assert init(good, 3, 5, None, wsb) == 1 and b'NULL workspace' in lib.eqd_dock_last_error()
    assert init(offs([0, 6, 4, 9]), 3, 5, p(ws), wsb) == 2
    assert init(good, 3, 5, p(ws), 64) == 4 and b'workspace too small' in lib.eqd_dock_last_error()
    full = (good, 3, 5, p(cost), p(plan), p(status), p(ws), wsb)
    for k in (3, 4, 5, 6):                              # cost, plan, status, workspace
        a = list(full)
        a[k] = None
        assert run(*a) == 1, k
    assert run(None, 3, 5, p(cost), p(plan), p(status), p(ws), wsb) == 1
    assert run(offs([1, 4, 9, 9]), 3, 5, p(cost), p(plan), p(status), p(ws), wsb) == 2
    assert run(offs([0, 6, 4, 9]), 3, 5, p(cost), p(plan), p(status), p(ws), wsb) == 2
    assert run(good, 3, 0, p(cost), p(plan), p(status), p(ws), wsb) == 2
    assert run(offs([0, 4, 4, DK.EMD_MAX_NODES]), 3, 5, p(cost), p(plan), p(status), p(ws), wsb) == 2
    assert b'EQD_DOCK_EMD_MAX_NODES' in lib.eqd_dock_last_error()
    assert run(good, 3, 5, p(cost), p(plan), p(status), p(ws), 64) == 4
    # nothing was written by the refused calls
    assert bool((plan.cpu() == 7.0).all()) and status.cpu().tolist() == [3, 3, 3] and bool((ws.cpu() == 0).all())
    # Python: the shapes EmdPlan.solve takes
    ep = DK.EmdPlan([4, 0, 5], 5, dev)
    with pytest.raises(ValueError, match='contiguous float32'):
        ep.solve(cost[:8], plan[:8])
    with pytest.raises(ValueError, match='counts'):
        DK.emd_uniform_batch(cost, [4, 4])
    with pytest.raises(RuntimeError, match='EQD_DOCK_EMD_MAX_NODES'):
        DK.EmdPlan([DK.EMD_MAX_NODES], 5, dev)
    # ... and the pair (init, solve) on the good sizes runs: the 0-row problem writes no plan row and status 0
    ep.solve(cost, plan)
    assert ep.failed() == [] and bool(torch.isfinite(plan.cpu()).all())


def pocket_inputs():
    """the inputs of parity_common.check_pocket_ot"""
    gen = torch.Generator().manual_seed(17)
    counts, K = list(OT_COUNTS), OT_K
    B = len(counts)
    pls = [torch.randn(n, 3, generator=gen) * 9 for n in counts]
    prs = [torch.randn(n, 3, generator=gen) * 9 + 2 for n in counts]
    Yl, Yr = torch.randn(B, K, 3, generator=gen) * 8, torch.randn(B, K, 3, generator=gen) * 8
    return pls, prs, Yl, Yr, torch.tensor([1.0, 0.5, 2.0, 1.5, 0.25])


def check_pocket_ot_loss(dev, monkeypatch=None):
    """pocket_ot_loss(solver='device'): ot, the plan and both keypoint gradients bit-equal to solver='host' on the
    check_pocket_ot inputs.  With `monkeypatch` the device call runs with losses._emd_lib patched to raise: the host
    solver is never called."""
    host_build()
    pls, prs, Yl, Yr, w = pocket_inputs()

    def run(**kw):
        a, b = Yl.clone().to(dev).requires_grad_(True), Yr.clone().to(dev).requires_grad_(True)
        ot, plan = losses.pocket_ot_loss(a, b, pls, prs, return_plan=True, **kw)
        (ot * w.to(ot.device)).sum().backward()
        return [t.detach().cpu() for t in (ot, plan, a.grad, b.grad)]

    host = run()
    if monkeypatch is not None:
        def refuse():
            raise AssertionError('the host solver was asked for')
        monkeypatch.setattr(losses, '_emd_lib', refuse)
    device = run(solver='device')
    reuse = run(solver='device', emd_plan=DK.EmdPlan(list(OT_COUNTS), OT_K, dev))
    if monkeypatch is not None:
        monkeypatch.undo()
    for nm, h, d, r in zip(('ot', 'plan', 'd Y_lig', 'd Y_rec'), host, device, reuse):
        assert torch.equal(h, d) and torch.equal(h, r), f'pocket_ot_loss: {nm} differs between the solvers'
    assert bool(torch.isfinite(host[0]).all()) and float(host[2].abs().max()) > 0
    with pytest.raises(ValueError, match='solver'):
        losses.pocket_ot_loss(Yl.to(dev), Yr.to(dev), pls, prs, solver='gpu')
    with pytest.raises(ValueError, match='EmdPlan holds'):
        losses.pocket_ot_loss(Yl.to(dev), Yr.to(dev), pls, prs, solver='device', emd_plan=DK.EmdPlan([3], OT_K, dev))


# ---- TrainStep(ot_solver='device') ----------------------------------------------------------------------------------
TRAIN_SIZES = ((41, 57), (66, 38), (120, 90), (23, 75))      # the 4-pair ragged batch of parity_common.check_train_step_forms
SIM_SIZES = ((21, 37), (46, 18), (33, 40), (13, 25))         # its small form on the simulator (tests/test_sim_parity.py)


def _bits(ts, loss):
    return loss.detach().cpu().numpy().tobytes(), ts.reducer.flat.detach().cpu().numpy().tobytes()


def check_train_step(dev, meter=False, bf16=False, dropout=0.0, replays=3):
    """TrainStep(ot_solver='device') against TrainStep(ot_solver='host') on the same batch and weights: loss and flat
    gradient bit-equal, host-enqueued and through step_eager; on the GPU also after capture() - ONE graph - over
    `replays` replays with the weights perturbed between them: after each, the plan buffer is emd_uniform_host of that
    replay's cost buffer, and at least one plan changed."""
    from equidock_public_amd import _lib, train_step as TS
    from tests import parity_common as pc
    host_build()
    gpu = torch.device(dev).type == 'cuda'
    sizes = TRAIN_SIZES if gpu else SIM_SIZES
    args = pc.port.default_args(iegmn_n_lays=2 if gpu else 1, skip_weight_h=0.75)
    if dropout:
        args = dict(pc.port.default_args(iegmn_n_lays=2 if gpu else 1, skip_weight_h=0.75, dropout=dropout),
                    hip_dropout_masks='library')
    sd = pc.port.init_state_dict(args, seed=17, rot_scale=40.0)
    g, lig_t, rec_t, pl, pr = pc.training_batch(sizes, 17, dev)
    B = len(sizes)

    def make(solver):
        net = pc.build_model(dict(args, hip_storage_dtype='bf16') if bf16 else args, sd, dev)
        if dropout:
            net.train(True)
        m = DK.DeviceMeter() if meter else None
        ts = TS.TrainStep(net, g, torch.cat(lig_t), torch.cat(rec_t), pl, pr, w_ot=pc.TRAIN_W_OT, w_int=pc.TRAIN_W_INT,
                          sigma=pc.TRAIN_SIGMA, surface_ct=pc.TRAIN_SURFACE_CT, meter=m, ot_solver=solver)
        return net, ts, m

    def run(ts, fn):
        torch.manual_seed(5)                             # (library-drawn dropout masks follow the generator)
        loss = fn()
        pc.sync(dev)
        return _bits(ts, loss)

    (net_h, host, meter_h), (net_d, device, meter_d) = make('host'), make('device')
    assert not hasattr(device, 'cost_host') and not hasattr(device, 'plan_host') and device._ev is None
    want = run(host, host.step_unfused)
    assert np.isfinite(np.frombuffer(want[0], dtype=np.float32)).all()
    assert run(device, device.step_unfused) == want, 'host-enqueued: the device solver changes the loss or the gradient'
    assert torch.equal(device.plan.cpu(), host.plan.cpu()) and device.ot_failed() == []
    assert run(device, device.step_eager) == run(host, host.step_eager), 'step_eager(solver) differs'
    assert run(device, lambda: device.step_eager(solver='host')) == run(host, host.step_eager)
    with pytest.raises(RuntimeError, match='no host gap'):
        device.last_ot_exposed_ms()
    with pytest.raises(RuntimeError, match='ot_failed'):
        host.ot_failed()
    with pytest.raises(ValueError, match='ot_solver'):
        TS.TrainStep(net_h, g, torch.cat(lig_t), torch.cat(rec_t), pl, pr, ot_solver='gpu')
    if gpu:
        host.capture()
        device.capture()                                 # succeeds: no synchronisation and no host copy is left in the step
        assert len(device._graphs) == 1 and len(host._graphs) == 3
        plans = []
        for rep in range(replays):
            if rep:
                with torch.no_grad():
                    for (_, a), (_, b) in zip(net_h.named_parameters(), net_d.named_parameters()):
                        noise = torch.randn(a.shape, generator=torch.Generator().manual_seed(40 + rep)).to(dev) * 0.02
                        a.add_(noise * a.abs())
                        b.copy_(a)
            want = run(host, host.step)
            assert run(device, device.step) == want, f'replay {rep}: the device solver changes the loss or the gradient'
            ref, _ = losses.emd_uniform_host(device.cost.cpu(), device.counts)
            assert torch.equal(device.plan.cpu(), ref), f'replay {rep}: the plan buffer is not the host solver\'s plan'
            assert device.ot_failed() == []
            plans.append(ref)
        if replays > 1:
            assert any(not torch.equal(plans[0], q) for q in plans[1:]), 'the perturbed weights changed no plan'
    if meter:
        assert len(meter_d) == len(meter_h) > 0
        assert meter_d.rows().tobytes() == meter_h.rows().tobytes()
