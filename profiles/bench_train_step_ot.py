"""The training step with the transport plans solved on the host against on the device (TrainStep(ot_solver=...)), and the
solve alone, on the MI355X; one JSON line (profiles/train_step_ot_bench.log keeps the output).

Part 1, per workload (B fp32: 8 pairs x (200, 200), 8 layers; C bf16: 64 pairs x (300, 300), 8 layers; 30 pocket points per
pair, bench.py's time_train_step setting): two TrainStep objects on the same weights and batch, ot_solver='host' and
'device', each measured captured (`step`) and host-enqueued (`step_unfused`): ms per step over --steps steps per
repetition, --reps alternating repetitions (host, device, host, ...) after two warm-up repetitions; medians and ranges.

Part 2, the solve alone: eqd_dock_emd_solve on a prepared workspace (dock.EmdPlan.solve) by device events around 20
back-to-back calls, for 8 and 64 problems of 30 x 50 and for 64 problems of 12 .. 200 rows x 50, resident and general
body; beside it the wall time of the host solver (eqd_host_emd_uniform, pinned buffer to pinned buffer: what
TrainStep._solve_on_host does) on the same matrices.

The host solver runs on --host-threads threads (default 16: what a command gets on a shared MI355X machine; the
library's own default, min(problems, hardware threads / 2, 64), would size its pool from the whole box), in the solve
timings and in the host-mode TrainStep alike.

usage (GPU box): python profiles/bench_train_step_ot.py [--reps R] [--steps S] [--workloads B,C] [--host-threads T]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from equidock_public_amd import config, dock as DK, graph, losses, model, synthetic, train_step as TS  # noqa: E402

_ap = argparse.ArgumentParser()
_ap.add_argument('--reps', type=int, default=7)
_ap.add_argument('--steps', type=int, default=20)
_ap.add_argument('--workloads', default='B,C')
_ap.add_argument('--host-threads', type=int, default=16)
ARGS = _ap.parse_args()
dev = torch.device('cuda:0')
WORKLOADS = {'B': (8, (200, 200), 8, 'f32'), 'C': (64, (300, 300), 8, 'bf16')}      # pairs, sizes, layers, storage
N_POCKET, K = 30, 50


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {'median': round(float(np.median(v)), 4), 'min': round(float(v.min()), 4), 'max': round(float(v.max()), 4)}


def make_steps(name):
    ppg, sizes, L, dtype = WORKLOADS[name]
    args = config.published_args(iegmn_n_lays=L, shared_layers=False, skip_weight_h=0.75, device=dev)
    if dtype == 'bf16':
        args['hip_storage_dtype'] = 'bf16'
    sd = config.seeded_state_dict(args, seed=0)
    pairs = synthetic.make_pairs([sizes] * ppg, seed=1000)
    g = graph.batch_pairs(pairs).to(dev)
    rng = np.random.default_rng(77)
    lig_t = torch.cat([torch.from_numpy(p[0]['x']) for p in pairs])
    rec_t = torch.cat([torch.from_numpy(p[1]['x']) for p in pairs])
    pl, pr = [], []
    for lig, rec in pairs:
        n = min(N_POCKET, lig['x'].shape[0], rec['x'].shape[0])
        pl.append(torch.from_numpy(lig['new_x'][rng.permutation(lig['x'].shape[0])[:n]].copy()))
        pr.append(torch.from_numpy(rec['x'][rng.permutation(rec['x'].shape[0])[:n]].copy()))
    out = {}
    for solver in ('host', 'device'):
        net = model.Rigid_Body_Docking_Net(args).to(dev)
        net.load_state_dict(sd)
        net.train(True)
        out[solver] = TS.TrainStep(net, g, lig_t, rec_t, pl, pr, ot_solver=solver, n_threads=min(ARGS.host_threads, ppg))
    return ppg, out


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def bench_steps(name, reps, steps):
    ppg, ts = make_steps(name)
    row = {'pairs': ppg, 'pocket_points_per_pair': N_POCKET, 'steps_per_repetition': steps, 'repetitions': reps}
    for form in ('unfused', 'captured'):
        if form == 'captured':
            for t in ts.values():
                t.capture()
        fns = {s: (t.step if form == 'captured' else t.step_unfused) for s, t in ts.items()}
        ms = {'host': [], 'device': []}
        for rep in range(-2, reps):
            for s in ('host', 'device'):
                v = timed(fns[s], steps)
                if rep >= 0:
                    ms[s].append(v)
        lh, ld = float(fns['host']()), float(fns['device']())
        torch.cuda.synchronize()
        same = (lh == ld and torch.equal(ts['host'].reducer.flat, ts['device'].reducer.flat)
                and torch.equal(ts['host'].plan, ts['device'].plan))
        row[form] = {'host_ms': stats(ms['host']), 'device_ms': stats(ms['device']),
                     'host_pairs_per_s': round(ppg * 1e3 / np.median(ms['host']), 1),
                     'device_pairs_per_s': round(ppg * 1e3 / np.median(ms['device']), 1),
                     'device_over_host_time': round(float(np.median(ms['device']) / np.median(ms['host'])), 4),
                     'loss_gradient_plan_bits_equal': bool(same), 'failed_problems': ts['device'].ot_failed()}
        print(f"{name} {form}: " + json.dumps(row[form]), file=sys.stderr, flush=True)
    ex = []
    for _ in range(10):
        ts['host'].step()
        ex.append(ts['host'].last_ot_exposed_ms())
    row['host_ot_exposed_ms'] = stats(ex)
    return row


def seeded_cost(counts, seed):
    gen = torch.Generator().manual_seed(seed)
    mats = []
    for n in counts:
        pl, pr = torch.randn(n, 3, generator=gen) * 9, torch.randn(n, 3, generator=gen) * 9 + 2
        yl, yr = torch.randn(K, 3, generator=gen) * 8, torch.randn(K, 3, generator=gen) * 8
        mats.append(torch.cdist(pl, yl) ** 2 + torch.cdist(pr, yr) ** 2)
    return torch.cat(mats).to(torch.float32).contiguous()


def bench_solve(counts, reps, calls=20):
    cost_h = seeded_cost(counts, 9).pin_memory()
    plan_h = torch.empty_like(cost_h).pin_memory()
    ns = torch.tensor(counts, dtype=torch.int32)
    vals = torch.empty(len(counts), dtype=torch.float64)
    lib = losses._emd_lib()
    cost = cost_h.to(dev)
    plan = torch.empty_like(cost)
    ep = DK.EmdPlan(counts, K, dev)
    t = {'resident': [], 'general': [], 'host': []}
    for rep in range(-2, reps):
        for body in ('resident', 'general'):
            ep.solve(cost, plan, resident=body == 'resident')
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                ep.solve(cost, plan, resident=body == 'resident')
            e1.record()
            e1.synchronize()
            if rep >= 0:
                t[body].append(e0.elapsed_time(e1) / calls)
        t0 = time.perf_counter()
        rc = lib.eqd_host_emd_uniform(len(counts), C.c_void_p(ns.data_ptr()), K, C.c_void_p(cost_h.data_ptr()),
                                      C.c_void_p(plan_h.data_ptr()), C.c_void_p(vals.data_ptr()),
                                      min(ARGS.host_threads, len(counts)))
        if rep >= 0:
            t['host'].append(1e3 * (time.perf_counter() - t0))
        assert rc == 0
    same = torch.equal(plan.cpu(), plan_h) and ep.failed() == []
    return {'problems': len(counts), 'rows_min_max': [int(min(counts)), int(max(counts))], 'device_resident_ms': stats(t['resident']),
            'device_general_ms': stats(t['general']), 'host_solver_wall_ms': stats(t['host']), 'plans_bit_equal': bool(same)}


def main():
    reps = max(ARGS.reps, 3)
    res = {'metric': 'train_step_ot', 'device': torch.cuda.get_device_name(dev), 'host_cpus': len(os.sched_getaffinity(0)),
           'host_solver_threads': ARGS.host_threads, 'steps': {}, 'solve': {}}
    for name in [w for w in ARGS.workloads.split(',') if w]:
        res['steps'][name] = bench_steps(name, reps, ARGS.steps)
    rng = np.random.default_rng(5)
    for tag, counts in (('8 x (30 x 50)', [30] * 8), ('64 x (30 x 50)', [30] * 64),
                        ('64 x (12..200 x 50)', [int(v) for v in rng.integers(12, 201, size=64)])):
        res['solve'][tag] = bench_solve(counts, reps)
        print(f"solve {tag}: " + json.dumps(res['solve'][tag]), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
