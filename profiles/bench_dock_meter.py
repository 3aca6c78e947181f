"""The evaluation stage of batched docking inference on the MI355X (equidock_public_amd.dock), one JSON line.

For C complexes whose coordinates are on the device (the three real DB5.5 results of tests/golden/eval_case.npz in turn,
copy k under its own seeded rigid motion), per C:

  host_loop_ms    the path this replaces: per complex four downloads and inference.rmsd_metrics +
                  inference.complex_and_interface_rmsd on the host (float32 numpy, LAPACK SVD)
  device_ms       dock.rmsd_metrics_batch (workspace + item-table copy, five launches) and ONE download of the [C][8] rows
  eval_ms         eqd_dock_meter_eval alone on a prepared workspace (dock.MeterPlan.eval), by device events around 20
                  back-to-back calls - what TrainStep(meter=...) adds to graph M
  max_abs_diff    largest |device - host| over the CRMSD / IRMSD of the batch (the two paths measure the same thing)

Medians over --reps alternating repetitions after two warm-ups of each, one process.

usage (GPU box): python profiles/bench_dock_meter.py [--reps R] [--cs 1,4,16,64]
(EQD_DOCK_SMALL=1: dry run on the x86 simulator, no GPU)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from equidock_public_amd import dock as DK, inference as INF  # noqa: E402

_ap = argparse.ArgumentParser()
_ap.add_argument('--reps', type=int, default=15)
_ap.add_argument('--cs', default='1,4,16,64')
ARGS = _ap.parse_args()
SMALL = os.environ.get('EQD_DOCK_SMALL') == '1'
if SMALL:
    from tests import dock_common as _dc
    DK.load_dock_library_for_testing(_dc.build_sim())
dev = torch.device('cpu' if SMALL else 'cuda:0')


def sync():
    if dev.type == 'cuda':
        torch.cuda.synchronize(dev)


def complexes(n):
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'eval_case.npz'))
    names = [str(v) for v in z['names']]
    out = []
    for k in range(n):
        nm = names[k % len(names)]
        rng = np.random.default_rng(k)
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        q = (q * np.sign(np.diag(r))).astype(np.float32)
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        t = rng.uniform(-20.0, 20.0, size=3).astype(np.float32)
        lm, lg, rg = (np.ascontiguousarray(z[f'{nm}_{s}'] @ q.T + t, dtype=np.float32) for s in ('lm', 'lg', 'rg'))
        out.append(tuple(torch.from_numpy(a).to(dev) for a in (lm, lg, rg)))
    return out


def host_loop(cx):
    out = []
    for lm, lg, rg in cx:
        a = [t.detach().cpu().numpy() for t in (lm, rg, lg, rg)]          # the reference's four copies per pair
        out.append(INF.complex_and_interface_rmsd(*a))
    return np.asarray(out, dtype=np.float64)


def device_pass(cx):
    m = DK.rmsd_metrics_batch([c[0] for c in cx], [c[1] for c in cx], [c[2] for c in cx])
    return m['metrics'].cpu().numpy()[:, 2:4]


def eval_alone(cx, calls=20):
    plan = DK.MeterPlan(DK._offsets([c[1].shape[0] for c in cx]), DK._offsets([c[2].shape[0] for c in cx]), dev)
    lp, lt, rt = (torch.cat([c[i] for c in cx], 0) for i in range(3))
    out = torch.empty(len(cx), DK.METER_COLS, dtype=torch.float64, device=dev)
    plan.eval(lp, None, lt, rt, out)
    sync()
    if dev.type != 'cuda':
        t0 = time.perf_counter()
        for _ in range(calls):
            plan.eval(lp, None, lt, rt, out)
        return 1e3 * (time.perf_counter() - t0) / calls
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        plan.eval(lp, None, lt, rt, out)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def med(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def main():
    reps = 3 if SMALL else max(ARGS.reps, 5)
    res = {'metric': 'dock_meter', 'device': 'simulator' if SMALL else torch.cuda.get_device_name(dev), 'reps': reps,
           'by_C': {}}
    for n in ([1, 3] if SMALL else [int(v) for v in ARGS.cs.split(',')]):
        cx = complexes(n)
        t = {'host': [], 'device': [], 'eval': []}
        for rep in range(-2, reps):
            sync()
            t0 = time.perf_counter()
            h = host_loop(cx)
            t1 = time.perf_counter()
            d = device_pass(cx)
            t2 = time.perf_counter()
            e = eval_alone(cx)
            if rep >= 0:
                t['host'].append(t1 - t0)
                t['device'].append(t2 - t1)
                t['eval'].append(e)
        row = {'rows': int(sum(c[0].shape[0] + c[2].shape[0] for c in cx)), 'host_loop_ms': 1e3 * med(t['host']),
               'device_ms': 1e3 * med(t['device']), 'eval_ms': med(t['eval']),
               'host_loop_ms_min_max': [1e3 * min(t['host']), 1e3 * max(t['host'])],
               'device_ms_min_max': [1e3 * min(t['device']), 1e3 * max(t['device'])],
               'max_abs_diff': float(np.abs(h - d).max())}
        row['ratio'] = row['host_loop_ms'] / row['device_ms']
        res['by_C'][str(n)] = row
        print(f"C={n:2d}: " + json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
