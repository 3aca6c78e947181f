"""The lDDT stage of batched docking evaluation on the MI355X (equidock_public_amd.dock.lddt_batch), one JSON line, also
written to profiles/dock_lddt_bench.log (--out).

Workload: seeded residue clouds with the heavy-atom counts of the 25 DB5.5 test complexes
(tests/golden/db5_test_atom_counts.json; built as profiles/bench_dock_surface.py builds them: residues of 4-14 atoms at
protein density, two touching globules), coordinates on the device; the model's ligand is the native's turned by 0.3 rad,
moved by ~3 A and jittered by 0.5 A per atom, the model's receptor is the native's.  Radius 15 A, thresholds 0.5 / 1 / 2 /
4 A.  Per C (the first C complexes):

  host_loop_ms    per complex three downloads and a float64 numpy evaluation of the same definitions: the dense distance
                  matrix of the native in row blocks, the model distance of the included pairs, the threshold decisions,
                  the integer sums (--host-reps repetitions, three for C = 1: the 25 complexes hold 6.9e8 ordered atom
                  pairs)
  device_ms       dock.lddt_batch (tables upload, workspace + item-table copy, four launches) and ONE download of the
                  [C][16] rows
  eval_ms         eqd_dock_lddt_eval alone on a prepared plan (dock.LddtPlan.eval), by device events around 20
                  back-to-back calls
  skipped_share   ordered block pairs the bound skips / all ordered block pairs (column 14)
  integers_agree  columns 4-13 of the device rows equal the host's integers; the scores are then the same quotients

Medians over --reps repetitions of the device pass after two warm-ups, one process.

usage (GPU box): python profiles/bench_dock_lddt.py [--reps R] [--host-reps H] [--cs 1,25] [--out FILE]
(EQD_DOCK_SMALL=1: dry run on the x86 simulator at reduced sizes, no GPU)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from equidock_public_amd import dock as DK  # noqa: E402

_ap = argparse.ArgumentParser()
_ap.add_argument('--reps', type=int, default=5)
_ap.add_argument('--host-reps', type=int, default=1)
_ap.add_argument('--cs', default='1,25')
_ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dock_lddt_bench.log'))
ARGS = _ap.parse_args()
SMALL = os.environ.get('EQD_DOCK_SMALL') == '1'
if SMALL:
    from tests import dock_common as _dc
    DK.load_dock_library_for_testing(_dc.build_sim())
dev = torch.device('cpu' if SMALL else 'cuda:0')
RADIUS, THRESHOLDS = 15.0, (0.5, 1.0, 2.0, 4.0)


def sync():
    if dev.type == 'cuda':
        torch.cuda.synchronize(dev)


def globule(rng, n_atoms, centre):
    """residues of 4-14 atoms (the last one takes the rest) around centres at ~140 A^3 per residue"""
    sizes = []
    while sum(sizes) < n_atoms:
        sizes.append(min(int(rng.integers(4, 15)), n_atoms - sum(sizes)))
    n = len(sizes)
    radius = (140.0 * n * 3.0 / (4.0 * np.pi)) ** (1.0 / 3.0)
    v = rng.standard_normal((n, 3))
    cen = v / np.linalg.norm(v, axis=1, keepdims=True) * radius * rng.uniform(0.0, 1.0, (n, 1)) ** (1.0 / 3.0) + centre
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    x = np.repeat(cen, sizes, axis=0) + rng.standard_normal((n_atoms, 3)) * 1.2
    return np.ascontiguousarray(x, dtype=np.float32), off, radius


def complexes(n):
    counts = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'db5_test_atom_counts.json')))['complexes']
    out = []
    for k in range(n):
        _, nl, nr = counts[k % len(counts)]
        if SMALL:
            nl, nr = nl // 8, nr // 8
        rng = np.random.default_rng(1000 + k)
        base = np.array([83.0, 72.0, 243.0])
        rx, ro, rr = globule(rng, nr, base)
        lx, lo, rl = globule(rng, nl, base)
        lx = (lx + np.float32([rr + rl - 3.0, 0.0, 0.0])).astype(np.float32)        # the globules overlap by 3 A
        ax = rng.standard_normal(3)
        ax /= np.linalg.norm(ax)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        R = np.eye(3) + np.sin(0.3) * K + (1 - np.cos(0.3)) * (K @ K)
        c = lx.astype(np.float64).mean(0)
        lp = (lx.astype(np.float64) - c) @ R.T + c + rng.standard_normal(3) * 1.7 + rng.standard_normal(lx.shape) * 0.5
        out.append(dict(lig_pred=torch.from_numpy(np.ascontiguousarray(lp, dtype=np.float32)).to(dev),
                        lig=torch.from_numpy(lx).to(dev), rec=torch.from_numpy(rx).to(dev), lo=lo, ro=ro))
    return out


def _dist(a, b):
    dx, dy, dz = a[:, None, 0] - b[None, :, 0], a[:, None, 1] - b[None, :, 1], a[:, None, 2] - b[None, :, 2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def host_one(lig_pred, lig, rec, lo, ro):
    """[N all, N inter, P_k all, P_k inter] (int64 [10]) of one complex"""
    xn = np.concatenate((lig, rec)).astype(np.float64)
    xm = np.concatenate((lig_pred, rec)).astype(np.float64)
    nl, n = len(lig), len(xn)
    first = np.concatenate((lo[:-1].astype(np.int64), ro[:-1].astype(np.int64) + nl))
    resid = np.repeat(np.arange(len(first)), np.diff(np.concatenate((first, [n]))))
    side = np.arange(n) >= nl
    tot = np.zeros(10, dtype=np.int64)
    for i0 in range(0, n, 256):                     # (row blocks bound the temporaries: one complex has 20 058 atoms)
        i1 = min(i0 + 256, n)
        dn = _dist(xn[i0:i1], xn)
        inc = (dn < RADIUS) & (resid[i0:i1, None] != resid[None, :])
        r, c = np.nonzero(inc)                      # the model distance only for the included pairs
        e = xm[i0 + r] - xm[c]
        diff = np.abs(np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]) - dn[r, c])
        inter = side[i0 + r] != side[c]
        tot[0] += len(r)
        tot[1] += int(inter.sum())
        for k, t in enumerate(THRESHOLDS):
            ok = diff < t
            tot[2 + k] += int(ok.sum())
            tot[6 + k] += int((ok & inter).sum())
    return tot


def host_loop(cx):
    return np.asarray([host_one(c['lig_pred'].detach().cpu().numpy(), c['lig'].detach().cpu().numpy(),
                                c['rec'].detach().cpu().numpy(), c['lo'], c['ro']) for c in cx], dtype=np.int64)


def device_pass(cx):
    s = DK.lddt_batch([c['lig_pred'] for c in cx], [c['lig'] for c in cx], [c['rec'] for c in cx], [c['lo'] for c in cx],
                      [c['ro'] for c in cx], inclusion_radius=RADIUS, thresholds=THRESHOLDS)
    return s['rows'].cpu().numpy()


def eval_alone(cx, calls=20):
    plan = DK.LddtPlan([c['lo'] for c in cx], [c['ro'] for c in cx], dev)
    lp, lt, rt = (torch.cat([c[k] for c in cx], 0) for k in ('lig_pred', 'lig', 'rec'))
    out = plan.outputs()
    plan.eval(lp, None, lt, rt, *out, inclusion_radius=RADIUS, thresholds=THRESHOLDS)
    sync()
    if dev.type != 'cuda':
        t0 = time.perf_counter()
        plan.eval(lp, None, lt, rt, *out, inclusion_radius=RADIUS, thresholds=THRESHOLDS)
        return 1e3 * (time.perf_counter() - t0), plan.atom_pairs
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        plan.eval(lp, None, lt, rt, *out, inclusion_radius=RADIUS, thresholds=THRESHOLDS)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls, plan.atom_pairs


def med(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def main():
    reps = 1 if SMALL else max(ARGS.reps, 3)
    res = {'metric': 'dock_lddt', 'device': 'simulator' if SMALL else torch.cuda.get_device_name(dev), 'reps': reps,
           'host_reps': max(ARGS.host_reps, 1), 'radius': RADIUS, 'thresholds': list(THRESHOLDS),
           'pruning': DK.lddt_pruning_enabled(), 'by_C': {}}
    for n in ([1, 2] if SMALL else [int(v) for v in ARGS.cs.split(',')]):
        cx = complexes(n)
        t = {'host': [], 'device': [], 'eval': []}
        for _ in range(max(ARGS.host_reps, 3 if n == 1 else 1)):
            sync()
            t0 = time.perf_counter()
            h = host_loop(cx)
            t['host'].append(time.perf_counter() - t0)
        for rep in range(-2, reps):
            sync()
            t1 = time.perf_counter()
            d = device_pass(cx)
            t2 = time.perf_counter()
            e, pairs = eval_alone(cx)
            if rep >= 0:
                t['device'].append(t2 - t1)
                t['eval'].append(e)
        blocks = [-(-c['lig'].shape[0] // DK.LDDT_BLOCK) - (-c['rec'].shape[0] // DK.LDDT_BLOCK) for c in cx]
        row = {'atoms': int(sum(c['lig'].shape[0] + c['rec'].shape[0] for c in cx)), 'atom_pairs': pairs,
               'included_pairs': int(d[:, 4].sum()), 'host_loop_ms': 1e3 * med(t['host']), 'device_ms': 1e3 * med(t['device']),
               'eval_ms': med(t['eval']), 'device_ms_min_max': [1e3 * min(t['device']), 1e3 * max(t['device'])],
               'skipped_share': float(d[:, 14].sum()) / float(sum(b * b for b in blocks)),
               'integers_agree': bool((h == d[:, 4:14].astype(np.int64)).all()),
               'lddt_min_max': [float(np.nanmin(d[:, 0])), float(np.nanmax(d[:, 0]))],
               'ilddt_min_max': [float(np.nanmin(d[:, 1])), float(np.nanmax(d[:, 1]))]}
        row['ratio'] = row['host_loop_ms'] / row['device_ms']
        res['by_C'][str(n)] = row
        print(f"C={n:2d}: " + json.dumps(row), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    with open(ARGS.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
