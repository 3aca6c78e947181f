"""The docking-quality stage of batched docking inference on the MI355X (equidock_public_amd.dock), one JSON line, also
written to profiles/dock_quality_bench.log (--out).

Workload: seeded residue clouds with the heavy-atom counts of the 25 DB5.5 test complexes
(tests/golden/db5_test_atom_counts.json; residues of 4-14 atoms at protein density, two touching globules; the model is
the native ligand under a seeded rotation of 6 degrees and a shift of 2 A), coordinates on the device.  Per C (the first
C complexes):

  host_loop_ms    per complex three downloads and a vectorised float64 numpy evaluation of the same definitions (all atom
                  pairs at once, np.linalg.svd)
  device_ms       dock.pose_quality_batch (tables upload, workspace + item-table copy, six launches) and ONE download of
                  the [C][16] rows
  eval_ms         eqd_dock_quality_eval alone on a prepared plan (dock.QualityPlan.eval), by device events around 20
                  back-to-back calls
  pruned_share    residue-pair tests the bound pruned / (2 x residue pairs)
  max_abs_diff    largest |device - host| over DockQ, fnat, iRMSD(bb), LRMSD of the batch; the integer columns must agree

Medians over --reps alternating repetitions after two warm-ups of each, one process.

usage (GPU box): python profiles/bench_dock_quality.py [--reps R] [--cs 1,4,16,25] [--out FILE]
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
_ap.add_argument('--reps', type=int, default=15)
_ap.add_argument('--cs', default='1,4,16,25')
_ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dock_quality_bench.log'))
ARGS = _ap.parse_args()
SMALL = os.environ.get('EQD_DOCK_SMALL') == '1'
if SMALL:
    from tests import dock_common as _dc
    DK.load_dock_library_for_testing(_dc.build_sim())
dev = torch.device('cpu' if SMALL else 'cuda:0')
CUTS = (5.0, 10.0, 3.0)


def sync():
    if dev.type == 'cuda':
        torch.cuda.synchronize(dev)


def globule(rng, n_atoms, centre):
    """residues of 4-14 atoms (the last one takes the rest) around centres at ~140 A^3 per residue; backbone = the first four"""
    sizes = []
    while sum(sizes) < n_atoms:
        sizes.append(min(int(rng.integers(4, 15)), n_atoms - sum(sizes)))
    n = len(sizes)
    radius = (140.0 * n * 3.0 / (4.0 * np.pi)) ** (1.0 / 3.0)
    v = rng.standard_normal((n, 3))
    cen = v / np.linalg.norm(v, axis=1, keepdims=True) * radius * rng.uniform(0.0, 1.0, (n, 1)) ** (1.0 / 3.0) + centre
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    x = np.repeat(cen, sizes, axis=0) + rng.standard_normal((n_atoms, 3)) * 1.2
    bb = np.concatenate([np.arange(k) < 4 for k in sizes]).astype(np.uint8)
    return np.ascontiguousarray(x, dtype=np.float32), off, bb, radius


def complexes(n):
    counts = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'db5_test_atom_counts.json')))['complexes']
    out = []
    for k in range(n):
        _, nl, nr = counts[k % len(counts)]
        if SMALL:
            nl, nr = nl // 8, nr // 8
        rng = np.random.default_rng(1000 + k)
        base = np.array([83.0, 72.0, 243.0])
        rt, ro, rbb, rr = globule(rng, nr, base)
        lt, lo, lbb, rl = globule(rng, nl, base)
        lt = (lt + np.float32([rr + rl - 3.0, 0.0, 0.0])).astype(np.float32)        # the globules overlap by 3 A
        ax = rng.standard_normal(3)
        ax /= np.linalg.norm(ax)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        a = np.deg2rad(6.0)
        R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
        c = lt.astype(np.float64).mean(0)
        lp = np.ascontiguousarray((lt - c) @ R.T + c + ax * 2.0, dtype=np.float32)
        out.append(dict(lp=torch.from_numpy(lp).to(dev), lt=torch.from_numpy(lt).to(dev), rt=torch.from_numpy(rt).to(dev),
                        lo=lo, ro=ro, lbb=lbb, rbb=rbb))
    return out


def _kabsch(P, T):
    cp, ct = P.mean(0), T.mean(0)
    U, S, Vt = np.linalg.svd((P - cp).T @ (T - ct))
    R = Vt.T @ U.T
    if np.linalg.det(R) < 0:
        R = (Vt.T @ np.diag([1.0, 1.0, -1.0])) @ U.T
    return R, ct - R @ cp


def _rmsd(R, b, P, T):
    e = P @ R.T + b - T
    return float(np.sqrt(np.mean(np.sum(e * e, axis=1))))


def host_one(lp, lt, rt, lo, ro, lbb, rbb):
    lp, lt, rt = (a.astype(np.float64) for a in (lp, lt, rt))
    lbb, rbb = lbb != 0, rbb != 0

    def dist(a, b):
        out = np.empty((len(a), len(b)))
        for i0 in range(0, len(a), 1024):          # (blocks of ligand rows bound the temporaries)
            d = a[i0:i0 + 1024, None, :] - b[None, :, :]
            out[i0:i0 + 1024] = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        return out

    def pairs(mask):
        return np.logical_or.reduceat(np.logical_or.reduceat(mask, lo[:-1], axis=0), ro[:-1], axis=1)

    dn, dm = dist(lt, rt), dist(lp, rt)
    cn, cm = pairs(dn < CUTS[0]), pairs(dm < CUTS[0])
    N, M, S = int(cn.sum()), int(cm.sum()), int((cn & cm).sum())
    near = pairs(dn < CUTS[1])
    wl, wr = np.repeat(near.any(1), np.diff(lo)) & lbb, np.repeat(near.any(0), np.diff(ro)) & rbb
    fnat = S / N if N else float('nan')
    irmsd = lrmsd = float('nan')
    if wl.any() or wr.any():
        P, T = np.concatenate((lp[wl], rt[wr])), np.concatenate((lt[wl], rt[wr]))
        irmsd = _rmsd(*_kabsch(P, T), P, T)
    if lbb.any() and rbb.any():
        lrmsd = _rmsd(*_kabsch(rt[rbb], rt[rbb]), lp[lbb], lt[lbb])
    dockq = (fnat + 1.0 / (1.0 + (irmsd / 1.5) ** 2) + 1.0 / (1.0 + (lrmsd / 8.5) ** 2)) / 3.0
    return [dockq, fnat, irmsd, lrmsd, N, M, S, int((dm < CUTS[2]).sum())]


def host_loop(cx):
    out = []
    for c in cx:
        lp, lt, rt = (c[k].detach().cpu().numpy() for k in ('lp', 'lt', 'rt'))
        out.append(host_one(lp, lt, rt, c['lo'].astype(np.int64), c['ro'].astype(np.int64), c['lbb'], c['rbb']))
    return np.asarray(out, dtype=np.float64)


def tables(cx):
    return [c['lo'] for c in cx], [c['ro'] for c in cx], [c['lbb'] for c in cx], [c['rbb'] for c in cx]


def device_pass(cx):
    q = DK.pose_quality_batch([c['lp'] for c in cx], [c['lt'] for c in cx], [c['rt'] for c in cx], *tables(cx))
    return q['quality'].cpu().numpy()


def eval_alone(cx, calls=20):
    plan = DK.QualityPlan(*tables(cx), dev)
    lp, lt, rt = (torch.cat([c[k] for c in cx], 0) for k in ('lp', 'lt', 'rt'))
    out = torch.empty(len(cx), DK.QUALITY_COLS, dtype=torch.float64, device=dev)
    plan.eval(lp, None, lt, rt, out)
    sync()
    if dev.type != 'cuda':
        t0 = time.perf_counter()
        for _ in range(calls):
            plan.eval(lp, None, lt, rt, out)
        return 1e3 * (time.perf_counter() - t0) / calls, plan.residue_pairs
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        plan.eval(lp, None, lt, rt, out)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls, plan.residue_pairs


def med(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def main():
    reps = 2 if SMALL else max(ARGS.reps, 5)
    res = {'metric': 'dock_quality', 'device': 'simulator' if SMALL else torch.cuda.get_device_name(dev), 'reps': reps,
           'pruning': DK.quality_pruning_enabled(), 'by_C': {}}
    for n in ([1, 2] if SMALL else [int(v) for v in ARGS.cs.split(',')]):
        cx = complexes(n)
        t = {'host': [], 'device': [], 'eval': []}
        for rep in range(-2, reps):
            sync()
            t0 = time.perf_counter()
            h = host_loop(cx)
            t1 = time.perf_counter()
            d = device_pass(cx)
            t2 = time.perf_counter()
            e, pairs = eval_alone(cx)
            if rep >= 0:
                t['host'].append(t1 - t0)
                t['device'].append(t2 - t1)
                t['eval'].append(e)
        same_ints = bool((h[:, 4:] == d[:, [5, 6, 7, 11]]).all())
        row = {'atoms': int(sum(c['lt'].shape[0] + c['rt'].shape[0] for c in cx)), 'residue_pairs': pairs,
               'host_loop_ms': 1e3 * med(t['host']), 'device_ms': 1e3 * med(t['device']), 'eval_ms': med(t['eval']),
               'host_loop_ms_min_max': [1e3 * min(t['host']), 1e3 * max(t['host'])],
               'device_ms_min_max': [1e3 * min(t['device']), 1e3 * max(t['device'])],
               'pruned_share': float(d[:, 13].sum()) / (2.0 * pairs), 'integer_columns_agree': same_ints,
               'max_abs_diff': float(np.nanmax(np.abs(h[:, :4] - d[:, [0, 1, 3, 4]]))),
               'dockq_min_max': [float(np.nanmin(d[:, 0])), float(np.nanmax(d[:, 0]))]}
        row['ratio'] = row['host_loop_ms'] / row['device_ms']
        res['by_C'][str(n)] = row
        print(f"C={n:2d}: " + json.dumps(row), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    with open(ARGS.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
