"""The surface stage of batched docking evaluation on the MI355X (equidock_public_amd.dock.surface_area_batch), one JSON
line, also written to profiles/dock_surface_bench.log (--out).

Workload: seeded residue clouds with the heavy-atom counts of the 25 DB5.5 test complexes
(tests/golden/db5_test_atom_counts.json; residues of 4-14 atoms at protein density, two touching globules, radii drawn
from the four table values), coordinates on the device, 96 sphere points, probe 1.4 A.  Per C (the first C complexes):

  host_loop_ms    per complex two downloads and a float64 numpy evaluation of the same definitions: centre distances in
                  row blocks, the partners under the skip rule, then per atom the exact point test on its partners
  device_ms       dock.surface_area_batch (tables upload, workspace + item-table copy, five launches) and ONE download of
                  the [C][12] rows
  eval_ms         eqd_dock_sasa_eval alone on a prepared plan (dock.SurfacePlan.eval), by device events around 20
                  back-to-back calls
  skipped_share   partner tests the skip rule leaves out / all ordered atom pairs of the complexes (counted on the host)
  max_abs_diff    largest |device - host| over the area columns 0-5 of the batch; the integer columns must agree

Medians over --reps alternating repetitions after two warm-ups of each, one process.

usage (GPU box): python profiles/bench_dock_surface.py [--reps R] [--cs 1,4,16,25] [--out FILE]
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
_ap.add_argument('--cs', default='1,4,16,25')
_ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dock_surface_bench.log'))
ARGS = _ap.parse_args()
SMALL = os.environ.get('EQD_DOCK_SMALL') == '1'
if SMALL:
    from tests import dock_common as _dc
    DK.load_dock_library_for_testing(_dc.build_sim())
dev = torch.device('cpu' if SMALL else 'cuda:0')
PROBE, POINTS = 1.4, 96
RADII = np.float32([1.70, 1.55, 1.52, 1.80])


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
    return np.ascontiguousarray(x, dtype=np.float32), off, rng.choice(RADII, n_atoms).astype(np.float32), radius


def complexes(n):
    counts = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'db5_test_atom_counts.json')))['complexes']
    out = []
    for k in range(n):
        _, nl, nr = counts[k % len(counts)]
        if SMALL:
            nl, nr = nl // 8, nr // 8
        rng = np.random.default_rng(1000 + k)
        base = np.array([83.0, 72.0, 243.0])
        rx, ro, rrad, rr = globule(rng, nr, base)
        lx, lo, lrad, rl = globule(rng, nl, base)
        lx = (lx + np.float32([rr + rl - 3.0, 0.0, 0.0])).astype(np.float32)        # the globules overlap by 3 A
        out.append(dict(lig=torch.from_numpy(lx).to(dev), rec=torch.from_numpy(rx).to(dev), lo=lo, ro=ro, lrad=lrad, rrad=rrad))
    return out


SPHERE = DK.sphere_points(POINTS)


def host_one(lig, rec, lrad, rrad):
    """([sasa ligand, sasa receptor, sasa complex, bsa, bsa ligand, bsa receptor, buried atoms ligand, buried atoms
    receptor, points alone, points in complex], partners kept)"""
    x = np.concatenate((lig, rec)).astype(np.float64)
    R = np.concatenate((lrad, rrad)).astype(np.float64) + PROBE
    nl, n = len(lig), len(x)
    side = np.arange(n) >= nl
    pts = np.full((n, 2), POINTS, dtype=np.int64)
    kept = 0
    for i0 in range(0, n, 512):                     # (row blocks bound the temporaries: one complex has 20 058 atoms)
        d = x[i0:i0 + 512, None, :] - x[None, :, :]
        near = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) < (R[i0:i0 + 512, None] + R[None, :]) + 1e-6
        for r in range(near.shape[0]):
            i = i0 + r
            near[r, i] = False
            j = np.nonzero(near[r])[0]
            kept += len(j)
            if len(j) == 0:
                continue
            q = x[i] + R[i] * SPHERE
            e = q[:, None, :] - x[j][None, :, :]
            hit = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2] < (R[j] * R[j])[None, :]
            pts[i, 0] = POINTS - int(hit[:, side[j] == side[i]].any(1).sum())
            pts[i, 1] = POINTS - int(hit.any(1).sum())
    w = 4 * np.pi * R * R / POINTS
    alone, cplx, bur = w * pts[:, 0], w * pts[:, 1], w * (pts[:, 0] - pts[:, 1])
    b = pts[:, 0] > pts[:, 1]
    return [alone[:nl].sum(), alone[nl:].sum(), cplx.sum(), bur.sum(), bur[:nl].sum(), bur[nl:].sum(), b[:nl].sum(),
            b[nl:].sum(), pts[:, 0].sum(), pts[:, 1].sum()], kept


def host_loop(cx):
    out, kept = [], 0
    for c in cx:
        row, k = host_one(c['lig'].detach().cpu().numpy(), c['rec'].detach().cpu().numpy(), c['lrad'], c['rrad'])
        out.append(row)
        kept += k
    return np.asarray(out, dtype=np.float64), kept


def tables(cx):
    return [c['lrad'] for c in cx], [c['rrad'] for c in cx], [c['lo'] for c in cx], [c['ro'] for c in cx]


def device_pass(cx):
    s = DK.surface_area_batch([c['lig'] for c in cx], [c['rec'] for c in cx], *tables(cx), probe=PROBE, n_points=POINTS)
    return s['rows'].cpu().numpy()


def eval_alone(cx, calls=20):
    lr, rr, lo, ro = tables(cx)
    plan = DK.SurfacePlan(lo, ro, lr, rr, dev, n_points=POINTS)
    lig, rec = torch.cat([c['lig'] for c in cx], 0), torch.cat([c['rec'] for c in cx], 0)
    out = plan.outputs()
    plan.eval(lig, rec, *out, probe=PROBE)
    sync()
    if dev.type != 'cuda':
        calls = 1
        t0 = time.perf_counter()
        plan.eval(lig, rec, *out, probe=PROBE)
        return 1e3 * (time.perf_counter() - t0) / calls, plan.atom_pairs
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        plan.eval(lig, rec, *out, probe=PROBE)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls, plan.atom_pairs


def med(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def main():
    reps = 1 if SMALL else max(ARGS.reps, 3)
    res = {'metric': 'dock_surface', 'device': 'simulator' if SMALL else torch.cuda.get_device_name(dev), 'reps': reps,
           'n_points': POINTS, 'probe': PROBE, 'all_partners': DK.surface_all_partners(), 'by_C': {}}
    for n in ([1, 2] if SMALL else [int(v) for v in ARGS.cs.split(',')]):
        cx = complexes(n)
        t = {'host': [], 'device': [], 'eval': []}
        for rep in range(-2, reps):
            sync()
            t0 = time.perf_counter()
            h, kept = host_loop(cx)
            t1 = time.perf_counter()
            d = device_pass(cx)
            t2 = time.perf_counter()
            e, pairs = eval_alone(cx)
            if rep >= 0:
                t['host'].append(t1 - t0)
                t['device'].append(t2 - t1)
                t['eval'].append(e)
        same_ints = bool((h[:, 6:] == d[:, [6, 7, 10, 11]]).all())
        row = {'atoms': int(sum(c['lig'].shape[0] + c['rec'].shape[0] for c in cx)), 'atom_pairs': pairs,
               'host_loop_ms': 1e3 * med(t['host']), 'device_ms': 1e3 * med(t['device']), 'eval_ms': med(t['eval']),
               'host_loop_ms_min_max': [1e3 * min(t['host']), 1e3 * max(t['host'])],
               'device_ms_min_max': [1e3 * min(t['device']), 1e3 * max(t['device'])],
               'skipped_share': 1.0 - kept / float(pairs), 'partners_per_atom': kept / float(sum(c['lig'].shape[0] + c['rec'].shape[0] for c in cx)),
               'integer_columns_agree': same_ints, 'max_abs_diff': float(np.abs(h[:, :6] - d[:, :6]).max()),
               'bsa_min_max': [float(d[:, 3].min()), float(d[:, 3].max())]}
        row['ratio'] = row['host_loop_ms'] / row['device_ms']
        res['by_C'][str(n)] = row
        print(f"C={n:2d}: " + json.dumps(row), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    with open(ARGS.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
