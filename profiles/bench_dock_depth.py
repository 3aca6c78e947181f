"""The depth stage of batched docking evaluation on the MI355X (equidock_public_amd.dock.residue_depth_batch), one JSON
line, also written to profiles/dock_depth_bench.log (--out).

Workload: seeded residue clouds with the heavy-atom counts of the 25 DB5.5 test complexes
(tests/golden/db5_test_atom_counts.json; residues of 4-14 atoms at protein density, two touching globules, radii drawn
from the four table values), coordinates on the device, 96 sphere points, probe 1.4 A.  Per C (the first C complexes):

  host_loop_ms    per complex two downloads and a float64 numpy evaluation of the same definitions: the exposure of every
                  sphere point on the atom's partners under the partner rule, the vertices of the exposed points, then
                  per tile of 64 target atoms the nearest vertex with the same skip rule (the own tile first, then only
                  the vertex tiles whose centre-and-reach bound can beat an atom's minimum so far)
  device_ms       dock.residue_depth_batch (tables upload, workspace + tile-table copy, five launches) and ONE download of
                  the [C][16] rows
  eval_ms         eqd_dock_depth_eval alone on a prepared plan (dock.DepthPlan.eval), by device events around 20
                  back-to-back calls; eval_noprune_ms: the same with prune = 0
  skipped_groups  column 14 summed over the batch; vertices: column 13
  max_abs_diff    largest |device - host| over the mean columns 0-2 and 6-7 of the batch; the integer columns 8, 9, 12, 13
                  must agree

Medians over --reps alternating repetitions after one warm-up of each, one process.

usage (GPU box): python profiles/bench_dock_depth.py [--reps R] [--cs 1,4,16,25] [--out FILE]
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
_ap.add_argument('--reps', type=int, default=3)
_ap.add_argument('--cs', default='1,4,16,25')
_ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dock_depth_bench.log'))
ARGS = _ap.parse_args()
SMALL = os.environ.get('EQD_DOCK_SMALL') == '1'
if SMALL:
    from tests import dock_common as _dc
    DK.load_dock_library_for_testing(_dc.build_sim())
dev = torch.device('cpu' if SMALL else 'cuda:0')
PROBE, POINTS, TILE = 1.4, 96, 64
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


def sq(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def host_exposure(x, R, side):
    """exposed [n][P][2] (alone, in complex) by the point test on the partners under the partner rule"""
    n = len(x)
    exposed = np.ones((n, POINTS, 2), dtype=bool)
    for i0 in range(0, n, 512):                     # (row blocks bound the temporaries: one complex has 20 058 atoms)
        near = np.sqrt(sq(x[i0:i0 + 512, None, :] - x[None, :, :])) < (R[i0:i0 + 512, None] + R[None, :]) + 1e-6
        for r in range(near.shape[0]):
            i = i0 + r
            near[r, i] = False
            j = np.nonzero(near[r])[0]
            if len(j) == 0:
                continue
            hit = sq((x[i] + R[i] * SPHERE)[:, None, :] - x[j][None, :, :]) < (R[j] * R[j])[None, :]
            exposed[i, :, 0] = ~hit[:, side[j] == side[i]].any(1)
            exposed[i, :, 1] = ~hit.any(1)
    return exposed


def host_nearest(x, tiles, vert, cen, reach):
    """s [len(x)]: per tile of target rows (`tiles`: [(a, b)]) the minimum over the vertex tiles (`vert`: one [m][3] per
    tile, None without a vertex; centre and reach per tile) - own tile first, then the tiles the bound cannot rule out"""
    s = np.full(len(x), np.inf)
    live = np.asarray([v is not None for v in vert])
    for t, (a, b) in enumerate(tiles):
        xt = x[a:b]
        m = sq(xt[:, None, :] - vert[t][None, :, :]).min(1) if vert[t] is not None else np.full(b - a, np.inf)
        bound = np.sqrt(sq(xt[:, None, :] - cen[None, :, :])) - reach[None, :] - 1e-6           # [rows][tiles]
        need = live & ((bound <= 0) | (bound * bound < m[:, None])).any(0)
        need[t] = False
        if need.any():
            v = np.concatenate([vert[k] for k in np.nonzero(need)[0]])
            m = np.minimum(m, sq(xt[:, None, :] - v[None, :, :]).min(1))
        s[a:b] = m
    return s


def host_one(lig, rec, lrad, rrad):
    """[mean depth ligand alone, receptor alone, all in complex, gain ligand, gain receptor, deepened atoms ligand,
    receptor, vertices alone, in complex]"""
    x = np.concatenate((lig, rec)).astype(np.float64)
    r = np.concatenate((lrad, rrad)).astype(np.float64)
    nl, n = len(lig), len(x)
    side = np.arange(n) >= nl
    exposed = host_exposure(x, r + PROBE, side)
    vert = x[:, None, :] + r[:, None, None] * SPHERE[None, :, :]
    tiles = [(a, min(a + TILE, nl)) for a in range(0, nl, TILE)] + [(a, min(a + TILE, n)) for a in range(nl, n, TILE)]
    s = np.empty((n, 2))
    for state in (0, 1):
        tv, cen, reach = [], np.zeros((len(tiles), 3)), np.zeros(len(tiles))
        for t, (a, b) in enumerate(tiles):
            e = exposed[a:b, :, state]
            own = e.any(1)
            tv.append(vert[a:b][e] if own.any() else None)
            if own.any():
                cen[t] = x[a:b][own].mean(0)
                reach[t] = (np.sqrt(sq(x[a:b][own] - cen[t])) + r[a:b][own]).max()
        if state == 0:                              # alone: each side against its own tiles
            ntl = (nl + TILE - 1) // TILE
            s[:nl, 0] = host_nearest(x[:nl], tiles[:ntl], tv[:ntl], cen[:ntl], reach[:ntl])
            s[nl:, 0] = host_nearest(x[nl:], [(a - nl, b - nl) for a, b in tiles[ntl:]], tv[ntl:], cen[ntl:], reach[ntl:])
        else:
            s[:, 1] = host_nearest(x, tiles, tv, cen, reach)
    d = np.sqrt(s)
    gain, deep = d[:, 1] - d[:, 0], s[:, 1] > s[:, 0]
    return [d[:nl, 0].sum() / nl, d[nl:, 0].sum() / (n - nl), d[:, 1].sum() / n, gain[:nl].sum() / nl, gain[nl:].sum() / (n - nl),
            deep[:nl].sum(), deep[nl:].sum(), exposed[:, :, 0].sum(), exposed[:, :, 1].sum()]


def host_loop(cx):
    return np.asarray([host_one(c['lig'].detach().cpu().numpy(), c['rec'].detach().cpu().numpy(), c['lrad'], c['rrad'])
                       for c in cx], dtype=np.float64)


def tables(cx):
    return [c['lrad'] for c in cx], [c['rrad'] for c in cx], [c['lo'] for c in cx], [c['ro'] for c in cx]


def device_pass(cx):
    s = DK.residue_depth_batch([c['lig'] for c in cx], [c['rec'] for c in cx], *tables(cx), probe=PROBE, n_points=POINTS)
    return s['rows'].cpu().numpy()


def eval_alone(cx, prune, calls=20):
    lr, rr, lo, ro = tables(cx)
    plan = DK.DepthPlan(lo, ro, lr, rr, dev, n_points=POINTS)
    lig, rec = torch.cat([c['lig'] for c in cx], 0), torch.cat([c['rec'] for c in cx], 0)
    out = plan.outputs()
    plan.eval(lig, rec, *out, probe=PROBE, prune=prune)
    sync()
    if dev.type != 'cuda':
        t0 = time.perf_counter()
        plan.eval(lig, rec, *out, probe=PROBE, prune=prune)
        return 1e3 * (time.perf_counter() - t0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        plan.eval(lig, rec, *out, probe=PROBE, prune=prune)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def med(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def main():
    reps = 1 if SMALL else max(ARGS.reps, 3)
    res = {'metric': 'dock_depth', 'device': 'simulator' if SMALL else torch.cuda.get_device_name(dev), 'reps': reps,
           'n_points': POINTS, 'probe': PROBE, 'pruning': DK.depth_pruning_enabled(), 'by_C': {}}
    for n in ([1, 2] if SMALL else [int(v) for v in ARGS.cs.split(',')]):
        cx = complexes(n)
        t = {'host': [], 'device': [], 'eval': [], 'noprune': []}
        for rep in range(-1, reps):
            sync()
            t0 = time.perf_counter()
            h = host_loop(cx)
            t1 = time.perf_counter()
            d = device_pass(cx)
            t2 = time.perf_counter()
            e, e_off = eval_alone(cx, True), eval_alone(cx, False)
            if rep >= 0:
                t['host'].append(t1 - t0)
                t['device'].append(t2 - t1)
                t['eval'].append(e)
                t['noprune'].append(e_off)
            print(f"C={n:2d} rep {rep}: host {t1 - t0:.2f} s, device {1e3 * (t2 - t1):.2f} ms", file=sys.stderr, flush=True)
        same_ints = bool((h[:, 5:] == d[:, [8, 9, 12, 13]]).all())
        row = {'atoms': int(sum(c['lig'].shape[0] + c['rec'].shape[0] for c in cx)),
               'host_loop_ms': 1e3 * med(t['host']), 'device_ms': 1e3 * med(t['device']), 'eval_ms': med(t['eval']),
               'eval_noprune_ms': med(t['noprune']),
               'host_loop_ms_min_max': [1e3 * min(t['host']), 1e3 * max(t['host'])],
               'device_ms_min_max': [1e3 * min(t['device']), 1e3 * max(t['device'])],
               'vertices_complex': int(d[:, 13].sum()), 'skipped_groups': int(d[:, 14].sum()),
               'integer_columns_agree': same_ints, 'max_abs_diff': float(np.abs(h[:, :5] - d[:, [0, 1, 2, 6, 7]]).max()),
               'depth_gain_ligand_min_max': [float(d[:, 6].min()), float(d[:, 6].max())]}
        row['ratio'] = row['host_loop_ms'] / row['device_ms']
        res['by_C'][str(n)] = row
        print(f"C={n:2d}: " + json.dumps(row), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    with open(ARGS.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
