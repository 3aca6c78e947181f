"""The graphs stage of batched docking inference on the MI355X (equidock_public_amd.dock), one JSON line:

  split   where the looped path's `graphs` time goes, per C: host preparation (parsing is not included: the inputs are
          residue lists), uploads, kernels + the edge-count synchronisation, the downloads the host collate needs, and
          graph.batch_pairs.  Measured on an instrumented restatement of featurize.knn_graph_device that synchronises
          between the parts, so the parts add up to a little more than the stage itself.
  stage   dock_complexes(..., batched_graphs=False) against batched_graphs=True on the same complexes, alternating in
          one process: medians of batch_seconds['graphs'] and ['total'] (device-synchronised, as dock_complexes takes
          them) after two warm-ups of each.  The looped samples are also split into three interleaved groups; the
          spread of their medians is the yardstick's own noise.

The complexes are the three real ones of tests/golden (graph_case, graph_case_pair300, graph_case_big) replicated to
C = 1, 4, 16, 24, each copy under its own seeded rigid motion.  --looped-only --root DIR runs the looped path of another
checkout (the parent commit) on the same inputs.

usage (GPU box): python profiles/bench_dock_graphs.py [--reps R] [--max-it K] [--cs 1,4,16,24]
(EQD_DOCK_SMALL=1: dry run on the x86 simulators, two small complexes, no GPU)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

HERE_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ap = argparse.ArgumentParser()
_ap.add_argument('--root', default=HERE_ROOT, help='checkout whose equidock_public_amd is measured')
_ap.add_argument('--looped-only', action='store_true', help='only dock_complexes as that checkout has it (no batched_graphs)')
_ap.add_argument('--reps', type=int, default=15)
_ap.add_argument('--max-it', type=int, default=50, help='clash-removal cap (the clash stage is not what is measured)')
_ap.add_argument('--cs', default='1,4,16,24')
ARGS = _ap.parse_args()
ROOT = os.path.abspath(ARGS.root)
sys.path.insert(0, ROOT)
from equidock_public_amd import _lib, dock as DK, featurize as FZ, graph as G  # noqa: E402

SMALL = os.environ.get('EQD_DOCK_SMALL') == '1'
if SMALL:
    from tests.hostsim import build as _hs
    from tests import dock_common as _dc
    _lib.load_library_for_testing(_hs.build())
    DK.load_dock_library_for_testing(_dc.build_sim())
dev = torch.device('cpu' if SMALL else 'cuda:0')
CUTOFF, K = 30.0, 10


def sync():
    if dev.type == 'cuda':
        torch.cuda.synchronize(dev)


def seeded_rigid(seed):
    rng = np.random.default_rng(seed)
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q.astype(np.float32), rng.uniform(-20.0, 20.0, size=3).astype(np.float32)


def complexes(n):
    """n complexes: the real fixture complexes in turn, copy k moved by the rigid motion of seed k (both sides alike)"""
    from tests import dock_common as dc
    names = ('graph_case_tiny', 'graph_case') if SMALL else dc.REAL
    base = [dc.fixture_residues(nm) for nm in names]
    out = []
    for k in range(n):
        R, t = seeded_rigid(k)
        lig, rec = base[k % len(base)]
        out.append(tuple([FZ.Residue(r.chain, r.number, r.resname, r.atom_names, r.elements, r.coords @ R.T + t) for r in side]
                         for side in (lig, rec)))
    return out


def looped_split(cx):
    """The looped graphs stage of dock_complexes with a synchronisation and a clock between its parts."""
    lib = _lib.load_library()
    parts = dict.fromkeys(('host', 'upload', 'kernels_sync', 'download', 'batch_pairs'), 0.0)
    f64 = dict(dtype=torch.float64, device=dev)
    st = _lib.stream_ptr(dev)
    graphs = []
    sync()
    for lig_in, rec_in in cx:
        t0 = time.perf_counter()
        lig_res, lig_all = DK._side(lig_in)
        rec_res, rec_all = DK._side(rec_in)
        lig, rec, lig_ca, rec_ca = FZ.preprocess_unbound_bound(lig_res, rec_res, inference=True)
        host = []
        for residues, ca in ((lig, lig_ca), (rec, rec_ca)):
            loc, n_i, u_i, v_i = FZ.local_frames(residues)
            R, t = FZ.rigid_transform_kabsch_3d(loc.T, np.asarray(ca).T)
            x = ((R @ loc.T) + t).T
            n_i, u_i, v_i = (R @ n_i.T).T, (R @ u_i.T).T, (R @ v_i.T).T
            atoms, off = FZ.atoms_ragged(residues)
            res = np.asarray([[FZ.residue_type_id(r.resname)] for r in residues], dtype=np.float32)
            host.append((atoms, off, x, n_i, u_i, v_i, res))
        t1 = time.perf_counter()
        parts['host'] += t1 - t0
        up = []
        for atoms, off, x, n_i, u_i, v_i, res in host:
            a = torch.as_tensor(np.ascontiguousarray(atoms, dtype=np.float32)).to(dev)
            o = torch.as_tensor(np.ascontiguousarray(off, dtype=np.int32)).to(dev)
            xs = [torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64)).to(dev) for v in (x, n_i, u_i, v_i)]
            up.append((a, o, xs, torch.as_tensor(x.astype(np.float32)).to(dev), torch.as_tensor(res).to(dev)))
        atoms_dev = [torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev) for v in (lig_all, rec_all)]
        sync()
        t2 = time.perf_counter()
        parts['upload'] += t2 - t1
        for a, o, xs, x32, res in up:
            n = int(o.numel() - 1)
            D = torch.empty(n, n, **f64)
            nbr = torch.empty(n, K, dtype=torch.int32, device=dev)
            nbd = torch.empty(n, K, **f64)
            deg = torch.empty(n, dtype=torch.int32, device=dev)
            mu = torch.empty(n, 5, dtype=torch.float32, device=dev)
            with _lib.device_guard(dev):
                _lib.check(lib.eqd_protein_graph_distances(n, _lib.ptr(a), _lib.ptr(o), _lib.ptr(D), st))
                _lib.check(lib.eqd_protein_graph_select(n, K, C.c_double(CUTOFF), _lib.ptr(D), _lib.ptr(xs[0]), _lib.ptr(nbr),
                                                        _lib.ptr(nbd), _lib.ptr(deg), _lib.ptr(mu), st))
            eoff = torch.zeros(n + 1, dtype=torch.int32, device=dev)
            eoff[1:] = torch.cumsum(deg, 0)
            E, _ = (int(v) for v in torch.stack([eoff[-1], deg.min()]).tolist())
            src = torch.empty(E, dtype=torch.int32, device=dev)
            dst = torch.empty(E, dtype=torch.int32, device=dev)
            he = torch.empty(E, 27, dtype=torch.float32, device=dev)
            with _lib.device_guard(dev):
                _lib.check(lib.eqd_protein_graph_edges(n, K, _lib.ptr(eoff), _lib.ptr(nbr), _lib.ptr(nbd), _lib.ptr(xs[0]),
                                                       _lib.ptr(xs[1]), _lib.ptr(xs[2]), _lib.ptr(xs[3]), _lib.ptr(src),
                                                       _lib.ptr(dst), _lib.ptr(he), st))
            graphs.append({'x': x32, 'res_feat': res, 'mu_r_norm': mu, 'src': src, 'dst': dst, 'he': he})
        sync()
        parts['kernels_sync'] += time.perf_counter() - t2
        del atoms_dev
    t3 = time.perf_counter()
    host_graphs = [{k: v.cpu().numpy() for k, v in g.items()} for g in graphs]
    t4 = time.perf_counter()
    parts['download'] = t4 - t3
    pairs = [(dict(host_graphs[2 * i], new_x=host_graphs[2 * i]['x']), host_graphs[2 * i + 1]) for i in range(len(cx))]
    G.batch_pairs(pairs).to(dev)
    sync()
    parts['batch_pairs'] = time.perf_counter() - t4
    return parts


def med(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def stage(net, cx, reps, max_it):
    kw = dict(device=dev, cutoff=CUTOFF, max_neighbor=K, max_it=max_it)
    modes = [('looped', {} if ARGS.looped_only else {'batched_graphs': False})]
    if not ARGS.looped_only:
        modes.append(('batched', {'batched_graphs': True}))
    samples = {m: {'graphs': [], 'total': []} for m, _ in modes}
    for rep in range(-2, reps):                      # two warm-ups of each, then alternating
        for m, extra in modes:
            r = DK.dock_complexes(net, cx, **kw, **extra)
            if rep >= 0:
                for k in ('graphs', 'total'):
                    samples[m][k].append(r[0]['batch_seconds'][k])
    out = {}
    for m, s in samples.items():
        out[m] = {'graphs_ms': 1e3 * med(s['graphs']), 'total_ms': 1e3 * med(s['total']),
                  'graphs_ms_min': 1e3 * min(s['graphs']), 'graphs_ms_max': 1e3 * max(s['graphs'])}
    groups = [1e3 * med(samples['looped']['graphs'][g::3]) for g in range(3)]
    out['looped']['graphs_ms_group_medians'] = groups
    out['looped']['graphs_ms_spread'] = max(groups) - min(groups)
    if 'batched' in out:
        out['graphs_ratio'] = out['looped']['graphs_ms'] / out['batched']['graphs_ms']
        out['stats'] = dict(DK.last_graph_stats)
    return out


def main():
    from tests import dock_common as dc
    net, _, _ = dc.seeded_net(dev)
    reps = 3 if SMALL else max(ARGS.reps, 5)
    res = {'metric': 'dock_graphs', 'root': 'this checkout' if ROOT == HERE_ROOT else 'other checkout',
           'device': 'simulator' if SMALL else torch.cuda.get_device_name(dev), 'reps': reps, 'max_it': ARGS.max_it,
           'cutoff': CUTOFF, 'max_neighbor': K, 'by_C': {}}
    for n in ([1, 2] if SMALL else [int(v) for v in ARGS.cs.split(',')]):
        cx = complexes(n)
        row = {'residues': int(sum(len(FZ.filter_residues(s)) for c in cx for s in c))}
        for _ in range(2):
            looped_split(cx)
        splits = [looped_split(cx) for _ in range(3 if SMALL else 5)]
        row['looped_split_ms'] = {k: 1e3 * med([s[k] for s in splits]) for k in splits[0]}
        row.update(stage(net, cx, reps, 3 if SMALL else ARGS.max_it))
        res['by_C'][str(n)] = row
        print(f"C={n:2d}: " + json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
