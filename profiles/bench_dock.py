"""Batched docking inference on the MI355X (equidock_public_amd.dock), one JSON line:

  clash removal   at fixed work (loss_stop = -1, max_it = K: every complex runs exactly K iterations): the sequential loop
                  of inference.remove_clashes (eqd_clash_iterations, one complex after the other) against ONE
                  remove_clashes_batch (libequidock_dock.so) over the same complexes, for C = 1, 4, 16, 25 seeded
                  synthetic atom clouds with the DB5.5 test-set sizes (tests/golden/db5_test_atom_counts.json, the first
                  C complexes in name order).  Rate = complexes x iterations / s; both paths poll once (check_every =
                  K + 1), device-synchronised, after a warm-up run.
  dock_complexes  end to end (graphs, one batched forward, apply_rigid, clash removal with the reference's stop rule) on
                  the real complexes of tests/golden (graph_case, graph_case_pair300, graph_case_big) with seeded weights:
                  complexes/s, batched against one complex per call.

usage (GPU box): python profiles/bench_dock.py [--iters K] [--reps R]
(EQD_DOCK_SMALL=1: dry run on the x86 simulators, tiny sizes, no GPU)"""
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

SMALL = os.environ.get('EQD_DOCK_SMALL') == '1'
if SMALL:
    from equidock_public_amd import _lib
    from tests.hostsim import build as _hs
    from tests import dock_common as _dc
    _lib.load_library_for_testing(_hs.build())
    DK.load_dock_library_for_testing(_dc.build_sim())
dev = torch.device('cpu' if SMALL else 'cuda:0')


def sync():
    if dev.type == 'cuda':
        torch.cuda.synchronize(dev)


def cloud(n, center, rng):
    """n points uniformly in a ball at protein density (~1 atom per 12 A^3)"""
    r = (3 * n * 12.0 / (4 * np.pi)) ** (1 / 3)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * r * rng.random((n, 1)) ** (1 / 3) + center).astype(np.float32)


def db5_clouds(seed=0):
    sizes = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'db5_test_atom_counts.json')))['complexes']
    rng = np.random.default_rng(seed)
    out = []
    for name, nl, nr in sizes:
        if SMALL:
            nl, nr = max(8, nl // 100), max(8, nr // 100)
        rr, rl = (3 * nr * 12.0 / (4 * np.pi)) ** (1 / 3), (3 * nl * 12.0 / (4 * np.pi)) ** (1 / 3)
        rec = cloud(nr, np.zeros(3), rng)
        lig = cloud(nl, np.array([0.8 * (rr + rl), 0.0, 0.0]), rng)     # overlapping surfaces
        out.append((name, torch.from_numpy(lig).to(dev), torch.from_numpy(rec).to(dev)))
    return out


def timed(fn, reps):
    fn()                                     # warm-up
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def clash_rates(K, reps):
    cx = db5_clouds()
    rows = {}
    for C in (1, 4, 16, 25):
        sub = cx[:C]

        def seq():
            for _, l, r in sub:
                INF.remove_clashes(l, r, loss_stop=-1.0, max_it=K, check_every=K + 1)

        def bat():
            DK.remove_clashes_batch([l for _, l, _ in sub], [r for _, _, r in sub], loss_stop=-1.0, max_it=K, check_every=K + 1)
        ts, tb = timed(seq, reps), timed(bat, reps)
        rows[str(C)] = {'sequential_cit_per_s': C * K / ts, 'batched_cit_per_s': C * K / tb, 'ratio': ts / tb,
                        'sequential_ms_per_iteration': 1e3 * ts / K, 'batched_ms_per_iteration': 1e3 * tb / K}
        print(f"clash removal C={C:2d}: sequential {C * K / ts:9.1f}, batched {C * K / tb:9.1f} complex-iterations/s "
              f"(x{ts / tb:.1f})", file=sys.stderr, flush=True)
    return rows


def end_to_end(reps):
    from tests import dock_common as dc
    names = ('graph_case_tiny', 'graph_case') if SMALL else dc.REAL
    net, _, _ = dc.seeded_net(dev)
    cx = [dc.fixture_residues(n) for n in names]
    kw = dict(device=dev, max_it=5 if SMALL else 2000)
    last = {}

    def batched():
        last['r'] = DK.dock_complexes(net, cx, **kw)

    def one_by_one():
        DK.dock_complexes(net, cx, max_complexes_per_batch=1, **kw)
    tb, t1 = timed(batched, reps), timed(one_by_one, reps)
    r = last['r']
    return {'complexes': list(names), 'atoms': [[x['n_ligand_atoms'], x['n_receptor_atoms']] for x in r],
            'clash_iterations': [x['clash_iterations'] for x in r],
            'batched_complexes_per_s': len(cx) / tb, 'one_by_one_complexes_per_s': len(cx) / t1,
            'batched_stage_seconds': {k: v for k, v in r[0]['batch_seconds'].items() if k != 'n_complexes'}}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--iters', type=int, default=3 if SMALL else 100)
    p.add_argument('--reps', type=int, default=1 if SMALL else 3)
    a = p.parse_args()
    res = {'metric': 'dock', 'device': 'simulator' if SMALL else torch.cuda.get_device_name(dev),
           'clash_fixed_work': {'iterations': a.iters, 'by_C': clash_rates(a.iters, a.reps)},
           'dock_complexes': end_to_end(a.reps)}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
