"""Checks of the batched lDDT and interface lDDT (equidock_public_amd.dock.lddt_batch / LddtPlan, eqd_dock_lddt_* of
libequidock_dock.so) shared by the simulator tests (tests/test_dock_lddt_sim.py) and the GPU tests
(tests/test_dock_lddt_gpu.py).

Yardstick: `ref64`, a float64 numpy evaluation of the definitions of include/equidock_dock.h written without the kernels'
decomposition (no tiles, no staging): dense blocked fp64 distance matrices of the native and of the model, the threshold
decisions on them, `np.add.reduceat` over the residue tables, and the block bound for column 14.  Every result is a count
of threshold decisions or a quotient of two such counts, so everything is compared for EQUALITY: the per-atom counts and
columns 4-14 as integers, columns 0-3 and the per-residue scores bit for bit, NaN positions included.  Every case asserts
from the yardstick alone a margin on every decision it rests on - |d_n - radius| over the pairs in different residues,
||d_m - d_n| - t_k| over the included pairs, |gap - (radius + 1e-6)| over the block pairs - of more than 1e-6 A for the
real complexes and more than 1e-9 A for the seeded ones: fp64 rounding (1e-13 A at these coordinates) cannot turn a
decision.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from equidock_public_amd import _lib, dock as DK
from tests import dock_common as dc

RADIUS, THRESHOLDS = 15.0, (0.5, 1.0, 2.0, 4.0)
OFFSET = np.array([83.0, 72.0, 243.0])         # a PDB-like frame
# the kernels as built (csrc_dock/eqd_dock_lddt.hip): rows per block, column blocks and column atoms staged per item
BLOCK, STAGE = 64, 8
COLS = BLOCK * STAGE
REAL_MARGIN, SEEDED_MARGIN = 1e-6, 1e-9


# ---- the float64 yardstick ------------------------------------------------------------------------------------------
def _dist(a, b):
    d = a[:, None, :] - b[None, :, :]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def _score(v):
    """(P0 + P1 + P2 + P3) / (4 N) of rows [.., 5] = N, P0..P3 (int64); NaN where N == 0"""
    v = np.asarray(v, dtype=np.int64)
    n, p = v[..., 0], v[..., 1:5].sum(-1)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(n == 0, np.nan, p.astype(np.float64) / (4.0 * n.astype(np.float64)))


def ref64(lig_pred, rec_pred, lig_true, rec_true, lo, ro, radius=RADIUS, thresholds=THRESHOLDS):
    """counts [n][10] (ligand rows first), residue scores [r][2], the 16 columns, and the margins `incl_margin`,
    `thr_margin`, `gap_margin`, the largest intra-chain |d_m - d_n| `intra_shift`"""
    xn = np.concatenate((np.asarray(lig_true, dtype=np.float64), np.asarray(rec_true, dtype=np.float64)))
    xm = np.concatenate((np.asarray(lig_pred, dtype=np.float64),
                         np.asarray(rec_true if rec_pred is None else rec_pred, dtype=np.float64)))
    nl, n = len(lig_true), len(xn)
    lo, ro = np.asarray(lo, dtype=np.int64), np.asarray(ro, dtype=np.int64)
    assert lo[0] == 0 and ro[0] == 0 and lo[-1] == nl and ro[-1] == n - nl and xm.shape == xn.shape
    first = np.concatenate((lo[:-1], ro[:-1] + nl))
    resid = np.repeat(np.arange(len(first)), np.diff(np.concatenate((first, [n]))))
    side = np.arange(n) >= nl
    counts = np.zeros((n, 10), dtype=np.int64)
    incl_margin = thr_margin = np.inf
    intra_shift = 0.0
    for i0 in range(0, n, 512):
        i1 = min(i0 + 512, n)
        dn, dm = _dist(xn[i0:i1], xn), _dist(xm[i0:i1], xm)
        other = resid[i0:i1, None] != resid[None, :]
        if other.any():
            incl_margin = min(incl_margin, float(np.abs(dn - radius)[other].min()))
        inc = other & (dn < radius)
        inter = inc & (side[i0:i1, None] != side[None, :])
        diff = np.abs(dm - dn)
        if inc.any():
            thr_margin = min([thr_margin] + [float(np.abs(diff - t)[inc].min()) for t in thresholds])
        if (inc & ~inter).any():
            intra_shift = max(intra_shift, float(diff[inc & ~inter].max()))
        counts[i0:i1, 0] = inc.sum(1)
        counts[i0:i1, 5] = inter.sum(1)
        for k, t in enumerate(thresholds):
            ok = diff < t
            counts[i0:i1, 1 + k] = (inc & ok).sum(1)
            counts[i0:i1, 6 + k] = (inter & ok).sum(1)
    res = np.add.reduceat(counts, first, axis=0)
    res_lddt = np.stack((_score(res[:, :5]), _score(res[:, 5:])), axis=1)
    tl, tr = counts[:nl].sum(0), counts[nl:].sum(0)
    tot = tl + tr
    # the block bound: blocks of BLOCK consecutive rows of each side, centroid = row-order sum / count
    cen, rad = [], []
    for a, b in ((0, nl), (nl, n)):
        for q in range(a, b, BLOCK):
            x = xn[q:min(q + BLOCK, b)]
            c = np.cumsum(x, axis=0)[-1] / float(len(x))
            cen.append(c)
            rad.append(_dist(x, c[None])[:, 0].max())
    cen, rad = np.asarray(cen), np.asarray(rad)
    gap = (_dist(cen, cen) - rad[:, None]) - rad[None, :]
    row = np.zeros(16)
    row[0], row[1], row[2], row[3] = _score(tot[:5]), _score(tot[5:]), _score(tl[:5]), _score(tr[:5])
    row[4], row[5], row[6:10], row[10:14] = tot[0], tot[5], tot[1:5], tot[6:10]
    row[14] = int((gap >= radius + 1e-6).sum())
    return {'counts': counts, 'res_lddt': res_lddt, 'row': row, 'row_noprune': np.concatenate((row[:14], [0.0, 0.0])),
            'incl_margin': incl_margin, 'thr_margin': thr_margin, 'intra_shift': intra_shift,
            'gap_margin': float(np.abs(gap - (radius + 1e-6)).min()), 'blocks': len(rad)}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def check_complex(name, got, ref, margin, prune=True):
    """one complex of a batch (see `run`) against the yardstick: every integer equal, every score bit for bit"""
    assert ref['incl_margin'] > margin, (name, 'inclusion margin', ref['incl_margin'])
    assert ref['thr_margin'] > margin, (name, 'threshold margin', ref['thr_margin'])
    assert ref['gap_margin'] > margin, (name, 'block gap margin', ref['gap_margin'])
    assert got['counts'].dtype == np.int32 and got['counts'].shape == ref['counts'].shape
    bad = np.nonzero((got['counts'] != ref['counts']).any(1))[0]
    assert len(bad) == 0, (name, 'counts differ at rows', bad[:8], got['counts'][bad[:8]], ref['counts'][bad[:8]])
    c = ref['counts']
    for block in (c[:, :5], c[:, 5:]):                          # 0 <= P0 <= P1 <= P2 <= P3 <= N for every atom
        assert (block[:, 1] >= 0).all() and (np.diff(block[:, 1:], axis=1) >= 0).all() and (block[:, 4] <= block[:, 0]).all()
    want = ref['row'] if prune else ref['row_noprune']
    assert np.array_equal(got['row'][4:], want[4:]), (name, got['row'][4:], want[4:])
    assert _bits(got['row'][:4]) == _bits(want[:4]), (name, got['row'][:4], want[:4])
    assert got['res_lddt'].shape == ref['res_lddt'].shape
    assert _bits(got['res_lddt']) == _bits(ref['res_lddt']), (name, 'residue scores differ')


# ---- running --------------------------------------------------------------------------------------------------------
def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run(dev, cases, radius=RADIUS, thresholds=THRESHOLDS, full=False):
    """one lddt_batch over `cases` [(lig_pred, rec_pred or None, lig_true, rec_true, lig residue offsets, rec residue
    offsets)] -> per complex {'row' [16], 'counts' [n][10] (ligand rows first), 'res_lddt' [r][2]} on the host; rec_pred
    goes in only when a case has one (then every case's, a missing one being its rec_true)"""
    cases = list(cases)
    recs_p = None
    if any(c[1] is not None for c in cases):
        recs_p = [_t(c[3] if c[1] is None else c[1], dev) for c in cases]
    out = DK.lddt_batch([_t(c[0], dev) for c in cases], [_t(c[2], dev) for c in cases], [_t(c[3], dev) for c in cases],
                        [c[4] for c in cases], [c[5] for c in cases], rec_pred_list=recs_p, inclusion_radius=radius,
                        thresholds=thresholds)
    kind = torch.device(dev).type
    for k in DK.LDDT_KEYS:
        assert out[k].dtype == torch.float64 and out[k].shape == (len(cases),) and out[k].device.type == kind
    assert out['rows'].shape == (len(cases), DK.LDDT_COLS) and out['lig_counts'].dtype == torch.int32
    if full:
        return out
    rows = out['rows'].cpu().numpy()
    lc, rc = out['lig_counts'].cpu().numpy(), out['rec_counts'].cpu().numpy()
    ls, rs = out['lig_res_lddt'].cpu().numpy(), out['rec_res_lddt'].cpu().numpy()
    res, a = [], [0, 0, 0, 0]
    for c, case in enumerate(cases):
        b = [a[0] + len(case[2]), a[1] + len(case[3]), a[2] + len(case[4]) - 1, a[3] + len(case[5]) - 1]
        res.append({'row': rows[c], 'counts': np.concatenate((lc[a[0]:b[0]], rc[a[1]:b[1]])),
                    'res_lddt': np.concatenate((ls[a[2]:b[2]], rs[a[3]:b[3]]))})
        a = b
    assert a == [len(lc), len(rc), len(ls), len(rs)]
    return res


def same_bits(a, b, what, with_skipped=True):
    for k in ('counts', 'res_lddt'):
        assert a[k].tobytes() == b[k].tobytes(), (what, k)
    n = 16 if with_skipped else 14
    assert a['row'][:n].tobytes() == b['row'][:n].tobytes(), (what, 'row', a['row'], b['row'])


# ---- cases ------------------------------------------------------------------------------------------------------------
def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


POSES = (('EquiDock', 'lig_equidock'), ('no clashes', 'lig_no_clashes'), ('native', 'lig_true'))


@functools.lru_cache(maxsize=None)
def real_cases():
    """1AVX and 1HCF of tests/golden/dockq_case.npz: the EquiDock pose, the no-clashes pose and the native as model; the
    model's receptor is the native's"""
    z = np.load(os.path.join(dc.GOLDEN, 'dockq_case.npz'))
    out = {}
    for nm in ('1AVX', '1HCF'):
        lo, ro = z[f'{nm}_lig_true_res_off'], z[f'{nm}_rec_true_res_off']
        for tag, key in POSES:
            assert (z[f'{nm}_{key}_names'] == z[f'{nm}_lig_true_names']).all()
            out[f'{nm} {tag}'] = (z[f'{nm}_{key}_atoms'], None, z[f'{nm}_lig_true_atoms'], z[f'{nm}_rec_true_atoms'], lo, ro)
    return out


def _residue_sizes(rng, n_atoms, mode):
    if mode == 'one':
        return np.int64([n_atoms])
    if mode == 'single':
        return np.ones(n_atoms, dtype=np.int64)
    sizes, left = [], n_atoms
    while left > 0:
        k = min(int(rng.integers(4, 15)), left)
        sizes.append(k)
        left -= k
    return np.asarray(sizes, dtype=np.int64)


def _globule(rng, n_atoms, centre, mode):
    """a seeded globule at protein density: residue centres uniform in a ball of 16 A^3 per atom, the atoms of a residue
    within ~1.5 A of its centre; (atoms float32, residue offsets, ball radius)"""
    sizes = _residue_sizes(rng, n_atoms, mode)
    rad = (3.0 * 16.0 * n_atoms / (4.0 * np.pi)) ** (1.0 / 3.0)
    v = rng.standard_normal((len(sizes), 3))
    cen = v / np.linalg.norm(v, axis=1, keepdims=True) * rad * rng.uniform(0.0, 1.0, (len(sizes), 1)) ** (1.0 / 3.0)
    x = np.repeat(cen, sizes, axis=0) + rng.standard_normal((n_atoms, 3)) * 0.9 + centre
    return _f32(x), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), rad


def _rotation(rng, angle):
    ax = rng.standard_normal(3)
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def globules(n_lig, n_rec, seed, mode='random', gap=0.8):
    """two touching globules of n_lig and n_rec atoms at the PDB-like offset; the model's ligand is the native's turned by
    0.4 rad about its centre, moved by ~3 A and jittered by 0.7 A per atom (every threshold gets hits and misses)"""
    rng = np.random.default_rng(seed)
    lx, lo, ball_l = _globule(rng, n_lig, OFFSET, mode)
    ball_r = (3.0 * 16.0 * n_rec / (4.0 * np.pi)) ** (1.0 / 3.0)
    rx, ro, _ = _globule(rng, n_rec, OFFSET + np.array([(ball_l + ball_r) * gap, 0.0, 0.0]), mode)
    c = lx.astype(np.float64).mean(0)
    lp = (lx.astype(np.float64) - c) @ _rotation(rng, 0.4).T + c + rng.standard_normal(3) * 2.0 + rng.standard_normal(lx.shape) * 0.7
    return (_f32(lp), None, lx, rx, lo, ro)


# ligand x receptor atoms: 1 x 1; (BLOCK - 1, BLOCK, BLOCK + 1) x (COLS - 1, COLS, COLS + 1); the blocks of both sides
# together either side of one stage (7 + 1, 7 + 1, 8 + 1 blocks); several items per row block (5 + 21 blocks: 4 items);
# one residue per side; single-atom residues; a residue across the first block boundary
EDGES = {'edge_1x1': (1, 1, 701, 'random')}
EDGES.update({f'edge_{nl}x{nr}': (nl, nr, 710 + 3 * i + j, 'random')
              for i, nl in enumerate((BLOCK - 1, BLOCK, BLOCK + 1)) for j, nr in enumerate((COLS - 1, COLS, COLS + 1))})
EDGES.update({f'edge_{BLOCK}x{nr}': (BLOCK, nr, 720 + j, 'random')
              for j, nr in enumerate((COLS - BLOCK - 1, COLS - BLOCK, COLS - BLOCK + 1))})
EDGES.update({'edge_several_items': (300, 1300, 730, 'random'), 'edge_one_residue': (20, 30, 731, 'one'),
              'edge_single_atoms': (40, 50, 732, 'single'), 'edge_straddle': (90, 70, 733, 'random')})


@functools.lru_cache(maxsize=None)
def edge_cases():
    out = {k: globules(nl, nr, seed, mode) for k, (nl, nr, seed, mode) in EDGES.items()}
    # the two single atoms of edge_1x1: 3 A apart in the native, 3.7 A in the model
    lp, _, lx, rx, lo, ro = out['edge_1x1']
    out['edge_1x1'] = (_f32(lx + np.float32([0.5, 0.25, 0.25])), None, lx, _f32(lx + np.float32([2.0, 2.0, 1.0])), lo, ro)
    # edge_straddle: a ligand residue of rows 58-69
    lp, _, lx, rx, lo, ro = out['edge_straddle']
    lo = np.int32(sorted(set(int(v) for v in lo if v <= BLOCK - 6 or v >= BLOCK + 6) | {BLOCK - 6, BLOCK + 6}))
    out['edge_straddle'] = (lp, None, lx, rx, lo, ro)
    return out


@functools.lru_cache(maxsize=None)
def degenerate_cases():
    out = {}
    lp, _, lx, rx, lo, ro = globules(70, 90, 801)
    far = np.float32([200.0, 0.0, 0.0])
    out['far_sides'] = (_f32(lp - far), None, _f32(lx - far), rx, lo, ro)                 # no inter-chain pair
    out['out_of_range_1x1'] = (_f32(OFFSET[None] + [[0.5, 0.0, 0.0]]), None, _f32(OFFSET[None]),
                               _f32(OFFSET[None] + [[20.0, 3.0, 1.0]]), np.int32([0, 1]), np.int32([0, 1]))
    out['identical'] = (lx, None, lx, rx, lo, ro)
    out['ligand_100A_away'] = (_f32(lx + np.float32([0.0, 100.0, 0.0])), None, lx, rx, lo, ro)
    # ONE rigid motion of both sides of the model: nothing changes but fp32 rounding (the non-NULL rec_pred)
    rng = np.random.default_rng(802)
    R, t = _rotation(rng, 1.1), np.array([31.0, -17.0, 55.0])
    c = np.concatenate((lx, rx)).astype(np.float64).mean(0)
    out['common_rigid_motion'] = (_f32((lx.astype(np.float64) - c) @ R.T + c + t), _f32((rx.astype(np.float64) - c) @ R.T + c + t),
                                  lx, rx, lo, ro)
    return out


def seeded_cases():
    return {**edge_cases(), **degenerate_cases()}


def all_cases():
    return {**real_cases(), **seeded_cases()}


def margin_of(name):
    return REAL_MARGIN if name in real_cases() else SEEDED_MARGIN


_refs = {}


def reference(name):
    """the yardstick of a case of this file - computed once, shared by the tests, never changed"""
    if name not in _refs:
        _refs[name] = ref64(*all_cases()[name])
    return _refs[name]


_measured = {}


def measured(dev, group):
    """the cases of a group ('real': the six poses, 'seeded': every other case) in ONE batch each - computed once per
    device type and shared by the tests"""
    key = (torch.device(dev).type, group)
    if key not in _measured:
        cases = real_cases() if group == 'real' else seeded_cases()
        names = list(cases)
        _measured[key] = dict(zip(names, run(dev, [cases[n] for n in names])))
    return _measured[key]


def check_names(dev, group, names):
    got = measured(dev, group)
    for n in names:
        check_complex(n, got[n], reference(n), margin_of(n))
    return {n: got[n] for n in names}


# ---- the checks -------------------------------------------------------------------------------------------------------
# the table of the issue (numpy float64, radius 15, thresholds 0.5 / 1 / 2 / 4): ligand atoms, receptor atoms, N all,
# N inter, P inter per threshold, lDDT, ilDDT
TABLE = {'1AVX EquiDock': (1286, 1630, 1207834, 106372, (1484, 2966, 5764, 11560), 0.916438, 0.051174),
         '1AVX no clashes': (1286, 1630, 1207834, 106372, (884, 1754, 3550, 7474), 0.914759, 0.032109),
         '1HCF EquiDock': (809, 1802, 945052, 115514, (4574, 8880, 17780, 35162), 0.895334, 0.143697),
         '1HCF no clashes': (809, 1802, 945052, 115514, (2702, 5388, 11266, 24140), 0.889276, 0.094136),
         '1AVX native': (1286, 1630, 1207834, 106372, (106372,) * 4, 1.0, 1.0),
         '1HCF native': (809, 1802, 945052, 115514, (115514,) * 4, 1.0, 1.0)}


def check_yardstick_reproduces_the_table():
    """2. CPU: ref64 on the six real poses gives the issue's table - the integers exactly, the scores to the six printed
    digits (exactly 1.0 for the native as model) - and intra-chain pairs are preserved at every threshold"""
    f = real_cases()
    assert set(f) == set(TABLE)
    for name, t in TABLE.items():
        r = reference(name)
        row = r['row']
        assert (len(f[name][2]), len(f[name][3])) == t[:2]
        assert (int(row[4]), int(row[5])) == t[2:4], (name, row[4:6])
        assert tuple(int(v) for v in row[10:14]) == t[4], (name, row[10:14])
        assert r['intra_shift'] < 3e-3 and (row[6:10] - row[10:14] == row[4] - row[5]).all(), (name, r['intra_shift'])
        if name.endswith('native'):
            assert row[0] == 1.0 and row[1] == 1.0 and row[2] == 1.0 and row[3] == 1.0
        else:
            assert abs(row[0] - t[5]) <= 5e-7 and abs(row[1] - t[6]) <= 5e-7, (name, row[:2])
        assert r['incl_margin'] > REAL_MARGIN and r['thr_margin'] > REAL_MARGIN and r['gap_margin'] > REAL_MARGIN


def check_real(dev):
    """2. the six real poses in ONE batch against the yardstick"""
    got = check_names(dev, 'real', list(real_cases()))
    for name, t in TABLE.items():
        row = got[name]['row']
        assert (int(row[4]), int(row[5])) == t[2:4] and tuple(int(v) for v in row[10:14]) == t[4]
        assert row[14] > 0                                      # block pairs are skipped


def check_edges(dev):
    """3. block and stage edges, several items per row block, one residue per side, single-atom residues, a residue across
    a block boundary"""
    cases = edge_cases()
    got = check_names(dev, 'seeded', list(cases))
    sizes = {(len(c[2]), len(c[3])) for c in cases.values()}
    assert {(nl, nr) for nl in (BLOCK - 1, BLOCK, BLOCK + 1) for nr in (COLS - 1, COLS, COLS + 1)} <= sizes and (1, 1) in sizes
    nblk = {n: -(-len(c[2]) // BLOCK) - (-len(c[3]) // BLOCK) for n, c in cases.items()}
    assert {STAGE, STAGE + 1} <= set(nblk.values()) and nblk['edge_several_items'] > 3 * STAGE
    assert all(reference(n)['blocks'] == b for n, b in nblk.items())
    c = cases['edge_one_residue']
    assert len(c[4]) == 2 and len(c[5]) == 2
    r = got['edge_one_residue']['row']
    assert r[4] == r[5] > 0 and (r[6:10] == r[10:14]).all()    # no intra pair exists
    c = cases['edge_single_atoms']
    assert len(c[4]) == len(c[2]) + 1 and len(c[5]) == len(c[3]) + 1
    lo = cases['edge_straddle'][4]
    assert any(a < BLOCK < b for a, b in zip(lo[:-1], lo[1:]))
    r = got['edge_1x1']
    assert r['row'][4] == 2 and r['counts'].tolist() == [[1, 0, 1, 1, 1, 1, 0, 1, 1, 1]] * 2 and r['row'][0] == 0.75
    for n in cases:                                             # every threshold gets hits and misses
        row = got[n]['row']
        if row[4] > 1000:
            assert 0 < row[6] < row[7] < row[8] < row[9] <= row[4], (n, row)


def check_degenerate(dev):
    """4. degenerate sets"""
    cases = degenerate_cases()
    got = check_names(dev, 'seeded', list(cases))
    r = got['far_sides']
    assert r['row'][5] == 0 and np.isnan(r['row'][1]) and 0.0 < r['row'][0] <= 1.0 and (r['row'][10:14] == 0).all()
    assert np.isnan(r['res_lddt'][:, 1]).all() and (r['counts'][:, 5:] == 0).all()
    r = got['out_of_range_1x1']
    assert np.isnan(r['row'][:4]).all() and (r['row'][4:14] == 0).all() and (r['counts'] == 0).all()
    assert r['row'][14] == 2                                    # its two ordered block pairs fall to the bound
    assert np.isnan(r['res_lddt']).all()
    for n in ('identical', 'common_rigid_motion'):
        r = got[n]
        assert (r['row'][:4] == 1.0).all() and r['row'][5] > 0, (n, r['row'])
        ok = ~np.isnan(r['res_lddt'])
        assert ok[:, 0].all() and ok[:, 1].any() and (r['res_lddt'][ok] == 1.0).all()
    assert cases['common_rigid_motion'][1] is not None
    assert np.abs(cases['common_rigid_motion'][1] - cases['common_rigid_motion'][3]).max() > 10.0
    r = got['ligand_100A_away']
    assert r['row'][5] > 0 and (r['row'][10:14] == 0).all() and r['row'][1] == 0.0 and r['row'][0] > 0.5


def check_pruning_switch(dev, monkeypatch):
    """5. prune off, the EQD_DOCK_LDDT_PRUNE=0 environment and prune on: the same bits except column 14"""
    cases = all_cases()
    names = ['1HCF EquiDock', 'edge_several_items', 'edge_65x513', 'far_sides']
    cs = [cases[n] for n in names]
    on = [measured(dev, 'real' if n in real_cases() else 'seeded')[n] for n in names]
    assert DK.lddt_pruning_enabled()
    monkeypatch.setenv('EQD_DOCK_LDDT_PRUNE', '0')
    assert not DK.lddt_pruning_enabled()
    env_off = run(dev, cs)
    monkeypatch.undo()
    assert DK.lddt_pruning_enabled()
    plan = DK.LddtPlan([c[4] for c in cs], [c[5] for c in cs], dev)
    arg = {}
    for flag in (False, True):
        counts, res, rows = plan.outputs()
        plan.eval(torch.cat([_t(c[0], dev) for c in cs]), None, torch.cat([_t(c[2], dev) for c in cs]),
                  torch.cat([_t(c[3], dev) for c in cs]), counts, res, rows, prune=flag)
        arg[flag] = (counts.cpu().numpy(), res.cpu().numpy(), rows.cpu().numpy())
    assert arg[False][0].tobytes() == arg[True][0].tobytes() and arg[False][1].tobytes() == arg[True][1].tobytes()
    assert arg[False][2][:, :14].tobytes() == arg[True][2][:, :14].tobytes()
    assert (arg[False][2][:, 14] == 0).all() and (arg[True][2][:, 14] > 0).any()
    for i, n in enumerate(names):
        check_complex(n, env_off[i], reference(n), margin_of(n), prune=False)
        same_bits(on[i], env_off[i], f'{n}: pruning on vs off', with_skipped=False)
        assert env_off[i]['row'][14] == 0 and arg[True][2][i].tobytes() == on[i]['row'].tobytes()
    assert on[0]['row'][14] > 0 and on[3]['row'][14] > 0


def check_bits(dev):
    """6. each complex alone, first, last, in a permuted batch and in three runs: the same bits"""
    cases = all_cases()
    names = ['1HCF EquiDock', 'edge_63x511', 'edge_several_items', 'common_rigid_motion']
    cs = [cases[n] for n in names]
    k = len(cs)
    runs = [run(dev, cs) for _ in range(3)]
    perm = [2, 0, 3, 1]
    permuted = run(dev, [cs[p] for p in perm])
    for i, n in enumerate(names):
        same_bits(runs[0][i], runs[1][i], f'{n}: run to run')
        same_bits(runs[0][i], runs[2][i], f'{n}: run to run')
        same_bits(runs[0][i], permuted[perm.index(i)], f'{n}: permuted')
        same_bits(runs[0][i], run(dev, [cs[i]])[0], f'{n}: alone')
        same_bits(runs[0][i], measured(dev, 'real' if n in real_cases() else 'seeded')[n], f'{n}: in its group batch')
    for s in range(1, k):                                       # the batch rotated: every complex comes first and last
        order = [(s + j) % k for j in range(k)]
        rot = run(dev, [cs[j] for j in order])
        for j, o in enumerate(order):
            same_bits(runs[0][o], rot[j], f'{names[o]}: rotated batch')


def check_validation_errors(dev):
    """1. ABI; refused before any launch, with a message (the entry points and lddt_batch); nothing is written"""
    lib = DK.load_dock_library()
    assert lib.eqd_dock_lddt_abi() == DK.DOCK_LDDT_ABI == 1 and DK.LDDT_COLS == 16 and DK.LDDT_BLOCK == BLOCK
    assert lib.eqd_dock_abi_version() == 1 and len(DK.LDDT_KEYS) == 15
    lig, rec = torch.zeros(4, 3, device=dev), torch.ones(5, 3, device=dev)
    lo, ro = np.int32([0, 2, 4]), np.int32([0, 1, 5])
    good = dict(lig_res_offsets=[lo], rec_res_offsets=[ro])
    out = DK.lddt_batch([lig], [lig], [rec], **good)
    assert out['rows'].shape == (1, 16) and float(out['lddt'][0]) == 1.0
    with pytest.raises(ValueError, match='predicted ligands for'):
        DK.lddt_batch([lig, lig], [lig], [rec], **good)
    with pytest.raises(ValueError, match='predicted ligands for'):
        DK.lddt_batch([lig], [lig], [rec], rec_pred_list=[rec, rec], **good)
    with pytest.raises(ValueError, match='are needed'):
        DK.lddt_batch([lig], [lig], [rec])
    with pytest.raises(ValueError, match='complex 0: ligand: residue offsets'):
        DK.lddt_batch([lig], [lig], [rec], **dict(good, lig_res_offsets=[np.int32([0, 2, 2, 4])]))
    with pytest.raises(ValueError, match='rows for tables of'):
        DK.lddt_batch([lig[:3]], [lig[:3]], [rec], **good)
    with pytest.raises(ValueError, match='predicted ligand rows for'):
        DK.lddt_batch([lig[:3]], [lig], [rec], **good)
    plan = out['plan']
    with pytest.raises(ValueError, match='the plan holds 1 complexes'):
        DK.lddt_batch([lig, lig], [lig, lig], [rec, rec], plan=plan)
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(_lib.EquidockHipError, match='inclusion_radius'):
            DK.lddt_batch([lig], [lig], [rec], inclusion_radius=bad, **good)
        with pytest.raises(_lib.EquidockHipError, match=r'thresholds\[2\]'):
            DK.lddt_batch([lig], [lig], [rec], thresholds=(0.5, 1.0, bad, 4.0), **good)

    def offs(v):
        return np.ascontiguousarray(np.asarray(v, dtype=np.int32))

    def p(a):
        return a.ctypes.data_as(C.c_void_p)

    la, ra, lro, rro = offs([0, 4, 8]), offs([0, 5, 10]), offs([0, 2, 4]), offs([0, 2, 4])
    wsb = lib.eqd_dock_lddt_workspace_bytes(2, p(la), p(ra), p(lro), p(rro))
    assert wsb > 0
    bad = offs([0, 6, 4])                                       # non-monotone
    assert lib.eqd_dock_lddt_workspace_bytes(2, p(bad), p(ra), p(lro), p(rro)) == 0
    assert b'complex 1 has -2 ligand' in lib.eqd_dock_last_error()
    assert lib.eqd_dock_lddt_workspace_bytes(2, p(offs([0, 4, 4])), p(ra), p(lro), p(rro)) == 0          # an empty side
    assert b'complex 1 has 0 ligand' in lib.eqd_dock_last_error()
    assert lib.eqd_dock_lddt_workspace_bytes(2, p(offs([1, 4, 8])), p(ra), p(lro), p(rro)) == 0          # not starting at 0
    assert b'need 0' in lib.eqd_dock_last_error()
    assert lib.eqd_dock_lddt_workspace_bytes(2, p(la), p(ra), p(offs([0, 5, 7])), p(rro)) == 0          # 5 residues, 4 atoms
    assert b'tiles its complex' in lib.eqd_dock_last_error()
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    l2, r2 = torch.cat([lig, lig]), torch.cat([rec, rec])
    lf, rf = _t(np.int32([0, 2, 4, 6, 8]), dev), _t(np.int32([0, 2, 5, 7, 10]), dev)
    cnt = torch.full((18, 10), 7, dtype=torch.int32, device=dev)
    res = torch.full((8, 2), 7.0, dtype=torch.float64, device=dev)
    rows = torch.full((2, 16), 7.0, dtype=torch.float64, device=dev)
    st = DK._stream(dev)
    W = C.c_void_p(ws.data_ptr())
    assert lib.eqd_dock_lddt_init(2, p(bad), p(ra), p(lro), p(rro), W, C.c_size_t(wsb), st) == 2
    assert lib.eqd_dock_lddt_init(2, p(la), p(ra), p(lro), p(rro), W, C.c_size_t(64), st) == 4
    assert b'workspace too small' in lib.eqd_dock_last_error()

    def ev(la_, size, radius=15.0, thr=(0.5, 1.0, 2.0, 4.0), thr_null=False):
        return lib.eqd_dock_lddt_eval(2, p(la_), p(ra), p(lro), p(rro), C.c_void_p(l2.data_ptr()), C.c_void_p(0),
                                      C.c_void_p(l2.data_ptr()), C.c_void_p(r2.data_ptr()), C.c_void_p(lf.data_ptr()),
                                      C.c_void_p(rf.data_ptr()), C.c_double(radius),
                                      C.c_void_p(0) if thr_null else (C.c_double * 4)(*thr), 1,
                                      C.c_void_p(cnt.data_ptr()), C.c_void_p(cnt[8:].data_ptr()), C.c_void_p(res.data_ptr()),
                                      C.c_void_p(res[4:].data_ptr()), C.c_void_p(rows.data_ptr()), W, C.c_size_t(size), st)

    assert ev(bad, wsb) == 2 and b'complex 1 has -2 ligand' in lib.eqd_dock_last_error()
    assert ev(offs([0, 4, 4]), wsb) == 2 and ev(offs([1, 4, 8]), wsb) == 2
    assert ev(la, 64) == 4 and b'workspace too small' in lib.eqd_dock_last_error()
    assert ev(la, wsb, thr_null=True) == 1
    for v in (0.0, -1.0, float('inf'), float('nan')):
        assert ev(la, wsb, radius=v) == 2 and b'inclusion_radius' in lib.eqd_dock_last_error()
        for k in range(4):
            thr = [0.5, 1.0, 2.0, 4.0]
            thr[k] = v
            assert ev(la, wsb, thr=thr) == 2 and b'thresholds[%d]' % k in lib.eqd_dock_last_error()
    # nothing was written by the refused calls
    assert bool((cnt.cpu() == 7).all()) and bool((res.cpu() == 7.0).all()) and bool((rows.cpu() == 7.0).all())
    assert bool((ws.cpu() == 0).all())
    # and the same buffers take a good call
    assert lib.eqd_dock_lddt_init(2, p(la), p(ra), p(lro), p(rro), W, C.c_size_t(wsb), st) == 0
    assert ev(la, wsb) == 0
    assert rows.cpu()[:, 0].tolist() == [1.0, 1.0] and int(cnt.cpu()[:, 0].sum()) == int(rows.cpu()[:, 4].sum()) > 0


LDDT_FIELDS = {'lddt', 'ilddt', 'lddt_pairs', 'ilddt_pairs'}


def check_dock_complexes_lddt(dev, names, max_it, check_every):
    """dock_complexes(lddt=True): its fields equal a direct lddt_batch on the returned ligand_atoms; lddt=False returns
    what the call returns without the argument; without ground truth the option is refused"""
    net, _, _ = dc.seeded_net(dev)
    residues = [dc.fixture_residues(n) for n in names]
    truths = [lig for lig, _ in residues]
    kw = dict(remove_clashes=True, max_it=max_it, check_every=check_every, device=dev, ground_truth=truths)
    with pytest.raises(ValueError, match='lddt=True needs ground_truth'):
        DK.dock_complexes(net, residues, lddt=True, device=dev)
    plain = DK.dock_complexes(net, residues, **kw)
    off = DK.dock_complexes(net, residues, lddt=False, **kw)
    res = DK.dock_complexes(net, residues, lddt=True, **kw)
    tabs = [(DK.atom_table(lig), DK.atom_table(rec)) for lig, rec in residues]
    want = DK.lddt_batch([r['ligand_atoms'][_t(t[0][1], dev)] for r, t in zip(res, tabs)], [_t(t[0][0], dev) for t in tabs],
                         [_t(t[1][0], dev) for t in tabs], [t[0][2] for t in tabs], [t[1][2] for t in tabs])['rows'].cpu().numpy()
    for i in range(len(residues)):
        q, o, r = plain[i], off[i], res[i]
        assert set(o) == set(q) and set(o['batch_seconds']) == set(q['batch_seconds'])
        assert not (LDDT_FIELDS & set(q)) and set(r) - set(q) == LDDT_FIELDS, set(r) ^ set(q)
        assert set(r['batch_seconds']) - set(q['batch_seconds']) == {'lddt'}
        for a in (o, r):
            assert a['rotation'].tobytes() == q['rotation'].tobytes() and torch.equal(a['ligand_atoms'], q['ligand_atoms'])
            assert np.float64(a['crmsd']).tobytes() == np.float64(q['crmsd']).tobytes()
        assert _bits([r['lddt'], r['ilddt']]) == _bits(want[i, :2]), (names[i], r['lddt'], r['ilddt'], want[i])
        assert (r['lddt_pairs'], r['ilddt_pairs']) == (int(want[i, 4]), int(want[i, 5])) and r['lddt_pairs'] > 0
        assert isinstance(r['lddt'], float) and isinstance(r['lddt_pairs'], int) and 0.0 < r['lddt'] <= 1.0
    return res


def check_command_line(dev, tmp_path, capsys, names, max_it=5):
    """the command line's --lddt on a directory written with dock_common.write_pdb: exit 0, every complex's line ends with
    its lDDT and ilDDT - those of dock_complexes(lddt=True) on the same files to the printed digits -, the summary line is
    there; without the flag no line mentions lDDT; a missing ground-truth file gives exit 1 and names the file"""
    net, args, sd = dc.seeded_net(dev)
    ckpt = tmp_path / 'db5_model_best.pth'
    torch.save({'args': dict(args, device=torch.device('cpu'), graph_cutoff=30.0, graph_max_neighbor=10,
                             pocket_cutoff=8.0, intersection_loss_weight=10.0), 'state_dict': sd}, ckpt)
    inp, gt = tmp_path / 'in', tmp_path / 'gt'
    inp.mkdir()
    gt.mkdir()
    tags = [f'CX{k}A' for k in range(len(names))]
    for nm, fx in zip(tags, names):
        lig, rec = dc.fixture_residues(fx)
        dc.write_pdb(lig, inp / f'{nm}_l_b.pdb')
        dc.write_pdb(rec, gt / f'{nm}_r_b_COMPLEX.pdb')
        dc.write_pdb(lig, gt / f'{nm}_l_b_COMPLEX.pdb')
    complexes = [(str(inp / f'{nm}_l_b.pdb'), str(gt / f'{nm}_r_b_COMPLEX.pdb')) for nm in tags]
    truths = [str(gt / f'{nm}_l_b_COMPLEX.pdb') for nm in tags]
    base = ['--checkpoint', str(ckpt), '--input-dir', str(inp), '--gt-dir', str(gt), '--remove-clashes', '--max-it',
            str(max_it), '--device', str(dev)]

    def cli(out, *flags, code=0):
        capsys.readouterr()
        rc = DK.main(base + ['--out-dir', str(tmp_path / out)] + list(flags))
        cap = capsys.readouterr()
        assert rc == code, cap.err
        return cap.out.strip().splitlines(), cap.err

    plain, _ = cli('out0')
    assert not any('lDDT' in ln for ln in plain)
    want = DK.dock_complexes(net, complexes, remove_clashes=True, max_it=max_it, device=dev, ground_truth=truths, lddt=True)
    lines, _ = cli('out1', '--lddt')
    pat = re.compile(r'^(\w+): .*  lDDT ([\d.]+|nan)  ilDDT ([\d.]+|nan)$')
    for ln, nm, r in zip(lines, tags, want):
        m = pat.match(ln)
        assert m and m.group(1) == nm and m.group(2) == f"{r['lddt']:.4f}" and m.group(3) == f"{r['ilddt']:.4f}", (ln, r)
    il = np.float64([r['ilddt'] for r in want])
    ok = il[~np.isnan(il)]
    assert ok.size > 0
    tail = "ilDDT median/mean/std: %.4f / %.4f / %.4f" % (np.median(ok), np.mean(ok), np.std(ok))
    if ok.size < il.size:
        tail += "  undefined %d" % (il.size - ok.size)
    assert lines[-1] == tail, (lines[-1], tail)
    assert len(lines) == len(plain) + 1
    os.remove(truths[-1])
    _, err = cli('out2', '--lddt', code=1)
    assert os.path.basename(truths[-1]) in err and '--lddt' in err
