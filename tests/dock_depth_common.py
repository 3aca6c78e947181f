"""Checks of the batched residue depth (equidock_public_amd.dock.residue_depth_batch / DepthPlan / spearman /
surface_feature_analysis, eqd_dock_depth_* of libequidock_dock.so) shared by the simulator tests
(tests/test_dock_depth_sim.py) and the GPU tests (tests/test_dock_depth_gpu.py).

Yardstick: `ref64_depth`, a float64 numpy evaluation of the definitions of include/equidock_dock.h written without the
kernels' decomposition (no tiles, no staging, no pruning): the exposure of every sphere point as in
tests/dock_surface_common.ref64, the vertices x_i + r_i * u_k of the exposed points, and per atom the minimum of the
header's expression over ALL vertices of the state, dense.

Required agreement.  s_alone and s_complex of every atom: EQUAL, bit for bit.  Every integer column (8-13, 15): equal;
columns 12 / 13 also equal surface_area_batch's points_alone / points_complex on the same inputs.  depth: within 1 ulp
(relative 2^-52) of np.sqrt of the yardstick's s.  Residue means and columns 0-7: within BOUND = 1e-9 Angstrom absolute:
sums of at most 2e4 non-negative terms of at most 30 A differ between summation orders by at most n * eps * total ~
2e4 * 1.1e-16 * 6e5 ~ 1.3e-9 A in the worst case; at the sizes tested here (<= 3 000 atoms) that is 3e-11 A.  Every case
asserts from the yardstick that no point test lies within 1e-9 A of its sphere (`margin`).

Measured over all cases of this file (the tests print both):
    kernels on the x86 simulator    depth == np.sqrt(s) on every atom: yes    worst error of a mean 3.331e-15 A
    kernels on the MI355X           depth == np.sqrt(s) on every atom: yes    worst error of a mean 3.331e-15 A
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from equidock_public_amd import _lib, dock as DK
from tests import dock_common as dc
from tests import dock_surface_common as sc
from tests.dock_surface_common import fixture_cases as surface_fixture_cases, globules, radii_by_name

BOUND = 1e-9
ULP = 2.0 ** -52
PROBE, POINTS = 1.4, 96
TILE, ROWS = 64, 256                # the kernels as built (csrc_dock/eqd_dock_depth.hip): rows per tile, per finish step
INT_COLS = (8, 9, 10, 11, 12, 13, 15)


# ---- the float64 yardstick ------------------------------------------------------------------------------------------
def exposure64(x, R, side, u):
    """exposed [n][P][2] bool (alone, in complex) of the points x_i + R_i * u_k, and the margin of the point tests"""
    n = len(x)
    D = np.empty((n, n))
    for i0 in range(0, n, 512):
        d = x[i0:i0 + 512, None, :] - x[None, :, :]
        D[i0:i0 + 512] = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    cand = (D < R[:, None] + R[None, :] + 0.5) & ~np.eye(n, dtype=bool)
    exposed = np.ones((n, len(u), 2), dtype=bool)
    margin = np.inf
    for i in range(n):
        j = np.nonzero(cand[i])[0]
        if len(j) == 0:
            continue
        q = x[i] + R[i] * u
        d = q[:, None, :] - x[j][None, :, :]
        s = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        margin = min(margin, float(np.abs(np.sqrt(s) - R[j][None, :]).min()))
        hit = s < (R[j] * R[j])[None, :]
        exposed[i, :, 0] = ~hit[:, side[j] == side[i]].any(1)
        exposed[i, :, 1] = ~hit.any(1)
    return exposed, margin


def nearest64(x, v):
    """per row of x the minimum over the vertices v of (dx dx + dy dy) + dz dz, d = x - v; +inf without vertices"""
    out = np.full(len(x), np.inf)
    if len(v) == 0:
        return out
    for i0 in range(0, len(x), 128):
        d = x[i0:i0 + 128, None, :] - v[None, :, :]
        out[i0:i0 + 128] = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).min(1)
    return out


def ca_rows(names, off):
    """independent of dock._ca_rows: the first row named CA of every residue, -1 without one"""
    out = []
    for a, b in zip(off[:-1], off[1:]):
        hit = [k for k in range(int(a), int(b)) if names is not None and str(names[k]).strip() == 'CA']
        out.append(hit[0] if hit else -1)
    return np.asarray(out, dtype=np.int64)


def ref64_depth(lig, rec, lrad, rrad, lo, ro, lnames=None, rnames=None, probe=PROBE, n_points=POINTS):
    x = np.concatenate((np.asarray(lig, dtype=np.float64), np.asarray(rec, dtype=np.float64)))
    r = np.concatenate((np.asarray(lrad, dtype=np.float32), np.asarray(rrad, dtype=np.float32))).astype(np.float64)
    nl, n = len(lig), len(x)
    side = np.arange(n) >= nl
    u = DK.sphere_points(n_points)
    exposed, margin = exposure64(x, r + probe, side, u)
    vert = x[:, None, :] + r[:, None, None] * u[None, :, :]                    # [n][P][3]: one multiply, one add
    s = np.empty((n, 2))
    s[:nl, 0] = nearest64(x[:nl], vert[:nl][exposed[:nl, :, 0]])
    s[nl:, 0] = nearest64(x[nl:], vert[nl:][exposed[nl:, :, 0]])
    s[:, 1] = nearest64(x, vert[exposed[:, :, 1]])
    depth = np.sqrt(s)
    lo, ro = np.asarray(lo, dtype=np.int64), np.asarray(ro, dtype=np.int64)
    first = np.concatenate((lo[:-1], ro[:-1] + nl))
    count = np.diff(np.concatenate((first, [n]))).astype(np.float64)
    ca = np.concatenate((ca_rows(lnames, lo), np.where(ca_rows(rnames, ro) >= 0, ca_rows(rnames, ro) + nl, -1)))
    res = np.full((len(first), 4), np.nan)
    res[:, 0] = np.add.reduceat(depth[:, 0], first) / count
    res[:, 1] = np.add.reduceat(depth[:, 1], first) / count
    res[ca >= 0, 2] = depth[ca[ca >= 0], 0]
    res[ca >= 0, 3] = depth[ca[ca >= 0], 1]
    deep = s[:, 1] > s[:, 0]
    deep_res = np.add.reduceat(deep.astype(np.int64), first) > 0
    nrl = len(lo) - 1
    va_l, va_r, vc = int(exposed[:nl, :, 0].sum()), int(exposed[nl:, :, 0].sum()), int(exposed[:, :, 1].sum())
    gain = depth[:, 1] - depth[:, 0]
    row = np.float64([depth[:nl, 0].sum() / nl, depth[nl:, 0].sum() / (n - nl), depth[:, 1].sum() / n, depth[:nl, 0].max(),
                      depth[nl:, 0].max(), depth[:, 1].max(), gain[:nl].sum() / nl, gain[nl:].sum() / (n - nl),
                      deep[:nl].sum(), deep[nl:].sum(), deep_res[:nrl].sum(), deep_res[nrl:].sum(), va_l + va_r, vc, np.nan,
                      (1 if va_l == 0 else 0) | (2 if va_r == 0 else 0) | (4 if vc == 0 else 0)])
    return {'s': s, 'depth': depth, 'res': res, 'row': row, 'margin': margin, 'exposed': exposed, 'ca': ca, 'nl': nl}


_worst = {}


def check_complex(name, got, ref, key):
    """one complex of a batch (see `run`) against the yardstick"""
    assert ref['margin'] > 1e-9, (name, ref['margin'])
    assert got['depth'].dtype == np.float64 and got['depth'].shape == (len(ref['s']), 4)
    bad = np.nonzero((got['depth'][:, :2] != ref['s']).any(1))[0]
    assert len(bad) == 0, (name, 'squared depths differ at rows', bad[:8], got['depth'][bad[:8], :2], ref['s'][bad[:8]])
    want = np.sqrt(ref['s'])
    assert (np.abs(got['depth'][:, 2:] - want) <= ULP * want).all(), (name, 'depth is not within 1 ulp of sqrt(s)')
    w = _worst.setdefault(key, {'equal': True, 'err': 0.0})
    w['equal'] = w['equal'] and bool((got['depth'][:, 2:] == want).all())
    row = got['row']
    for k in INT_COLS:
        assert row[k] == ref['row'][k], (name, DK.DEPTH_KEYS[k], row[k], ref['row'][k])
    assert row[14] >= 0 and row[14] == np.floor(row[14])
    err = max(float(np.abs(got['res'][:, :2] - ref['res'][:, :2]).max()), float(np.abs(row[:8] - ref['row'][:8]).max()))
    assert err <= BOUND, f"{name}: worst mean error {err:.3e} > {BOUND:g}"
    # maxima are order-free: equal to the yardstick's up to the square root's ulp
    assert (np.abs(row[3:6] - ref['row'][3:6]) <= ULP * ref['row'][3:6]).all(), (name, row[3:6], ref['row'][3:6])
    no_ca = ref['ca'] < 0
    assert np.array_equal(np.isnan(got['res'][:, 2]), no_ca) and np.array_equal(np.isnan(got['res'][:, 3]), no_ca), name
    assert got['res'][~no_ca, 2:].tobytes() == got['depth'][ref['ca'][~no_ca], 2:].tobytes(), (name, 'CA depths')
    w['err'] = max(w['err'], err)
    return err


def report(dev):
    key = torch.device(dev).type
    w = _worst.get(key, {'equal': True, 'err': 0.0})
    print(f"dock depth [{key}]: depth == np.sqrt(s) everywhere so far: {'yes' if w['equal'] else 'no'}; worst mean error "
          f"{w['err']:.3e} A (bound {BOUND:g})")


# ---- running --------------------------------------------------------------------------------------------------------
def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run(dev, cases, n_points=POINTS, probe=PROBE, full=False, plan=None):
    """one residue_depth_batch over `cases` [(lig, rec, lig radii, rec radii, lig residue offsets, rec residue offsets, lig
    names, rec names)] -> per complex {'row' [16], 'depth' [n][4] (ligand rows first), 'res' [r][4]} on the host"""
    cases = list(cases)
    out = DK.residue_depth_batch([_t(c[0], dev) for c in cases], [_t(c[1], dev) for c in cases], [c[2] for c in cases],
                                 [c[3] for c in cases], [c[4] for c in cases], [c[5] for c in cases],
                                 lig_names=[c[6] for c in cases], rec_names=[c[7] for c in cases], probe=probe,
                                 n_points=n_points, plan=plan)
    kind = torch.device(dev).type
    for k in DK.DEPTH_KEYS:
        assert out[k].dtype == torch.float64 and out[k].shape == (len(cases),) and out[k].device.type == kind
    assert out['rows'].shape == (len(cases), DK.DEPTH_COLS) and out['lig_depth'].dtype == torch.float64
    if full:
        return out
    rows = out['rows'].cpu().numpy()
    lp, rp = out['lig_depth'].cpu().numpy(), out['rec_depth'].cpu().numpy()
    la, ra = out['lig_res_depth'].cpu().numpy(), out['rec_res_depth'].cpu().numpy()
    res, a = [], [0, 0, 0, 0]
    for c, case in enumerate(cases):
        b = [a[0] + len(case[0]), a[1] + len(case[1]), a[2] + len(case[4]) - 1, a[3] + len(case[5]) - 1]
        res.append({'row': rows[c], 'depth': np.concatenate((lp[a[0]:b[0]], rp[a[1]:b[1]])),
                    'res': np.concatenate((la[a[2]:b[2]], ra[a[3]:b[3]]))})
        a = b
    assert a == [len(lp), len(rp), len(la), len(ra)]
    return res


def same_bits(a, b, what, but_skipped=False):
    for k in ('depth', 'res'):
        assert a[k].tobytes() == b[k].tobytes(), (what, k)
    cols = [k for k in range(DK.DEPTH_COLS) if not (but_skipped and k == 14)]
    assert a['row'][cols].tobytes() == b['row'][cols].tobytes(), (what, 'row', a['row'], b['row'])


# ---- cases ------------------------------------------------------------------------------------------------------------
def synth_names(off):
    """N CA C O CB ... per residue; every third residue has no atom named CA (nor has a residue of one atom)"""
    pool = ['N', 'CA', 'C', 'O', 'CB', 'CG', 'CD', 'CE', 'NZ', 'OH', 'SD', 'CZ', 'NE', 'OG']
    out = []
    for k, (a, b) in enumerate(zip(off[:-1], off[1:])):
        nm = [pool[j] if j < len(pool) else f'X{j}' for j in range(int(b - a))]
        if k % 3 == 2 and len(nm) > 1:
            nm[1] = 'CX'
        out += nm
    return np.asarray(out, dtype=str)


def named(case):
    return tuple(case) + (synth_names(case[4]), synth_names(case[5]))


@functools.lru_cache(maxsize=None)
def fixture_cases():
    """1AVX and 1HCF of tests/golden/dockq_case.npz, native and lig_equidock poses, with their atom names"""
    z = np.load(os.path.join(dc.GOLDEN, 'dockq_case.npz'))
    return {k: tuple(v) + (z[f'{k[:4]}_lig_true_names'], z[f'{k[:4]}_rec_true_names'])
            for k, v in surface_fixture_cases().items()}


# sides either side of the 64-row vertex / target tile and of the finish step (256), sides of ONE atom, a residue of more
# than 64 atoms (dock_surface_common.EDGES)
EDGE_NAMES = ('edge_63x255', 'edge_64x256', 'edge_65x257', 'edge_255x63', 'edge_256x64', 'edge_257x65', 'edge_1x70',
              'edge_70x1', 'edge_1x1', 'edge_long_residue')
P_EDGES = (1, 63, 64, 65, 96, 130)          # either side of the 64-bit mask word


@functools.lru_cache(maxsize=None)
def edge_cases():
    e = sc.edge_cases()
    return {k: named(e[k]) for k in EDGE_NAMES}


@functools.lru_cache(maxsize=None)
def p_case(n_points):
    return named(sc.p_case(n_points))


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def degenerate_cases():
    out = {}
    lx, rx, lr, rr, lo, ro = globules(70, 90, 601)
    # two sides far apart; no atom names at all: every CA depth is NaN
    out['far_sides'] = (_f32(lx - np.float32([200.0, 0.0, 0.0])), rx, lr, rr, lo, ro, None, None)
    # a buried tile: the ligand's first 64 rows packed inside a ball of 2 A, enclosed by two shells of ligand atoms
    seed = 701
    while True:
        rng = np.random.default_rng(seed)
        v = rng.standard_normal((64, 3))
        core = v / np.linalg.norm(v, axis=1, keepdims=True) * 2.0 * rng.uniform(0.0, 1.0, (64, 1)) ** (1.0 / 3.0)
        shell = np.concatenate((DK.sphere_points(150) * 4.5, DK.sphere_points(220) * 6.2)) + rng.standard_normal((370, 3)) * 0.1
        ex = _f32(np.concatenate((core, shell)) + sc.OFFSET)
        er = rng.choice(sc.RADII, len(ex)).astype(np.float32)
        eo = np.int32(list(range(0, 64, 8)) + list(range(64, len(ex), 10)) + [len(ex)])
        gx, gr, go, _ = sc._globule(rng, 60, sc.OFFSET + np.array([11.0, 0.0, 0.0]))
        case = named((ex, gx, er, gr, eo, go))
        if ref64_depth(*case)['margin'] > 1e-9:
            break
        seed += 1000
    out['buried_tile'] = case
    return out


def all_cases():
    return {**fixture_cases(), **edge_cases(), **degenerate_cases()}


_refs = {}


def reference(name, case, n_points=POINTS):
    if (name, n_points) not in _refs:
        _refs[(name, n_points)] = ref64_depth(*case, n_points=n_points)
    return _refs[(name, n_points)]


_measured = {}


def batch_order():
    """the real poses with edge cases between them"""
    f, rest = list(fixture_cases()), list(edge_cases()) + list(degenerate_cases())
    k = (len(rest) + len(f) - 1) // len(f)
    order = []
    for i, n in enumerate(f):
        order += [n] + rest[i * k:(i + 1) * k]
    assert sorted(order) == sorted(all_cases())
    return order


def measured(dev):
    """ALL cases of this file (P = 96) in ONE batch - computed once per device type and shared by the tests"""
    key = torch.device(dev).type
    if key not in _measured:
        cases, names = all_cases(), batch_order()
        _measured[key] = dict(zip(names, run(dev, [cases[n] for n in names])))
    return _measured[key]


def check_names(dev, names):
    got, cases, key = measured(dev), all_cases(), torch.device(dev).type
    for n in names:
        check_complex(n, got[n], reference(n, cases[n]), key)
    report(dev)
    return {n: got[n] for n in names}


def _surface_points(dev, cases, n_points=POINTS):
    out = DK.surface_area_batch([_t(c[0], dev) for c in cases], [_t(c[1], dev) for c in cases], [c[2] for c in cases],
                                [c[3] for c in cases], [c[4] for c in cases], [c[5] for c in cases], n_points=n_points)
    return out['rows'][:, 10:12].cpu().numpy()


# ---- the checks -------------------------------------------------------------------------------------------------------
def check_yardstick_reproduces_the_issue():
    """CPU: ref64_depth on 1AVX gives the figures recorded with the issue's prototype"""
    f = fixture_cases()
    r = reference('1AVX_native', f['1AVX_native'])
    assert len(r['s']) == 2916 and (r['row'][12], r['row'][13]) == (15304, 13998), r['row']
    assert abs(max(r['row'][3], r['row'][4]) - 6.94) < 0.005, r['row'][3:5]
    assert r['row'][8] + r['row'][9] == 186, r['row'][8:10]
    e = reference('1AVX_EQUIDOCK', f['1AVX_EQUIDOCK'])
    assert int((e['s'][:, 1] < e['s'][:, 0]).sum()) == 7      # depth_complex >= depth_alone is NOT an invariant
    s = sc.reference('1AVX_native', f['1AVX_native'][:6])
    assert (s['points_alone'], s['points_complex']) == (15304, 13998)


def check_real(dev):
    """1AVX and 1HCF, native and lig_equidock poses, in ONE batch with the edge cases between them; columns 12 / 13 are
    surface_area_batch's point counts on the same inputs"""
    names = list(fixture_cases())
    got = check_names(dev, names)
    order = batch_order()
    pos = [order.index(n) for n in names]
    assert all(b - a > 1 for a, b in zip(pos[:-1], pos[1:])), pos
    pts = _surface_points(dev, [fixture_cases()[n] for n in names])
    for n, p in zip(names, pts):
        assert got[n]['row'][12:14].tobytes() == p.tobytes(), (n, got[n]['row'][12:14], p)
        assert got[n]['row'][14] > 0 and got[n]['row'][15] == 0
    assert got['1AVX_native']['row'][8] + got['1AVX_native']['row'][9] == 186


def check_edges(dev):
    """tile and finish-step edges, sides and residues of one atom, a residue of more than 64 atoms; n_points either side of
    the mask word"""
    cases = edge_cases()
    got = check_names(dev, list(cases))
    per_side = {len(c[k]) for c in cases.values() for k in (0, 1)}
    for size in (TILE, ROWS):
        assert {size - 1, size, size + 1} <= per_side, (size, per_side)
    assert 1 in per_side and np.diff(cases['edge_long_residue'][4]).max() > 64
    pts = _surface_points(dev, list(cases.values()))
    for n, p in zip(cases, pts):
        assert got[n]['row'][12:14].tobytes() == p.tobytes(), (n, got[n]['row'][12:14], p)
    key = torch.device(dev).type
    for P in P_EDGES:
        case = p_case(P)
        g = run(dev, [case], n_points=P)[0]
        check_complex(f'P={P}', g, reference(f'P={P}', case, P), key)
        assert g['row'][12:14].tobytes() == _surface_points(dev, [case], P)[0].tobytes(), P
    report(dev)


def check_degenerate(dev):
    """a 64-row-aligned tile without any exposed vertex; two sides far apart; atom names omitted"""
    cases = degenerate_cases()
    got = check_names(dev, list(cases))
    r = reference('buried_tile', cases['buried_tile'])
    assert not r['exposed'][:TILE].any(), 'the first tile of the ligand must own no vertex in either state'
    assert r['exposed'][TILE:r['nl']].any() and np.isfinite(r['s']).all() and r['s'][:TILE, 0].min() > 1.0
    g, r = got['far_sides'], reference('far_sides', cases['far_sides'])
    assert g['row'][12] == g['row'][13] > 0 and (g['row'][8:12] == 0).all()
    assert g['depth'][:, 0].tobytes() == g['depth'][:, 1].tobytes() and g['depth'][:, 2].tobytes() == g['depth'][:, 3].tobytes()
    assert np.isnan(g['res'][:, 2:]).all() and (r['ca'] < 0).all()
    assert g['row'][6] == 0.0 and g['row'][7] == 0.0
    # residues without a CA among residues with one
    e = reference('edge_65x257', edge_cases()['edge_65x257'])
    assert (e['ca'] < 0).any() and (e['ca'] >= 0).any()


def check_pruning_switch(dev, monkeypatch):
    """EQD_DOCK_DEPTH_PRUNE=0 against the default on the real poses: every output is bit-equal but column 14, which is 0
    when off and > 0 when on"""
    cases = fixture_cases()
    names = list(cases)
    default = measured(dev)
    assert DK.depth_pruning_enabled()
    monkeypatch.setenv('EQD_DOCK_DEPTH_PRUNE', '0')
    assert not DK.depth_pruning_enabled()
    off = run(dev, [cases[n] for n in names])
    monkeypatch.undo()
    assert DK.depth_pruning_enabled()
    for n, g in zip(names, off):
        same_bits(default[n], g, f'{n}: pruning on vs off', but_skipped=True)
        assert g['row'][14] == 0 and default[n]['row'][14] > 0, (n, g['row'][14], default[n]['row'][14])


def check_bits(dev):
    """each complex of a batch of two real poses and two edge cases alone, first, last, in permuted batches and twice in a
    row: the same bytes"""
    cases = all_cases()
    names = ['1AVX_EQUIDOCK', 'edge_65x257', '1HCF_native', 'buried_tile']
    cs = [cases[n] for n in names]
    k = len(cs)
    together, again = run(dev, cs), run(dev, cs)
    first, last = {0}, {k - 1}
    for i, n in enumerate(names):
        same_bits(together[i], again[i], f'{n}: run to run')
        same_bits(together[i], run(dev, [cs[i]])[0], f'{n}: alone')
        same_bits(together[i], measured(dev)[n], f'{n}: in the batch of all cases')
    for perm in ([2, 0, 3, 1], [1, 3, 0, 2], [3, 1, 2, 0]):    # every complex comes first and last once
        permuted = run(dev, [cs[p] for p in perm])
        first.add(perm[0])
        last.add(perm[-1])
        for j, o in enumerate(perm):
            same_bits(together[o], permuted[j], f'{names[o]}: permuted batch {perm}')
    assert first == last == set(range(k))


def check_validation_errors(dev):
    """refused before any launch, with a message (the entry points and residue_depth_batch)"""
    lib = DK.load_dock_library()
    assert lib.eqd_dock_depth_abi() == DK.DOCK_DEPTH_ABI == 1 and DK.DEPTH_COLS == 16 and len(DK.DEPTH_KEYS) == 16
    lig, rec = torch.zeros(4, 3, device=dev), torch.ones(5, 3, device=dev)
    lo, ro = np.int32([0, 2, 4]), np.int32([0, 1, 5])
    lr, rr = np.float32([1.7, 1.55, 1.52, 1.8]), np.full(5, 1.7, np.float32)
    good = dict(lig_radii=[lr], rec_radii=[rr], lig_res_offsets=[lo], rec_res_offsets=[ro])
    assert DK.residue_depth_batch([lig], [rec], **good)['rows'].shape == (1, 16)
    with pytest.raises(ValueError, match='ligands for'):
        DK.residue_depth_batch([lig, lig], [rec], **good)
    with pytest.raises(ValueError, match='are needed'):
        DK.residue_depth_batch([lig], [rec])
    with pytest.raises(ValueError, match='complex 0: ligand: residue offsets'):
        DK.residue_depth_batch([lig], [rec], **dict(good, lig_res_offsets=[np.int32([0, 2, 3])]))
    with pytest.raises(ValueError, match='rows for tables of'):
        DK.residue_depth_batch([lig[:3]], [rec], **good)
    with pytest.raises(ValueError, match='atom names for'):
        DK.residue_depth_batch([lig], [rec], lig_names=[['N', 'CA']], **good)
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='complex 0: ligand: radii must be finite and > 0'):
            DK.residue_depth_batch([lig], [rec], **dict(good, lig_radii=[np.float32([1.7, bad, 1.5, 1.8])]))
        with pytest.raises(ValueError, match='complex 0: receptor: radii'):
            DK.residue_depth_batch([lig], [rec], **dict(good, rec_radii=[np.float32([1.7, 1.7, 1.7, 1.7, bad])]))
    for bad in (0.0, float('nan'), float('inf')):
        with pytest.raises(_lib.EquidockHipError, match='probe'):
            DK.residue_depth_batch([lig], [rec], probe=bad, **good)
    for bad in (0, 1025):
        with pytest.raises(ValueError, match='sphere_points'):
            DK.residue_depth_batch([lig], [rec], n_points=bad, **good)
    # a plan of another size; tensors on the wrong kind of device
    plan = DK.DepthPlan([lo, lo], [ro, ro], [lr, lr], [rr, rr], dev)
    with pytest.raises(ValueError, match='the plan holds 2 complexes'):
        DK.residue_depth_batch([lig], [rec], plan=plan)
    with pytest.raises(ValueError, match='rows for tables of'):
        DK.residue_depth_batch([lig, lig[:3]], [rec, rec], plan=plan)
    if torch.device(dev).type == 'cuda':
        with pytest.raises(_lib.EquidockHipError, match='no CPU fallback'):
            DK.residue_depth_batch([lig.cpu()], [rec.cpu()], **good)
    elif torch.cuda.is_available():
        with pytest.raises(_lib.EquidockHipError, match='only takes CPU tensors'):
            DK.residue_depth_batch([lig.cuda()], [rec.cuda()], **good)
    else:
        with pytest.raises(_lib.EquidockHipError, match='only takes CPU tensors'):
            DK._require_device(_FakeCuda(), 'depth inputs')

    def offs(v):
        return np.ascontiguousarray(np.asarray(v, dtype=np.int32))

    def p(a):
        return a.ctypes.data_as(C.c_void_p)

    la, ra, lro, rro = offs([0, 4, 8]), offs([0, 5, 10]), offs([0, 2, 4]), offs([0, 2, 4])
    wsb = lib.eqd_dock_depth_workspace_bytes(2, p(la), p(ra), p(lro), p(rro), 96)
    assert wsb > 0
    bad = offs([0, 6, 4])
    assert lib.eqd_dock_depth_workspace_bytes(2, p(bad), p(ra), p(lro), p(rro), 96) == 0
    assert b'complex 1 has -2 ligand' in lib.eqd_dock_last_error()
    assert lib.eqd_dock_depth_workspace_bytes(2, p(offs([0, 4, 4])), p(ra), p(lro), p(rro), 96) == 0         # an empty side
    assert lib.eqd_dock_depth_workspace_bytes(2, p(offs([1, 4, 8])), p(ra), p(lro), p(rro), 96) == 0
    assert lib.eqd_dock_depth_workspace_bytes(2, p(la), p(ra), p(offs([0, 5, 7])), p(rro), 96) == 0         # 5 residues, 4 atoms
    assert b'tiles its complex' in lib.eqd_dock_last_error()
    for P in (0, 1025, -3):
        assert lib.eqd_dock_depth_workspace_bytes(2, p(la), p(ra), p(lro), p(rro), P) == 0
        assert b'n_points' in lib.eqd_dock_last_error()
    assert lib.eqd_dock_depth_workspace_bytes(2, p(la), p(ra), p(lro), p(rro), 1024) > wsb                  # 16 mask words
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    l2, r2 = torch.cat([lig, lig]), torch.cat([rec, rec])
    lrad, rrad = torch.full((8,), 1.7, device=dev), torch.full((10,), 1.7, device=dev)
    lf, rf = _t(np.int32([0, 2, 4, 6, 8]), dev), _t(np.int32([0, 2, 5, 7, 10]), dev)
    lca, rca = _t(np.int32([0, -1, 4, 6]), dev), _t(np.int32([-1, 2, 5, 7]), dev)
    sphere = _t(DK.sphere_points(96), dev)
    dep = torch.full((18, 4), 7.0, dtype=torch.float64, device=dev)
    res = torch.full((8, 4), 7.0, dtype=torch.float64, device=dev)
    rows = torch.full((2, 16), 7.0, dtype=torch.float64, device=dev)
    st = DK._stream(dev)
    W = C.c_void_p(ws.data_ptr())
    assert lib.eqd_dock_depth_init(2, p(bad), p(ra), p(lro), p(rro), 96, W, C.c_size_t(wsb), st) == 2
    assert lib.eqd_dock_depth_init(2, p(la), p(ra), p(lro), p(rro), 0, W, C.c_size_t(wsb), st) == 2
    assert lib.eqd_dock_depth_init(2, p(la), p(ra), p(lro), p(rro), 96, W, C.c_size_t(64), st) == 4
    assert b'workspace too small' in lib.eqd_dock_last_error()

    def ev(la_, size, P=96, probe=1.4, sph=sphere):
        return lib.eqd_dock_depth_eval(2, p(la_), p(ra), p(lro), p(rro), C.c_void_p(l2.data_ptr()), C.c_void_p(r2.data_ptr()),
                                       C.c_void_p(lrad.data_ptr()), C.c_void_p(rrad.data_ptr()), C.c_void_p(lf.data_ptr()),
                                       C.c_void_p(rf.data_ptr()), C.c_void_p(lca.data_ptr()), C.c_void_p(rca.data_ptr()),
                                       C.c_void_p(sph.data_ptr()) if sph is not None else C.c_void_p(0), P, C.c_double(probe),
                                       1, C.c_void_p(dep.data_ptr()), C.c_void_p(dep[8:].data_ptr()),
                                       C.c_void_p(res.data_ptr()), C.c_void_p(res[4:].data_ptr()),
                                       C.c_void_p(rows.data_ptr()), W, C.c_size_t(size), st)

    assert ev(bad, wsb) == 2
    assert ev(la, 64) == 4
    assert ev(la, wsb, sph=None) == 1
    for P in (0, 1025):
        assert ev(la, wsb, P=P) == 2 and b'n_points' in lib.eqd_dock_last_error()
    for v in (0.0, -1.0, float('inf'), float('nan')):
        assert ev(la, wsb, probe=v) == 2 and b'probe' in lib.eqd_dock_last_error()
    # nothing was written by the refused calls
    assert bool((dep.cpu() == 7.0).all()) and bool((res.cpu() == 7.0).all()) and bool((rows.cpu() == 7.0).all())
    assert bool((ws.cpu() == 0).all())


class _FakeCuda:
    """a stand-in with the one attribute dock._require_device reads (no GPU at hand: the converse device check)"""
    is_cuda = True
    device = 'cuda:0'


def _ranks_by_hand(v):
    out = []
    for i in range(len(v)):
        less = sum(1 for j in range(len(v)) if v[j] < v[i])
        same = sum(1 for j in range(len(v)) if v[j] == v[i])
        out.append(less + (same + 1) / 2.0)
    return np.float64(out)


def spearman_by_hand(a, b):
    if len(a) < 2:
        return float('nan')
    ra, rb = _ranks_by_hand(list(a)), _ranks_by_hand(list(b))
    da, db = ra - ra.mean(), rb - rb.mean()
    den = np.sqrt((da * da).sum() * (db * db).sum())
    return float((da * db).sum() / den) if den > 0 else float('nan')


def check_spearman():
    """against a double-loop rank implementation (ties, a constant input, n < 2, perfect +-1) and scipy when it imports"""
    rng = np.random.default_rng(11)
    sets = [(rng.standard_normal(50), rng.standard_normal(50)), (rng.integers(0, 5, 40).astype(float), rng.standard_normal(40)),
            (rng.integers(0, 3, 30).astype(float), rng.integers(0, 4, 30).astype(float)), (np.arange(7.0), np.arange(7.0) ** 3),
            (np.arange(7.0), -np.exp(np.arange(7.0))), (np.float64([1, 2]), np.float64([5, 4]))]
    for a, b in sets:
        got, want = DK.spearman(a, b), spearman_by_hand(a, b)
        assert abs(got - want) <= 1e-14, (got, want)
        assert DK.spearman(torch.from_numpy(a), b) == got
    assert DK.spearman(np.arange(7.0), np.arange(7.0) ** 3) == 1.0 and DK.spearman(np.arange(7.0), -np.exp(np.arange(7.0))) == -1.0
    assert np.isnan(DK.spearman(np.ones(9), rng.standard_normal(9))) and np.isnan(DK.spearman(rng.standard_normal(9), np.zeros(9)))
    assert np.isnan(DK.spearman([], [])) and np.isnan(DK.spearman([1.0], [2.0]))
    with pytest.raises(ValueError, match='spearman'):
        DK.spearman([1.0, 2.0], [1.0])
    try:
        from scipy import stats
    except ImportError:
        return
    for a, b in sets:
        assert abs(DK.spearman(a, b) - float(stats.spearmanr(a, b)[0])) <= 1e-12


# ---- the surface-feature analysis -------------------------------------------------------------------------------------
def _heavy(name, element):
    el = element.strip().upper()
    return (el or name.strip().lstrip('0123456789')[:1].upper()) not in ('H', 'D')


def residue_means_by_hand(lig, rec, probe=PROBE, n_points=POINTS):
    """the yardstick's mean depth alone of every residue of two residue lists that has a heavy atom, keyed by (side, list
    index) - a mapping written without dock.atom_table"""
    sides, first = [], []
    for res in (lig, rec):
        xs, rad, off, idx = [], [], [0], []
        for i, r in enumerate(res):
            rows = [(nm, el, xyz) for nm, el, xyz in zip(r.atom_names, r.elements, r.coords) if _heavy(nm, el)]
            if not rows:
                continue
            idx.append(i)
            xs += [xyz for _, _, xyz in rows]
            rad += [DK.ATOM_RADII.get(el.strip().upper() or nm.strip().lstrip('0123456789')[:1].upper(), DK.DEFAULT_RADIUS)
                    for nm, el, _ in rows]
            off.append(len(xs))
        sides.append((np.float32(xs).reshape(-1, 3), np.float32(rad), np.int32(off)))
        first.append(idx)
    ref = ref64_depth(sides[0][0], sides[1][0], sides[0][1], sides[1][1], sides[0][2], sides[1][2], probe=probe,
                      n_points=n_points)
    assert ref['margin'] > 1e-9
    nrl = len(first[0])
    out = {(0, i): ref['res'][k, 0] for k, i in enumerate(first[0])}
    out.update({(1, i): ref['res'][nrl + k, 0] for k, i in enumerate(first[1])})
    return out


def check_surface_feature_analysis(dev, names=('graph_case', 'graph_case_tiny')):
    """surface_feature_analysis on residue lists: the depth vectors are the yardstick's residue means picked by an
    independent mapping, the features are -mu_r_norm[:, 4] of protein_graphs_batch, the correlation is spearman of the
    two; a side with a single residue that passes the filter is unmappable: NaN, nothing raised"""
    from equidock_public_amd import featurize as FZ
    pairs = [dc.fixture_residues(n) for n in names]
    lig0, rec0 = pairs[0]
    keep0 = [i for i, r in enumerate(lig0) if len(r.atom('N')) == 1 and len(r.atom('CA')) == 1 and len(r.atom('C')) == 1]
    # a ligand in which only ONE residue keeps its CA: one graph node cannot be matched to anything
    crippled = [r if i == keep0[0] or i not in keep0 else
                FZ.Residue(r.chain, r.number, r.resname, ['CX' if a == 'CA' else a for a in r.atom_names], r.elements, r.coords)
                for i, r in enumerate(lig0)]
    res = DK.surface_feature_analysis(pairs + [(crippled, rec0)], dev)
    assert len(res) == len(pairs) + 1
    for (lig, rec), r in zip(pairs, res):
        want = residue_means_by_hand(lig, rec)
        for side, (tag, rs) in enumerate((('ligand', lig), ('receptor', rec))):
            keep = [i for i, q in enumerate(rs) if len(q.atom('N')) == 1 and len(q.atom('CA')) == 1 and len(q.atom('C')) == 1]
            d, f = r[f'depth_{tag}'], r[f'feature_{tag}']
            assert d.dtype == np.float64 and f.dtype == np.float64 and len(d) == len(f) == r[f'n_{tag}'] == len(keep) > 2
            assert np.abs(d - np.float64([want[(side, i)] for i in keep])).max() <= BOUND
            g = DK.protein_graphs_batch([([rs[i] for i in keep], FZ.alpha_carbon_array([rs[i] for i in keep]))], 30.0, 10, dev)[0]
            assert np.array_equal(f, -g['host']['mu_r_norm'][:, 4].astype(np.float64))
            rho = r[f'spearman_{tag}']
            assert isinstance(rho, float) and rho == DK.spearman(d, f) and abs(rho - spearman_by_hand(d, f)) <= 1e-14
            assert -1.0 <= rho <= 1.0
    bad = res[-1]
    assert np.isnan(bad['spearman_ligand']) and bad['n_ligand'] == 0 and len(bad['depth_ligand']) == 0
    # the crippled ligand's atoms are the first ligand's: the receptor's depths alone do not notice
    assert bad['depth_receptor'].tobytes() == res[0]['depth_receptor'].tobytes() and bad['spearman_receptor'] == res[0]['spearman_receptor']
    return res


def check_surface_analysis_command_line(dev, tmp_path, capsys, names=('graph_case', 'graph_case_tiny')):
    """python -m equidock_public_amd.surface_analysis on a directory written with dock_common.write_pdb: one SPEARMAN line
    per ligand file with surface_feature_analysis's number, then the median; an empty directory gives exit 1"""
    from equidock_public_amd import surface_analysis as SA
    d = tmp_path / 'complexes'
    d.mkdir()
    tags = [f'CX{k}A' for k in range(len(names))]
    for nm, fx in zip(tags, names):
        lig, rec = dc.fixture_residues(fx)
        dc.write_pdb(lig, d / f'{nm}_l_b_COMPLEX.pdb')
        dc.write_pdb(rec, d / f'{nm}_r_b_COMPLEX.pdb')
    pairs = [(str(d / f'{nm}_l_b_COMPLEX.pdb'), str(d / f'{nm}_r_b_COMPLEX.pdb')) for nm in tags]
    want = DK.surface_feature_analysis(pairs, dev)
    capsys.readouterr()
    assert SA.main(['--dir', str(d), '--device', str(dev)]) == 0, capsys.readouterr().err
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == len(tags) + 1
    for ln, (lig, _), r in zip(lines, pairs, want):
        assert ln == f"SPEARMAN for file {lig} = {r['spearman_ligand']:.6f} ({r['n_ligand']} residues)", ln
    med = float(np.median([r['spearman_ligand'] for r in want]))
    assert lines[-1] == f"SPEARMAN median: {med:.6f} ({len(tags)} of {len(tags)} files)", lines[-1]
    empty = tmp_path / 'empty'
    empty.mkdir()
    assert SA.main(['--dir', str(empty), '--device', str(dev)]) == 1
    assert 'no *_l_b_COMPLEX.pdb' in capsys.readouterr().err


# ---- dock_complexes and the command line ------------------------------------------------------------------------------
DEPTH_FIELDS = {'depth_gain_ligand', 'depth_gain_receptor', 'deepened_atoms_ligand', 'deepened_atoms_receptor',
                'deepened_residues_ligand', 'deepened_residues_receptor'}


def check_dock_complexes_depth(dev, names, max_it, check_every):
    """dock_complexes(depth=True), with and without ground truth: its fields equal a direct residue_depth_batch on the
    returned ligand_atoms; depth=False returns what the call returns without the argument"""
    net, _, _ = dc.seeded_net(dev)
    residues = [dc.fixture_residues(n) for n in names]
    truths = [lig for lig, _ in residues]
    kw = dict(remove_clashes=True, max_it=max_it, check_every=check_every, device=dev)
    plain = DK.dock_complexes(net, residues, **kw)
    off = DK.dock_complexes(net, residues, depth=False, **kw)
    res = DK.dock_complexes(net, residues, depth=True, **kw)
    with_gt = DK.dock_complexes(net, residues, depth=True, ground_truth=truths, **kw)
    plain_gt = DK.dock_complexes(net, residues, ground_truth=truths, **kw)
    tabs = [(DK.atom_table(lig), DK.atom_table(rec), DK.atom_radii(lig), DK.atom_radii(rec)) for lig, rec in residues]
    want = DK.residue_depth_batch([r['ligand_atoms'][_t(t[0][1], dev)] for r, t in zip(res, tabs)],
                                  [_t(t[1][0], dev) for t in tabs], [t[2] for t in tabs], [t[3] for t in tabs],
                                  [t[0][2] for t in tabs], [t[1][2] for t in tabs])['rows'].cpu().numpy()
    for i in range(len(residues)):
        q, o, r, g = plain[i], off[i], res[i], with_gt[i]
        assert set(o) == set(q) and set(o['batch_seconds']) == set(q['batch_seconds'])
        assert not (DEPTH_FIELDS & set(q)) and set(r) - set(q) == DEPTH_FIELDS, set(r) ^ set(q)
        assert set(g) - set(plain_gt[i]) == DEPTH_FIELDS, set(g) ^ set(plain_gt[i])
        assert set(r['batch_seconds']) - set(q['batch_seconds']) == {'depth'}
        for a in (o, r, g):
            assert a['rotation'].tobytes() == q['rotation'].tobytes() and torch.equal(a['ligand_atoms'], q['ligand_atoms'])
            assert a['clash_iterations'] == q['clash_iterations']
        for a in (r, g):
            got = np.float64([a['depth_gain_ligand'], a['depth_gain_receptor'], a['deepened_atoms_ligand'],
                              a['deepened_atoms_receptor'], a['deepened_residues_ligand'], a['deepened_residues_receptor']])
            assert got.tobytes() == want[i, 6:12].tobytes(), (names[i], got, want[i])
            assert isinstance(a['depth_gain_ligand'], float) and isinstance(a['deepened_atoms_ligand'], int)
        assert np.float64(g['crmsd']).tobytes() == np.float64(plain_gt[i]['crmsd']).tobytes()
    return res


def check_command_line(dev, tmp_path, capsys, names, max_it=5):
    """the command line's --depth on a directory written with dock_common.write_pdb (no ground-truth ligands): every
    complex's line ends with its depth gains and deepened residues - those of dock_complexes(depth=True) on the same files
    to the printed digits -, then the summary of the ligand's gain; without the flag no line mentions the depth"""
    import re
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
    complexes = [(str(inp / f'{nm}_l_b.pdb'), str(gt / f'{nm}_r_b_COMPLEX.pdb')) for nm in tags]
    base = ['--checkpoint', str(ckpt), '--input-dir', str(inp), '--gt-dir', str(gt), '--remove-clashes', '--max-it',
            str(max_it), '--device', str(dev)]

    def cli(out, *flags):
        capsys.readouterr()
        assert DK.main(base + ['--out-dir', str(tmp_path / out)] + list(flags)) == 0, capsys.readouterr().err
        return capsys.readouterr().out.strip().splitlines()

    plain = cli('out0')
    assert not any('depth gain' in ln or 'deepened' in ln for ln in plain)
    want = DK.dock_complexes(net, complexes, remove_clashes=True, max_it=max_it, device=dev, depth=True)
    lines = cli('out1', '--depth')
    pat = re.compile(r'^(\w+): .*  depth gain (-?[\d.]+) / (-?[\d.]+)  deepened residues (\d+) / (\d+)$')
    for ln, nm, r in zip(lines, tags, want):
        m = pat.match(ln)
        assert m and m.group(1) == nm, ln
        assert (m.group(2), m.group(3)) == (f"{r['depth_gain_ligand']:.3f}", f"{r['depth_gain_receptor']:.3f}"), (ln, r)
        assert (int(m.group(4)), int(m.group(5))) == (r['deepened_residues_ligand'], r['deepened_residues_receptor'])
    gain = np.float64([r['depth_gain_ligand'] for r in want])
    assert lines[-1] == "depth gain median/mean/std: %.3f / %.3f / %.3f" % (np.median(gain), np.mean(gain), np.std(gain))
    assert len(lines) == len(plain) + 1
