"""Checks of the batched solvent-accessible surface (equidock_public_amd.dock.surface_area_batch / SurfacePlan /
sphere_points / atom_radii, eqd_dock_sasa_* of libequidock_dock.so) shared by the simulator tests
(tests/test_dock_surface_sim.py) and the GPU tests (tests/test_dock_surface_gpu.py).

Yardstick: `ref64`, a float64 numpy evaluation of the definitions of include/equidock_dock.h written without the kernels'
decomposition (no tiles, no lists, no staging): the dense fp64 centre-distance matrix of a complex, candidate partners
d_ij < R_i + R_j + 0.5, then per atom the exact point test with the header's expressions.  Every integer (both point
counts of every atom, columns 6-11) must equal it exactly; areas (per residue, columns 0-5) within BOUND = 1e-6 square
Angstrom absolute: sums of at most 2e4 non-negative fp64 terms totalling at most 2e4 A^2 differ between summation orders
by at most n * eps * total ~ 2e4 * 1.1e-16 * 2e4 ~ 4e-8 A^2, and the bound is about 20 times that.  Every case asserts
from the yardstick that no point test lies within 1e-9 A of its sphere (`margin`) and that no skip decision
(d_ij >= R_i + R_j + 1e-6) lies within 1e-9 A of its threshold (`skip_margin`).

Measured worst area error over all cases of this file (the tests print it):
    kernels on the x86 simulator    8.367e-11
    kernels on the MI355X           8.367e-11
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from equidock_public_amd import _lib, dock as DK
from tests import dock_common as dc

BOUND = 1e-6
PROBE, POINTS = 1.4, 96
OFFSET = np.array([83.0, 72.0, 243.0])         # a PDB-like frame
RADII = np.float32([1.70, 1.55, 1.52, 1.80])
# the kernels as built (csrc_dock/eqd_dock_sasa.hip): atoms per lists item, residues per chunk of the lists kernel, list
# entries per atom, partners per staged segment, rows per step of the finish kernel, atoms per workgroup of the point kernel
TILE, CHUNK, CAP, SEG, ROWS, WAVES = 64, 256, 96, 64, 256, 4


# ---- the float64 yardstick ------------------------------------------------------------------------------------------
def ref64(lig, rec, lrad, rrad, lo, ro, probe=PROBE, n_points=POINTS):
    """points [n][2] (ligand rows first), residue areas, the 12 columns by name, `margin`, `skip_margin`, `kept` (partners
    per atom under the skip rule) and `pairs`"""
    x = np.concatenate((np.asarray(lig, dtype=np.float64), np.asarray(rec, dtype=np.float64)))
    R = np.concatenate((np.asarray(lrad, dtype=np.float32), np.asarray(rrad, dtype=np.float32))).astype(np.float64) + probe
    nl, n = len(lig), len(x)
    side = np.arange(n) >= nl
    u = DK.sphere_points(n_points)
    D = np.empty((n, n))
    for i0 in range(0, n, 512):
        d = x[i0:i0 + 512, None, :] - x[None, :, :]
        D[i0:i0 + 512] = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    reach = R[:, None] + R[None, :]
    off_diag = ~np.eye(n, dtype=bool)
    skip_margin = float(np.abs(D - (reach + 1e-6))[off_diag].min()) if n > 1 else np.inf
    kept = ((D < reach + 1e-6) & off_diag).sum(1)
    cand = (D < reach + 0.5) & off_diag
    pts = np.zeros((n, 2), dtype=np.int64)
    margin = np.inf
    for i in range(n):
        j = np.nonzero(cand[i])[0]
        if len(j) == 0:
            pts[i] = n_points
            continue
        q = x[i] + R[i] * u                                     # [P][3]
        d = q[:, None, :] - x[j][None, :, :]
        s = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        margin = min(margin, float(np.abs(np.sqrt(s) - R[j][None, :]).min()))
        hit = s < (R[j] * R[j])[None, :]
        same = side[j] == side[i]
        pts[i, 0] = n_points - int(hit[:, same].any(1).sum())
        pts[i, 1] = n_points - int(hit.any(1).sum())
    w = 4 * np.pi * R * R / n_points
    a_alone, a_cplx, a_bur = w * pts[:, 0], w * pts[:, 1], w * (pts[:, 0] - pts[:, 1])
    lo, ro = np.asarray(lo, dtype=np.int64), np.asarray(ro, dtype=np.int64)
    first = np.concatenate((lo[:-1], ro[:-1] + nl))
    res_area = np.stack((np.add.reduceat(a_alone, first), np.add.reduceat(a_cplx, first)), axis=1)
    bur_atom = pts[:, 0] > pts[:, 1]
    bur_res = np.add.reduceat(bur_atom.astype(np.int64), first) > 0
    nrl = len(lo) - 1
    out = {'points': pts, 'res_area': res_area, 'margin': margin, 'skip_margin': skip_margin, 'kept': kept,
           'pairs': n * (n - 1),
           'sasa_ligand': float(a_alone[:nl].sum()), 'sasa_receptor': float(a_alone[nl:].sum()),
           'sasa_complex': float(a_cplx.sum()), 'bsa': float(a_bur.sum()), 'bsa_ligand': float(a_bur[:nl].sum()),
           'bsa_receptor': float(a_bur[nl:].sum()), 'buried_atoms_ligand': int(bur_atom[:nl].sum()),
           'buried_atoms_receptor': int(bur_atom[nl:].sum()), 'buried_residues_ligand': int(bur_res[:nrl].sum()),
           'buried_residues_receptor': int(bur_res[nrl:].sum()), 'points_alone': int(pts[:, 0].sum()),
           'points_complex': int(pts[:, 1].sum())}
    return out


_worst = {}


def check_complex(name, got, ref, key):
    """one complex of a batch (see `run`) against the yardstick; returns its worst area error"""
    assert ref['margin'] > 1e-9, (name, ref['margin'])
    assert ref['skip_margin'] > 1e-9, (name, ref['skip_margin'])
    assert got['points'].dtype == np.int32 and got['points'].shape == ref['points'].shape
    bad = np.nonzero((got['points'] != ref['points']).any(1))[0]
    assert len(bad) == 0, (name, 'point counts differ at rows', bad[:8], got['points'][bad[:8]], ref['points'][bad[:8]])
    row = got['row']
    for k, col in enumerate(DK.SURFACE_KEYS[6:], start=6):
        assert row[k] == ref[col], (name, col, row[k], ref[col])
    err = float(np.abs(got['res_area'] - ref['res_area']).max())
    for k, col in enumerate(DK.SURFACE_KEYS[:6]):
        err = max(err, abs(row[k] - ref[col]))
    assert err <= BOUND, f"{name}: worst area error {err:.3e} > {BOUND:g}"
    _worst[key] = max(_worst.get(key, 0.0), err)
    return err


def report(dev):
    key = torch.device(dev).type
    print(f"dock surface [{key}]: kernels' worst area error so far {_worst.get(key, 0.0):.3e} A^2 (bound {BOUND:g})")


# ---- running --------------------------------------------------------------------------------------------------------
def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run(dev, cases, n_points=POINTS, probe=PROBE, full=False):
    """one surface_area_batch over `cases` [(lig, rec, lig radii, rec radii, lig residue offsets, rec residue offsets)] ->
    per complex {'row' [12], 'points' [n][2] (ligand rows first), 'res_area' [r][2]} on the host"""
    cases = list(cases)
    out = DK.surface_area_batch([_t(c[0], dev) for c in cases], [_t(c[1], dev) for c in cases], [c[2] for c in cases],
                                [c[3] for c in cases], [c[4] for c in cases], [c[5] for c in cases], probe=probe,
                                n_points=n_points)
    kind = torch.device(dev).type
    for k in DK.SURFACE_KEYS:
        assert out[k].dtype == torch.float64 and out[k].shape == (len(cases),) and out[k].device.type == kind
    assert out['rows'].shape == (len(cases), DK.SASA_COLS) and out['lig_points'].dtype == torch.int32
    if full:
        return out
    rows = out['rows'].cpu().numpy()
    lp, rp = out['lig_points'].cpu().numpy(), out['rec_points'].cpu().numpy()
    la, ra = out['lig_res_area'].cpu().numpy(), out['rec_res_area'].cpu().numpy()
    res, a = [], [0, 0, 0, 0]
    for c, case in enumerate(cases):
        b = [a[0] + len(case[0]), a[1] + len(case[1]), a[2] + len(case[4]) - 1, a[3] + len(case[5]) - 1]
        res.append({'row': rows[c], 'points': np.concatenate((lp[a[0]:b[0]], rp[a[1]:b[1]])),
                    'res_area': np.concatenate((la[a[2]:b[2]], ra[a[3]:b[3]]))})
        a = b
    assert a == [len(lp), len(rp), len(la), len(ra)]
    return res


def same_bits(a, b, what):
    for k in ('row', 'points', 'res_area'):
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


# ---- cases ------------------------------------------------------------------------------------------------------------
def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def radii_by_name(names):
    """C 1.70, N 1.55, O 1.52, S 1.80, anything else 1.80 by the first letter of the atom name"""
    return np.float32([DK.ATOM_RADII.get(str(nm).lstrip('0123456789')[:1].upper(), DK.DEFAULT_RADIUS) for nm in names])


@functools.lru_cache(maxsize=None)
def fixture_cases():
    """1AVX and 1HCF of tests/golden/dockq_case.npz: the native pose and the lig_equidock pose"""
    z = np.load(os.path.join(dc.GOLDEN, 'dockq_case.npz'))
    out = {}
    for nm in ('1AVX', '1HCF'):
        lrad, rrad = radii_by_name(z[f'{nm}_lig_true_names']), radii_by_name(z[f'{nm}_rec_true_names'])
        lo, ro = z[f'{nm}_lig_true_res_off'], z[f'{nm}_rec_true_res_off']
        assert (z[f'{nm}_lig_equidock_names'] == z[f'{nm}_lig_true_names']).all()
        for tag, key in (('native', 'lig_true'), ('EQUIDOCK', 'lig_equidock')):
            out[f'{nm}_{tag}'] = (z[f'{nm}_{key}_atoms'], z[f'{nm}_rec_true_atoms'], lrad, rrad, lo, ro)
    return out


def _sizes(rng, n_atoms, big=None):
    """residue sizes of 4-14 atoms that add up to n_atoms (the last one takes what is left; n_atoms < 0: -n_atoms residues
    of 4-14 atoms); `big`: the first residue's"""
    if n_atoms < 0:
        return rng.integers(4, 15, -n_atoms).astype(np.int64)
    sizes = [] if big is None else [big]
    left = n_atoms - sum(sizes)
    while left > 0:
        k = min(int(rng.integers(4, 15)), left)
        sizes.append(k)
        left -= k
    return np.asarray(sizes, dtype=np.int64)


def _globule(rng, n_atoms, centre, big=None):
    """a seeded globule at protein density: residue centres uniform in a ball of 140 A^3 per residue, the atoms of a
    residue within ~1.5 A of its centre, radii drawn from the four table values"""
    sizes = _sizes(rng, n_atoms, big)
    n_atoms = int(sizes.sum())
    rad = (3.0 * 140.0 * len(sizes) / (4.0 * np.pi)) ** (1.0 / 3.0)
    v = rng.standard_normal((len(sizes), 3))
    cen = v / np.linalg.norm(v, axis=1, keepdims=True) * rad * rng.uniform(0.0, 1.0, (len(sizes), 1)) ** (1.0 / 3.0)
    x = np.repeat(cen, sizes, axis=0) + rng.standard_normal((n_atoms, 3)) * 0.9 + centre
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return _f32(x), rng.choice(RADII, n_atoms).astype(np.float32), off, rad


def globules(n_lig, n_rec, seed, big=None, gap=0.8, n_points=POINTS):
    """two touching globules of n_lig and n_rec atoms (a negative number: that many residues) at the PDB-like offset, reseeded until the yardstick's conditions on
    the inputs hold; `big` (side, atoms): the first residue of that side has that many atoms"""
    while True:
        rng = np.random.default_rng(seed)
        lx, lr, lo, ball_l = _globule(rng, n_lig, OFFSET, big[1] if big and big[0] == 0 else None)
        ball_r = (3.0 * 140.0 * max(n_rec / 9.0 if n_rec > 0 else -n_rec, 1.0) / (4.0 * np.pi)) ** (1.0 / 3.0)      # (about 9 atoms per residue)
        rx, rr, ro, _ = _globule(rng, n_rec, OFFSET + np.array([(ball_l + ball_r) * gap, 0.0, 0.0]),
                                 big[1] if big and big[0] == 1 else None)
        case = (lx, rx, lr, rr, lo, ro)
        r = ref64(*case, n_points=n_points)
        if r['margin'] > 1e-9 and r['skip_margin'] > 1e-9:
            return case
        seed += 1000


# atoms per side either side of the point kernel's workgroup (4 atoms), of the atom tile / staged segment (64) and of
# the finish step (256), residues either side of the lists kernel's chunk (256), a side of ONE atom, a residue of more than 64 atoms
EDGES = {'edge_3x5': (3, 5, 401, None), 'edge_4x4': (4, 4, 402, None), 'edge_5x3': (5, 3, 403, None),
         'edge_63x255': (63, 255, 404, None), 'edge_64x256': (64, 256, 405, None), 'edge_65x257': (65, 257, 406, None),
         'edge_255x63': (255, 63, 407, None), 'edge_256x64': (256, 64, 408, None), 'edge_257x65': (257, 65, 409, None),
         'edge_1x70': (1, 70, 410, None), 'edge_70x1': (70, 1, 411, None), 'edge_1x1': (1, 1, 412, None),
         'edge_long_residue': (90, 40, 413, (0, 70)),
         # residues of both sides together either side of the lists kernel's chunk
         'edge_res_255': (-100, -155, 414, None), 'edge_res_256': (-100, -156, 415, None), 'edge_res_257': (-100, -157, 416, None)}
P_EDGES = (1, 63, 64, 65, 96, 130)


@functools.lru_cache(maxsize=None)
def edge_cases():
    out = {k: globules(nl, nr, seed, big) for k, (nl, nr, seed, big) in EDGES.items()}
    # the two single atoms of edge_1x1 overlap: 2 A apart
    lx, rx, lr, rr, lo, ro = out['edge_1x1']
    out['edge_1x1'] = (lx, _f32(lx + np.float32([2.0, 0.25, -0.5])), lr, rr, lo, ro)
    return out


@functools.lru_cache(maxsize=None)
def p_case(n_points):
    return globules(37, 70, 500 + n_points, n_points=n_points)


@functools.lru_cache(maxsize=None)
def degenerate_cases():
    out = {}
    lx, rx, lr, rr, lo, ro = globules(70, 90, 601)
    out['far_ligand'] = (_f32(lx - np.float32([200.0, 0.0, 0.0])), rx, lr, rr, lo, ro)
    # ligand row 0 enclosed by a shell of 40 ligand atoms 1.5 A away (each buries almost a hemisphere of its points)
    seed = 602
    while True:
        rng = np.random.default_rng(seed)
        shell = DK.sphere_points(40) * 1.5 + rng.standard_normal((40, 3)) * 0.05
        ex = _f32(np.concatenate((np.zeros((1, 3)), shell)) + OFFSET)
        er = np.concatenate((np.float32([1.52]), rng.choice(RADII, 40).astype(np.float32)))
        gx, gr, go, _ = _globule(rng, 30, OFFSET + np.array([7.0, 0.0, 0.0]))
        case = (ex, gx, er, gr, np.int32([0, 1, 41]), go)
        r = ref64(*case)
        if r['margin'] > 1e-9 and r['skip_margin'] > 1e-9:
            break
        seed += 1000
    out['enclosed_atom'] = case
    # 400 atoms jittered inside a 3 A ball: every atom has 399 partners, no list holds them
    seed = 603
    while True:
        rng = np.random.default_rng(seed)
        v = rng.standard_normal((400, 3))
        bx = _f32(v / np.linalg.norm(v, axis=1, keepdims=True) * 3.0 * rng.uniform(0.0, 1.0, (400, 1)) ** (1.0 / 3.0) + OFFSET)
        br = rng.choice(RADII, 400).astype(np.float32)
        case = (bx[:250], bx[250:], br[:250], br[250:], np.int32([0, 100, 250]), np.int32([0, 1, 80, 150]))
        r = ref64(*case)
        if r['margin'] > 1e-9 and r['skip_margin'] > 1e-9:
            break
        seed += 1000
    out['dense_ball'] = case
    return out


def all_cases():
    return {**fixture_cases(), **edge_cases(), **degenerate_cases()}


_refs = {}


def reference(name, case, n_points=POINTS):
    if (name, n_points) not in _refs:
        _refs[(name, n_points)] = ref64(*case, n_points=n_points)
    return _refs[(name, n_points)]


_measured = {}


def measured(dev):
    """ALL cases of this file (P = 96) in ONE batch - computed once per device type and shared by the tests"""
    key = torch.device(dev).type
    if key not in _measured:
        cases = all_cases()
        names = list(cases)
        _measured[key] = dict(zip(names, run(dev, [cases[n] for n in names])))
    return _measured[key]


def check_names(dev, names):
    got, cases, key = measured(dev), all_cases(), torch.device(dev).type
    for n in names:
        check_complex(n, got[n], reference(n, cases[n]), key)
    report(dev)
    return {n: got[n] for n in names}


# ---- the checks -------------------------------------------------------------------------------------------------------
# the table of the issue (float64 evaluation recorded there): ligand atoms, receptor atoms, SASA ligand, SASA receptor,
# SASA complex, BSA (square Angstrom), margin (Angstrom)
TABLE = {'1AVX_native': (1286, 1630, 8773.2, 9353.3, 16569.8, 1556.6, 3.3e-7),
         '1HCF_native': (809, 1802, 5997.7, 13823.2, 17717.7, 2103.2, 3.8e-7)}


def check_yardstick_reproduces_the_table():
    """2. CPU: ref64 on the fixture natives gives the issue's table to 0.1 A^2"""
    f = fixture_cases()
    for name, t in TABLE.items():
        r = reference(name, f[name])
        assert (len(f[name][0]), len(f[name][1])) == t[:2]
        got = (r['sasa_ligand'], r['sasa_receptor'], r['sasa_complex'], r['bsa'])
        assert np.abs(np.array(got) - np.array(t[2:6])).max() <= 0.1, (name, got, t)
        assert 0.5 * t[6] < r['margin'] < 2.0 * t[6], (name, r['margin'], t[6])
        assert abs(r['bsa'] - (r['sasa_ligand'] + r['sasa_receptor'] - r['sasa_complex'])) < 1e-6


def check_sphere_and_radii(tmp_path):
    """sphere_points is the golden-section spiral of unit vectors; atom_radii follows atom_table's rows"""
    for n in (1, 2, 96, 1024):
        u = DK.sphere_points(n)
        assert u.dtype == np.float64 and u.shape == (n, 3) and np.abs(np.linalg.norm(u, axis=1) - 1.0).max() < 1e-15
        k = np.arange(n)
        assert np.array_equal(u[:, 2], 1.0 - (2.0 * k + 1.0) / n)
        phi = k * np.pi * (3.0 - np.sqrt(5.0))
        assert np.abs(u[:, 0] - np.sqrt(1 - u[:, 2] ** 2) * np.cos(phi)).max() < 1e-12
    for n in (0, 1025):
        with pytest.raises(ValueError, match='sphere_points'):
            DK.sphere_points(n)
    lines = ["ATOM      1  N   GLY B   2       1.000   2.000   3.000  1.00  0.00           N",
             "ATOM      2  H   GLY B   2       1.500   2.000   3.000  1.00  0.00           H",
             "ATOM      3  CA  GLY B   2       2.000   2.000   3.000  1.00  0.00           C",
             "ATOM      4  SG  CYS B   3       3.000   2.000   3.000  1.00  0.00",
             "ATOM      5 1HB  CYS B   3       3.500   2.000   3.000  1.00  0.00",
             "ATOM      6 2OXT CYS B   3       4.000   2.000   3.000  1.00  0.00",
             "ATOM      7  CA  ION A   1       5.000   2.000   3.000  1.00  0.00          CA",
             "ATOM      8  O   SER A   1       5.000   2.000   3.000  1.00  0.00           O"]
    path = tmp_path / 'x.pdb'
    path.write_text('\n'.join(lines) + '\nEND\n')
    r = DK.atom_radii(str(path))
    assert r.dtype == np.float32 and len(r) == len(DK.atom_table(str(path))[0])
    assert r.tolist() == np.float32([1.55, 1.70, 1.80, 1.52, 1.80, 1.52]).tolist()
    lig, _ = dc.fixture_residues('graph_case_tiny')
    assert len(DK.atom_radii(lig)) == len(DK.atom_table(lig)[0])


def check_real(dev):
    """3. 1AVX and 1HCF, native and lig_equidock poses, in ONE batch"""
    got = check_names(dev, list(fixture_cases()))
    for nm in ('1AVX', '1HCF'):
        assert got[f'{nm}_native']['row'][3] > 1000.0 and got[f'{nm}_native']['row'][8] > 10


def check_edges(dev):
    """4. tile, chunk, segment and workgroup edges, a side of one atom, a long residue; P either side of the wave"""
    cases = edge_cases()
    check_names(dev, list(cases))
    per_side = {len(c[k]) for c in cases.values() for k in (0, 1)}
    for size in (WAVES, TILE, ROWS):
        assert {size - 1, size, size + 1} <= per_side, (size, per_side)
    assert SEG == TILE and 1 in per_side
    assert {CHUNK - 1, CHUNK, CHUNK + 1} <= {len(c[4]) + len(c[5]) - 2 for c in cases.values()}
    assert np.diff(cases['edge_long_residue'][4]).max() > 64
    for n, c in cases.items():
        r = reference(n, c)
        assert (r['kept'] <= CAP).mean() > 0.9 and (len(c[0]) + len(c[1]) < 60 or r['bsa'] > 0.0), (n, r['kept'].max(), r['bsa'])
    assert any(reference(n, c)['kept'].sum() < reference(n, c)['pairs'] for n, c in cases.items())      # partners are skipped
    key = torch.device(dev).type
    for P in P_EDGES:
        case = p_case(P)
        check_complex(f'P={P}', run(dev, [case], n_points=P)[0], reference(f'P={P}', case, P), key)
    report(dev)


def check_degenerate(dev):
    """5. degenerate sets"""
    cases = degenerate_cases()
    got = check_names(dev, list(cases))
    g = got['far_ligand']
    assert g['row'][3] == 0.0 and g['row'][4] == 0.0 and g['row'][5] == 0.0 and (g['row'][6:10] == 0).all()
    assert (g['points'][:, 0] == g['points'][:, 1]).all() and g['row'][10] == g['row'][11] > 0
    assert np.array_equal(g['res_area'][:, 0], g['res_area'][:, 1])
    assert got['enclosed_atom']['points'][0].tolist() == [0, 0]
    r = reference('dense_ball', cases['dense_ball'])
    assert r['kept'].min() > CAP            # every list cap is exceeded: the all-partners path
    assert got['dense_ball']['row'][11] > 0


def check_all_partners_switch(dev, monkeypatch):
    """6. EQD_DOCK_SASA_ALL_PARTNERS=1 against the default on the real batch: every output is bit-equal"""
    cases = fixture_cases()
    names = list(cases)
    default = measured(dev)
    assert not DK.surface_all_partners()
    monkeypatch.setenv('EQD_DOCK_SASA_ALL_PARTNERS', '1')
    assert DK.surface_all_partners()
    forced = run(dev, [cases[n] for n in names])
    monkeypatch.undo()
    assert not DK.surface_all_partners()
    for n, g in zip(names, forced):
        same_bits(default[n], g, f'{n}: all partners vs lists')


def check_bits(dev):
    """7. each complex of the real batch alone, first, last, in a permuted batch and twice in a row: the same bits"""
    cases = fixture_cases()
    names = list(cases)
    cs = [cases[n] for n in names]
    k = len(cs)
    assert k == 4
    together, again = run(dev, cs), run(dev, cs)
    perm = [2, 0, 3, 1]
    permuted = run(dev, [cs[p] for p in perm])
    for i, n in enumerate(names):
        same_bits(together[i], again[i], f'{n}: run to run')
        same_bits(together[i], permuted[perm.index(i)], f'{n}: permuted')
        same_bits(together[i], run(dev, [cs[i]])[0], f'{n}: alone')
        same_bits(together[i], measured(dev)[n], f'{n}: in the batch of all cases')
    for s in range(1, k):                                       # the batch rotated: every complex comes first and last
        order = [(s + j) % k for j in range(k)]
        rot = run(dev, [cs[j] for j in order])
        same_bits(together[order[0]], rot[0], f'{names[order[0]]}: first')
        same_bits(together[order[-1]], rot[-1], f'{names[order[-1]]}: last')
        for j, o in enumerate(order):
            same_bits(together[o], rot[j], f'{names[o]}: rotated batch')


def check_validation_errors(dev):
    """1. refused before any launch, with a message (the entry points and surface_area_batch)"""
    lib = DK.load_dock_library()
    assert lib.eqd_dock_sasa_abi() == DK.DOCK_SASA_ABI == 1 and DK.SASA_COLS == 12 and lib.eqd_dock_abi_version() == 1
    lig, rec = torch.zeros(4, 3, device=dev), torch.ones(5, 3, device=dev)
    lo, ro = np.int32([0, 2, 4]), np.int32([0, 1, 5])
    lr, rr = np.float32([1.7, 1.55, 1.52, 1.8]), np.full(5, 1.7, np.float32)
    good = dict(lig_radii=[lr], rec_radii=[rr], lig_res_offsets=[lo], rec_res_offsets=[ro])
    assert DK.surface_area_batch([lig], [rec], **good)['rows'].shape == (1, 12)
    with pytest.raises(ValueError, match='ligands for'):
        DK.surface_area_batch([lig, lig], [rec], **good)
    with pytest.raises(ValueError, match='are needed'):
        DK.surface_area_batch([lig], [rec])
    with pytest.raises(ValueError, match='complex 0: ligand: residue offsets'):
        DK.surface_area_batch([lig], [rec], **dict(good, lig_res_offsets=[np.int32([0, 2, 3])]))
    with pytest.raises(ValueError, match='rows for tables of'):
        DK.surface_area_batch([lig[:3]], [rec], **good)
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='complex 0: ligand: radii must be finite and > 0'):
            DK.surface_area_batch([lig], [rec], **dict(good, lig_radii=[np.float32([1.7, bad, 1.5, 1.8])]))
        with pytest.raises(ValueError, match='complex 0: receptor: radii'):
            DK.surface_area_batch([lig], [rec], **dict(good, rec_radii=[np.float32([1.7, 1.7, 1.7, 1.7, bad])]))
    for bad in (0.0, float('nan'), float('inf')):
        with pytest.raises(_lib.EquidockHipError, match='probe'):
            DK.surface_area_batch([lig], [rec], probe=bad, **good)
    for bad in (0, 1025):
        with pytest.raises(ValueError, match='sphere_points'):
            DK.surface_area_batch([lig], [rec], n_points=bad, **good)

    def offs(v):
        return np.ascontiguousarray(np.asarray(v, dtype=np.int32))

    def p(a):
        return a.ctypes.data_as(C.c_void_p)

    la, ra, lro, rro = offs([0, 4, 8]), offs([0, 5, 10]), offs([0, 2, 4]), offs([0, 2, 4])
    wsb = lib.eqd_dock_sasa_workspace_bytes(2, p(la), p(ra), p(lro), p(rro), 96)
    assert wsb > 0
    bad = offs([0, 6, 4])
    assert lib.eqd_dock_sasa_workspace_bytes(2, p(bad), p(ra), p(lro), p(rro), 96) == 0
    assert b'complex 1 has -2 ligand' in lib.eqd_dock_last_error()
    assert lib.eqd_dock_sasa_workspace_bytes(2, p(offs([0, 4, 4])), p(ra), p(lro), p(rro), 96) == 0          # an empty side
    assert lib.eqd_dock_sasa_workspace_bytes(2, p(offs([1, 4, 8])), p(ra), p(lro), p(rro), 96) == 0
    assert lib.eqd_dock_sasa_workspace_bytes(2, p(la), p(ra), p(offs([0, 5, 7])), p(rro), 96) == 0          # 5 residues, 4 atoms
    assert b'tiles its complex' in lib.eqd_dock_last_error()
    for P in (0, 1025, -3):
        assert lib.eqd_dock_sasa_workspace_bytes(2, p(la), p(ra), p(lro), p(rro), P) == 0
        assert b'n_points' in lib.eqd_dock_last_error()
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    l2, r2 = torch.cat([lig, lig]), torch.cat([rec, rec])
    lrad, rrad = torch.full((8,), 1.7, device=dev), torch.full((10,), 1.7, device=dev)
    lf, rf = _t(np.int32([0, 2, 4, 6, 8]), dev), _t(np.int32([0, 2, 5, 7, 10]), dev)
    sphere = _t(DK.sphere_points(96), dev)
    pts = torch.full((18, 2), 7, dtype=torch.int32, device=dev)
    area = torch.full((8, 2), 7.0, dtype=torch.float64, device=dev)
    rows = torch.full((2, 12), 7.0, dtype=torch.float64, device=dev)
    st = DK._stream(dev)
    W = C.c_void_p(ws.data_ptr())
    assert lib.eqd_dock_sasa_init(2, p(bad), p(ra), p(lro), p(rro), 96, W, C.c_size_t(wsb), st) == 2
    assert lib.eqd_dock_sasa_init(2, p(la), p(ra), p(lro), p(rro), 0, W, C.c_size_t(wsb), st) == 2
    assert lib.eqd_dock_sasa_init(2, p(la), p(ra), p(lro), p(rro), 96, W, C.c_size_t(64), st) == 4
    assert b'workspace too small' in lib.eqd_dock_last_error()

    def ev(la_, size, P=96, probe=1.4, sph=sphere):
        return lib.eqd_dock_sasa_eval(2, p(la_), p(ra), p(lro), p(rro), C.c_void_p(l2.data_ptr()), C.c_void_p(r2.data_ptr()),
                                      C.c_void_p(lrad.data_ptr()), C.c_void_p(rrad.data_ptr()), C.c_void_p(lf.data_ptr()),
                                      C.c_void_p(rf.data_ptr()), C.c_void_p(sph.data_ptr()) if sph is not None else C.c_void_p(0),
                                      P, C.c_double(probe), 0, C.c_void_p(pts.data_ptr()), C.c_void_p(pts[8:].data_ptr()),
                                      C.c_void_p(area.data_ptr()), C.c_void_p(area[4:].data_ptr()),
                                      C.c_void_p(rows.data_ptr()), W, C.c_size_t(size), st)

    assert ev(bad, wsb) == 2
    assert ev(la, 64) == 4
    assert ev(la, wsb, sph=None) == 1
    for P in (0, 1025):
        assert ev(la, wsb, P=P) == 2 and b'n_points' in lib.eqd_dock_last_error()
    for v in (0.0, -1.0, float('inf'), float('nan')):
        assert ev(la, wsb, probe=v) == 2 and b'probe' in lib.eqd_dock_last_error()
    # nothing was written by the refused calls
    assert bool((pts.cpu() == 7).all()) and bool((area.cpu() == 7.0).all()) and bool((rows.cpu() == 7.0).all())
    assert bool((ws.cpu() == 0).all())


SURFACE_FIELDS = {'sasa_ligand', 'sasa_receptor', 'sasa_complex', 'bsa', 'buried_atoms_ligand', 'buried_atoms_receptor',
                  'buried_residues_ligand', 'buried_residues_receptor'}


def check_dock_complexes_surface(dev, names, max_it, check_every):
    """9. dock_complexes(surface=True) with and without ground_truth: its fields equal a direct surface_area_batch on the
    returned ligand_atoms; surface=False returns what the call returns without the argument"""
    net, _, _ = dc.seeded_net(dev)
    residues = [dc.fixture_residues(n) for n in names]
    truths = [lig for lig, _ in residues]
    kw = dict(remove_clashes=True, max_it=max_it, check_every=check_every, device=dev)
    plain = DK.dock_complexes(net, residues, **kw)
    off = DK.dock_complexes(net, residues, surface=False, **kw)
    res = DK.dock_complexes(net, residues, surface=True, **kw)
    with_gt = DK.dock_complexes(net, residues, surface=True, ground_truth=truths, **kw)
    plain_gt = DK.dock_complexes(net, residues, ground_truth=truths, **kw)
    tabs = [(DK.atom_table(lig), DK.atom_table(rec), DK.atom_radii(lig), DK.atom_radii(rec)) for lig, rec in residues]
    n = len(residues)
    ligs = [r['ligand_atoms'][_t(t[0][1], dev)] for r, t in zip(res, tabs)] + [_t(t[0][0], dev) for t in tabs]
    recs = [_t(t[1][0], dev) for t in tabs] * 2
    want = DK.surface_area_batch(ligs, recs, [t[2] for t in tabs] * 2, [t[3] for t in tabs] * 2, [t[0][2] for t in tabs] * 2,
                                 [t[1][2] for t in tabs] * 2)['rows'].cpu().numpy()
    for i in range(n):
        q, o, r, g = plain[i], off[i], res[i], with_gt[i]
        assert set(o) == set(q) and set(o['batch_seconds']) == set(q['batch_seconds'])
        assert set(r) - set(q) == SURFACE_FIELDS, set(r) ^ set(q)
        assert set(g) - set(plain_gt[i]) == SURFACE_FIELDS | {'bsa_native'}, set(g) ^ set(plain_gt[i])
        assert set(r['batch_seconds']) - set(q['batch_seconds']) == {'surface'}
        for a in (o, r, g):
            assert a['rotation'].tobytes() == q['rotation'].tobytes() and torch.equal(a['ligand_atoms'], q['ligand_atoms'])
            assert a['clash_iterations'] == q['clash_iterations']
        for a in (r, g):
            got = np.float64([a['sasa_ligand'], a['sasa_receptor'], a['sasa_complex'], a['bsa'], a['buried_atoms_ligand'],
                              a['buried_atoms_receptor'], a['buried_residues_ligand'], a['buried_residues_receptor']])
            assert got.tobytes() == want[i, [0, 1, 2, 3, 6, 7, 8, 9]].tobytes(), (names[i], got, want[i])
            assert isinstance(a['bsa'], float) and isinstance(a['buried_atoms_ligand'], int)
        assert np.float64(g['bsa_native']).tobytes() == want[n + i, 3].tobytes() and g['bsa_native'] > 0.0
        assert np.float64(g['crmsd']).tobytes() == np.float64(plain_gt[i]['crmsd']).tobytes()
    return res


def check_command_line(dev, tmp_path, capsys, names, max_it=5):
    """9. the command line's --surface on a directory written with dock_common.write_pdb: without ground-truth ligands it
    prints the BSA and the buried residues of every complex and the BSA summary; with them the native BSA as well; the
    numbers are those of dock_complexes(surface=True) on the same files to the printed digits; without the flag no line
    mentions the surface"""
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
    assert not any('BSA' in ln for ln in plain)
    want = DK.dock_complexes(net, complexes, remove_clashes=True, max_it=max_it, device=dev, surface=True)
    lines = cli('out1', '--surface')
    pat = re.compile(r'^(\w+): .*  BSA ([\d.]+)  buried residues (\d+) / (\d+)$')
    for ln, nm, r in zip(lines, tags, want):
        m = pat.match(ln)
        assert m and m.group(1) == nm and m.group(2) == f"{r['bsa']:.1f}", (ln, r['bsa'])
        assert (int(m.group(3)), int(m.group(4))) == (r['buried_residues_ligand'], r['buried_residues_receptor'])
    bsa = np.float64([r['bsa'] for r in want])
    assert lines[-1] == "BSA median/mean/std: %.1f / %.1f / %.1f" % (np.median(bsa), np.mean(bsa), np.std(bsa)), lines[-1]
    assert not any('native BSA' in ln for ln in lines) and len(lines) == len(plain) + 1
    # with the ground-truth ligands present: the native BSA per complex and its summary
    truths = []
    for nm, fx in zip(tags, names):
        dc.write_pdb(dc.fixture_residues(fx)[0], gt / f'{nm}_l_b_COMPLEX.pdb')
        truths.append(str(gt / f'{nm}_l_b_COMPLEX.pdb'))
    want = DK.dock_complexes(net, complexes, remove_clashes=True, max_it=max_it, device=dev, surface=True, ground_truth=truths)
    lines = cli('out2', '--surface')
    pat = re.compile(r'^(\w+): .*  BSA ([\d.]+)  buried residues (\d+) / (\d+)  native BSA ([\d.]+)$')
    for ln, nm, r in zip(lines, tags, want):
        m = pat.match(ln)
        assert m and m.group(2) == f"{r['bsa']:.1f}" and m.group(5) == f"{r['bsa_native']:.1f}", (ln, r)
    nat = np.float64([r['bsa_native'] for r in want])
    assert lines[-1] == "native BSA median/mean/std: %.1f / %.1f / %.1f" % (np.median(nat), np.mean(nat), np.std(nat))
    assert lines[-2].startswith('BSA median/mean/std: ') and (nat > 0).all()
