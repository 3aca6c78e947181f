"""Checks of the batched docking quality (equidock_public_amd.dock.pose_quality_batch / atom_table / QualityPlan,
eqd_dock_quality_* of libequidock_dock.so) shared by the simulator tests (tests/test_dock_quality_sim.py) and the GPU
tests (tests/test_dock_quality_gpu.py).

Yardstick: `ref64`, a float64 numpy evaluation of the definitions of include/equidock_dock.h - every atom pair by brute
force, np.linalg.svd - written without the kernels' decomposition (no tiles, no staging, no moments).  Integer columns
(5-11, 13) must equal it exactly; columns 0-4 within BOUND = 1e-10 (Angstrom, DockQ units): the same fp64 arithmetic in
the batched RMSD meter measures 8.5e-14 A at worst under a bound of 6.2e-7.  Every case asserts from the yardstick that
no atom pair lies within 1e-6 A of a cutoff in either pose, and that no pruning decision lies within 1e-9 A of its
threshold.

Measured worst error of columns 0-4 over all cases of this file (the tests print it):
    kernels on the x86 simulator    1.323e-13
    kernels on the MI355X           1.323e-13

tests/golden/dockq_case.npz was written once from the reference's shipped data files (PDB coordinates) by

    import numpy as np
    from equidock_public_amd import dock as DK
    T = 'test_sets_pdb/'
    out = {}
    for nm in ('1AVX', '1HCF'):
        for key, path in (('lig_true', f'db5_test_random_transformed/complexes/{nm}_l_b_COMPLEX.pdb'),
                          ('rec_true', f'db5_test_random_transformed/complexes/{nm}_r_b_COMPLEX.pdb'),
                          ('lig_equidock', f'db5_equidock_results/{nm}_l_b_EQUIDOCK.pdb'),
                          ('lig_no_clashes', f'db5_equidock_no_clashes_results/{nm}_l_b_EQUIDOCK_NO_CLASHES.pdb')):
            atoms, index, res_off, bb, names = DK.atom_table(T + path)
            out[f'{nm}_{key}_atoms'], out[f'{nm}_{key}_names'], out[f'{nm}_{key}_res_off'] = atoms, names.astype('U4'), res_off
    np.savez_compressed('tests/golden/dockq_case.npz', **out)
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from equidock_public_amd import _lib, dock as DK
from tests import dock_common as dc

BOUND = 1e-10
CUTS = (5.0, 10.0, 3.0)                        # contact, interface, clash
OFFSET = np.array([83.0, 72.0, 243.0])         # a PDB-like frame
BB = ('N', 'CA', 'C', 'O')
# the kernels as built (csrc_dock/eqd_dock_quality.hip)
TILE, CHUNK, STAGE, ROWS = 8, 32, 512, 256


# ---- the float64 yardstick ------------------------------------------------------------------------------------------
def _kabsch64(P, T):
    """(R, b, reflection branch taken, smallest / largest singular value) of the superposition of P onto T"""
    cp, ct = P.mean(0), T.mean(0)
    U, S, Vt = np.linalg.svd((P - cp).T @ (T - ct))
    R = Vt.T @ U.T
    reflect = bool(np.linalg.det(R) < 0)
    if reflect:
        R = (Vt.T @ np.diag([1.0, 1.0, -1.0])) @ U.T
    return R, ct - R @ cp, reflect, (float(S[2] / S[0]) if S[0] > 0 else 0.0)


def _rmsd(R, b, P, T):
    e = P @ R.T + b - T
    return float(np.sqrt(np.mean(np.sum(e * e, axis=1))))


def _dist(a, b):
    out = np.empty((len(a), len(b)))
    for i0 in range(0, len(a), 512):           # (blocks: the 10 044-atom ligand)
        d = a[i0:i0 + 512, None, :] - b[None, :, :]
        out[i0:i0 + 512] = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    return out


def _per_residue_pair(mask, lo, ro):
    """any over the atom pairs of every (ligand residue, receptor residue) block of a boolean [A_l][A_r] matrix"""
    rows = np.logical_or.reduceat(mask, lo[:-1], axis=0)
    return np.logical_or.reduceat(rows, ro[:-1], axis=1)


def _bounds(x, off):
    cen = np.stack([x[off[k]:off[k + 1]].sum(0) / (off[k + 1] - off[k]) for k in range(len(off) - 1)])
    d = x - np.repeat(cen, np.diff(off), axis=0)
    r = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return cen, np.maximum.reduceat(r, off[:-1])


def ref64(lp, rp, lt, rt, lo, ro, lbb, rbb, cuts=CUTS):
    """the 16 columns by name, plus `margin` (the closest any atom distance of either pose comes to a cutoff),
    `prune_margin`, `flags_mask` (the flag bits that are well determined) and `pairs` (residue pairs)"""
    lp, lt, rt = (np.asarray(a, dtype=np.float64) for a in (lp, lt, rt))
    rp = rt if rp is None else np.asarray(rp, dtype=np.float64)
    lo, ro = np.asarray(lo, dtype=np.int64), np.asarray(ro, dtype=np.int64)
    lbb, rbb = np.asarray(lbb) != 0, np.asarray(rbb) != 0
    cc, ic, kc = cuts
    dn, dm = _dist(lt, rt), _dist(lp, rp)
    cn, cm = _per_residue_pair(dn < cc, lo, ro), _per_residue_pair(dm < cc, lo, ro)
    N, M, S = int(cn.sum()), int(cm.sum()), int((cn & cm).sum())
    out = {'native_contacts': N, 'model_contacts': M, 'shared_contacts': S, 'clashes': int((dm < kc).sum()),
           'fnat': S / N if N else float('nan'), 'fnonnat': (M - S) / M if M else 0.0,
           'margin': float(min(np.abs(d - c).min() for d in (dn, dm) for c in cuts)), 'pairs': cn.size}
    near = _per_residue_pair(dn < ic, lo, ro)
    il, ir = near.any(1), near.any(0)
    out['interface_residues_ligand'], out['interface_residues_receptor'] = int(il.sum()), int(ir.sum())
    wl, wr = np.repeat(il, np.diff(lo)) & lbb, np.repeat(ir, np.diff(ro)) & rbb
    out['interface_backbone_rows'] = int(wl.sum() + wr.sum())
    fi = fr = False
    cond_i = cond_r = 0.0
    if out['interface_backbone_rows']:
        P, T = np.concatenate((lp[wl], rp[wr])), np.concatenate((lt[wl], rt[wr]))
        R, b, fi, cond_i = _kabsch64(P, T)
        out['irmsd_backbone'] = _rmsd(R, b, P, T)
    else:
        out['irmsd_backbone'] = float('nan')
    if lbb.any() and rbb.any():
        R, b, fr, cond_r = _kabsch64(rp[rbb], rt[rbb])
        out['lrmsd'] = _rmsd(R, b, lp[lbb], lt[lbb])
    else:
        out['lrmsd'] = float('nan')
    out['dockq'] = (out['fnat'] + 1.0 / (1.0 + (out['irmsd_backbone'] / 1.5) ** 2) + 1.0 / (1.0 + (out['lrmsd'] / 8.5) ** 2)) / 3.0
    out['flags'] = int(fi) | (int(fr) << 1)
    out['flags_mask'] = (1 if cond_i > 1e-6 else 0) | (2 if cond_r > 1e-6 else 0)
    # the bound of the residue-pair search: each residue pair is tested once per pose
    pruned, pm = 0, np.inf
    for L, G in ((lt, rt), (lp, rp)):
        (cl, rl), (cr, rr) = _bounds(L, lo), _bounds(G, ro)
        e = cl[:, None, :] - cr[None, :, :]
        gap = (np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]) - rl[:, None]) - rr[None, :]
        at = max(cuts) + 1e-6
        pruned += int((gap >= at).sum())
        pm = min(pm, float(np.abs(gap - at).min()))
    out['pruned_pairs'], out['prune_margin'] = pruned, pm
    return out


EXACT = ('native_contacts', 'model_contacts', 'shared_contacts', 'interface_residues_ligand', 'interface_residues_receptor',
         'interface_backbone_rows', 'clashes', 'pruned_pairs')
REAL_COLS = ('dockq', 'fnat', 'fnonnat', 'irmsd_backbone', 'lrmsd')
_worst = {}


def check_row(name, row, ref, key, pruning=True):
    """one row of the [C][16] buffer against the yardstick; returns the row's worst error of columns 0-4"""
    assert ref['margin'] > 1e-6, (name, ref['margin'])
    assert ref['prune_margin'] > 1e-9, (name, ref['prune_margin'])
    col = {k: row[i] for i, k in enumerate(DK.QUALITY_KEYS)}
    for k in EXACT:
        want = ref[k] if (k != 'pruned_pairs' or pruning) else 0
        assert col[k] == want, (name, k, col[k], want)
    err = 0.0
    for k in REAL_COLS:
        if np.isnan(ref[k]):
            assert np.isnan(col[k]), (name, k, col[k])
        else:
            e = abs(col[k] - ref[k])
            assert not np.isnan(col[k]) and e <= BOUND, f"{name}: {k} {col[k]!r} vs {ref[k]!r}: error {e:.3e} > {BOUND:g}"
            err = max(err, e)
    assert row[14] == 0.0 and row[15] == 0.0
    assert int(row[12]) & ref['flags_mask'] == ref['flags'] & ref['flags_mask'], (name, row[12], ref['flags'], ref['flags_mask'])
    _worst[key] = max(_worst.get(key, 0.0), err)
    return err


def report(dev):
    key = torch.device(dev).type
    print(f"dock quality [{key}]: kernels' worst error of columns 0-4 so far {_worst.get(key, 0.0):.3e} (bound {BOUND:g})")


# ---- cases: (lp, rp | None, lt, rt, lig_res_off, rec_res_off, lig_bb, rec_bb) --------------------------------------------
def _f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def _rot(rng, degrees=None):
    if degrees is None:
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        return q * np.sign(np.linalg.det(q))
    ax = rng.standard_normal(3)
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    t = np.deg2rad(degrees)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def _moved(x, R, shift):
    c = x.astype(np.float64).mean(0)
    return _f32((x - c) @ R.T + c + shift)


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(os.path.join(dc.GOLDEN, 'dockq_case.npz'))
    out = {}
    for nm in ('1AVX', '1HCF'):
        names_l, names_r = z[f'{nm}_lig_true_names'], z[f'{nm}_rec_true_names']
        for model in ('lig_equidock', 'lig_no_clashes'):
            assert (z[f'{nm}_{model}_names'] == names_l).all() and (z[f'{nm}_{model}_res_off'] == z[f'{nm}_lig_true_res_off']).all()
        out[nm] = dict(lt=z[f'{nm}_lig_true_atoms'], rt=z[f'{nm}_rec_true_atoms'], eq=z[f'{nm}_lig_equidock_atoms'],
                       nc=z[f'{nm}_lig_no_clashes_atoms'], lo=z[f'{nm}_lig_true_res_off'], ro=z[f'{nm}_rec_true_res_off'],
                       lbb=np.isin(names_l, BB).astype(np.uint8), rbb=np.isin(names_r, BB).astype(np.uint8))
    return out


@functools.lru_cache(maxsize=None)
def fixture_cases():
    f = fixture()
    return {f'{nm}_{tag}': (f[nm][key], None, f[nm]['lt'], f[nm]['rt'], f[nm]['lo'], f[nm]['ro'], f[nm]['lbb'], f[nm]['rbb'])
            for nm in ('1AVX', '1HCF') for tag, key in (('EQUIDOCK', 'eq'), ('NO_CLASHES', 'nc'))}


def _graph_case_tables(name):
    """heavy atoms of a tests/golden/graph_case* complex through atom_table on its residue lists"""
    lig, rec = dc.fixture_residues(name)
    return DK.atom_table(lig), DK.atom_table(rec)


@functools.lru_cache(maxsize=None)
def graph_cases():
    """the three graph_case complexes: the native is itself, the model the native under a seeded rigid motion"""
    out = {}
    for k, name in enumerate(dc.REAL):
        seed = 40 + k
        while True:
            rng = np.random.default_rng(seed)
            (la, _, lo, lbb, _), (ra, _, ro, rbb, _) = _graph_case_tables(name)
            case = (_moved(la, _rot(rng, 4.0), rng.standard_normal(3) * 1.5), None, la, ra, lo, ro, lbb, rbb)
            r = reference(name, case)
            if r['margin'] > 1e-6 and r['prune_margin'] > 1e-9:
                break
            _refs.pop(name)
            seed += 100
        out[name] = case
    return out


NEAR = (('1AVX', 1.0, 0.5, 11), ('1AVX', 2.0, 1.0, 12), ('1AVX', 4.0, 2.0, 13), ('1AVX', 8.0, 3.0, 14),
        ('1HCF', 1.0, 0.5, 15), ('1HCF', 3.0, 1.5, 16), ('1HCF', 5.0, 2.0, 17), ('1HCF', 8.0, 3.0, 18),
        # beyond that range: on these natives 8 degrees and 3 A in the worst direction (straight away from the receptor)
        # still leave DockQ above 0.5 (measured with ref64), so the poses that reach the acceptable and incorrect classes
        # need larger motions
        ('1AVX', 12.0, 4.5, 19), ('1HCF', 15.0, 6.0, 20), ('1AVX', 20.0, 8.0, 21), ('1HCF', 25.0, 10.0, 22))


@functools.lru_cache(maxsize=None)
def near_native_cases():
    """each fixture native under seeded rotations of 1-8 degrees about the ligand centroid plus shifts of 0.5-3 A (and
    four larger motions, see NEAR), and the exact prediction"""
    f = fixture()
    out = {}
    for nm, deg, shift, seed in NEAR:
        name = f'{nm}_near_{deg:g}deg_{shift:g}A'
        while True:
            rng = np.random.default_rng(seed)
            v = rng.standard_normal(3)
            q = f[nm]
            case = (_moved(q['lt'], _rot(rng, deg), v / np.linalg.norm(v) * shift), None, q['lt'], q['rt'], q['lo'], q['ro'],
                    q['lbb'], q['rbb'])
            r = reference(name, case)
            if r['margin'] > 1e-6 and r['prune_margin'] > 1e-9:
                break
            _refs.pop(name)
            seed += 100
        out[name] = case
    q = f['1HCF']
    out['1HCF_exact'] = (q['lt'].copy(), None, q['lt'], q['rt'], q['lo'], q['ro'], q['lbb'], q['rbb'])
    return out


def cloud(n_res_l, n_res_r, seed, big=None, sizes=(1, 14)):
    """seeded residue clouds at the PDB-like offset: residue centres on two touching slabs, 1-14 atoms within ~1.5 A of
    their centre, atoms named N, CA, C, O, CB, ... in order (so a residue of k atoms has min(k, 4) backbone rows);
    `big` (side, residue, atoms): one residue with that many atoms.  The model is the native ligand rotated by 6 degrees
    and shifted by 2 A.  Reseeded until no distance lies within 1e-6 of a cutoff."""
    while True:
        rng = np.random.default_rng(seed)
        sides = []
        for s, n in enumerate((n_res_l, n_res_r)):
            ext = max(8.0, 2.2 * np.sqrt(n))
            cen = rng.uniform(-1.0, 1.0, (n, 3)) * np.array([4.0, ext, ext]) + OFFSET + np.array([-5.5 if s == 0 else 5.5, 0.0, 0.0])
            if n == 1:
                cen = OFFSET[None, :] + np.array([[-1.9 if s == 0 else 1.9, 0.0, 0.0]])
            na = rng.integers(sizes[0], sizes[1] + 1, n)
            if big is not None and big[0] == s:
                na[big[1]] = big[2]
            if n == 1:
                na[:] = 1
            off = np.concatenate([[0], np.cumsum(na)]).astype(np.int32)
            x = np.repeat(cen, na, axis=0) + (rng.standard_normal((off[-1], 3)) * 0.9 if n > 1 else 0.0)
            bb = np.concatenate([(np.arange(k) < 4) for k in na]).astype(np.uint8)
            sides.append((_f32(x), off, bb))
        (lt, lo, lbb), (rt, ro, rbb) = sides
        v = rng.standard_normal(3)
        lp = _moved(lt, _rot(rng, 6.0), v / np.linalg.norm(v) * (2.0 if n_res_l > 1 else 0.3))
        case = (lp, None, lt, rt, lo, ro, lbb, rbb)
        r = ref64(*case)
        if r['margin'] > 1e-6 and r['prune_margin'] > 1e-9:
            return case
        seed += 1000


# residue counts either side of the residue tile (8) and chunk (32), atom counts either side of the 512-atom staging of a
# chunk (32 residues of ~7.5 atoms: ~240; `sizes` 14-18 atoms per residue: 32 residues pass 512), backbone rows either
# side of the 256-row moment tile, a 1 x 1 complex of one atom each, a residue longer than the staging
EDGES = {'edge_7x31': (7, 31, 201, None, (1, 14)), 'edge_8x32': (8, 32, 202, None, (1, 14)),
         'edge_9x33': (9, 33, 203, None, (1, 14)), 'edge_17x65': (17, 65, 204, None, (1, 14)),
         'edge_stage_under': (10, 32, 205, None, (15, 15)),           # 480 receptor atoms in the one chunk
         'edge_stage_over': (10, 33, 206, None, (16, 17)),            # > 512 atoms in the first chunk
         'edge_bb_256': (20, 44, 207, None, (4, 4)),                  # (20 + 44) x 4 = 256 backbone rows and atoms
         'edge_bb_257': (21, 44, 208, None, (4, 5)),
         'edge_long_residue': (9, 12, 209, (1, 3, 600), (1, 14)),     # a receptor residue of 600 atoms (> the staging)
         'edge_1x1': (1, 1, 210, None, (1, 1))}


@functools.lru_cache(maxsize=None)
def edge_cases():
    return {k: cloud(nl, nr, seed, big, sizes) for k, (nl, nr, seed, big, sizes) in EDGES.items()}


@functools.lru_cache(maxsize=None)
def degenerate_cases():
    rng = np.random.default_rng(77)
    out = {}
    lp, _, lt, rt, lo, ro, lbb, rbb = cloud(6, 9, 301)
    far = np.float32([40.0, 0.0, 0.0])
    # the native's sides 40 A apart, the model docked: no native contact, no interface residue
    out['no_native_contact'] = (_f32(lt), None, _f32(lt - far), rt, lo, ro, lbb, rbb)
    # the model 40 A away: no model contact
    out['no_model_contact'] = (_f32(lt - far), None, lt, rt, lo, ro, lbb, rbb)
    out['no_ligand_backbone'] = (lp, None, lt, rt, lo, ro, np.zeros_like(lbb), rbb)
    # an interface of one backbone row: one atom per side in reach, the only backbone row of the ligand; the receptor's
    # backbone lies outside the interface
    lt1 = _f32(OFFSET + np.array([[0.0, 0.0, 0.0], [-14.0, 1.0, 0.0], [-15.0, -2.0, 3.0]]))
    rt1 = _f32(OFFSET + np.array([[4.0, 0.5, 0.0], [19.0, 1.0, 2.0], [21.0, -1.0, 1.0], [20.0, 3.0, -2.0]]))
    o3, o4 = np.int32([0, 1, 2, 3]), np.int32([0, 1, 2, 3, 4])
    out['one_interface_row'] = (_moved(lt1, _rot(rng, 5.0), np.array([0.4, 0.2, -0.3])), None, lt1, rt1, o3, o4,
                                np.uint8([1, 0, 0]), np.uint8([0, 1, 1, 1]))
    s = np.array([-7.0, -3.0, 0.5, 2.0, 4.3, 9.1, 12.4])[:, None]
    line = _f32(OFFSET + s * np.array([[1.0, 2.0, -0.5]]) / np.linalg.norm([1.0, 2.0, -0.5]))
    # (a receptor residue far from the ligand and off the line keeps the receptor's own backbone set well conditioned)
    u = np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    far_res = _f32(OFFSET + 27.0 * u + np.array([[1.0, 0.0, 2.0], [-1.0, 1.5, 0.0], [0.5, -2.0, -1.0], [2.0, 1.0, 1.0]]))
    out['collinear'] = (_moved(line[:4], _rot(rng, 7.0), np.array([0.5, -0.2, 0.3])), None, line[:4],
                        np.concatenate((line[4:], far_res)), np.int32([0, 2, 4]), np.int32([0, 1, 3, 7]), np.ones(4, np.uint8),
                        np.ones(7, np.uint8))
    return out


def all_cases():
    return {**fixture_cases(), **graph_cases(), **near_native_cases(), **edge_cases(), **degenerate_cases()}


_refs = {}


def reference(name, case):
    if name not in _refs:
        _refs[name] = ref64(*case)
    return _refs[name]


# ---- running --------------------------------------------------------------------------------------------------------
def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run(dev, cases, cuts=CUTS, full=False):
    """one pose_quality_batch over `cases` -> the [C][16] rows on the host"""
    cases = list(cases)
    rp = [_t(c[1] if c[1] is not None else c[3], dev) for c in cases] if any(c[1] is not None for c in cases) else None
    out = DK.pose_quality_batch([_t(c[0], dev) for c in cases], [_t(c[2], dev) for c in cases], [_t(c[3], dev) for c in cases],
                                [c[4] for c in cases], [c[5] for c in cases], [c[6] for c in cases], [c[7] for c in cases],
                                rec_pred_list=rp, contact_cutoff=cuts[0], interface_cutoff=cuts[1], clash_cutoff=cuts[2])
    for k in DK.QUALITY_KEYS:
        assert out[k].dtype == torch.float64 and out[k].shape == (len(cases),) and out[k].device.type == torch.device(dev).type
    return out if full else out['quality'].cpu().numpy()


_rows = {}


def measured(dev):
    """ALL cases of this file in ONE batch - computed once per device type and shared by the tests"""
    key = torch.device(dev).type
    if key not in _rows:
        cases = all_cases()
        names = list(cases)
        _rows[key] = (names, run(dev, [cases[n] for n in names]))
    return _rows[key]


def check_names(dev, names):
    all_names, rows = measured(dev)
    cases = all_cases()
    key = torch.device(dev).type
    for n in names:
        check_row(n, rows[all_names.index(n)], reference(n, cases[n]), key)
    report(dev)
    return {n: rows[all_names.index(n)] for n in names}


# the table of the issue (computed there by a separate script): atoms L / R, residues L / R, native contacts, model
# contacts, fnat, fnonnat, interface residues L / R, iRMSD(bb), LRMSD(bb), DockQ, atom pairs < 3 A
TABLE = {'1AVX_EQUIDOCK': (1286, 1630, 172, 223, 63, 547, '0.000', '1.000', 49, 93, '14.967', '35.793', '0.021', 1500),
         '1AVX_NO_CLASHES': (1286, 1630, 172, 223, 63, 32, '0.000', '1.000', 49, 93, '15.690', '38.724', '0.018', 31),
         '1HCF_EQUIDOCK': (809, 1802, 101, 242, 72, 688, '0.056', '0.994', 61, 82, '11.687', '25.431', '0.057', 2044),
         '1HCF_NO_CLASHES': (809, 1802, 101, 242, 72, 20, '0.083', '0.700', 61, 82, '8.103', '13.689', '0.132', 39)}


def check_yardstick_reproduces_the_table():
    """CPU: ref64 on the fixture gives the table to the digits printed"""
    for name, case in fixture_cases().items():
        r, t = reference(name, case), TABLE[name]
        got = (len(case[2]), len(case[3]), len(case[4]) - 1, len(case[5]) - 1, r['native_contacts'], r['model_contacts'],
               f"{r['fnat']:.3f}", f"{r['fnonnat']:.3f}", r['interface_residues_ligand'], r['interface_residues_receptor'],
               f"{r['irmsd_backbone']:.3f}", f"{r['lrmsd']:.3f}", f"{r['dockq']:.3f}", r['clashes'])
        assert got == t, (name, got, t)
        assert r['margin'] > 1e-5, (name, r['margin'])      # (over all three cutoffs in both poses)


def check_real(dev):
    """1. the four fixture models and the three graph_case complexes (in the one batch of `measured`)"""
    rows = check_names(dev, list(fixture_cases()) + list(graph_cases()))
    big = graph_cases()['graph_case_big']
    assert len(big[2]) > 10000 and rows['graph_case_big'][5] > 0


def check_near_native(dev):
    """2. near-native poses: fnat in (0.2, 0.9) occurs, DockQ lies on both sides of 0.23, 0.49 and 0.80; an exact
    prediction gives fnat 1, RMSDs below the bound and DockQ 1"""
    cases = near_native_cases()
    rows = check_names(dev, list(cases))
    refs = [reference(n, cases[n]) for n in cases if n != '1HCF_exact']
    assert any(0.2 < r['fnat'] < 0.9 for r in refs), [r['fnat'] for r in refs]
    dq = np.array([r['dockq'] for r in refs])
    for edge in (0.23, 0.49, 0.80):
        assert (dq < edge).any() and (dq >= edge).any(), (edge, dq)
    e = rows['1HCF_exact']
    assert e[1] == 1.0 and 0.0 <= e[3] <= BOUND and 0.0 <= e[4] <= BOUND and abs(e[0] - 1.0) <= BOUND and e[2] == 0.0, e


def check_edges(dev):
    """3. tile, chunk, staging and moment-tile edges"""
    cases = edge_cases()
    check_names(dev, list(cases))
    sizes = {n: (len(c[4]) - 1, len(c[5]) - 1, len(c[3]), int(c[6].sum() + c[7].sum())) for n, c in cases.items()}
    assert {sizes[n][0] for n in ('edge_7x31', 'edge_8x32', 'edge_9x33')} == {TILE - 1, TILE, TILE + 1}
    assert {sizes[n][1] for n in ('edge_7x31', 'edge_8x32', 'edge_9x33')} == {CHUNK - 1, CHUNK, CHUNK + 1}
    assert sizes['edge_17x65'][:2] == (2 * TILE + 1, 2 * CHUNK + 1)
    assert sizes['edge_stage_under'][2] < STAGE and sizes['edge_stage_under'][1] == CHUNK
    assert cases['edge_stage_over'][5][CHUNK] > STAGE            # the first chunk alone holds more atoms than are staged
    assert sizes['edge_bb_256'][3] == ROWS and sizes['edge_bb_257'][3] > ROWS and sizes['edge_7x31'][3] < ROWS
    assert np.diff(cases['edge_long_residue'][5]).max() > STAGE
    assert sizes['edge_1x1'][:3] == (1, 1, 1) and len(cases['edge_1x1'][2]) == 1
    for n, c in cases.items():
        r = reference(n, c)
        if n == 'edge_1x1':
            assert r['pairs'] == 1
            continue
        assert r['native_contacts'] > 0 and r['native_contacts'] < r['pairs'] and r['pruned_pairs'] > 0, (n, r)


def check_degenerate(dev):
    """4. degenerate sets"""
    cases = degenerate_cases()
    rows = check_names(dev, list(cases))
    r = rows['no_native_contact']
    assert r[5] == 0 and np.isnan(r[1]) and np.isnan(r[0]) and r[6] > 0 and r[2] == 1.0 and np.isfinite(r[4])
    assert r[8] == 0 and r[9] == 0 and r[10] == 0 and np.isnan(r[3])                 # no interface residue either
    r = rows['no_model_contact']
    assert r[6] == 0 and r[2] == 0.0 and r[5] > 0 and r[1] == 0.0 and np.isfinite(r[0])
    r = rows['no_ligand_backbone']
    assert np.isnan(r[4]) and np.isnan(r[0]) and np.isfinite(r[3]) and r[5] > 0
    r = rows['one_interface_row']
    assert r[10] == 1 and r[8] == 1 and r[9] == 1 and 0.0 <= r[3] <= BOUND
    assert rows['collinear'][10] == 7 and rows['collinear'][9] == 2           # the seven rows on the line
    # rec_pred given as a rigidly moved receptor against rec_pred = None with the ligand moved by the inverse: the motion
    # g(x, y, z) = (-y + 8, x - 16, z) - a quarter turn about z and a shift - is exact in fp32 on these coordinates, so the
    # two calls describe the same geometry bit for bit and columns 0-4 must agree within the bound
    lp, _, lt, rt, lo, ro, lbb, rbb = edge_cases()['edge_9x33']

    def g(x):
        y = np.stack([-x[:, 1] + np.float32(8.0), x[:, 0] - np.float32(16.0), x[:, 2]], axis=1)
        assert y.dtype == np.float32
        x64 = x.astype(np.float64)
        assert (y.astype(np.float64) == np.stack([-x64[:, 1] + 8.0, x64[:, 0] - 16.0, x64[:, 2]], axis=1)).all()
        return np.ascontiguousarray(y)

    given = (g(lp), g(rt), lt, rt, lo, ro, lbb, rbb)
    a, b = run(dev, [given])[0], run(dev, [(lp, None, lt, rt, lo, ro, lbb, rbb)])[0]
    key = torch.device(dev).type
    check_row('rec_pred_given', a, ref64(*given), key)
    assert np.abs(a[:5] - b[:5]).max() <= BOUND, (a[:5], b[:5])
    assert a[5:12].tobytes() == b[5:12].tobytes() and a[3] > 0.1 and a[4] > 0.1


def check_bits(dev):
    """5. a complex's row alone, first, last, in a permuted batch and on a second run is identical as bits"""
    e, f = edge_cases(), fixture_cases()
    cases = [e['edge_17x65'], f['1HCF_NO_CLASHES'], e['edge_1x1'], e['edge_long_residue'], degenerate_cases()['collinear']]
    n = len(cases)
    perm = [3, 0, 4, 2, 1]
    together, again = run(dev, cases), run(dev, cases)
    permuted = run(dev, [cases[p] for p in perm])
    assert together.tobytes() == again.tobytes(), 'run to run'
    for i in range(n):
        alone = run(dev, [cases[i]])[0]
        rest = [cases[j] for j in range(n) if j != i]
        first, last = run(dev, [cases[i]] + rest)[0], run(dev, rest + [cases[i]])[-1]
        for what, row in (('alone', alone), ('first', first), ('last', last), ('permuted', permuted[perm.index(i)])):
            assert row.tobytes() == together[i].tobytes(), (i, what, row, together[i])


def check_pruning(dev, monkeypatch):
    """6. the same batch with pruning disabled: the same bits in every column but 13"""
    e, f = edge_cases(), fixture_cases()
    names = ['edge_17x65', '1AVX_NO_CLASHES', 'edge_long_residue', 'edge_stage_over']
    cases = [{**e, **f}[n] for n in names]
    on = run(dev, cases)
    monkeypatch.setenv('EQD_DOCK_QUALITY_PRUNE', '0')
    assert not DK.quality_pruning_enabled()
    off = run(dev, cases)
    monkeypatch.undo()
    assert DK.quality_pruning_enabled()
    keep = [k for k in range(16) if k != 13]
    assert on[:, keep].tobytes() == off[:, keep].tobytes(), (on, off)
    assert (off[:, 13] == 0).all() and (on[:, 13] > 0).all()
    key = torch.device(dev).type
    for n, c, row in zip(names, cases, off):
        check_row(n, row, reference(n, c), key, pruning=False)


def check_validation_errors(dev):
    """7. refused before any launch, with a message (the three entry points and pose_quality_batch)"""
    lib = DK.load_dock_library()
    lig, rec = torch.zeros(4, 3, device=dev), torch.ones(5, 3, device=dev)
    lo, ro, lb, rb = np.int32([0, 2, 4]), np.int32([0, 1, 5]), np.uint8([1, 0, 1, 0]), np.ones(5, np.uint8)
    good = dict(lig_res_offsets=[lo], rec_res_offsets=[ro], lig_backbone=[lb], rec_backbone=[rb])
    assert DK.pose_quality_batch([lig], [lig], [rec], **good)['quality'].shape == (1, 16)
    with pytest.raises(ValueError, match='predicted ligands for'):
        DK.pose_quality_batch([lig, lig], [lig], [rec], **good)
    with pytest.raises(ValueError, match='complex 0: 3 predicted ligand rows for 4 true ones'):
        DK.pose_quality_batch([lig[:3]], [lig], [rec], **good)
    with pytest.raises(ValueError, match='complex 0: ligand: residue offsets'):
        DK.pose_quality_batch([lig], [lig], [rec], **dict(good, lig_res_offsets=[np.int32([0, 2, 3])]))
    with pytest.raises(ValueError, match='complex 0: receptor: residue offsets'):
        DK.pose_quality_batch([lig], [lig], [rec], **dict(good, rec_res_offsets=[np.int32([0, 3, 3, 5])]))
    with pytest.raises(ValueError, match='rows for tables of'):
        DK.pose_quality_batch([lig[:3]], [lig[:3]], [rec], **good)
    with pytest.raises(ValueError, match='are needed'):
        DK.pose_quality_batch([lig], [lig], [rec])
    with pytest.raises(_lib.EquidockHipError, match='contact_cutoff'):
        DK.pose_quality_batch([lig], [lig], [rec], contact_cutoff=0.0, **good)
    wrong = torch.zeros(4, 3, device='cuda' if torch.device(dev).type == 'cpu' and torch.cuda.is_available() else 'cpu')
    if wrong.device.type != torch.device(dev).type:
        with pytest.raises(_lib.EquidockHipError, match='no CPU fallback|only takes CPU tensors'):
            DK.pose_quality_batch([wrong], [wrong], [rec], **good)

    def offs(v):
        return np.ascontiguousarray(np.asarray(v, dtype=np.int32))

    def p(a):
        return a.ctypes.data_as(C.c_void_p)

    la, ra, lr, rr = offs([0, 4, 8]), offs([0, 5, 10]), offs([0, 2, 4]), offs([0, 2, 4])
    wsb = lib.eqd_dock_quality_workspace_bytes(2, p(la), p(ra), p(lr), p(rr))
    assert wsb > 0
    bad = offs([0, 6, 4])
    assert lib.eqd_dock_quality_workspace_bytes(2, p(bad), p(ra), p(lr), p(rr)) == 0
    assert b'complex 1 has -2 ligand' in lib.eqd_dock_last_error()
    assert lib.eqd_dock_quality_workspace_bytes(2, p(offs([0, 4, 4])), p(ra), p(lr), p(rr)) == 0          # an empty side
    assert lib.eqd_dock_quality_workspace_bytes(2, p(offs([1, 4, 8])), p(ra), p(lr), p(rr)) == 0
    assert lib.eqd_dock_quality_workspace_bytes(2, p(la), p(ra), p(offs([0, 5, 7])), p(rr)) == 0          # 5 residues, 4 atoms
    assert b'tiles its complex' in lib.eqd_dock_last_error()
    assert lib.eqd_dock_quality_workspace_bytes(2, p(la), p(ra), p(lr), p(offs([0, 2, 2]))) == 0          # no residue
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    out = torch.full((2, 16), 7.0, dtype=torch.float64, device=dev)
    l2, r2 = torch.cat([lig, lig]), torch.cat([rec, rec])
    lf, rf = _t(np.int32([0, 2, 4, 6, 8]), dev), _t(np.int32([0, 2, 5, 7, 10]), dev)
    lbb, rbb = torch.ones(8, dtype=torch.uint8, device=dev), torch.ones(10, dtype=torch.uint8, device=dev)
    st = DK._stream(dev)
    W = C.c_void_p(ws.data_ptr())
    assert lib.eqd_dock_quality_init(2, p(bad), p(ra), p(lr), p(rr), W, C.c_size_t(wsb), st) == 2
    assert lib.eqd_dock_quality_init(2, p(la), p(ra), p(lr), p(rr), W, C.c_size_t(64), st) == 4
    assert b'workspace too small' in lib.eqd_dock_last_error()

    def ev(la_, size, cuts, first=lf):
        return lib.eqd_dock_quality_eval(2, p(la_), p(ra), p(lr), p(rr), C.c_void_p(l2.data_ptr()), C.c_void_p(0),
                                         C.c_void_p(l2.data_ptr()), C.c_void_p(r2.data_ptr()),
                                         C.c_void_p(first.data_ptr()) if first is not None else C.c_void_p(0),
                                         C.c_void_p(rf.data_ptr()), C.c_void_p(lbb.data_ptr()), C.c_void_p(rbb.data_ptr()),
                                         C.c_double(cuts[0]), C.c_double(cuts[1]), C.c_double(cuts[2]), 1,
                                         C.c_void_p(out.data_ptr()), W, C.c_size_t(size), st)

    assert ev(bad, wsb, CUTS) == 2
    assert ev(la, 64, CUTS) == 4
    assert ev(la, wsb, CUTS, first=None) == 1
    for k in range(3):
        for v in (0.0, -1.0, float('inf'), float('nan')):
            cuts = list(CUTS)
            cuts[k] = v
            assert ev(la, wsb, cuts) == 2 and b'cutoff' in lib.eqd_dock_last_error()
    # nothing was written by the refused calls
    assert bool((out.cpu() == 7.0).all()) and bool((ws.cpu() == 0).all())


def check_atom_table(tmp_path):
    """atom_table on a written file: file order (not the sorted grouping), hydrogens dropped, the index among all ATOM
    rows, insertion codes split residues, the same table from the residue list"""
    from equidock_public_amd import featurize as FZ
    lines = ["ATOM      1  N   GLY B   2       1.000   2.000   3.000  1.00  0.00           N",
             "ATOM      2  H   GLY B   2       1.500   2.000   3.000  1.00  0.00           H",
             "ATOM      3  CA  GLY B   2       2.000   2.000   3.000  1.00  0.00           C",
             "ATOM      4  N   ALA B   2A      3.000   2.000   3.000  1.00  0.00           N",
             "ATOM      5 HB1  ALA B   2A      3.500   2.000   3.000  1.00  0.00",
             "ATOM      6  CB  ALA B   2A      4.000   2.000   3.000  1.00  0.00           C",
             "ATOM      7  O   SER A   1       5.000   2.000   3.000  1.00  0.00           O",
             "HETATM    8  O   HOH A   9       9.000   9.000   9.000  1.00  0.00           O"]
    path = tmp_path / 'x.pdb'
    path.write_text('\n'.join(lines) + '\nEND\n')
    atoms, index, off, bb, names = DK.atom_table(str(path))
    assert atoms.dtype == np.float32 and atoms[:, 0].tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]
    assert index.tolist() == [0, 2, 3, 5, 6] and off.tolist() == [0, 2, 4, 5] and off.dtype == np.int32
    assert bb.tolist() == [1, 1, 1, 0, 1] and bb.dtype == np.uint8 and names.tolist() == ['N', 'CA', 'N', 'CB', 'O']
    res = [FZ.Residue('B', 2, 'GLY', ['N', 'H', 'CA'], ['N', 'H', 'C'], atoms[[0, 0, 1]]),
           FZ.Residue('A', 1, 'SER', ['O'], ['O'], atoms[[4]])]
    a2, i2, o2, b2, n2 = DK.atom_table(res)
    assert i2.tolist() == [0, 2, 3] and o2.tolist() == [0, 2, 3] and b2.tolist() == [1, 1, 1] and n2.tolist() == ['N', 'CA', 'O']


def check_dock_complexes_quality(dev, names, max_it, check_every):
    """9. dock_complexes(quality=True): its values equal pose_quality_batch on the returned ligand_atoms, and the same call
    with quality=False returns what it does without the argument - same keys, same bits"""
    net, _, _ = dc.seeded_net(dev)
    residues = [dc.fixture_residues(n) for n in names]
    truths = [lig for lig, _ in residues]
    kw = dict(remove_clashes=True, max_it=max_it, check_every=check_every, device=dev, ground_truth=truths)
    plain = DK.dock_complexes(net, residues, **kw)
    off = DK.dock_complexes(net, residues, quality=False, **kw)
    res = DK.dock_complexes(net, residues, quality=True, **kw)
    added = {'dockq', 'fnat', 'fnonnat', 'irmsd_backbone', 'lrmsd', 'native_contacts', 'model_contacts', 'clashes'}
    tabs = [(DK.atom_table(lig), DK.atom_table(rec)) for lig, rec in residues]
    want = DK.pose_quality_batch([r['ligand_atoms'][_t(tl[1], dev)] for r, (tl, _) in zip(res, tabs)],
                                 [_t(tl[0], dev) for tl, _ in tabs], [_t(tr[0], dev) for _, tr in tabs],
                                 [tl[2] for tl, _ in tabs], [tr[2] for _, tr in tabs], [tl[3] for tl, _ in tabs],
                                 [tr[3] for _, tr in tabs])['quality'].cpu().numpy()
    for i, (r, q, o) in enumerate(zip(res, plain, off)):
        assert set(o) == set(q) and set(o['batch_seconds']) == set(q['batch_seconds'])
        assert set(r) - set(q) == added, set(r) ^ set(q)
        assert set(r['batch_seconds']) - set(q['batch_seconds']) == {'quality'}
        for a in (o, r):
            assert a['rotation'].tobytes() == q['rotation'].tobytes() and a['translation'].tobytes() == q['translation'].tobytes()
            assert torch.equal(a['ligand_atoms'], q['ligand_atoms']) and a['clash_iterations'] == q['clash_iterations']
            assert np.float64(a['crmsd']).tobytes() == np.float64(q['crmsd']).tobytes()
            assert np.float64(a['irmsd']).tobytes() == np.float64(q['irmsd']).tobytes()
        got = np.float64([r['dockq'], r['fnat'], r['fnonnat'], r['irmsd_backbone'], r['lrmsd'], r['native_contacts'],
                          r['model_contacts']])
        assert got.tobytes() == want[i, :7].tobytes(), (names[i], got, want[i])
        assert r['clashes'] == int(want[i, 11]) and isinstance(r['clashes'], int) and isinstance(r['dockq'], float)
        assert r['native_contacts'] > 0
    lig0 = residues[0][0]
    from equidock_public_amd import featurize as FZ
    renamed = list(lig0)
    r0 = renamed[0]
    renamed[0] = FZ.Residue(r0.chain, r0.number, r0.resname, ['XX'] + list(r0.atom_names[1:]), r0.elements, r0.coords)
    with pytest.raises(ValueError, match='complex 0'):
        DK.dock_complexes(net, residues[:1], quality=True, **dict(kw, ground_truth=[renamed]))
    with pytest.raises(ValueError, match='ground_truth'):
        DK.dock_complexes(net, residues[:1], quality=True, **dict(kw, ground_truth=None))
    return res
