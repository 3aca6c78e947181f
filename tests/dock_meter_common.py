"""Checks of the batched RMSD meter (equidock_public_amd.dock.rmsd_metrics_batch / DeviceMeter, eqd_dock_meter_* of
libequidock_dock.so) shared by the simulator tests (tests/test_dock_meter_sim.py) and the GPU tests
(tests/test_dock_meter_gpu.py).

Yardstick: `ref64`, a float64 numpy evaluation of the reference's definitions (src/utils/eval.py:27-36, Kabsch of
src/utils/protein_utils.py:31-64 with np.linalg.svd, the interface pair list of eval_pdb_outputset.py:80-94).
Error: |got - ref64| in Angstrom per column.  Bound: ONE TENTH of the worst distance of the float32 host path
(inference.rmsd_metrics / inference.complex_and_interface_rmsd) from the same yardstick over this file's cases - fp64
accumulation on the device has to be clearly better than the float32 path it replaces.

Measured (all 13 cases of this file; the tests print these figures):
    float32 host path, worst distance from the yardstick    6.214e-06 A   (so the bound is 6.214e-07 A)
    kernels on the x86 simulator, worst error               8.527e-14 A
    kernels on the MI355X, worst error                      8.527e-14 A
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from equidock_public_amd import _lib, dock as DK, inference as INF
from tests import dock_common as dc

CUTOFF = 8.0
OFFSET = np.array([83.0, 72.0, 243.0])        # a PDB-like frame (1DE4's receptor)
COLS = ('ligand_rmsd', 'receptor_rmsd', 'complex_rmsd', 'interface_rmsd')


# ---- the float64 yardstick ------------------------------------------------------------------------------------------
def _kabsch64(P, T):
    """(RMSD of R p + b - t, reflection branch taken, smallest / largest singular value)"""
    cp, ct = P.mean(0), T.mean(0)
    H = (P - cp).T @ (T - ct)
    U, S, Vt = np.linalg.svd(H)
    R = Vt.T @ U.T
    reflect = bool(np.linalg.det(R) < 0)
    if reflect:
        R = (Vt.T @ np.diag([1.0, 1.0, -1.0])) @ U.T
    b = ct - R @ cp
    e = (R @ P.T).T + b - T
    return float(np.sqrt(np.mean(np.sum(e * e, axis=1)))), reflect, (float(S[2] / S[0]) if S[0] > 0 else 0.0)


def ref64(lp, rp, lt, rt, cutoff=CUTOFF):
    lp, lt, rt = (np.asarray(a, dtype=np.float64) for a in (lp, lt, rt))
    rp = rt if rp is None else np.asarray(rp, dtype=np.float64)
    out = {'ligand_rmsd': float(np.sqrt(np.mean(np.sum((lp - lt) ** 2, axis=1)))),
           'receptor_rmsd': float(np.sqrt(np.mean(np.sum((rp - rt) ** 2, axis=1))))}
    out['complex_rmsd'], fc, cond_c = _kabsch64(np.concatenate((lp, rp)), np.concatenate((lt, rt)))
    d = np.sqrt(((lt[:, None, :] - rt[None, :, :]) ** 2).sum(-1))
    al, ar = np.where(d < cutoff)                                         # the pair list: a row once per partner
    out['interface_pairs'] = int(al.size)
    out['margin'] = float(np.abs(d - cutoff).min())
    fi, cond_i = False, 0.0
    if al.size:
        out['interface_rmsd'], fi, cond_i = _kabsch64(np.concatenate((lp[al], rp[ar])), np.concatenate((lt[al], rt[ar])))
    else:
        out['interface_rmsd'] = float('nan')
    out['flags'] = int(fc) | (int(fi) << 1)
    out['flags_mask'] = (1 if cond_c > 1e-6 else 0) | (2 if cond_i > 1e-6 else 0)     # bits that are well determined
    return out


def host32(lp, rp, lt, rt):
    """the reference-pinned float32 host path this feature replaces"""
    rp = rt if rp is None else rp
    lig, rec, cpx = INF.rmsd_metrics(lp, rp, lt, rt)
    out = {'ligand_rmsd': float(lig), 'receptor_rmsd': float(rec), 'complex_rmsd': float(cpx)}
    d = np.sqrt(((np.asarray(lt, np.float64)[:, None, :] - np.asarray(rt, np.float64)[None, :, :]) ** 2).sum(-1))
    out['interface_rmsd'] = float(INF.complex_and_interface_rmsd(lp, rp, lt, rt)[1]) if (d < CUTOFF).any() else float('nan')
    return out


# ---- cases ----------------------------------------------------------------------------------------------------------
def _rot(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q * np.sign(np.linalg.det(q))


def _f32(*arrays):
    return tuple(None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in arrays)


def cloud_case(n_l, n_r, seed):
    """seeded clouds at a PDB-like offset whose surfaces touch (a few points: closer together, so that some pair is under
    the cutoff and some above), with a rotated and shifted ligand prediction"""
    rng = np.random.default_rng(seed)
    small = n_l + n_r <= 8
    lt = rng.standard_normal((n_l, 3)) * (3.0 if small else 6.0) + OFFSET
    rt = rng.standard_normal((n_r, 3)) * (3.0 if small else 7.0) + OFFSET + np.array([6.0 if small else 11.0, 0.0, 0.0])
    R = _rot(rng)
    lp = (lt - lt.mean(0)) @ R.T + lt.mean(0) + rng.standard_normal(3) * 4.0 + rng.standard_normal((n_l, 3)) * 0.3
    return _f32(lp, None, lt, rt)


@functools.lru_cache(maxsize=None)
def golden_cases():
    z = np.load(os.path.join(dc.GOLDEN, 'eval_case.npz'))
    cases = {str(nm): _f32(z[f'{nm}_lm'], None, z[f'{nm}_lg'], z[f'{nm}_rg']) for nm in z['names']}
    m = np.load(os.path.join(dc.GOLDEN, 'inference_case.npz'))
    cases['meter'] = _f32(m['m_lp'], m['m_rp'], m['m_lt'], m['m_rt'])
    return cases


EDGE_SHAPES = ((1, 3), (2, 2), (255, 513), (256, 512), (257, 1025))      # either side of the 256-row tile and 512-partner chunk
EDGE_SEEDS = (105, 101, 102, 103, 104)          # (every case has pairs under and above the cutoff)


@functools.lru_cache(maxsize=None)
def edge_cases():
    return {f'edge_{n_l}x{n_r}': cloud_case(n_l, n_r, seed) for (n_l, n_r), seed in zip(EDGE_SHAPES, EDGE_SEEDS)}


@functools.lru_cache(maxsize=None)
def degenerate_cases():
    rng = np.random.default_rng(7)
    cases = {}
    lt = rng.standard_normal((3, 3)) * 2.0 + OFFSET
    cases['no_pair'] = _f32(lt + rng.standard_normal((3, 3)), None, lt, (OFFSET + 100.0)[None, :])
    lt = OFFSET + np.array([[0.0, 0.0, 0.0], [-9.0, 1.0, 0.0], [-14.0, -2.0, 3.0]])
    rt = OFFSET + np.array([[5.0, 0.5, 0.0], [15.0, 1.0, 2.0]])
    cases['one_pair'] = _f32(lt @ _rot(rng).T + 3.0, None, lt, rt)                        # rank-1 interface H
    s = np.array([-7.0, -3.0, 0.5, 2.0, 4.0, 9.0, 12.0])[:, None]
    line = OFFSET + s * np.array([[1.0, 2.0, -0.5]]) / np.linalg.norm([1.0, 2.0, -0.5])
    cases['collinear'] = _f32((line[:4] - OFFSET) @ _rot(rng).T + OFFSET + 1.0, None, line[:4], line[4:])
    lp, _, lt, rt = cloud_case(40, 55, 9)
    cases['exact'] = (lt.copy(), None, lt, rt)
    return cases


def all_cases():
    return {**golden_cases(), **edge_cases(), **degenerate_cases()}


# ---- running --------------------------------------------------------------------------------------------------------
def _t(a, dev):
    return torch.from_numpy(a).to(dev)


def run(dev, cases, interface=True, explicit_rec_pred=False):
    """one rmsd_metrics_batch over `cases` (a list of (lp, rp | None, lt, rt)) -> the [C][8] rows on the host.  The
    receptor prediction list is passed when any case has one (the others pass rec_true) or `explicit_rec_pred`."""
    cases = list(cases)
    with_rp = explicit_rec_pred or any(c[1] is not None for c in cases)
    rp = [_t(c[1] if c[1] is not None else c[3], dev) for c in cases] if with_rp else None
    out = DK.rmsd_metrics_batch([_t(c[0], dev) for c in cases], [_t(c[2], dev) for c in cases],
                                [_t(c[3], dev) for c in cases], rp, cutoff=CUTOFF, interface=interface)
    for k in COLS + ('interface_pairs', 'flags'):
        assert out[k].dtype == torch.float64 and out[k].shape == (len(cases),) and out[k].device.type == torch.device(dev).type
    return out['metrics'].cpu().numpy()


_measured = {}


def measured(dev):
    """All cases of this file in ONE batch, the yardstick and the float32 host path of every case - computed once per
    device type and shared by the tests.  Returns dict(names, rows, ref, f32, f32_distance, bound, kernel_error)."""
    key = torch.device(dev).type
    if key in _measured:
        return _measured[key]
    cases = all_cases()
    names = list(cases)
    rows = run(dev, [cases[n] for n in names])
    ref = {n: ref64(*cases[n]) for n in names}
    f32 = {n: host32(*cases[n]) for n in names}
    dist, err = 0.0, 0.0
    for i, n in enumerate(names):
        for k, col in enumerate(COLS):
            r = ref[n][col]
            if np.isnan(r):
                continue
            dist = max(dist, abs(f32[n][col] - r))
            if not np.isnan(rows[i, k]):
                err = max(err, abs(rows[i, k] - r))
    print(f"dock meter [{key}]: float32 host path worst distance from the float64 yardstick {dist:.3e} A, "
          f"bound {0.1 * dist:.3e} A, kernels' worst error {err:.3e} A over {len(names)} cases")
    _measured[key] = dict(names=names, rows=rows, ref=ref, f32=f32, f32_distance=dist, bound=0.1 * dist, kernel_error=err)
    return _measured[key]


def check_case(m, name):
    """every column of one case against the yardstick at the bound; pair count exact; flags where well determined"""
    assert m['f32_distance'] > 0.0, "the float32 path's distance is 0: the bound has collapsed"
    i, ref, row = m['names'].index(name), m['ref'][name], m['rows'][m['names'].index(name)]
    for k, col in enumerate(COLS):
        if np.isnan(ref[col]):
            assert np.isnan(row[k]), (name, col, row[k])
        else:
            assert not np.isnan(row[k]) and abs(row[k] - ref[col]) <= m['bound'], \
                f"{name}: {col} {row[k]!r} vs {ref[col]!r}: error {abs(row[k] - ref[col]):.3e} > bound {m['bound']:.3e}"
    assert row[4] == ref['interface_pairs'], (name, row[4], ref['interface_pairs'])
    assert row[6] == 0.0 and row[7] == 0.0
    mask = ref['flags_mask']
    assert int(row[5]) & mask == ref['flags'] & mask, (name, row[5], ref['flags'], mask)
    return i


def check_golden(dev):
    """the recorded results of the reference (float32) at the float32 path's own distance, the yardstick at the bound,
    and the reflection branches of the real data: the interface sets of 1AVX and 1HCF take it, nothing else does"""
    m = measured(dev)
    z = np.load(os.path.join(dc.GOLDEN, 'eval_case.npz'))
    tol = m['f32_distance']
    for nm in ('1AVX', '1H1V', '1HCF'):
        i = check_case(m, nm)
        assert abs(m['rows'][i, 2] - float(z[f'{nm}_crmsd'])) <= tol, (nm, m['rows'][i, 2], float(z[f'{nm}_crmsd']), tol)
        assert abs(m['rows'][i, 3] - float(z[f'{nm}_irmsd'])) <= tol, (nm, m['rows'][i, 3], float(z[f'{nm}_irmsd']), tol)
        assert m['ref'][nm]['flags_mask'] == 3
        assert int(m['rows'][i, 5]) == (0 if nm == '1H1V' else 2), (nm, m['rows'][i, 5])
    i = check_case(m, 'meter')
    g = np.load(os.path.join(dc.GOLDEN, 'inference_case.npz'))
    for k, key in ((0, 'm_ligand'), (1, 'm_receptor'), (2, 'm_complex')):
        assert abs(m['rows'][i, k] - float(g[key])) <= tol, (key, m['rows'][i, k], float(g[key]), tol)
    assert m['rows'][i, 1] > 0.5          # (this case has a receptor prediction of its own)


def check_edges(dev):
    m = measured(dev)
    for name in edge_cases():
        check_case(m, name)
        ref = m['ref'][name]
        assert ref['margin'] > 1e-9, (name, ref['margin'])      # the decisions cannot depend on the operation order
        assert ref['interface_pairs'] > 0, name


def check_degenerate(dev):
    m = measured(dev)
    for name in degenerate_cases():
        check_case(m, name)
    i = m['names'].index('no_pair')
    assert np.isnan(m['rows'][i, 3]) and m['rows'][i, 4] == 0 and np.isfinite(m['rows'][i, :3]).all()
    assert m['ref']['one_pair']['interface_pairs'] == 1
    i = m['names'].index('exact')
    assert (m['rows'][i, :4] <= m['bound']).all() and not np.isnan(m['rows'][i, :4]).any(), m['rows'][i]


def check_bits(dev):
    """five complexes of mixed sizes: a complex's row is bit-identical alone, first, last, in a permuted batch and from
    run to run, with the interface on and off (which leaves columns 0-2 as they are)"""
    e, g = edge_cases(), golden_cases()
    cases = [e['edge_257x1025'], g['1HCF'], e['edge_1x3'], g['1AVX'], e['edge_255x513']]
    cases = [(c[0], None, c[2], c[3]) for c in cases]
    n = len(cases)
    perm = [3, 0, 4, 2, 1]
    for interface in (True, False):
        together = run(dev, cases, interface)
        again = run(dev, cases, interface)
        permuted = run(dev, [cases[p] for p in perm], interface)
        assert together.tobytes() == again.tobytes(), 'run to run'
        for i in range(n):
            alone = run(dev, [cases[i]], interface)[0]
            rest = [cases[j] for j in range(n) if j != i]
            first, last = run(dev, [cases[i]] + rest, interface)[0], run(dev, rest + [cases[i]], interface)[-1]
            for what, row in (('alone', alone), ('first', first), ('last', last), ('permuted', permuted[perm.index(i)])):
                assert row.tobytes() == together[i].tobytes(), (interface, i, what, row, together[i])
        if interface:
            on = together
        else:
            assert on[:, :3].tobytes() == together[:, :3].tobytes(), 'columns 0-2 change with the interface'
            assert np.isnan(together[:, 3]).all() and (together[:, 4] == 0).all()


def check_rec_pred(dev):
    m = measured(dev)
    c = edge_cases()['edge_255x513']
    null, given = run(dev, [c]), run(dev, [c], explicit_rec_pred=True)
    assert null.tobytes() == given.tobytes()
    shifted = (c[0], c[3] + np.float32([0.5, -0.25, 1.0]), c[2], c[3])
    row, ref = run(dev, [shifted])[0], ref64(*shifted)
    assert row[1] > 1.0
    for k, col in enumerate(COLS):
        assert abs(row[k] - ref[col]) <= m['bound'], (col, row[k], ref[col], m['bound'])


def check_device_meter(dev):
    """DeviceMeter fed two batches (2 and 5 complexes) against the host Meter_Unbound_Bound fed the same complexes one by
    one, at the float32 path's distance"""
    m = measured(dev)
    cases = [all_cases()[n] for n in ('1AVX', 'meter', 'edge_2x2', '1H1V', 'edge_256x512', '1HCF', 'edge_1x3')]
    host, meter = INF.Meter_Unbound_Bound(), DK.DeviceMeter(interface=True)
    for c in cases:
        host.update_rmsd(c[0], c[3] if c[1] is None else c[1], c[2], c[3])
    for part in (cases[:2], cases[2:]):
        meter.update_batch([_t(c[0], dev) for c in part], [_t(c[3] if c[1] is None else c[1], dev) for c in part],
                           [_t(c[2], dev) for c in part], [_t(c[3], dev) for c in part])
    assert len(meter) == len(cases)
    tol = m['f32_distance']
    for red in ('mean', 'median'):
        dc.close(np.asarray(meter.summarize(red)), np.asarray(host.summarize(red), dtype=np.float64), tol, f'summarize({red})')
        dc.close(np.asarray(meter.summarize_with_std(red)), np.asarray(host.summarize_with_std(red), dtype=np.float64), tol,
                 f'summarize_with_std({red})')
    ir = np.asarray([ref64(*c)['interface_rmsd'] for c in cases])
    got = meter.summarize_interface('mean')
    assert not np.isnan(ir).any()
    assert abs(got[0] - ir.mean()) <= tol and abs(got[1] - ir.std()) <= tol, (got, ir)
    for fn in (meter.summarize, meter.summarize_with_std, meter.summarize_interface):
        with pytest.raises(ValueError, match='Meter_Unbound_Bound: reduction_rmsd mis specified!'):
            fn('max')
    with pytest.raises(ValueError, match='Meter_Unbound_Bound: reduction_rmsd mis specified!'):
        host.summarize('max')
    return meter


def check_validation_errors(dev):
    """refused before any launch, with a message: an empty side, decreasing offsets, a short workspace, a bad cutoff
    (the library), a tensor on the wrong device and mismatched row counts (Python)"""
    lib = DK.load_dock_library()
    lig, rec = torch.zeros(4, 3, device=dev), torch.ones(5, 3, device=dev)
    with pytest.raises(RuntimeError, match='complex 1 has 0 ligand'):
        DK.rmsd_metrics_batch([lig, lig[:0]], [lig, lig[:0]], [rec, rec])
    assert lib.eqd_dock_last_error()
    with pytest.raises(ValueError, match='complex 1: 3 predicted ligand rows for 4 true ones'):
        DK.rmsd_metrics_batch([lig, lig[:3]], [lig, lig], [rec, rec])
    with pytest.raises(ValueError, match='predicted ligands for'):
        DK.rmsd_metrics_batch([lig, lig], [lig], [rec, rec])
    wrong = torch.zeros(4, 3, device='cuda' if torch.device(dev).type == 'cpu' and torch.cuda.is_available() else 'cpu')
    if wrong.device.type != torch.device(dev).type:
        with pytest.raises(_lib.EquidockHipError, match='no CPU fallback|only takes CPU tensors'):
            DK.rmsd_metrics_batch([wrong], [wrong], [wrong])

    def offs(v):
        return np.ascontiguousarray(np.asarray(v, dtype=np.int32))

    def p(a):
        return a.ctypes.data_as(C.c_void_p)

    good_l, good_r = offs([0, 4, 8]), offs([0, 5, 10])
    wsb = lib.eqd_dock_meter_workspace_bytes(2, p(good_l), p(good_r))
    assert wsb > 0
    bad = offs([0, 6, 4])
    assert lib.eqd_dock_meter_workspace_bytes(2, p(bad), p(good_r)) == 0
    assert b'complex 1 has -2 ligand' in lib.eqd_dock_last_error()
    assert lib.eqd_dock_meter_workspace_bytes(2, p(offs([0, 4, 4])), p(good_r)) == 0
    assert lib.eqd_dock_meter_workspace_bytes(2, p(offs([1, 4, 8])), p(good_r)) == 0
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    out = torch.full((2, 8), 7.0, dtype=torch.float64, device=dev)
    l2, r2 = torch.cat([lig, lig]), torch.cat([rec, rec])
    st = DK._stream(dev)
    assert lib.eqd_dock_meter_init(2, p(bad), p(good_r), C.c_void_p(ws.data_ptr()), C.c_size_t(wsb), st) == 2
    assert lib.eqd_dock_meter_init(2, p(good_l), p(good_r), C.c_void_p(ws.data_ptr()), C.c_size_t(64), st) == 4
    assert b'workspace too small' in lib.eqd_dock_last_error()

    def ev(lo, ro, size, cutoff):
        return lib.eqd_dock_meter_eval(2, p(lo), p(ro), C.c_void_p(l2.data_ptr()), C.c_void_p(0), C.c_void_p(l2.data_ptr()),
                                       C.c_void_p(r2.data_ptr()), C.c_double(cutoff), 1, C.c_void_p(out.data_ptr()),
                                       C.c_void_p(ws.data_ptr()), C.c_size_t(size), st)

    assert ev(bad, good_r, wsb, 8.0) == 2
    assert ev(good_l, offs([0, 5, 5]), wsb, 8.0) == 2 and b'complex 1 has 4 ligand and 0 receptor' in lib.eqd_dock_last_error()
    assert ev(good_l, good_r, 64, 8.0) == 4
    for cutoff in (0.0, -1.0, float('inf'), float('nan')):
        assert ev(good_l, good_r, wsb, cutoff) == 2 and b'cutoff' in lib.eqd_dock_last_error()
    # nothing was written by the refused calls
    assert bool((out.cpu() == 7.0).all()) and bool((ws.cpu() == 0).all())


# ---- TrainStep(meter=...) -------------------------------------------------------------------------------------------
TRAIN_SIZES = ((41, 57), (66, 38), (120, 90), (23, 75))      # the 4-pair ragged batch of parity_common.check_train_step_forms


def check_train_step_meter(dev):
    """TrainStep with and without a meter: same loss and flat-gradient bits (host-enqueued and, on the GPU, after capture
    over two replays); the meter's rows are rmsd_metrics_batch on the step's ligand output, bit for bit; 2 x B rows after
    two steps"""
    from equidock_public_amd import train_step as TS
    from equidock_public_amd import build as B
    from tests import parity_common as pc
    B.build_host(verbose=False)                    # the exact transport solver of the step
    gpu = torch.device(dev).type == 'cuda'
    args = pc.port.default_args(iegmn_n_lays=2 if gpu else 1, skip_weight_h=0.75)      # (the simulator is slow)
    sd = pc.port.init_state_dict(args, seed=17, rot_scale=40.0)
    g, lig_t, rec_t, pl, pr = pc.training_batch(TRAIN_SIZES, 17, dev)
    B = len(TRAIN_SIZES)

    def steps(meter):
        net = pc.build_model(args, sd, dev)
        ts = TS.TrainStep(net, g, torch.cat(lig_t), torch.cat(rec_t), pl, pr, w_ot=pc.TRAIN_W_OT, w_int=pc.TRAIN_W_INT,
                          sigma=pc.TRAIN_SIGMA, surface_ct=pc.TRAIN_SURFACE_CT, meter=meter)
        got = []
        forms = [ts.step_unfused] + ([ts.capture().step] if gpu else [])
        for fn in forms:
            for _ in range(2):
                loss = fn()
                pc.sync(dev)
                got.append((loss.detach().cpu().numpy().tobytes(), ts.reducer.flat.detach().cpu().numpy().tobytes()))
        return net, got

    _, plain = steps(None)
    meter = DK.DeviceMeter()
    net, metered = steps(meter)
    assert plain == metered, 'the meter changes the loss or the gradient bits'
    rows = meter.rows()
    assert rows.shape == (len(metered) * B, 8), rows.shape
    with torch.no_grad():
        lig = net.forward_batched(g)[0]
    lo = np.concatenate([[0], np.cumsum([s[0] for s in TRAIN_SIZES])])
    want = DK.rmsd_metrics_batch([lig[lo[i]:lo[i + 1]] for i in range(B)], [t.to(dev) for t in lig_t],
                                 [t.to(dev) for t in rec_t], interface=False)['metrics'].cpu().numpy()
    for k in range(len(metered)):
        assert rows[k * B:(k + 1) * B].tobytes() == want.tobytes(), (k, rows[k * B:(k + 1) * B], want)
    assert (want[:, 0] > 0).all() and (want[:, 1] == 0).all() and (want[:, 2] > 0).all()


# ---- dock_complexes(ground_truth=...) -------------------------------------------------------------------------------
def check_dock_complexes_ground_truth(dev, names, max_it, check_every):
    """the fixture complexes through the seeded net with the input ligand as its own ground truth: crmsd / irmsd are
    inference.complex_and_interface_rmsd on the C-alpha rows of the returned ligand_atoms (at the float32 path's
    distance), and rotation, translation and ligand_atoms keep the bits of a call without ground truth"""
    from equidock_public_amd import featurize as FZ
    tol = measured(dev)['f32_distance']
    net, _, _ = dc.seeded_net(dev)
    residues = [dc.fixture_residues(n) for n in names]
    kw = dict(remove_clashes=True, max_it=max_it, check_every=check_every, device=dev)
    plain = DK.dock_complexes(net, residues, **kw)
    res = DK.dock_complexes(net, residues, ground_truth=[lig for lig, _ in residues], **kw)
    for name, (lig_res, rec_res), r, q in zip(names, residues, res, plain):
        assert set(r) - set(q) == {'crmsd', 'irmsd', 'ligand_rmsd', 'interface_pairs'}, set(r) ^ set(q)
        assert set(r['batch_seconds']) - set(q['batch_seconds']) == {'metrics'}
        assert r['rotation'].tobytes() == q['rotation'].tobytes() and r['translation'].tobytes() == q['translation'].tobytes()
        assert torch.equal(r['ligand_atoms'], q['ligand_atoms']) and r['clash_iterations'] == q['clash_iterations']
        li, ri = DK._ca_index(lig_res), DK._ca_index(rec_res)
        lig_all, rec_all = FZ.atoms_ragged(lig_res)[0], FZ.atoms_ragged(rec_res)[0]
        assert len(li) == len(lig_res) or len(li) > 0
        c, i = INF.complex_and_interface_rmsd(r['ligand_atoms'].cpu().numpy()[li], rec_all[ri], lig_all[li], rec_all[ri])
        assert isinstance(r['crmsd'], float) and abs(r['crmsd'] - float(c)) <= tol, (name, r['crmsd'], c, tol)
        assert abs(r['irmsd'] - float(i)) <= tol, (name, r['irmsd'], i, tol)
        d = np.sqrt(((lig_all[li].astype(np.float64)[:, None] - rec_all[ri].astype(np.float64)[None]) ** 2).sum(-1))
        assert r['interface_pairs'] == int((d < CUTOFF).sum()) > 0
        assert r['ligand_rmsd'] > 0
    with pytest.raises(ValueError, match='complex 1: the ligand has'):
        DK.dock_complexes(net, residues[:2], ground_truth=[residues[0][0], residues[1][0][:-1]], **kw)
    return res
