"""The surface function G(x) = -sigma log(1e-3 + sum_k exp(-|x - c_k|^2 / sigma)) in float64, and single-step checks of the
three kernel families built on it, at the shapes where their tiling changes:

  k_dock_eval / _grad / _step   (csrc_dock/eqd_dock_clash.hip)   256-row tiles x 512-partner chunks
  k_clash_lig / _rec / _grad / _step (csrc/eqd_data_kernels.hip) 256-row blocks, partners staged 1 024 at a time
  k_pair_losses_fwd / _bwd      (csrc/eqd_loss_kernels.hip)      256-row sweeps, partners staged 1 024 at a time

Shared by tests/test_surface_sim.py (the x86 simulator builds) and tests/test_surface_gpu.py.  The loss is
oracle/loss_port.body_intersection_loss (pinned to the reference's compute_body_intersection_loss) on float64 tensors,
gradients come from float64 autograd.  Errors are measured against per-row absolute-contribution scales, not against a
tensor maximum: a ligand row's scale is sum_k 2 e_ik |a_i - b_k| (w_i + w_k), e_ik = exp(-|a_i - b_k|^2 / sigma),
w = [ct - G >= 0] / (n (1e-3 + S)); an angle's scale weights it with the row's lever arm |d a_i / d euler_j|.

Every case asserts its own coverage from the float64 reference: each row tile of the kernel under test holds an active
row (ct - G > 0), each partner chunk a partner whose Gaussian term to some active row exceeds 1e-3, no row sits within
MARGIN of the relu's kink (where an fp32 evaluation may legitimately take the other branch), and a clash case's loss is
on the intended side of the step-size switch at 2."""
import ctypes as C
import os

import numpy as np
import torch

from equidock_public_amd import inference as INF
from oracle import loss_port as lp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

CENTRE = np.array([83.0, 72.0, 243.0])  # PDB frames are not centred (1DE4's receptor centroid)
MARGIN = 1e-3                           # smallest |ct - G| allowed for any row
PARTNER_MIN = 1e-3                      # a partner "counts" for a chunk when e_ik to an active row exceeds this
ULPS_SEEN = 1000                        # eta |g| must exceed this many ulps of the state component it moves

# Bounds on |kernel - float64| / scale, 5 - 10 x the worst of the simulator and the MI355X.  From
# zero angles R is the identity in fp32 too, so the moved ligand is exact and only exp / log / the sums round; from
# non-zero angles the fp32 rotation of atoms 250 A from the origin moves them by ~1e-5 A against partner distances of
# a few A.
TOL_CLASH_LOSS = {'exact': 2e-6, 'rotated': 5e-5}       # measured 2.6e-7, 9.8e-6
TOL_CLASH_GRAD = {'exact': 1e-7, 'rotated': 1e-4}       # measured 1.2e-8, 1.9e-5
TOL_PAIR_FWD = 5e-6                                     # measured 5.9e-7
TOL_PAIR_BWD = 5e-6                                     # measured 5.0e-7

ETA = {'high': np.float32(1e-3), 'low': np.float32(1e-4), 'late': np.float32(1e-2)}

# start states: (euler, it); `it` = 1501 selects eta = 1e-2 whatever the loss
STATES = {'zero': ((0.0, 0.0, 0.0), 0),
          'angles': ((0.3, -1.1, 0.7), 1501),
          'pitch90': ((-0.4, 2.2, 1.5607), 1501)}


# ---- float64 reference --------------------------------------------------------------------------------------------
def rot_mat(euler):
    """src/inference_rigid.py:46-73 restated: R = RZ(yaw) RY(pitch) RX(roll) for euler = (roll, yaw, pitch)."""
    roll, yaw, pitch = euler[0], euler[1], euler[2]
    o, z = torch.ones_like(roll), torch.zeros_like(roll)
    cr, sr, cy, sy, cp, sp = torch.cos(roll), torch.sin(roll), torch.cos(yaw), torch.sin(yaw), torch.cos(pitch), torch.sin(pitch)
    RX = torch.stack([o, z, z, z, cr, -sr, z, sr, cr]).reshape(3, 3)
    RY = torch.stack([cp, z, sp, z, o, z, -sp, z, cp]).reshape(3, 3)
    RZ = torch.stack([cy, -sy, z, sy, cy, z, z, z, o]).reshape(3, 3)
    return RZ @ RY @ RX


def _surface_terms(a, b, sigma, ct):
    """Detached float64 pieces of the loss at moved ligand atoms a [n, 3] and receptor atoms b [m, 3]."""
    d = a[:, None, :] - b[None, :, :]
    dist = d.norm(dim=2)
    E = torch.exp(-(dist * dist) / sigma)
    S_l, S_r = E.sum(1), E.sum(0)
    r_l = ct + sigma * torch.log(1e-3 + S_l)
    r_r = ct + sigma * torch.log(1e-3 + S_r)
    w_l = (r_l >= 0).double() / (a.shape[0] * (1e-3 + S_l))
    w_r = (r_r >= 0).double() / (b.shape[0] * (1e-3 + S_r))
    contrib = 2 * E * dist * (w_l[:, None] + w_r[None, :])     # |d loss / d a_i| <= sum_k contrib_ik
    return dict(E=E, r_lig=r_l, r_rec=r_r, row_scale=contrib.sum(1))


def clash_reference(lig0, rec, euler, trans, sigma, ct):
    """One evaluation of the clash-removal loss at the state (euler, trans) for the float32 inputs the kernel gets:
    loss, d loss / d (trans, euler), their scales, and what the coverage checks need."""
    p = torch.as_tensor(np.asarray(lig0, dtype=np.float32)).double()
    b = torch.as_tensor(np.asarray(rec, dtype=np.float32)).double()
    e = torch.tensor(np.asarray(euler, dtype=np.float32), dtype=torch.float64, requires_grad=True)
    t = torch.tensor(np.asarray(trans, dtype=np.float32), dtype=torch.float64, requires_grad=True)
    a = p @ rot_mat(e).t() + t
    loss = lp.body_intersection_loss(a, b, sigma, ct)
    loss.backward()
    loss = float(loss.detach())
    ref = _surface_terms(a.detach(), b, sigma, ct)
    J = torch.autograd.functional.jacobian(rot_mat, e.detach())                 # [3, 3, 3]: d R / d euler_j
    lever = torch.einsum('xyj,iy->ijx', J, p).norm(dim=2)                       # [n, 3]: |d a_i / d euler_j|
    s = ref['row_scale']
    ref.update(loss=loss, grad=np.concatenate([t.grad.numpy(), e.grad.numpy()]),
               scale_loss=loss,                          # a sum of non-negative row terms
               scale_grad=np.concatenate([np.full(3, float(s.sum())), (s[:, None] * lever).sum(0).numpy()]))
    return ref


def pair_reference(preds, tgts, recs, sigma, ct, wm, wi):
    """Per-pair (mse, inter) and d (sum_p wm_p mse_p + wi_p inter_p) / d lig_pred in float64, with per-row scales."""
    leaves = [torch.as_tensor(np.asarray(a, dtype=np.float32)).double().requires_grad_(True) for a in preds]
    T = [torch.as_tensor(np.asarray(x, dtype=np.float32)).double() for x in tgts]
    R = [torch.as_tensor(np.asarray(x, dtype=np.float32)).double() for x in recs]
    mse, inter = lp.pair_losses(leaves, T, R, sigma, ct)
    ((mse * torch.tensor(wm, dtype=torch.float64)).sum() + (inter * torch.tensor(wi, dtype=torch.float64)).sum()).backward()
    mse, inter = mse.detach(), inter.detach()
    out = []
    for p, (a, t, b) in enumerate(zip(leaves, T, R)):
        ref = _surface_terms(a.detach(), b, sigma, ct)
        n = a.shape[0]
        mse_part = 2 * (a.detach() - t).norm(dim=1) / (3 * n)
        ref.update(mse=float(mse[p]), inter=float(inter[p]), grad=a.grad.numpy(),
                   row_scale_grad=(abs(wi[p]) * ref['row_scale'] + abs(wm[p]) * mse_part).numpy())
        out.append(ref)
    return out


def coverage_problems(ref, rows, chunk, what):
    """What makes a case vacuous for a kernel with `rows`-row tiles and `chunk`-partner chunks, on both sides."""
    E, act_l, act_r = ref['E'], ref['r_lig'] > 0, ref['r_rec'] > 0
    n, m = E.shape
    bad = []
    for side, act in (('ligand', act_l), ('receptor', act_r)):
        for t0 in range(0, act.shape[0], rows):
            if not bool(act[t0:t0 + rows].any()):
                bad.append(f'{what}: {side} rows {t0}..{min(t0 + rows, act.shape[0]) - 1} hold no active row')
    to_l = E[act_l].amax(0) if bool(act_l.any()) else torch.zeros(m, dtype=E.dtype)    # receptor partners of ligand rows
    to_r = E[:, act_r].amax(1) if bool(act_r.any()) else torch.zeros(n, dtype=E.dtype)  # ligand partners of receptor rows
    for side, best in (('receptor', to_l), ('ligand', to_r)):
        for c0 in range(0, best.shape[0], chunk):
            if not bool((best[c0:c0 + chunk] > PARTNER_MIN).any()):
                bad.append(f'{what}: {side} partners {c0}..{min(c0 + chunk, best.shape[0]) - 1} add nothing to an active row')
    kink = float(torch.cat([ref['r_lig'].abs(), ref['r_rec'].abs()]).min())
    if kink < MARGIN:
        bad.append(f'{what}: a row sits {kink:.1e} from the relu kink')
    return bad


# ---- geometry -----------------------------------------------------------------------------------------------------
def clouds(n_lig, n_rec, seed, sigma, ct, target, rows=256, chunk=512):
    """Seeded interpenetrating ligand and receptor clouds (float64 [n, 3], world frame, around CENTRE): two balls of
    0.01 atoms / A^3 whose centres are moved apart until the loss is about 4 (target 'high') or 1 ('low'); then every
    `rows`-row tile without an active row and every `chunk`-partner chunk without a contributing partner gets one atom
    moved 0.5 - 2 A from an atom of the other side, and atoms within MARGIN of the kink are nudged."""
    rng = np.random.default_rng(seed)

    def ball(n):
        radius = max(2.0, (3 * n / (4 * np.pi * 0.01)) ** (1 / 3))
        u = rng.normal(size=(n, 3))
        return u / np.linalg.norm(u, axis=1, keepdims=True) * radius * rng.uniform(size=(n, 1)) ** (1 / 3)
    A0, B0 = ball(n_lig), ball(n_rec)
    axis = np.array([0.8, 0.5, -0.33]) / np.linalg.norm([0.8, 0.5, -0.33])

    def place(D):
        return CENTRE + A0 + 0.5 * D * axis, CENTRE + B0 - 0.5 * D * axis

    def terms(A, B):
        return _surface_terms(torch.from_numpy(A), torch.from_numpy(B), sigma, ct)

    def loss_of(ref):
        return float(ref['r_lig'].clamp(min=0).mean() + ref['r_rec'].clamp(min=0).mean())
    want = {'high': 4.0, 'low': 1.0}[target]
    lo, hi = 0.0, 2.0 * (np.abs(A0).max() + np.abs(B0).max()) + 10.0
    for _ in range(30):
        D = 0.5 * (lo + hi)
        if loss_of(terms(*place(D))) > want:
            lo = D
        else:
            hi = D
    A, B = place(D)

    def near(X, i, Y, j):
        v = rng.normal(size=3)
        X[i] = Y[j] + v / np.linalg.norm(v) * rng.uniform(0.5, 2.0)
    for _ in range(20):
        ref = terms(A, B)
        act_l, act_r = (ref['r_lig'] > 0).numpy(), (ref['r_rec'] > 0).numpy()
        moved = False
        for X, Y, act in ((A, B, act_l), (B, A, act_r)):
            for t0 in range(0, len(X), rows):
                if not act[t0:t0 + rows].any():
                    near(X, rng.integers(t0, min(t0 + rows, len(X))), Y, rng.integers(len(Y)))
                    moved = True
        if moved:
            continue
        E = ref['E'].numpy()
        for X, Y, best, act_y in ((B, A, E[act_l].max(0), act_l), (A, B, E[:, act_r].max(1), act_r)):
            for c0 in range(0, len(X), chunk):
                if not (best[c0:c0 + chunk] > PARTNER_MIN).any():
                    near(X, rng.integers(c0, min(c0 + chunk, len(X))), Y, rng.choice(np.flatnonzero(act_y)))
                    moved = True
        if moved:
            continue
        for X, r in ((A, ref['r_lig'].numpy()), (B, ref['r_rec'].numpy())):
            for i in np.flatnonzero(np.abs(r) < 5 * MARGIN):
                X[i] += rng.normal(size=3) * 0.05
                moved = True
        if not moved:
            return A, B
    raise AssertionError(f'clouds({n_lig}, {n_rec}, seed={seed}): coverage not reached')


# ---- one exact step of the clash kernels ------------------------------------------------------------------------
# (n_lig, n_rec, loss side of 2) around each kernel's tile and chunk edges; a side of one atom, or of fewer atoms than
# it has tiles to cover on the other side, forces a deep overlap ('high')
DOCK_SHAPES = [(1, 1, 'high'), (1, 513, 'high'), (257, 1, 'high'), (255, 511, 'low'), (256, 512, 'high'),
               (257, 513, 'low'), (511, 1025, 'high'), (513, 1024, 'low'), (1025, 2049, 'high')]
SINGLE_SHAPES = [(1, 1, 'high'), (256, 1024, 'high'), (257, 1025, 'low'), (1023, 1, 'high'), (1025, 1023, 'high'),
                 (2049, 1025, 'low')]


def _state_bytes(states):
    host = (INF.EqdClashState * len(states))()
    for h, (euler, it) in zip(host, states):
        h.euler[:] = [float(np.float32(v)) for v in euler]
        h.trans[:] = [0.0, 0.0, 0.0]
        h.it, h.done, h.loss = it, 0, 0.0
    return torch.frombuffer(bytearray(host), dtype=torch.uint8)


def _read_states(t, n):
    return (INF.EqdClashState * n).from_buffer_copy(t.cpu().numpy().tobytes())


def _fields(s):
    return (tuple(np.float32(v).tobytes() for v in s.euler), tuple(np.float32(v).tobytes() for v in s.trans),
            np.float32(s.loss).tobytes(), s.it)


def make_clash_case(n_lig, n_rec, target, state, seed, sigma=8.0, ct=8.0, rows=256, chunk=512):
    """One case: the world clouds of `target` loss, the ligand given in the frame that R(euler) of the start state
    maps onto them (translation 0: the offset lives in the coordinates)."""
    euler, it = STATES[state]
    A, B = clouds(n_lig, n_rec, seed, sigma, ct, target, rows, chunk)
    R = rot_mat(torch.tensor(np.asarray(euler, dtype=np.float32), dtype=torch.float64)).numpy()
    lig0 = (A @ R).astype(np.float32)                           # R^T a_i, row-wise
    return dict(lig0=lig0, rec=B.astype(np.float32), euler=euler, it=it, target=target, sigma=sigma, ct=ct,
                what=f'({n_lig}, {n_rec}) {state}')


def clash_cases(shapes, states, rows, chunk):
    """Every (shape, start state) case, each with clouds of its own seed."""
    return [make_clash_case(nl, nr, target, state, seed=1000 * k + 7 * j, rows=rows, chunk=chunk)
            for k, (nl, nr, target) in enumerate(shapes) for j, state in enumerate(states)]


def check_step(case, before, after, rows, chunk):
    """The kernel's loss and the gradient recovered from its update against float64; returns the worst error / scale
    of the loss and of the gradient."""
    what = case['what']
    ref = clash_reference(case['lig0'], case['rec'], before[0], before[1], case['sigma'], case['ct'])
    bad = coverage_problems(ref, rows, chunk, what)
    assert not bad, bad
    loss64 = ref['loss']
    assert (loss64 >= 2.1) if case['target'] == 'high' else (loss64 <= 1.9), (what, loss64, case['target'])
    eta = ETA['late'] if case['it'] > 1500 else ETA[case['target']]
    s0 = np.concatenate([np.float32(before[1]), np.float32(before[0])]).astype(np.float64)
    s1 = np.concatenate([np.float32(after[1]), np.float32(after[0])]).astype(np.float64)
    g = (s0 - s1) / float(eta)
    g64 = ref['grad']
    ulp = np.spacing(np.maximum(np.abs(s0), np.abs(s1)).astype(np.float32)).astype(np.float64)
    seen = float(eta) * np.abs(g64) / ulp
    assert (seen >= ULPS_SEEN).all(), (what, 'eta |g| spans too few ulps of the state', seen)
    quant = ulp / float(eta) + 2.0 ** -23 * np.abs(g64)       # the state's rounding, not the kernel's arithmetic
    e_loss = abs(after[2] - loss64) / ref['scale_loss']
    e_grad = float((np.maximum(np.abs(g - g64) - quant, 0.0) / ref['scale_grad']).max())
    kind = 'exact' if not any(before[0]) else 'rotated'
    assert e_loss <= TOL_CLASH_LOSS[kind], f'{what}: loss {after[2]!r} vs float64 {loss64!r} ({e_loss:.2e} of the scale)'
    assert e_grad <= TOL_CLASH_GRAD[kind], (f'{what}: gradient {g} vs float64 {g64}: {e_grad:.2e} of the scale '
                                            f'{ref["scale_grad"]}')
    return e_loss, e_grad


def dock_steps(dev, cases, rows=256, chunk=512):
    """One exact iteration of eqd_dock_clash_iterations for the cases as ONE batch, compared with float64; then a second
    iteration only raises `done` (n_done = C) and a third changes nothing.  Returns the worst (loss, gradient) errors."""
    from equidock_public_amd import dock as DK
    lib = DK.load_dock_library()
    n = len(cases)
    lo = DK._offsets([c['lig0'].shape[0] for c in cases])
    ro = DK._offsets([c['rec'].shape[0] for c in cases])
    lop, rop = lo.ctypes.data_as(C.c_void_p), ro.ctypes.data_as(C.c_void_p)
    caps = np.ascontiguousarray(np.asarray([c['it'] + 1 for c in cases], dtype=np.int32))
    lig = torch.from_numpy(np.concatenate([c['lig0'] for c in cases])).to(dev)
    rec = torch.from_numpy(np.concatenate([c['rec'] for c in cases])).to(dev)
    wsb = lib.eqd_dock_clash_workspace_bytes(n, lop, rop)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    states = torch.empty(n * C.sizeof(INF.EqdClashState), dtype=torch.uint8, device=dev)
    n_done = torch.empty(1, dtype=torch.int32, device=dev)
    st = DK._stream(dev)
    DK.check(lib.eqd_dock_clash_init(n, lop, rop, caps.ctypes.data_as(C.c_void_p), C.c_void_p(states.data_ptr()),
                                     C.c_void_p(n_done.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_size_t(wsb), st))
    states.copy_(_state_bytes([(c['euler'], c['it']) for c in cases]).to(dev))
    sig, ct = cases[0]['sigma'], cases[0]['ct']
    assert all(c['sigma'] == sig and c['ct'] == ct for c in cases)

    def iterate():
        DK.check(lib.eqd_dock_clash_iterations(1, n, lop, rop, C.c_void_p(lig.data_ptr()), C.c_void_p(rec.data_ptr()),
                                               C.c_float(sig), C.c_float(ct), C.c_float(-1.0),
                                               C.c_void_p(states.data_ptr()), C.c_void_p(n_done.data_ptr()),
                                               C.c_void_p(ws.data_ptr()), C.c_size_t(wsb), st))
        return _read_states(states, n), int(n_done.cpu()[0])
    s1, d1 = iterate()
    assert d1 == 0, d1
    worst = [0.0, 0.0]
    for c, s in zip(cases, s1):
        assert s.it == c['it'] + 1 and s.done == 0, (c['what'], s.it, s.done)
        errs = check_step(c, (c['euler'], (0.0, 0.0, 0.0)), (tuple(s.euler), tuple(s.trans), s.loss), rows, chunk)
        worst = [max(w, e) for w, e in zip(worst, errs)]
    s2, d2 = iterate()
    assert d2 == n, (d2, n)
    for c, a, b in zip(cases, s1, s2):
        assert _fields(a) == _fields(b) and b.done == 1, (c['what'], 'second iteration changed the state')
    s3, d3 = iterate()
    assert d3 == n and all(_fields(a) == _fields(b) and b.done == 1 for a, b in zip(s2, s3)), 'third iteration'
    return worst


def single_step(dev, case, rows=256, chunk=1024):
    """The same for eqd_clash_iterations (one complex; no completion counter)."""
    from equidock_public_amd import _lib
    lib = _lib.load_library()
    lig = torch.from_numpy(case['lig0']).to(dev)
    rec = torch.from_numpy(case['rec']).to(dev)
    n, m = lig.shape[0], rec.shape[0]
    wsb = lib.eqd_clash_workspace_bytes(n, m)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    state = _state_bytes([(case['euler'], case['it'])]).to(dev)
    st = _lib.stream_ptr(dev)

    def iterate():
        _lib.check(lib.eqd_clash_iterations(1, n, m, _lib.ptr(lig), _lib.ptr(rec), C.c_float(case['sigma']),
                                            C.c_float(case['ct']), C.c_float(-1.0), int(case['it'] + 1), _lib.ptr(state),
                                            _lib.ptr(ws), C.c_size_t(wsb), st))
        return _read_states(state, 1)[0]
    s1 = iterate()
    assert s1.it == case['it'] + 1 and s1.done == 0, (case['what'], s1.it, s1.done)
    errs = check_step(case, (case['euler'], (0.0, 0.0, 0.0)), (tuple(s1.euler), tuple(s1.trans), s1.loss), rows, chunk)
    s2 = iterate()
    assert _fields(s1) == _fields(s2) and s2.done == 1, (case['what'], 'second iteration changed the state')
    s3 = iterate()
    assert _fields(s2) == _fields(s3) and s3.done == 1, (case['what'], 'third iteration changed the state')
    return errs


# ---- pair losses at chunk edges ---------------------------------------------------------------------------------
PAIR_SIZES = [(1, 1), (1025, 7), (7, 1025), (1024, 1024), (1023, 2049), (2049, 300)]


def pair_batch(dev, sizes=PAIR_SIZES):
    from equidock_public_amd import graph as G, synthetic
    return G.batch_pairs(synthetic.make_pairs(sizes, 4)).to(dev)      # only the segmentation of the batch is used


def pair_losses_at_edges(dev, g, sizes, sigma, ct, seed=21):
    """losses.pair_losses on one ragged batch against float64: per pair mse / inter against their own values, every row
    of d lig_pred against its own scale.  Returns the worst (forward, backward) errors."""
    from equidock_public_amd import losses
    preds, tgts, recs = [], [], []
    rng = np.random.default_rng(seed)
    for p, (nl, nr) in enumerate(sizes):
        A, B = clouds(nl, nr, seed + p, sigma, ct, 'high', rows=256, chunk=1024)
        preds.append(A.astype(np.float32))
        tgts.append((A + rng.normal(size=A.shape)).astype(np.float32))
        recs.append(B.astype(np.float32))
    wm = [1.0 + 0.37 * p for p in range(len(sizes))]               # distinct pair weights
    wi = [1.3 - 0.21 * p for p in range(len(sizes))]
    refs = pair_reference(preds, tgts, recs, sigma, ct, wm, wi)
    for (nl, nr), ref in zip(sizes, refs):
        bad = coverage_problems(ref, 256, 1024, f'pair ({nl}, {nr}) sigma {sigma}')
        assert not bad, bad
    pd = torch.from_numpy(np.concatenate(preds)).to(dev).requires_grad_(True)
    mse, inter = losses.pair_losses(g, pd, torch.from_numpy(np.concatenate(tgts)).to(dev),
                                    torch.from_numpy(np.concatenate(recs)).to(dev), sigma, ct)
    ((mse * torch.tensor(wm, device=dev)).sum() + (inter * torch.tensor(wi, device=dev)).sum()).backward()
    mse, inter, grad = mse.detach().cpu().double(), inter.detach().cpu().double(), pd.grad.cpu().double().numpy()
    e_fwd = e_bwd = 0.0
    off = 0
    for p, ((nl, nr), ref) in enumerate(zip(sizes, refs)):
        what = f'pair {p} ({nl}, {nr}) sigma {sigma}'
        for name, got, want in (('mse', float(mse[p]), ref['mse']), ('inter', float(inter[p]), ref['inter'])):
            e = abs(got - want) / want
            assert e <= TOL_PAIR_FWD, f'{what}: {name} {got!r} vs float64 {want!r} ({e:.2e})'
            e_fwd = max(e_fwd, e)
        rows = np.abs(grad[off:off + nl] - ref['grad']).max(1) / ref['row_scale_grad']
        i = int(rows.argmax())
        assert rows[i] <= TOL_PAIR_BWD, (f'{what}: d lig_pred row {i} {grad[off + i]} vs float64 {ref["grad"][i]} '
                                         f'({rows[i]:.2e} of the row scale {ref["row_scale_grad"][i]:.3e})')
        e_bwd = max(e_bwd, float(rows[i]))
        off += nl
    return e_fwd, e_bwd
