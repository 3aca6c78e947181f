"""The keypoint / Kabsch head in float64, and operator checks of the kernels that compute it:

  k_kabsch_fwd / _bwd            (csrc/eqd_head_kernels.hip)   one wave per pair, lane t holds keypoints t and t + 64
  k_keypoint* / k_head_u*        (csrc/eqd_head_kernels.hip)   K-head attention pooling, one-head backward past 64 heads
  the rigid apply fused into k_kabsch_fwd / _bwd                ligand rows at a stride of 64 lanes

Shared by tests/test_head_sim.py (the x86 simulator build) and tests/test_head_gpu.py.  Kabsch is
oracle/iegmn_port.kabsch (pinned to the reference's rigid_docking_model.py:563-589) on float64 tensors; its guard draws
are the exact [B, 10, 3] diagonals the kernel receives through `svd_draws`, gradients come from float64 autograd through
torch.linalg.svd.  Errors are measured per quantity: T absolutely (it is orthonormal), b against |mean_r| + |mean_l|
(keypoints sit up to ~300 A from the origin, as in PDB frames), dY against the pair's largest |dY|.

Every Kabsch case asserts its own coverage from the float64 reference: at every guard decision the smallest singular
value and the smallest |S_i^2 - S_j^2| sit outside [1/2, 2] x their thresholds (1e-3, 1e-2) and more than
DECISION_ULPS fp32 ulps of S_0 away from them, so that an fp32 evaluation cannot take the other branch; S_2 / S_0 is
large enough that the sign of det A cannot flip; the decomposed A's singular values are min |S_i - S_j| / S_0 >=
GAP_FLOOR apart (float64 autograd of the SVD stays well conditioned); and each batch holds both det signs and the guard
iteration counts it was built for."""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

from equidock_public_amd import _lib as L
from oracle import iegmn_port as port

CENTRE = np.array([83.0, 72.0, 243.0])  # PDB frames are not centred (1DE4's receptor centroid)
S_MIN, GAP_MIN = 1e-3, 1e-2             # the reference's guard thresholds (rigid_docking_model.py:574)
DECISION_FACTOR = 2.0                   # a decision value lies below threshold / 2 or above 2 x threshold ...
DECISION_ULPS = 32                      # ... and further than this many fp32 ulps of S_0 (of S_0^2 for the gap) from it
DET_REL = 2e-4                          # S_2 / S_0 at least this: |det A| well away from 0 next to the fp32 error of A
GAP_FLOOR = 1e-3                        # gradient cases: min_{i != j} |S_i - S_j| / S_0 at least this
NEAR = (1.2 * GAP_FLOOR, 2.5 * GAP_FLOOR)   # the near-degenerate but legal group: smallest relative gap in this range

# Bounds, 5 - 10 x the worst of the simulator and the MI355X.  'near' holds the pairs whose two
# closest singular values are 1.2 - 2.5e-3 of S_0 apart: with det A < 0, T = U diag(1, 1, -1) V^T and the backward's
# denominator S_1 - S_2 are conditioned by that gap, so the fp32 SVD's rounding is amplified by ~1 / gap.
TOL_T = {'well': 3e-6, 'near': 4e-4, 'guard': 5e-6}        # measured 4.4e-7, 5.8e-5, 6.9e-7
TOL_B = {'well': 1e-6, 'near': 1e-4, 'guard': 1e-6}        # measured 1.6e-7, 1.7e-5, 1.5e-7
TOL_DY = {'well': 5e-6, 'near': 1.5e-3, 'guard': 1.5e-5}   # measured 7.8e-7, 2.2e-4, 1.9e-6
TOL_A = 5e-7                # A_out vs float64, of S_0; measured 8.8e-8
TOL_ORTH = 5e-6             # |T T^T - I|, and |det T - 1| <= 3 x this; measured 6.7e-7
TOL_PLANAR = 2e-6           # status 11 with planar keypoints: |T T^T - I|, |T v_j - u_j|; measured 2.3e-7
TOL_KP = 1e-6               # keypoints, of the segment's largest |z|; measured 1.5e-7
TOL_KP_GRAD = 5e-5          # keypoint gradients, of their scales (check_keypoint_pool); measured 6.5e-6
TOL_APPLY = 1e-6            # the fused apply's forward, of |x0| |T| + |b| per row; measured 1.2e-7
TOL_APPLY_BWD = 5e-6        # its backward (head backward from d_lig vs from dT / db), of each tensor's largest; measured 6.4e-7

# ---- float64 Kabsch ---------------------------------------------------------------------------------------------


def _f64(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float32)).double()


def kabsch_reference(yl, yr, draws=None, dT=None, db=None):
    """oracle/iegmn_port.kabsch on float64 copies of the float32 keypoints the kernel gets, its guard fed the kernel's
    diagonal draws [10, 3].  Returns T, b, A (the decomposed, guarded A), it (guard iterations), S (the singular values
    of every SVD taken, in order), and with dT / db the float64 autograd gradients d(<T, dT> + <b, db>) / d Yl, Yr."""
    Yl, Yr = _f64(yl).requires_grad_(True), _f64(yr).requires_grad_(True)
    d = None if draws is None else _f64(draws)
    status = []
    # (an 11th decision ends the reference: port.kabsch raises, as the reference exits; the kernel reports status 11)
    T, b, A = port.kabsch(Yr, Yl, None if d is None else (lambda it: torch.diag(d[min(it, 9)] * (it < 10))), status)
    it = status[0]
    assert d is not None or it == 0, 'the guard fired without explicit draws'
    An = ((Yr - Yr.mean(0)).t() @ (Yl - Yl.mean(0))).detach()
    S = [torch.linalg.svdvals(An)]
    for n in range(it):                                   # the same sequence of A the oracle decomposed
        An = An + torch.diag(d[n])
        S.append(torch.linalg.svdvals(An))
    out = dict(T=T.detach().numpy(), b=b.detach().view(3).numpy(), A=A.detach().numpy(), it=it,
               S=[s.numpy() for s in S], det=float(torch.det(A.detach())),
               scale_b=float(Yr.detach().mean(0).norm() + Yl.detach().mean(0).norm()))
    if dT is not None:
        ((T * _f64(dT)).sum() + (b.view(3) * _f64(db)).sum()).backward()
        out.update(dYl=Yl.grad.numpy(), dYr=Yr.grad.numpy())
    return out


def _clear(x, th, err):
    """'low' / 'high' when x is clearly on one side of th, None when an fp32 evaluation might see the other side."""
    if x <= th / DECISION_FACTOR and th - x >= err:
        return 'low'
    if x >= th * DECISION_FACTOR and x - th >= err:
        return 'high'
    return None


def guard_problems(S_list, it):
    """What makes the guard's decisions fragile, or not the ones intended: decision n must be 'unstable' for n < it and
    'stable' at n = it (no decision after a 10th unstable one)."""
    bad = []
    for n, S in enumerate(S_list):
        S = np.sort(np.asarray(S))[::-1]
        ulp = DECISION_ULPS * 2.0 ** -24 * S[0]
        gap = min(abs(S[0] ** 2 - S[1] ** 2), abs(S[0] ** 2 - S[2] ** 2), abs(S[1] ** 2 - S[2] ** 2))
        c_min, c_gap = _clear(S[2], S_MIN, ulp), _clear(gap, GAP_MIN, 2 * S[0] * ulp)
        if 'low' in (c_min, c_gap):
            unstable = True
        elif c_min == c_gap == 'high':
            unstable = False
        else:
            bad.append(f'decision {n}: min S {S[2]:.3e} / gap {gap:.3e} too close to the thresholds (S_0 {S[0]:.3e})')
            continue
        if unstable != (n < it):
            bad.append(f'decision {n}: unstable={unstable}, intended {n < it}')
    return bad


def decomposed_problems(S, grads=True):
    """The decomposed A: the sign of det A must be unambiguous and, for gradient cases, its singular values separated."""
    S = np.sort(np.asarray(S))[::-1]
    bad = []
    if S[2] < DET_REL * S[0]:
        bad.append(f'S_2 / S_0 = {S[2] / S[0]:.1e}: the sign of det A is fragile')
    if grads and min(S[0] - S[1], S[1] - S[2]) < GAP_FLOOR * S[0]:
        bad.append(f'singular values {S} closer than {GAP_FLOOR:g} of S_0')
    return bad


def rel_gap(S):
    S = np.sort(np.asarray(S))[::-1]
    return min(S[0] - S[1], S[1] - S[2]) / S[0]


# ---- seeded Kabsch cases ------------------------------------------------------------------------------------------


def _rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    a, b, c, d = q
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])


def _offset(rng):
    v = rng.normal(size=3)
    return CENTRE * rng.uniform(0.3, 1.2) + 20.0 * v


def _shaped_cloud(rng, K, svals):
    """K centred points whose scatter matrix X^T X has eigenvalues svals (K >= 4)."""
    X = rng.normal(size=(K, 3))
    X -= X.mean(0)
    w, Q = np.linalg.eigh(X.T @ X)
    X = X @ Q @ np.diag(w ** -0.5)                      # orthonormal columns
    return X @ np.diag(np.sqrt(svals)) @ _rotation(rng).T


def full_rank_pair(rng, K, spread, sign, group):
    """Ligand keypoints of spread `spread` A around a PDB-like offset, receptor keypoints a rotated (sign = -1: reflected)
    copy of them elsewhere, plus noise: A = R M C has the scatter C's singular values.  group 'near': the two closest
    singular values NEAR of S_0 apart."""
    S0 = K * spread ** 2
    if group == 'near':
        g = rng.uniform(1.5, 2.0) * GAP_FLOOR
        r1 = rng.uniform(0.3, 0.8)
        rel = (1.0, r1, r1 - g) if rng.uniform() < 0.5 else (1.0, 1.0 - g, r1)
        noise = 0.0
    else:
        r1 = rng.uniform(0.35, 0.85)
        rel = (1.0, r1, rng.uniform(0.05, r1 - 0.2))
        noise = 0.02 * spread
    X = _shaped_cloud(rng, K, S0 * np.asarray(rel))
    M = np.diag([1.0, 1.0, float(sign)])
    yl = X + _offset(rng)
    yr = X @ (_rotation(rng) @ M).T + _offset(rng) + noise * rng.normal(size=X.shape)
    return yl.astype(np.float32), yr.astype(np.float32)


def guard_pair(rng, kind, K):
    """Keypoints on which the guard must fire: 'rank' (K <= 3: the centred A has rank K - 1), 'planar' (the ligand's
    keypoints on the plane z = 0 exactly: A has a zero column, the SVD's rank-deficient branch runs) and 'collapsed'
    (every keypoint within ~1e-3 A of one point, as when all heads attend one node)."""
    if kind == 'rank':
        yl = rng.normal(size=(K, 3)) * 1.5 + _offset(rng)
        yr = (yl - yl.mean(0)) @ _rotation(rng).T + _offset(rng) + 0.1 * rng.normal(size=(K, 3))
    elif kind == 'planar':
        X = rng.normal(size=(K, 3)) * 1.2
        X[:, 2] = 0.0
        yl = X + np.array([*_offset(rng)[:2], 0.0])
        yr = X @ _rotation(rng).T + _offset(rng) + 0.05 * rng.normal(size=(K, 3))
    else:
        c = _offset(rng)
        yl = c + 1e-3 * rng.normal(size=(K, 3))
        yr = _offset(rng) + 1e-3 * rng.normal(size=(K, 3))
    return yl.astype(np.float32), yr.astype(np.float32)


def guard_draws(rng, yl, yr, n_it, kind):
    """[10, 3] float32 draws under which the guard takes exactly n_it iterations, every decision clear (guard_problems) and
    the final A well separated: n_it - 1 draws too small to stabilise A, then one from U[0.3, 1)."""
    for _ in range(500):
        d = np.zeros((10, 3), np.float32)
        small = 3e-5 if kind != 'collapsed' else 1e-5
        d[:n_it - 1] = rng.uniform(0.0, small, size=(n_it - 1, 3))
        d[n_it - 1] = rng.uniform(0.3, 1.0, size=3)
        d[n_it:] = rng.uniform(0.0, 1.0, size=(10 - n_it, 3))
        try:
            ref = kabsch_reference(yl, yr, d)
        except RuntimeError:          # still unstable after the 10th draw
            continue
        if ref['it'] == n_it and not guard_problems(ref['S'], n_it) and not decomposed_problems(ref['S'][-1]):
            return d
    raise AssertionError(f'no clear draws for a {kind} pair with {n_it} iterations')


def kabsch_batch(K, seed, n_pairs=6):
    """A seeded batch of full-rank pairs at K keypoints: spreads 1 - 100 A, det signs alternating, the last two pairs in
    the near-degenerate group.  K <= 3 gives guard pairs instead (rank deficient, 1 .. 10 guard iterations)."""
    rng = np.random.default_rng(seed)
    pairs, groups, draws, its = [], [], [], []
    spreads = [1.0, 100.0, 3.0, 30.0, 10.0, 50.0]
    for p in range(n_pairs):
        if K <= 3:
            n_it = [1, 2, 10, 1, 5, 3][p % 6]
            yl, yr = guard_pair(rng, 'rank', K)
            d = guard_draws(rng, yl, yr, n_it, 'rank')
            groups.append('guard')
        else:
            group = 'near' if p >= n_pairs - 2 else 'well'
            for _ in range(100):
                yl, yr = full_rank_pair(rng, K, spreads[p % 6], 1 if p % 2 == 0 else -1, group)
                ref = kabsch_reference(yl, yr)
                bad = guard_problems(ref['S'], 0) + decomposed_problems(ref['S'][0])
                if group == 'near' and not NEAR[0] <= rel_gap(ref['S'][0]) <= NEAR[1]:
                    bad.append('not near-degenerate')
                if not bad:
                    break
            else:
                raise AssertionError(f'K={K} pair {p}: {bad}')
            d, n_it = np.zeros((10, 3), np.float32), 0
            groups.append(group)
        pairs.append((yl, yr))
        draws.append(d)
        its.append(n_it)
    return dict(K=K, pairs=pairs, groups=groups, draws=np.stack(draws), its=its, what=f'K={K}')


def guard_batch(kind, K, its, seed):
    """Pairs of one guard kind at K keypoints with the given iteration counts."""
    rng = np.random.default_rng(seed)
    pairs, draws = [], []
    for n_it in its:
        yl, yr = guard_pair(rng, kind, K)
        draws.append(guard_draws(rng, yl, yr, n_it, kind))
        pairs.append((yl, yr))
    return dict(K=K, pairs=pairs, groups=['guard'] * len(its), draws=np.stack(draws), its=list(its),
                what=f'{kind} K={K}')


# ---- the operators ----------------------------------------------------------------------------------------------


def _P(t):
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())


def _sync(dev):
    if torch.device(dev).type == 'cuda':
        torch.cuda.synchronize()


def kabsch_fwd(dev, Y, draws=None, seed=0):
    """eqd_kabsch_fwd on Y [2B, K, 3] (ligands first): T [B, 3, 3], b [B, 3], A_out [B, 3, 3], status [B] on the host."""
    B, K = Y.shape[0] // 2, Y.shape[1]
    Yd = torch.from_numpy(np.ascontiguousarray(Y, np.float32)).to(dev)
    dr = None if draws is None else torch.from_numpy(np.ascontiguousarray(draws, np.float32)).to(dev)
    T, b, A = (torch.full((B, n), float('nan'), device=dev) for n in (9, 3, 9))
    status = torch.full((B,), -1, dtype=torch.int32, device=dev)
    L.check(L._lib.eqd_kabsch_fwd(B, K, _P(Yd), _P(dr), int(seed), _P(T), _P(b), _P(A), _P(status), L.stream_ptr(dev)))
    _sync(dev)
    return (T.cpu().view(B, 3, 3).numpy(), b.cpu().numpy(), A.cpu().view(B, 3, 3).numpy(),
            status.cpu().numpy().tolist())


def kabsch_bwd(dev, Y, A, T, dT, db):
    """eqd_kabsch_bwd: dY [2B, K, 3] on the host.  dY starts as NaN: the header says the call overwrites it."""
    B, K = Y.shape[0] // 2, Y.shape[1]
    dd = [torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev) for x in (Y, A, T, dT, db)]
    dY = torch.full((2 * B, K, 3), float('nan'), device=dev)
    L.check(L._lib.eqd_kabsch_bwd(B, K, *[_P(x) for x in dd], _P(dY), L.stream_ptr(dev)))
    _sync(dev)
    return dY.cpu().numpy()


def _Y(batch):
    return np.concatenate([np.stack([yl for yl, _ in batch['pairs']]), np.stack([yr for _, yr in batch['pairs']])])


def check_kabsch_batch(dev, batch, seed=0):
    """eqd_kabsch_fwd / _bwd on one batch against float64, pair by pair.  Returns {quantity: worst error / scale}."""
    K, B = batch['K'], len(batch['pairs'])
    Y = _Y(batch)
    rng = np.random.default_rng(seed + 17)
    dT, db = rng.normal(size=(B, 3, 3)), rng.normal(size=(B, 3))
    T, b, A, status = kabsch_fwd(dev, Y, batch['draws'])
    dY = kabsch_bwd(dev, Y, A, T, dT, db)
    worst = {}
    signs = set()
    for p, ((yl, yr), group, n_it) in enumerate(zip(batch['pairs'], batch['groups'], batch['its'])):
        what = f"{batch['what']} pair {p} ({group}, {n_it} guard iterations)"
        ref = kabsch_reference(yl, yr, batch['draws'][p], dT[p], db[p])
        bad = guard_problems(ref['S'], n_it) + decomposed_problems(ref['S'][-1])
        assert not bad and ref['it'] == n_it, (what, bad, ref['it'])
        assert status[p] == ref['it'], f'{what}: status {status[p]} != the reference iteration count {ref["it"]}'
        S0 = float(ref['S'][-1].max())
        e = dict(T=float(np.abs(T[p] - ref['T']).max()),
                 b=float(np.abs(b[p] - ref['b']).max()) / ref['scale_b'],
                 A=float(np.abs(A[p] - ref['A']).max()) / S0,
                 orth=float(np.abs(T[p].astype(np.float64) @ T[p].T - np.eye(3)).max()))
        gl, gr = dY[p], dY[B + p]
        scale = max(np.abs(ref['dYl']).max(), np.abs(ref['dYr']).max())
        e['dY'] = max(np.abs(gl - ref['dYl']).max(), np.abs(gr - ref['dYr']).max()) / scale
        det_T = np.linalg.det(T[p].astype(np.float64))     # diag(1, 1, sign det A) makes T proper whatever det A is
        assert abs(det_T - 1.0) <= 3 * TOL_ORTH, f'{what}: det T {det_T:+.7f}, det A {ref["det"]:+.3e}'
        signs.add(int(np.sign(ref['det'])))
        assert e['T'] <= TOL_T[group], f'{what}: T {T[p].tolist()} vs float64 {ref["T"].tolist()} ({e["T"]:.2e})'
        assert e['b'] <= TOL_B[group], f'{what}: b {b[p]} vs float64 {ref["b"]} ({e["b"]:.2e} of {ref["scale_b"]:.1f})'
        assert e['A'] <= TOL_A, f'{what}: A_out {A[p].tolist()} vs float64 {ref["A"].tolist()} ({e["A"]:.2e} of S_0)'
        assert e['orth'] <= TOL_ORTH, f'{what}: |T T^T - I| = {e["orth"]:.2e}'
        assert e['dY'] <= TOL_DY[group], f'{what}: dY {e["dY"]:.2e} of the largest |dY| {scale:.3e}'
        for k, v in e.items():
            key = f'{k} ({group})' if k in ('T', 'b', 'dY') else k
            worst[key] = max(worst.get(key, 0.0), v)
    return worst, signs


def check_status_11(dev, K=1, n_pairs=3):
    """All-zero draws with K = 1 keep A = 0 through the 10 guard iterations: status 11 ("unstable", model.py), finite T
    and b, A_out = 0 + the 10 zero draws and not one more (the next pair's draws are non-zero), a finite backward (the
    denominator clamp: with S = 0 every dP_ij is 0 / 0 without it) equal to the mean path alone, dA being 0."""
    rng = np.random.default_rng(5)
    yl, yr = (rng.normal(size=(n_pairs, K, 3)) * 2 + CENTRE).astype(np.float32), \
        (rng.normal(size=(n_pairs, K, 3)) * 2 - CENTRE).astype(np.float32)
    draws = np.zeros((n_pairs, 10, 3), np.float32)
    draws[1:] = rng.uniform(0.3, 1.0, size=(n_pairs - 1, 10, 3))     # pair 0 unstable; the others' draws follow it
    Y = np.concatenate([yl, yr])
    T, b, A, status = kabsch_fwd(dev, Y, draws)
    assert status[0] == 11, status
    assert np.isfinite(T[0]).all() and np.isfinite(b[0]).all(), (T[0], b[0])
    assert (A[0] == 0).all(), f'A_out {A[0].tolist()}: the guard added draws beyond its 10th iteration'
    for p in range(1, n_pairs):      # A = diag(draw 0): stable after one draw
        assert status[p] == 1 and np.allclose(A[p], np.diag(draws[p, 0]), rtol=0, atol=0), (p, status[p], A[p])
    dT, db = rng.normal(size=(n_pairs, 3, 3)), rng.normal(size=(n_pairs, 3))
    dY = kabsch_bwd(dev, Y, A, T, dT, db)
    assert np.isfinite(dY).all(), dY[[0, n_pairs]]
    # K = 1, dA = 0: d Yr = db, d Yl = -T^T db (the mean path of b = mean_r - T mean_l)
    want_r, want_l = db[0], -(T[0].astype(np.float64).T @ db[0])
    assert np.abs(dY[n_pairs, 0] - want_r).max() <= 1e-6 * np.abs(want_r).max(), (dY[n_pairs, 0], want_r)
    assert np.abs(dY[0, 0] - want_l).max() <= 1e-6 * max(1.0, np.abs(want_l).max()), (dY[0, 0], want_l)
    return status


def check_planar_unstable(dev, K=64, n_pairs=3, seed=9):
    """Planar ligand keypoints whose draws never touch the zero column: A keeps rank 2 through all 10 iterations, status
    11, and T comes from the SVD's rank-deficient branch (U[:, 2] = U[:, 0] x U[:, 1]): T must be orthonormal, finite,
    and map the two leading right singular vectors of A_out onto the left ones."""
    rng = np.random.default_rng(seed)
    pairs = [guard_pair(rng, 'planar', K) for _ in range(n_pairs)]
    draws = rng.uniform(0.3, 1.0, size=(n_pairs, 10, 3)).astype(np.float32)
    draws[:, :, 2] = 0.0
    Y = _Y(dict(pairs=pairs))
    T, b, A, status = kabsch_fwd(dev, Y, draws)
    worst = 0.0
    for p, (yl, yr) in enumerate(pairs):
        assert status[p] == 11, status
        A64 = ((_f64(yr) - _f64(yr).mean(0)).t() @ (_f64(yl) - _f64(yl).mean(0))).numpy() + np.diag(draws[p].astype(np.float64).sum(0))
        assert (A[p][:, 2] == 0).all(), A[p]
        U, S, Vt = np.linalg.svd(A64)
        assert S[2] == 0.0 and S[1] > 1e3 * DECISION_ULPS * 2.0 ** -24 * S[0], S
        Tp = T[p].astype(np.float64)
        e = max(float(np.abs(Tp @ Tp.T - np.eye(3)).max()), float(np.abs(Tp @ Vt[:2].T - U[:, :2]).max()))
        assert np.isfinite(b[p]).all() and e <= TOL_PLANAR, (p, e, T[p])
        worst = max(worst, e)
    return worst


def check_seeded_draws(dev, K, seed=1234):
    """svd_draws = NULL: the kernel's own hash draws.  Guard pairs must end in 1..10 iterations with a proper orthonormal
    T, and two runs must agree bit for bit."""
    rng = np.random.default_rng(seed)
    kinds = ['rank'] * 3 if K <= 3 else ['planar', 'collapsed', 'planar']
    pairs = [guard_pair(rng, k, K) for k in kinds]
    Y = _Y(dict(pairs=pairs))
    r1 = kabsch_fwd(dev, Y, None, seed=seed)
    r2 = kabsch_fwd(dev, Y, None, seed=seed)
    for a, b in zip(r1, r2):
        assert np.array_equal(np.asarray(a), np.asarray(b)), 'seeded Kabsch differs run to run'
    T, b, A, status = r1
    for p in range(len(pairs)):
        assert 1 <= status[p] <= 10, status
        Tp = T[p].astype(np.float64)
        assert np.abs(Tp @ Tp.T - np.eye(3)).max() <= TOL_ORTH, Tp
        assert abs(np.linalg.det(Tp) - 1.0) <= 3 * TOL_ORTH, (Tp, A[p])
    return status


def check_kabsch_limit(dev):
    """129 keypoints: EQD_ERR_UNSUPPORTED from both entry points, the message naming the limit."""
    B, K = 2, 129
    Y = torch.zeros(2 * B, K, 3, device=dev)
    T, b, A = (torch.zeros(B, n, device=dev) for n in (9, 3, 9))
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    rc = L._lib.eqd_kabsch_fwd(B, K, _P(Y), None, 0, _P(T), _P(b), _P(A), _P(status), L.stream_ptr(dev))
    msg = L._lib.eqd_last_error().decode()
    assert rc == 3 and '128' in msg and '129' in msg, (rc, msg)
    rc = L._lib.eqd_kabsch_bwd(B, K, _P(Y), _P(A), _P(T), _P(T), _P(b), _P(Y), L.stream_ptr(dev))
    msg = L._lib.eqd_last_error().decode()
    assert rc == 3 and '128' in msg and '129' in msg, (rc, msg)


# ---- keypoint pooling -------------------------------------------------------------------------------------------
KP_SIZES = ((1, 40), (1030, 1), (65, 129))     # 1-node segments on both sides, one segment longer than 1 024 nodes


def keypoint_reference(seg, K, Wk, Wq, hm, H, Z, dY):
    """check_keypoints_and_apply's formula in float64: Y[s] = softmax_nodes(H_s Wk^(k) . Wq^(k) qmean[partner(s)] / 8)
    Z_s with qmean the per-segment mean of hm, and the gradients of <Y, dY> by autograd."""
    leaves = [x.double().clone().requires_grad_(True) for x in (Wk, Wq, hm, H, Z)]
    Wk_, Wq_, hm_, H_, Z_ = leaves
    S = len(seg) - 1
    B = S // 2
    qm = torch.stack([hm_[seg[s]:seg[s + 1]].mean(0) for s in range(S)])
    Ys, tot = [], 0.0
    for s in range(S):
        partner = s + B if s < B else s - B
        n0, n1 = seg[s], seg[s + 1]
        att = torch.softmax(
            F.linear(H_[n0:n1], Wk_).view(-1, K, 64).transpose(0, 1) @
            F.linear(qm[partner:partner + 1], Wq_).view(1, K, 64).transpose(0, 1).transpose(1, 2) / 8.0, dim=1).view(K, -1)
        y = att @ Z_[n0:n1]
        Ys.append(y.detach())
        tot = tot + (y * dY[s].double()).sum()
    tot.backward()
    return torch.stack(Ys), qm.detach(), {n: x.grad for n, x in zip(('dWk', 'dWq', 'd_hm', 'dH', 'dZ'), leaves)}


def check_keypoint_pool(dev, K, sizes=KP_SIZES, seed=7):
    """eqd_keypoint_pool_fwd / _bwd against float64.  Keypoints over the segment's largest |z|; dWk, dWq over their own
    largest element; dH, dZ, d_hm row by row over the segment's largest row (at least 1e-3 of the tensor's).  Returns the
    worst (keypoint, gradient) errors."""
    from tests import parity_common as pc
    g, pk, gs = pc.small_graph(dev, sizes=sizes, degrade=False)
    torch.manual_seed(seed)
    N, B = pk.n_nodes, pk.n_pairs
    Wk, Wq = torch.randn(K * 64, 64) * 0.3, torch.randn(K * 64, 64) * 0.3
    hm, H = torch.randn(N, 64), torch.randn(N, 64)
    Z = (torch.randn(N, 3) * 5 + torch.from_numpy(CENTRE).float()).contiguous()
    dYr = torch.randn(2 * B, K, 3)
    seg = pk.seg_off.cpu().tolist()
    Yref, qm, grads = keypoint_reference(seg, K, Wk, Wq, hm, H, Z, dYr)
    dd = [t.to(dev).contiguous() for t in (Wk, Wq, qm.float(), H, Z, dYr)]
    Y, scores, lse = (torch.zeros(2 * B, K, 3, device=dev), torch.zeros(N, K, device=dev), torch.zeros(2 * B, K, device=dev))
    qp, u = torch.zeros(2 * B, K, 64, device=dev), torch.zeros(2 * B, K, 64, device=dev)
    L.check(L._lib.eqd_keypoint_pool_fwd(C.byref(gs), K, _P(dd[0]), _P(dd[1]), _P(dd[2]), _P(dd[3]), _P(dd[4]), _P(Y),
                                         _P(scores), _P(lse), _P(qp), _P(u), L.stream_ptr(dev)))
    wsb = L._lib.eqd_keypoint_pool_bwd_workspace_bytes(C.byref(gs), K)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    dH, dZ, dhm = (torch.full((N, w), float('nan'), device=dev) for w in (64, 3, 64))
    dWk, dWq = torch.zeros(K * 64, 64, device=dev), torch.zeros(K * 64, 64, device=dev)
    L.check(L._lib.eqd_keypoint_pool_bwd(C.byref(gs), K, _P(dd[0]), _P(dd[1]), _P(dd[2]), _P(qp), _P(u), _P(dd[3]),
                                         _P(dd[4]), _P(scores), _P(lse), _P(dd[5]), _P(dH), _P(dZ), _P(dWk), _P(dWq),
                                         _P(dhm), _P(ws), C.c_size_t(wsb), L.stream_ptr(dev)))
    _sync(dev)
    Y = Y.cpu().double()
    e_kp = 0.0
    for s in range(2 * B):
        sc = float(Z[seg[s]:seg[s + 1]].double().abs().max())
        e = float((Y[s] - Yref[s]).abs().max()) / sc
        assert e <= TOL_KP, f'K={K} segment {s} ({seg[s + 1] - seg[s]} nodes): keypoints {e:.2e} of |z| {sc:.1f}'
        e_kp = max(e_kp, e)
    e_gr = 0.0
    for nm, got in (('dWk', dWk), ('dWq', dWq)):
        ref = grads[nm]
        e = float((got.cpu().double() - ref).abs().max()) / float(ref.abs().max())
        assert e <= TOL_KP_GRAD, f'K={K} {nm}: {e:.2e} of its largest element'
        e_gr = max(e_gr, e)
    for nm, got in (('dH', dH), ('dZ', dZ), ('d_hm', dhm)):
        ref, got = grads[nm], got.cpu().double()
        floor = 1e-3 * float(ref.abs().max())
        for s in range(2 * B):
            r = ref[seg[s]:seg[s + 1]]
            e = float((got[seg[s]:seg[s + 1]] - r).abs().max()) / max(float(r.abs().max()), floor)
            assert e <= TOL_KP_GRAD, f'K={K} {nm} segment {s} ({seg[s + 1] - seg[s]} nodes): {e:.2e}'
            e_gr = max(e_gr, e)
    return e_kp, e_gr


# ---- model level ------------------------------------------------------------------------------------------------
# ligands of 1, 64, 65 and 129 nodes: below, at and past the fused apply's 64-row stride.  The 1-node ligand's keypoints
# coincide, A = 0 and the guard fires: MODEL_DRAWS makes it stable after one draw (A = diag(0.9, 0.5, 0.2)).
MODEL_SIZES = ((1, 30), (64, 20), (65, 70), (129, 33))
MODEL_STATUS = [1, 0, 0, 0]
HEAD_SIZES = ((64, 20), (65, 70), (129, 33))


def model_draws(dev, n_pairs=len(MODEL_SIZES)):
    d = torch.zeros(n_pairs, 10, 3)
    d[0, 0] = torch.tensor([0.9, 0.5, 0.2])
    return d.to(dev)


def check_model(dev, K, layers=2):
    from tests import parity_common as pc
    pc.check_model_vs_oracle(dev, MODEL_SIZES, layers=layers, seed=21, pair_seed=35, args_over=dict(num_att_heads=K),
                             what=f'num_att_heads={K}', svd_draws=model_draws(dev), svd_status=MODEL_STATUS)


def _head_net(dev, K, sizes, layers, bf16=False):
    from equidock_public_amd import graph as G, synthetic
    from tests import parity_common as pc
    args = port.default_args(iegmn_n_lays=layers, skip_weight_h=0.75, num_att_heads=K)
    sd = port.init_state_dict(args, seed=3)
    net = pc.build_model(dict(args, hip_storage_dtype='bf16') if bf16 else args, sd, dev)
    net.iegmn_original.svd_draws = model_draws(dev, len(sizes))
    g = G.batch_pairs(synthetic.make_pairs(list(sizes), 36)).to(dev)
    return net, g


def check_fused_apply(dev, K, sizes=MODEL_SIZES, layers=2):
    """The rigid apply fused into k_kabsch_fwd / _bwd at ligands of 1, 64, 65, 129 rows.  Forward: the model's ligand
    output equals T x0 + b in float64 from the kernel's own T and b, row by row, over |x0| |T| + |b|.  Backward: the
    head's backward from d_lig alone (dT / db summed inside k_kabsch_bwd over the pair's ligand rows at a stride of 64)
    equals the head's backward from the external dT = d_lig^T x0, db = colsum d_lig (float64 sums, rounded once)."""
    net, g = _head_net(dev, K, sizes, layers)
    ie = net.iegmn_original
    lig, Yl, Yr, T, b = [t.detach() for t in net.forward_batched(g)]
    _sync(dev)
    assert ie.last_svd_status.cpu().tolist() == MODEL_STATUS[:len(sizes)], ie.last_svd_status
    lc = [int(v) for v in g.batch_num_nodes('ligand')]
    x0 = g.pack().x0.cpu().double()[:sum(lc)]
    T64, b64 = T.cpu().double(), b.cpu().double()
    e_fwd, lo = 0.0, 0
    for p, n in enumerate(lc):
        x = x0[lo:lo + n]
        want = x @ T64[p].t() + b64[p]
        scale = x.abs().max(1).values * float(T64[p].abs().sum(1).max()) + float(b64[p].abs().max())
        e = float(((lig.cpu().double()[lo:lo + n] - want).abs().max(1).values / scale).max())
        assert e <= TOL_APPLY, f'K={K} ligand {p} ({n} rows): fused apply {e:.2e} of the row scale'
        e_fwd = max(e_fwd, e)
        lo += n
    torch.manual_seed(11)
    d_lig = torch.randn(sum(lc), 3)
    dT = torch.stack([d_lig[o:o + n].double().t() @ x0[o:o + n] for o, n in zip(np.cumsum([0] + lc[:-1]), lc)]).float()
    db = torch.stack([d_lig[o:o + n].double().sum(0) for o, n in zip(np.cumsum([0] + lc[:-1]), lc)]).float()
    dh1, dx1, hg1 = ie.head_backward(g, d_lig.to(dev), None, None, None, None)
    dh2, dx2, hg2 = ie.head_backward(g, None, None, None, dT.to(dev), db.to(dev))
    _sync(dev)
    e_bwd = 0.0
    for nm, a, r in [('d h_L', dh1, dh2), ('d x_L', dx1, dx2)] + [(k, hg1[k], hg2[k]) for k in hg1]:
        a, r = a.cpu().double(), r.cpu().double()
        e = float((a - r).abs().max()) / max(float(r.abs().max()), 1e-30)
        assert e <= TOL_APPLY_BWD, f'K={K} apply backward {nm}: {e:.2e} of its largest element'
        e_bwd = max(e_bwd, e)
    return e_fwd, e_bwd


def check_model_limit(dev, K=129):
    from equidock_public_amd import graph as G, synthetic
    from tests import parity_common as pc
    import pytest
    args = port.default_args(iegmn_n_lays=1, skip_weight_h=0.75, num_att_heads=K)
    sd = port.init_state_dict(args, seed=3)
    net = pc.build_model(args, sd, dev)
    g = G.batch_pairs(synthetic.make_pairs([(20, 30)], 36)).to(dev)
    with pytest.raises(L.EquidockHipError, match='num_att_heads=129 .*1..128'):
        net(g, epoch=0)
