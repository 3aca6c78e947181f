"""The node update of an IEGMN layer in float64, and operator checks of every kernel body behind eqd_launch_rowchain
(csrc/eqd_node_kernels.hip):

  k_rowchain_res_fwd            fp32 forward of a 64-wide layer, tiles <= CUs, h0 65..80 wide, weights resident in LDS
  k_rowchain<1, ., 1> / <1, ., 2>   tiles <= CUs / tiles > CUs (EQD_ROWCHAIN_OCC forces either)
  k_rowchain<2, ., 1>           EQD_ROW_TILES=2
  k_rowwave                     EQD_ROWWAVE=1
  k_rowres                      >= 3 tiles per CU or EQD_ROWWAVE=2; EQD_ROWRES_TPS forces the tiles per workgroup
  k_rowres80                    bf16 mode, a 65..80-wide job in the chain, k_rowres sizes; EQD_ROWRES80=0 turns it off

Shared by tests/test_node_chain_sim.py (the x86 simulator build) and tests/test_node_chain_gpu.py.

The reference (node_reference) writes the forward and the backward out by hand on float64 copies of the float32 inputs,
with the LeakyReLU branch taken from the y_act the kernel returned; test_reference_is_autograd pins it to float64
autograd.  In bf16 mode every MFMA operand is rounded to bf16 where the kernels round it (the R(...) calls, each with
the source line it restates).  The same function evaluated in float32 is the yardstick the bounds come from: a bound is
8 x the distance of that float32 evaluation from float64, never the kernels' own error.

Every case asserts its own coverage: the kernel name of the forward and of the backward launch (eqd_profile_*), the
increment of eqd_chain_resident_launches(), and for what the profiler cannot name (the register budget of k_rowchain,
k_rowres against k_rowres80) the host-side condition that selects it (expected_bodies)."""
import ctypes as C

import torch

from equidock_public_amd import _lib as L
from tests import parity_common as pc

SLOPE, EPS = 0.01, 1e-5
NAMES_FWD = ('h_out', 'y_act', 'a1n')
NAMES_ROW = ('d_h', 'd_aggr_msg', 'd_h0', 'd_aggr_cross')
NAMES_W = ('dWn1', 'dbn1', 'dln_g', 'dln_b', 'dWn2', 'dbn2')
CLASS_OF = dict([(n, 'fwd') for n in NAMES_FWD] + [(n, 'row') for n in NAMES_ROW] + [(n, 'w') for n in NAMES_W])
GUARD_ROWS, SENTINEL = 16, 12345.0
NEAR_KINK_REL, NEAR_KINK_SHARE = 1e-6, 1e-4      # fewer than 1 in 10^4 pre-activations within 1e-6 max|z| of the kink

# ---- widths -------------------------------------------------------------------------------------------------------
# (d_in, d0) in {(64, 69), (64, 64), (69, 69), (64, 80), (64, 4)}, ld_cross = 80 for d_in = 69 else 64, one case with
# ld_cross = 72 > d_in = 64; with and without aggr_cross; skip weights 0.25 / 0.75 and exactly 0 and 1.
CONFIGS = {c['id']: c for c in (
    dict(id='64x69', d=64, d0=69, ldc=64, cross=True, s=0.75),
    dict(id='64x64', d=64, d0=64, ldc=64, cross=True, s=0.25),
    dict(id='69x69', d=69, d0=69, ldc=80, cross=True, s=0.75),
    dict(id='64x80', d=64, d0=80, ldc=64, cross=True, s=0.25),
    dict(id='64x4', d=64, d0=4, ldc=64, cross=True, s=0.75),
    dict(id='64x69-nocross', d=64, d0=69, ldc=64, cross=False, s=0.25),
    dict(id='64x64-nocross', d=64, d0=64, ldc=64, cross=False, s=0.75),
    dict(id='69x69-nocross', d=69, d0=69, ldc=80, cross=False, s=0.25),
    dict(id='64x69-ld72', d=64, d0=69, ldc=72, cross=True, s=0.25),
    dict(id='64x64-s0', d=64, d0=64, ldc=64, cross=True, s=0.0),
    dict(id='64x69-s1', d=64, d0=69, ldc=64, cross=True, s=1.0),
)}
FAMILIES = ('plain', 'norm30', 'shift')
ROW_EDGES = (1, 15, 16, 17, 31, 32, 33, 48, 255, 256, 257)

# ---- kernel bodies: the switches that select them --------------------------------------------------------------------
BODIES = {
    'default': {},
    'chain-noresident': {'EQD_CHAIN_RESIDENT': '0'},
    'chain-occ1': {'EQD_ROWCHAIN_OCC': '1'},
    'chain-occ2': {'EQD_ROWCHAIN_OCC': '2'},
    'chain-2tiles': {'EQD_ROWWAVE': '0', 'EQD_ROW_TILES': '2'},
    'rowwave': {'EQD_ROWWAVE': '1'},
    'rowres': {'EQD_ROWWAVE': '2'},
    'rowres-tps1': {'EQD_ROWWAVE': '2', 'EQD_ROWRES_TPS': '1'},
    'rowres-tps3': {'EQD_ROWWAVE': '2', 'EQD_ROWRES_TPS': '3'},
    'rowres-tps5': {'EQD_ROWWAVE': '2', 'EQD_ROWRES_TPS': '5'},
    'rowres-tps16': {'EQD_ROWWAVE': '2', 'EQD_ROWRES_TPS': '16'},
    'rowres-no80': {'EQD_ROWWAVE': '2', 'EQD_ROWRES80': '0'},
}
SWITCHES = ('EQD_CHAIN_RESIDENT', 'EQD_ROWCHAIN_OCC', 'EQD_ROWWAVE', 'EQD_ROW_TILES', 'EQD_ROWRES_TPS', 'EQD_ROWRES80')
RR_WAVES = 8            # waves of a k_rowres workgroup (csrc/eqd_rowres_inl.h): more tiles than this = the two-slot path


def rr_blocks(rows, tps):
    """workgroups of a k_rowres launch (rr_blocks, csrc/eqd_node_kernels.hip) and the tiles the last one owns"""
    nt = (rows + 15) // 16
    nb = (nt + tps - 1) // tps
    return nb, nt - (nb - 1) * tps


def _rowres_rows():
    """Row counts against EQD_ROWRES_TPS: (a) the last workgroup owns fewer tiles than the others, (b) it owns exactly
    one, partial, tile, (c) tiles per workgroup > waves (the two-slot path).  With one tile per workgroup (a) does not
    exist, and a last workgroup without tiles never does: rr_blocks rounds the workgroup count up from the tile count."""
    out = []
    for tps, rows, kind in ((1, 39, 'b'), (3, 80, 'a'), (3, 57, 'b'), (5, 115, 'a'), (5, 81, 'b'), (16, 405, 'ac'),
                            (16, 257, 'bc'), (16, 144, 'c')):
        nb, last = rr_blocks(rows, tps)
        if 'a' in kind:
            assert nb > 1 and 1 < last < tps or (last < tps and rows % 16 == 0), (tps, rows)
        if 'b' in kind:
            assert nb > 1 and last == 1 and rows % 16 != 0, (tps, rows)
        if 'c' in kind:
            assert tps > RR_WAVES and min(tps, (rows + 15) // 16) > RR_WAVES, (tps, rows)
        what = {'a': 'last-wg-fewer-tiles', 'b': 'last-wg-one-partial-tile', 'c': 'two-slot'}
        out.append((f'rowres-tps{tps}', rows, '+'.join(what[k] for k in kind)))
    return out


ROWRES_ROWS = _rowres_rows()


def expected_bodies(env, cfg, bf16, rows, cus):
    """What eqd_launch_rowchain must pick for the forward and the backward chain of this case - the host-side conditions
    of rw_eligible / rw80_eligible / cr_fwd_eligible restated from the widths alone.  Returns per direction the name
    the profiler reports and the body (which also tells what the name cannot: the register budget of k_rowchain - tiles
    against the CU count - and k_rowres80 - bf16 and a 65..80-wide job)."""
    d, d0, cross = cfg['d'], cfg['d0'], cfg['cross']
    tiles = (rows + 15) // 16
    f = env.get('EQD_ROWWAVE')
    mode = int(f) if f in ('0', '1', '2') else (2 if tiles >= 3 * cus else 0)
    two = env.get('EQD_ROW_TILES') == '2'
    occ = env.get('EQD_ROWCHAIN_OCC')
    res80 = env.get('EQD_ROWRES80') != '0'

    def chain(resident_ok):
        blocks = (rows + 31) // 32 if two else tiles
        if resident_ok and not occ and env.get('EQD_CHAIN_RESIDENT') != '0' and not two and not bf16 and blocks <= cus:
            return 'k_rowchain', 'k_rowchain_res_fwd'
        if two:
            return 'k_rowchain', 'k_rowchain<2,1>'
        one = occ == '1' if occ in ('1', '2') else blocks <= cus
        return 'k_rowchain', 'k_rowchain<1,1>' if one else 'k_rowchain<1,2>'

    def pick(all64, wide_ok, wide, resident_ok):
        if mode and all64:
            return ('k_rowwave', 'k_rowwave') if mode == 1 else ('k_rowres', 'k_rowres')
        if mode == 2 and bf16 and res80 and wide_ok and wide:
            return 'k_rowres', 'k_rowres80'
        return chain(resident_ok)
    # forward: outputs d (job 1) and 64 (job 2); sources h (d), aggr_msg (64), aggr_cross (d), h0 (d0)
    fwd = pick(d == 64 and 64 <= d0 <= 80, d >= 64 and 64 <= d0 <= 80, d > 64 or d0 > 64,
               d == 64 and cross and 65 <= d0 <= 80)
    # backward: outputs d, d, 64, d, d0, d; every source 64 wide or the d-wide LDS tile
    bwd = pick(d == 64 and d0 == 64, d >= 64 and d0 >= 4, d > 64 or d0 > 64, False)
    return fwd, bwd


# ---- inputs -------------------------------------------------------------------------------------------------------


def make_case(cfg, rows, family='plain', drop=False, seed=31):
    """Host tensors of one case.  plain: randn * 0.5 (check_node_update's inputs); norm30: h, h0 with rows of norm ~30
    (LayerNorm outputs of a trained layer times a skip sum); shift: bn1 + 20, every LayerNorm input row has a mean far
    above its spread.  drop: nn.Dropout factors at p = 0.25 and one row whose factors are all zero.  The case is re-seeded
    until the float64 reference has fewer than NEAR_KINK_SHARE of its pre-activations next to the LeakyReLU kink."""
    d, d0, ldc, cross = cfg['d'], cfg['d0'], cfg['ldc'], cfg['cross']
    for attempt in range(20):
        gen = torch.Generator().manual_seed(seed + 1000 * attempt)
        mk = lambda *sh: torch.randn(*sh, generator=gen) * 0.5      # noqa: E731
        h, am, ac, h0 = mk(rows, d), mk(rows, 64), torch.zeros(rows, ldc), mk(rows, d0)
        ac[:, :d] = mk(rows, d)
        if family == 'norm30':
            h = h * (30.0 / h.norm(dim=1, keepdim=True))
            h0 = h0 * (30.0 / h0.norm(dim=1, keepdim=True))
        Wn1, bn1 = mk(d, d0 + 2 * d + 64) * 0.3, mk(d)
        if family == 'shift':
            bn1 = bn1 + 20.0
        lg, lb = 1.0 + 0.2 * torch.randn(d, generator=gen), 0.2 * torch.randn(d, generator=gen)
        Wn2, bn2 = mk(64, d) * 0.3, mk(64)
        mul = None
        if drop:
            mul = (torch.rand(rows, d, generator=gen) >= 0.25).float() / 0.75
            if rows > 1:
                mul[rows - 1 if rows < 40 else rows // 2] = 0.0      # zero_row(case)
        case = dict(cfg=cfg, rows=rows, family=family, h=h, am=am, ac=ac if cross else None, h0=h0, Wn1=Wn1, bn1=bn1, lg=lg,
                    lb=lb, Wn2=Wn2, bn2=bn2, mul=mul, w=torch.randn(rows, 64, generator=gen))
        z = node_reference(case, 0)['pre']
        share = float((z.abs() < NEAR_KINK_REL * float(z.abs().max())).double().mean())
        if share < NEAR_KINK_SHARE:
            assert attempt == 0 or rows * d < 2 / NEAR_KINK_SHARE, 'only a tiny case may need another seed'
            return case
    raise AssertionError('no seed keeps the pre-activations away from the LeakyReLU kink')


def zero_row(case):
    """the row whose dropout factors are all zero (the last row of a small case: inside the partial tile), or None"""
    rows = case['rows']
    return None if case['mul'] is None or rows == 1 else (rows - 1 if rows < 40 else rows // 2)


# ---- the reference ------------------------------------------------------------------------------------------------


def _rb(t):
    """round to nearest even to bf16, in t's dtype (what pack_bf4 does to an MFMA operand)"""
    return t.float().to(torch.bfloat16).to(t.dtype)


def node_reference(case, bf16, dtype=torch.float64, y_act=None, a1n=None):
    """Forward and backward of the node update in `dtype` from the float32 inputs, by hand.

    y_act: the kernel's y_act; the LeakyReLU branch of an element is its sign (y_act = mul * LeakyReLU(z): the sign of z
    wherever mul != 0, and no gradient where mul == 0).  None: the branch of the reference's own pre-activation.
    a1n: the kernel's a1n; the second GEMM and dWn2 are then STAGED on it (no bf16 rounding decision stays open).
    bf16 = 1: R() rounds an MFMA operand to bf16; everything else stays in `dtype` as it stays fp32 in the kernels."""
    cfg = case['cfg']
    d, s, cross = cfg['d'], cfg['s'], cfg['cross']
    skip = d == 64
    alpha = s if skip else 1.0
    R = _rb if bf16 else (lambda t: t)
    c = lambda t: t.to(dtype)      # noqa: E731
    h, am, h0, W1, b1, lg, lb, W2, b2, G = (c(case[k]) for k in ('h', 'am', 'h0', 'Wn1', 'bn1', 'lg', 'lb', 'Wn2', 'bn2', 'w'))
    mul = None if case['mul'] is None else c(case['mul'])
    if cross:
        X = torch.cat([h, am, c(case['ac'])[:, :d], h0], 1)
        W1x = W1
    else:      # aggr_cross = NULL: the block is dropped (eqd_driver.hip: eqd_node_update_fwd skips the source)
        X = torch.cat([h, am, h0], 1)
        W1x = torch.cat([W1[:, :d + 64], W1[:, 2 * d + 64:]], 1)
    # forward.  bf16 rounding points: the rows X and the weights W of every source when lin_mma forms its operands
    # (eqd_linear_inl.h:283-298 pack_bf4 of a[] and b[]; eqd_rowwave_inl.h:161-169; eqd_rowres_inl.h:99, :177 and :217-225;
    # eqd_rowres80_inl.h:58, :82-96), fp32 accumulate, bias / LeakyReLU / dropout factor / LayerNorm in fp32
    pre = R(X) @ R(W1x).t() + b1
    pos = (pre > 0) if y_act is None else (c(y_act) > 0)
    y = torch.where(pos, pre, SLOPE * pre)
    if mul is not None:
        y = y * mul
    mean = y.mean(1, keepdim=True)
    cen = y - mean
    rstd = 1.0 / torch.sqrt((cen * cen).mean(1, keepdim=True) + EPS)
    xh = cen * rstd
    a1 = xh * lg + lb
    a1_in = a1 if a1n is None else c(a1n)
    # the second job reads a1n as an LDS tile in fp32 and rounds it as the B operand (eqd_linear_inl.h:283 / :295,
    # eqd_rowwave_inl.h:185-197 `local ? pack_bf4(Bl...)`, eqd_rowres_inl.h:177 / :217, eqd_rowres80_inl.h:82)
    u = R(a1_in) @ R(W2).t() + b2
    out = dict(pre=pre, y_act=y, a1n=a1, h_out=s * u + (1 - s) * h if skip else u)
    # backward.  d a1n = alpha * d_h_out Wn2: d_h_out and the transposed weights rounded as operands of the chain's first
    # job (eqd_driver.hip:1252 w_rs = 1: the same lin_mma, WT = true); its fp32 result is NOT rounded - the next job is the
    # LayerNorm / LeakyReLU backward in fp32 (eqd_node_kernels.hip:572-608), not an MFMA
    da1 = alpha * (R(G) @ R(W2))
    out['dln_g'], out['dln_b'] = (da1 * xh).sum(0), da1.sum(0)
    dx = da1 * lg
    s1, s2 = dx.mean(1, keepdim=True), (dx * xh).mean(1, keepdim=True)
    dz = rstd * (dx - s1 - xh * s2) * torch.where(pos, torch.ones((), dtype=dtype), torch.full((), SLOPE, dtype=dtype))
    if mul is not None:
        dz = dz * mul
    # dz, kept in fp32 in its LDS tile and in the workspace, is rounded as the operand of the four dx jobs and of the
    # eqd_atb jobs; so are Wn1's column blocks (eqd_driver.hip:1272) and the eqd_atb operands X = dz / d_h_out and
    # Y = the layer inputs / a1n (eqd_node_kernels.hip:1289-1292 atb_mma, :1491 / :1517 atb_fast); the column sums that
    # give dbn1 / dbn2 stay fp32 (:1694), and so does the skip term (1 - s) d_h_out (EqdLinJob.R)
    dX = R(dz) @ R(W1x)
    slack = None
    if bf16:      # what the open roundings of dz can move (see the bounds below): one bf16 spacing per open element
        a = dz.double().abs()
        ulp = torch.exp2(torch.floor(torch.log2(a.clamp(min=1e-300))) - 7)
        to_tie = ulp / 2 - (dz.double() - _rb(dz).double()).abs()
        move = torch.where(to_tie <= open_eps(case['family']) * a.max(1, keepdim=True).values, ulp, torch.zeros_like(ulp))
        sX, sW = move @ R(W1x).double().abs(), move.t() @ R(X).double().abs()
    out['d_h'] = dX[:, :d] + ((1 - s) * G if skip else 0.0)
    out['d_aggr_msg'] = dX[:, d:d + 64]
    if cross:
        out['d_aggr_cross'] = dX[:, d + 64:2 * d + 64]
        out['d_h0'] = dX[:, 2 * d + 64:]
    else:
        out['d_aggr_cross'] = None
        out['d_h0'] = dX[:, d + 64:]
    dW1 = R(dz).t() @ R(X)
    if not cross:      # dWn1's aggr_cross columns come back as the caller left them (zero)
        dW1 = torch.cat([dW1[:, :d + 64], torch.zeros(d, d, dtype=dtype), dW1[:, d + 64:]], 1)
    if bf16:
        if not cross:
            sW = torch.cat([sW[:, :d + 64], torch.zeros(d, d, dtype=torch.float64), sW[:, d + 64:]], 1)
        o = d + 64 + (d if cross else 0)
        slack = dict(d_h=sX[:, :d], d_aggr_msg=sX[:, d:d + 64], d_aggr_cross=sX[:, d + 64:2 * d + 64], d_h0=sX[:, o:],
                     dWn1=sW)
    out['slack'], out['dz'] = slack, dz
    out['dWn1'], out['dbn1'] = dW1, dz.sum(0)
    out['dWn2'], out['dbn2'] = alpha * (R(G).t() @ R(a1_in)), alpha * G.sum(0)
    return out


def autograd_reference(case):
    """float64 autograd of the formula as written (fp32 mode), for test_reference_is_autograd"""
    import torch.nn.functional as F
    cfg = case['cfg']
    d, s = cfg['d'], cfg['s']
    keys = ('h', 'am', 'ac', 'h0', 'Wn1', 'bn1', 'lg', 'lb', 'Wn2', 'bn2')
    lv = {k: (None if case[k] is None else case[k].double().clone().requires_grad_(True)) for k in keys}
    blocks = [lv['h'], lv['am']] + ([lv['ac'][:, :d]] if cfg['cross'] else [torch.zeros(case['rows'], d, dtype=torch.float64)])
    z = F.leaky_relu(F.linear(torch.cat(blocks + [lv['h0']], 1), lv['Wn1'], lv['bn1']), SLOPE)
    if case['mul'] is not None:
        z = z * case['mul'].double()
    a1 = F.layer_norm(z, (d,), lv['lg'], lv['lb'], EPS)
    u = F.linear(a1, lv['Wn2'], lv['bn2'])
    ho = s * u + (1 - s) * lv['h'] if d == 64 else u
    (ho * case['w'].double()).sum().backward()
    g1 = lv['Wn1'].grad.clone()
    if not cfg['cross']:
        g1[:, d + 64:2 * d + 64] = 0
    return dict(h_out=ho.detach(), y_act=z.detach(), a1n=a1.detach(), d_h=lv['h'].grad, d_aggr_msg=lv['am'].grad,
                d_h0=lv['h0'].grad, d_aggr_cross=lv['ac'].grad[:, :d] if cfg['cross'] else None, dWn1=g1,
                dbn1=lv['bn1'].grad, dln_g=lv['lg'].grad, dln_b=lv['lb'].grad, dWn2=lv['Wn2'].grad, dbn2=lv['bn2'].grad)


# ---- the operator ---------------------------------------------------------------------------------------------------


def _guarded(dev, rows, cols, fill):
    """[rows + GUARD_ROWS][cols]: the body filled with `fill`, GUARD_ROWS rows of a sentinel behind it"""
    t = torch.full((rows + GUARD_ROWS, cols), fill, dtype=torch.float32, device=dev)
    t[rows:] = SENTINEL
    return t


def resident_launches():
    fn = pc.lib().eqd_chain_resident_launches
    fn.restype = C.c_longlong
    fn.argtypes = []
    return int(fn())


def run_kernels(dev, case, bf16, calls=1):
    """eqd_node_update_fwd, then `calls` x eqd_node_update_bwd into the same gradient buffers.  Every output and the
    workspace start as NaN with GUARD_ROWS sentinel rows behind them (the accumulated parameter gradients start as
    zeros).  Returns the 13 tensors on the host, the whole d_aggr_cross rows, the launch names of the two calls and the
    resident-body launches of the forward."""
    cfg, rows = case['cfg'], case['rows']
    d, d0, ldc, cross = cfg['d'], cfg['d0'], cfg['ldc'], cfg['cross']
    nan = float('nan')
    dd = {k: (None if case[k] is None else case[k].to(dev).contiguous())
          for k in ('h', 'am', 'ac', 'h0', 'Wn1', 'bn1', 'lg', 'lb', 'Wn2', 'bn2', 'mul', 'w')}
    prm = L.EqdNodeUpdateParams()
    prm.d_in, prm.d0, prm.d_out, prm.ld_cross = d, d0, 64, ldc
    prm.Wn1, prm.bn1, prm.ln_g, prm.ln_b, prm.Wn2, prm.bn2 = (dd[k].data_ptr() for k in ('Wn1', 'bn1', 'lg', 'lb', 'Wn2', 'bn2'))
    prm.skip_weight_h, prm.slope, prm.ln_eps, prm.bf16 = cfg['s'], SLOPE, EPS, int(bf16)
    prm.drop_mul = None if dd['mul'] is None else dd['mul'].data_ptr()
    P, lib, st = pc.P, pc.lib(), pc.st(dev)
    buf = dict(h_out=_guarded(dev, rows, 64, nan), y_act=_guarded(dev, rows, d, nan), a1n=_guarded(dev, rows, d, nan),
               d_h=_guarded(dev, rows, d, nan), d_aggr_msg=_guarded(dev, rows, 64, nan), d_h0=_guarded(dev, rows, d0, nan),
               d_aggr_cross=_guarded(dev, rows, ldc, nan),
               dWn1=_guarded(dev, d, d0 + 2 * d + 64, 0.0), dbn1=_guarded(dev, 1, d, 0.0), dln_g=_guarded(dev, 1, d, 0.0),
               dln_b=_guarded(dev, 1, d, 0.0), dWn2=_guarded(dev, 64, d, 0.0), dbn2=_guarded(dev, 1, 64, 0.0))
    acp = P(dd['ac']) if cross else None
    before = resident_launches()
    names_f = pc.launch_names(dev, lambda: L.check(lib.eqd_node_update_fwd(
        rows, C.byref(prm), P(dd['h']), P(dd['am']), acp, P(dd['h0']), P(buf['h_out']), P(buf['y_act']), P(buf['a1n']), st)))
    resident = resident_launches() - before
    wsb = lib.eqd_node_update_bwd_workspace_bytes(rows, C.byref(prm))
    assert wsb > 0 and wsb % 4 == 0, wsb
    ws = torch.full((wsb // 4 + 64,), nan, dtype=torch.float32, device=dev)
    ws[wsb // 4:] = SENTINEL
    gr = L.EqdNodeUpdateGrads()
    gr.dWn1, gr.dbn1, gr.dln_g, gr.dln_b, gr.dWn2, gr.dbn2 = (buf[k].data_ptr() for k in NAMES_W)

    def bwd():
        L.check(lib.eqd_node_update_bwd(rows, C.byref(prm), P(dd['h']), P(dd['am']), acp, P(dd['h0']), P(buf['y_act']),
                                        P(buf['a1n']), P(dd['w']), P(buf['d_h']), P(buf['d_aggr_msg']),
                                        P(buf['d_aggr_cross']) if cross else None, P(buf['d_h0']), C.byref(gr), P(ws),
                                        C.c_size_t(wsb), st))
    names_b = pc.launch_names(dev, bwd)
    for _ in range(calls - 1):
        bwd()
    pc.sync(dev)
    assert resident_launches() - before == resident, 'the backward launched the forward-only resident body'
    host = {k: v.cpu() for k, v in buf.items()}
    n_body = dict(dWn1=d, dWn2=64)
    got = {}
    for k, t in host.items():
        n = n_body.get(k, rows if CLASS_OF[k] != 'w' else 1)
        assert bool((t[n:] == SENTINEL).all()), f'{k}: the guard rows behind the buffer were written'
        got[k] = t[:n] if CLASS_OF[k] != 'w' or k in n_body else t[0]
    assert bool((ws[wsb // 4:] == SENTINEL).all()), 'the guard behind the workspace was written'
    return got, names_f, names_b, resident


def rel_max(got, ref):
    """max|got - ref| / max|ref|; a reference that is zero throughout (skip_weight_h = 0: dWn2, dbn2) wants exact zeros"""
    got, ref = got.double(), ref.double()
    m = float(ref.abs().max())
    if m == 0:
        return float('inf') if float(got.abs().max()) > 0 else 0.0
    return float((got - ref).abs().max()) / m


def rel_l2(got, ref):
    got, ref = got.double(), ref.double()
    n = float(ref.norm())
    return float((got - ref).norm()) / n if n > 0 else (float('inf') if float(got.norm()) > 0 else 0.0)


# ---- bounds -------------------------------------------------------------------------------------------------------
# A bound is FACTOR x the worst distance of the FLOAT32 evaluation of node_reference from its float64 evaluation (fp32
# mode: plain float32; bf16 mode: float32 with the same rounding points, branches and staging) over every case of both
# drivers, per input family and tensor class, rounded up to one significant digit - the reference's own float32
# distance, never the kernels' error.  HISTORY.md holds the measured table next to the kernels' figures;
# tests/test_node_chain_sim.py::test_float32_yardstick re-measures the float32 evaluation over the simulator's cases and
# fails if it exceeds what is recorded here.  Classes: fwd (h_out, y_act, a1n), row (d_h, d_aggr_msg, d_aggr_cross,
# d_h0), w (the six parameter gradients; w_l2 their rel-L2).
#
# bf16 mode has two rounding decisions that the float32 arithmetic before them leaves open:
#  * a1n before the second GEMM.  h_out is compared staged on the kernel's own a1n (class fwd), and end to end from the
#    inputs: at most max(2, 2 % of the rows) rows may hold an element above the staged bound, and every element stays
#    under FACTOR x the worst such deviation of the float32 evaluation (F32_FLIP).
#  * dz before the four dx jobs and the dWn1 GEMMs.  dz is not an output, so nothing can be staged on it.  The raw
#    distance of the row / w classes is held to FACTOR x the float32 evaluation's raw distance (which these flips
#    dominate: ~7e-4), and - the sharp check - the distance in EXCESS of what the open elements can move (class row_x /
#    w_x): an element of dz is open when its float64 value lies within open_eps() x its row's max|dz| of a bf16 tie; it may move its
#    output row by one bf16 spacing times |W|, and exactly that much is subtracted element by element.
FACTOR = 8.0
F32_MEASURED = {     # worst float32-evaluation distance over the cases of both drivers (yardstick(), 256 CUs)
    ('fp32', 'plain'): dict(fwd=8.23e-7, row=5.53e-7, w=8.25e-7, w_l2=5.08e-7),
    ('fp32', 'norm30'): dict(fwd=8.89e-7, row=5.19e-7, w=7.82e-7, w_l2=4.76e-7),
    ('fp32', 'shift'): dict(fwd=2.51e-6, row=7.51e-7, w=1.70e-6, w_l2=1.84e-6),
    ('bf16', 'plain'): dict(row=6.52e-4, w=2.68e-4, w_l2=6.72e-5, dz=4.37e-7),
    ('bf16', 'norm30'): dict(row=8.47e-4, w=8.24e-4, w_l2=1.97e-4, dz=5.83e-7),
    ('bf16', 'shift'): dict(row=6.33e-4, w=6.95e-4, w_l2=1.26e-4, dz=7.52e-7),
}
F32_FLIP = {'plain': 8.74e-4, 'norm30': 6.17e-4, 'shift': 8.94e-4}      # h_out end to end, bf16 mode: worst float32-evaluation deviation
# rows >= 4 096 (GPU driver): the parameter gradients sum over many rows, but the float32 evaluation's distance does not
# grow there (torch sums a long GEMM dimension in blocks; its worst at 4 096 .. 40 000 rows is below its worst at <= 405
# rows in every class), so the bounds carry no growth factor and the kernels have to meet them at every size.
FLIP_ROWS_MIN, FLIP_ROWS_SHARE = 2, 0.02
# The cap is a condition on the inputs, and in the shift family the reference alone breaks it: there a1n's float32
# distance is 3.5 x the plain family's (1.15e-6 against 3.27e-7: a mean far above the spread costs the LayerNorm digits
# in any float32 evaluation), ties are crossed in proportion, and the float32 evaluation of the reference puts 3 of 48
# and 7 of 257 rows beyond the staged bound (cap 2 and 5).  The cap of that family alone is scaled by that ratio, rounded
# up; a body that does not round a1n at all moves every row (mutation 6) and fails it as before.
FLIP_CAP_SCALE = {'plain': 1, 'norm30': 1, 'shift': 4}


def one_digit_up(x):
    import math
    e = math.floor(math.log10(x))
    return math.ceil(x / 10 ** e - 1e-9) * 10 ** e


TOL = {k: {c: one_digit_up(FACTOR * v) for c, v in m.items()} for k, m in F32_MEASURED.items()}
for _fam in FAMILIES:      # bf16 mode: staged h_out, y_act, a1n and the excess classes are held to the fp32-mode bounds -
    # with the operands rounded at the same points and the open roundings accounted for, fp32 summation order is all
    # that is left (the float32 evaluation's own distance there is 3.3e-7 .. 1.2e-6 fwd and <= 2e-7 in excess: smaller)
    TOL['bf16', _fam].update(fwd=TOL['fp32', _fam]['fwd'], row_x=TOL['fp32', _fam]['row'], w_x=TOL['fp32', _fam]['w'])


def open_eps(family):
    """an element of dz is open within 8 x the float32 evaluation's own per-row distance of dz from float64"""
    return TOL['bf16', family]['dz']


def flip_cap(rows, family):
    return FLIP_CAP_SCALE[family] * max(FLIP_ROWS_MIN, int(FLIP_ROWS_SHARE * rows))


def flip_tol(family):
    return one_digit_up(FACTOR * F32_FLIP[family])


# ---- one case -------------------------------------------------------------------------------------------------------


def distances(case, bf16, got, y_act, a1n):
    """Every asserted figure of `got` (13 tensors: the kernels', or the float32 evaluation's) against float64:
    {tensor: max|got - ref64| / max|ref64|}, '<w tensor>:l2', in bf16 mode '<tensor>:x' (the distance in excess of the
    open dz roundings), 'h_out:e2e' (worst element, end to end) and 'h_out:dev' (per-row worst, for the row count)."""
    d, cross = case['cfg']['d'], case['cfg']['cross']
    ref = node_reference(case, bf16, torch.float64, y_act, a1n if bf16 else None)
    out = {}
    for k in NAMES_FWD + NAMES_ROW + NAMES_W:
        if ref[k] is None:
            continue
        g = (got[k][:, :d] if k == 'd_aggr_cross' and got[k].shape[1] > d else got[k]).double()
        out[k] = rel_max(g, ref[k])
        if CLASS_OF[k] == 'w':
            out[k + ':l2'] = rel_l2(g, ref[k])
        if bf16 and k in ref['slack'] and (k != 'd_aggr_cross' or cross):
            m = float(ref[k].abs().max())
            out[k + ':x'] = float(((g - ref[k]).abs() - ref['slack'][k]).clamp(min=0).max()) / m if m > 0 else out[k]
    if 'dz' in got:      # (the float32 evaluation only: dz is not an output of the operator) per row, what open_eps() is 8 x of
        out['dz'] = float(((got['dz'].double() - ref['dz']).abs() / ref['dz'].abs().max(1, keepdim=True).values.clamp(min=1e-300)).max())
    if bf16:
        ref_e = node_reference(case, 1, torch.float64, y_act, None)['h_out']
        dev_rows = ((got['h_out'].double() - ref_e).abs() / float(ref_e.abs().max())).max(1).values
        out['h_out:e2e'], out['h_out:dev'] = float(dev_rows.max()), dev_rows
    return out


def float32_evaluation(case, bf16, y_act, a1n):
    """the yardstick: node_reference in float32 - same inputs, branches, rounding points and staging"""
    r = node_reference(case, bf16, torch.float32, y_act, a1n if bf16 else None)
    if bf16:      # (its end-to-end h_out: not staged)
        r = dict(r, h_out_e2e=node_reference(case, 1, torch.float32, y_act, None)['h_out'])
    return r


def _class_key(k):
    name, _, suffix = k.partition(':')
    return 'dz' if name == 'dz' else CLASS_OF[name] + {'': '', 'l2': '_l2', 'x': '_x'}[suffix]


def check_case(dev, case, bf16, env, cus, calls=1, measure=None):
    """One case under the switches `env` (already in the environment): coverage, guard rows, finiteness, padding, and
    every tensor against float64.  Returns the kernel outputs.  measure: a dict that collects the worst distances of the
    kernels and of the float32 evaluation per (mode, family, class)."""
    cfg, rows, fam = case['cfg'], case['rows'], case['family']
    d, ldc, cross = cfg['d'], cfg['ldc'], cfg['cross']
    mode = 'bf16' if bf16 else 'fp32'
    what = f"{cfg['id']} rows={rows} {fam} {mode}{' drop' if case['mul'] is not None else ''} {env}"
    got, names_f, names_b, resident = run_kernels(dev, case, bf16, calls)
    # ---- coverage: the body that ran ----
    (name_f, body_f), (name_b, body_b) = expected_bodies(env, cfg, bf16, rows, cus)
    assert names_f == [name_f], f'{what}: forward launched {names_f}, expected {name_f} ({body_f})'
    assert names_b and names_b[0] == name_b, f'{what}: backward launched {names_b}, expected {name_b} ({body_b}) first'
    assert resident == (1 if body_f == 'k_rowchain_res_fwd' else 0), f'{what}: {resident} resident launches, body {body_f}'
    # ---- everything the header says is written is finite; the padding of d_aggr_cross ----
    for k in NAMES_FWD + NAMES_ROW + NAMES_W:
        if k != 'd_aggr_cross':
            assert bool(torch.isfinite(got[k]).all()), f'{what}: {k} holds non-finite values'
    if cross:
        dac = got['d_aggr_cross']
        assert bool(torch.isfinite(dac[:, :d]).all()), f'{what}: d_aggr_cross holds non-finite values'
        if ldc > d and d % 4 != 0:      # the header: zeros when d_in is not a multiple of 4, else untouched
            assert bool((dac[:, d:] == 0).all()), f'{what}: padding columns of d_aggr_cross are not exact zeros'
        elif ldc > d:
            assert bool(torch.isnan(dac[:, d:]).all()), f'{what}: padding columns of d_aggr_cross were written'
    else:
        assert bool(torch.isnan(got['d_aggr_cross']).all()), f'{what}: d_aggr_cross written without aggr_cross'
        assert bool((got['dWn1'][:, d + 64:2 * d + 64] == 0).all()), f'{what}: dWn1 aggr_cross block written'
    zr = zero_row(case)
    if zr is not None:      # the all-zero dropout row: z = 0 exactly, variance 0, a1n = ln_b
        assert bool((got['y_act'][zr] == 0).all()) and bool((got['a1n'][zr] == case['lb']).all()), f'{what}: zero row {zr}'
    # ---- against float64 ----
    raw = got
    if calls > 1:      # (accumulated: `calls` backward calls into the same buffers)
        got = dict(got, **{k: got[k] / calls for k in NAMES_W})
    tol = TOL[mode, fam]
    dist = distances(case, bf16, got, got['y_act'], got['a1n'])
    print(what + f': {body_f} / {body_b}\n   ' + ' '.join(f'{k} {v:.1e}' for k, v in dist.items() if k != 'h_out:dev'))
    for k, e in dist.items():
        if k.startswith('h_out:'):
            continue
        cls = _class_key(k)
        bound = tol[cls]
        assert e <= bound, f'{what}: {k} is {e:.3e} of max|ref64| from float64 (bound {bound:.0e})'
    if bf16:
        n_rows = int((dist['h_out:dev'] > tol['fwd']).sum())
        assert n_rows <= flip_cap(rows, fam), f'{what}: {n_rows} rows of h_out beyond {tol["fwd"]:.0e} end to end (cap {flip_cap(rows, fam)})'
        assert dist['h_out:e2e'] <= flip_tol(fam), f'{what}: h_out end to end {dist["h_out:e2e"]:.3e} > {flip_tol(fam):.0e}'
    if measure is not None:
        f32 = float32_evaluation(case, bf16, got['y_act'], got['a1n'])
        d32 = distances(case, bf16, f32, got['y_act'], got['a1n'])
        if bf16:
            dev32 = ((f32['h_out_e2e'].double() - node_reference(case, 1, torch.float64, got['y_act'], None)['h_out']).abs()
                     / float(f32['h_out_e2e'].abs().max())).max(1).values
            d32['h_out:e2e'], d32['h_out:dev'] = float(dev32.max()), dev32
        big = 'rows >= 4096' if rows >= 4096 else ''
        for k in list(dist) + ['dz']:
            if k == 'dz':
                key, vals = (mode, fam, 'dz', ''), (0.0, d32[k])
            elif k == 'h_out:dev':
                key = (mode, fam, 'h_out rows beyond the staged bound / cap', '')
                vals = (int((dist[k] > tol['fwd']).sum()) / flip_cap(rows, fam), int((d32[k] > tol['fwd']).sum()) / flip_cap(rows, fam))
            elif k == 'h_out:e2e':
                key, vals = (mode, fam, 'h_out end to end', ''), (dist[k], d32[k])
            else:
                cls = _class_key(k)
                key, vals = (mode, fam, cls, big if cls.startswith('w') else ''), (dist[k], d32[k])
            m = measure.setdefault(key, [0.0, 0.0])
            m[0], m[1] = max(m[0], vals[0]), max(m[1], vals[1])
        measure.setdefault('bodies', set()).update({(body_f, mode, 'forward'), (body_b, mode, 'backward')})
    return raw


def check_twice(dev, case, bf16, env, cus):
    """the parameter gradients are accumulated: two backward calls into the same buffers give exactly twice one call's"""
    once = check_case(dev, case, bf16, env, cus, calls=1)
    twice = check_case(dev, case, bf16, env, cus, calls=2)
    for k in NAMES_W:
        assert torch.equal(twice[k], 2 * once[k]), f'{k}: two accumulated calls are not twice one call ({env})'
    for k in NAMES_FWD + NAMES_ROW:
        if k != 'd_aggr_cross' or case['cfg']['cross']:
            a, b = once[k], twice[k]
            assert torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)), f'{k} differs between two runs ({env})'


def apply_env(monkeypatch, env):
    for k in SWITCHES:
        if k not in env:
            monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    L.reload_tunables()


def check_bodies_agree(dev, monkeypatch, case, bf16, bodies, cus):
    """the same inputs under several bodies: k_rowchain_res_fwd and k_rowchain<1, false, 1> bit for bit (forward
    tensors), every other pair to the bound each holds against float64 - no looser form-against-form tolerance"""
    res = {}
    for b in bodies:
        apply_env(monkeypatch, BODIES[b])
        got = check_case(dev, case, bf16, BODIES[b], cus)
        res[b] = (got, expected_bodies(BODIES[b], case['cfg'], bf16, case['rows'], cus))
    tol = TOL['bf16' if bf16 else 'fp32', case['family']]
    d = case['cfg']['d']
    names = list(res)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            (ga, (fa, ba)), (gb, (fb, bb)) = res[a], res[b]
            if {fa[1], fb[1]} == {'k_rowchain_res_fwd', 'k_rowchain<1,1>'}:
                for k in NAMES_FWD:
                    assert torch.equal(ga[k], gb[k]), f'{k}: {a} and {b} claim bit identity'
            for k in NAMES_FWD + NAMES_ROW + NAMES_W:
                if k == 'd_aggr_cross' and not case['cfg']['cross']:
                    continue
                x, y = (ga[k][:, :d], gb[k][:, :d]) if k == 'd_aggr_cross' else (ga[k], gb[k])
                if bf16 and k == 'h_out':      # (the two bodies' a1n may round to different bf16 neighbours: flip_tol)
                    assert rel_max(x, y) <= flip_tol(case['family']), (k, a, b)
                    continue
                e = rel_max(x, y)
                assert e <= tol[CLASS_OF[k]], f'{k}: {a} against {b}: {e:.3e} > {tol[CLASS_OF[k]]:.0e}'


# ---- parametrisations -----------------------------------------------------------------------------------------------


def reaches(body, cfg, bf16, rows=33, cus=256):
    """does the parametrisation `body` make this configuration run the body it is named after, forward or backward?"""
    want = dict([('default', None), ('chain-noresident', 'k_rowchain<1,1>'), ('chain-occ1', 'k_rowchain<1,1>'),
                 ('chain-occ2', 'k_rowchain<1,2>'), ('chain-2tiles', 'k_rowchain<2,1>'), ('rowwave', 'k_rowwave'),
                 ('rowres-no80', 'k_rowres')] + [(b, ('k_rowres', 'k_rowres80')) for b in BODIES if b.startswith('rowres') and b != 'rowres-no80'])[body]
    f, b = expected_bodies(BODIES[body], cfg, bf16, rows, cus)
    if want is None:
        return True
    want = want if isinstance(want, tuple) else (want,)
    return f[1] in want or b[1] in want


def thinned_cases(bodies=tuple(BODIES), rows_list=ROW_EDGES):
    """Every body x {fp32, bf16} at every row edge; the configuration, the input family and dropout rotate along the
    row edges (the full cross product is ~50 x as many cases).  Returns (id, body, bf16, config id, rows, family, drop)."""
    out = []
    for bi, body in enumerate(bodies):
        for bf16 in (0, 1):
            ok = [c for c in CONFIGS.values() if reaches(body, c, bf16)]
            assert ok, (body, bf16)
            for ri, rows in enumerate(rows_list):
                cfg = ok[(ri + bi + bf16) % len(ok)]
                fam = FAMILIES[(ri + 2 * bi + bf16) % 3]
                drop = (ri + bi) % 2 == 1
                out.append((f"{body}-{'bf16' if bf16 else 'fp32'}-{cfg['id']}-r{rows}-{fam}{'-drop' if drop else ''}",
                            body, bf16, cfg['id'], rows, fam, drop))
    return out


def rowres_cases():
    out = []
    for i, (body, rows, kind) in enumerate(ROWRES_ROWS):
        for bf16 in (0, 1):
            ok = [c for c in CONFIGS.values() if reaches(body, c, bf16)]
            cfg = ok[(i + 3 * bf16) % len(ok)]
            fam, drop = FAMILIES[(i + bf16) % 3], (i + bf16) % 2 == 0
            out.append((f"{body}-{kind}-{'bf16' if bf16 else 'fp32'}-{cfg['id']}-r{rows}-{fam}{'-drop' if drop else ''}",
                        body, bf16, cfg['id'], rows, fam, drop))
    return out


def report(measure):
    """the measured table of a run: tensor class x mode x family, kernels and float32 evaluation, and the bodies covered"""
    lines = []
    for key in sorted(k for k in measure if k != 'bodies'):
        mode, fam, cls, big = key
        k, f = measure[key]
        lines.append(f'measured {mode:5s} {fam:7s} {cls:5s} {big:3s} kernels {k:.2e}  float32 evaluation {f:.2e}')
    for b in sorted(measure.get('bodies', ())):
        lines.append('covered  %-20s %-5s %s' % b)
    return '\n'.join(lines)


def big_rows(cus):
    """default switches across tiles == CUs, CUs + 1 and the 3 x CUs threshold of k_rowres, and 40 000 rows"""
    return (16 * cus, 16 * cus + 1, 16 * cus + 16, 48 * cus - 16, 48 * cus, 48 * cus + 1, 40000)


def big_cases(cus):
    out = []
    ids = ('64x69', '69x69', '64x64', '64x80', '64x69-nocross')
    for i, rows in enumerate(big_rows(cus)):
        for bf16 in (0, 1):
            cfg, fam, drop = CONFIGS[ids[(i + 2 * bf16) % len(ids)]], FAMILIES[(i + bf16) % 3], (i + bf16) % 2 == 1
            out.append((f"default-{'bf16' if bf16 else 'fp32'}-{cfg['id']}-r{rows}-{fam}{'-drop' if drop else ''}",
                        'default', bf16, cfg['id'], rows, fam, drop))
    return out


def yardstick(cases):
    """The float32 evaluation of node_reference against float64 over `cases`, from the reference alone (its own branches;
    bf16 mode staged on the float64 a1n rounded to float32): {(mode, family, class, row bucket): worst distance} in the
    layout of F32_MEASURED / F32_FLIP / and the worst share of the flip cap the float32 evaluation uses."""
    worst = {}
    for _, _, bf16, cfgid, rows, fam, drop in cases:
        case = make_case(CONFIGS[cfgid], rows, fam, drop)
        r64 = node_reference(case, bf16)
        y_act, a1n = r64['y_act'].float(), r64['a1n'].float()
        f32 = float32_evaluation(case, bf16, y_act, a1n)
        dist = distances(case, bf16, f32, y_act, a1n)
        mode = 'bf16' if bf16 else 'fp32'
        if bf16:
            ref_e = node_reference(case, 1, torch.float64, y_act, None)['h_out']
            dev = ((f32['h_out_e2e'].double() - ref_e).abs() / float(ref_e.abs().max())).max(1).values
            dist['h_out:e2e'] = float(dev.max())
            dist['h_out:cap'] = int((dev > TOL[mode, fam]['fwd']).sum()) / flip_cap(rows, fam)
        dist.pop('h_out:dev', None)
        bucket = 4096 if rows >= 4096 else 0
        for k, e in dist.items():
            cls = k if k.startswith('h_out:') else _class_key(k)
            key = (mode, fam, cls, bucket if cls.startswith('w') else 0)
            worst[key] = max(worst.get(key, 0.0), e)
    return worst


# one case per body (and mode) for the accumulation check, and the sets of bodies compared with each other on one case
TWICE = (('default', 0, '64x69'), ('chain-noresident', 1, '69x69'), ('chain-occ2', 0, '64x4'), ('chain-2tiles', 1, '64x64'),
         ('rowwave', 0, '64x64'), ('rowwave', 1, '64x80'), ('rowres', 0, '64x64'), ('rowres-tps3', 1, '64x64'),
         ('rowres', 1, '69x69'), ('rowres-tps16', 0, '64x64-nocross'))
AGREE = ((0, '64x69', 33, 'plain', ('default', 'chain-noresident', 'chain-occ2', 'chain-2tiles', 'rowwave', 'rowres')),
         (0, '64x64', 257, 'shift', ('default', 'chain-2tiles', 'rowwave', 'rowres', 'rowres-tps16')),
         (1, '64x64', 130, 'norm30', ('default', 'chain-occ2', 'chain-2tiles', 'rowwave', 'rowres', 'rowres-tps3')),
         (1, '69x69', 49, 'plain', ('default', 'chain-2tiles', 'rowres', 'rowres-tps1', 'rowres-no80')))
