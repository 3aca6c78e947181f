"""The weight-gradient GEMMs in float64, and operator checks of every kernel body behind eqd_atb
(csrc/eqd_node_kernels.hip):  out += scale (X * LeakyReLU'(xmask))^T Y  plus the column sums of X, as k_atb + k_atb_reduce.

  general<4|5, fp32|bf16>        any M in 4..80, any alignment: the shifting loaders, 4 or 5 row blocks of 16
  fast<plain|masked>             fp32, M == 64, 16-byte aligned X rows; fast == 1: a whole aligned 64-column block of Y,
                                 fast == 2: a ragged or unaligned block through the shifting loader
  fast_bf<f32|ybf, plain|masked> bf16 mode of the same: two chunks in LDS, one barrier per chunk; ybf: a saved bf16 Y
                                 (whole blocks through the byte permute, ragged ones converted)

Shared by tests/test_atb_sim.py (the x86 simulator build) and tests/test_atb_gpu.py.

The profiler only says `k_atb`, so the host planner (atb_units / atb_next_batch) is restated here (expected_plan): the
body of every unit, the launch split, the parts per unit and the chunks a workgroup walks.  The restatement is pinned to
the library by eqd_atb_partial_bytes() for every case, every case lists the properties it exists for (`props`) and the
driver asserts them from the plan, together with the launch names.

The reference (atb_reference) works in float64 on float64 copies of the float32 inputs; the LeakyReLU factor is ONE
float32 multiply (exact: no rounding decision is open), bf16 mode rounds X * factor and Y where the kernels round them
and takes the column sums from the unrounded values.  The same function in float32 is the yardstick the bounds come
from: a bound is 8 x the distance of that float32 evaluation from float64, never the kernels' own error (DESIGN.md
section 3)."""
import ctypes as C

import torch

from equidock_public_amd import _lib as L
from tests import parity_common as pc
from tests.node_chain_common import one_digit_up, rel_l2, rel_max

SLOPE = 0.01
GUARD_ROWS, SENTINEL = 16, 12345.0
CHUNK, PSTRIDE, MAXUNITS, MAXBLOCKS, TARGET_WGS = 64, 5200, 128, 256, 1024      # ATB_ROWS, ATB_PSTRIDE, ATB_MAXUNITS, ...
ERR_SHAPE, ERR_WORKSPACE = 2, 4
SWITCHES = ('EQD_ATB_WGS', 'EQD_ATB_XCD_ALIGN', 'EQD_ATB_TAIL')
ROW_EDGES = (0, 1, 63, 64, 65, 127, 128, 129, 200)
SCALES = (0.0, 1.0, 0.5, -2.0)
BF16_NAN = 0x7fc0


def job(M, N, rows, **kw):
    """one EqdAtbJob of a case.  xoff / yoff: the operand starts that many floats (4-byte units) past a 16-byte boundary;
    xkey / ykey / okey / bkey: jobs that name the same key share that buffer (None: a buffer of the job's own)"""
    j = dict(M=M, N=N, rows=rows, ldx=M, ldy=N, masked=False, bias=False, bf16=0, ybf=0, scale=1.0, trans=False, xoff=0,
             yoff=0, xkey=None, ykey=None, okey=None, bkey=None)
    assert set(kw) <= set(j), kw
    j.update(kw)
    return j


def _keys(case):
    """the jobs with every buffer key filled in"""
    out = []
    for i, j in enumerate(case['jobs']):
        j = dict(j)
        for k in ('xkey', 'ykey', 'okey'):
            if j[k] is None:
                j[k] = f'{k[0]}{i}'
        j['bkey'] = (j['bkey'] or f'b{i}') if j['bias'] else None
        out.append(j)
    return out


# ---- the host planner restated ------------------------------------------------------------------------------------------


def body_name(u, j):
    if u['fast'] == 0:
        return f"general<{(j['M'] + 15) // 16 if j['M'] > 64 else 4},{'bf16' if j['bf16'] else 'fp32'}>"
    mk = 'masked' if j['masked'] else 'plain'
    return f"fast_bf<{'ybf' if j['ybf'] else 'f32'},{mk}>" if j['bf16'] else f'fast<{mk}>'


def expected_plan(jobs, wgs=None, xcd_align=True):
    """atb_units + atb_next_batch (csrc/eqd_node_kernels.hip) from the shapes alone.  jobs: job() dicts with their keys
    filled in; wgs: the value of EQD_ATB_WGS when it is set (any value switches the doubling rule off; one outside
    64..4096 leaves the target at 1024); xcd_align: False under EQD_ATB_XCD_ALIGN=0.  Returns the launches - lists of
    units (job index, n0, nchunks, fast, body, nparts, walk = the most chunks one of its workgroups walks) -, `per` of
    every launch, the partial floats eqd_atb_partial_bytes must report and the launch names."""
    units = []
    for i, j in enumerate(jobs):
        nchunks = (j['rows'] + CHUNK - 1) // CHUNK if j['rows'] > 0 else 0
        al_x = j['xoff'] % 4 == 0      # (the mask lies at the same offset of its own allocation)
        al_y = j['yoff'] % 4 == 0
        for n0 in range(0, j['N'], CHUNK):
            xfast = j['M'] == 64 and j['rows'] > 0 and j['ldx'] % 4 == 0 and al_x
            if not xfast:
                fast = 0
            elif j['N'] - n0 >= 64 and j['ldy'] % 4 == 0 and al_y:
                fast = 1
            else:
                fast = 2 if (j['N'] - n0 >= 4 or n0 >= 4) else 0
            if j['ybf'] and fast and not j['bf16']:      # the fp32 fast body has no bf16 loader
                fast = 0
            # (not run: an operand of 2 GB and more sends the bf16 fast body's 32-bit byte offsets to the general body)
            if fast and j['bf16'] and (j['rows'] * j['ldx'] * 4 >= 2 ** 31 or j['rows'] * j['ldy'] * 4 >= 2 ** 31):
                fast = 0
            u = dict(job=i, n0=n0, nchunks=nchunks, fast=fast)
            u['body'] = body_name(u, j)
            units.append(u)
    launches, pers, first = [], [], 0
    while first < len(units):
        n = 0
        while first + n < len(units) and n < MAXUNITS:
            c, cj = units[first + n], jobs[units[first + n]['job']]
            clash = False
            for o in units[first:first + n]:
                oj = jobs[o['job']]
                same_tile = oj['okey'] == cj['okey'] and o['n0'] == c['n0']
                same_bias = cj['bkey'] is not None and oj['bkey'] == cj['bkey'] and o['n0'] == 0 and c['n0'] == 0
                clash = clash or same_tile or same_bias
            if clash:
                break
            n += 1
        base = int(wgs) if wgs is not None and 64 <= int(wgs) <= 4096 else TARGET_WGS
        target = base * max(1, (n + 35) // 36)
        if wgs is None and units[first]['nchunks'] > 8 * (target // n):
            target *= 2
        target = min(target, 4096)
        per = (target + n - 1) // n
        if xcd_align and per >= 8:
            per = (per + 7) // 8 * 8
        per = min(per, MAXBLOCKS)
        for u in units[first:first + n]:
            u['nparts'] = min(u['nchunks'], per)
            u['walk'] = -(-u['nchunks'] // u['nparts']) if u['nparts'] else 0
        launches.append(units[first:first + n])
        pers.append(per)
        first += n
    names = []
    for la in launches:
        names += (['k_atb'] if max(u['nparts'] for u in la) > 0 else []) + ['k_atb_reduce']
    floats = max([sum(u['nparts'] for u in la) * PSTRIDE for la in launches] or [0])
    return dict(units=units, launches=launches, per=pers, floats=floats, names=names)


def _prop(plan, jobs, p):
    """one stated property of a case, from its plan"""
    units, key, _, arg = plan['units'], *p.partition(':')
    if key == 'body':
        return any(u['body'] == arg for u in units)
    if key == 'only':      # every unit that has rows runs this body
        return all(u['body'] == arg for u in units if u['nchunks'])
    if key == 'fast':
        return any(u['fast'] == int(arg) for u in units if u['nchunks'])
    if key == 'launches':
        return len(plan['launches']) == int(arg)
    if key == 'walk>=':
        return max(u['walk'] for u in units) >= int(arg)
    if key == 'unequal-walks':      # nparts does not divide nchunks: the workgroups of one unit walk k and k - 1 chunks
        return any(u['nparts'] and u['nchunks'] % u['nparts'] for u in units)
    if key == 'ragged-rows':
        return any(jobs[u['job']]['rows'] % CHUNK for u in units)
    if key == 'early-exit':      # a unit with fewer parts than its launch's grid is wide (c >= u.nparts)
        return any(u['nparts'] < max(v['nparts'] for v in la) for la in plan['launches'] for u in la)
    if key == 'per':
        return int(arg) in plan['per']
    if key == 'per-not-multiple-of-8':
        return any(p_ >= 8 and p_ % 8 for p_ in plan['per'])
    if key == 'per-capped':
        return MAXBLOCKS in plan['per']
    if key == 'split-inside-a-job':      # the 128-unit limit falls between two column blocks of one job
        return any(len(a) == MAXUNITS and a[-1]['job'] == b[0]['job'] for a, b in zip(plan['launches'], plan['launches'][1:]))
    if key == 'units':
        return len(units) == int(arg)
    if key == 'mixed-masks':
        return len({jobs[u['job']]['masked'] for u in units}) == 2
    if key == 'bias-only-first-block':
        return any(jobs[u['job']]['bias'] and u['n0'] > 0 for u in units)
    raise KeyError(p)


def case_plan(case):
    env = case.get('env', {})
    jobs = _keys(case)
    return jobs, expected_plan(jobs, env.get('EQD_ATB_WGS'), env.get('EQD_ATB_XCD_ALIGN') != '0')


def assert_props(case):
    jobs, plan = case_plan(case)
    for p in case['props']:
        assert _prop(plan, jobs, p), f"{case['id']}: the case no longer has the property it exists for: {p}"
    return jobs, plan


# ---- inputs and the reference ------------------------------------------------------------------------------------------


def _rb(t):
    """round to nearest even to bf16, in t's dtype (pack_bf4 of an MFMA operand)"""
    return t.float().to(torch.bfloat16).to(t.dtype)


def make_data(case, seed=17):
    """host tensors of a case: X / mask per xkey, Y per ykey (a saved-bf16 Y holds bf16 values), and the prior contents
    of out per okey ([M][N]) and of bias_out per bkey - non-zero, so that the accumulation is part of every check"""
    gen = torch.Generator().manual_seed(seed)
    d = dict(X={}, mask={}, Y={}, out={}, bias={})
    for j in _keys(case):
        if j['xkey'] not in d['X']:
            d['X'][j['xkey']] = torch.randn(j['rows'], j['M'], generator=gen) * 0.5
            d['mask'][j['xkey']] = torch.randn(j['rows'], j['M'], generator=gen)
        assert d['X'][j['xkey']].shape == (j['rows'], j['M']), 'jobs that share X have the same shape'
        if j['ykey'] not in d['Y']:
            y = torch.randn(j['rows'], j['N'], generator=gen)
            d['Y'][j['ykey']] = _rb(y) if j['ybf'] else y
        assert d['Y'][j['ykey']].shape == (j['rows'], j['N'])
        if j['okey'] not in d['out']:
            d['out'][j['okey']] = torch.randn(j['M'], j['N'], generator=gen)
        if j['bias'] and j['bkey'] not in d['bias']:
            d['bias'][j['bkey']] = torch.randn(j['M'], generator=gen)
    return d


def _tree_sum(t):
    """sum over dim 0 in a fixed pairwise order (elementwise adds only)"""
    while t.shape[0] > 1:
        if t.shape[0] % 2:
            t = torch.cat([t, torch.zeros_like(t[:1])])
        t = t[0::2] + t[1::2]
    return t[0]


def _f32_chunks(t):
    """[rows][c] float32 -> [chunks][64][c], zero rows behind the last one (adding their zeros is exact)"""
    rows, c = t.shape
    n = max(1, -(-rows // CHUNK))
    out = torch.zeros(n * CHUNK, c, dtype=torch.float32)
    out[:rows] = t
    return out.view(n, CHUNK, c)


def f32_product(A, B):
    """A^T B in float32 in a FIXED order, out of elementwise IEEE operations only (a product, then an add: nothing fused,
    nothing that depends on the BLAS build or on the thread count): per 64-row chunk the rows one after the other, then
    the chunks pairwise.  torch's own float32 GEMM moved by 5 x between 2 and 4 threads on these shapes."""
    assert A.dtype == B.dtype == torch.float32
    a, b = _f32_chunks(A), _f32_chunks(B)
    acc = torch.zeros(a.shape[0], A.shape[1], B.shape[1], dtype=torch.float32)
    for r in range(CHUNK):
        acc = acc + a[:, r, :, None] * b[:, r, None, :]
    return _tree_sum(acc)


def f32_colsum(X):
    """column sums in float32 in the same fixed order"""
    x = _f32_chunks(X)
    acc = torch.zeros(x.shape[0], X.shape[1], dtype=torch.float32)
    for r in range(CHUNK):
        acc = acc + x[:, r]
    return _tree_sum(acc)


def atb_reference(case, data, dtype=torch.float64):
    """what eqd_atb leaves in every out [M][N] and bias_out [M], in `dtype` (float64: the reference; float32: the yardstick)"""
    out = {k: v.to(dtype).clone() for k, v in data['out'].items()}
    bias = {k: v.to(dtype).clone() for k, v in data['bias'].items()}
    for j in _keys(case):
        X, Y = data['X'][j['xkey']], data['Y'][j['ykey']]
        # ONE float32 multiply by 1 or slope (atb_store / atb_fast: v *= lrelu_grad(mask, slope)): exact in IEEE arithmetic
        Xe = X * torch.where(data['mask'][j['xkey']] > 0, 1.0, SLOPE).float() if j['masked'] else X
        assert Xe.dtype == torch.float32
        # bf16 mode: both MFMA operands rounded when they are formed (atb_mma<., true> pack_bf4 of a[] and b[]; atb_fast_bf:
        # pack_bf4 of xv / yv as the chunk is written to LDS); a saved-bf16 Y is taken at its stored values in either mode
        A, B = (_rb(Xe), _rb(Y)) if j['bf16'] else (Xe, Y)
        s = j['scale'] if j['scale'] != 0 else 1.0      # (k_atb_reduce: `if (J.scale != 0.f) s *= J.scale`)
        f32 = dtype == torch.float32      # the yardstick: a fixed summation order (f32_product)
        out[j['okey']] += s * (f32_product(A, B) if f32 else A.to(dtype).t() @ B.to(dtype))
        if j['bias']:      # "column sums stay fp32": from the unrounded Xe
            bias[j['bkey']] += s * (f32_colsum(Xe) if f32 else Xe.to(dtype).sum(0))
    return out, bias


def distances(got, ref):
    """{class: worst over the case's buffers}: out = max|got - ref| / max|ref|, out_l2 = rel-L2, bias"""
    (go, gb), (ro, rb_) = got, ref
    d = dict(out=0.0, out_l2=0.0)
    for k in ro:
        d['out'], d['out_l2'] = max(d['out'], rel_max(go[k], ro[k])), max(d['out_l2'], rel_l2(go[k], ro[k]))
    if rb_:
        d['bias'] = max(rel_max(gb[k], rb_[k]) for k in rb_)
    return d


# ---- bounds -------------------------------------------------------------------------------------------------------------
# A bound is FACTOR x the worst distance of the FLOAT32 evaluation of atb_reference (same inputs, same rounding points,
# the fixed summation order of f32_product / f32_colsum: elementwise IEEE operations only, so the figures are the same
# on every machine and at every thread count) from its float64 evaluation over every case of both drivers, per mode and
# class, rounded up to one significant digit - the reference's own float32 distance, never the kernels' error.
# Measured with yardstick() over all_cases(gpu=True) (424 cases: the simulator's and the GPU file's larger ones), kernel
# sources of d1b9fc3; tests/test_atb_sim.py::test_float32_yardstick re-measures it and fails if anything exceeds the
# record.  (An earlier form of the yardstick used torch's float32 GEMM: 6.1e-7 at 1 - 2 threads, 3.3e-6 at 4 and more.)
# Rows >= 4 096 (6 161 .. 16 389 rows) against the cases below that, fp32 / bf16 mode: out 3.1e-7 / 2.3e-7 against
# 5.2e-7 / 3.0e-7, out_l2 1.7e-7 / 1.3e-7 against 2.9e-7 / 1.2e-7, bias 4.0e-7 / 3.0e-7 against 3.1e-7 / 2.9e-7: the
# chunked order does not grow with the row count beyond 1.3 x (64 sequential adds, then a pairwise tree).  The table
# holds the worst over ALL sizes, the bounds carry no growth factor, and the kernels have to meet them at every size.
# Column sums: 5 x, not 8 x - the bound stays at the 2e-6 it had under the torch-sum yardstick, not looser.
FACTOR, FACTOR_BIAS = 8.0, 5.0
F32_MEASURED = {      # yardstick(all_cases(gpu=True)), fixed-order float32 evaluation against float64
    'fp32': dict(out=5.16e-7, out_l2=2.88e-7, bias=3.98e-7),
    'bf16': dict(out=3.02e-7, out_l2=1.33e-7, bias=3.01e-7),
}
TOL = {m: {c: one_digit_up((FACTOR_BIAS if c == 'bias' else FACTOR) * v) for c, v in t.items()} for m, t in F32_MEASURED.items()}


def mode_of(case):
    modes = {bool(j['bf16']) for j in case['jobs']}
    assert len(modes) == 1, 'one mode per case'
    return 'bf16' if modes.pop() else 'fp32'


def yardstick(cases):
    """the float32 evaluation against float64 over `cases`: {(mode, class, rows >= 4096): worst distance}"""
    worst = {}
    for case in cases:
        data = make_data(case)
        d = distances(atb_reference(case, data, torch.float32), atb_reference(case, data))
        big = max(j['rows'] for j in case['jobs']) >= 4096
        for c, e in d.items():
            k = (mode_of(case), c, big)
            worst[k] = max(worst.get(k, 0.0), e)
    return worst


# ---- the operator -------------------------------------------------------------------------------------------------------


def _embed(dev, mat, ld, off, bf16=False):
    """`mat` as rows of stride `ld` inside a larger allocation: GUARD_ROWS rows of NaN before and after, NaN in the
    padding columns, the first element `off` 4-byte units past a 16-byte boundary.  Returns (buffer, address)."""
    rows, cols = mat.shape
    assert ld >= cols
    per4 = 2 if bf16 else 1      # elements per 4 bytes
    n = (rows + 2 * GUARD_ROWS) * ld + (off + 4) * per4
    if bf16:
        buf = torch.full((n,), BF16_NAN, dtype=torch.int16)      # (0x7fc0: a bf16 NaN)
        mat = mat.to(torch.bfloat16).view(torch.int16)
    else:
        buf = torch.full((n,), float('nan'), dtype=torch.float32)
    start = GUARD_ROWS * ld + off * per4
    if rows:
        buf[start:start + rows * ld].view(rows, ld)[:, :cols] = mat
    buf = buf.to(dev)
    assert buf.data_ptr() % 16 == 0 and (GUARD_ROWS * ld * buf.element_size()) % 16 == 0
    return buf, buf.data_ptr() + start * buf.element_size()


OUT_PAD_R, OUT_PAD_C, BIAS_PAD = 2, 3, 8


def _out_buffer(dev, init, trans):
    """the [M][N] block (stored [N][M] when trans) inside a wider sentinel-filled matrix; returns (buffer, address, o_rs, o_cs)"""
    blk = init.t() if trans else init
    r, c = blk.shape
    buf = torch.full((r + 2 * OUT_PAD_R, c + 2 * OUT_PAD_C), SENTINEL, dtype=torch.float32)
    buf[OUT_PAD_R:OUT_PAD_R + r, OUT_PAD_C:OUT_PAD_C + c] = blk
    buf = buf.to(dev)
    w = buf.shape[1]
    return (buf, buf.data_ptr() + 4 * (OUT_PAD_R * w + OUT_PAD_C)) + ((1, w) if trans else (w, 1))


def _out_read(buf, trans, what):
    """the block back on the host as [M][N]; everything around it must still be the sentinel, bit for bit"""
    h = buf.cpu().clone()
    blk = h[OUT_PAD_R:h.shape[0] - OUT_PAD_R, OUT_PAD_C:h.shape[1] - OUT_PAD_C].clone()
    h[OUT_PAD_R:h.shape[0] - OUT_PAD_R, OUT_PAD_C:h.shape[1] - OUT_PAD_C] = SENTINEL
    assert bool((h == SENTINEL).all()), f'{what}: written outside [M] x [N]'
    return blk.t() if trans else blk


class Device:
    """the buffers of one case on `dev` and its EqdAtbJob array"""

    def __init__(self, dev, case, data):
        self.dev, self.case, self.jobs = dev, case, _keys(case)
        self.keep, self.out, self.bias = [], {}, {}
        xs, ys = {}, {}
        arr = (L.EqdAtbJob * max(1, len(self.jobs)))()
        for i, j in enumerate(self.jobs):
            if j['xkey'] not in xs:
                xb, xp = _embed(dev, data['X'][j['xkey']], j['ldx'], j['xoff'])
                mb, mp = _embed(dev, data['mask'][j['xkey']], j['ldx'], j['xoff'])
                xs[j['xkey']] = (xp, mp, j['ldx'], j['xoff'])
                self.keep += [xb, mb]
            assert xs[j['xkey']][2:] == (j['ldx'], j['xoff'])
            if j['ykey'] not in ys:
                yb, yp = _embed(dev, data['Y'][j['ykey']], j['ldy'], j['yoff'], bool(j['ybf']))
                ys[j['ykey']] = (yp, j['ldy'], j['yoff'], j['ybf'])
                self.keep.append(yb)
            assert ys[j['ykey']][1:] == (j['ldy'], j['yoff'], j['ybf'])
            if j['okey'] not in self.out:
                self.out[j['okey']] = _out_buffer(dev, data['out'][j['okey']], j['trans']) + (j['trans'],)
            assert self.out[j['okey']][4] == j['trans']
            if j['bias'] and j['bkey'] not in self.bias:
                b = torch.full((j['M'] + 2 * BIAS_PAD,), SENTINEL, dtype=torch.float32)
                b[BIAS_PAD:BIAS_PAD + j['M']] = data['bias'][j['bkey']]
                self.bias[j['bkey']] = b.to(dev)
            A = arr[i]
            A.X, A.xmask, A.ldx, A.M = xs[j['xkey']][0], (xs[j['xkey']][1] if j['masked'] else None), j['ldx'], j['M']
            A.Y, A.ldy, A.N, A.rows = ys[j['ykey']][0], j['ldy'], j['N'], j['rows']
            A.out, A.o_rs, A.o_cs = self.out[j['okey']][1:4]
            A.bias_out = self.bias[j['bkey']].data_ptr() + 4 * BIAS_PAD if j['bias'] else None
            A.slope, A.scale, A.bf16, A.y_bf16 = SLOPE, j['scale'], j['bf16'], j['ybf']
        self.arr, self.n = arr, len(self.jobs)

    def partial_bytes(self):
        return int(pc.lib().eqd_atb_partial_bytes(self.arr, self.n))

    def call(self, part, nbytes):
        return pc.lib().eqd_atb(self.arr, self.n, pc.P(part), C.c_size_t(nbytes), pc.st(self.dev))

    def read(self):
        what = self.case['id']
        out = {k: _out_read(v[0], v[4], f'{what} out {k}') for k, v in self.out.items()}
        bias = {}
        for k, b in self.bias.items():
            h = b.cpu()
            assert bool((h[:BIAS_PAD] == SENTINEL).all()) and bool((h[-BIAS_PAD:] == SENTINEL).all()), f'{what}: bias_out {k} guards'
            bias[k] = h[BIAS_PAD:-BIAS_PAD].clone()
        return out, bias


def run_kernels(dev, case, data, plan):
    """one eqd_atb call of the case from fresh buffers: the partial workspace NaN-filled with 64 sentinel floats behind
    what the library asked for.  Returns ((out, bias) on the host, launch names)."""
    D = Device(dev, case, data)
    nb = D.partial_bytes()
    assert nb == 4 * plan['floats'] + 256, f"{case['id']}: eqd_atb_partial_bytes {nb} != 4 x {plan['floats']} + 256: expected_plan is not the library's planner"
    part = torch.full((nb // 4 + 64,), float('nan'), dtype=torch.float32)
    part[nb // 4:] = SENTINEL
    part = part.to(dev)
    names = pc.launch_names(dev, lambda: L.check(D.call(part, nb)))
    pc.sync(dev)
    assert bool((part[nb // 4:] == SENTINEL).all()), f"{case['id']}: written behind the partial workspace"
    return D.read(), names


def check_case(dev, case, measure=None, twice=False):
    """One case (its switches already in the environment): the stated properties and the launch names from the plan,
    the guards, finiteness, and every out / bias_out against float64.  twice: a second run from the same initial buffers
    must give the same bits (no atomics)."""
    jobs, plan = assert_props(case)
    mode = mode_of(case)
    data = make_data(case)
    got, names = run_kernels(dev, case, data, plan)
    assert names == plan['names'], f"{case['id']}: launched {names}, expected {plan['names']}"
    for k, t in list(got[0].items()) + list(got[1].items()):
        assert bool(torch.isfinite(t).all()), f"{case['id']}: {k} holds non-finite values (a row or column beyond the matrix not zeroed)"
    dist = distances(got, atb_reference(case, data))
    print(f"{case['id']} [{mode}] " + ' '.join(sorted({u['body'] for u in plan['units'] if u['nchunks']})) + ': ' +
          ' '.join(f'{k} {v:.1e}' for k, v in dist.items()))
    for c, e in dist.items():
        assert e <= TOL[mode][c], f"{case['id']}: {c} is {e:.3e} of max|ref64| from float64 (bound {TOL[mode][c]:.0e})"
    if measure is not None:
        d32 = distances(atb_reference(case, data, torch.float32), atb_reference(case, data))
        for c, e in dist.items():
            m = measure.setdefault((mode, c), [0.0, 0.0])
            m[0], m[1] = max(m[0], e), max(m[1], d32[c])
        measure.setdefault('bodies', set()).update(u['body'] for u in plan['units'] if u['nchunks'])
    if twice:
        again, _ = run_kernels(dev, case, data, plan)
        for a, b in zip(got, again):
            for k in a:
                assert torch.equal(a[k], b[k]), f"{case['id']}: {k} differs between two runs from the same buffers"
    return got


def report(measure):
    lines = []
    for key in sorted(k for k in measure if k != 'bodies'):
        k, f = measure[key]
        lines.append(f'measured {key[0]:5s} {key[1]:7s} kernels {k:.2e}  float32 evaluation {f:.2e}  bound {TOL[key[0]][key[1]]:.0e}')
    for b in sorted(measure.get('bodies', ())):
        lines.append(f'covered  {b}')
    return '\n'.join(lines)


def apply_env(monkeypatch, env):
    for k in SWITCHES:
        if k not in env:
            monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    L.reload_tunables()


# ---- cases --------------------------------------------------------------------------------------------------------------
# Row edges: a single job at every rows in ROW_EDGES (chunk = 64 rows) for each configuration below; the mask, bias_out,
# the scale and the transposed output rotate along the row edges, so every body runs masked and plain, with and
# without the column sums.
def _edge_configs():
    gen = [dict(M=4, N=4), dict(M=16, N=20), dict(M=69, N=64), dict(M=69, N=69), dict(M=80, N=64), dict(M=80, N=271),
           dict(M=64, N=64, xoff=1), dict(M=64, N=64, ldx=69)]
    fastn = [dict(M=64, N=n) for n in (64, 128, 192, 65, 67, 69, 131)] + \
        [dict(M=64, N=64, ldy=65), dict(M=64, N=64, yoff=1), dict(M=64, N=128, ldx=72)]
    out = [('general-fp32', dict(c, bf16=0)) for c in gen] + [('general-bf16', dict(c, bf16=1)) for c in gen]
    out += [('general-ybf-fp32', dict(M=64, N=64, ldy=64, ybf=1, bf16=0)), ('general-ybf-fp32', dict(M=69, N=69, ldy=72, ybf=1, bf16=0))]
    out += [('fast-fp32', dict(c, bf16=0)) for c in fastn] + [('fast_bf-f32', dict(c, bf16=1)) for c in fastn]
    out += [('fast_bf-ybf', dict(M=64, N=n, ldy=ld, ybf=1, bf16=1)) for n, ld in ((64, 64), (128, 128), (69, 72), (68, 68), (132, 136))]
    return out


def _edge_props(group, c, masked):
    """what a row-edge configuration exists for (checked for every rows > 0)"""
    mk = 'masked' if masked else 'plain'
    mode = 'bf16' if c['bf16'] else 'fp32'
    if group.startswith('general'):
        return [f"only:general<{5 if c['M'] > 64 else 4},{mode}>"]
    body = {'fast-fp32': f'fast<{mk}>', 'fast_bf-f32': f'fast_bf<f32,{mk}>', 'fast_bf-ybf': f'fast_bf<ybf,{mk}>'}[group]
    n, ldy = c['N'], c.get('ldy', c['N'])
    whole = ldy % 4 == 0 and c.get('yoff', 0) == 0
    props = [f'only:{body}']
    if whole and n >= 64:
        props.append('fast:1')      # whole aligned blocks (a saved-bf16 Y: the byte-permute path)
    if not whole or n % 64:
        props.append('fast:2')      # ragged or unaligned blocks (a saved-bf16 Y: the converted path)
    return props


def edge_cases(groups=None):
    out = []
    for ci, (group, c) in enumerate(_edge_configs()):
        if groups is not None and group not in groups:
            continue
        for ri, rows in enumerate(ROW_EDGES):
            k = ri + ci
            masked, bias = k % 2 == 1, (k // 2) % 2 == 1
            j = job(rows=rows, masked=masked, bias=bias, scale=SCALES[k % 4], trans=k % 3 == 0, **c)
            tag = '-'.join(f'{a}{v}' for a, v in c.items() if a not in ('bf16', 'ybf'))
            cid = f"{group}-{tag}-r{rows}{'-masked' if masked else ''}{'-bias' if bias else ''}-s{SCALES[k % 4]:g}{'-T' if k % 3 == 0 else ''}"
            out.append(dict(id=cid, group=group, jobs=[j], props=_edge_props(group, c, masked) if rows else ['launches:1']))
    return out


EDGE_GROUPS = ('general-fp32', 'general-bf16', 'general-ybf-fp32', 'fast-fp32', 'fast_bf-f32', 'fast_bf-ybf')
FAMILIES = {      # body family -> (M, mode, saved-bf16 Y, the bodies its masked and plain units run)
    'general-fp32': dict(M=69, bf16=0, ybf=0, bodies=('general<5,fp32>',)),
    'general-bf16': dict(M=69, bf16=1, ybf=0, bodies=('general<5,bf16>',)),
    'fast-fp32': dict(M=64, bf16=0, ybf=0, bodies=('fast<plain>', 'fast<masked>')),
    'fast_bf-f32': dict(M=64, bf16=1, ybf=0, bodies=('fast_bf<f32,plain>', 'fast_bf<f32,masked>')),
    'fast_bf-ybf': dict(M=64, bf16=1, ybf=1, bodies=('fast_bf<ybf,plain>', 'fast_bf<ybf,masked>')),
}


def shared_x_jobs(fam, units, rows, ragged_job=True):
    """`units` units in one call that share X (and its mask), as the model's calls do: jobs of one 64-column block each,
    four different Y among them, masked and plain units mixed, every third with column sums, the scales rotating - and,
    with ragged_job, one 69-wide Y (two units: a whole block and one of 5 columns) in the middle"""
    f = FAMILIES[fam]
    ldy = 72 if f['ybf'] else 69
    jobs, n = [], 0
    while n < units:
        i = len(jobs)
        wide = ragged_job and n == units // 2 and units - n >= 2
        jobs.append(job(f['M'], 69 if wide else 64, rows, ldy=ldy if wide else 64, masked=i % 3 == 1, bias=i % 3 == 0,
                        scale=SCALES[i % 4], trans=i % 5 == 2, bf16=f['bf16'], ybf=f['ybf'], xkey='x',
                        ykey='ywide' if wide else f'y{i % 4}'))
        n += 2 if wide else 1
    return jobs


def many_unit_cases(gpu=False):
    """Three and more chunks per workgroup with unequal walks.  With n <= 36 units the planner gives per = ceil(1024 / n)
    rounded up to a multiple of 8: 32 units -> per = 32, and rows = 64 x 32 x 3 + 17 = 6 161 make 97 chunks, so workgroup 0
    of every unit walks 4 chunks and the others 3, the last chunk ragged.  (From 37 units on the target doubles - 1024 x
    ceil(n / 36) -: 40 units give per = 56, and the same walks need 64 x 56 x 3 + 17 = 10 769 rows; that size runs on
    the device only.)"""
    out = []
    for fam, f in FAMILIES.items():
        props = ['units:32', 'per:32', 'walk>=:4', 'unequal-walks', 'ragged-rows', 'mixed-masks', 'launches:1'] + [f'body:{b}' for b in f['bodies']]
        out.append(dict(id=f'shared-x-32-units-{fam}', jobs=shared_x_jobs(fam, 32, 64 * 32 * 3 + 17), props=props))
        if gpu:
            props = ['units:40', 'per:56', 'walk>=:4', 'unequal-walks', 'ragged-rows', 'mixed-masks', 'launches:1'] + [f'body:{b}' for b in f['bodies']]
            out.append(dict(id=f'shared-x-40-units-{fam}', jobs=shared_x_jobs(fam, 40, 64 * 56 * 3 + 17), props=props))
    # EQD_ATB_WGS = 64: 8 units -> per = 8; 1 537 rows = 25 chunks: walks of 4 and 3
    for fam in ('general-bf16', 'fast-fp32', 'fast_bf-ybf'):
        out.append(dict(id=f'wgs64-8-units-{fam}', env={'EQD_ATB_WGS': '64'}, jobs=shared_x_jobs(fam, 8, 1537),
                        props=['units:8', 'per:8', 'walk>=:4', 'unequal-walks', 'ragged-rows', 'launches:1']))
    # EQD_ATB_WGS = 4096: 20 units -> ceil(4096 / 20) = 205, rounded up to 208; EQD_ATB_XCD_ALIGN = 0 leaves 147 for 7 units
    # and 205 for the 20.  One unit has 64 x per + 5 rows - one chunk more than parts, so its workgroup 0 walks two and a
    # wrong rounding of per shows in nparts -, the others are small (the cost of a case is units x chunks)
    def one_long(fam, units, per):
        f = FAMILIES[fam]
        return [job(f['M'], 64, 64 * per + 5 if i == 1 else 70 + i, masked=i % 3 == 1, bias=i % 3 != 2, scale=SCALES[i % 4],
                    bf16=f['bf16'], ybf=f['ybf']) for i in range(units)]
    out.append(dict(id='wgs4096-20-units-fast_bf-f32', env={'EQD_ATB_WGS': '4096'}, jobs=one_long('fast_bf-f32', 20, 208),
                    props=['units:20', 'per:208', 'walk>=:2', 'unequal-walks', 'ragged-rows', 'early-exit']))
    out.append(dict(id='xcd0-7-units-fast-fp32', env={'EQD_ATB_XCD_ALIGN': '0'}, jobs=one_long('fast-fp32', 7, 147),
                    props=['units:7', 'per:147', 'per-not-multiple-of-8', 'walk>=:2', 'unequal-walks']))
    out.append(dict(id='wgs4096-xcd0-20-units-general-fp32', env={'EQD_ATB_WGS': '4096', 'EQD_ATB_XCD_ALIGN': '0'},
                    jobs=one_long('general-fp32', 20, 205),
                    props=['units:20', 'per:205', 'per-not-multiple-of-8', 'walk>=:2', 'unequal-walks']))
    return out


def planner_cases():
    out = []
    # jobs of 1, 3 and 40 chunks in one call: per is capped at 256, so nparts = 1, 3, 40 and the grid is 40 wide - 39 and 37
    # workgroups of the small units leave at `c >= u.nparts`
    for fam, f in FAMILIES.items():
        jobs = [job(f['M'], 64, r, masked=i == 1, bias=i != 1, scale=SCALES[i + 1], bf16=f['bf16'], ybf=f['ybf'])
                for i, r in enumerate((50, 190, 2500))]
        out.append(dict(id=f'mixed-sizes-{fam}', jobs=jobs, props=['early-exit', 'per-capped', 'launches:1', 'units:3']))
    # one unit of 257 chunks: per = 1024 is capped at ATB_MAXBLOCKS = 256 parts, workgroup 0 walks two chunks
    for fam in ('fast-fp32', 'general-bf16'):
        f = FAMILIES[fam]
        out.append(dict(id=f'per-cap-one-unit-{fam}', jobs=[job(f['M'], 64, 64 * 256 + 5, bias=True, masked=True, bf16=f['bf16'])],
                        props=['units:1', 'per-capped', 'walk>=:2', 'unequal-walks']))
    # shared-weight layers: two / three jobs accumulate into the same out -> that many launches, and the sum
    for fam, k in (('fast-fp32', 2), ('general-bf16', 3), ('fast_bf-ybf', 3), ('general-fp32', 2)):
        f = FAMILIES[fam]
        jobs = [job(f['M'], 131 if f['ybf'] == 0 else 132, 150 + 37 * i, ldy=131 if f['ybf'] == 0 else 136, masked=i == 1,
                    bias=True, scale=SCALES[(i + 1) % 4], trans=k == 3, bf16=f['bf16'], ybf=f['ybf'], okey='w', bkey='b')
                for i in range(k)]
        out.append(dict(id=f'same-out-{k}-jobs-{fam}', jobs=jobs, props=[f'launches:{k}', f'units:{3 * k}']))
    # two jobs that share only bias_out
    for fam in ('fast_bf-f32', 'general-fp32'):
        f = FAMILIES[fam]
        jobs = [job(f['M'], 64, 100 + 30 * i, bias=True, scale=(0.5, -2.0)[i], bf16=f['bf16'], bkey='b') for i in range(2)]
        out.append(dict(id=f'same-bias-only-{fam}', jobs=jobs, props=['launches:2', 'units:2']))
    # 130 units: 43 jobs of three column blocks + one of one; the 128-unit limit falls behind the second block of job 42
    for fam in ('fast-fp32', 'fast_bf-f32'):
        f = FAMILIES[fam]
        jobs = [job(64, 192, 70, masked=i % 2 == 1, bias=i % 4 == 0, scale=SCALES[i % 4], bf16=f['bf16'], xkey='x', ykey=f'y{i % 3}')
                for i in range(43)] + [job(64, 64, 70, bf16=f['bf16'], xkey='x', ykey='ylast', bias=True)]
        out.append(dict(id=f'130-units-{fam}', jobs=jobs, props=['units:130', 'launches:2', 'split-inside-a-job']))
    # N = 271 with bias_out: five column blocks, only the n0 == 0 unit may write the column sums
    for M, bf16 in ((80, 0), (64, 0), (64, 1), (69, 1)):
        out.append(dict(id=f"n271-bias-M{M}-{'bf16' if bf16 else 'fp32'}", jobs=[job(M, 271, 333, bias=True, masked=True, scale=0.5, bf16=bf16, ldy=271 if M != 64 else 272)],
                        props=['units:5', 'bias-only-first-block', 'launches:1']))
    # every scale, normal and transposed output, on one body each
    for fam in ('general-fp32', 'fast_bf-ybf'):
        f = FAMILIES[fam]
        jobs = [job(f['M'], 64, 130, bias=True, scale=s, trans=t, bf16=f['bf16'], ybf=f['ybf'], xkey='x') for s in SCALES for t in (False, True)]
        out.append(dict(id=f'scales-and-strides-{fam}', jobs=jobs, props=['units:8', 'launches:1']))
    return out


def all_cases(gpu=False):
    return edge_cases() + many_unit_cases(gpu) + planner_cases()


# ---- contract errors -----------------------------------------------------------------------------------------------------


def check_contract_errors(dev):
    """every refusal returns before any launch: the error code, no launch, nothing written"""
    good = job(64, 64, 100, bias=True)
    bad = [('M=3', dict(good, M=3, ldx=3), ERR_SHAPE), ('M=81', dict(good, M=81, ldx=81), ERR_SHAPE),
           ('N=3', dict(good, N=3, ldy=3), ERR_SHAPE), ('rows=-1', dict(good), ERR_SHAPE),
           ('y_bf16 ldy%4', dict(good, ybf=1, bf16=1, N=66, ldy=66), ERR_SHAPE),
           ('y_bf16 Y 4 bytes off', dict(good, ybf=1, bf16=1, yoff=1), ERR_SHAPE),
           ('workspace 4 bytes short', dict(good), ERR_WORKSPACE), ('partial NULL', dict(good), ERR_WORKSPACE)]
    for what, j, code in bad:
        # (a good job first: the refusal of job 1 must come before job 0 is launched)
        case = dict(id='contract ' + what, jobs=[dict(good), j], props=[])
        data = make_data(case)
        D = Device(dev, case, data)
        if what == 'rows=-1':
            D.arr[1].rows = -1
        before = D.read()
        part = torch.full((4 * PSTRIDE + 64,), SENTINEL, dtype=torch.float32).to(dev)
        nbytes = 4 * part.numel()
        if code == ERR_WORKSPACE:      # two units of two chunks each: 4 x 5200 floats
            assert D.partial_bytes() == 4 * 4 * PSTRIDE + 256
            if what != 'partial NULL':
                nbytes = 4 * 4 * PSTRIDE - 4
        else:
            assert D.partial_bytes() == 0, what      # (the size query refuses the same jobs)
        rc = []
        names = pc.launch_names(dev, lambda: rc.append(D.call(None if what == 'partial NULL' else part, nbytes)))
        pc.sync(dev)
        assert rc == [code], f'{what}: eqd_atb returned {rc}, expected {code}'
        assert names == [], f'{what}: launched {names} before refusing'
        after = D.read()
        for a, b in zip(before, after):
            for k in a:
                assert torch.equal(a[k], b[k]), f'{what}: {k} written by a refused call'
        assert bool((part == SENTINEL).all()), f'{what}: the workspace was written by a refused call'


# ---- bodies agree ---------------------------------------------------------------------------------------------------------
# The same job on two bodies.  Bit equality is demanded only where the code sums in the same order:
#  * a saved-bf16 Y against an fp32 tensor that holds the same values, on the SAME body: ld4_bf16_fix (general body) puts
#    the same fp32 values into the Y tile, and atb_fast_bf<true, .> writes the same bf16 groups to LDS as pack_bf4 of
#    those values (an exact value rounds to itself; the byte permute only moves the halves), the MFMA sequence is the
#    same -> equal bits, in bf16 mode on both bodies and in fp32 mode on the general body.
#  * M = 64 aligned (fast bodies) against the same X 4 bytes off (general body): the general body feeds an MFMA the rows
#    4 (ks + u) + g of a chunk, u = 0..7 - rows 0..31 then 32..63 -, atb_fast_bf the k-groups tr, tr + 16, tr + 32,
#    tr + 48 - rows {0..7, 16..23, 32..39, 48..55} then the rest -; fp32 mode: the same MFMA order, but the column sums
#    are taken per wave and added pairwise in the fast body, row by row in the general one.  Different orders: both
#    are held to their float64 bound, no form-against-form tolerance.
#  * fp32 mode, a saved-bf16 Y with M = 64 aligned runs the general body (forced), the fp32 tensor the fast one: bound.
AGREE = (
    ('ybf-vs-f32-fast_bf', dict(M=64, N=132, ldy=136, bf16=1, masked=True), dict(ybf=1), dict(ybf=0), True),
    ('ybf-vs-f32-general-bf16', dict(M=69, N=69, ldy=72, bf16=1, masked=True), dict(ybf=1), dict(ybf=0), True),
    ('ybf-vs-f32-general-fp32', dict(M=69, N=69, ldy=72, bf16=0), dict(ybf=1), dict(ybf=0), True),
    ('ybf-general-vs-f32-fast-fp32', dict(M=64, N=64, ldy=64, bf16=0), dict(ybf=1), dict(ybf=0), False),
    ('aligned-vs-4-bytes-off-fp32', dict(M=64, N=131, bf16=0, masked=True), dict(xoff=0), dict(xoff=1), False),
    ('aligned-vs-4-bytes-off-bf16', dict(M=64, N=131, bf16=1), dict(xoff=0), dict(xoff=1), False),
)


def check_bodies_agree(dev, name, base, va, vb, bits, rows=333):
    cases = [dict(id=f'{name}-{i}', jobs=[job(rows=rows, bias=True, scale=0.5, **dict(base, **v))], props=[]) for i, v in enumerate((va, vb))]
    data = make_data(dict(cases[0], jobs=[dict(cases[0]['jobs'][0], ybf=1)]))      # bf16 values of Y for both
    res, bodies = [], []
    for case in cases:
        jobs, plan = case_plan(case)
        bodies.append({u['body'] for u in plan['units']})
        got, _ = run_kernels(dev, case, data, plan)
        dist = distances(got, atb_reference(case, data))
        for c, e in dist.items():
            assert e <= TOL[mode_of(case)][c], f"{case['id']}: {c} {e:.3e} > {TOL[mode_of(case)][c]:.0e}"
        res.append(got)
    same_body = bodies[0] == bodies[1] or {b.replace('ybf', 'f32') for b in bodies[0]} == bodies[1]
    assert same_body == bits, f'{name}: bodies {bodies}'
    if bits:
        for a, b in zip(*res):
            for k in a:
                assert torch.equal(a[k], b[k]), f'{name}: {k} differs between {bodies[0]} and {bodies[1]}'


# ---- the ride-along tails, on against off ------------------------------------------------------------------------------
# With EQD_ATB_TAIL=0 the end of the backward is k_linear (d h[0]) -> k_embed_bwd -> k_atb ...; by default, at sizes where
# eqd_atb_tail_wanted holds (one row tile per workgroup, no LDS-resident row kernels: small batches), the linear job runs as
# trailing workgroups of the first k_atb and the embedding partials as trailing workgroups of the first k_atb_reduce.  Both
# forms run the same bodies on the same tiles - linear_tile<1> on 16-row tile b, embed_bwd_body on 16-node block b, the
# partials reduced through the same deferred list - so every output and every element of the flat gradient must have the
# same bits.  (Reading the code shows no order difference: the weight-gradient units themselves are planned alike, the
# tails only add grid rows behind them.)
TAIL_CONFIGS = {
    'fp32-2-layers': dict(over=dict(iegmn_n_lays=2), sizes=((30, 34), (32, 32)), atb_launches=1),
    'bf16-2-layers': dict(over=dict(iegmn_n_lays=2, hip_storage_dtype='bf16'), sizes=((30, 34), (32, 32)), atb_launches=1),
    'shared-layers': dict(over=dict(iegmn_n_lays=5, shared_layers=True), sizes=((14, 18), (16, 16)), atb_launches=2),
    'over-128-units': dict(over=dict(iegmn_n_lays=12), sizes=((14, 18), (16, 16)), atb_launches=2),
    'nodes-not-multiple-of-16': dict(over=dict(iegmn_n_lays=2), sizes=((29, 33), (31, 30)), atb_launches=1),
}


def _model_step(dev, args, sizes):
    from equidock_public_amd import graph as G
    from equidock_public_amd import synthetic
    from oracle import iegmn_port as port
    net = pc.build_model(args, port.init_state_dict(args, seed=4), dev)
    g = G.batch_pairs(synthetic.make_pairs(list(sizes), 21)).to(dev)
    flat = net.iegmn_original.enable_flat_grads()
    lib_ = pc.lib()
    L.profiling = True
    L.check(lib_.eqd_profile_begin(pc.st(dev), 1024))
    try:
        outs = net.forward_batched(g)
        (outs[0].square().sum() + outs[1].square().sum() + outs[2].square().sum()).backward()
        pc.sync(dev)
    finally:
        n = lib_.eqd_profile_end()
        L.profiling = False
    assert 0 < n < 1024
    names = [lib_.eqd_profile_name(i).decode() for i in range(n)]
    return [o.detach().cpu().clone() for o in outs], flat.detach().cpu().clone(), names


def check_tails(dev, monkeypatch, name):
    from oracle import iegmn_port as port
    cfg = TAIL_CONFIGS[name]
    args = dict(port.default_args(skip_weight_h=0.75), **cfg['over'])
    assert sum(a + b for a, b in cfg['sizes']) % 16 == (11 if name.startswith('nodes-not') else 0)
    res = {}
    try:
        for mode in ('off', 'on'):
            apply_env(monkeypatch, {'EQD_ATB_TAIL': '0'} if mode == 'off' else {})
            res[mode] = _model_step(dev, args, cfg['sizes'])
    finally:
        apply_env(monkeypatch, {})
    (oa, fa, na), (ob, fb, nb) = res['off'], res['on']
    first = na.index('k_atb')
    assert na[first - 2:first] == ['k_linear', 'k_embed_bwd'], f'{name}: tails off: {na[first - 3:first + 1]} before the first k_atb'
    fb_ = nb.index('k_atb')
    assert nb[fb_ - 1] not in ('k_linear', 'k_embed_bwd') and nb[fb_ - 2] not in ('k_linear', 'k_embed_bwd'), f'{name}: tails on: {nb[fb_ - 2:fb_ + 1]}'
    assert 'k_embed_bwd' not in nb, f'{name}: tails on still launches k_embed_bwd'
    rest = list(na)
    del rest[first - 2:first]
    assert rest == nb, f'{name}: the two forms differ in more than the two tail launches'
    assert na.count('k_atb') == nb.count('k_atb') and (na.count('k_atb') >= cfg['atb_launches']), (name, na.count('k_atb'))
    if name == 'over-128-units':
        assert na.count('k_atb') >= 2
    assert float(fa.abs().sum()) > 0 and bool(torch.isfinite(fa).all())
    for i, (a, b) in enumerate(zip(oa, ob)):
        assert torch.equal(a, b), f'{name}: output {i} differs between the tails on and off'
    diff = (fa != fb).nonzero().flatten()
    assert diff.numel() == 0, f'{name}: {diff.numel()} of {fa.numel()} flat-gradient elements differ between the tails on and off (first at {int(diff[0])})'
