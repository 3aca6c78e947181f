"""Phase stamps inside ONE launch of the resident forward node chain on 3 200 rows (workload B's node count), through
eqd_selftest_node_chain_fwd: form 0 (two jobs), 1 (+ the head's job), 5 (+ the next layer's five projections).
usage (GPU box): python profiles/exp_trace_chain_proj.py <library built with -DEQD_TRACE -fgpu-rdc>"""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from equidock_public_amd import _lib as L
from tests import chain_resident_proj_common as crp
lib = L.load_library_for_testing(sys.argv[1])
dev = torch.device('cuda:0')
rows, d0 = 3200, 69
gen = torch.Generator().manual_seed(3)
mk = lambda *sh: (torch.randn(*sh, generator=gen) * 0.3).to(dev).contiguous()      # noqa: E731
bufs = dict(h=mk(rows, 64), aggr_msg=mk(rows, 64), aggr_cross=mk(rows, 64), h0=mk(rows, d0), Wn1=mk(64, d0 + 192), Bn1=mk(64),
            ln_g=1 + mk(64), ln_b=mk(64), Wn2=mk(64, 64), Bn2=mk(64), W1=mk(64, 128), B1=mk(64), WQ=mk(64, 64), WK=mk(64, 64),
            WV=mk(64, 64), WM=mk(64, 64), BM=mk(64))
for k in ('a1n', 'y_act', 'h_out', 'P', 'Q', 'qa', 'ka', 'va', 'hm'):
    bufs[k] = torch.zeros(rows, 64, device=dev)
fn = lib.eqd_selftest_node_chain_fwd
fn.restype = C.c_int
fn.argtypes = [C.c_void_p, C.c_void_p]
for form in (0, 1, 5):
    t = crp.EqdNodeChainFwdTest()
    t.rows, t.d0, t.form, t.skip_weight_h, t.slope, t.ln_eps = rows, d0, form, 0.75, 0.01, 1e-5
    for k, v in bufs.items():
        setattr(t, k, v.data_ptr())
    for _ in range(6):
        L.check(fn(C.byref(t), L.stream_ptr(dev)))
    torch.cuda.synchronize()
    buf = (C.c_longlong * 1024)()
    lib.eqd_trace_fetch(buf)
    ck = lambda s: buf[2 * s]      # noqa: E731
    t0 = ck(200)
    names = [(211, 'ordinary loads requested'), (203, 'node_mlp.0 chunks done, vm_wait<0>'), (212, 'remainder step'),
             (201, 'LayerNorm epilogue'), (216, 'node_mlp.4 MFMAs'), (202, 'node_mlp.4 epilogue')]
    names += [(218 + j, f'carried job {j}') for j in range(form)]
    print(f'form {form}: clock64 ticks from kernel entry (workgroup 0, wave 0)')
    prev = t0
    for s, nm in names:
        print(f'   {nm:38s} at {ck(s) - t0:7d}  (+{ck(s) - prev:6d})')
        prev = ck(s)
    wg = [(buf[512 + 2 * i], buf[512 + 2 * i + 1]) for i in range(200)]
    print('   wall_clock64 (100 MHz) per workgroup: avg %.1f ticks, launch span %d ticks' %
          (sum(e - s for s, e in wg) / 200, max(e for s, e in wg) - min(s for s, e in wg)))
