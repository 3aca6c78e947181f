"""Job boundaries inside the FORWARD node chain of the last layer (workload B model): forward passes only, so the last chain
launch that wrote the trace slots is layer 7's forward chain.  usage (GPU box): python profiles/exp_trace_chain_fwd.py <library built with -DEQD_TRACE -fgpu-rdc>"""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from equidock_public_amd import _lib as L, graph, model, synthetic
from oracle import iegmn_port as port
lib = L.load_library_for_testing(sys.argv[1])
dev = torch.device('cuda:0')
args = port.default_args(iegmn_n_lays=8, skip_weight_h=0.75, device=dev)
net = model.Rigid_Body_Docking_Net(args).to(dev)
net.load_state_dict(port.init_state_dict(args, 0))
g = graph.batch_pairs(synthetic.make_pairs([(200, 200)] * 8, 1000)).to(dev)
with torch.no_grad():
    for _ in range(4):
        net.forward_batched(g)
torch.cuda.synchronize()
buf = (C.c_longlong * 1024)()
lib.eqd_trace_fetch(buf)
ck = [buf[2 * s] for s in range(200, 204)]
print('forward node chain, workgroup 0, clock64 ticks: zero tiles -> end job0 -> end job1:', [ck[i + 1] - ck[i] for i in range(2)], 'total', ck[2] - ck[0])
for jj in (0, 1):
    b = [buf[2 * (210 + 4 * jj + i)] for i in range(4)]
    print(f'   job {jj}: prologue {b[1] - b[0]:6d} | steps {b[2] - b[1]:6d} | next-job prefetch {b[3] - b[2]:6d} | epilogue+sync {buf[2 * (201 + jj)] - b[3]:6d}')
wg = [(buf[512 + 2 * i], buf[512 + 2 * i + 1]) for i in range(200)]
print('wall_clock64 (100 MHz) per workgroup: avg %.1f ticks, launch span %d ticks' % (sum(e - s for s, e in wg) / 200, max(e for s, e in wg) - min(s for s, e in wg)))
