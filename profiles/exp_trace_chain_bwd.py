"""Phase boundaries inside the resident backward node chain (k_rowchain_res_bwd, six-job form), taken from a full model
backward with a -DEQD_TRACE -fgpu-rdc library.  The model is workload B's with every layer 64 wide, so that the LAST chain
launch of the pass - layer 0's, which leaves its stamps in the trace slots - is an eligible six-job chain (the same launch
profiles/exp_trace_chain.py reads for k_rowchain).  usage (GPU box): python profiles/exp_trace_chain_bwd.py <library>"""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from equidock_public_amd import _lib as L, graph, model, synthetic
from oracle import iegmn_port as port

if __name__ == '__main__':
    lib = L.load_library_for_testing(sys.argv[1])
    dev = torch.device('cuda:0')
    args = port.default_args(iegmn_n_lays=8, skip_weight_h=0.75, device=dev, use_mean_node_features=False)
    net = model.Rigid_Body_Docking_Net(args).to(dev)
    net.load_state_dict(port.init_state_dict(args, 0))
    g = graph.batch_pairs(synthetic.make_pairs([(200, 200)] * 8, 1000)).to(dev)
    fn = lib.eqd_chain_resident_bwd_launches
    fn.restype = C.c_longlong
    for _ in range(3):
        lig, Yl, Yr, T, b = net.forward_batched(g)
        (lig.square().sum() + Yl.square().sum()).backward()
    torch.cuda.synchronize()
    print('resident backward launches:', fn(), '(8 per pass when every layer is 64 wide)')
    buf = (C.c_longlong * 1024)()
    lib.eqd_trace_fetch(buf)
    ck = [buf[2 * s] for s in range(200, 210)]
    names = ['ordinary loads requested (entry -> first copy)', '31 copies issued, six dh chunks multiplied (4 slots refilled)',
             'dh epilogue (residual from LDS, store, tile 2)', 'vm_wait<0> + barrier: exposed wait for the refills',
             'alpha dH Wn2 + barrier', 'LeakyReLU / LayerNorm backward + barrier', 'd aggr_msg', 'd aggr_cross', 'dh0acc']
    print('k_rowchain_res_bwd<DH>, workgroup 0 (clock64 ticks between stamps):')
    for i, n in enumerate(names):
        print(f'   {ck[i + 1] - ck[i]:7d}  {n}')
    print(f'   total {ck[9] - ck[0]} ticks')
    wg = [(buf[512 + 2 * i], buf[512 + 2 * i + 1]) for i in range(200)]
    print('wall_clock64 (100 MHz) per workgroup: avg %.1f ticks, launch span %d ticks' % (sum(e - s for s, e in wg) / 200, max(e for s, e in wg) - min(s for s, e in wg)))
