"""Workload of the kernel table profiles/dock_graphs_kernels.md: the two proteins of tests/golden/graph_case_big.npz
(1 270 and 40 residues) through dock.protein_graphs_batch, and through the per-protein path for comparison.

usage (GPU box, once per setting of EQD_DOCK_GRAPH_PRUNE):
    rocprofv3 --kernel-trace --stats -f csv -d OUT -- python profiles/trace_dock_graphs.py [--calls N]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from equidock_public_amd import dock as DK, featurize as FZ  # noqa: E402
from tests import dock_graph_common as gc  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--calls', type=int, default=5)
    p.add_argument('--lib', help='another build of libequidock_dock.so (kernel experiments)')
    a = p.parse_args()
    if a.lib:
        DK.load_dock_library_for_testing(a.lib)
    dev = torch.device('cuda:0')
    prots = gc.fixture_proteins(['graph_case_big'])
    for _ in range(a.calls):
        gc.batch_of(prots, dev)
        for q in prots:
            FZ.protein_graph(q['residues'], q['bound_ca'], 30.0, 10, dev)
    torch.cuda.synchronize(dev)
    print('pruning', DK.graph_pruning_enabled(), DK.last_graph_stats)


if __name__ == '__main__':
    main()
