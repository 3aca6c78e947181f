"""Workload of the kernel table profiles/dock_lddt_kernels.md: 5 calls of dock.lddt_batch on the 25 seeded clouds of
profiles/bench_dock_lddt.py, to be run under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.argv = sys.argv[:1]
from profiles import bench_dock_lddt as B  # noqa: E402

if __name__ == '__main__':
    cx = B.complexes(25)
    for _ in range(5):
        rows = B.device_pass(cx)
    torch.cuda.synchronize()
    print(rows[:, :2])
