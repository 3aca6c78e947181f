"""Workload of the kernel table profiles/dock_depth_kernels.md: 5 calls of dock.DepthPlan.eval on the 25 seeded clouds of
profiles/bench_dock_depth.py and 5 on the first one alone, then the same on dock.SurfacePlan.eval for comparison of the
exposure stage, to be run under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.argv = sys.argv[:1]
from equidock_public_amd import dock as DK  # noqa: E402
from profiles import bench_dock_depth as B  # noqa: E402

if __name__ == '__main__':
    for n in (1, 25):
        cx = B.complexes(n)
        lr, rr, lo, ro = B.tables(cx)
        lig, rec = torch.cat([c['lig'] for c in cx], 0), torch.cat([c['rec'] for c in cx], 0)
        for plan in (DK.DepthPlan(lo, ro, lr, rr, B.dev, n_points=B.POINTS), DK.SurfacePlan(lo, ro, lr, rr, B.dev, n_points=B.POINTS)):
            out = plan.outputs()
            for _ in range(5):
                rows = plan.eval(lig, rec, *out, probe=B.PROBE)
            torch.cuda.synchronize()
        print(n, rows[:, :2].sum(0).tolist())
