"""The reference's src/surface_analysis.py for a directory of bound complexes: per ligand file the Spearman correlation
between the residue depth and -mu_r_norm[:, 4], the widest-scale surface-aware node feature of the model's graphs.

    python -m equidock_public_amd.surface_analysis --dir DIR [--device cuda:0]

runs over every `*_l_b_COMPLEX.pdb` / `*_r_b_COMPLEX.pdb` pair of DIR through dock.surface_feature_analysis (one batched
graph pass, one batched depth pass) and prints one SPEARMAN line per ligand file, as the reference does, plus the median.
The depth is measured from the contact patch of the surface under the probe, not from MSMS's surface (see
include/equidock_dock.h), so the numbers are not Biopython's digit for digit.  A file whose residues cannot be matched to
its graph nodes is skipped, as in the reference.
"""
import argparse
import glob
import os
import sys

import numpy as np

from . import dock as DK

SUFFIX = '_l_b_COMPLEX.pdb'


def main(argv=None):
    p = argparse.ArgumentParser(prog='python -m equidock_public_amd.surface_analysis', description=__doc__.split('\n')[0])
    p.add_argument('--dir', required=True, help='<name>_l_b_COMPLEX.pdb and <name>_r_b_COMPLEX.pdb of every complex')
    p.add_argument('--device', default='cuda:0')
    p.add_argument('--cutoff', type=float, default=30.0, help='graph cutoff (Angstrom)')
    p.add_argument('--max-neighbor', type=int, default=10)
    p.add_argument('--probe', type=float, default=1.4)
    p.add_argument('--points', type=int, default=96, help='sphere points per atom')
    a = p.parse_args(argv)
    try:
        ligs = sorted(glob.glob(os.path.join(a.dir, '*' + SUFFIX)))
        if not ligs:
            raise FileNotFoundError(f"no *{SUFFIX} files in {a.dir}")
        pairs = []
        for lig in ligs:
            rec = lig[:-len(SUFFIX)] + '_r_b_COMPLEX.pdb'
            if not os.path.isfile(rec):
                raise FileNotFoundError(f"{rec} is missing (receptor of {os.path.basename(lig)})")
            pairs.append((lig, rec))
        res = DK.surface_feature_analysis(pairs, a.device, cutoff=a.cutoff, max_neighbor=a.max_neighbor, probe=a.probe,
                                          n_points=a.points)
        rho = []
        for (lig, _), r in zip(pairs, res):
            if r['n_ligand'] == 0:
                continue
            rho.append(r['spearman_ligand'])
            print(f"SPEARMAN for file {lig} = {r['spearman_ligand']:.6f} ({r['n_ligand']} residues)", flush=True)
        ok = np.asarray([v for v in rho if not np.isnan(v)], dtype=np.float64)
        print(f"SPEARMAN median: {float(np.median(ok)) if ok.size else float('nan'):.6f} ({len(rho)} of {len(pairs)} files)")
    except Exception as e:          # noqa: BLE001 - a command-line tool: report and exit non-zero
        print(f"error: {type(e).__name__}: {e}", file=sys.stderr)
        return 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
