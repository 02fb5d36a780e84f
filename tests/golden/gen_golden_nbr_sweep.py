"""Per-atom neighbor counts and distance sums of the REFERENCE for the neighbor sweep -> tests/golden/nbrsweep_<case>.npz.

    python tests/golden/gen_golden_nbr_sweep.py         (needs the reference checkout that gen_golden.py bootstraps; the outputs are committed)

The cases come from tests/_nbr_cases.py (those with a `golden` name: ortho, the skew cell under its four periodicities, slab,
rod, tiny).  The reference's AllPairs runs on each case's fp32 coordinates in float64; the file keeps the per-atom
neighbor count (int16) and the per-atom sum of neighbor distances (fp64), a few kB per case.  No pair lists, no inputs: the
cases are seeded, and a generator that has drifted from its fixtures shows as a count mismatch.  tests/test_neighbor_cases_host.py holds the fp64 oracle to them.

AllPairs only: the reference's CellList is no fixture for these geometries.  On the skew cell it returns fewer pairs than
its own AllPairs (34 371 against 35 108 on the prototype of that case), and it rejects partial periodicity.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as gg  # noqa: E402,F401  (bootstraps the reference import)

import torch  # noqa: E402
from torchani.neighbors import AllPairs  # noqa: E402

import _nbr_cases as nc  # noqa: E402


def main():
    for name in nc.GOLDEN_CASES:
        case = nc.case_by_name(name)
        n = case.n_atoms
        species = torch.from_numpy(case.species.astype(np.int64))
        coords = torch.from_numpy(case.coords).double()
        periodic = case.periodic
        cell = torch.from_numpy(case.cell).double() if periodic else None
        pbc = torch.tensor(case.pbc) if periodic else None
        nb = AllPairs()(case.rcr, species, coords, cell, pbc)
        idx = nb.indices.numpy()
        dist = nb.distances.numpy().astype(np.float64)
        # the half list seen from both ends
        count = np.bincount(idx[0], minlength=n) + np.bincount(idx[1], minlength=n)
        dsum = np.bincount(idx[0], weights=dist, minlength=n) + np.bincount(idx[1], weights=dist, minlength=n)
        assert count.max() < 2 ** 15
        out = os.path.join(HERE, f"nbrsweep_{case.golden}.npz")
        np.savez_compressed(out, count=count.astype(np.int16), dist_sum=dsum)
        print(f"{name}: {n} atoms, {idx.shape[1]} pairs (half list) -> {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
