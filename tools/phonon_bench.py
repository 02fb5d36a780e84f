"""Timings of the phonon path (torchani_amd.phonons) on the benzene_pbc_ani2x fixture cell: the block-sparse Hessian of the
supercell, the fold into compact force constants, D(q) and its eigenvalues on a Monkhorst-Pack mesh, and the density of states.

    python tools/phonon_bench.py [--repeats 3,3,4] [--mesh 16] [--runs 5] [--bins 1000] [--out profiles/phonons_bench.txt]

Every timing is a host clock around work that ends in a device synchronise, after one warm call of the same shapes: the median
and the range of --runs repetitions.  Seeded parameters (the fixture's seed): timings do not depend on the values.  The lines are
printed and appended to --out."""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, runs):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", default="3,3,4")
    ap.add_argument("--mesh", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--bins", type=int, default=1000)
    ap.add_argument("--eigensolver", default="device")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phonons_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "phonon_bench needs the GPU"
    from _util import load_golden, seeded_state
    from torchani_amd import grad, phonons
    from torchani_amd.engine import block_hessian_prepare, phonon_fold
    from torchani_amd.extras.io import PERIODIC_TABLE
    from torchani_amd.models import ANI2x
    from torchani_amd.utils import atomic_numbers_to_masses

    dev = torch.device("cuda:0")
    repeats = tuple(int(r) for r in args.repeats.split(","))
    g = load_golden("benzene_pbc_ani2x")
    model = ANI2x(state_dict=seeded_state("ani2x", 8, g["seed"]), device=dev, periodic_table_index=False,
                  cutoff_fn=g["cutoff_fn"], row_capacity=256)
    sp = torch.from_numpy(g["species"].astype(np.int64)).to(dev)
    x = torch.from_numpy(g["coords"]).to(dev)
    cell = torch.from_numpy(g["cell"]).to(dev)
    z = torch.tensor([PERIODIC_TABLE.index(s) for s in g["symbols"]], device=dev)[sp.reshape(-1)]
    masses = atomic_numbers_to_masses(z, dtype=torch.float64)
    sc = phonons.supercell(sp, x, cell, repeats)
    pbc = torch.ones(3, dtype=torch.bool, device=dev)
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    n, N = sp.numel(), sc.species.numel()
    widths = phonons._widths(sc.cell).tolist()
    emit(f"benzene_pbc_ani2x x {repeats}: {n} basis atoms, {N} atoms, perpendicular widths "
         + ", ".join(f"{w:.2f}" for w in widths) + f" A (4 R_c = {4 * float(model.cutoff):.1f}); median [min .. max] of {args.runs}, ms")
    hess = lambda: grad.energies_forces_and_sparse_hessians(model, sc.species, sc.coordinates, cell=sc.cell, pbc=pbc)   # noqa: E731
    emit("sparse Hessian of the supercell      %9.2f [%.2f .. %.2f]" % timed(hess, args.runs))
    H = hess().hessians
    emit("force_constants_from_hessian (all)   %9.2f [%.2f .. %.2f]"
         % timed(lambda: phonons.force_constants_from_hessian(H, sc, masses, reach=2 * float(model.cutoff)), args.runs))
    fc = phonons.force_constants_from_hessian(H, sc, masses, reach=2 * float(model.cutoff))
    op = block_hessian_prepare(H.index, H.blocks, torch.ones(N, dtype=torch.float64, device=dev))
    eb, ej, boff, poff, diag = phonons._compact_pattern(H.index, n, N)
    eb, ej = eb.int().contiguous(), ej.int().contiguous()
    emit("  of which anihip_phonon_fold        %9.3f [%.3f .. %.3f]"
         % timed(lambda: phonon_fold(op, n, repeats, eb, ej, boff, diag), args.runs))
    emit(f"  {H.nnz} blocks, {fc.phi.shape[0]} compact entries, exact {fc.exact}, n_missing {fc.n_missing}, translation_defect "
         f"{fc.translation_defect:.2e}")
    q, w = phonons.monkhorst_pack((args.mesh,) * 3, device=dev)
    emit(f"Monkhorst-Pack {args.mesh}^3: {q.shape[0]} q after time reversal, D(q) {3 * n} x {3 * n} complex128")
    chunk = q[:phonons.MESH_CHUNK].contiguous()
    emit("D(q), %4d q                          %9.3f [%.3f .. %.3f]"
         % ((chunk.shape[0],) + timed(lambda: phonons.dynamical_matrices(fc, chunk), args.runs)))
    emit("D(q) and dD/dk, %4d q                %9.3f [%.3f .. %.3f]"
         % ((chunk.shape[0],) + timed(lambda: phonons.dynamical_matrices(fc, chunk, derivatives=True), args.runs)))
    D = phonons.dynamical_matrices(fc, chunk)
    emit("torch.linalg.eigh (%s), %4d q    %9.2f [%.2f .. %.2f]"
         % ((args.eigensolver, chunk.shape[0]) + timed(lambda: phonons._eigh(D, args.eigensolver), args.runs)))
    emit("phonons.mesh, the whole mesh         %9.2f [%.2f .. %.2f]"
         % timed(lambda: phonons.mesh(fc, (args.mesh,) * 3, eigensolver=args.eigensolver), args.runs))
    pm = phonons.mesh(fc, (args.mesh,) * 3, eigensolver=args.eigensolver)
    emit("dos, %d modes x %d bins        %9.3f [%.3f .. %.3f]"
         % ((pm.frequencies.numel(), args.bins) + timed(lambda: pm.dos(args.bins), args.runs)))
    th = pm.thermodynamics([300.0])
    emit(f"  frequencies {pm.frequencies.min().item():.1f} .. {pm.frequencies.max().item():.1f} cm^-1, {th.n_imaginary} modes with "
         f"f <= 0 of {pm.frequencies.numel()}; supercell max |force| "
         f"{hess().forces.abs().max().item():.3f} Ha/A (the fixture is not relaxed)")
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
