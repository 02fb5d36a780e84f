"""Timings of Hessians with respect to the coordinates (grad.energies_forces_and_hessians, the batched path, and the autograd
loop of grad.forces_and_hessians) on fixtures of tests/golden: device-synchronised, after warm-up, median of several runs.

    python tools/hessian_bench.py [--runs 5] [--autograd-max 264] [--bases ch4_ani1x,dense90_ani2x,...]
                                  [--kind fixture|ani2xr|anir2s] [--sparse [--dense-max 1000] [--modes 10,50]]
                                  [--strain [--strain-budgets 4,16]]

Prints one JSON line per case.  Seeded parameters (the fixtures' seeds): timings do not depend on the values.
``--kind ani2xr`` / ``anir2s`` times that architecture (networks plus the xTB repulsion term) on the fixtures'
coordinates instead of the fixture's own ANI-2x / ANI-1x model.  ``--sparse`` times the block-sparse path
(grad.energies_forces_and_sparse_hessians) and the dense batched path in the same run (the dense one only up to
``--dense-max`` atoms), with the fixture's cell and pbc, the number of stored blocks and the peak device memory of each.
``--modes K[,K2..]`` adds grad.sparse_vibrational_analysis on that sparse Hessian: solver time and iterations for each K,
the time per call of anihip_block_hessian_spmm at m = 1, 8, 32, 64 beside m calls of BlockHessian.matvec, and (up to
``--dense-max`` atoms) the dense route: to_dense, mass weighting and fp64 torch.linalg.eigh.  ``--strain`` times
grad.energies_forces_and_strain_hessians with the fixture's cell and pbc: peak device memory, the number of atom chunks
under the default budget (grad.HESSIAN_BUDGET_BYTES) and, with ``--strain-budgets 4,16`` (GiB), the same call under larger
budgets."""
from __future__ import annotations

import argparse
import json
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
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, [round(t * 1e3, 3) for t in ts]


def modes_row(H, g, sp, ks, runs, dense):
    """Timings of grad.sparse_vibrational_analysis and its operator on a BlockHessian."""
    from torchani_amd import grad
    from torchani_amd.engine import block_hessian_prepare, block_hessian_spmm
    from torchani_amd.extras.io import PERIODIC_TABLE
    from torchani_amd.utils import atomic_numbers_to_masses

    dev = sp.device
    z = torch.tensor([PERIODIC_TABLE.index(s) for s in g["symbols"]], device=dev)
    masses = atomic_numbers_to_masses(torch.where(sp >= 0, z[sp.clamp(min=0)], torch.full_like(sp, -1)),
                                      dtype=torch.float64)
    row = {}
    for k in ks:
        va = grad.sparse_vibrational_analysis(masses, H, k)
        row[f"modes{k}_ms"], row[f"modes{k}_runs"] = timed(lambda: grad.sparse_vibrational_analysis(masses, H, k), runs)
        row[f"modes{k}_iter"] = va.n_iter
        row[f"modes{k}_lowest"] = [round(v, 6) for v in va.eigenvalues[0, :3].tolist()]
    op = block_hessian_prepare(H.index, H.blocks, masses.reshape(-1))
    row["prepare_ms"], _ = timed(lambda: block_hessian_prepare(H.index, H.blocks, masses.reshape(-1)), runs)
    N = sp.numel()
    for m in (1, 8, 32, 64):
        X = torch.randn((N, 3, m), device=dev)
        Y = torch.empty_like(X)
        reps = 20

        def calls():
            for _ in range(reps):
                block_hessian_spmm(op, X, Y)
        row[f"spmm_m{m}_ms"] = round(timed(calls, runs)[0] / reps, 4)
        cols = [X[:, :, i].contiguous() for i in range(m)]

        def matvecs():
            for v in cols:
                H.matvec(v)
        row[f"matvec_x{m}_ms"] = round(timed(matvecs, max(1, runs // 2))[0], 3)
    if dense:
        def eigh():
            D = H.to_dense().double()
            w = masses.rsqrt().repeat_interleave(3, dim=1)
            return torch.linalg.eigh(0.5 * (D + D.transpose(1, 2)) * w.unsqueeze(2) * w.unsqueeze(1))
        row["dense_eigh_ms"], _ = timed(eigh, max(1, runs // 2))
    return row


def main():
    from _util import load_golden, seeded_state

    from torchani_amd import grad
    from torchani_amd.models import ANI1x, ANI2x, ANI2xr, ANIr2s
    from torchani_amd.weights import arch_spec

    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--autograd-max", type=int, default=264)
    ap.add_argument("--bases", default="ch4_ani1x,dense90_ani2x,small_ani2x,1hz5_ani2x")
    ap.add_argument("--kind", default="fixture", choices=("fixture", "ani2xr", "anir2s"))
    ap.add_argument("--sparse", action="store_true", help="block-sparse path beside the dense one")
    ap.add_argument("--dense-max", type=int, default=1000, help="--sparse: largest system the dense path is timed on")
    ap.add_argument("--modes", default="", help="--sparse: lowest normal modes, K[,K2..] of them")
    ap.add_argument("--strain", action="store_true", help="strain second derivatives instead of coordinate Hessians")
    ap.add_argument("--strain-budgets", default="", help="--strain: also time under these chunk budgets [GiB]")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for base in args.bases.split(","):
        g = load_golden(base)
        species = g["species"].astype(np.int64)
        if args.kind == "fixture":
            ctor = ANI2x if g["kind"] == "ani2x" else ANI1x
            model = ctor(state_dict=seeded_state(g["kind"], 8, g["seed"]), device=dev, periodic_table_index=False,
                         cutoff_fn=g["cutoff_fn"], row_capacity=256)
        else:
            ctor = ANI2xr if args.kind == "ani2xr" else ANIr2s
            model = ctor(state_dict=seeded_state(args.kind, 8, g["seed"]), device=dev, periodic_table_index=False,
                         neighborlist="batch", row_capacity=256)
            symbols = arch_spec(args.kind)[0]
            species = np.asarray([symbols.index(s) for s in g["symbols"]] + [-1])[species]   # (-1 stays -1)
        sp = torch.from_numpy(species).to(dev)
        x = torch.from_numpy(g["coords"]).to(dev)
        A = int((sp >= 0).sum())
        row = {"case": base, "model": g["kind"] if args.kind == "fixture" else args.kind, "atoms": A}
        if args.strain:
            cell = None if g["cell"] is None else torch.from_numpy(g["cell"]).to(dev)
            pbc = None if g["pbc"] is None else torch.from_numpy(np.asarray(g["pbc"])).to(dev)
            runs = max(1, args.runs if A < 5000 else 3)
            L_aev = model.aev_computer.engine().L
            row_bytes = model.neural_networks._pack(dev).rows_hvp_row_bytes(sp.numel())
            default = grad.HESSIAN_BUDGET_BYTES
            for gib in [None] + [float(b) for b in args.strain_budgets.split(",") if b]:
                budget = default if gib is None else int(gib * 2**30)
                grad.HESSIAN_BUDGET_BYTES = budget
                try:
                    key = "strain" if gib is None else f"strain_{gib:g}gib"
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    grad.energies_forces_and_strain_hessians(model, sp, x, cell=cell, pbc=pbc)
                    row[key + "_peak_gib"] = round(torch.cuda.max_memory_allocated() / 2**30, 3)
                    row[key + "_chunks"] = -(-A // grad.strain_hessian_chunk_atoms(L_aev, row_bytes, budget))
                    row[key + "_ms"], row[key + "_runs"] = timed(
                        lambda: grad.energies_forces_and_strain_hessians(model, sp, x, cell=cell, pbc=pbc), runs)
                finally:
                    grad.HESSIAN_BUDGET_BYTES = default
            print(json.dumps(row), flush=True)
            continue
        if args.sparse:
            cell = None if g["cell"] is None else torch.from_numpy(g["cell"]).to(dev)
            pbc = None if g["pbc"] is None else torch.from_numpy(np.asarray(g["pbc"])).to(dev)
            runs = max(1, args.runs if A < 5000 else 2)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            out = grad.energies_forces_and_sparse_hessians(model, sp, x, cell=cell, pbc=pbc)
            row["nnz"] = out.hessians.nnz
            row["sparse_peak_gib"] = round(torch.cuda.max_memory_allocated() / 2**30, 3)
            del out
            row["sparse_ms"], row["sparse_runs"] = timed(
                lambda: grad.energies_forces_and_sparse_hessians(model, sp, x, cell=cell, pbc=pbc), runs)
            if args.modes:
                row.update(modes_row(grad.energies_forces_and_sparse_hessians(model, sp, x, cell=cell, pbc=pbc).hessians,
                                     g, sp, [int(k) for k in args.modes.split(",")], runs, A <= args.dense_max))
            if A <= args.dense_max:
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                grad.energies_forces_and_hessians(model, sp, x, cell=cell, pbc=pbc)
                row["dense_peak_gib"] = round(torch.cuda.max_memory_allocated() / 2**30, 3)
                row["dense_ms"], row["dense_runs"] = timed(
                    lambda: grad.energies_forces_and_hessians(model, sp, x, cell=cell, pbc=pbc), runs)
                row["dense_over_sparse"] = round(row["dense_ms"] / row["sparse_ms"], 2)
            print(json.dumps(row), flush=True)
            continue
        row["batched_ms"], row["batched_runs"] = timed(lambda: grad.energies_forces_and_hessians(model, sp, x),
                                                       max(1, args.runs if A < 500 else 3))
        if A <= args.autograd_max:
            def loop():
                xs = x.detach().clone().requires_grad_(True)
                grad.forces_and_hessians(model((sp, xs)).energies, xs)
            row["autograd_ms"], row["autograd_runs"] = timed(loop, max(1, args.runs if A < 100 else 3))
            row["speedup"] = round(row["autograd_ms"] / row["batched_ms"], 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
