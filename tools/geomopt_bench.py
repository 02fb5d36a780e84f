"""Per-iteration GPU time of the L-BFGS step (anihip_lbfgs_step: four kernels) next to the energies-and-forces evaluation it
drives, at full history: memory = 100, fmax = 0 (nothing converges) and --iters > 100 iterations, so that the ring is full
and wraps.  HIP events around each part of every iteration; medians over the iterations after the first 101.
    python tools/geomopt_bench.py [--iters 130] [--json out.json] [--only config2,conformers2560,config3]
    python tools/geomopt_bench.py --trace-summary run_kernel_trace.csv   (of `rocprofv3 --kernel-trace` over a run above:
                                  the median time per kernel over the calls after the first 101, i.e. at full history)
  config2        256 molecules of A = 28 (tests/golden/cfg2_xyz13_28_ani2x.npz), batch mode (graph replay from the third call)
  conformers2560 those 256 molecules ten times over: 2560 conformers, 71 680 atom slots
  config3        the 46 357-atom solvated 1hz5 box, periodic, cell mode
    python tools/geomopt_bench.py --constraints [--out profiles/geomopt_constraints_bench.txt]
                                  the 2560 conformers with one dihedral constraint each (geomopt.CVConstraints) against the same
                                  batch without: whole steps (optimizer, restore, evaluation, projection), the two optimizers
                                  alternating in one process, median (fastest, slowest) ms per step over 7 repeats
    python tools/geomopt_bench.py --saddle [--out profiles/saddle_bench.txt]
                                  ms per step of geomopt.SaddleOptimizer split into the exact Hessian, anihip_saddle_project,
                                  torch.linalg.eigh, anihip_saddle_step, the evaluation and anihip_saddle_accept, on config 2's 256
                                  molecules and on the 90-atom dense90 molecule, hessian_every 1 and 5; HIP events around each
                                  part, median (fastest, slowest) over 5 repeats of 10 steps
    python tools/geomopt_bench.py --irc [--out profiles/irc_bench.txt]
                                  the same for a point of geomopt.ReactionPathFollower: the exact Hessian, anihip_irc_project,
                                  torch.linalg.eigh, anihip_irc_step, the evaluation and anihip_irc_commit; fmax = 0 and no
                                  energy test, so that every entry takes every point
Bytes moved per L-BFGS step are estimated from the shapes (lbfgs_step_bytes), so that the achieved rate can be compared
with HBM: S and Y read twice in fp32 and the fp64 m x m matrices of k_lb_solve, which outweigh S and Y for small molecules."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")


def lbfgs_step_bytes(C, A, memory):
    """Device bytes one step moves at full history, per molecule: k_lb_dots and k_lb_direction each read S and Y
    [memory][3A] fp32; k_lb_solve reads the upper triangles of R^-1 (from its transpose, for a) and of R^-1 (for t) and all of
    Y^T Y, fp64 m x m: 2 m^2 x 8 bytes.  (The partial sums, coordinates and forces are a few per cent on top.)"""
    return C * (2 * 2 * memory * 3 * A * 4 + 2 * memory * memory * 8)


def measure(name, model, sp, x, cell, pbc, iters, memory=100):
    from torchani_amd.geomopt import GeometryOptimizer, lbfgs_workspace_bytes

    opt = GeometryOptimizer(model, sp, x, cell, pbc, memory=memory)
    opt.fmax = 0.0
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(iters)]
    for k in range(iters):
        e0, e1, e2 = ev[k]
        e0.record()
        opt._lbfgs_step()
        e1.record()
        opt._evaluate()
        e2.record()
    torch.cuda.synchronize()
    opt.raise_on_overflow()
    full = range(memory + 1, iters)
    lb = np.array([ev[k][0].elapsed_time(ev[k][1]) for k in full]) * 1e3
    ef = np.array([ev[k][1].elapsed_time(ev[k][2]) for k in full]) * 1e3
    C, A = sp.shape
    out = {"workload": name, "molecules": C, "atoms_per_molecule": A, "memory": memory, "iterations": iters,
           "iterations_timed": len(lb), "lbfgs_us_median": float(np.median(lb)), "lbfgs_us_min": float(lb.min()),
           "energies_forces_us_median": float(np.median(ef)), "ratio_median": float(np.median(lb) / np.median(ef)),
           "step_MB": lbfgs_step_bytes(C, A, memory) / 1e6,
           "step_TB_per_s": lbfgs_step_bytes(C, A, memory) / (np.median(lb) * 1e-6) / 1e12,
           "workspace_MB": lbfgs_workspace_bytes(C, A, memory) / 1e6,
           "n_steps_min": int(opt.n_steps.min())}
    print(json.dumps(out), flush=True)
    return out


def constraints_ab(model, sp, x, out_path, repeats=7, steps=30, memory=10):
    """ms per step() of a constrained and an unconstrained optimizer on the same batch, alternating."""
    from torchani_amd import md
    from torchani_amd.geomopt import CVConstraints, GeometryOptimizer

    assert bool((sp[:, :4] >= 0).all())
    opts = {"unconstrained": GeometryOptimizer(model, sp, x, memory=memory),
            "constrained": GeometryOptimizer(model, sp, x, memory=memory, constraints=CVConstraints(md.dihedral(0, 1, 2, 3)))}
    for opt in opts.values():
        opt.fmax = 0.0
        for _ in range(5):   # (the third evaluation captures the automatic HIP graph)
            opt.step()
    torch.cuda.synchronize()
    ms = {k: [] for k in opts}
    for _ in range(repeats):
        for name, opt in opts.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                opt.step()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / steps)
    opts["constrained"].raise_on_failed_constraints()
    it = opts["constrained"].constraint_iterations
    lines = [f"tools/geomopt_bench.py --constraints: {sp.shape[0]} conformers of A = {sp.shape[1]}, one dihedral constraint each, "
             f"memory {memory}; step() = L-BFGS step (+ restore) + evaluation (+ projection); {repeats} repeats of {steps} steps, "
             "the two optimizers alternating in one process; median (fastest, slowest) ms per step"]
    for name, v in ms.items():
        lines.append(f"  {name:14s} {np.median(v):.4f} ({min(v):.4f}, {max(v):.4f})")
    lo = max(min(v) for v in ms.values())
    hi = min(max(v) for v in ms.values())
    lines.append(f"  difference of the medians {1e3 * (np.median(ms['constrained']) - np.median(ms['unconstrained'])):+.1f} us per step; "
                 + ("the two ranges overlap: no difference is resolved" if lo <= hi else "the two ranges do not overlap"))
    lines.append(f"  restore iterations of the last step: {int(it.min())} .. {int(it.max())}")
    text = "\n".join(lines)
    print(text, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")


SADDLE_PARTS = ("exact Hessian", "anihip_saddle_project", "torch.linalg.eigh", "anihip_saddle_step", "evaluation",
                "anihip_saddle_accept")


def saddle_parts(model, sp, x, hessian_every, repeats=5, steps=10):
    """ms per step of each part of SaddleOptimizer.step() (its phases _refresh_hessians, _move and _judge taken apart), per
    repeat of `steps` steps: {part: [ms per step, one per repeat]}.  fmax = 0: nothing converges."""
    import ctypes

    from torchani_amd import _lib
    from torchani_amd.engine import _stream
    from torchani_amd.geomopt import SaddleOptimizer

    L = _lib.lib()
    opt = SaddleOptimizer(model, sp, x, hessian_every=hessian_every)
    opt.fmax = 0.0
    for _ in range(hessian_every + 1):   # (warm-up: every shape once, the automatic HIP graph captured)
        opt.step()
    torch.cuda.synchronize()
    out = {part: [] for part in SADDLE_PARTS + ("whole step",)}
    for _ in range(repeats):
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(7)] for _ in range(steps)]
        for k in range(steps):
            st = opt._state
            ev[k][0].record()
            opt._refresh_hessians()
            ev[k][1].record()
            st.fmax, st.follow = 0.0, 0
            opt._project(st, opt._projected)
            ev[k][2].record()
            lam, V = torch.linalg.eigh(opt._projected)
            lam, V = lam.contiguous(), V.contiguous()
            ev[k][3].record()
            _lib.check(L.anihip_saddle_step(_stream(), ctypes.byref(st), lam.data_ptr(), V.data_ptr()))
            ev[k][4].record()
            e, f = opt._model_eval(opt.coordinates)
            e, f = e.to(torch.float64).contiguous(), f.to(torch.float32).contiguous()
            ev[k][5].record()
            _lib.check(L.anihip_saddle_accept(_stream(), ctypes.byref(st), e.data_ptr(), f.data_ptr(),
                                              int((opt._calls + 1) % hessian_every != 0)))
            opt._calls += 1
            ev[k][6].record()
        torch.cuda.synchronize()
        for i, part in enumerate(SADDLE_PARTS):
            out[part].append(sum(ev[k][i].elapsed_time(ev[k][i + 1]) for k in range(steps)) / steps)
        out["whole step"].append(sum(ev[k][0].elapsed_time(ev[k][6]) for k in range(steps)) / steps)
    opt.raise_on_overflow()
    opt.raise_on_status()
    out["accepted"] = int(opt.n_steps.sum())
    out["rejected"] = int(opt.n_rejected.sum())
    return out


def saddle_bench(out_path):
    from torchani_amd.models import ANI2x

    dev = torch.device("cuda:0")
    cases = []
    with np.load(os.path.join(GOLD, "cfg2_xyz13_28_ani2x.npz")) as z:
        cases.append(("config 2: 256 molecules, A = 28 (3A = 84)", z["species"].astype(np.int64), z["coords"]))
    with np.load(os.path.join(GOLD, "dense90_ani2x.npz")) as z:
        cases.append(("dense90: 1 molecule, A = 90 (3A = 270)", z["species"].astype(np.int64), z["coords"]))
    lines = ["tools/geomopt_bench.py --saddle: ms per step() of geomopt.SaddleOptimizer, HIP events around each part, "
             "median (fastest, slowest) over 5 repeats of 10 steps; seeded ANI-2x x 8, fmax = 0"]
    for name, sp, x in cases:
        model = ANI2x(seed=0, device=dev, periodic_table_index=False, neighborlist="batch")
        for h in (1, 5):
            r = saddle_parts(model, torch.from_numpy(sp).to(dev), torch.from_numpy(x).to(dev), h)
            whole = np.median(r["whole step"])
            lines.append(f"{name}, hessian_every {h}: whole step {whole:.3f} ({min(r['whole step']):.3f}, "
                         f"{max(r['whole step']):.3f}) ms; steps accepted {r['accepted']}, rejected {r['rejected']}")
            new = 0.0
            for part in SADDLE_PARTS:
                v = r[part]
                lines.append(f"  {part:22s} {np.median(v):8.4f} ({min(v):.4f}, {max(v):.4f})  {100 * np.median(v) / whole:5.1f} %")
                if part.startswith("anihip_saddle"):
                    new += np.median(v)
            lines.append(f"  the three new entry points together: {new:.4f} ms = {100 * new / whole:.1f} % of the step")
    text = "\n".join(lines)
    print(text, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")


IRC_PARTS = ("exact Hessian", "anihip_irc_project", "torch.linalg.eigh", "anihip_irc_step", "evaluation", "anihip_irc_commit")
ANI2X_MASSES = (1.008, 12.011, 14.007, 15.999, 32.06, 18.998, 35.45)   # H C N O S F Cl, the element indices of ANI-2x


def irc_parts(model, sp, x, hessian_every, repeats=5, steps=10):
    """ms per point of each part of ReactionPathFollower.step() (its phases _refresh_hessians, _move and _judge taken apart),
    per repeat of `steps` points: {part: [ms per point, one per repeat]}."""
    import ctypes

    from torchani_amd import _lib
    from torchani_amd.engine import _stream
    from torchani_amd.geomopt import ReactionPathFollower

    L = _lib.lib()
    masses = torch.tensor(ANI2X_MASSES + (0.0,), dtype=torch.float64, device=sp.device)[sp]
    total = hessian_every + 1 + repeats * steps
    opt = ReactionPathFollower(model, sp, x, masses=masses, hessian_every=hessian_every, step=0.02, max_points=total + 1,
                               fmax=0.0, energy_floor=1e30)
    for _ in range(hessian_every + 1):   # (warm-up: every shape once, the automatic HIP graph captured)
        opt.step()
    torch.cuda.synchronize()
    out = {part: [] for part in IRC_PARTS + ("whole point",)}
    st = opt._state
    for _ in range(repeats):
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(7)] for _ in range(steps)]
        for k in range(steps):
            ev[k][0].record()
            opt._refresh_hessians()
            ev[k][1].record()
            _lib.check(L.anihip_irc_project(_stream(), ctypes.byref(st), opt._projected.data_ptr()))
            ev[k][2].record()
            lam, V = torch.linalg.eigh(opt._projected)
            lam, V = lam.contiguous(), V.contiguous()
            ev[k][3].record()
            _lib.check(L.anihip_irc_step(_stream(), ctypes.byref(st), lam.data_ptr(), V.data_ptr()))
            ev[k][4].record()
            e, f = opt._model_eval(opt.coordinates)
            e, f = e.to(torch.float64).contiguous(), f.to(torch.float32).contiguous()
            ev[k][5].record()
            _lib.check(L.anihip_irc_commit(_stream(), ctypes.byref(st), e.data_ptr(), f.data_ptr(),
                                           int((opt._calls + 1) % hessian_every != 0)))
            opt._calls += 1
            ev[k][6].record()
        torch.cuda.synchronize()
        for i, part in enumerate(IRC_PARTS):
            out[part].append(sum(ev[k][i].elapsed_time(ev[k][i + 1]) for k in range(steps)) / steps)
        out["whole point"].append(sum(ev[k][0].elapsed_time(ev[k][6]) for k in range(steps)) / steps)
    opt.raise_on_overflow()
    opt.raise_on_status()
    out["points"] = opt.n_points.cpu().tolist()
    assert min(out["points"]) == total, "an entry stopped early"
    return out


def irc_bench(out_path):
    from torchani_amd.models import ANI2x

    dev = torch.device("cuda:0")
    cases = []
    with np.load(os.path.join(GOLD, "cfg2_xyz13_28_ani2x.npz")) as z:
        cases.append(("config 2: 256 molecules, A = 28 (3A = 84)", z["species"].astype(np.int64), z["coords"]))
    with np.load(os.path.join(GOLD, "dense90_ani2x.npz")) as z:
        cases.append(("dense90: 1 molecule, A = 90 (3A = 270)", z["species"].astype(np.int64), z["coords"]))
    lines = ["tools/geomopt_bench.py --irc: ms per point (step()) of geomopt.ReactionPathFollower, HIP events around each part, "
             "median (fastest, slowest) over 5 repeats of 10 points; seeded ANI-2x x 8, step 0.02, fmax = 0, no energy test"]
    for name, sp, x in cases:
        model = ANI2x(seed=0, device=dev, periodic_table_index=False, neighborlist="batch")
        for h in (1, 5):
            r = irc_parts(model, torch.from_numpy(sp).to(dev), torch.from_numpy(x).to(dev), h)
            whole = np.median(r["whole point"])
            lines.append(f"{name}, hessian_every {h}: whole point {whole:.3f} ({min(r['whole point']):.3f}, "
                         f"{max(r['whole point']):.3f}) ms")
            new = 0.0
            for part in IRC_PARTS:
                v = r[part]
                lines.append(f"  {part:22s} {np.median(v):8.4f} ({min(v):.4f}, {max(v):.4f})  {100 * np.median(v) / whole:5.1f} %")
                if part.startswith("anihip_irc"):
                    new += np.median(v)
            lines.append(f"  the three new entry points together: {new:.4f} ms = {100 * new / whole:.1f} % of the point")
    text = "\n".join(lines)
    print(text, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")


def trace_summary(path, skip=101):
    """Median duration (us) of each k_lb_* kernel over its calls after the first `skip`, and their sum."""
    import collections
    import csv

    per = collections.defaultdict(list)
    for r in csv.DictReader(open(path)):
        if "k_lb_" in r["Kernel_Name"]:
            name = r["Kernel_Name"].split("(")[0].replace("anihip::", "").replace("void ", "")
            per[name].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    med = {k: float(np.median(v[skip:])) for k, v in per.items()}
    return {"median_us_after_call": skip, **med, "sum_us": sum(med.values())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=130)
    ap.add_argument("--json", default=None)
    ap.add_argument("--only", default="config2,conformers2560,config3")
    ap.add_argument("--trace-summary", default=None, metavar="CSV")
    ap.add_argument("--constraints", action="store_true")
    ap.add_argument("--saddle", action="store_true")
    ap.add_argument("--irc", action="store_true")
    ap.add_argument("--out", default=None, metavar="TXT")
    args = ap.parse_args()
    if args.trace_summary:
        print(json.dumps(trace_summary(args.trace_summary)))
        return
    if args.saddle:
        saddle_bench(args.out)
        return
    if args.irc:
        irc_bench(args.out)
        return
    assert args.iters > 101, "the history is full from iteration 101 on"
    from torchani_amd.models import ANI2x

    dev = torch.device("cuda:0")
    want = args.only.split(",")
    res = {}
    with np.load(os.path.join(GOLD, "cfg2_xyz13_28_ani2x.npz")) as z:
        sp2, x2 = z["species"].astype(np.int64), z["coords"]
    if args.constraints:
        model = ANI2x(seed=0, device=dev, periodic_table_index=False, neighborlist="batch")
        constraints_ab(model, torch.from_numpy(np.tile(sp2, (10, 1))).to(dev), torch.from_numpy(np.tile(x2, (10, 1, 1))).to(dev),
                       args.out)
        return
    if "config2" in want:
        model = ANI2x(seed=0, device=dev, periodic_table_index=False, neighborlist="batch")
        res["config2"] = measure("config 2: 256 molecules, A = 28", model, torch.from_numpy(sp2).to(dev),
                                 torch.from_numpy(x2).to(dev), None, None, args.iters)
    if "conformers2560" in want:
        model = ANI2x(seed=0, device=dev, periodic_table_index=False, neighborlist="batch")
        res["conformers2560"] = measure("2560 conformers, A = 28", model, torch.from_numpy(np.tile(sp2, (10, 1))).to(dev),
                                        torch.from_numpy(np.tile(x2, (10, 1, 1))).to(dev), None, None, args.iters)
    if "config3" in want:
        model = ANI2x(seed=0, device=dev, periodic_table_index=False, neighborlist="cell")
        with np.load(os.path.join(GOLD, "cfg3_1hz5_water_ani2x.npz")) as z:
            sp3, x3, cell = z["species"].astype(np.int64), z["coords"], z["cell"]
        res["config3"] = measure("config 3: 1hz5 solvated, 46 357 atoms, periodic", model, torch.from_numpy(sp3).to(dev),
                                 torch.from_numpy(x3).to(dev), torch.from_numpy(cell).to(dev), (True, True, True), args.iters)
    if args.json:
        os.makedirs(os.path.dirname(args.json) or ".", exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
