"""MD step rate (cf. the reference's tools/md-benchmark.py, which drives the same path through ASE):

    python tools/md_bench.py [--side 64] [--steps 20]                      the host driver with and without Verlet-skin reuse
    python tools/md_bench.py --integrator both --langevin --repeats 7 ...  host driver (md.MolecularDynamics) against the
                                                                           on-device integrator (md.BatchedDynamics)
    python tools/md_bench.py --integrator device --constraints none rigid-water --dt 2 ...
                                                                           the device integrator without and with bond-length
                                                                           constraints (md.hydrogen_constraints), alternating
    python tools/md_bench.py --integrator device --langevin --barostat ...  NVT, NVT with the virial-carrying evaluation, and NPT
                                                                           (stochastic cell rescaling), alternating: the cost of
                                                                           the barostat split into the evaluation's and its own
    python tools/md_bench.py --integrator device --langevin --barostat --constraints rigid-water --dt 2 ...
                                                                           the same three with rigid waters (or X-H bonds): NPT by
                                                                           molecular cell rescaling (barostat_scaling="molecular")
    python tools/md_bench.py --beads 32 --system molecules --repeats 7 ...  path-integral MD (md.RingPolymerDynamics, PILE) against
    python tools/md_bench.py --beads 8 --side 10 --repeats 7 ...            the classical Langevin step of md.BatchedDynamics on the
                                                                           same [R beads, A] batch: the first 256 / beads molecules
                                                                           of config 2 as ring polymers, or beads copies of the box

    python tools/md_bench.py --exchange-every 1 --rungs 8 --system molecules --repeats 7 ...
                                                                           temperature replica exchange (md.ReplicaExchangeDynamics):
                                                                           every molecule of config 2 as a ladder of --rungs replicas,
                                                                           the exchanging step against exchange_every=0 on one batch
    python tools/md_bench.py --bias restraints --system molecules --langevin --repeats 7 ...
    python tools/md_bench.py --bias metadynamics --hills 10000 [--shared-walkers] --system molecules --langevin --repeats 7 ...
                                                                           biased MD (md.BatchedDynamics(bias=...)) against the
                                                                           unbiased step on one batch: one restraint per system
                                                                           (a dihedral of each molecule, a distance in the box),
                                                                           or a static 2-CV metadynamics bias of --hills hills
                                                                           per list, a list per molecule or one for all walkers

    python tools/md_bench.py --bias sites --system molecules --langevin --repeats 7 ...
    python tools/md_bench.py --bias coordination [--coordination-atoms 100] --side 10 --langevin --repeats 7 ...
                                                                           group CVs (md.center, md.coordination): a restraint on
                                                                           the distance between the centres of mass of the two
                                                                           halves of every molecule, or on the coordination number
                                                                           of all O against all H of the box (--coordination-atoms
                                                                           N: the first N of each)
    python tools/md_bench.py --observe series trajectory rdf msd vacf heatflux hfacf [--observe-every 10] [--lags 512] --langevin --repeats 7 ...
                                                                           observers (md.TimeSeries ... md.VelocityAutocorrelation):
                                                                           the step with each attached against the step without,
                                                                           the cost per sample next to the bytes it has to move

--system water is the periodic water box of bench.py (3 side^3 atoms); --system molecules is BASELINE config 2's batch of 256
molecules.  With --repeats R every (neighbor list, integrator) pair is timed R times, the integrators alternating, and the
median, the fastest and the slowest repeat are printed: the spread to hold a difference against.  Whenever the device integrator
is timed both models are built with row_capacity=256, since BatchedDynamics raises on a neighbor-row overflow instead of retrying."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import water_box  # noqa: E402

ELEMENT_MASSES = [1.008, 12.011, 14.007, 15.999, 32.06, 18.998, 35.45]   # ANI-2x element order


def load_system(args, dev):
    """species (element indices), coordinates, cell, pbc, the neighbor lists to time."""
    if args.system == "molecules":
        with np.load(os.path.join(ROOT, "tests", "golden", "cfg2_xyz13_28_ani2x.npz")) as z:
            sp, x = z["species"].astype(np.int64), z["coords"]
        return torch.from_numpy(sp).to(dev), torch.from_numpy(x).to(dev), None, None, ("batch",)
    sp, x, cell = water_box(args.side)
    return (torch.from_numpy(sp.astype(np.int64)).to(dev), torch.from_numpy(x).to(dev), torch.from_numpy(cell).to(dev),
            (True, True, True), ("cell_list", "verlet_cell_list"))


def make_driver(kind, args, model, sp, x, cell, pbc, masses):
    """kind: "host", "device", "device+hydrogens" / "device+rigid-water" for the device integrator with constraints,
    "device+virial" for NVT whose evaluations carry the virial, "device+npt" for the barostat; the last two also with
    constraints ("device+npt+rigid-water": molecular cell rescaling)."""
    from torchani_amd.geomopt import ModelEvaluator
    from torchani_amd.md import BatchedDynamics, MolecularDynamics, hydrogen_constraints

    temperature = 300.0 if args.langevin else None
    if kind == "host":
        md = MolecularDynamics(model, sp, x, cell, pbc, dt=args.dt, masses=masses, temperature=temperature, seed=1)
    else:
        constraints = None
        if kind.endswith(("hydrogens", "rigid-water")):   # (species are ANI-2x element indices: H = 0, O = 3)
            constraints = hydrogen_constraints(sp, x, cell, pbc, rigid_water=kind.endswith("rigid-water"), hydrogen=0, oxygen=3)
        npt = "+npt" in kind
        md = BatchedDynamics(model, sp, x, cell, pbc, dt=args.dt, masses=masses, temperature=temperature, seed=1,
                             constraints=constraints, pressure=1.0 if npt else None, barostat_time=args.barostat_time,
                             barostat_scaling="molecular" if npt and constraints is not None else "atomic")
        if "+virial" in kind:   # the NVT step with the evaluation that the barostat needs, and nothing else of it
            md._model_eval = ModelEvaluator(model, sp, cell, pbc, stress=True)
    md.set_temperature(300.0)
    if kind != "host" and npt:
        # (the seed-0 weights are no physical potential: at 1 bar the box would run away and the step time with its density;
        # by default the target is the pressure the box starts with)
        md.pressure.copy_(md.pressures() if args.pressure is None else torch.full_like(md.pressure, args.pressure))
        md.volume0 = md.volumes().item()
    return md


def bench_beads(args, dev):
    """RingPolymerDynamics (PILE, --temperature) against BatchedDynamics (Langevin at beads x that, what the beads are sampled at) on one
    [R beads, A] batch, in one process, the repeats alternating.  Both run the same evaluation, kick and launch count; they
    differ in the drift kernel."""
    from torchani_amd.md import BatchedDynamics, RingPolymerDynamics
    from torchani_amd.models import ANI2x

    P = args.beads
    sp, x, cell, pbc, lists = load_system(args, dev)
    if args.system == "molecules":
        sp, x = sp[:sp.shape[0] // P], x[:sp.shape[0] // P]
    # (a batch of boxes goes through the all-pairs builder: the cell list handles one system at a time)
    nl = args.neighborlist or ("auto" if cell is not None else lists[0])
    masses = torch.tensor(ELEMENT_MASSES, device=dev)[sp.clamp(min=0)]
    R, A = sp.shape
    rep = lambda t: t.repeat_interleave(P, dim=0)   # noqa: E731
    drivers = {}
    for kind in ("classical", "ring-polymer"):
        model = ANI2x(seed=0, device=dev, periodic_table_index=False, neighborlist=nl, row_capacity=256)
        if kind == "classical":
            md = BatchedDynamics(model, rep(sp), rep(x), cell, pbc, dt=args.dt, masses=rep(masses), temperature=P * args.temperature, seed=1)
            md.set_temperature(P * args.temperature)
        else:
            md = RingPolymerDynamics(model, sp, x, cell, pbc, beads=P, dt=args.dt, masses=masses, temperature=args.temperature, seed=1)
            md.set_temperature(args.temperature)
        md.run(args.warmup)
        drivers[kind] = md
    times = {kind: [] for kind in drivers}
    for _ in range(args.repeats):
        for kind, md in drivers.items():
            times[kind].append(timed(md, args.steps))
    n_atoms = int((sp >= 0).sum()) * P
    for kind, md in drivers.items():
        t = np.array(times[kind]) * 1e3
        extra = ""
        if kind == "ring-polymer":
            extra = (f", spring energy {md.spring_energies().mean().item():.4f} Ha, centroid-virial kinetic energy "
                     f"{md.quantum_kinetic_energies().mean().item():.4f} Ha per polymer")
        print(f"{nl:17s} {kind:12s} {R} x {P} beads x {A} atoms, dt {args.dt:g} fs, {n_atoms} bead atoms: {np.median(t):.3f} ms/step "
              f"(fastest {t.min():.3f}, slowest {t.max():.3f} of {len(t)} repeats of {args.steps} steps) = "
              f"{n_atoms / (np.median(t) * 1e-3) / 1e6:.2f} M bead-atom*steps/s, bead T = {md.temperatures().mean().item():.0f} K{extra}")


def bench_exchange(args, dev):
    """ReplicaExchangeDynamics with --exchange-every against the same class with exchange_every=0 (the step of BatchedDynamics)
    on one [molecules x rungs, A] batch, in one process, the repeats alternating: every molecule is a ladder of --rungs
    replicas on a geometric ladder from --temperature to twice that.  The difference is the attempt's two launches and the
    gather of the temperatures, once per --exchange-every steps."""
    from torchani_amd.md import ReplicaExchangeDynamics, temperature_ladder
    from torchani_amd.models import ANI2x

    K = args.rungs
    sp, x, cell, pbc, lists = load_system(args, dev)
    nl = args.neighborlist or ("auto" if cell is not None else lists[0])
    masses = torch.tensor(ELEMENT_MASSES, device=dev)[sp.clamp(min=0)]
    L, A = sp.shape
    rep = lambda t: t.repeat_interleave(K, dim=0)   # noqa: E731
    T = temperature_ladder(args.temperature, 2.0 * args.temperature, K).repeat(L)
    drivers = {}
    for kind, every in (("no exchange", 0), (f"every {args.exchange_every}", args.exchange_every)):
        model = ANI2x(seed=0, device=dev, periodic_table_index=False, neighborlist=nl, row_capacity=256)
        md = ReplicaExchangeDynamics(model, rep(sp), rep(x), cell, pbc, dt=args.dt, masses=rep(masses), temperature=T, seed=1,
                                     ladders=torch.arange(L * K).view(L, K), exchange_every=every)
        md.set_temperature(T)
        md.run(args.warmup)
        drivers[kind] = md
    times = {kind: [] for kind in drivers}
    for _ in range(args.repeats):
        for kind, md in drivers.items():
            times[kind].append(timed(md, args.steps))
    n_atoms = int((sp >= 0).sum()) * K
    med = {}
    for kind, md in drivers.items():
        t = np.array(times[kind]) * 1e3
        med[kind] = np.median(t)
        extra = ""
        if md.exchange_every:
            extra = (f", {md.attempts_done} attempts, acceptance {md.acceptance_rates().mean().item():.3f}, "
                     f"{int(md.round_trips().sum())} round trips")
        print(f"{nl:17s} {kind:12s} {L} ladders x {K} rungs x {A} atoms, dt {args.dt:g} fs, {n_atoms} atoms: {np.median(t):.3f} ms/step "
              f"(fastest {t.min():.3f}, slowest {t.max():.3f} of {len(t)} repeats of {args.steps} steps) = "
              f"{n_atoms / (np.median(t) * 1e-3) / 1e6:.2f} M atom*steps/s{extra}")
    a, b = med.values()
    print(f"the attempts cost {(b - a) * 1e3:+.1f} us per step at one attempt per {args.exchange_every} steps (medians)")


def bench_bias(args, dev):
    """BatchedDynamics with ``bias=`` against the same step without, in one process, the repeats alternating.  Restraints: one
    launch more per step.  Metadynamics: --hills hills preloaded per list and pace 0, so the count stays what was asked for and
    the step is the hills kernel plus the apply kernel; the deposit (two small launches every pace steps) is not in it."""
    from torchani_amd import md as M
    from torchani_amd.models import ANI2x

    sp, x, cell, pbc, lists = load_system(args, dev)
    nl = args.neighborlist or lists[0]
    masses = torch.tensor(ELEMENT_MASSES, device=dev)[sp.clamp(min=0)]
    Cn, A = sp.shape
    temperature = 300.0 if args.langevin else None
    if args.bias == "restraints":
        cv = M.dihedral(0, 1, 2, 3) if cell is None else M.distance(0, 3)
        bias, what = [M.Restraint(cv, 1.0 if cell is None else 3.0, 0.01)], "one restraint per system"
    elif args.bias == "sites":
        # the two halves of every system's atoms: one gather, one apply and one spread launch more per step
        real = (sp >= 0).cpu()
        first = real & (torch.arange(A).view(1, -1) < (real.sum(dim=1) // 2).view(-1, 1))
        bias = [M.Restraint(M.distance(M.center(first), M.center(real & ~first)), 3.0, 0.01)]
        what = "one restraint on a distance between two centres of mass per system"
    elif args.bias == "coordination":
        if cell is None:
            raise SystemExit("--bias coordination is timed on --system water")
        oxygen, hydrogen = (sp[0] == 3).cpu(), (sp[0] == 0).cpu()   # (ANI-2x element indices)
        if args.coordination_atoms:
            oxygen &= torch.cumsum(oxygen, 0) <= args.coordination_atoms
            hydrogen &= torch.cumsum(hydrogen, 0) <= args.coordination_atoms
        width = 1.0 / torch.linalg.inv(cell.double().cpu()).norm(dim=0).max().item()
        r_max = min(6.0, 0.49 * width)
        bias = [M.Restraint(M.coordination(oxygen, hydrogen, 1.3, n=6, r_max=r_max), 2.0 * int(oxygen.sum()), 1e-6)]
        what = (f"one restraint on the coordination number of {int(oxygen.sum())} O against {int(hydrogen.sum())} H "
                f"({int(oxygen.sum()) * int(hydrogen.sum())} pairs, r_max {r_max:.2f} A)")
    else:
        if cell is not None:
            raise SystemExit("--bias metadynamics is timed on --system molecules")
        rs = np.random.RandomState(0)
        G, H = (1 if args.shared_walkers else Cn), max(1, args.hills)
        centers = np.stack([rs.uniform(-np.pi, np.pi, (G, H)), rs.uniform(1.0, 5.0, (G, H))], axis=1)
        hills = (torch.from_numpy(centers), torch.full((G, H), 1e-6, dtype=torch.float64),
                 torch.full((G,), args.hills, dtype=torch.int64))
        walkers = torch.zeros(Cn, dtype=torch.int64) if args.shared_walkers else None
        bias = [M.Metadynamics([M.dihedral(0, 1, 2, 3), M.distance(0, 4)], (0.3, 0.2), 1e-6, 0, walkers=walkers, max_hills=H,
                               hills=hills)]
        what = f"2-CV metadynamics, {args.hills} hills per list, {'one list of all walkers' if args.shared_walkers else 'a list per system'}"
    drivers = {}
    for kind, b in (("unbiased", None), ("biased", bias)):
        model = ANI2x(seed=0, device=dev, periodic_table_index=False, neighborlist=nl, row_capacity=256)
        d = M.BatchedDynamics(model, sp, x, cell, pbc, dt=args.dt, masses=masses, temperature=temperature, seed=1, bias=b)
        d.set_temperature(300.0)
        d.run(args.warmup)
        drivers[kind] = d
    times = {kind: [] for kind in drivers}
    for _ in range(args.repeats):
        for kind, d in drivers.items():
            times[kind].append(timed(d, args.steps))
    n_atoms = int((sp >= 0).sum())
    t = {kind: np.array(v) * 1e3 for kind, v in times.items()}
    for kind in drivers:
        print(f"{nl:17s} {kind:9s} {Cn} x {A} atoms ({n_atoms} real), dt {args.dt:g} fs: {np.median(t[kind]):.3f} ms/step (fastest "
              f"{t[kind].min():.3f}, slowest {t[kind].max():.3f} of {len(t[kind])} repeats of {args.steps} steps)")
    apart = t["biased"].min() > t["unbiased"].max() or t["biased"].max() < t["unbiased"].min()
    print(f"{what}: {(np.median(t['biased']) - np.median(t['unbiased'])) * 1e3:+.1f} us per step (medians); the ranges "
          f"{'separate' if apart else 'overlap: no difference can be claimed'}")


def make_observer(name, args, cell):
    """One observer of --observe, sampling every --observe-every steps."""
    from torchani_amd import md as M

    every = args.observe_every
    if name == "series":
        return M.TimeSeries(("potential", "kinetic", "temperature"), every=every, capacity=4096, on_full="wrap")
    if name == "trajectory":
        return M.Trajectory(every=every, capacity=8, velocities=True, on_full="wrap")
    if name == "rdf":
        pairs = [("O", "O"), ("O", "H")] if cell is not None else [("C", "C"), ("C", "H")]
        return M.RadialDistribution(pairs, r_max=args.rdf_rmax, bins=200, every=every)
    if name == "heatflux":
        return M.HeatFlux(every=every, capacity=4096, on_full="wrap")
    if name == "hfacf":
        return M.HeatFluxAutocorrelation(lags=args.lags, every=every)
    cls = M.MeanSquaredDisplacement if name == "msd" else M.VelocityAutocorrelation
    return cls(lags=args.lags, every=every, max_bytes=1 << 36)


def observer_bytes(name, obs, d):
    """The bytes one sample of ``obs`` has to move, from shapes (the estimate the measured cost is held against)."""
    n = d.species.numel()
    if name == "series":
        return sum(b[0].numel() * 8 * 2 for b in obs._buffers.values()), "reads and writes of the series' values"
    if name == "trajectory":
        return 2 * 2 * n * 3 * 4, "coordinates and velocities read and written once"
    if name == "rdf":   # the rows of the current coordinates, read once; the build that writes them is in the cost, not in the bytes
        rows = obs._engine.neighbors(obs._species32, d.coordinates, d.cell, d.pbc, mode=obs._mode, row_cap=256)
        entries = int(((rows.meta[:, 1] & 0xFFFF) + ((rows.meta[:, 1] >> 16) & 0xFFFF)).sum())
        return entries * 16 + n * (6 * 4 + 4), f"{entries} row entries of 16 B read once (the cost includes building the rows)"
    if name in ("heatflux", "hfacf"):   # one more evaluation of the model: held against the step, not against bytes
        return 0, "one evaluation of the model's flux stage"
    slots = min(obs.n_samples, obs.lags)
    per = obs._gather.numel() * 3 * obs.bytes_per_value
    return (slots + 1) * per, f"{slots} ring slots of {per} B read, one written"


def bench_observers(args, dev):
    """BatchedDynamics with one observer of --observe attached against the same step without, in one process, the repeats
    alternating: the cost of a sample is the difference of the medians times --observe-every."""
    from torchani_amd import md as M
    from torchani_amd.models import ANI2x

    sp, x, cell, pbc, lists = load_system(args, dev)
    nl = args.neighborlist or lists[0]
    masses = torch.tensor(ELEMENT_MASSES, device=dev)[sp.clamp(min=0)]
    Cn, A = sp.shape
    temperature = 300.0 if args.langevin else None
    drivers, observers = {}, {}
    for kind in ["none"] + list(args.observe):
        model = ANI2x(seed=0, device=dev, periodic_table_index=False, neighborlist=nl, row_capacity=256)
        d = M.BatchedDynamics(model, sp, x, cell, pbc, dt=args.dt, masses=masses, temperature=temperature, seed=1)
        d.set_temperature(300.0)
        if kind != "none":
            try:
                observers[kind] = d.attach(make_observer(kind, args, cell))
            except ValueError as err:   # (hfacf on open molecules: no volume)
                print(f"{kind}: refused ({err})")
                continue
        d.run(max(args.warmup, 2 * args.observe_every))
        drivers[kind] = d
    times = {kind: [] for kind in drivers}
    for _ in range(args.repeats):
        for kind, d in drivers.items():
            times[kind].append(timed(d, args.steps))
    t = {kind: np.array(v) * 1e3 for kind, v in times.items()}
    n_atoms = int((sp >= 0).sum())
    for kind in drivers:
        print(f"{nl:17s} observer {kind:10s} {Cn} x {A} atoms ({n_atoms} real), dt {args.dt:g} fs: {np.median(t[kind]):.3f} ms/step "
              f"(fastest {t[kind].min():.3f}, slowest {t[kind].max():.3f} of {len(t[kind])} repeats of {args.steps} steps)")
    for kind, obs in observers.items():
        apart = t[kind].min() > t["none"].max() or t[kind].max() < t["none"].min()
        per_sample = (np.median(t[kind]) - np.median(t["none"])) * 1e3 * args.observe_every
        nbytes, what = observer_bytes(kind, obs, drivers[kind])
        rate = f"{nbytes / (per_sample * 1e-6) / 1e9:.1f} GB/s of that estimate" if per_sample > 0 else "no cost resolved"
        if kind in ("heatflux", "hfacf"):
            rate = f"{per_sample * 1e-3 / np.median(t['none']):.2f} steps"
        print(f"{kind}: {per_sample:+.1f} us per sample (medians, one sample per {args.observe_every} steps), {obs.n_samples} samples; "
              f"{nbytes} B to move ({what}): {rate}; the ranges {'separate' if apart else 'overlap: no difference can be claimed'}")


def bench_flux_backward(args, dev):
    """The flux backward's own time against the force backward on the same rows and dE/dAEV (events around each launch, the two
    alternating)."""
    from torchani_amd.models import ANI2x

    sp, x, cell, pbc, lists = load_system(args, dev)
    model = ANI2x(seed=0, device=dev, periodic_table_index=False, neighborlist=args.neighborlist or lists[0], row_capacity=256)
    aevc, eng = model.aev_computer, model.aev_computer.engine()
    sp32, n = sp.to(torch.int32).contiguous(), sp.numel()
    c32 = x.to(torch.float32).contiguous()
    v = torch.randn((n, 3), device=dev) * 0.01
    nbrs = aevc.neighbor_rows(sp32, c32, cell, pbc, lo=0, hi=n)
    packed = model.neural_networks._pack(dev, None)
    mask = torch.empty(n, dtype=torch.int32, device=dev)
    aev = eng.forward(sp32, nbrs, slab_mask=mask, shard_rows=True)
    _, grad_aev, _ = packed.forward_backward(sp32, aev, lo=0, hi=n, want_grad=True, slab_mask=mask, shard_rows=True)
    acc = torch.zeros((n, 3), device=dev)
    runs = {"force backward": lambda: eng.backward(sp32, nbrs, grad_aev, grad_coords=acc, shard_rows=True, slab_mask=mask),
            "flux backward": lambda: eng.backward_flux(sp32, nbrs, grad_aev, v, slab_mask=mask, shard_rows=True)}
    t = {k: [] for k in runs}
    for r in range(args.repeats + 2):
        for k, f in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            if r >= 2:
                t[k].append(a.elapsed_time(b))
    for k, v_ in t.items():
        print(f"{k:15s} {n} atoms: {np.median(v_):.3f} ms (fastest {min(v_):.3f}, slowest {max(v_):.3f} of {len(v_)}; the flux "
              "backward includes the allocation of its [N, 3] result)")


def timed(md, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    md.run(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--system", choices=("water", "molecules"), default="water")
    ap.add_argument("--integrator", choices=("host", "device", "both"), default="host")
    ap.add_argument("--neighborlist", choices=("cell_list", "verlet_cell_list"), default=None,
                    help="--system water: time this neighbor list alone (default: both)")
    ap.add_argument("--langevin", action="store_true", help="Langevin dynamics at 300 K, friction 0.002 / fs (default: NVE)")
    ap.add_argument("--dt", type=float, default=0.5, help="time step, fs")
    ap.add_argument("--constraints", nargs="+", choices=("none", "hydrogens", "rigid-water"), default=["none"],
                    help="device integrator: X-H bonds (hydrogens) or whole waters (rigid-water) held rigid; several values are "
                         "timed against each other in one process")
    ap.add_argument("--barostat", action="store_true",
                    help="device integrator with --langevin: NVT, NVT with the virial-carrying evaluation and NPT timed against "
                         "each other in one process")
    ap.add_argument("--pressure", type=float, default=None, help="--barostat: target in bar (default: the initial pressure)")
    ap.add_argument("--barostat-time", type=float, default=1000.0, help="--barostat: relaxation time, fs")
    ap.add_argument("--beads", type=int, default=None,
                    help="path-integral MD with this many beads against the classical Langevin step on the same batch")
    ap.add_argument("--temperature", type=float, default=300.0,
                    help="--beads: the physical temperature, K; --exchange-every: the lowest rung (the highest is twice that)")
    ap.add_argument("--exchange-every", type=int, default=None,
                    help="temperature replica exchange with one attempt per this many steps against the same step without")
    ap.add_argument("--rungs", type=int, default=8, help="--exchange-every: replicas per ladder")
    ap.add_argument("--coordination-atoms", type=int, default=0,
                    help="--bias coordination: the first N oxygens against the first N hydrogens (default: all against all)")
    ap.add_argument("--bias", choices=("restraints", "metadynamics", "sites", "coordination"), default=None,
                    help="the device integrator with this bias against the same step without")
    ap.add_argument("--hills", type=int, default=1000, help="--bias metadynamics: hills held by every list")
    ap.add_argument("--shared-walkers", action="store_true", help="--bias metadynamics: every system a walker of one list")
    ap.add_argument("--observe", nargs="+", choices=("series", "trajectory", "rdf", "msd", "vacf", "heatflux", "hfacf"),
                    default=None,
                    help="the device integrator with each of these observers attached against the same step without")
    ap.add_argument("--observe-every", type=int, default=10, help="--observe: steps between samples")
    ap.add_argument("--lags", type=int, default=512, help="--observe msd / vacf: lags held")
    ap.add_argument("--rdf-rmax", type=float, default=5.0, help="--observe rdf: r_max, Angstrom")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--force-verlet", action="store_true",
                    help="refresh the skin list at every size (VerletRows.rebuild_above = inf): how the crossover was measured")
    args = ap.parse_args()
    from torchani_amd.models import ANI2x

    dev = torch.device("cuda:0")
    if args.beads is not None:
        return bench_beads(args, dev)
    if args.exchange_every is not None:
        if args.exchange_every < 1 or args.rungs < 2:
            ap.error("--exchange-every must be >= 1 and --rungs >= 2")
        return bench_exchange(args, dev)
    if args.bias is not None:
        if args.hills < 0:
            ap.error("--hills must be >= 0")
        return bench_bias(args, dev)
    if args.observe is not None:
        if args.observe_every < 1 or args.lags < 1:
            ap.error("--observe-every and --lags must be >= 1")
        bench_observers(args, dev)
        if "heatflux" in args.observe:
            bench_flux_backward(args, dev)
        return
    sp, x, cell, pbc, lists = load_system(args, dev)
    if args.neighborlist is not None and args.system == "water":
        lists = (args.neighborlist,)
    n_atoms = int((sp >= 0).sum())
    masses = torch.tensor(ELEMENT_MASSES, device=dev)[sp.clamp(min=0)]
    kinds = ("host", "device") if args.integrator == "both" else (args.integrator,)
    if args.constraints != ["none"]:
        if "device" not in kinds:
            ap.error("--constraints needs the device integrator")
        kinds = tuple(k for k in kinds if k != "device") + tuple("device" if c == "none" else "device+" + c
                                                                 for c in args.constraints)
    if args.barostat:
        if args.integrator != "device" or not args.langevin or cell is None or len(args.constraints) != 1:
            ap.error("--barostat needs --integrator device, --langevin, a periodic system and at most one kind of --constraints")
        held = "" if args.constraints == ["none"] else "+" + args.constraints[0]
        kinds = ("device" + held, "device+virial" + held, "device+npt" + held)
    for nl in lists:
        drivers = {}
        for kind in kinds:   # (a model each: the automatic HIP graph of a small system belongs to one species tensor)
            # (BatchedDynamics never reads the overflow status inside a step, so it cannot retry with longer neighbor rows as
            # the host driver's evaluation does: when it is timed, both models get the longest rows from the start)
            rows = {"row_capacity": 256} if any(k.startswith("device") for k in kinds) else {}
            model = ANI2x(seed=0, device=dev, periodic_table_index=False, neighborlist=nl, **rows)
            if args.force_verlet and model.aev_computer.verlet is not None:
                model.aev_computer.verlet.rebuild_above = float("inf")
            drivers[kind] = make_driver(kind, args, model, sp, x, cell, pbc, masses)
            drivers[kind].run(args.warmup)
        times = {kind: [] for kind in kinds}
        for _ in range(args.repeats):
            for kind in kinds:
                times[kind].append(timed(drivers[kind], args.steps))
        for kind in kinds:
            md, t = drivers[kind], np.array(times[kind]) * 1e3
            ver = md.model.aev_computer.verlet
            extra = (f", pair searches {ver.n_builds}, reuses {ver.n_reuses}, steps rebuilt outright {ver.n_direct}"
                     if ver is not None else "")
            spread = f" (fastest {t.min():.3f}, slowest {t.max():.3f} of {len(t)} repeats)" if len(t) > 1 else ""
            if getattr(md, "_clusters", None) is not None:   # the counts of the last step
                it = md.constraint_iterations.double().mean(dim=0).tolist()
                extra += (f", {int(md.n_constraints.sum())} constraints in {md.constraint_iterations.shape[0]} clusters, mean "
                          f"iterations of the last step: positions {it[0]:.2f}, velocities {it[1]:.2f}")
            if getattr(md, "barostat", False):
                extra += (f", target {md.pressure.item():.4g} bar, P = {md.pressures().item():.4g} bar, V / V0 = "
                          f"{md.volumes().item() / md.volume0:.5f}")
            print(f"{nl:17s} {kind:26s} {'langevin' if args.langevin else 'nve':8s} dt {args.dt:g} fs {n_atoms} atoms: "
                  f"{np.median(t):.3f} ms/step{spread} = {n_atoms / (np.median(t) * 1e-3) / 1e6:.2f} M atom*steps/s, "
                  f"{args.dt / (np.median(t) * 1e-3):.0f} fs simulated per second, T = {md.temperatures().mean().item():.0f} K{extra}")


if __name__ == "__main__":
    main()
