"""Minimal molecular-dynamics driver around ``ANI.energies_and_forces``.

The production caller of the energy+forces path in the reference is an ASE ``Calculator`` driving ASE's integrators
(torchani/ase.py:32-173, tools/md-benchmark.py); ASE is not available here, so this module carries the two pieces the
benchmark needs: a velocity-Verlet / Langevin (BAOAB) integrator on device tensors and the unit conventions
(Hartree, Angstrom, amu, fs).  Combined with ``neighborlist="verlet_cell_list"`` the pair search is reused between
steps (VerletCellList, neighbors.py:759-884).

``MolecularDynamics`` is host code only: every step is one stream-ordered ``energies_and_forces`` call plus a handful of
elementwise updates.  ``BatchedDynamics`` keeps the state on the device and integrates in libanihip (csrc/md.hip): two or
three launches around the force evaluation, no host synchronization in a step, a temperature and a friction per molecule,
fixed atoms, noise that is a pure function of (seed, step, replica id, atom) and coordinates kept as pairs of floats.
Bond-length constraints (``BondConstraints``, ``hydrogen_constraints``: SHAKE / RATTLE per cluster of coupled constraints) add
one launch to each half of the step.  ``pressure=`` adds an isotropic stochastic-cell-rescaling barostat (Bernetti and Bussi
2020) between the drift and the force evaluation: two launches that rescale the cell, the positions and the velocities.
With constraints, ``barostat_scaling="molecular"`` moves every constraint cluster as a rigid body instead (three launches, and
two or three after the kick for the centre-of-mass kinetic energy and the internal virial of the clusters).
``RingPolymerDynamics`` is path-integral MD on the same machinery: the batch holds the beads of R ring polymers, and its drift is
one launch that propagates the free ring polymer exactly in its normal modes with the PILE thermostat on them.
``ReplicaExchangeDynamics`` is temperature replica exchange over the entries of the batch: every ``exchange_every`` steps two
launches swap the temperatures of neighboring rungs of every ladder by the Metropolis rule and rescale the velocities.
``bias=`` adds restraints on collective variables (``distance``, ``angle``, ``dihedral``; ``Restraint``) and ``Metadynamics`` to
the forces between the evaluation and the kick (csrc/md_bias.hip): one launch more per evaluation, two with hills, and two per
deposit.  ``center`` (the centre of a group of atoms, usable wherever a CV takes an atom) and ``coordination`` (a coordination
number between two groups) enter the same kernels as sites appended to every entry (csrc/md_sites.hip): a gather in front of
them, at most two launches, and a spread behind them, one.
``attach(observer)`` samples a trajectory on the device inside ``step()`` (md_observe.py, csrc/md_observe.hip): ``TimeSeries``,
``Trajectory``, ``RadialDistribution``, ``MeanSquaredDisplacement``, ``VelocityAutocorrelation``, ``HeatFlux`` and
``HeatFluxAutocorrelation`` (the last two evaluate the model once more per sample).
``MBAR`` (md_mbar.py, csrc/mbar.hip) turns the series of umbrella windows and temperature ladders into free energies, potentials
of mean force and averages reweighted to states that were not sampled, on the device.
"""
from __future__ import annotations

import ctypes as C
import math
import typing as tp

import torch
from torch import Tensor

from . import _lib
from .md_bias import (CV, BiasTables, DeviceBias, Metadynamics, Restraint, Site, SiteTables, angle, build_bias_tables,  # noqa: F401
                      build_site_tables, center, coordination, dihedral, distance)
from .md_mbar import MBAR, ThermodynamicStates  # noqa: F401
from .md_observe import (HeatFlux, HeatFluxAutocorrelation, MeanSquaredDisplacement, Observer,  # noqa: F401
                         RadialDistribution, TimeSeries, Trajectory, VelocityAutocorrelation)

# CODATA 2018: 1 Ha = 4.3597447222071e-18 J, 1 amu = 1.66053906660e-27 kg  ->  (Ha / Angstrom) / amu in Angstrom / fs^2
ACC_UNIT = 4.3597447222071e-18 / 1e-10 / 1.66053906660e-27 * 1e10 * 1e-30
KB_HARTREE = 3.166811563e-6          # Boltzmann constant, Ha / K
BAR_PER_HARTREE_ANGSTROM3 = 4.3597447222071e7   # 1 Ha / Angstrom^3 = 4.3597447222071e-18 J / 1e-30 m^3, in bar (1e5 Pa)
ATOMIC_MASS = {1: 1.008, 6: 12.011, 7: 14.007, 8: 15.999, 9: 18.998, 16: 32.06, 17: 35.45}   # amu


def default_masses(model, species: Tensor) -> Tensor:
    """ATOMIC_MASS looked up by atomic number (fp32, on the device of ``species``); padding atoms get lut[0] = 0."""
    if not getattr(model, "periodic_table_index", False):   # (a standalone pair potential has no such attribute)
        raise ValueError("pass masses when species are element indices")
    lut = torch.zeros(120, dtype=torch.float32)
    for z, m in ATOMIC_MASS.items():
        lut[z] = m
    return lut.to(species.device)[species.clamp(min=0)]


class MolecularDynamics:
    """NVE (velocity Verlet) or NVT (Langevin, BAOAB splitting) dynamics of one system or a batch of molecules.

    species [C, A] (atomic numbers, or element indices if the model was built with periodic_table_index=False --
    then pass ``masses``), coords [C, A, 3] in Angstrom (kept unwrapped), dt in fs.
    """

    def __init__(self, model, species: Tensor, coords: Tensor, cell: tp.Optional[Tensor] = None,
                 pbc: tp.Optional[tp.Sequence[bool]] = None, dt: float = 0.5, masses: tp.Optional[Tensor] = None,
                 temperature: tp.Optional[float] = None, friction: float = 0.002, seed: int = 0) -> None:
        if not coords.is_cuda:
            raise ValueError("MolecularDynamics needs tensors on a ROCm device (no CPU fallback)")
        self.model, self.species, self.cell, self.pbc, self.dt = model, species, cell, pbc, float(dt)
        self.coords = coords.detach().to(torch.float32).clone().contiguous()
        if masses is None:
            masses = default_masses(model, species.to(coords.device))
        self.masses = masses.to(device=coords.device, dtype=torch.float32)
        self.real = (species >= 0)
        self.inv_m = torch.where(self.real, ACC_UNIT / self.masses.clamp(min=1e-6),
                                 torch.zeros_like(self.masses)).unsqueeze(-1)
        self.velocities = torch.zeros_like(self.coords)        # Angstrom / fs
        self.temperature, self.friction = temperature, float(friction)
        self.gen = torch.Generator(device=coords.device).manual_seed(seed)
        self.steps_done = 0
        self._eval()

    def _eval(self) -> None:
        out = self.model.energies_and_forces(self.species, self.coords, self.cell, self.pbc)
        self.potential_energies, self.forces = out.energies, out.forces

    # ---- observables (Hartree, K) ----------------------------------------------------------------------------
    def kinetic_energies(self) -> Tensor:
        ke = 0.5 * (self.masses.unsqueeze(-1) * self.velocities.pow(2)).sum(dim=(1, 2)) / ACC_UNIT
        return ke.double()

    def total_energies(self) -> Tensor:
        return self.potential_energies + self.kinetic_energies()

    def temperatures(self) -> Tensor:
        dof = 3.0 * self.real.sum(dim=1).clamp(min=1).double()
        return 2.0 * self.kinetic_energies() / (dof * KB_HARTREE)

    def set_temperature(self, kelvin: float) -> None:
        """Maxwell-Boltzmann velocities."""
        sigma = torch.sqrt(KB_HARTREE * kelvin * ACC_UNIT / self.masses.clamp(min=1e-6)).unsqueeze(-1)
        noise = torch.randn(self.coords.shape, generator=self.gen, device=self.coords.device)
        self.velocities = torch.where(self.real.unsqueeze(-1), sigma * noise, torch.zeros_like(noise))

    # ---- integrator --------------------------------------------------------------------------------------------
    def run(self, n_steps: int) -> None:
        dt = self.dt
        for _ in range(n_steps):
            self.velocities += (0.5 * dt) * self.forces * self.inv_m
            if self.temperature is None:
                self.coords += dt * self.velocities
            else:   # BAOAB: half drift, Ornstein-Uhlenbeck kick, half drift
                self.coords += (0.5 * dt) * self.velocities
                c1 = math.exp(-self.friction * dt)
                sigma = torch.sqrt(KB_HARTREE * self.temperature * ACC_UNIT * (1.0 - c1 * c1)
                                   / self.masses.clamp(min=1e-6)).unsqueeze(-1)
                noise = torch.randn(self.coords.shape, generator=self.gen, device=self.coords.device)
                self.velocities = torch.where(self.real.unsqueeze(-1), c1 * self.velocities + sigma * noise,
                                              torch.zeros_like(noise))
                self.coords += (0.5 * dt) * self.velocities
            self._eval()
            self.velocities += (0.5 * dt) * self.forces * self.inv_m
            self.steps_done += 1


_MB_STEP = 1 << 63   # Philox step words of the Maxwell-Boltzmann draws: the top bit set, apart from every drift's


def _per_molecule(value, name: str, n_mol: int) -> Tensor:
    """A number or a [C] tensor as fp32 [C] on the host's side of the argument checks (>= 0)."""
    t = torch.as_tensor(value, dtype=torch.float32)
    if t.dim() == 0:
        t = t.expand(n_mol)
    if tuple(t.shape) != (n_mol,):
        raise ValueError(f"{name} must be a number or a tensor of shape ({n_mol},), got {tuple(t.shape)}")
    if not bool((t >= 0).all()):
        raise ValueError(f"{name} must be >= 0")
    return t


# ---- bond-length constraints: the host side ---------------------------------------------------------------------------------

class BondConstraints:
    """Bond-length constraints of a batch: ``pairs`` int64 [C, K, 2], atom indices within each molecule, padded with (-1, -1);
    ``lengths`` [C, K] in Angstrom, or None for the distances in the initial coordinates."""

    def __init__(self, pairs: Tensor, lengths: tp.Optional[Tensor] = None) -> None:
        if pairs.dim() != 3 or pairs.shape[2] != 2 or pairs.dtype != torch.int64:
            raise ValueError("pairs must be an int64 tensor of shape [C, K, 2]")
        if lengths is not None and tuple(lengths.shape) != tuple(pairs.shape[:2]):
            raise ValueError(f"lengths must have shape {tuple(pairs.shape[:2])}, got {tuple(lengths.shape)}")
        self.pairs = pairs
        self.lengths = None if lengths is None else lengths.to(torch.float64)

    def counts(self) -> Tensor:
        """Constraints per molecule, int64 [C]."""
        return (self.pairs[..., 0] >= 0).sum(dim=1)


class ConstraintClusters(tp.NamedTuple):
    """The cluster tables of include/anihip.h (host tensors) and what the integrator derives from them."""
    atoms: Tensor          # int32 [Q, 8]: global atom index c A + i of each slot in ascending order, -1 past the cluster
    count: Tensor          # int32 [Q, 2]: atoms and constraints of the cluster
    bonds: Tensor          # uint8 [Q, 12, 2]: slots (a, b) of each constraint, in the order of ``pairs``
    d2: Tensor             # float64 [Q, 12]: squared lengths
    w: Tensor              # float64 [Q, 8]: inv_mass of each slot, 0 for a fixed atom
    molecule: Tensor       # int64 [Q]
    per_molecule: Tensor   # int64 [C]: constraints of each molecule
    owned: Tensor          # bool [C, A]: the active atoms that clusters move


def _ranks(group: Tensor, n_groups: int) -> tp.Tuple[Tensor, Tensor]:
    """The position of every element within its group, in the order given, and the group sizes."""
    size = torch.bincount(group, minlength=n_groups)
    order = torch.argsort(group, stable=True)
    rank = torch.empty_like(group)
    rank[order] = torch.arange(group.numel()) - (torch.cumsum(size, 0) - size)[group[order]]
    return rank, size


def build_constraint_clusters(species: Tensor, pairs: Tensor, lengths: Tensor, fixed: tp.Optional[Tensor] = None,
                              inv_mass: tp.Optional[Tensor] = None) -> ConstraintClusters:
    """Group the constraints ``pairs`` [C, K, 2] (padded with -1) of lengths [C, K] into clusters, the connected components
    of the constraint graph, and lay out the tables of include/anihip.h.  Pure host torch; the tensors may live anywhere.

    Clusters are ordered by their smallest atom, slots by atom index, constraints as in ``pairs``.  w = inv_mass [C, A] (1 if
    None) of an active atom and 0 of a fixed one.  Raises ValueError for a padding atom, a pair of two fixed atoms, a repeated
    pair, a cluster of more than 8 atoms or 12 constraints, and one of n atoms with more than 3n - 6 constraints (1 for n = 2,
    3 for n = 3), which no geometry satisfies independently."""
    NA, NB = _lib.MD_CLUSTER_ATOMS, _lib.MD_CLUSTER_BONDS
    species, pairs = species.cpu(), pairs.cpu().to(torch.int64)
    if species.dim() != 2 or pairs.dim() != 3 or pairs.shape[0] != species.shape[0] or pairs.shape[2] != 2:
        raise ValueError("expected species [C, A] and pairs [C, K, 2]")
    Cn, A = species.shape
    if tuple(lengths.shape) != tuple(pairs.shape[:2]):
        raise ValueError(f"lengths must have shape {tuple(pairs.shape[:2])}, got {tuple(lengths.shape)}")
    lengths = lengths.cpu().to(torch.float64)
    real = species >= 0
    fx = torch.zeros_like(real) if fixed is None else fixed.cpu().to(torch.bool)
    active = real & ~fx
    if bool(((pairs < 0).any(dim=-1) & ~(pairs == -1).all(dim=-1)).any()):
        raise ValueError("pairs are padded with (-1, -1): a pair with one negative index")
    mol, k = (pairs[..., 0] >= 0).nonzero(as_tuple=True)
    i, j, d = pairs[mol, k, 0], pairs[mol, k, 1], lengths[mol, k]

    def where(bad: Tensor) -> str:
        b = int(bad.nonzero()[0])
        return f"molecule {int(mol[b])}, pair {int(k[b])} = ({int(i[b])}, {int(j[b])})"

    bad = (i >= A) | (j >= A) | (i == j)
    if bool(bad.any()):
        raise ValueError(f"a constraint needs two different atoms below {A}: {where(bad)}")
    bad = ~(real[mol, i] & real[mol, j])
    if bool(bad.any()):
        raise ValueError(f"constraint on a padding atom: {where(bad)}")
    bad = ~(active[mol, i] | active[mol, j])
    if bool(bad.any()):
        raise ValueError(f"constraint between two fixed atoms: {where(bad)}")
    bad = ~(torch.isfinite(d) & (d > 0))
    if bool(bad.any()):
        raise ValueError(f"constraint lengths must be > 0: {where(bad)}")
    N = Cn * A
    gi, gj = mol * A + i, mol * A + j
    key = torch.minimum(gi, gj) * N + torch.maximum(gi, gj)
    if torch.unique(key).numel() != key.numel():
        first = {}
        for b, kk in enumerate(key.tolist()):
            if kk in first:
                bad = torch.zeros_like(key, dtype=torch.bool)
                bad[b] = True
                raise ValueError(f"constraint given twice: {where(bad)}")
            first[kk] = b
    # connected components by passing the smallest label along the constraints: a component of at most 8 atoms has a
    # diameter of at most 7, so labels still moving in round 8 belong to a larger one
    label = torch.arange(N)
    for _ in range(NA):
        low = torch.minimum(label[gi], label[gj])
        new = label.scatter_reduce(0, gi, low, "amin").scatter_reduce(0, gj, low, "amin")
        moved = new != label
        label = new
        if not bool(moved.any()):
            break
    else:
        at = int(moved.nonzero()[0])
        raise ValueError(f"a cluster of coupled constraints has more than {NA} atoms (molecule {at // A}, around atom {at % A})")
    nodes = torch.unique(torch.cat([gi, gj]))
    roots, q_node = torch.unique(label[nodes], return_inverse=True)
    Q = roots.numel()
    slot, n_atoms = _ranks(q_node, Q)
    if Q and int(n_atoms.max()) > NA:
        q = int(n_atoms.argmax())
        raise ValueError(f"a cluster of coupled constraints has more than {NA} atoms "
                         f"(molecule {int(roots[q]) // A}, around atom {int(roots[q]) % A}: {int(n_atoms[q])})")
    q_of, slot_of = torch.full((N,), -1, dtype=torch.int64), torch.full((N,), -1, dtype=torch.int64)
    q_of[nodes], slot_of[nodes] = q_node, slot
    qb = q_of[gi]
    bslot, n_bonds = _ranks(qb, Q)
    limit = torch.where(n_atoms == 2, torch.ones_like(n_atoms), 3 * n_atoms - 6)
    for bad, what in ((n_bonds > NB, f"more than {NB} constraints"), (n_bonds > limit, "more constraints than 3n - 6 (1 for n = 2)")):
        if bool(bad.any()):
            q = int(bad.nonzero()[0])
            raise ValueError(f"the cluster of molecule {int(roots[q]) // A} with smallest atom {int(roots[q]) % A} has {what}: "
                             f"{int(n_atoms[q])} atoms, {int(n_bonds[q])} constraints")
    atoms = torch.full((Q, NA), -1, dtype=torch.int32)
    atoms[q_node, slot] = nodes.to(torch.int32)
    bonds = torch.zeros((Q, NB, 2), dtype=torch.uint8)
    bonds[qb, bslot, 0], bonds[qb, bslot, 1] = slot_of[gi].to(torch.uint8), slot_of[gj].to(torch.uint8)
    d2 = torch.zeros((Q, NB), dtype=torch.float64)
    d2[qb, bslot] = d * d
    w_atom = torch.ones((Cn, A), dtype=torch.float64) if inv_mass is None else inv_mass.cpu().to(torch.float64)
    w_atom = torch.where(active, w_atom, torch.zeros_like(w_atom)).reshape(-1)
    w = torch.zeros((Q, NA), dtype=torch.float64)
    w[q_node, slot] = w_atom[nodes]
    owned = torch.zeros(N, dtype=torch.bool)
    owned[nodes] = True
    return ConstraintClusters(atoms, torch.stack([n_atoms, n_bonds], dim=1).to(torch.int32), bonds, d2, w, roots // A,
                              torch.bincount(mol, minlength=Cn), owned.view(Cn, A) & active)


def hydrogen_constraints(species: Tensor, coordinates: Tensor, cell: tp.Optional[Tensor] = None, pbc=None,
                         max_bond: float = 1.25, rigid_water: bool = False, *, hydrogen: int = 1,
                         oxygen: int = 8) -> BondConstraints:
    """X-H constraints from the geometry: every hydrogen is paired with its nearest heavy atom within ``max_bond`` Angstrom;
    with ``rigid_water`` the H-H pair of every oxygen that holds exactly two such hydrogens and has no heavy atom within
    1.3 ``max_bond`` is added, which makes the water rigid.  Lengths are the distances in ``coordinates``.

    ``hydrogen`` and ``oxygen`` are the values of ``species`` that mark the two elements: atomic numbers by default, 0 and 3
    for ANI-2x element indices.  With a cell the pairs of each system come from the engine's cell list (``aev.cell_list``,
    minimum image); without one, from the distance matrix of each molecule.  The integrator takes the plain difference of the
    unwrapped coordinates, so a bonded pair whose plain difference is not its minimum-image difference raises: unwrap the
    molecule first.  Pairs are ordered X-H by hydrogen index, then H-H by oxygen index."""
    if species.dim() != 2 or tuple(coordinates.shape) != (species.shape[0], species.shape[1], 3):
        raise ValueError("expected species [C, A] and coordinates [C, A, 3]")
    Cn, A = species.shape
    reach = 1.3 * max_bond if rigid_water else max_bond
    per_mol: tp.List[tp.Tuple[Tensor, Tensor]] = []
    for c in range(Cn):
        sp, x = species[c], coordinates[c].detach().to(torch.float64)
        # candidate pairs (i, j), each once: their minimum-image distance and whether the plain difference is another
        if cell is None:
            dist = (x.unsqueeze(1) - x.unsqueeze(0)).norm(dim=-1)
            real = sp >= 0
            i, j = torch.triu(real.unsqueeze(1) & real.unsqueeze(0) & (dist <= reach), diagonal=1).nonzero(as_tuple=True)
            dist = dist[i, j]
            wrapped = torch.zeros_like(i, dtype=torch.bool)
        else:
            from .aev import cell_list

            nb = cell_list(reach, species[c:c + 1], coordinates[c:c + 1], cell, pbc)
            i, j, dist = nb.indices[0], nb.indices[1], nb.distances.to(torch.float64)
            wrapped = ((x[i] - x[j]) - nb.diff_vectors.to(torch.float64)).abs().amax(dim=-1) > 1e-3
        a, b = torch.cat([i, j]), torch.cat([j, i])   # both orientations
        dist, wrapped = torch.cat([dist, dist]), torch.cat([wrapped, wrapped])
        a_h, b_h = sp[a] == hydrogen, sp[b] == hydrogen
        xh = a_h & ~b_h & (dist <= max_bond)
        h, heavy, dh, wr = a[xh], b[xh], dist[xh], wrapped[xh]
        # the nearest heavy atom of each hydrogen (the smallest index among equals)
        best = torch.full((A,), float("inf"), dtype=torch.float64, device=x.device).scatter_reduce(0, h, dh, "amin")
        near = dh == best[h]
        h, heavy, wr = h[near], heavy[near], wr[near]
        order = torch.argsort(h * A + heavy)
        h, heavy, wr = h[order], heavy[order], wr[order]
        first = torch.ones_like(h, dtype=torch.bool)
        first[1:] = h[1:] != h[:-1]
        h, heavy, wr = h[first], heavy[first], wr[first]
        if bool(wr.any()):
            bad = int(wr.nonzero()[0])
            raise ValueError(f"system {c}: the bond between atoms {int(heavy[bad])} and {int(h[bad])} crosses the cell boundary "
                             "(its plain difference is not its minimum-image difference); unwrap the molecule so that "
                             "its atoms lie next to each other")
        prs = torch.stack([heavy, h], dim=1)
        if rigid_water:
            n_h = torch.bincount(heavy, minlength=A)
            n_heavy = torch.bincount(a[~a_h & ~b_h], minlength=A)
            water = (sp == oxygen) & (n_h == 2) & (n_heavy == 0)
            sel = water[heavy]   # (sorted by hydrogen: a stable sort by oxygen keeps each water's hydrogens in order)
            hw = h[sel][torch.argsort(heavy[sel], stable=True)]
            prs = torch.cat([prs, hw.view(hw.numel() // 2, 2)])
        lens = (x[prs[:, 0]] - x[prs[:, 1]]).norm(dim=-1)
        per_mol.append((prs.cpu(), lens.cpu()))
    K = max(1, max(p.shape[0] for p, _ in per_mol))
    pairs = torch.full((Cn, K, 2), -1, dtype=torch.int64)
    lengths = torch.zeros((Cn, K), dtype=torch.float64)
    for c, (p, l) in enumerate(per_mol):
        pairs[c, :p.shape[0]], lengths[c, :p.shape[0]] = p, l
    return BondConstraints(pairs, lengths)


class BatchedDynamics:
    """NVE (velocity Verlet) or Langevin (BAOAB) dynamics of every molecule of species [C, A], coordinates [C, A, 3]
    (Angstrom, kept unwrapped), integrated on the device (csrc/md.hip; include/anihip.h has the exact definition).

    dt in fs.  temperature: None (NVE), a number or a [C] tensor in K (Langevin; one thermostat per molecule); friction: a
    number or a [C] tensor in 1 / fs.  Both become the device tensors ``temperature`` and ``friction`` (fp32 [C]), which may
    be overwritten between steps (annealing, replica ladders).  fixed: bool [C, A] atoms that never move.  replica_ids: int64
    [C] in 0 .. 2^32 - 1, the noise stream of each molecule (default: its batch index) -- a replica draws the same noise wherever it sits in
    the batch.  remove_drift: ``set_temperature`` removes each molecule's centre-of-mass velocity.

    constraints: a ``BondConstraints`` (``hydrogen_constraints`` makes one) of bond lengths to hold, by SHAKE / RATTLE in a
    geodesic BAOAB step (include/anihip.h): coupled constraints form clusters of at most 8 atoms and 12 constraints, the
    difference of two atoms is the plain one of the unwrapped coordinates (no minimum image), and there are no angle
    constraints.  Given ``lengths`` are imposed on the initial coordinates, and a bond more than 10 % off raises (a wrapped
    molecule or a wrong index).  ``constraint_tolerance`` is the relative residual to converge to, ``constraint_max_iterations``
    the sweeps allowed; ``run()`` raises when a cluster used them all.  ``temperatures()`` takes one degree of freedom off per
    constraint.  None, or pairs that are all padding, leaves the trajectory bit-identical to the unconstrained one.

    pressure: None (the cell never changes), or the target pressure in bar (a number or a [1] tensor) of an isotropic
    stochastic-cell-rescaling barostat (Bernetti and Bussi 2020; include/anihip.h has the exact move), with ``compressibility``
    the isothermal compressibility in 1 / bar (default: water's) and ``barostat_time`` the relaxation time in fs.  ``step()``
    becomes drift, barostat, evaluation, kick: the move uses the virial of the previous evaluation and the kinetic energy of
    the previous kick, and the forces always belong to the rescaled coordinates.  It needs Langevin dynamics (its noise is
    scaled by kT), one system (C = 1) in a cell periodic in all three directions, no fixed atoms and, with the default
    ``barostat_scaling="atomic"``, no constraints (x <- mu x would rescale every bond).  ``cell`` is then an fp32 clone that
    the dynamics owns and updates in place, ``cell64`` its fp64 master, and ``pressure`` an fp64 [1] device tensor in bar that
    may be overwritten between steps; ``volumes()`` and ``pressures()`` are the observables.  Every evaluation carries the virial (``stress=True``), which
    turns off the automatic HIP graph of small systems; ``neighborlist="verlet_cell_list"`` compares the cell with the one of
    its list on the host at every step, so it synchronizes and rebuilds whenever the cell has moved; a box that shrinks until
    a neighbor row overflows is caught by the overflow check of ``run()``.

    barostat_scaling: "atomic" (the default: every atom is rescaled), or "molecular", which accepts ``constraints``: every
    constraint cluster is translated rigidly by the displacement of its rescaled centre of mass, every other atom is rescaled
    as before, and the pressure is the molecular one, from the centre-of-mass kinetic energy of the clusters and the virial
    under that same scaling (anihip_md_group_terms and anihip_md_barostat_groups in include/anihip.h).  Bond vectors and
    relative velocities are untouched, so the constraints hold without another solver pass.  ``pressures()`` is then the
    molecular pressure; ``temperatures()`` is unchanged.  Every other restriction of the barostat stays.

    bias: None, or a sequence of ``Restraint`` and at most one ``Metadynamics`` on collective variables (``distance``,
    ``angle``, ``dihedral``: atoms of one entry, plain differences of the unwrapped coordinates, fp64; include/anihip.h has
    the exact definition).  Every evaluation is then the model followed by anihip_md_bias_apply on the forces held, so
    ``forces`` carries the bias and constraints compose as they are; ``potential_energies`` stays the model's, ``bias_energies``
    (fp64 [C], restraints + hills) is new and ``total_energies()`` includes it.  With a ``Metadynamics`` of pace p, ``step()``
    deposits after the kick whenever ``steps_done`` is a multiple of p: every walker appends one hill at its CV values, of the
    height that the bias just computed gives (all walkers see the bias of before the round), and the hills act from the next
    evaluation on; nothing is deposited at construction.  ``step()`` raises on the host before a deposit that would not fit
    ``max_hills``.  A CV may sit on a fixed atom (an anchor).  ``pressure=`` with ``bias=`` raises: the bias has no virial here.
    None, or a bias with no CV in any entry, launches nothing more and is bit-identical to the unbiased dynamics.  An index of
    a CV may be a ``center(atoms, weights="mass" | None)`` of a group of atoms (mass weights are the ``masses`` given, or the
    default ones), and ``coordination(group_a, group_b, r0, d0=0, n=6, r_max=None)`` is a CV like the others; its distances
    take the minimum image of ``cell`` along ``pbc`` (then ``r_max`` is needed, at most half the smallest perpendicular width),
    centres do not.  Up to 64 sites per entry, a centre one and a coordination number two.  A bias without any of them runs
    the path it ran before, bit for bit.  ``run()`` reads the status of the site tables with its other periodic checks.

    ``attach(observer)`` has ``step()`` sample an observer of md_observe.py whenever ``steps_done % observer.every == 0``, on the
    state the step leaves behind (after the kick, a deposit and, in ``ReplicaExchangeDynamics``, the attempt) and without a host
    read; ``run()`` reads the observers' status words with its other periodic checks.  Without observers ``step()`` launches and
    allocates what it did before them.

    Attributes: ``coordinates`` (fp32, updated in place; ``coordinates_lo`` is the residual of the two-float position),
    ``velocities`` (Angstrom / fs), ``forces`` and ``potential_energies`` at the coordinates, ``steps_done``.  ``step()`` never
    synchronizes with the host; ``run()`` reads the neighbor overflow status every ``check_every`` steps.
    """

    def __init__(self, model, species: Tensor, coordinates: Tensor, cell: tp.Optional[Tensor] = None, pbc=None, *,
                 dt: float = 0.5, masses: tp.Optional[Tensor] = None, temperature=None, friction=0.002,
                 fixed: tp.Optional[Tensor] = None, replica_ids: tp.Optional[Tensor] = None, seed: int = 0,
                 remove_drift: bool = True, constraints: tp.Optional[BondConstraints] = None,
                 constraint_tolerance: float = 1e-8, constraint_max_iterations: int = 64, pressure=None,
                 compressibility: float = 4.57e-5, barostat_time: float = 1000.0, barostat_scaling: str = "atomic",
                 bias=None) -> None:
        from .geomopt import ModelEvaluator
        from .utils import pbc_tuple

        if species.dim() != 2 or tuple(coordinates.shape) != (species.shape[0], species.shape[1], 3):
            raise ValueError("expected species [C, A] and coordinates [C, A, 3]")
        Cn, A = species.shape
        if not dt > 0:
            raise ValueError(f"dt must be > 0, got {dt}")
        friction = _per_molecule(friction, "friction", Cn)
        if temperature is not None:
            temperature = _per_molecule(temperature, "temperature", Cn)
        if masses is not None and tuple(masses.shape) != (Cn, A):
            raise ValueError(f"masses must have shape {(Cn, A)}, got {tuple(masses.shape)}")
        if fixed is not None and tuple(fixed.shape) != (Cn, A):
            raise ValueError(f"fixed must be a bool mask of shape {(Cn, A)}, got {tuple(fixed.shape)}")
        if replica_ids is not None and tuple(replica_ids.shape) != (Cn,):
            raise ValueError(f"replica_ids must have shape ({Cn},), got {tuple(replica_ids.shape)}")
        if replica_ids is not None and not bool(((replica_ids >= 0) & (replica_ids < 1 << 32)).all()):
            raise ValueError("replica_ids must be integers in 0 .. 2^32 - 1 (one Philox counter word)")
        if isinstance(seed, bool) or int(seed) != seed or not 0 <= seed < 1 << 64:
            raise ValueError(f"seed must be an integer in 0 .. 2^64 - 1, got {seed}")
        if constraints is not None and tuple(constraints.pairs.shape[:1]) != (Cn,):
            raise ValueError(f"constraints must hold pairs of shape ({Cn}, K, 2), got {tuple(constraints.pairs.shape)}")
        if not constraint_tolerance > 0 or constraint_max_iterations < 1:
            raise ValueError("constraint_tolerance must be > 0 and constraint_max_iterations >= 1")
        if barostat_scaling not in ("atomic", "molecular"):
            raise ValueError(f'barostat_scaling must be "atomic" or "molecular", got {barostat_scaling!r}')
        if barostat_scaling == "molecular" and pressure is None:
            raise ValueError('barostat_scaling="molecular" is a mode of the barostat: pass pressure=')
        self.barostat = pressure is not None
        self.molecular = barostat_scaling == "molecular"
        if self.barostat:
            if temperature is None:
                raise ValueError("the barostat needs Langevin dynamics (its noise is scaled by kT): pass temperature, not NVE")
            if Cn != 1:
                raise ValueError(f"the barostat handles one system (C = 1: the engine takes one cell per batch), got C = {Cn}")
            if cell is None or pbc is None or not all(pbc_tuple(pbc)):
                raise ValueError("the barostat needs a cell that is periodic in all three directions")
            if fixed is not None and bool(fixed.any()):
                raise ValueError("the barostat cannot rescale a system with fixed atoms")
            if not self.molecular and constraints is not None and bool((constraints.pairs >= 0).any()):
                raise ValueError("the barostat with atomic scaling does not support constraints (x <- mu x would rescale every "
                                 'bond): pass barostat_scaling="molecular", which moves every constraint cluster as a rigid body')
            if not compressibility > 0 or not barostat_time > 0:
                raise ValueError("compressibility and barostat_time must be > 0")
            pressure = torch.as_tensor(pressure, dtype=torch.float64)
            if pressure.dim() == 0:
                pressure = pressure.expand(Cn)
            if tuple(pressure.shape) != (Cn,):
                raise ValueError(f"pressure must be a number or a tensor of shape ({Cn},), got {tuple(pressure.shape)}")
        bias_tables = site_tables = None
        if bias is not None:
            if pressure is not None:
                raise ValueError("pressure= with bias= is not supported: the bias has no virial here")
            # (masses only where a mass-weighted centre asks for them: the masses given, not the 1 that fixed atoms get below)
            site_tables, bias_tables = build_site_tables(
                species, fixed, bias, temperature, cell=cell, pbc=pbc_tuple(pbc),
                masses=lambda: masses if masses is not None else default_masses(model, species))
            self._check_bias(bias_tables)
        if not (species.is_cuda and coordinates.is_cuda):
            raise ValueError("BatchedDynamics needs tensors on a ROCm device (no CPU fallback)")
        dev = coordinates.device
        if self.barostat:
            self.cell64 = cell.detach().to(device=dev, dtype=torch.float64).clone().contiguous()
            cell = self.cell64.to(torch.float32).contiguous()   # (owned: anihip_md_barostat rewrites it, the engine reads it)
            self.pressure = pressure.to(dev).contiguous()
            self._p0 = torch.empty_like(self.pressure)        # Hartree / Angstrom^3
            self._beta_T = float(compressibility) * BAR_PER_HARTREE_ANGSTROM3   # Angstrom^3 / Hartree
            self._tau_p = float(barostat_time)
            self.barostat_scale = torch.ones(Cn, dtype=torch.float64, device=dev)   # mu of the last move
        self._model_eval = ModelEvaluator(model, species, cell, pbc, stress=self.barostat)
        self.model, self.species, self.cell, self.pbc = model, species, cell, self._model_eval.pbc
        self.dt, self.seed, self.remove_drift = float(dt), int(seed), bool(remove_drift)
        self.coordinates = coordinates.detach().to(torch.float32).clone().contiguous()
        self.coordinates_lo = torch.zeros_like(self.coordinates)
        self.velocities = torch.zeros_like(self.coordinates)
        if masses is None:
            masses = default_masses(model, species)
        active = species >= 0
        if fixed is not None:
            active = active & ~fixed.to(device=dev, dtype=torch.bool)
        self._active = active.to(torch.uint8).contiguous()
        # (inactive atoms get mass 1: their inverse stays finite, and the kernels never read it)
        self.masses = torch.where(active, masses.to(device=dev, dtype=torch.float32), torch.ones((), device=dev)).contiguous()
        if not bool((self.masses > 0).all()):
            raise ValueError("masses must be > 0")
        self._inv_mass = (ACC_UNIT / self.masses.double()).float().contiguous()
        self.langevin = temperature is not None
        self.temperature = (temperature if self.langevin else torch.zeros(Cn)).to(dev).contiguous()
        self.friction = friction.to(dev).contiguous()
        self._kT = torch.empty_like(self.temperature)
        self._replica_ids = None if replica_ids is None else replica_ids.to(device=dev, dtype=torch.int64).contiguous()
        n_active = active.sum(dim=1)
        self._dof = (3 * n_active).clamp(min=1).double()
        # Three less once the centre-of-mass velocity has been removed, where it then stays removed: the total momentum is
        # conserved only in NVE and in a molecule without fixed atoms
        free = (species >= 0).sum(dim=1) == n_active
        self._dof_at_rest = (3 * n_active - 3 * (free if not self.langevin else torch.zeros_like(free))).clamp(min=1).double()
        self._drift_removed = False
        self._params = _lib.MdParams(Cn, A, _lib.MD_LANGEVIN if self.langevin else 0, 0, self.dt, self.seed, 0)
        self._workspace = torch.empty(_lib.lib().anihip_md_workspace_bytes(Cn, A), dtype=torch.uint8, device=dev)
        self._kinetic = torch.zeros(Cn, dtype=torch.float64, device=dev)
        self._kinetic_stale = False
        self._mb_draws = 0
        self.steps_done = 0
        self._observers: tp.List[Observer] = []
        self._clusters = None
        if constraints is not None and bool((constraints.pairs >= 0).any()):
            self._set_constraints(constraints, fixed, float(constraint_tolerance), int(constraint_max_iterations))
        # (a bias with no CV in any entry is no bias: nothing more is launched)
        self._bias = (DeviceBias(bias_tables, Cn, A, dev, site_tables)
                      if bias_tables is not None and bias_tables.kind.numel() else None)
        self.bias_energies = torch.zeros(Cn, dtype=torch.float64, device=dev) if self._bias is None else self._bias.bias_energies
        self._evaluate()
        if self.molecular:
            # the scaling groups are the constraint clusters (none: a table of no clusters) and the free atoms
            self._group_clusters = self._clusters if self._clusters is not None else _lib.MdClusters(
                0, None, None, None, None, None, None, 1.0, 1, 0, 0, 0)
            self._kinetic_mol = torch.zeros(Cn, dtype=torch.float64, device=dev)
            self._virial_mol = torch.zeros(Cn, dtype=torch.float64, device=dev)
            self._group_scratch = torch.empty(_lib.md_group_scratch_bytes(Cn, A), dtype=torch.uint8, device=dev)
            self._group_terms()

    def _set_constraints(self, constraints: BondConstraints, fixed: tp.Optional[Tensor], tolerance: float,
                         max_iterations: int) -> None:
        """Build the cluster tables, mark the atoms that clusters own, and put the coordinates on given lengths."""
        from .engine import _stream

        dev, (Cn, A) = self.coordinates.device, self.species.shape
        pairs = constraints.pairs.cpu()
        x = self.coordinates.double().cpu()
        at = torch.arange(Cn).view(-1, 1)
        dist = (x[at, pairs[..., 0].clamp(min=0)] - x[at, pairs[..., 1].clamp(min=0)]).norm(dim=-1)
        lengths = dist if constraints.lengths is None else constraints.lengths.cpu()
        cl = build_constraint_clusters(self.species, pairs, lengths, fixed, self._inv_mass)
        off = ((dist / lengths - 1.0).abs() > 0.1) & (pairs[..., 0] >= 0)
        if bool(off.any()):
            c, k = (int(t) for t in off.nonzero()[0])
            raise ValueError(f"molecule {c}: atoms {int(pairs[c, k, 0])} and {int(pairs[c, k, 1])} are {float(dist[c, k]):.3f} A "
                             f"apart, more than 10 % off their constrained length {float(lengths[c, k]):.3f} A (a molecule "
                             "wrapped across the cell, or a wrong index: the plain difference is taken, no minimum image)")
        self._active[cl.owned.to(dev)] = _lib.MD_ATOM_CLUSTER
        self.n_constraints = cl.per_molecule.to(dev)
        self._dof = (self._dof - self.n_constraints).clamp(min=1)
        self._dof_at_rest = (self._dof_at_rest - self.n_constraints).clamp(min=1)
        self._cluster_tables = tuple(t.to(dev).contiguous() for t in (cl.atoms, cl.count, cl.bonds, cl.d2, cl.w))
        self._cluster_host = cl
        self.constraint_iterations = torch.zeros((cl.atoms.shape[0], 2), dtype=torch.int32, device=dev)
        self._clusters = _lib.MdClusters(cl.atoms.shape[0], *(t.data_ptr() for t in self._cluster_tables),
                                         self.constraint_iterations.data_ptr(), tolerance, max_iterations,
                                         int(cl.count[:, 0].max()), int(cl.count[:, 1].max()), 0)
        if constraints.lengths is not None:
            # move(x, 0, .): SHAKE from rest along the bonds as they are; the velocity it leaves is discarded
            params = _lib.MdParams(Cn, A, 0, 0, 1.0, 0, 0)
            _lib.check(_lib.lib().anihip_md_constrain_drift(
                _stream(), C.byref(params), C.byref(self._clusters), None, None, None, self.coordinates.data_ptr(),
                self.coordinates_lo.data_ptr(), self.velocities.data_ptr(), torch.zeros_like(self.velocities).data_ptr()))
            self.velocities.zero_()
            self.raise_on_unconverged_constraints()

    def _project_velocities(self) -> None:
        from .engine import _stream

        if self._clusters is not None:
            _lib.check(_lib.lib().anihip_md_project_velocities(
                _stream(), C.byref(self._params), C.byref(self._clusters), self.coordinates.data_ptr(),
                self.coordinates_lo.data_ptr(), self.velocities.data_ptr()))

    def raise_on_unconverged_constraints(self) -> None:
        """Raise if a cluster used every iteration allowed in its last move or projection (one host synchronization)."""
        if self._clusters is None:
            return
        worst, q = self.constraint_iterations.max(dim=1).values.max(dim=0)
        if int(worst) >= self._clusters.max_iterations:
            cl, q = self._cluster_host, int(q)
            atoms = (cl.atoms[q, :int(cl.count[q, 0])] % self.species.shape[1]).tolist()
            it = self.constraint_iterations[q].tolist()
            raise RuntimeError(f"constraint cluster {q} (molecule {int(cl.molecule[q])}, atoms {atoms}) did not converge to "
                               f"{self._clusters.tolerance:g} in {self._clusters.max_iterations} iterations (positions {it[0]}, "
                               f"velocities {it[1]}): a smaller dt, or more iterations")

    def _check_bias(self, tables: BiasTables) -> None:
        """What a subclass refuses of a bias (host only, before anything is built)."""

    def _evaluate(self) -> None:
        """The model, then the bias on the forces held.  The evaluator hands out a tensor of its own at every call (the
        automatic HIP graph of small batches clones its static outputs, the eager path accumulates into a fresh buffer), so
        the bias is added in place: no engine buffer is read again after the step."""
        self.potential_energies, self.forces = self._model_eval(self.coordinates)
        if self._bias is not None:
            self._bias.apply(self.coordinates, self.coordinates_lo, self.forces)

    # ---- the three pieces of a step (anihip_md_drift, the model, anihip_md_kick) ---------------------------------
    def _drift(self) -> None:
        """First half kick and the position update (with the thermostat) on the forces held; advances the noise step."""
        from .engine import _stream

        if self.langevin:   # (every step: ``temperature`` is the user's to overwrite, by any means)
            torch.mul(self.temperature, KB_HARTREE, out=self._kT)
        self._params.step = self.steps_done
        rid = None if self._replica_ids is None else self._replica_ids.data_ptr()
        _lib.check(_lib.lib().anihip_md_drift(
            _stream(), C.byref(self._params), self._active.data_ptr(), self._inv_mass.data_ptr(), self._kT.data_ptr(),
            self.friction.data_ptr(), rid, self.coordinates.data_ptr(), self.coordinates_lo.data_ptr(),
            self.velocities.data_ptr(), self.forces.data_ptr()))
        if self._clusters is not None:
            _lib.check(_lib.lib().anihip_md_constrain_drift(
                _stream(), C.byref(self._params), C.byref(self._clusters), self._kT.data_ptr(), self.friction.data_ptr(), rid,
                self.coordinates.data_ptr(), self.coordinates_lo.data_ptr(), self.velocities.data_ptr(),
                self.forces.data_ptr()))
        self.steps_done += 1

    def _kick(self) -> None:
        """Second half kick on the forces held, and the kinetic energies."""
        from .engine import _stream

        if self._clusters is not None:   # (first: anihip_md_kick sums the kinetic energy of the projected velocities)
            _lib.check(_lib.lib().anihip_md_constrain_kick(
                _stream(), C.byref(self._params), C.byref(self._clusters), self.coordinates.data_ptr(),
                self.coordinates_lo.data_ptr(), self.velocities.data_ptr(), self.forces.data_ptr()))
        _lib.check(_lib.lib().anihip_md_kick(
            _stream(), C.byref(self._params), self._active.data_ptr(), self.masses.data_ptr(), self.velocities.data_ptr(),
            self.forces.data_ptr(), self._kinetic.data_ptr(), self._workspace.data_ptr(), self._workspace.numel()))
        self._kinetic_stale = False
        if self.molecular:
            self._group_terms()

    def _group_terms(self) -> None:
        """The centre-of-mass kinetic energy and the internal virial of the scaling groups (anihip_md_group_terms) from the
        coordinates, velocities and forces held, which must belong together: after a kick, or after velocities were set."""
        from .engine import _stream

        _lib.check(_lib.lib().anihip_md_group_terms(
            _stream(), C.byref(self._params), C.byref(self._group_clusters), self._active.data_ptr(), self.masses.data_ptr(),
            self.coordinates.data_ptr(), self.coordinates_lo.data_ptr(), self.velocities.data_ptr(), self.forces.data_ptr(),
            self._group_scratch.data_ptr(), self._kinetic_mol.data_ptr(), self._virial_mol.data_ptr()))

    def _barostat(self) -> None:
        """The volume move (anihip_md_barostat, or anihip_md_barostat_groups under molecular scaling) on the virial and the
        kinetic energy held (``step()`` refreshes a stale one before the drift), with the noise step of the drift before it:
        rescales cell64, cell, coordinates and velocities."""
        from .engine import _stream

        torch.div(self.pressure, BAR_PER_HARTREE_ANGSTROM3, out=self._p0)   # (every step: ``pressure`` is the user's to overwrite)
        rid = None if self._replica_ids is None else self._replica_ids.data_ptr()
        args = (_stream(), C.byref(self._params), self._beta_T, self._tau_p, self._active.data_ptr(), self._kT.data_ptr(),
                self._p0.data_ptr(), rid, self._model_eval.virial.data_ptr(), self._kinetic.data_ptr(), self.cell64.data_ptr(),
                self.cell.data_ptr(), self.coordinates.data_ptr(), self.coordinates_lo.data_ptr(), self.velocities.data_ptr(),
                self.barostat_scale.data_ptr())
        if self.molecular:   # (the group terms held are those of the last kick, or of the refresh in front of the drift)
            _lib.check(_lib.lib().anihip_md_barostat_groups(
                *args, C.byref(self._group_clusters), self.masses.data_ptr(), self._kinetic_mol.data_ptr(),
                self._virial_mol.data_ptr()))
        else:
            _lib.check(_lib.lib().anihip_md_barostat(*args))

    def attach(self, observer: Observer) -> Observer:
        """Have ``step()`` sample ``observer`` (``TimeSeries``, ``Trajectory``, ``RadialDistribution``,
        ``MeanSquaredDisplacement``, ``VelocityAutocorrelation``, ``HeatFlux``, ``HeatFluxAutocorrelation``) whenever ``steps_done % observer.every == 0``; returns it."""
        if not isinstance(observer, Observer):
            raise ValueError(f"attach() takes an observer of torchani_amd.md, got {type(observer).__name__}")
        observer._attach(self)
        self._observers.append(observer)
        return observer

    def step(self) -> None:
        """One time step (``_advance``), then the samples of the observers that are due.  No host synchronization."""
        self._advance()
        for observer in self._observers:
            if self.steps_done % observer.every == 0:
                observer._sample(self)

    def _advance(self) -> None:
        """Drift, the barostat's move if there is one, energies and forces at the new coordinates, kick, deposit."""
        if self.barostat and self._kinetic_stale:
            # velocities set since the last kick: the barostat takes the kinetic energy of before the drift, the same sum as
            # kinetic_energies() on the device, no host read
            self._kinetic.copy_(self.kinetic_energies())
            self._kinetic_stale = False
            if self.molecular:   # (the forces held are those of the coordinates held)
                self._group_terms()
        self._drift()
        if self.barostat:
            self._barostat()
        self._evaluate()
        self._kick()
        if self._bias is not None and self._bias.n_lists and self._bias.pace and self.steps_done % self._bias.pace == 0:
            # (kT as the drift of this step made it: KB_HARTREE temperature in fp32)
            self._bias.deposit(self._kT if self.langevin else None)

    def raise_on_overflow(self) -> None:
        """Raise if a neighbor row of the last evaluation overflowed (one host synchronization)."""
        self._model_eval.raise_on_overflow()

    def run(self, n_steps: int, check_every: int = 10) -> None:
        """``n_steps`` steps; the host reads the neighbor overflow status and the constraints' iteration counts every
        ``check_every`` steps and after the last."""
        if n_steps < 0 or check_every < 1:
            raise ValueError("n_steps must be >= 0 and check_every >= 1")
        for k in range(n_steps):
            self.step()
            if (k + 1) % check_every == 0 or k + 1 == n_steps:
                self.raise_on_overflow()
                self.raise_on_unconverged_constraints()
                if self._bias is not None:
                    self._bias.raise_on_bad_sites()
                for observer in self._observers:
                    observer.raise_on_status()

    # ---- velocities ------------------------------------------------------------------------------------------------
    def noise(self, step: int) -> Tensor:
        """The normal variates [C, A, 3] of noise step ``step`` (anihip_md_noise): what the drift of that step draws."""
        from .engine import _stream

        Cn, A = self.species.shape
        out = torch.empty((Cn, A, 3), dtype=torch.float32, device=self.coordinates.device)
        rid = None if self._replica_ids is None else self._replica_ids.data_ptr()
        _lib.check(_lib.lib().anihip_md_noise(_stream(), self.seed, step, Cn, A, rid, out.data_ptr()))
        return out

    def remove_center_of_mass_velocity(self) -> None:
        """Subtract each molecule's centre-of-mass velocity over its active atoms (anihip_md_remove_drift)."""
        from .engine import _stream

        _lib.check(_lib.lib().anihip_md_remove_drift(
            _stream(), C.byref(self._params), self._active.data_ptr(), self.masses.data_ptr(), self.velocities.data_ptr(),
            self._workspace.data_ptr(), self._workspace.numel()))
        self._project_velocities()
        self._kinetic_stale = True
        self._drift_removed = True

    def set_velocities(self, velocities: Tensor) -> None:
        """Copy ``velocities`` [C, A, 3] (Angstrom / fs) in; padding and fixed atoms keep zero.  They are taken to carry a
        centre-of-mass velocity (``temperatures()`` counts every degree of freedom) until
        ``remove_center_of_mass_velocity()`` is called."""
        self.velocities.copy_(velocities.to(self.velocities) * (self._active != 0).unsqueeze(-1))
        self._project_velocities()
        self._kinetic_stale = True
        self._drift_removed = False

    def set_temperature(self, kelvin) -> None:
        """Maxwell-Boltzmann velocities at ``kelvin`` (a number or a [C] tensor), drawn from the Philox stream of the
        dynamics at step words of their own (the top bit set, then a draw counter); then the drift is removed if
        ``remove_drift`` is on.  The thermostat's ``temperature`` is left alone."""
        kelvin = _per_molecule(kelvin, "temperature", self.species.shape[0]).to(self.coordinates.device)
        sigma = torch.sqrt((KB_HARTREE * kelvin).view(-1, 1) * self._inv_mass) * (self._active != 0)
        self.set_velocities(sigma.unsqueeze(-1) * self.noise(_MB_STEP | self._mb_draws))
        self._mb_draws += 1
        if self.remove_drift:
            self.remove_center_of_mass_velocity()

    # ---- observables (Hartree, K), no host read ------------------------------------------------------------------------
    def kinetic_energies(self) -> Tensor:
        """fp64 [C]: what the last kick computed, or a sum over the velocities if they were set since."""
        if self._kinetic_stale:
            v2 = self.velocities.double().pow(2).sum(dim=-1)
            return 0.5 * (self.masses.double() * (self._active != 0) * v2).sum(dim=1) / ACC_UNIT
        return self._kinetic.clone()

    def total_energies(self) -> Tensor:
        """Potential + bias + kinetic energies, fp64 [C]."""
        return self.potential_energies + self.bias_energies + self.kinetic_energies()

    # ---- observables of the bias, no host read -------------------------------------------------------------------------
    def _need_bias(self, lists: bool = False) -> DeviceBias:
        if self._bias is None or (lists and not self._bias.n_lists):
            raise ValueError("this dynamics has no " + ("Metadynamics" if lists else "bias"))
        return self._bias

    def collective_variables(self) -> Tensor:
        """fp64 [C, n_cv] at the coordinates of the last evaluation: one column per ``Restraint`` in the order given, then
        one per ``Metadynamics`` CV that no restraint holds; NaN where an entry does not have the CV."""
        b = self._need_bias()
        nan = torch.full((), float("nan"), dtype=torch.float64, device=b.cv_values.device)
        return torch.where(b.cv_index >= 0, b.cv_values[b.cv_index.clamp(min=0)], nan)

    def hills(self) -> tp.Tuple[Tensor, Tensor, Tensor]:
        """(centers fp64 [G, 2, max_hills], heights fp64 [G, max_hills], used int32 [G]): clones of the hill lists, what
        ``Metadynamics(hills=...)`` takes to go on from."""
        b = self._need_bias(lists=True)
        return b.centers.clone(), b.heights.clone(), b.used.clone()

    def metadynamics_bias(self, values: Tensor, list: int = 0) -> Tensor:   # noqa: A002
        """fp64 [n]: the bias V of list ``list`` at the CV values ``values`` [n] or [n, n_cv] (anihip_md_bias_hills)."""
        return self._need_bias(lists=True).hills_at(values, list)[0]

    def free_energies(self, values: Tensor, list: int = 0) -> Tensor:   # noqa: A002
        """fp64 [n], Hartree, up to a constant: -gamma / (gamma - 1) V for well-tempered metadynamics, -V for plain."""
        b = self._need_bias(lists=True)
        scale = -b.gamma / (b.gamma - 1.0) if b.gamma > 0 else -1.0
        return scale * b.hills_at(values, list)[0]

    def volumes(self) -> Tensor:
        """fp64 [1], Angstrom^3: |det| of the cell, of which a batch has one (the fp64 master under a barostat)."""
        if self.cell is None:
            raise ValueError("volumes() needs a cell")
        h = (self.cell64 if self.barostat else self.cell.to(device=self.coordinates.device, dtype=torch.float64)).reshape(9)
        det = h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6]) + h[2] * (h[3] * h[7] - h[4] * h[6])
        return det.abs().reshape(1)

    def pressures(self) -> Tensor:
        """fp64 [1], bar: (2 KE - tr W) / (3 V) from the current kinetic energy and the virial W of the last evaluation; with
        ``barostat_scaling="molecular"`` the molecular pressure (2 K_mol - (tr W + G)) / (3 V) of the scaling groups."""
        if not self.barostat:
            raise ValueError("pressures() needs the virial, which only a dynamics with pressure= evaluates")
        if self.molecular:
            if self._kinetic_stale:   # velocities set since the last kick
                self._group_terms()
            p = (2.0 * self._kinetic_mol - (self._model_eval.virial.diagonal().sum() + self._virial_mol)) / (3.0 * self.volumes())
            return p * BAR_PER_HARTREE_ANGSTROM3
        p = (2.0 * self.kinetic_energies() - self._model_eval.virial.diagonal().sum()) / (3.0 * self.volumes())
        return p * BAR_PER_HARTREE_ANGSTROM3

    def temperatures(self) -> Tensor:
        """2 KE / (dof k_B), dof = 3 (active atoms) less the molecule's constraints, less 3 where the centre-of-mass velocity has been removed
        (``set_temperature`` with ``remove_drift``, or ``remove_center_of_mass_velocity()``, since the velocities were last
        set) and the momentum is conserved (NVE, no fixed atom in the molecule)."""
        return 2.0 * self.kinetic_energies() / ((self._dof_at_rest if self._drift_removed else self._dof) * KB_HARTREE)


class RingPolymerDynamics(BatchedDynamics):
    """Path-integral MD (PIMD, TRPMD, RPMD) of R systems as ring polymers of ``beads`` = P copies each, integrated on the
    device: BAOAB with the free ring polymer propagated exactly in its normal modes and the path-integral Langevin thermostat
    (PILE) acting on those modes (anihip_md_rp_drift; include/anihip.h has the exact definition).

    species [R, A]; coordinates [R, A, 3] (all beads start on that point) or [R, P, A, 3] (a restart); species, masses and
    ``fixed`` are replicated over the beads.  The batch the base class integrates has C = R P entries, entry r P + j the bead
    j of polymer r, so one evaluation of the model gives the forces of all beads; with a cell, the P beads of the box share it.
    ``coordinates``, ``velocities``, ``forces`` and ``potential_energies`` are those of the batch, [R P, ...].

    temperature (required): the PHYSICAL temperature in K, a number or [R]; the beads are sampled at P T (the convention of
    Ceriotti et al. 2010).  It becomes the device tensor ``temperature`` [R P], the value repeated per bead, which may be
    overwritten between steps (the drift reads each polymer's first entry).  thermostat: "pile" (``friction`` in 1 / fs, a number
    or [R], damps the centroid, 0 leaves it alone; mode k > 0 gets 2 ``pile_lambda`` omega_k: 1 for PIMD, 0.5 for TRPMD), or None
    for RPMD, which conserves ``ring_polymer_energies()``.  replica_ids int64 [R]: polymer r draws the noise streams
    r P .. r P + P - 1, which must stay below 2^32; mode k of a polymer is driven by the stream of its entry r P + k.
    ``set_temperature(kelvin)`` draws the bead velocities at P kelvin.  remove_drift (default off) would remove the centre-of-
    mass velocity of every bead on its own.  Bond constraints, the barostat and ``bias=`` are not available with beads.

    ``step()``, ``run()``, the evaluator, the kick, the overflow check and the absence of host synchronization are the base
    class's.  ``kinetic_energies()`` and ``temperatures()`` keep their meaning per batch entry, that is per bead: they
    equilibrate at P T, not T.  The physical observables are ``quantum_kinetic_energies()``, ``centroids()``,
    ``spring_energies()`` and ``ring_polymer_energies()``, none of which reads on the host.
    """

    def __init__(self, model, species: Tensor, coordinates: Tensor, cell: tp.Optional[Tensor] = None, pbc=None, *,
                 beads: int, temperature=None, dt: float = 0.5, friction=0.002, pile_lambda: float = 1.0,
                 thermostat: tp.Optional[str] = "pile", masses: tp.Optional[Tensor] = None,
                 fixed: tp.Optional[Tensor] = None, replica_ids: tp.Optional[Tensor] = None, seed: int = 0,
                 remove_drift: bool = False, constraints=None, pressure=None, bias=None) -> None:
        if bias is not None:
            raise ValueError("RingPolymerDynamics does not support bias: a CV of a ring polymer (its centroid's, or every "
                             "bead's) is not implemented")
        if constraints is not None:
            raise ValueError("RingPolymerDynamics does not support constraints: bond constraints (SHAKE / RATTLE) with beads "
                             "are not implemented")
        if pressure is not None:
            raise ValueError("RingPolymerDynamics does not support pressure: the barostat with beads is not implemented")
        if isinstance(beads, bool) or int(beads) != beads or not 2 <= beads <= _lib.MD_RP_MAX_BEADS:
            raise ValueError(f"beads must be an integer in 2 .. {_lib.MD_RP_MAX_BEADS}, got {beads}")
        P = int(beads)
        if temperature is None:
            raise ValueError("RingPolymerDynamics needs temperature, the physical one: it sets the spring frequency "
                             "P k_B T / hbar with and without a thermostat")
        if thermostat not in ("pile", None):
            raise ValueError(f'thermostat must be "pile" or None, got {thermostat!r}')
        if not pile_lambda >= 0:
            raise ValueError(f"pile_lambda must be >= 0, got {pile_lambda}")
        if species.dim() != 2:
            raise ValueError("expected species [R, A]")
        R, A = species.shape
        if tuple(coordinates.shape) == (R, A, 3):
            coordinates = coordinates.unsqueeze(1).expand(R, P, A, 3)
        elif tuple(coordinates.shape) != (R, P, A, 3):
            raise ValueError(f"coordinates must have shape {(R, A, 3)} (all beads on one point) or {(R, P, A, 3)} (a restart), "
                             f"got {tuple(coordinates.shape)}")
        temperature = _per_molecule(temperature, "temperature", R)
        friction = _per_molecule(friction, "friction", R)
        if not bool((temperature > 0).all()):
            raise ValueError("temperature must be > 0")
        for t, name in ((masses, "masses"), (fixed, "fixed")):
            if t is not None and tuple(t.shape) != (R, A):
                raise ValueError(f"{name} must have shape {(R, A)}, got {tuple(t.shape)}")
        if replica_ids is None:
            replica_ids = torch.arange(R, dtype=torch.int64)
        if tuple(replica_ids.shape) != (R,):
            raise ValueError(f"replica_ids must have shape ({R},), got {tuple(replica_ids.shape)}")
        replica_ids = replica_ids.detach().cpu().to(torch.int64)
        if not bool(((replica_ids >= 0) & (replica_ids * P + (P - 1) < 1 << 32)).all()):
            raise ValueError(f"replica_ids r map to the noise streams r * beads + k, which must stay in 0 .. 2^32 - 1: with "
                             f"beads = {P} they must be in 0 .. {((1 << 32) - P) // P}")
        per_bead = lambda t: None if t is None else t.repeat_interleave(P, dim=0)   # noqa: E731
        super().__init__(model, per_bead(species), coordinates.reshape(R * P, A, 3), cell, pbc, dt=dt, masses=per_bead(masses),
                         temperature=per_bead(temperature), friction=per_bead(friction), fixed=per_bead(fixed),
                         replica_ids=(replica_ids.view(R, 1) * P + torch.arange(P)).reshape(-1), seed=seed,
                         remove_drift=remove_drift)
        self.beads, self.n_polymers, self.pile_lambda, self.thermostat = P, R, float(pile_lambda), thermostat
        # (the base class took temperature for Langevin dynamics: no degree of freedom is removed, which is right for RPMD
        # too, where the springs exchange momentum between the beads)
        self.langevin = thermostat == "pile"
        self._params.flags = _lib.MD_LANGEVIN if self.langevin else 0
        dev = self.coordinates.device
        self._n_active = (self._active.view(R, P, A)[:, 0] != 0).sum(dim=1).double()
        self._estimators = torch.zeros((R, 2), dtype=torch.float64, device=dev)
        self._centroids = torch.zeros((R, A, 3), dtype=torch.float64, device=dev)

    def _drift(self) -> None:
        """B, the exact free ring-polymer propagation with the PILE thermostat in the middle (anihip_md_rp_drift) on the
        forces held; advances the noise step."""
        from .engine import _stream

        torch.mul(self.temperature, KB_HARTREE, out=self._kT)   # (every step: ``temperature`` is the user's to overwrite)
        self._params.step = self.steps_done
        _lib.check(_lib.lib().anihip_md_rp_drift(
            _stream(), C.byref(self._params), self.beads, self.pile_lambda, self._active.data_ptr(), self._inv_mass.data_ptr(),
            self._kT.data_ptr(), self.friction.data_ptr(), self._replica_ids.data_ptr(), self.coordinates.data_ptr(),
            self.coordinates_lo.data_ptr(), self.velocities.data_ptr(), self.forces.data_ptr()))
        self.steps_done += 1

    def set_temperature(self, kelvin) -> None:
        """Maxwell-Boltzmann bead velocities for the physical temperature ``kelvin`` (a number or [R]): drawn at P kelvin, as
        the base class draws them.  The thermostat's ``temperature`` is left alone."""
        kelvin = _per_molecule(kelvin, "temperature", self.n_polymers)
        super().set_temperature((self.beads * kelvin).repeat_interleave(self.beads))

    # ---- observables of the polymers (Hartree, Angstrom), no host read ------------------------------------------------
    def _estimate(self) -> Tensor:
        """anihip_md_rp_estimators on the coordinates and forces held: (S_r, W_r) [R, 2], and the centroids."""
        from .engine import _stream

        torch.mul(self.temperature, KB_HARTREE, out=self._kT)
        _lib.check(_lib.lib().anihip_md_rp_estimators(
            _stream(), C.byref(self._params), self.beads, self._active.data_ptr(), self.masses.data_ptr(), self._kT.data_ptr(),
            self.coordinates.data_ptr(), self.coordinates_lo.data_ptr(), self.forces.data_ptr(), self._estimators.data_ptr(),
            self._centroids.data_ptr(), self._workspace.data_ptr(), self._workspace.numel()))
        return self._estimators

    def centroids(self) -> Tensor:
        """fp64 [R, A, 3]: the mean of each atom's beads."""
        self._estimate()
        return self._centroids.clone()

    def spring_energies(self) -> Tensor:
        """fp64 [R], Hartree: sum_j sum_i 1/2 m_i omega_P^2 |q_ij - q_i,j+1|^2 with omega_P = P k_B T / hbar."""
        return self._estimate()[:, 0].clone()

    def quantum_kinetic_energies(self, estimator: str = "centroid_virial") -> Tensor:
        """fp64 [R], Hartree: the instantaneous value of the quantum kinetic energy estimator, to be averaged along the run.
        "centroid_virial": 3 N kT / 2 - W / (2 P), W = sum_j sum_i (q_ij - centroid_i) . f_ij; "primitive": 3 N P kT / 2 - S / P,
        S the spring energy.  N is the number of active atoms and T the physical temperature."""
        if estimator not in ("centroid_virial", "primitive"):
            raise ValueError(f'estimator must be "centroid_virial" or "primitive", got {estimator!r}')
        est, P = self._estimate(), self.beads
        kT = KB_HARTREE * self.temperature.view(self.n_polymers, P)[:, 0].double()
        if estimator == "centroid_virial":
            return 1.5 * self._n_active * kT - est[:, 1] / (2.0 * P)
        return 1.5 * self._n_active * P * kT - est[:, 0] / P

    def ring_polymer_energies(self) -> Tensor:
        """fp64 [R], Hartree: sum_j (KE_j + V_j) + S, what ``thermostat=None`` conserves."""
        beads = (self.kinetic_energies() + self.potential_energies).view(self.n_polymers, self.beads).sum(dim=1)
        return beads + self.spring_energies()


def temperature_ladder(t_min: float, t_max: float, n: int) -> Tensor:
    """fp64 [n]: a geometric ladder t_min (t_max / t_min)^(k / (n - 1)), the spacing of equal acceptance for a constant heat
    capacity."""
    if isinstance(n, bool) or int(n) != n or n < 2:
        raise ValueError(f"a ladder needs n >= 2 rungs, got {n}")
    if not 0 < t_min < t_max:
        raise ValueError(f"expected 0 < t_min < t_max, got {t_min} and {t_max}")
    k = torch.arange(int(n), dtype=torch.float64) / (int(n) - 1)
    return float(t_min) * (float(t_max) / float(t_min)) ** k


class LadderTables(tp.NamedTuple):
    """The tables of anihip_md_exchange (include/anihip.h) on the host."""
    slot: Tensor          # int32 [L, K]: the batch entry at each rung, -1 past the end of a shorter ladder
    count: Tensor         # int32 [L]: rungs of each ladder
    rung_of: Tensor       # int32 [C]: -1 for an entry in no ladder
    ladder_of: Tensor     # int32 [C]: 0 for an entry in no ladder (never read for it)
    rung_temperatures: Tensor   # fp32 [L, K], K; 0 past the end of a shorter ladder
    direction: Tensor     # int8 [C]: +1 at rung 0, -1 at the top rung, 0 between


def build_ladders(ladders: tp.Optional[Tensor], temperature: Tensor, species: tp.Optional[Tensor] = None,
                  fixed: tp.Optional[Tensor] = None) -> LadderTables:
    """The ladder tables of ``ReplicaExchangeDynamics`` from ``ladders`` (None: one ladder of all C entries in batch order, or
    int64 [L, K] of batch indices, -1 padding the tail of a shorter ladder) and the initial ``temperature`` [C] in K.  Rung
    order is column order.  Raises ValueError for a ladder of fewer than two rungs, an index outside the batch, padding that
    is not a tail, an entry in two ladders, temperatures that are not strictly increasing along a ladder, and ``species``
    [C, A] or ``fixed`` [C, A] that differ within a ladder.  Host tensors; reads no device."""
    temperature = temperature.detach().cpu().to(torch.float32)
    Cn = temperature.shape[0]
    if ladders is None:
        ladders = torch.arange(Cn, dtype=torch.int64).view(1, Cn)
    ladders = torch.as_tensor(ladders).detach().cpu()
    if ladders.dim() != 2 or ladders.dtype not in (torch.int64, torch.int32):
        raise ValueError("ladders must be an integer tensor [L, K] of batch indices (-1 padding)")
    ladders = ladders.to(torch.int64)
    L, K = ladders.shape
    if L < 1 or K < 2:
        raise ValueError(f"ladders must hold at least one ladder of at least 2 rungs, got shape {(L, K)}")
    if bool(((ladders < -1) | (ladders >= Cn)).any()):
        raise ValueError(f"ladders must hold batch indices in 0 .. {Cn - 1}, or -1 as padding")
    used = ladders >= 0
    count = used.sum(dim=1)
    if bool((used != (torch.arange(K).view(1, K) < count.view(L, 1))).any()):
        raise ValueError("the -1 padding of a ladder must be its tail: rung order is column order, without gaps")
    if bool((count < 2).any()):
        raise ValueError(f"ladder {int((count < 2).nonzero()[0])} has fewer than 2 rungs")
    members = ladders[used]
    if members.unique().numel() != members.numel():
        seen = torch.bincount(members, minlength=Cn)
        raise ValueError(f"batch entry {int((seen > 1).nonzero()[0])} is in two ladders (or twice in one)")
    rung_t = torch.where(used, temperature[ladders.clamp(min=0)], torch.zeros(()))
    if bool((rung_t[used] <= 0).any()):
        raise ValueError("the temperatures of a ladder must be > 0")
    falling = used[:, 1:] & ~(rung_t[:, 1:] > rung_t[:, :-1])
    if bool(falling.any()):
        l, k = (int(t) for t in falling.nonzero()[0])
        raise ValueError(f"the initial temperatures must be strictly increasing along each ladder: ladder {l} has "
                         f"{float(rung_t[l, k]):g} K at rung {k} and {float(rung_t[l, k + 1]):g} K at rung {k + 1}")
    first = ladders[:, :1].expand(L, K)[used]
    for t, name in ((species, "species"), (fixed, "fixed")):
        if t is not None:
            t = t.detach().cpu()
            if bool((t[members] != t[first]).any()):
                raise ValueError(f"{name} differ within a ladder: the rungs of a ladder are replicas of one system")
    rung_of = torch.full((Cn,), -1, dtype=torch.int32)
    ladder_of = torch.zeros(Cn, dtype=torch.int32)
    rung_of[members] = torch.arange(K, dtype=torch.int32).view(1, K).expand(L, K)[used]
    ladder_of[members] = torch.arange(L, dtype=torch.int32).view(L, 1).expand(L, K)[used]
    direction = torch.zeros(Cn, dtype=torch.int8)
    direction[ladders[:, 0]] = 1
    direction[ladders[torch.arange(L), count - 1]] = -1
    return LadderTables(ladders.to(torch.int32), count.to(torch.int32), rung_of, ladder_of, rung_t, direction)


class ReplicaExchangeDynamics(BatchedDynamics):
    """Temperature replica exchange (parallel tempering) on the device: the batch holds L ladders of replicas of one system
    each, every replica a Langevin trajectory of ``BatchedDynamics`` at the temperature of its rung, and every
    ``exchange_every`` steps neighboring rungs of every ladder try to swap their TEMPERATURES by the Metropolis rule on the
    potential energies held (anihip_md_exchange; include/anihip.h has the exact definition).  Coordinates, forces, neighbor
    state and noise streams stay with the batch entry; an accepted swap rescales the two entries' velocities by
    sqrt(T_new / T_old), so nothing is evaluated again and no step reads on the host.

    species [C, A], coordinates, cell, pbc and every keyword of ``BatchedDynamics`` keep their meaning.  temperature
    (required): a [C] tensor in K, the initial temperature of every entry.  ladders: None for one ladder of all C entries in
    batch order, or int64 [L, K] of batch indices, rung order being column order and -1 padding the tail of a shorter ladder;
    the initial temperatures must increase strictly along a ladder, no entry may be in two, and the entries of a ladder must
    have the same species and ``fixed`` mask.  Entries in no ladder are plain Langevin trajectories.  ladder_ids: int64 [L]
    in 0 .. 2^32 - 1, the stream of each ladder's decisions (default: its index) -- with ``replica_ids`` a ladder follows the
    same trajectory wherever it sits in the batch.  NVE (no temperature) is refused, and so is ``pressure=``: the barostat
    handles one system (C = 1) and a ladder has at least two entries.

    ``step()`` is the inherited step and then, when ``steps_done`` is a multiple of ``exchange_every``, one attempt with the
    attempt number ``attempts_done``: even attempts pair the rungs (0, 1), (2, 3), ..., odd ones (1, 2), (3, 4), ....  After
    an attempt ``temperature`` of every ladder member is rewritten from ``rung_temperatures`` (fp32 [L, K], K, a device tensor
    that may be overwritten between steps and is converted to kT at every attempt) through the rung of the entry.
    ``exchange_every=0`` never exchanges and is bit-identical to ``BatchedDynamics``.  Friction stays with the entry.
    Constraints are allowed: a uniform velocity scale keeps the RATTLE condition, so no projection follows.  ``bias=`` may
    hold restraints (umbrella windows in every rung): the Metropolis rule then takes ``potential_energies + bias_energies``,
    summed on the device.  ``Metadynamics`` is refused: its bias would have to follow the rung, not the entry.

    Observables, device tensors read without host synchronization: ``rungs()`` int32 [C] (-1: in no ladder),
    ``replicas_at_rungs()`` int32 [L, K] (-1 padding), ``exchange_attempts`` and ``exchange_accepts`` int64 [L, K - 1] per pair
    (k, k + 1), ``acceptance_rates()``, ``round_trips()`` int32 [C] (rung 0 to the top rung and back) and ``by_rung(t)``,
    which gathers any [C, ...] tensor to [L, K, ...] (zeros in the padding).
    """

    def __init__(self, model, species: Tensor, coordinates: Tensor, cell: tp.Optional[Tensor] = None, pbc=None, *,
                 temperature=None, ladders: tp.Optional[Tensor] = None, exchange_every: int = 100,
                 ladder_ids: tp.Optional[Tensor] = None, pressure=None, **kw) -> None:
        if temperature is None:
            raise ValueError("ReplicaExchangeDynamics needs temperature, a [C] tensor: NVE has no temperatures to exchange")
        if pressure is not None:
            raise ValueError("ReplicaExchangeDynamics does not support pressure: the barostat handles one system (C = 1) and a "
                             "ladder has at least two entries")
        if isinstance(exchange_every, bool) or int(exchange_every) != exchange_every or exchange_every < 0:
            raise ValueError(f"exchange_every must be an integer >= 0, got {exchange_every}")
        if species.dim() != 2:
            raise ValueError("expected species [C, A]")
        Cn = species.shape[0]
        temperature = torch.as_tensor(temperature)
        if tuple(temperature.shape) != (Cn,):
            raise ValueError(f"temperature must be a tensor of shape ({Cn},), one per batch entry, got {tuple(temperature.shape)}")
        tables = build_ladders(ladders, temperature, species, kw.get("fixed"))
        L, K = tables.slot.shape
        if ladder_ids is not None:
            ladder_ids = torch.as_tensor(ladder_ids).detach().cpu().to(torch.int64)
            if tuple(ladder_ids.shape) != (L,) or not bool(((ladder_ids >= 0) & (ladder_ids < 1 << 32)).all()):
                raise ValueError(f"ladder_ids must be {L} integers in 0 .. 2^32 - 1 (one Philox counter word)")
        super().__init__(model, species, coordinates, cell, pbc, temperature=temperature, **kw)
        dev = self.coordinates.device
        self.exchange_every, self.attempts_done = int(exchange_every), 0
        self.n_ladders, self.max_rungs = L, K
        self._slot, self._count, self._rung_of, self._ladder_of, self.rung_temperatures, self._direction = (
            t.to(dev).contiguous() for t in tables)
        self._rung_kT = torch.empty_like(self.rung_temperatures)
        self._ladder_ids = None if ladder_ids is None else ladder_ids.to(dev).contiguous()
        self.exchange_attempts = torch.zeros((L, K - 1), dtype=torch.int64, device=dev)
        self.exchange_accepts = torch.zeros((L, K - 1), dtype=torch.int64, device=dev)
        self._round_trips = torch.zeros(Cn, dtype=torch.int32, device=dev)
        self._exchange_scale = torch.ones(Cn, dtype=torch.float64, device=dev)
        # the gather of ``temperature`` after an attempt: members [M], their ladders [M] (int64: index tensors, no host read)
        self._members = (self._rung_of >= 0).nonzero().view(-1)
        self._member_ladders = self._ladder_of[self._members].long()
        self._ladders = _lib.MdLadders(
            L, K, 0, 0, self._slot.data_ptr(), self._count.data_ptr(), self._rung_of.data_ptr(), self._rung_kT.data_ptr(),
            None if self._ladder_ids is None else self._ladder_ids.data_ptr(), self.exchange_attempts.data_ptr(),
            self.exchange_accepts.data_ptr(), self._direction.data_ptr(), self._round_trips.data_ptr(),
            self._exchange_scale.data_ptr())
        self._exchange_params = _lib.MdParams(Cn, species.shape[1], _lib.MD_LANGEVIN, 0, self.dt, self.seed, 0)
        self._exchange_energies = torch.empty(Cn, dtype=torch.float64, device=dev)

    def _check_bias(self, tables: BiasTables) -> None:
        if tables.members.numel():
            raise ValueError("ReplicaExchangeDynamics does not support Metadynamics: temperatures are swapped, so the bias "
                             "would have to follow the rung, not the batch entry; restraints are fine")

    def _exchange(self) -> None:
        """One attempt (anihip_md_exchange) on the potential and kinetic energies held, then ``temperature`` of the ladder
        members from ``rung_temperatures`` through their new rungs."""
        from .engine import _stream

        torch.mul(self.rung_temperatures, KB_HARTREE, out=self._rung_kT)   # (every attempt: the user's to overwrite)
        self._exchange_params.step = self.attempts_done
        energies = self.potential_energies
        if self._bias is not None:   # (the rungs differ in temperature alone: the restraints count as potential energy)
            energies = torch.add(self.potential_energies, self.bias_energies, out=self._exchange_energies)
        _lib.check(_lib.lib().anihip_md_exchange(
            _stream(), C.byref(self._exchange_params), C.byref(self._ladders), energies.data_ptr(),
            self._active.data_ptr(), self.velocities.data_ptr(), self._kinetic.data_ptr()))
        self.attempts_done += 1
        rung = self._rung_of[self._members].long()
        self.temperature.index_copy_(0, self._members, self.rung_temperatures[self._member_ladders, rung])

    def _advance(self) -> None:
        """The inherited step, then one exchange attempt when ``steps_done`` is a multiple of ``exchange_every``: observers
        sample what the attempt leaves behind.  No host synchronization."""
        super()._advance()
        if self.exchange_every and self.steps_done % self.exchange_every == 0:
            self._exchange()

    # ---- observables, no host read ------------------------------------------------------------------------------------
    def rungs(self) -> Tensor:
        """int32 [C]: the rung of each batch entry, -1 for an entry in no ladder."""
        return self._rung_of.clone()

    def replicas_at_rungs(self) -> Tensor:
        """int32 [L, K]: the batch entry at each rung, -1 past the end of a shorter ladder."""
        return self._slot.clone()

    def acceptance_rates(self) -> Tensor:
        """fp64 [L, K - 1]: accepts / attempts of each pair (k, k + 1); 0 where nothing was attempted."""
        return self.exchange_accepts.double() / self.exchange_attempts.clamp(min=1).double()

    def round_trips(self) -> Tensor:
        """int32 [C]: how often each entry has come back to rung 0 after reaching the top rung of its ladder."""
        return self._round_trips.clone()

    def by_rung(self, tensor: Tensor) -> Tensor:
        """Any [C, ...] tensor gathered to [L, K, ...] through the current occupancy; zeros in the padding."""
        if tensor.shape[:1] != self._rung_of.shape:
            raise ValueError(f"expected a tensor of shape [{self._rung_of.shape[0]}, ...], got {tuple(tensor.shape)}")
        out = tensor[self._slot.clamp(min=0).long()]
        used = (self._slot >= 0).view(self.n_ladders, self.max_rungs, *([1] * (tensor.dim() - 1)))
        return torch.where(used, out, torch.zeros((), dtype=out.dtype, device=out.device))
