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
"""
from __future__ import annotations

import ctypes as C
import math
import typing as tp

import torch
from torch import Tensor

from . import _lib

# CODATA 2018: 1 Ha = 4.3597447222071e-18 J, 1 amu = 1.66053906660e-27 kg  ->  (Ha / Angstrom) / amu in Angstrom / fs^2
ACC_UNIT = 4.3597447222071e-18 / 1e-10 / 1.66053906660e-27 * 1e10 * 1e-30
KB_HARTREE = 3.166811563e-6          # Boltzmann constant, Ha / K
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


class BatchedDynamics:
    """NVE (velocity Verlet) or Langevin (BAOAB) dynamics of every molecule of species [C, A], coordinates [C, A, 3]
    (Angstrom, kept unwrapped), integrated on the device (csrc/md.hip; include/anihip.h has the exact definition).

    dt in fs.  temperature: None (NVE), a number or a [C] tensor in K (Langevin; one thermostat per molecule); friction: a
    number or a [C] tensor in 1 / fs.  Both become the device tensors ``temperature`` and ``friction`` (fp32 [C]), which may
    be overwritten between steps (annealing, replica ladders).  fixed: bool [C, A] atoms that never move.  replica_ids: int64
    [C] in 0 .. 2^32 - 1, the noise stream of each molecule (default: its batch index) -- a replica draws the same noise wherever it sits in
    the batch.  remove_drift: ``set_temperature`` removes each molecule's centre-of-mass velocity.

    Attributes: ``coordinates`` (fp32, updated in place; ``coordinates_lo`` is the residual of the two-float position),
    ``velocities`` (Angstrom / fs), ``forces`` and ``potential_energies`` at the coordinates, ``steps_done``.  ``step()`` never
    synchronizes with the host; ``run()`` reads the neighbor overflow status every ``check_every`` steps.
    """

    def __init__(self, model, species: Tensor, coordinates: Tensor, cell: tp.Optional[Tensor] = None, pbc=None, *,
                 dt: float = 0.5, masses: tp.Optional[Tensor] = None, temperature=None, friction=0.002,
                 fixed: tp.Optional[Tensor] = None, replica_ids: tp.Optional[Tensor] = None, seed: int = 0,
                 remove_drift: bool = True) -> None:
        from .geomopt import ModelEvaluator

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
        if not (species.is_cuda and coordinates.is_cuda):
            raise ValueError("BatchedDynamics needs tensors on a ROCm device (no CPU fallback)")
        dev = coordinates.device
        self._model_eval = ModelEvaluator(model, species, cell, pbc)
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
        self._evaluate()

    def _evaluate(self) -> None:
        self.potential_energies, self.forces = self._model_eval(self.coordinates)

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
        self.steps_done += 1

    def _kick(self) -> None:
        """Second half kick on the forces held, and the kinetic energies."""
        from .engine import _stream

        _lib.check(_lib.lib().anihip_md_kick(
            _stream(), C.byref(self._params), self._active.data_ptr(), self.masses.data_ptr(), self.velocities.data_ptr(),
            self.forces.data_ptr(), self._kinetic.data_ptr(), self._workspace.data_ptr(), self._workspace.numel()))
        self._kinetic_stale = False

    def step(self) -> None:
        """One time step: drift, energies and forces at the new coordinates, kick.  No host synchronization."""
        self._drift()
        self._evaluate()
        self._kick()

    def raise_on_overflow(self) -> None:
        """Raise if a neighbor row of the last evaluation overflowed (one host synchronization)."""
        self._model_eval.raise_on_overflow()

    def run(self, n_steps: int, check_every: int = 10) -> None:
        """``n_steps`` steps; the host reads the neighbor overflow status every ``check_every`` steps and after the last."""
        if n_steps < 0 or check_every < 1:
            raise ValueError("n_steps must be >= 0 and check_every >= 1")
        for k in range(n_steps):
            self.step()
            if (k + 1) % check_every == 0 or k + 1 == n_steps:
                self.raise_on_overflow()

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
        self._kinetic_stale = True
        self._drift_removed = True

    def set_velocities(self, velocities: Tensor) -> None:
        """Copy ``velocities`` [C, A, 3] (Angstrom / fs) in; padding and fixed atoms keep zero.  They are taken to carry a
        centre-of-mass velocity (``temperatures()`` counts every degree of freedom) until
        ``remove_center_of_mass_velocity()`` is called."""
        self.velocities.copy_(velocities.to(self.velocities) * self._active.unsqueeze(-1))
        self._kinetic_stale = True
        self._drift_removed = False

    def set_temperature(self, kelvin) -> None:
        """Maxwell-Boltzmann velocities at ``kelvin`` (a number or a [C] tensor), drawn from the Philox stream of the
        dynamics at step words of their own (the top bit set, then a draw counter); then the drift is removed if
        ``remove_drift`` is on.  The thermostat's ``temperature`` is left alone."""
        kelvin = _per_molecule(kelvin, "temperature", self.species.shape[0]).to(self.coordinates.device)
        sigma = torch.sqrt((KB_HARTREE * kelvin).view(-1, 1) * self._inv_mass) * self._active
        self.set_velocities(sigma.unsqueeze(-1) * self.noise(_MB_STEP | self._mb_draws))
        self._mb_draws += 1
        if self.remove_drift:
            self.remove_center_of_mass_velocity()

    # ---- observables (Hartree, K), no host read ------------------------------------------------------------------------
    def kinetic_energies(self) -> Tensor:
        """fp64 [C]: what the last kick computed, or a sum over the velocities if they were set since."""
        if self._kinetic_stale:
            v2 = self.velocities.double().pow(2).sum(dim=-1)
            return 0.5 * (self.masses.double() * self._active * v2).sum(dim=1) / ACC_UNIT
        return self._kinetic.clone()

    def total_energies(self) -> Tensor:
        return self.potential_energies + self.kinetic_energies()

    def temperatures(self) -> Tensor:
        """2 KE / (dof k_B), dof = 3 (active atoms), less 3 where the centre-of-mass velocity has been removed
        (``set_temperature`` with ``remove_drift``, or ``remove_center_of_mass_velocity()``, since the velocities were last
        set) and the momentum is conserved (NVE, no fixed atom in the molecule)."""
        return 2.0 * self.kinetic_energies() / ((self._dof_at_rest if self._drift_removed else self._dof) * KB_HARTREE)
