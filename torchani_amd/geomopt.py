"""Batched L-BFGS geometry optimization on the HIP engine: ASE's ``LBFGS`` (no line search) applied to every molecule of a
batch independently, the optimizer step in libanihip (anihip_lbfgs_step, csrc/lbfgs.hip: four launches per step whatever
the history length, the batch size or the molecule size).

Per molecule c, at iteration k (energies in Hartree, lengths in Angstrom, defaults ASE's converted with ``units``):

1. f_k = the forces with padding atoms (species < 0) and ``fixed`` atoms zeroed (ASE's FixAtoms);
2. converged_c |= max_i |f_k,i| < fmax.  A converged molecule is frozen: it never moves again, its coordinates stay
   bit-identical;
3. k > 0: the pair s = x_k - x_k-1, y = f_k-1 - f_k is stored only if s.y > 0 (in fp64), the oldest pair dropped beyond
   ``memory``.  ASE stores every pair; one of non-positive curvature makes the inverse Hessian indefinite, and the step
   can then go uphill;
4. p = -H g, g = -f_k, H the L-BFGS inverse Hessian of the stored pairs with H0 = I / alpha;
5. if max_i |p_i| >= maxstep, p is scaled by maxstep / max_i |p_i|; x_k+1 = x_k + damping p and n_steps_c += 1.

Periodic systems are optimized in a fixed cell with unwrapped coordinates (as in md.py).  ``step()`` never synchronizes
with the host; ``run()`` reads the converged count and the neighbor overflow status every ``check_every`` steps.  The model
is an ``ANI`` model (``energies_and_forces`` with ``check_overflow=False`` and the same species tensor at every step, so small
systems replay the automatic HIP graph) or a standalone pair potential of ``torchani_amd.potentials``, evaluated through its
``accumulate`` on its own neighbor rows without autograd.
"""
from __future__ import annotations

import ctypes as C
import typing as tp

import torch
from torch import Tensor

from . import _lib
from .engine import _stream
from .tuples import OptimizedGeometries
from .units import HARTREE_TO_EV
from .utils import pbc_tuple

DEFAULT_ALPHA = 70.0 / HARTREE_TO_EV   # ASE LBFGS(alpha=70 eV / A^2), in Hartree / A^2
DEFAULT_FMAX = 0.05 / HARTREE_TO_EV    # ASE Optimizer.run(fmax=0.05 eV / A), in Hartree / A
MAX_MEMORY = _lib.LBFGS_MAX_MEMORY


def lbfgs_workspace_bytes(n_mol: int, atoms_per_mol: int, memory: int) -> int:
    """Bytes of the optimizer's device workspace: the layout of csrc/lbfgs.hip (lb_layout), computed on the host."""
    if n_mol < 1 or atoms_per_mol < 1 or not 1 <= memory <= MAX_MEMORY:
        raise ValueError(f"n_mol and atoms_per_mol must be >= 1 and memory in 1 .. {MAX_MEMORY}")
    Cn, A = int(n_mol), int(atoms_per_mol)
    n = 3 * A
    n_pad = -(-n // 64) * 64
    V = 1
    while V < 16 and V < n_pad // 64:
        V *= 2
    G = -(-n_pad // (64 * V))
    M1 = memory + 1
    NV = 4 * M1 + 1
    Gc = -(-A // 64)
    regions = [Cn * 4 * 4, Cn * 2 * M1 * 8, Cn * M1 * M1 * 8, Cn * M1 * M1 * 8, Cn * M1 * M1 * 8, Cn * M1 * 8,
               Cn * G * NV * 8, Cn * Gc * 8, Cn * n * 8, Cn * n_pad * 4, Cn * n_pad * 4, Cn * M1 * n_pad * 4,
               Cn * M1 * n_pad * 4]
    return sum(-(-r // 256) * 256 for r in regions)


def _check_run_args(fmax: float, steps: int, check_every: int) -> None:
    if not fmax >= 0:
        raise ValueError(f"fmax must be >= 0, got {fmax}")
    if steps < 0 or check_every < 1:
        raise ValueError("steps must be >= 0 and check_every >= 1")


class ModelEvaluator:
    """Energies [C] (fp64) and forces [C, A, 3] (fp32) of a model at fp32 coordinates that the caller updates in place, queued
    on the stream without a host synchronization (GeometryOptimizer, md.BatchedDynamics).  The model is an ``ANI`` model
    (``energies_and_forces`` with ``check_overflow=False`` and the same species tensor at every call, so small systems replay
    the automatic HIP graph) or a standalone pair potential, evaluated through its ``accumulate`` on its own neighbor rows.

    ``stress=True`` also keeps ``virial`` (fp64 [3, 3], Hartree: dE/d strain of all atoms together) of every evaluation, from
    ``energies_and_forces(stress=True)`` or the ``virial=`` argument of ``accumulate``.  An evaluation that carries the virial
    is not replayed from the automatic HIP graph."""

    def __init__(self, model, species: Tensor, cell: tp.Optional[Tensor], pbc, stress: bool = False) -> None:
        from .potentials import _Standalone

        self.model, self.species, self.cell = model, species, cell
        self.stress, self.virial = bool(stress), None
        # (a host tuple once: a pbc tensor would cost a synchronization at every evaluation)
        self.pbc = pbc_tuple(pbc)
        self.standalone = isinstance(model, _Standalone)
        if self.standalone:
            self._species32 = model._to_elem_idxs(species, True).to(torch.int32).contiguous()
            self._rows = None

    def __call__(self, coordinates: Tensor) -> tp.Tuple[Tensor, Tensor]:
        if self.standalone:
            Cn, A = self.species.shape
            rows = self.model._standalone_rows(self._species32, coordinates, self.cell, self.pbc)
            atomic = torch.zeros(Cn * A, dtype=torch.float32, device=coordinates.device)
            grad = torch.zeros((Cn * A, 3), dtype=torch.float32, device=coordinates.device)
            if self.stress:
                self.virial = torch.zeros((3, 3), dtype=torch.float64, device=coordinates.device)
            self.model.accumulate(self._species32, rows, atomic, grad, virial=self.virial)
            self._rows = rows
            return atomic.view(Cn, A).to(torch.float64).sum(dim=1), grad.neg_().view(Cn, A, 3)
        # (``stress`` is passed only when asked for: the default call is the one any model with this method takes)
        kw = {"stress": True} if self.stress else {}
        out = self.model.energies_and_forces(self.species, coordinates, self.cell, self.pbc, check_overflow=False, **kw)
        if self.stress:
            self.virial = out.virial
        return out.energies, out.forces.to(torch.float32).contiguous()

    def raise_on_overflow(self) -> None:
        """Raise if a neighbor row of the last evaluation overflowed (one host synchronization)."""
        if self.standalone:
            if self._rows is not None and self._rows.overflowed():
                raise RuntimeError(f"{type(self.model).__name__}: an atom has more than {_lib.MAX_RAD} neighbors inside the "
                                   f"cutoff ({self.model.cutoff} A): the forces would be wrong")
            return
        m = self.model
        if not m._overflow_impossible(self.species, self.cell, self.pbc):
            m.aev_computer.last_neighbors().raise_on_overflow()
        m._raise_on_pair_overflow()


class GeometryOptimizer:
    """L-BFGS minimization of the energy of every molecule of species [C, A], coordinates [C, A, 3] (Angstrom).

    memory: stored pairs (1 .. MAX_MEMORY), maxstep: the longest atom step (Angstrom), alpha: H0 = I / alpha (Hartree /
    Angstrom^2), damping: factor of every step, fixed: bool [C, A] atoms that never move.  Attributes: ``coordinates``
    (fp32, updated in place), ``energies`` [C] and ``forces`` [C, A, 3] at them, ``converged`` (bool [C]), ``n_steps``
    (int32 [C]) and ``last_step`` (fp32 [C, A, 3], the displacement the last step applied).
    """

    def __init__(self, model, species: Tensor, coordinates: Tensor, cell: tp.Optional[Tensor] = None, pbc=None, *,
                 memory: int = 100, maxstep: float = 0.2, alpha: float = DEFAULT_ALPHA, damping: float = 1.0,
                 fixed: tp.Optional[Tensor] = None) -> None:
        if species.dim() != 2 or tuple(coordinates.shape) != (species.shape[0], species.shape[1], 3):
            raise ValueError("expected species [C, A] and coordinates [C, A, 3]")
        if isinstance(memory, bool) or int(memory) != memory or not 1 <= memory <= MAX_MEMORY:
            raise ValueError(f"memory must be an integer in 1 .. {MAX_MEMORY}, got {memory}")
        if not maxstep > 0:
            raise ValueError(f"maxstep must be > 0, got {maxstep}")
        if not alpha > 0 or not damping > 0:
            raise ValueError("alpha and damping must be > 0")
        if fixed is not None and tuple(fixed.shape) != tuple(species.shape):
            raise ValueError(f"fixed must be a bool mask of shape {tuple(species.shape)}, got {tuple(fixed.shape)}")
        if not (species.is_cuda and coordinates.is_cuda):
            raise ValueError("GeometryOptimizer needs tensors on a ROCm device (no CPU fallback)")
        dev = coordinates.device
        Cn, A = species.shape
        self._model_eval = ModelEvaluator(model, species, cell, pbc)
        self.model, self.species, self.cell, self.pbc = model, species, cell, self._model_eval.pbc
        self._dtype = coordinates.dtype
        self.coordinates = coordinates.detach().to(torch.float32).clone().contiguous()
        active = species >= 0
        if fixed is not None:
            active = active & ~fixed.to(device=dev, dtype=torch.bool)
        self._active = active.to(torch.uint8).contiguous()
        self._params = _lib.LbfgsParams(Cn, A, int(memory), 0, 1.0 / float(alpha), float(maxstep), float(damping),
                                        DEFAULT_FMAX)
        self.fmax = DEFAULT_FMAX
        self._workspace = torch.zeros(lbfgs_workspace_bytes(Cn, A, int(memory)), dtype=torch.uint8, device=dev)
        self.converged = torch.zeros(Cn, dtype=torch.bool, device=dev)
        self.n_steps = torch.zeros(Cn, dtype=torch.int32, device=dev)
        self.last_step = torch.zeros_like(self.coordinates)
        self._evaluate()

    def _evaluate(self) -> None:
        """energies and forces at the current coordinates, queued on the stream."""
        self.energies, self.forces = self._model_eval(self.coordinates)

    def _lbfgs_step(self) -> None:
        """The optimizer step alone (anihip_lbfgs_step): coordinates, last_step, converged and n_steps updated."""
        self._params.fmax = float(self.fmax)
        _lib.check(_lib.lib().anihip_lbfgs_step(
            _stream(), C.byref(self._params), self._active.data_ptr(), self.coordinates.data_ptr(), self.forces.data_ptr(),
            self._workspace.data_ptr(), self._workspace.numel(), self.last_step.data_ptr(), self.converged.data_ptr(),
            self.n_steps.data_ptr()))

    def step(self) -> None:
        """One optimizer step on the forces at the current coordinates (convergence tested against ``self.fmax``), then the
        energies and forces at the new coordinates.  No host synchronization."""
        self._lbfgs_step()
        self._evaluate()

    def raise_on_overflow(self) -> None:
        """Raise if a neighbor row of the last evaluation overflowed (one host synchronization)."""
        self._model_eval.raise_on_overflow()

    def run(self, fmax: float = DEFAULT_FMAX, steps: int = 1000, check_every: int = 10) -> OptimizedGeometries:
        """At most ``steps`` steps until every molecule has max |f_i| < fmax (Hartree / Angstrom).  The host reads the
        converged count and the overflow status every ``check_every`` steps and after the last one; molecules whose final
        forces are below fmax count as converged."""
        _check_run_args(fmax, steps, check_every)
        self.fmax = float(fmax)
        for k in range(steps):
            self.step()
            if (k + 1) % check_every == 0 or k + 1 == steps:
                self.raise_on_overflow()
                if bool(self.converged.all()):
                    break
        if steps == 0:
            self.raise_on_overflow()
        fm = (self.forces * self._active.unsqueeze(-1)).to(torch.float64).norm(dim=-1).amax(dim=1)
        self.converged |= fm < self.fmax
        return self.result()

    def result(self) -> OptimizedGeometries:
        """The current state as OptimizedGeometries: copies, which later steps leave alone."""
        return OptimizedGeometries(self.species, self.coordinates.to(self._dtype, copy=True), self.energies.clone(),
                                   self.forces.to(self._dtype, copy=True), self.converged.clone(), self.n_steps.clone())


def optimize_geometry(model, species: Tensor, coordinates: Tensor, cell: tp.Optional[Tensor] = None, pbc=None,
                      **kw) -> OptimizedGeometries:
    """``GeometryOptimizer(model, species, coordinates, cell, pbc, memory=, maxstep=, alpha=, damping=, fixed=)
    .run(fmax=, steps=, check_every=)``."""
    run_kw = {k: kw.pop(k) for k in ("fmax", "steps", "check_every") if k in kw}
    _check_run_args(run_kw.get("fmax", DEFAULT_FMAX), run_kw.get("steps", 1000), run_kw.get("check_every", 10))
    return GeometryOptimizer(model, species, coordinates, cell, pbc, **kw).run(**run_kw)
