"""Named tuples returned by the public API (mirrors torchani/tuples.py:32-36,92-96), and the block-sparse Hessian."""
from __future__ import annotations

import typing as tp

from torch import Tensor


class Neighbors(tp.NamedTuple):
    """Half neighbor list of the reference (neighbors.py:22-29): indices [2, P] into the flattened atoms,
    distances [P], diff_vectors [P, 3] = r[indices[0]] - r[indices[1]] (+ image shift)."""

    indices: Tensor
    distances: Tensor
    diff_vectors: Tensor


class SpeciesAEV(tp.NamedTuple):
    species: Tensor
    aevs: Tensor


class SpeciesEnergies(tp.NamedTuple):
    species: Tensor
    energies: Tensor


class SpeciesEnergiesAtomicCharges(tp.NamedTuple):
    """Output of ANIq models (torchani/tuples.py:59-62)."""

    species: Tensor
    energies: Tensor
    atomic_charges: Tensor


class EnergiesScalars(tp.NamedTuple):
    """Return type of ANI.compute_from_neighbors / compute_from_external_neighbors (torchani/tuples.py:8-10)."""

    energies: Tensor
    scalars: tp.Optional[Tensor] = None


class EnergiesForces(tp.NamedTuple):
    """What grad.energies_and_forces returns: the reference's two-field tuple (torchani/tuples.py:13-15)."""

    energies: Tensor
    forces: Tensor


class FusedEnergiesForces(tp.NamedTuple):
    """Result of the fused engine path (ANI.energies_and_forces): energies [C] float64 Hartree, forces [C,A,3] float32 Ha/A,
    atomic_energies [C,A] float32 (network part only, no self energies)."""

    energies: Tensor
    forces: Tensor
    atomic_energies: Tensor
    virial: tp.Optional[Tensor] = None   # [3,3] float64 Hartree (stress=True): dE/d strain; stress = virial / volume


class HeatFlux(tp.NamedTuple):
    """What grad.heat_flux returns, in Hartree Angstrom / fs: total = kinetic + convective + virial [C, 3] (float64), the
    convective terms sum_i 1/2 m_i |v_i|^2 v_i and sum_i e_i v_i, the virial term -sum_i q_i, and atomic [C, A, 3] (float32),
    the rows q_i = sum_j d_ij (dE_i/d d_ij . v_j)."""

    total: Tensor
    kinetic: Tensor
    convective: Tensor
    virial: Tensor
    atomic: Tensor


class SpeciesForces(tp.NamedTuple):
    """members_forces: energies [M, C], forces [M, C, A, 3] (torchani/tuples.py)."""

    species: Tensor
    energies: Tensor
    forces: Tensor


class SpeciesEnergiesQBC(tp.NamedTuple):
    species: Tensor
    energies: Tensor
    qbcs: Tensor


class AtomicStdev(tp.NamedTuple):
    species: Tensor
    energies: Tensor
    stdev_atomic_energies: Tensor


class ForceMagnitudes(tp.NamedTuple):
    species: Tensor
    magnitudes: Tensor


class ForceStdev(tp.NamedTuple):
    species: Tensor
    magnitudes: Tensor
    relative_stdev: Tensor
    relative_range: Tensor


class EnergiesForcesHessians(tp.NamedTuple):
    """What grad.energies_forces_and_hessians returns (torchani/tuples.py:18-21): hessians [C, 3A, 3A]."""

    energies: Tensor
    forces: Tensor
    hessians: Tensor


class ForcesHessians(tp.NamedTuple):
    """What grad.forces_and_hessians returns (torchani/tuples.py:24-26)."""

    forces: Tensor
    hessians: Tensor


class VibAnalysis(tp.NamedTuple):
    """Frequencies, normal modes, force constants and reduced masses of grad.vibrational_analysis (torchani/tuples.py:36-42)."""

    freqs: Tensor
    modes: Tensor
    fconstants: Tensor
    rmasses: Tensor


class OptimizedGeometries(tp.NamedTuple):
    """What geomopt.GeometryOptimizer.run / geomopt.optimize_geometry return: coordinates [C, A, 3] in the input dtype,
    energies [C] (float64) and forces [C, A, 3] of a final evaluation at those coordinates, converged (bool [C]) and
    n_steps (int32 [C], the steps each molecule moved)."""

    species: Tensor
    coordinates: Tensor
    energies: Tensor
    forces: Tensor
    converged: Tensor
    n_steps: Tensor


class OptimizedSaddles(tp.NamedTuple):
    """What geomopt.SaddleOptimizer.run / geomopt.optimize_saddle return: coordinates [C, A, 3] in the input dtype, energies [C]
    (float64) and forces [C, A, 3] at them, converged (bool [C]), n_steps (int32 [C], the accepted steps), and from one exact
    Hessian at the final geometry, projected like the optimizer's: eigenvalues [C] (float64, Hartree / Angstrom^2) and modes
    [C, A, 3] (float64, unit vectors) of the followed mode, and n_negative (int64 [C]), the number of eigenvalues below
    -negative_tol.  A converged entry with n_negative != 1 is a stationary point of another index."""

    species: Tensor
    coordinates: Tensor
    energies: Tensor
    forces: Tensor
    converged: Tensor
    n_steps: Tensor
    eigenvalues: Tensor
    modes: Tensor
    n_negative: Tensor


class ReactionPaths(tp.NamedTuple):
    """What geomopt.follow_reaction_path returns for C saddles followed for at most P = max_points points to each side:
    coordinates [C, 2P + 1, A, 3] in the input dtype, energies and arc_lengths [C, 2P + 1] (float64; Hartree and Angstrom
    amu^1/2).  Index P is the saddle (arc length 0); the forward points (along the saddle's ``modes``) sit at P + 1, P + 2, ...,
    the backward points at P - 1, P - 2, ... with negative arc lengths; unused slots are NaN.  n_forward, n_backward (int32
    [C]) count the points of each side, reasons (int32 [C, 2], forward then backward) tell why each side ended
    (geomopt.IRC_REASONS)."""

    species: Tensor
    coordinates: Tensor
    energies: Tensor
    arc_lengths: Tensor
    n_forward: Tensor
    n_backward: Tensor
    reasons: Tensor


class PMF(tp.NamedTuple):
    """What md.MBAR.pmf returns: free_energy (float64, in kT, the minimum at 0, inf in empty bins) of shape [bins] or
    [bins_0, bins_1], edges (a tuple of one float64 tensor [bins + 1] per column) and counts (int64, the samples per bin)."""

    free_energy: Tensor
    edges: tp.Tuple[Tensor, ...]
    counts: Tensor


class TorsionScan(tp.NamedTuple):
    """What geomopt.torsion_scan returns for M molecules and K angles: angles [K] (rad, the targets), energies [M, K]
    (float64, Hartree) of the relaxed geometries coordinates [M, K, A, 3], converged (bool [M, K]) and torques [M, K]
    (Hartree / rad) = dE* / d angle = minus the constraint's multiplier.  A scan of one molecule drops the M axis."""

    angles: Tensor
    energies: Tensor
    coordinates: Tensor
    converged: Tensor
    torques: Tensor


class SparseVibAnalysis(tp.NamedTuple):
    """What grad.sparse_vibrational_analysis returns for C molecules and k modes: freqs [C, k], modes [C, k, A, 3],
    fconstants [C, k] and rmasses [C, k] as in VibAnalysis (zero on padding atoms), eigenvalues [C, k] of the mass-weighted
    Hessian (fp64, Hartree / (amu Angstrom^2), ascending), residuals [C, k] = ||A q - theta q|| of the mass-weighted unit
    modes q, and n_iter, the solver's iteration count (0 when every molecule was solved densely)."""

    freqs: Tensor
    modes: Tensor
    fconstants: Tensor
    rmasses: Tensor
    eigenvalues: Tensor
    residuals: Tensor
    n_iter: int


class BlockHessian:
    """Block-sparse Hessian with respect to the coordinates of a batch (grad.energies_forces_and_sparse_hessians).

    index: int64 [2, nnz] of flattened atom indices c * A + a; blocks: [nnz, 3, 3] with
    blocks[p][x, y] = d^2 E / d r_{index[0, p], x} d r_{index[1, p], y}.  The pattern is symmetric ((i, j) and (j, i) are both
    stored), never crosses molecules and holds no padding atom.  The engine stores it by columns: the entries with
    index[1] = a are contiguous, index[0] ascending."""

    def __init__(self, index: Tensor, blocks: Tensor, n_molecules: int, n_atoms: int) -> None:
        if index.dim() != 2 or index.shape[0] != 2 or blocks.shape != (index.shape[1], 3, 3):
            raise ValueError("index must be [2, nnz] and blocks [nnz, 3, 3]")
        self.index = index
        self.blocks = blocks
        self.n_molecules = int(n_molecules)
        self.n_atoms = int(n_atoms)

    @property
    def nnz(self) -> int:
        return int(self.index.shape[1])

    def __repr__(self) -> str:
        return f"BlockHessian(n_molecules={self.n_molecules}, n_atoms={self.n_atoms}, nnz={self.nnz})"

    def to_dense(self) -> Tensor:
        """[C, 3A, 3A]: the layout of grad.energies_forces_and_hessians (zeros outside the pattern)."""
        import torch

        C, A = self.n_molecules, self.n_atoms
        H = torch.zeros((C, A, 3, A, 3), dtype=self.blocks.dtype, device=self.blocks.device)
        i, j = self.index[0], self.index[1]
        H[i // A, i % A, :, j % A, :] = self.blocks
        return H.reshape(C, 3 * A, 3 * A)

    def to_sparse_coo(self) -> Tensor:
        """Coalesced torch sparse COO tensor [C 3A, C 3A] of the scalar entries (row 3 (c A + a) + x)."""
        import torch

        n = 3 * self.n_molecules * self.n_atoms
        x = torch.arange(3, device=self.index.device)
        rows = (3 * self.index[0]).view(-1, 1, 1) + x.view(1, 3, 1)
        cols = (3 * self.index[1]).view(-1, 1, 1) + x.view(1, 1, 3)
        idx = torch.stack([rows.expand(-1, 3, 3).reshape(-1), cols.expand(-1, 3, 3).reshape(-1)])
        return torch.sparse_coo_tensor(idx, self.blocks.reshape(-1), (n, n)).coalesce()

    def matvec(self, v: Tensor) -> Tensor:
        """H v for v of C * A * 3 elements ([C, A, 3], [C, 3A] or flat): the result has v's shape."""
        import torch

        N = self.n_molecules * self.n_atoms
        if v.numel() != 3 * N:
            raise ValueError(f"v must hold {3 * N} elements (C * A * 3)")
        vf = v.reshape(N, 3).to(self.blocks.dtype)
        prod = torch.bmm(self.blocks, vf[self.index[1]].unsqueeze(-1)).squeeze(-1)
        out = torch.zeros((N, 3), dtype=self.blocks.dtype, device=self.blocks.device).index_add_(0, self.index[0], prod)
        return out.reshape(v.shape)


class EnergiesForcesSparseHessians(tp.NamedTuple):
    """What grad.energies_forces_and_sparse_hessians returns: hessians is a BlockHessian."""

    energies: Tensor
    forces: Tensor
    hessians: BlockHessian


class EnergiesForcesStrainHessians(tp.NamedTuple):
    """What grad.energies_forces_and_strain_hessians returns.  With the strain x -> x S, cell -> cell S at S = I:
    virial [C, 3, 3] = d E_c / d S (per molecule), strain_hessians [C, 3, 3, 3, 3] = d^2 E_c / d S_ab d S_pq (all 81
    components, rotations included) and internal_strain [C, A, 3, 3, 3] = d^2 E_c / d x_iy d S_ab (x unstrained)."""

    energies: Tensor
    forces: Tensor
    virial: Tensor
    strain_hessians: Tensor
    internal_strain: Tensor


class Supercell(tp.NamedTuple):
    """What phonons.supercell returns: r1 x r2 x r3 copies of a primitive cell of n atoms, N = r1 r2 r3 n atoms in cell-major
    order (atom ((l1 r2 + l2) r3 + l3) n + b).  species [1, N], coordinates [1, N, 3] (built in float64 as tau_b + l . a, cast
    once to the input dtype), cell [3, 3] (rows r_k a_k), basis int32 [N] (b) and lattice int32 [N, 3] (l) of every atom,
    repeats, and the primitive data in float64: primitive_species [n], primitive_coordinates [n, 3], primitive_cell [3, 3]."""

    species: Tensor
    coordinates: Tensor
    cell: Tensor
    basis: Tensor
    lattice: Tensor
    repeats: tp.Tuple[int, int, int]
    primitive_species: Tensor
    primitive_coordinates: Tensor
    primitive_cell: Tensor


class ForceConstants(tp.NamedTuple):
    """Compact force constants of a crystal (phonons.force_constants): entry e is the 3 x 3 block phi[e] = Phi(b; b', n)
    (Hartree / Angstrom^2, float64) between basis atom b = ent_b[e] in some cell and basis atom b' = ent_bp[e] in the cell
    displaced by the lattice vector nvec[e] (int32 [m, 3]; rvec = nvec @ cell in Angstrom).  The entries are sorted by (b, b'):
    those of basis atom b are boff[b] .. boff[b + 1], those of the pair (b, b') poff[b n + b'] .. poff[b n + b' + 1] (int32).
    cell [3, 3], positions [n, 3] and masses [n] (amu) are the primitive cell's, in float64.  exact: every perpendicular width
    of the supercell exceeds four radial cutoffs, so D(q) is exact at any q and not only at commensurate ones.
    translation_defect: the largest deviation of a translated block from its mean over max |phi|; n_missing: translated
    blocks that were not stored.  energy (Hartree) and max_force (Hartree / Angstrom) are the supercell's (None when built
    from a Hessian alone): a max_force that is not small means the frequencies are not those of a minimum."""

    cell: Tensor
    positions: Tensor
    masses: Tensor
    repeats: tp.Tuple[int, int, int]
    boff: Tensor
    poff: Tensor
    ent_b: Tensor
    ent_bp: Tensor
    nvec: Tensor
    rvec: Tensor
    phi: Tensor
    exact: bool
    translation_defect: float
    n_missing: int
    energy: tp.Optional[Tensor] = None
    max_force: tp.Optional[Tensor] = None

    @property
    def n_basis(self) -> int:
        return int(self.masses.numel())


class PhononModes(tp.NamedTuple):
    """What phonons.modes returns for Q wave vectors of a crystal with n basis atoms: q [Q, 3] (fractional), frequencies
    [Q, 3n] in the unit asked for (ascending, imaginary ones negative), eigenvalues [Q, 3n] of D(q) (Hartree / (amu
    Angstrom^2)), eigenvectors complex128 [Q, 3n, 3n] (columns; None unless asked for) and group_velocities [Q, 3n, 3]
    (Angstrom / fs; None unless asked for)."""

    q: Tensor
    frequencies: Tensor
    eigenvalues: Tensor
    eigenvectors: tp.Optional[Tensor]
    group_velocities: tp.Optional[Tensor]


class PhononThermodynamics(tp.NamedTuple):
    """Harmonic thermodynamics per primitive cell at temperatures [T] (K): zero_point_energy (Hartree, a scalar tensor),
    free_energy [T] (Helmholtz, Hartree), entropy [T] and heat_capacity [T] (C_v; Hartree / K), and n_imaginary, the number
    of modes of the mesh with f <= 0, which are left out of every sum."""

    temperatures: Tensor
    zero_point_energy: Tensor
    free_energy: Tensor
    entropy: Tensor
    heat_capacity: Tensor
    n_imaginary: int


class PhononMesh:
    """Frequencies on a Monkhorst-Pack mesh (phonons.mesh): q [Q, 3], weights [Q] (sum 1, q and -q merged), frequencies
    [Q, 3n] in ``unit`` and eigenvalues [Q, 3n] of D(q)."""

    def __init__(self, q: Tensor, weights: Tensor, frequencies: Tensor, eigenvalues: Tensor, unit: str) -> None:
        self.q = q
        self.weights = weights
        self.frequencies = frequencies
        self.eigenvalues = eigenvalues
        self.unit = unit

    def dos(self, bins: int, f_max: tp.Optional[float] = None, sigma: tp.Optional[float] = None,
            f_min: float = 0.0) -> tp.Tuple[Tensor, Tensor]:
        """(centres [bins], g [bins]) of the Gaussian-smeared density of states g(f) = sum_{q, nu} w_q G_sigma(f - f_{q nu})
        per primitive cell and frequency unit, on the regular centres f_min + (k + 1/2) (f_max - f_min) / bins.  f_max
        defaults to 1.05 x the largest frequency, sigma to two bin widths."""
        from . import phonons

        return phonons.dos(self, bins, f_max=f_max, sigma=sigma, f_min=f_min)

    def thermodynamics(self, temperatures) -> PhononThermodynamics:
        from . import phonons

        return phonons.thermodynamics(self, temperatures)
