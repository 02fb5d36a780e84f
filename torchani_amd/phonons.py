"""Phonons of periodic crystals from block-sparse supercell Hessians: force constants, dynamical matrices, band structures,
densities of states, harmonic thermodynamics and group velocities.

Conventions.  The primitive cell has lattice rows a_1, a_2, a_3 (Angstrom) and n basis atoms at tau_b with masses m_b.  The
supercell of repeats = (r_1, r_2, r_3) holds N_c = r_1 r_2 r_3 cells in cell-major order: atom ((l_1 r_2 + l_2) r_3 + l_3) n + b
at tau_b + l . a (built in float64, cast once).  Phi(b; b', n) is the 3 x 3 block between atom b of a cell and atom b' of the cell
displaced by the lattice vector n: the mean, over the N_c cells l, of the symmetrized supercell block between (b, l) and
(b', l + n mod repeats) (anihip_phonon_fold).  The dynamical matrix uses the lattice-vector phase convention,

    D(q)_{3b+x, 3b'+y} = (m_b m_b')^-1/2 sum_n Phi(b; b', n)_xy exp(2 pi i q . n),

q in fractional reciprocal coordinates, so D(q + G) = D(q), D is Hermitian and D(-q) = conj D(q).  Its eigenvalues are in
Hartree / (amu Angstrom^2), the unit grad.vibrational_analysis diagonalizes, and become frequencies through grad._freq_unit,
imaginary ones negative.

At a commensurate q (every q_k r_k an integer) D(q) is exact for any supercell: the images that the supercell folds onto one
atom carry equal phases.  At a general q it is exact only when every perpendicular width of the supercell exceeds twice the
reach of the Hessian's blocks (for an ANI model 2 R_c, i.e. widths above 4 R_c): then every pair has one image
(ForceConstants.exact).  The lattice vector of an entry is the minimum image by atom distance from the ideal positions in
float64; among equidistant images the first in a fixed order is taken with its full weight: there is no Wigner-Seitz
splitting.  Not done either: the non-analytic LO-TO correction, symmetry beyond time reversal, anharmonicity, more than one
GPU.
"""
from __future__ import annotations

import math
import typing as tp

import torch
from torch import Tensor

from . import _lib
from . import units as _units
from .tuples import BlockHessian, ForceConstants, PhononMesh, PhononModes, PhononThermodynamics, Supercell

# sqrt(eigenvalue of D) in sqrt(Hartree / (amu Angstrom^2)) -> angular frequency in rad / fs (the constants of units)
SQRT_MHESSIAN_TO_RAD_PER_FS = math.sqrt(_units.HARTREE_TO_JOULE / _units.AMU_TO_KG) / _units.ANGSTROM_TO_METER * 1e-15
HBAR = _lib.MD_HBAR                  # Hartree fs
KB = 3.166811563e-6                  # Hartree / K (md.KB_HARTREE)
COMMENSURATE_TOL = 1e-9
TIE_TOL = 1e-9                       # images within this relative squared distance of the nearest count as equidistant
LEX_SPAN = 1 << 16                   # lattice-vector components lie inside +-LEX_SPAN (the tie order's radix)
MESH_CHUNK = 512                     # q points per dynamical-matrix batch of phonons.mesh


def _check_repeats(repeats) -> tp.Tuple[int, int, int]:
    try:
        r = tuple(int(x) for x in repeats)
        whole = all(int(x) == x for x in repeats)
    except (TypeError, ValueError):
        raise ValueError(f"repeats must be three integers >= 1, got {repeats!r}") from None
    if len(r) != 3 or min(r) < 1 or not whole:
        raise ValueError(f"repeats must be three integers >= 1, got {repeats!r}")
    return r  # type: ignore[return-value]


def _check_pbc(pbc) -> None:
    if pbc is None:
        return
    flags = pbc.tolist() if isinstance(pbc, Tensor) else list(pbc)
    if len(flags) != 3 or not all(bool(f) for f in flags):
        raise ValueError("phonons need a cell that is periodic along all three axes")


def _cells(repeats: tp.Tuple[int, int, int], device) -> Tensor:
    """int64 [N_c, 3]: the cell indices l in cell-major order (l_3 fastest)."""
    return torch.cartesian_prod(*[torch.arange(r, device=device) for r in repeats]).reshape(-1, 3)


def _supercell(species: Tensor, coordinates: Tensor, cell: Tensor, repeats) -> Supercell:
    """phonons.supercell without the device check (the host tests run it on CPU tensors)."""
    r = _check_repeats(repeats)
    if cell is None or tuple(cell.shape) != (3, 3):
        raise ValueError("cell must be [3, 3]")
    n = species.numel()
    if species.dim() > 2 or (species.dim() == 2 and species.shape[0] != 1) or coordinates.numel() != 3 * n or n < 1:
        raise ValueError("species must be [1, n] and coordinates [1, n, 3]: one primitive cell")
    a = cell.detach().to(torch.float64)
    tau = coordinates.detach().reshape(n, 3).to(torch.float64)
    cells = _cells(r, species.device)
    x = (tau.unsqueeze(0) + _rows_times(cells.to(torch.float64), a).unsqueeze(1)).reshape(1, -1, 3)
    nc = cells.shape[0]
    scale = torch.tensor(r, dtype=torch.float64, device=cell.device).unsqueeze(1)
    return Supercell(species.reshape(1, n).repeat(1, nc), x.to(coordinates.dtype), (a * scale).to(cell.dtype),
                     torch.arange(n, dtype=torch.int32, device=species.device).repeat(nc),
                     cells.to(torch.int32).repeat_interleave(n, dim=0), r, species.reshape(n), tau, a)


def supercell(species: Tensor, coordinates: Tensor, cell: Tensor, repeats, pbc=None) -> Supercell:
    """tuples.Supercell of repeats = (r_1, r_2, r_3) copies of the primitive cell species [1, n], coordinates [1, n, 3],
    cell [3, 3], in cell-major order.  pbc, when given, must be periodic along all three axes."""
    from .engine import _require_cuda

    _check_repeats(repeats)
    _check_pbc(pbc)
    _require_cuda(species, coordinates, cell)
    return _supercell(species, coordinates, cell, repeats)


def _rows_times(v: Tensor, a: Tensor) -> Tensor:
    """v [..., 3] times the 3 x 3 matrix a (rows a_k): v_0 a_0 + v_1 a_1 + v_2 a_2, written out.  The pattern construction
    stays on elementwise device kernels: no BLAS or LAPACK call on these 3 x 3 problems."""
    return v[..., 0:1] * a[0] + v[..., 1:2] * a[1] + v[..., 2:3] * a[2]


def _inverse_and_volume(a: Tensor) -> tp.Tuple[Tensor, Tensor]:
    """(inv(a), det(a)) of a cell [3, 3] in closed form: the columns of the inverse are the cross products a_j x a_k / det."""
    cr = torch.stack([torch.linalg.cross(a[1], a[2]), torch.linalg.cross(a[2], a[0]), torch.linalg.cross(a[0], a[1])])
    det = (a[0] * cr[0]).sum()
    return cr.T / det, det


def _widths(cell: Tensor) -> Tensor:
    """The three perpendicular widths of a cell [3, 3] (float64)."""
    a = cell.to(torch.float64)
    cr = torch.stack([torch.linalg.cross(a[1], a[2]), torch.linalg.cross(a[2], a[0]), torch.linalg.cross(a[0], a[1])])
    return (a[0] * cr[0]).sum().abs() / cr.norm(dim=1)


def _shifts(device) -> Tensor:
    return torch.cartesian_prod(*[torch.arange(-1, 2, device=device)] * 3)   # int64 [27, 3], a fixed order


def _lattice_vectors(positions: Tensor, cell: Tensor, repeats: tp.Tuple[int, int, int], b: Tensor, j: Tensor) -> Tensor:
    """int64 [m, 3]: the lattice vector n from the cell of basis atom b [m] to the image of supercell atom j [m] nearest to
    it, from the ideal positions in float64.  Rounding the fractional supercell components of tau_b' + l' . a - tau_b gives
    the minimum image when the supercell is wide; its 27 neighbours are compared by distance for the skewed and thin ones.
    Images within TIE_TOL (relative, squared distance) of the nearest count as equidistant: the one whose lattice vector
    comes first in lexicographic order is taken for b < b' (for b = b': when the cell of j comes before its mirror cell),
    the last one otherwise, so that the two directions of a pair take opposite vectors."""
    n = positions.shape[0]
    r = torch.tensor(repeats, dtype=torch.int64, device=positions.device)
    lc, bp = j // n, j % n
    lp = torch.stack([lc // (repeats[1] * repeats[2]), (lc // repeats[2]) % repeats[1], lc % repeats[2]], dim=1)   # [m, 3]
    d = positions[bp] + _rows_times(lp.to(torch.float64), cell) - positions[b]
    frac = _rows_times(d, _inverse_and_volume(cell)[0]) / r.to(torch.float64)   # fractional supercell components
    base = lp - r * torch.round(frac).to(torch.int64)
    cand = base.unsqueeze(1) + _shifts(positions.device).unsqueeze(0) * r    # [m, 27, 3]
    dc = positions[bp].unsqueeze(1) + _rows_times(cand.to(torch.float64), cell) - positions[b].unsqueeze(1)
    d2 = (dc * dc).sum(dim=2)
    near = d2 <= d2.amin(dim=1, keepdim=True) * (1.0 + TIE_TOL) + 1e-300
    rank = ((cand[..., 0] + LEX_SPAN) * (2 * LEX_SPAN) + cand[..., 1] + LEX_SPAN) * (2 * LEX_SPAN) + cand[..., 2] + LEX_SPAN
    # the pair seen from the other side has the negated candidates: it must take the negated vector (D(q) Hermitian)
    mirror = ((-lp % r)[:, 0] * repeats[1] + (-lp % r)[:, 1]) * repeats[2] + (-lp % r)[:, 2]
    first = (b < bp) | ((b == bp) & (lc <= mirror))
    pick = torch.where(first, torch.where(near, rank, torch.full_like(rank, 8 * LEX_SPAN ** 3)).argmin(dim=1),
                       torch.where(near, rank, torch.full_like(rank, -1)).argmax(dim=1))
    return torch.gather(cand, 1, pick.view(-1, 1, 1).expand(-1, 1, 3)).squeeze(1)


def _compact_pattern(index: Tensor, n: int, n_atoms: int):
    """The home cell's columns of a column-sorted index, sorted by (b, b', j): (ent_b, ent_j int64 [m], boff int32 [n + 1],
    poff int32 [n^2 + 1], diag_entry int32 [n])."""
    home = (index[1] < n).nonzero().squeeze(1)
    b, j = index[1][home], index[0][home]
    order = torch.argsort((b * n + j % n) * n_atoms + j)
    b, j = b[order], j[order]
    dev = index.device
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    boff = torch.cat([zero, torch.bincount(b, minlength=n).cumsum(0)]).to(torch.int32)
    poff = torch.cat([zero, torch.bincount(b * n + j % n, minlength=n * n).cumsum(0)]).to(torch.int32)
    diag = torch.full((n,), -1, dtype=torch.int32, device=dev)
    own = (b == j).nonzero().squeeze(1)
    diag[b[own]] = own.to(torch.int32)
    return b, j, boff, poff, diag


def force_constants_from_hessian(hessian: BlockHessian, supercell: Supercell, masses: Tensor, acoustic_sum_rule: bool = True,
                                 reach: tp.Optional[float] = None) -> ForceConstants:
    """tuples.ForceConstants from the BlockHessian of ``supercell`` (one molecule of N = N_c n atoms in the order of
    phonons.supercell), computed by a model or built by hand; masses [n] or [1, n] (amu) of the primitive cell.

    anihip_block_hessian_prepare (unit masses) symmetrizes the blocks; the compact pattern is the home cell's columns,
    built on the device with torch; anihip_phonon_fold averages every entry over the N_c translations.  acoustic_sum_rule
    replaces Phi(b; b, 0) by minus the symmetrized sum of b's other entries, which puts the three acoustic eigenvalues at
    Gamma at zero.  reach: the largest distance (Angstrom) at which the Hessian couples two atoms (2 R_c for an ANI model);
    ``exact`` is set when every perpendicular width of the supercell exceeds twice that, and is False without it."""
    from .engine import _require_cuda, block_hessian_prepare, phonon_fold

    if not isinstance(hessian, BlockHessian):
        raise TypeError("hessian must be a tuples.BlockHessian")
    sc = supercell
    n = int(sc.primitive_species.numel())
    r = _check_repeats(sc.repeats)
    N = n * r[0] * r[1] * r[2]
    if hessian.n_molecules != 1 or hessian.n_atoms != N:
        raise ValueError(f"the Hessian must be that of the supercell: 1 molecule of {N} atoms, got {hessian!r}")
    if masses.numel() != n or masses.dim() > 2:
        raise ValueError(f"masses must be [n] = [{n}] (the primitive cell's), got {list(masses.shape)}")
    _require_cuda(hessian.index, hessian.blocks, masses, sc.primitive_coordinates, sc.primitive_cell)
    dev = hessian.blocks.device
    with torch.no_grad():
        m64 = masses.detach().reshape(n).to(torch.float64)
        if not bool((torch.isfinite(m64) & (m64 > 0)).all()):
            raise ValueError("masses must be positive and finite")
        index, blocks = hessian.index, hessian.blocks
        if hessian.nnz > 1:
            key = index[1] * N + index[0]
            if bool((key[1:] <= key[:-1]).any()):   # a hand-built Hessian: put it in column order once
                order = torch.argsort(key)
                index, blocks = index[:, order], blocks[order]
        op = block_hessian_prepare(index, blocks, torch.ones(N, dtype=torch.float64, device=dev))
        ent_b, ent_j, boff, poff, diag = _compact_pattern(index, n, N)
        a, tau = sc.primitive_cell.to(torch.float64), sc.primitive_coordinates.to(torch.float64)
        nvec = _lattice_vectors(tau, a, r, ent_b, ent_j)
        b32, j32 = ent_b.to(torch.int32).contiguous(), ent_j.to(torch.int32).contiguous()
        phi, missing, defect = phonon_fold(op, n, r, b32, j32, *((boff, diag) if acoustic_sum_rule else (None, None)))
        if phi.numel():
            n_missing, dmax, pmax = torch.stack([missing.sum().double(), defect.max(), phi.abs().max()]).tolist()
        else:
            n_missing, dmax, pmax = 0.0, 0.0, 0.0
        widths = _widths(a * torch.tensor(r, dtype=torch.float64, device=dev).unsqueeze(1))
        exact = reach is not None and bool((widths > 2.0 * float(reach)).all())
    return ForceConstants(a, tau, m64, r, boff, poff, b32, (ent_j % n).to(torch.int32), nvec.to(torch.int32).contiguous(),
                          _rows_times(nvec.to(torch.float64), a).contiguous(), phi, exact, dmax / pmax if pmax > 0 else 0.0,
                          int(n_missing))


def force_constants(model, species: Tensor, coordinates: Tensor, cell: Tensor, repeats, masses: tp.Optional[Tensor] = None,
                    acoustic_sum_rule: bool = True, pbc=None) -> ForceConstants:
    """tuples.ForceConstants of the crystal species [1, n], coordinates [1, n, 3], cell [3, 3] from the analytic block-sparse
    Hessian of its supercell: phonons.supercell, grad.energies_forces_and_sparse_hessians with all three axes periodic,
    force_constants_from_hessian with reach = 2 R_c.  masses [n] (amu) default to the standard atomic masses of the species.

    The geometry is taken as given: ``max_force`` of the result is the largest force component of the supercell, and unless
    it is small (a relaxed structure) the frequencies are not those of a minimum.  The models served are those of the
    sparse Hessian: ANI-r2s raises ValueError, D3 (ANI-2dr) and standalone pair potentials NotImplementedError."""
    from . import grad
    from .engine import _require_cuda
    from .utils import atomic_numbers_to_masses

    _check_repeats(repeats)
    _check_pbc(pbc)
    n = species.numel()
    if masses is not None and (masses.numel() != n or masses.dim() > 2):
        raise ValueError(f"masses must be [n] = [{n}] (the primitive cell's), got {list(masses.shape)}")
    _require_cuda(species, coordinates, cell, masses)
    sc = _supercell(species, coordinates, cell, repeats)
    if masses is None:
        z = species.reshape(-1) if getattr(model, "periodic_table_index", False) else model.atomic_numbers[species.reshape(-1)]
        masses = atomic_numbers_to_masses(z, dtype=torch.float64)
    out = grad.energies_forces_and_sparse_hessians(model, sc.species, sc.coordinates, cell=sc.cell,
                                                   pbc=torch.ones(3, dtype=torch.bool, device=cell.device))
    fc = force_constants_from_hessian(out.hessians, sc, masses, acoustic_sum_rule, reach=2.0 * float(model.cutoff))
    return fc._replace(energy=out.energies.detach().reshape(-1)[0], max_force=out.forces.detach().abs().max())


def _as_q(fc: ForceConstants, q) -> Tensor:
    if isinstance(q, Tensor):
        if q.dim() != 2 or q.shape[1] != 3 or q.shape[0] < 1:
            raise ValueError(f"q must be [Q, 3] with Q >= 1 (fractional reciprocal coordinates), got {list(q.shape)}")
        return q.detach().to(torch.float64).contiguous()
    qt = torch.as_tensor(q, dtype=torch.float64)
    if qt.dim() != 2 or qt.shape[1] != 3 or qt.shape[0] < 1:
        raise ValueError(f"q must be [Q, 3] with Q >= 1 (fractional reciprocal coordinates), got {list(qt.shape)}")
    return qt.to(fc.phi.device).contiguous()


def is_commensurate(q: Tensor, repeats: tp.Sequence[int]) -> Tensor:
    """bool [Q]: every q_k r_k is an integer (to 1e-9)."""
    t = q.to(torch.float64) * torch.tensor(list(repeats), dtype=torch.float64, device=q.device)
    return ((t - torch.round(t)).abs() <= COMMENSURATE_TOL).all(dim=1)


def dynamical_matrices(fc: ForceConstants, q, derivatives: bool = False, allow_aliasing: bool = False):
    """D(q) complex128 [Q, 3n, 3n] for q [Q, 3] (a device tensor, or a nested sequence) from anihip_phonon_dynmat; with
    derivatives also dD / dk [Q, 3, 3n, 3n], k the Cartesian wave vector in rad / Angstrom.  On a supercell that is not
    ``exact`` a q that is not commensurate with it raises ValueError unless allow_aliasing: D(q) then interpolates with one
    of several images per pair."""
    from .engine import _require_cuda, phonon_dynmat

    qt = _as_q(fc, q)
    if not fc.exact and not allow_aliasing and not bool(is_commensurate(qt, fc.repeats).all()):
        raise ValueError(f"the supercell {fc.repeats} is narrower than four cutoffs, so D(q) is exact only at q commensurate "
                         "with it: pass allow_aliasing=True to interpolate anyway, or use a larger supercell")
    _require_cuda(qt, fc.phi)
    D, dD = phonon_dynmat(fc.n_basis, fc.poff, fc.nvec, fc.phi, fc.rvec, fc.masses, qt, derivatives)
    return (D, dD) if derivatives else D


def _eigh(D: Tensor, eigensolver: str) -> tp.Tuple[Tensor, Tensor]:
    if eigensolver == "device":
        return torch.linalg.eigh(D)
    if eigensolver == "host":
        lam, vec = torch.linalg.eigh(D.cpu())
        return lam.to(D.device), vec.to(D.device)
    raise ValueError('eigensolver must be "device" or "host"')


def _signed_sqrt(lam: Tensor) -> Tensor:
    return lam.abs().sqrt() * torch.sign(lam)


def modes(fc: ForceConstants, q, unit: str = "cm^-1", eigenvectors: bool = False, group_velocities: bool = False,
          eigensolver: str = "device", allow_aliasing: bool = False) -> PhononModes:
    """tuples.PhononModes at q [Q, 3]: torch.linalg.eigh of the complex128 batch D(q), on the device ("device") or on a host
    copy ("host").  Frequencies as grad.vibrational_analysis: sqrt |eigenvalue| / 2 pi in ``unit``, negative for negative
    eigenvalues.  Group velocities v = Re(e^H dD/dk_a e) / (2 omega) in Angstrom / fs with omega in rad / fs; zero where
    |omega| is below 1e-6 of the largest in the call (the acoustic modes at Gamma have no defined direction).  Inside a
    degenerate set the individual velocities depend on the eigenvector basis eigh returns; only their sum is defined."""
    from . import grad

    to_unit = grad._freq_unit(unit)
    if eigensolver not in ("device", "host"):
        raise ValueError('eigensolver must be "device" or "host"')
    qt = _as_q(fc, q)
    with torch.no_grad():
        out = dynamical_matrices(fc, qt, derivatives=group_velocities, allow_aliasing=allow_aliasing)
        D, dD = out if group_velocities else (out, None)
        lam, vec = _eigh(D, eigensolver)
        root = _signed_sqrt(lam)
        vel = None
        if group_velocities:
            num = (vec.conj().unsqueeze(1) * (dD @ vec.unsqueeze(1))).sum(dim=2).real.permute(0, 2, 1)   # [Q, 3n, 3]
            small = (root.abs() <= 1e-6 * root.abs().max()).unsqueeze(2)
            den = (2.0 * root).unsqueeze(2)
            vel = torch.where(small, torch.zeros_like(num),
                              SQRT_MHESSIAN_TO_RAD_PER_FS * num / torch.where(small, torch.ones_like(den), den))
    return PhononModes(qt, to_unit(root / (2 * math.pi)), lam, vec if eigenvectors else None, vel)


def band_path(points, n_per_segment: int, cell: tp.Optional[Tensor] = None, device=None) -> tp.Tuple[Tensor, Tensor]:
    """(q [S n_per_segment + 1, 3], length [S n_per_segment + 1]) along the S segments between consecutive ``points``
    (fractional reciprocal coordinates): n_per_segment equal steps per segment, every end point included once.  length is
    the cumulative path length in rad / Angstrom with the reciprocal lattice 2 pi inv(cell)^T of ``cell`` [3, 3], or in
    fractional units without one.  The tensors are float64 on ``device`` (default: the cell's, else the CPU)."""
    p = torch.as_tensor(points, dtype=torch.float64).cpu()
    if p.dim() != 2 or p.shape[1] != 3 or p.shape[0] < 2 or int(n_per_segment) < 1:
        raise ValueError("points must be [P >= 2, 3] and n_per_segment >= 1")
    k = int(n_per_segment)
    recip = torch.eye(3, dtype=torch.float64) if cell is None else \
        2 * math.pi * torch.linalg.inv(cell.detach().to(torch.float64).cpu()).T     # rows b_k
    t = torch.arange(k, dtype=torch.float64) / k
    seg = [p[s] + t.unsqueeze(1) * (p[s + 1] - p[s]) for s in range(p.shape[0] - 1)]
    q = torch.cat(seg + [p[-1:]])
    step = ((q[1:] - q[:-1]) @ recip).norm(dim=1)
    length = torch.cat([torch.zeros(1, dtype=torch.float64), step.cumsum(0)])
    dev = device if device is not None else (cell.device if cell is not None else "cpu")
    return q.to(dev), length.to(dev)


def monkhorst_pack(mesh, shift=(0, 0, 0), device=None) -> tp.Tuple[Tensor, Tensor]:
    """(q [Q, 3], weights [Q]) of the regular mesh q_k = (i_k + shift_k / 2) / mesh_k, i_k < mesh_k, folded into [-1/2, 1/2),
    with q and -q merged by time reversal (D(-q) = conj D(q) has the same eigenvalues): the weights sum to 1.  shift_k is 0
    (the mesh holds Gamma) or 1 (half a step off)."""
    try:
        m = [int(x) for x in mesh]
        s = [int(x) for x in shift]
    except (TypeError, ValueError):
        raise ValueError("mesh and shift must be three integers each") from None
    if len(m) != 3 or min(m) < 1 or len(s) != 3 or any(x not in (0, 1) for x in s):
        raise ValueError("mesh must be three integers >= 1 and shift three values of 0 or 1")
    idx = torch.cartesian_prod(*[torch.arange(x) for x in m]).reshape(-1, 3)
    mt, st = torch.tensor(m), torch.tensor(s)
    mate = (mt - idx - st) % mt                                          # -q on the mesh
    lin = (idx[:, 0] * m[1] + idx[:, 1]) * m[2] + idx[:, 2]
    lin_mate = (mate[:, 0] * m[1] + mate[:, 1]) * m[2] + mate[:, 2]
    keep = lin <= lin_mate
    w = torch.where(lin == lin_mate, 1.0, 2.0).to(torch.float64)[keep] / idx.shape[0]
    q = (idx[keep].to(torch.float64) + 0.5 * st.to(torch.float64)) / mt.to(torch.float64)
    q = q - torch.floor(q + 0.5)
    dev = device if device is not None else "cpu"
    return q.to(dev), w.to(dev)


def mesh(fc: ForceConstants, mesh, shift=(0, 0, 0), unit: str = "cm^-1", eigensolver: str = "device",
         allow_aliasing: bool = False) -> PhononMesh:
    """tuples.PhononMesh: the frequencies on monkhorst_pack(mesh, shift), MESH_CHUNK q points per batch."""
    q, w = monkhorst_pack(mesh, shift, device=fc.phi.device)
    freqs, lams = [], []
    for lo in range(0, q.shape[0], MESH_CHUNK):
        md = modes(fc, q[lo:lo + MESH_CHUNK], unit=unit, eigensolver=eigensolver, allow_aliasing=allow_aliasing)
        freqs.append(md.frequencies)
        lams.append(md.eigenvalues)
    return PhononMesh(q, w, torch.cat(freqs), torch.cat(lams), unit)


def dos(pm: PhononMesh, bins: int, f_max: tp.Optional[float] = None, sigma: tp.Optional[float] = None,
        f_min: float = 0.0) -> tp.Tuple[Tensor, Tensor]:
    """PhononMesh.dos: anihip_phonon_dos over the mesh's frequencies (one workgroup per bin, a fixed summation order)."""
    from .engine import phonon_dos

    if int(bins) < 1:
        raise ValueError("bins must be >= 1")
    if f_max is None:
        f_max = 1.05 * float(pm.frequencies.max())
    if not f_max > f_min:
        raise ValueError("f_max must exceed f_min")
    df = (float(f_max) - float(f_min)) / int(bins)
    sigma = 2.0 * df if sigma is None else float(sigma)
    if not sigma > 0:
        raise ValueError("sigma must be positive")
    f = pm.frequencies.to(torch.float64).contiguous()
    w = pm.weights.to(torch.float64).unsqueeze(1).expand_as(f).contiguous()
    first = float(f_min) + 0.5 * df
    g = phonon_dos(f.reshape(-1), w.reshape(-1), first, df, sigma, int(bins))
    return first + df * torch.arange(int(bins), dtype=torch.float64, device=g.device), g


def thermodynamics(pm: PhononMesh, temperatures) -> PhononThermodynamics:
    """PhononMesh.thermodynamics: the closed forms of independent harmonic oscillators, per primitive cell, in float64 torch.
    With e = hbar omega and x = e / (k_B T):  E_0 = sum w e / 2,  F = E_0 + k_B T sum w ln(1 - exp(-x)),
    S = k_B sum w (x / (exp(x) - 1) - ln(1 - exp(-x))),  C_v = k_B sum w (x / (2 sinh(x / 2)))^2.  Modes with f <= 0 are
    left out and counted."""
    lam = pm.eigenvalues.to(torch.float64)
    T = torch.as_tensor(temperatures, dtype=torch.float64, device=lam.device).reshape(-1)
    if bool((T < 0).any()):
        raise ValueError("temperatures must be >= 0 K")
    real = lam > 0
    e = HBAR * SQRT_MHESSIAN_TO_RAD_PER_FS * torch.where(real, lam, torch.ones_like(lam)).sqrt()       # [Q, 3n] Hartree
    w = pm.weights.to(torch.float64).unsqueeze(1) * real                                                # excluded: weight 0
    zpe = 0.5 * (w * e).sum()
    hot = T > 0
    kT = KB * torch.where(hot, T, torch.ones_like(T))
    x = e.unsqueeze(0) / kT.view(-1, 1, 1)                                                              # [T, Q, 3n]
    # ln(1 - exp(-x)), accurate at both ends: 1 - exp(-x) rounds to 1 for large x, and cancels for small x
    log_term = torch.where(x > 0.5, torch.log1p(-torch.exp(-x)), torch.log(-torch.expm1(-x)))
    F = zpe + kT * (w * log_term).sum(dim=(1, 2))
    S = KB * (w * (x / torch.expm1(x) - log_term)).sum(dim=(1, 2))
    half = 0.5 * x
    Cv = KB * (w * (half / torch.sinh(half)) ** 2).sum(dim=(1, 2))
    zero = torch.zeros_like(T)
    return PhononThermodynamics(T, zpe, torch.where(hot, F, zpe.expand_as(T)), torch.where(hot, S, zero),
                                torch.where(hot, Cv, zero), int((~real).sum()))
