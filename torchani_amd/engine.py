"""Tensor-level front-end of the C ABI: torch tensors in, torch tensors out, current HIP stream.

PyTorch is used here only as plumbing (device memory, streams); all arithmetic of the hot path happens
inside libanihip.so.  Every function requires CUDA(ROCm) tensors and raises otherwise -- there is no
eager/CPU fallback on purpose.
"""
from __future__ import annotations

import ctypes as C
import typing as tp

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .constants import AEVConstants


def _ptr(t: tp.Optional[Tensor]) -> tp.Optional[int]:
    return None if t is None else t.data_ptr()


def _row_ptr(t: Tensor, row_offset: int, row_len: int) -> int:
    """Base pointer of a [*, row_len] fp32 buffer whose first row is atom ``row_offset``: the C ABI indexes
    rows by absolute atom index but only touches the central range, so a rank can keep buffers of its shard
    alone (the shifted base is never dereferenced outside the shard's rows)."""
    return t.data_ptr() - 4 * row_offset * row_len


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _require_cuda(*ts: tp.Optional[Tensor]) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            # same error class as the reference for non-CUDA input to the native path
            # (aev/_computer.py:444-447)
            raise ValueError("torchani_amd's HIP engine needs tensors on a ROCm device (no CPU fallback)")


class NeighborRows(tp.NamedTuple):
    """Fixed-capacity, species-sorted full neighbor rows (format: include/anihip.h)."""

    meta: Tensor      # [N, 6] int32 (uint32 words)
    ent: Tensor       # [(hi-lo) * row_cap, 4] float32
    status: Tensor    # [8] int32
    row_cap: int
    lo: int
    hi: int
    symmetric: bool = True   # j in row i <=> i in row j (false for LAMMPS full lists with ghost atoms)

    def overflowed(self) -> bool:
        """Synchronising read of the device-side status word: did any row exceed its capacity (and was zeroed)?"""
        return bool(int(self.status[0].item()) & (_lib.ST_ROW_OVERFLOW | _lib.ST_ENTRY_OVERFLOW))

    def raise_on_overflow(self) -> None:
        """Synchronising check of the device-side status words."""
        st = int(self.status[0].item())
        if st & (_lib.ST_ROW_OVERFLOW | _lib.ST_ENTRY_OVERFLOW):
            raise RuntimeError(
                f"neighbor row overflow (status={st}): an atom has more than row_capacity={self.row_cap} "
                f"neighbors within the radial cutoff, > {_lib.MAX_ANG} within the angular cutoff or > 255 of "
                "one species; raise row_capacity (max 256)")


def rows_to_half(nbrs: NeighborRows, n_atoms: int) -> tp.Tuple[Tensor, Tensor, Tensor]:
    """Neighbor rows -> the reference's half list (indices [2, P] int64, distances [P], diff_vectors [P, 3] = r_i - r_j
    (+ shift)): what ``torch.ops.cell_list.cell_list`` / ``FastCellList`` return (csrc/cell_list.cpp:342-354,
    neighbors.py:285-294).  anihip_nbr_rows_to_half, two calls: count, then write (one host sync for P)."""
    L = _lib.lib()
    dev = nbrs.meta.device
    ws = torch.empty(L.anihip_nbr_rows_to_half_workspace_bytes(nbrs.hi - nbrs.lo), dtype=torch.uint8, device=dev)
    npairs = torch.zeros(1, dtype=torch.int64, device=dev)
    args = (_stream(), n_atoms, nbrs.lo, nbrs.hi, _ptr(nbrs.meta), _ptr(nbrs.ent), _ptr(ws), ws.numel())
    _lib.check(L.anihip_nbr_rows_to_half(*args, 0, None, None, None, _ptr(npairs)))
    P = int(npairs.item())
    idx = torch.empty((2, P), dtype=torch.int64, device=dev)
    dist = torch.empty(P, dtype=torch.float32, device=dev)
    diff = torch.empty((P, 3), dtype=torch.float32, device=dev)
    if P:
        _lib.check(L.anihip_nbr_rows_to_half(*args, P, _ptr(idx), _ptr(dist), _ptr(diff), _ptr(npairs)))
    return idx, dist, diff


class SparsePattern(tp.NamedTuple):
    """Structure of a block-sparse Hessian over the rows of a call (hessian_pattern): R(a) = {a} U row(a) as CSR
    (roff [N + 1] int64, rlist int32), the block pattern P(a) = U_{i in R(a)} R(i) by columns (poff [N + 1] int64, index
    int64 [2, nnz]: the entries of column a are poff[a] .. poff[a + 1], rows ascending) and host copies of the offsets."""

    roff: Tensor
    rlist: Tensor
    poff: Tensor
    index: Tensor
    roff_host: np.ndarray
    poff_host: np.ndarray

    @property
    def nnz(self) -> int:
        return int(self.poff_host[-1])


def _exclusive_scan(counts: Tensor) -> Tensor:
    out = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=counts.device)
    torch.cumsum(counts, 0, out=out[1:])
    return out


def hessian_pattern(species: Tensor, nbrs: NeighborRows) -> SparsePattern:
    """R lists and block pattern of the flattened atoms (anihip_hess_sparse_rlist, anihip_hess_sparse_pattern; two calls
    each, count then fill; two host syncs).  Symmetric rows only."""
    _require_cuda(species)
    if not nbrs.symmetric:
        raise NotImplementedError("sparse Hessians need symmetric neighbor rows (the library's own builders)")
    L = _lib.lib()
    n = species.numel()
    dev = species.device
    rcnt = torch.empty(n, dtype=torch.int32, device=dev)
    _lib.check(L.anihip_hess_sparse_rlist(_stream(), n, _ptr(species), _ptr(nbrs.meta), _ptr(nbrs.ent), None, _ptr(rcnt),
                                          None))
    roff = _exclusive_scan(rcnt)
    roff_host = roff.cpu().numpy()
    rlist = torch.empty(max(int(roff_host[-1]), 1), dtype=torch.int32, device=dev)
    _lib.check(L.anihip_hess_sparse_rlist(_stream(), n, _ptr(species), _ptr(nbrs.meta), _ptr(nbrs.ent), _ptr(roff), None,
                                          _ptr(rlist)))
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    pcnt = torch.empty(n, dtype=torch.int32, device=dev)
    _lib.check(L.anihip_hess_sparse_pattern(_stream(), n, _ptr(roff), _ptr(rlist), None, 0, _ptr(pcnt), None,
                                            _ptr(status)))
    poff = _exclusive_scan(pcnt)
    poff_host = poff.cpu().numpy()
    if int(status.item()):
        raise RuntimeError("sparse Hessian pattern: an atom couples to more than 4096 atoms")
    nnz = int(poff_host[-1])
    index = torch.empty((2, nnz), dtype=torch.int64, device=dev)
    if nnz:
        _lib.check(L.anihip_hess_sparse_pattern(_stream(), n, _ptr(roff), _ptr(rlist), _ptr(poff), nnz, None,
                                                _ptr(index), _ptr(status)))
    return SparsePattern(roff, rlist, poff, index, roff_host, poff_host)


def hessian_items(species: Tensor, pat: SparsePattern, num_species: int, n0: int, n1: int) -> tp.Tuple[Tensor, Tensor]:
    """(row_atom, row_dir) int32 [3 sum_{n0 <= a < n1} |R(a)|]: the item rows of the direction atoms n0 .. n1, the rows of a
    species contiguous (anihip_hess_sparse_items)."""
    dev = species.device
    n_rows = 3 * int(pat.roff_host[n1] - pat.roff_host[n0])
    row_atom = torch.empty(max(n_rows, 1), dtype=torch.int32, device=dev)
    row_dir = torch.empty(max(n_rows, 1), dtype=torch.int32, device=dev)
    scratch = torch.empty(num_species * (n1 - n0) + 1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().anihip_hess_sparse_items(_stream(), num_species, n0, n1, _ptr(species), _ptr(pat.roff),
                                                   _ptr(pat.rlist), _ptr(scratch), _ptr(row_atom), _ptr(row_dir)))
    return row_atom[:n_rows], row_dir[:n_rows]


def hessian_extract(pat: SparsePattern, n0: int, n1: int, scratch: Tensor, blocks: Tensor) -> None:
    """blocks of the columns of the direction atoms n0 .. n1 out of scratch [K, N, 3] (slab 3 a + c - 3 n0 = column (a, c)),
    writing zeros back to exactly the positions read (anihip_hess_sparse_extract)."""
    n = scratch.shape[1]
    _lib.check(_lib.lib().anihip_hess_sparse_extract(
        _stream(), n, int(pat.poff_host[n0]), int(pat.poff_host[n1]), _ptr(pat.index), pat.nnz, 3 * n0, scratch.shape[0],
        _ptr(scratch), _ptr(blocks)))


class BlockOperator(tp.NamedTuple):
    """The mass-weighted, symmetrized operator A = M^-1/2 ((H + H^T) / 2) M^-1/2 of a BlockHessian in the layout of
    anihip_block_hessian_spmm (block_hessian_prepare): column offsets coff [N + 1] int64, rows int32 [nnz], the transpose
    partner of each entry int64 [nnz], ablocks fp32 [nnz, 3, 3] (entry p = (row j, column a) holds A_ja), the entry of each
    atom's diagonal block diag int64 [N] (-1: padding) and the per-atom Gershgorin row-sum bound gersh fp64 [N]."""

    coff: Tensor
    rows: Tensor
    partner: Tensor
    ablocks: Tensor
    diag: Tensor
    gersh: Tensor

    @property
    def n_atoms(self) -> int:
        return int(self.diag.numel())


def block_hessian_prepare(index: Tensor, blocks: Tensor, masses: Tensor) -> BlockOperator:
    """anihip_block_hessian_prepare over a column-sorted index int64 [2, nnz], blocks fp32 [nnz, 3, 3] and masses [N] (amu);
    one host sync for the status word.  Raises ValueError for an index out of range or not sorted by columns, a block whose
    transpose is missing, or an atom with blocks but no diagonal block."""
    _require_cuda(index, blocks, masses)
    dev = blocks.device
    n = masses.numel()
    nnz = int(index.shape[1])
    index = index.to(torch.int64).contiguous()
    blocks = blocks.to(torch.float32).contiguous()
    masses = masses.to(torch.float64).contiguous()
    coff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    rows = torch.empty(nnz, dtype=torch.int32, device=dev)
    partner = torch.empty(nnz, dtype=torch.int64, device=dev)
    ablocks = torch.empty((nnz, 3, 3), dtype=torch.float32, device=dev)
    diag = torch.empty(n, dtype=torch.int64, device=dev)
    gersh = torch.empty(n, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().anihip_block_hessian_prepare(
        _stream(), n, nnz, _ptr(index), _ptr(blocks), _ptr(masses), _ptr(coff), _ptr(rows), _ptr(partner), _ptr(ablocks),
        _ptr(gersh), _ptr(diag), _ptr(status)))
    st = int(status.item())
    if st & _lib.BLOCK_HESSIAN_BAD_INDEX:
        raise ValueError("BlockHessian index out of range or not sorted by columns")
    if st & _lib.BLOCK_HESSIAN_NO_PARTNER:
        raise ValueError("BlockHessian pattern is not symmetric: a block (i, j) is stored without (j, i)")
    if st & _lib.BLOCK_HESSIAN_NO_DIAGONAL:
        raise ValueError("BlockHessian has an atom with off-diagonal blocks but no diagonal block")
    return BlockOperator(coff, rows, partner, ablocks, diag, gersh)


def block_hessian_spmm(op: BlockOperator, x: Tensor, out: tp.Optional[Tensor] = None) -> Tensor:
    """Y = A X (anihip_block_hessian_spmm) for X fp32 [N, 3, m] (or any shape of N * 3 * m elements, vector index fastest),
    1 <= m <= 64; Y has X's shape."""
    _require_cuda(x)
    n = op.n_atoms
    if x.dtype != torch.float32 or not x.is_contiguous() or x.numel() % (3 * max(n, 1)):
        raise ValueError(f"x must be contiguous float32 of N * 3 * m elements (N = {n})")
    m = x.numel() // (3 * n) if n else 1
    if not 1 <= m <= _lib.BLOCK_HESSIAN_MAX_VECTORS:
        raise ValueError(f"anihip_block_hessian_spmm takes 1 .. {_lib.BLOCK_HESSIAN_MAX_VECTORS} vectors, got {m}")
    y = torch.empty_like(x) if out is None else out
    _lib.check(_lib.lib().anihip_block_hessian_spmm(_stream(), n, m, _ptr(op.coff), _ptr(op.rows), _ptr(op.ablocks), _ptr(x),
                                                    _ptr(y)))
    return y


def phonon_fold(op: BlockOperator, n_basis: int, repeats: tp.Sequence[int], ent_b: Tensor, ent_j: Tensor,
                boff: tp.Optional[Tensor] = None, diag_entry: tp.Optional[Tensor] = None) -> tp.Tuple[Tensor, Tensor, Tensor]:
    """anihip_phonon_fold: (phi fp64 [m, 3, 3], missing int32 [m], defect fp64 [m]) of the compact entries (ent_b, ent_j)
    int32 [m] over the unit-mass operator of a supercell of repeats copies of n_basis atoms.  boff int32 [n_basis + 1] and
    diag_entry int32 [n_basis] impose the acoustic sum rule."""
    _require_cuda(op.coff, op.rows, op.ablocks, ent_b, ent_j, boff, diag_entry)
    r1, r2, r3 = (int(r) for r in repeats)
    m = int(ent_b.numel())
    if op.n_atoms != n_basis * r1 * r2 * r3 or int(ent_j.numel()) != m:
        raise ValueError("the operator does not belong to this supercell, or ent_b and ent_j differ in length")
    for t in (ent_b, ent_j, boff, diag_entry):
        if t is not None and (t.dtype != torch.int32 or not t.is_contiguous()):
            raise ValueError("the compact pattern must be contiguous int32 tensors")
    dev = op.ablocks.device
    phi = torch.empty((m, 3, 3), dtype=torch.float64, device=dev)
    missing = torch.empty(m, dtype=torch.int32, device=dev)
    defect = torch.empty(m, dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().anihip_phonon_fold(_stream(), n_basis, r1, r2, r3, _ptr(op.coff), _ptr(op.rows), _ptr(op.ablocks), m,
                                             _ptr(ent_b), _ptr(ent_j), _ptr(boff), _ptr(diag_entry), _ptr(phi), _ptr(missing),
                                             _ptr(defect)))
    return phi, missing, defect


def phonon_dynmat(n_basis: int, poff: Tensor, nvec: Tensor, phi: Tensor, rvec: Tensor, masses: Tensor, q: Tensor,
                  derivatives: bool = False) -> tp.Tuple[Tensor, tp.Optional[Tensor]]:
    """anihip_phonon_dynmat: D complex128 [Q, 3n, 3n] (a view of the interleaved fp64 output, no copy) and, with derivatives,
    dD / dk complex128 [Q, 3, 3n, 3n] for q fp64 [Q, 3]."""
    _require_cuda(poff, nvec, phi, rvec, masses, q)
    Q, d = int(q.shape[0]), 3 * n_basis
    for t, dt in ((poff, torch.int32), (nvec, torch.int32), (phi, torch.float64), (rvec, torch.float64),
                  (masses, torch.float64), (q, torch.float64)):
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError("anihip_phonon_dynmat takes contiguous int32 patterns and float64 values")
    dmat = torch.empty((Q, d, d, 2), dtype=torch.float64, device=q.device)
    dder = torch.empty((Q, 3, d, d, 2), dtype=torch.float64, device=q.device) if derivatives else None
    _lib.check(_lib.lib().anihip_phonon_dynmat(_stream(), n_basis, Q, _ptr(poff), _ptr(nvec), _ptr(phi), _ptr(rvec),
                                               _ptr(masses), _ptr(q), _ptr(dmat), _ptr(dder)))
    return torch.view_as_complex(dmat), (None if dder is None else torch.view_as_complex(dder))


def phonon_dos(freqs: Tensor, weights: Tensor, f_first: float, df: float, sigma: float, bins: int) -> Tensor:
    """anihip_phonon_dos: fp64 [bins], sum_i weights[i] G_sigma(f_first + k df - freqs[i]) for freqs, weights fp64 [M]."""
    _require_cuda(freqs, weights)
    if freqs.dtype != torch.float64 or weights.dtype != torch.float64 or freqs.shape != weights.shape:
        raise ValueError("freqs and weights must be float64 tensors of one shape")
    freqs, weights = freqs.contiguous(), weights.contiguous()
    out = torch.empty(int(bins), dtype=torch.float64, device=freqs.device)
    _lib.check(_lib.lib().anihip_phonon_dos(_stream(), freqs.numel(), _ptr(freqs), _ptr(weights), float(f_first), float(df),
                                            float(sigma), int(bins), _ptr(out)))
    return out


class AevEngine:
    """Neighbor rows + AEV forward/backward for one set of AEV constants."""

    def __init__(self, consts: AEVConstants) -> None:
        self.consts = consts
        p = _lib.AevParams()
        p.num_species = consts.num_species
        p.n_shf_r, p.n_shf_a, p.n_shf_z = len(consts.ShfR), len(consts.ShfA), len(consts.ShfZ)
        p.Rcr, p.Rca = consts.Rcr, consts.Rca
        p.EtaR, p.EtaA, p.Zeta = consts.EtaR, consts.EtaA, consts.Zeta
        if consts.cutoff_fn not in _lib.CUTOFF_KINDS:
            raise ValueError(f"Unsupported cutoff function {consts.cutoff_fn!r}: the HIP kernels have "
                             f"{sorted(_lib.CUTOFF_KINDS)}")
        p.cutoff_kind = _lib.CUTOFF_KINDS[consts.cutoff_fn]
        if not (1 <= p.n_shf_r <= 32 and 1 <= p.n_shf_a <= 16 and 1 <= p.n_shf_z <= 16 and 1 <= p.num_species <= 7):
            raise ValueError(
                "HIP AEV kernels support up to 32 radial shifts, angular grids up to 16 x 16 and up to 7 species; "
                f"got nR={p.n_shf_r}, nA x nZ={p.n_shf_a}x{p.n_shf_z}, S={p.num_species}")
        # the published grids (16 radial shifts, 8x4 = ANI-2x or 4x8 = ANI-1x angular terms) run through the tuned kernels
        # with slab masks and the forward-mode derivative; any other grid through the general kernels (csrc/aev_generic.hip)
        self.tuned = p.n_shf_r == 16 and (p.n_shf_a, p.n_shf_z) in ((8, 4), (4, 8))
        self.params = p
        self.L = consts.out_dim
        self._host_table: tp.Optional[np.ndarray] = None
        self._tables: tp.Dict[torch.device, Tensor] = {}

    def host_table(self) -> np.ndarray:
        if self._host_table is None:
            c = self.consts
            shfr = np.asarray(c.ShfR, dtype=np.float32)
            shfa = np.asarray(c.ShfA, dtype=np.float32)
            shfz = np.asarray(c.ShfZ, dtype=np.float32)
            out = np.zeros(_lib.TABLE_FLOATS, dtype=np.float32)
            _lib.check(_lib.lib().anihip_aev_table_pack(
                C.byref(self.params), shfr.ctypes.data, shfa.ctypes.data, shfz.ctypes.data, out.ctypes.data))
            self._host_table = out
        return self._host_table

    def table(self, device: torch.device) -> Tensor:
        t = self._tables.get(device)
        if t is None:
            t = torch.from_numpy(self.host_table()).to(device)
            self._tables[device] = t
        return t

    # ---- neighbor rows ----------------------------------------------------------------------------
    def neighbors(self, species: Tensor, coords: Tensor, cell: tp.Optional[Tensor] = None,
                  pbc: tp.Optional[tp.Sequence[bool]] = None, lo: int = 0, hi: tp.Optional[int] = None,
                  mode: str = "auto", row_cap: int = 128, max_cells: tp.Optional[int] = None) -> NeighborRows:
        """species [C,A] int32, coords [C,A,3] float32 (contiguous).  mode: batch | cell | auto."""
        _require_cuda(species, coords, cell)
        assert species.dtype == torch.int32 and coords.dtype == torch.float32
        assert species.is_contiguous() and coords.is_contiguous()
        Cn, A = species.shape
        n = Cn * A
        hi = n if hi is None else hi
        dev = coords.device
        pbc_mask = 0
        cell_t = None
        if cell is not None and pbc is not None and any(bool(b) for b in pbc):
            cell_t = cell.detach().to(device=dev, dtype=torch.float32).contiguous()
            pbc_mask = sum((1 << k) for k in range(3) if bool(pbc[k]))
        if mode == "auto":
            # the reference switches from all-pairs to the cell list at 190 (pbc) / 1770 atoms
            # (neighbors.py:324); a wave sweeps 64 candidates at a time so the crossover is later here
            mode = "cell" if (Cn == 1 and A > 512) else "batch"
        if mode == "cell" and Cn != 1:
            raise ValueError("the cell-list builder handles one system at a time (neighbors.py:373-381)")
        row_cap = int(min(max(row_cap, 1), _lib.MAX_RAD))
        n_central = max(hi - lo, 0)
        meta = torch.empty((n, _lib.META_WORDS), dtype=torch.int32, device=dev)
        ent = torch.empty((max(n_central, 1) * row_cap, 4), dtype=torch.float32, device=dev)
        # (the two builders reset the status words in their first kernel, include/anihip.h; an empty range returns early)
        status = (torch.empty if n_central > 0 else torch.zeros)(_lib.STATUS_WORDS, dtype=torch.int32, device=dev)
        L = _lib.lib()
        if mode == "batch":
            ws = torch.empty(L.anihip_nbr_workspace_bytes(n, 1), dtype=torch.uint8, device=dev)
            _lib.check(L.anihip_nbr_build_batch(
                _stream(), C.byref(self.params), Cn, A, _ptr(species), _ptr(coords), _ptr(cell_t), pbc_mask,
                lo, hi, _ptr(ws), ws.numel(), _ptr(meta), _ptr(ent), n_central * row_cap, _ptr(status)))
        elif mode == "cell":
            if max_cells is None:
                max_cells = max(4096, 2 * n)
            ws = torch.empty(L.anihip_nbr_workspace_bytes(n, max_cells), dtype=torch.uint8, device=dev)
            _lib.check(L.anihip_nbr_build_cell(
                _stream(), C.byref(self.params), n, _ptr(species), _ptr(coords), _ptr(cell_t), pbc_mask, lo,
                hi, max_cells, _ptr(ws), ws.numel(), _ptr(meta), _ptr(ent), n_central * row_cap,
                _ptr(status)))
        else:
            raise ValueError(f"unknown neighbor mode {mode!r}")
        return NeighborRows(meta, ent, status, row_cap, lo, hi)

    def rows_from_half(self, species: Tensor, indices: Tensor, diff_vectors: Tensor, lo: int = 0,
                       hi: tp.Optional[int] = None, row_cap: int = 128) -> NeighborRows:
        """Neighbor rows from an external half list: indices [2, P] int64 (flattened atom indices),
        diff_vectors [P, 3] = r[indices[0]] - r[indices[1]] (+ image shift), neighbors.py:22-29,105-112."""
        _require_cuda(species, indices, diff_vectors)
        assert species.dtype == torch.int32 and species.is_contiguous()
        n = species.numel()
        hi = n if hi is None else hi
        dev = species.device
        idx = indices.to(torch.int64).contiguous()
        diff = diff_vectors.detach().to(torch.float32).contiguous()
        assert idx.dim() == 2 and idx.shape[0] == 2 and diff.shape == (idx.shape[1], 3)
        row_cap = int(min(max(row_cap, 1), _lib.MAX_RAD))
        n_central = max(hi - lo, 0)
        meta = torch.empty((n, _lib.META_WORDS), dtype=torch.int32, device=dev)
        ent = torch.empty((max(n_central, 1) * row_cap, 4), dtype=torch.float32, device=dev)
        status = torch.zeros(_lib.STATUS_WORDS, dtype=torch.int32, device=dev)
        L = _lib.lib()
        ws = torch.empty(L.anihip_nbr_half_workspace_bytes(n_central), dtype=torch.uint8, device=dev)
        _lib.check(L.anihip_nbr_from_half(
            _stream(), C.byref(self.params), n, _ptr(species), idx.shape[1], _ptr(idx), _ptr(diff), lo, hi,
            _ptr(ws), ws.numel(), _ptr(meta), _ptr(ent), n_central * row_cap, _ptr(status)))
        return NeighborRows(meta, ent, status, row_cap, lo, hi)

    def rows_from_full(self, species: Tensor, coords: Tensor, ilist_unique: Tensor, jlist: Tensor,
                       numneigh: Tensor, row_cap: int = 128) -> NeighborRows:
        """Neighbor rows from a LAMMPS-style full list (aev/_computer.py:420-438): species [1, A] int32, coords
        [1, A, 3] float32 incl. ghost atoms; listed atom ilist_unique[g] has numneigh[g] consecutive jlist
        entries."""
        _require_cuda(species, coords, ilist_unique, jlist, numneigh)
        assert species.dtype == torch.int32 and coords.dtype == torch.float32
        assert species.is_contiguous() and coords.is_contiguous()
        n = species.numel()
        dev = coords.device
        il = ilist_unique.to(torch.int32).contiguous()
        jl = jlist.to(torch.int32).contiguous()
        nn = numneigh.to(torch.int32).contiguous()
        start = (torch.cumsum(nn.to(torch.int64), 0) - nn.to(torch.int64)).contiguous()
        row_cap = int(min(max(row_cap, 1), _lib.MAX_RAD))
        meta = torch.empty((n, _lib.META_WORDS), dtype=torch.int32, device=dev)
        ent = torch.empty((n * row_cap, 4), dtype=torch.float32, device=dev)
        status = torch.zeros(_lib.STATUS_WORDS, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().anihip_nbr_from_full(
            _stream(), C.byref(self.params), n, _ptr(species), _ptr(coords), il.numel(), _ptr(il), _ptr(nn),
            _ptr(start), _ptr(jl), _ptr(meta), _ptr(ent), n * row_cap, _ptr(status)))
        return NeighborRows(meta, ent, status, row_cap, 0, n, symmetric=False)

    def refresh_rows(self, species: Tensor, coords: Tensor, coords_build: Tensor, verlet: NeighborRows,
                     lo: int = 0, hi: tp.Optional[int] = None, row_cap: int = 128) -> NeighborRows:
        """Rows for the current coordinates from rows built at coords_build with cutoff Rcr + skin
        (anihip_nbr_refresh): no pair search, valid while no atom moved more than skin / 2."""
        _require_cuda(species, coords, coords_build)
        assert coords.dtype == torch.float32 and coords.is_contiguous() and coords_build.is_contiguous()
        n = species.numel()
        hi = n if hi is None else hi
        assert verlet.lo <= lo and hi <= verlet.hi and verlet.lo == 0, "Verlet rows must cover the central range"
        row_cap = int(min(max(row_cap, 1), _lib.MAX_RAD))
        n_central = max(hi - lo, 0)
        dev = coords.device
        meta = torch.empty((n, _lib.META_WORDS), dtype=torch.int32, device=dev)
        ent = torch.empty((max(n_central, 1) * row_cap, 4), dtype=torch.float32, device=dev)
        status = torch.zeros(_lib.STATUS_WORDS, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().anihip_nbr_refresh(
            _stream(), C.byref(self.params), n, lo, hi, _ptr(species), _ptr(coords), _ptr(coords_build),
            _ptr(verlet.meta), _ptr(verlet.ent), _ptr(meta), _ptr(ent), n_central * row_cap, _ptr(status)))
        return NeighborRows(meta, ent, status, row_cap, lo, hi)

    # ---- AEV ----------------------------------------------------------------------------------------
    @property
    def n_slabs(self) -> int:
        """Number of 32-wide slabs of an AEV row in slab order (include/anihip.h)."""
        if not self.tuned:
            return -(-self.L // 32)   # (a general grid: plain 32-column slabs of the row)
        S = self.params.num_species
        return (S + 1) // 2 + S * (S + 1) // 2

    def forward(self, species: Tensor, nbrs: NeighborRows, out: tp.Optional[Tensor] = None,
                slab_mask: tp.Optional[Tensor] = None, shard_rows: bool = False) -> Tensor:
        """AEV rows [N, L] for the central atoms nbrs.lo..nbrs.hi (other rows are left untouched).
        slab_mask (optional int32 [N], written for the same atoms): flags of the slabs of each row that are
        not identically zero, consumed by PackedNetworks.forward_backward.
        shard_rows=True: the result holds only the rows lo..hi ([hi - lo, L], row 0 = atom lo)."""
        _require_cuda(species, slab_mask)
        n = species.numel()
        rows0 = nbrs.lo if shard_rows else 0
        if out is None:
            if shard_rows:
                out = torch.empty((nbrs.hi - nbrs.lo, self.L), dtype=torch.float32, device=species.device)
            else:
                alloc = torch.empty if (nbrs.lo == 0 and nbrs.hi == n) else torch.zeros
                out = alloc((n, self.L), dtype=torch.float32, device=species.device)
        assert out.dtype == torch.float32 and out.is_contiguous()
        assert out.numel() == ((nbrs.hi - nbrs.lo) if shard_rows else n) * self.L
        if slab_mask is not None:
            assert slab_mask.dtype == torch.int32 and slab_mask.numel() == n and slab_mask.is_contiguous()
        _lib.check(_lib.lib().anihip_aev_forward(
            _stream(), C.byref(self.params), _ptr(self.table(species.device)), n, nbrs.lo, nbrs.hi,
            _ptr(species), _ptr(nbrs.meta), _ptr(nbrs.ent), _row_ptr(out, rows0, self.L), _ptr(slab_mask),
            _ptr(nbrs.status)))
        return out

    def forward_update(self, species: Tensor, nbrs: NeighborRows, shard_rows: bool = True) -> tp.Tuple[Tensor, Tensor]:
        """(AEV rows, slab flags) for the central atoms of nbrs in buffers the engine KEEPS between calls and updates in
        place (anihip_aev_forward_update): a row is zero outside its flagged slabs, and those zeros are written once -- a
        later call only touches the slabs that were or are flagged (0.6 KB instead of 4 KB per water atom and step).  The
        pair is valid until the next call of this method; one pair is kept (same number of atoms and central range, else a
        fresh one).  For the hot loop of energies_and_forces; ``forward`` hands out buffers of the caller's own."""
        _require_cuda(species)
        n = species.numel()
        rows = (nbrs.hi - nbrs.lo) if shard_rows else n
        # (the stream is part of the key: the kept pair is ordered by the stream that updates it, another stream gets its own)
        key = (n, nbrs.lo, nbrs.hi, rows, species.device, _stream())
        hit = self.__dict__.get("_rows_kept")
        if hit is None or hit[0] != key:
            self.__dict__["_rows_kept"] = None   # (release the old pair before the new one is allocated)
            # (two flag buffers, alternating: the kernel reads the previous call's and writes this call's)
            hit = [key, torch.zeros((rows, self.L), dtype=torch.float32, device=species.device),
                   torch.zeros(n, dtype=torch.int32, device=species.device),
                   torch.zeros(n, dtype=torch.int32, device=species.device)]
            self.__dict__["_rows_kept"] = hit
        _, out, prev, mask = hit
        _lib.check(_lib.lib().anihip_aev_forward_update(
            _stream(), C.byref(self.params), _ptr(self.table(species.device)), n, nbrs.lo, nbrs.hi,
            _ptr(species), _ptr(nbrs.meta), _ptr(nbrs.ent), _row_ptr(out, nbrs.lo if shard_rows else 0, self.L),
            _ptr(prev), _ptr(mask), _ptr(nbrs.status)))
        hit[2], hit[3] = mask, prev
        return out, mask

    def release_rows(self) -> None:
        """Free the buffers ``forward_update`` keeps (4 KB per central atom + two flag words per atom); the next call
        allocates and fills a fresh pair."""
        self.__dict__["_rows_kept"] = None
        self.__dict__["_rows_seen"] = None

    def rows_wanted(self, n: int, lo: int, hi: int, device: torch.device) -> bool:
        """Policy of the callers that MAY keep rows (models.ANI.energies_and_forces): a kept pair pays off from the second
        consecutive call with the same atom count and central range on -- a call whose sizes differ from the previous call's
        (batched screening, one-off evaluations) works on buffers of its own, pins nothing and memsets nothing."""
        key = (n, lo, hi, device, _stream())
        seen = self.__dict__.get("_rows_seen")
        self.__dict__["_rows_seen"] = key
        if seen != key:
            if self.__dict__.get("_rows_kept") is not None:
                self.__dict__["_rows_kept"] = None   # (sizes changed: the old pair is of no use any more)
            return False
        return True

    def __getstate__(self):
        # kept rows / flags are scratch tied to this object and its stream: never copied or pickled with it
        state = dict(self.__dict__)
        state.pop("_rows_kept", None)
        state.pop("_rows_seen", None)
        return state

    def __deepcopy__(self, memo):
        import copy

        new = object.__new__(type(self))
        memo[id(self)] = new
        for k, v in self.__getstate__().items():
            new.__dict__[k] = copy.deepcopy(v, memo)
        return new

    def jvp(self, species: Tensor, nbrs: NeighborRows, tangent: Tensor) -> Tensor:
        """J t [N, L]: derivative of the AEV rows of nbrs' central atoms along the coordinate direction tangent [N, 3]
        (anihip_aev_jvp; the reference's cuaev double backward)."""
        _require_cuda(species, tangent)
        n = species.numel()
        t = tangent.detach().to(torch.float32).contiguous()
        assert t.numel() == 3 * n
        out = torch.empty((n, self.L), dtype=torch.float32, device=species.device) \
            if (nbrs.lo == 0 and nbrs.hi == n) else torch.zeros((n, self.L), dtype=torch.float32, device=species.device)
        _lib.check(_lib.lib().anihip_aev_jvp(
            _stream(), C.byref(self.params), _ptr(self.table(species.device)), n, nbrs.lo, nbrs.hi, _ptr(species),
            _ptr(nbrs.meta), _ptr(nbrs.ent), _ptr(t), _ptr(out), _ptr(nbrs.status)))
        return out

    def jvp_batched(self, species: Tensor, nbrs: NeighborRows, tangent: Tensor) -> Tensor:
        """J t[k] [K, N, L] for K coordinate directions tangent [K, N, 3] in one launch (anihip_aev_jvp_batched)."""
        _require_cuda(species, tangent)
        n = species.numel()
        t = tangent.detach().to(torch.float32).contiguous()
        K = t.shape[0]
        assert t.numel() == 3 * n * K
        out = torch.zeros((K, n, self.L), dtype=torch.float32, device=species.device)
        _lib.check(_lib.lib().anihip_aev_jvp_batched(
            _stream(), C.byref(self.params), _ptr(self.table(species.device)), n, nbrs.lo, nbrs.hi, _ptr(species),
            _ptr(nbrs.meta), _ptr(nbrs.ent), K, _ptr(t), _ptr(out), _ptr(nbrs.status)))
        return out

    def backward_second(self, species: Tensor, nbrs: NeighborRows, grad_aev: Tensor, tangent: Tensor,
                        dgrad: tp.Optional[Tensor] = None) -> Tensor:
        """out[k] = J^T dgrad[k] + (D_{tangent[k]} J^T) grad_aev  [K, N, 3] (anihip_aev_backward_second): the derivative of
        the backward along K coordinate directions; dgrad None = zeros."""
        _require_cuda(species, grad_aev, tangent, dgrad)
        if not nbrs.symmetric:
            raise NotImplementedError("second derivatives need symmetric neighbor rows (the library's own builders)")
        n = species.numel()
        g = grad_aev.detach().to(torch.float32).contiguous()
        t = tangent.detach().to(torch.float32).contiguous()
        K = t.shape[0]
        assert g.numel() == n * self.L and t.numel() == 3 * n * K
        dg = (torch.zeros((K, n, self.L), dtype=torch.float32, device=species.device) if dgrad is None
              else dgrad.detach().to(torch.float32).contiguous())
        assert dg.numel() == K * n * self.L
        out = torch.zeros((K, n, 3), dtype=torch.float32, device=species.device)
        _lib.check(_lib.lib().anihip_aev_backward_second(
            _stream(), C.byref(self.params), _ptr(self.table(species.device)), n, nbrs.lo, nbrs.hi, _ptr(species),
            _ptr(nbrs.meta), _ptr(nbrs.ent), _ptr(g), K, _ptr(t), _ptr(dg), _ptr(out), _ptr(nbrs.status)))
        return out

    def jvp_items(self, species: Tensor, nbrs: NeighborRows, row_atom: Tensor, row_dir: Tensor) -> Tensor:
        """daev [R, L] over item rows (anihip_aev_jvp_items): row q = d aev_{row_atom[q]} along the unit direction
        row_dir[q] = 3 a + c (component c of flattened atom a)."""
        _require_cuda(species, row_atom, row_dir)
        n = species.numel()
        R = row_atom.numel()
        out = torch.empty((R, self.L), dtype=torch.float32, device=species.device)
        _lib.check(_lib.lib().anihip_aev_jvp_items(
            _stream(), C.byref(self.params), _ptr(self.table(species.device)), n, _ptr(species), _ptr(nbrs.meta),
            _ptr(nbrs.ent), R, _ptr(row_atom), _ptr(row_dir), _ptr(out)))
        return out

    def backward_second_items(self, species: Tensor, nbrs: NeighborRows, grad_aev: Tensor, row_atom: Tensor,
                              row_dir: Tensor, dir0: int, dgrad: Tensor, out: Tensor) -> None:
        """out[row_dir[q] - dir0] += J_i^T dgrad[q] + (D_t J_i^T) grad_aev over item rows (anihip_aev_backward_second_items);
        out [K, N, 3] float32, dgrad [R, L]."""
        _require_cuda(species, grad_aev, row_atom, row_dir, dgrad, out)
        if not nbrs.symmetric:
            raise NotImplementedError("second derivatives need symmetric neighbor rows (the library's own builders)")
        n = species.numel()
        R = row_atom.numel()
        grad_aev = grad_aev.detach().to(torch.float32).contiguous()
        assert grad_aev.numel() == n * self.L
        assert dgrad.dtype == torch.float32 and dgrad.is_contiguous() and dgrad.numel() == R * self.L
        assert out.dtype == torch.float32 and out.is_contiguous() and out.shape[1:] == (n, 3)
        _lib.check(_lib.lib().anihip_aev_backward_second_items(
            _stream(), C.byref(self.params), _ptr(self.table(species.device)), n, _ptr(species), _ptr(nbrs.meta),
            _ptr(nbrs.ent), _ptr(grad_aev), R, _ptr(row_atom), _ptr(row_dir), dir0, out.shape[0], _ptr(dgrad), _ptr(out)))

    def jvp_strain_items(self, species: Tensor, nbrs: NeighborRows, row_atom: Tensor, row_dir: Tensor) -> Tensor:
        """daev [R, L] over strain item rows (anihip_aev_jvp_strain_items): row q = d aev_{row_atom[q]} / d S_ab,
        row_dir[q] = 3 a + b (x -> x S, cell -> cell S)."""
        _require_cuda(species, row_atom, row_dir)
        n = species.numel()
        R = row_atom.numel()
        out = torch.empty((R, self.L), dtype=torch.float32, device=species.device)
        _lib.check(_lib.lib().anihip_aev_jvp_strain_items(
            _stream(), C.byref(self.params), _ptr(self.table(species.device)), n, _ptr(species), _ptr(nbrs.meta),
            _ptr(nbrs.ent), R, _ptr(row_atom), _ptr(row_dir), _ptr(out)))
        return out

    def backward_second_strain_items(self, species: Tensor, nbrs: NeighborRows, grad_aev: Tensor, row_atom: Tensor,
                                     row_dir: Tensor, dgrad: Tensor, out: Tensor, ss: Tensor) -> None:
        """out [9, N, 3] += the strained-frame mixed derivative of the rows' atoms, ss [C, 9, 9] (float64) += their
        strain-strain contraction (anihip_aev_backward_second_strain_items); dgrad [R, L] = H_net J d' of the rows."""
        _require_cuda(species, grad_aev, row_atom, row_dir, dgrad, out, ss)
        if not nbrs.symmetric:
            raise NotImplementedError("second derivatives need symmetric neighbor rows (the library's own builders)")
        n = species.numel()
        R = row_atom.numel()
        grad_aev = grad_aev.detach().to(torch.float32).contiguous()
        assert grad_aev.numel() == n * self.L
        assert dgrad.dtype == torch.float32 and dgrad.is_contiguous() and dgrad.numel() == R * self.L
        assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == (9, n, 3)
        assert ss.dtype == torch.float64 and ss.is_contiguous() and ss.shape[1:] == (9, 9) and n % ss.shape[0] == 0
        _lib.check(_lib.lib().anihip_aev_backward_second_strain_items(
            _stream(), C.byref(self.params), _ptr(self.table(species.device)), n, n // ss.shape[0], _ptr(species),
            _ptr(nbrs.meta), _ptr(nbrs.ent), _ptr(grad_aev), R, _ptr(row_atom), _ptr(row_dir), _ptr(dgrad), _ptr(out),
            _ptr(ss)))

    def backward(self, species: Tensor, nbrs: NeighborRows, grad_aev: Tensor,
                 grad_coords: tp.Optional[Tensor] = None, shard_rows: bool = False,
                 virial: tp.Optional[Tensor] = None, slab_mask: tp.Optional[Tensor] = None,
                 fixed_point: bool = False) -> Tensor:
        """grad_coords [N,3] += d(sum grad_aev*aev)/d coords for the central atoms of nbrs.
        shard_rows=True: grad_aev holds only the rows lo..hi.
        slab_mask (int32 [N], as written by forward): grad_aev is valid only inside the flagged slabs of each row
        (what PackedNetworks.forward_backward leaves behind); None: whole rows are valid.
        virial (optional float64 [3,3], overwritten): sum_ij dE/d d_ij (x) d_ij over those central atoms.
        fixed_point=True: grad_coords is an int64 [N,3] accumulator in units of 2^-32 (ANIHIP_BWD_FIXED_POINT): the sums
        are order-independent, i.e. bit-reproducible; convert with ``fixed_to_float``."""
        _require_cuda(species, grad_aev, slab_mask)
        n = species.numel()
        assert grad_aev.dtype == torch.float32 and grad_aev.is_contiguous()
        assert grad_aev.numel() == ((nbrs.hi - nbrs.lo) if shard_rows else n) * self.L
        if slab_mask is not None:
            assert slab_mask.dtype == torch.int32 and slab_mask.numel() == n and slab_mask.is_contiguous()
        if grad_coords is None:
            grad_coords = torch.zeros((n, 3), dtype=torch.int64 if fixed_point else torch.float32, device=species.device)
        assert grad_coords.dtype == (torch.int64 if fixed_point else torch.float32) and grad_coords.is_contiguous()
        flags = (_lib.BWD_SYMMETRIC if nbrs.symmetric else 0) | (_lib.BWD_FIXED_POINT if fixed_point else 0)
        args = (_stream(), C.byref(self.params), _ptr(self.table(species.device)), n, nbrs.lo, nbrs.hi,
                _ptr(species), _ptr(nbrs.meta), _ptr(nbrs.ent),
                _row_ptr(grad_aev, nbrs.lo if shard_rows else 0, self.L), _ptr(slab_mask), flags,
                _ptr(grad_coords))
        if virial is None:
            _lib.check(_lib.lib().anihip_aev_backward(*args, _ptr(nbrs.status)))
        else:
            _require_cuda(virial)
            assert virial.dtype == torch.float64 and virial.is_contiguous() and virial.numel() == 9
            _lib.check(_lib.lib().anihip_aev_backward_virial(*args, _ptr(virial), _ptr(nbrs.status)))
        return grad_coords

    def backward_flux(self, species: Tensor, nbrs: NeighborRows, grad_aev: Tensor, vectors: Tensor,
                      slab_mask: tp.Optional[Tensor] = None, shard_rows: bool = False) -> Tensor:
        """q [N, 3] (float32): q_i = sum_j d_ij (g_ij . vectors[j]) over the neighbors j of the central atoms of nbrs, with
        g_ij = d(sum grad_aev * aev_i)/d d_ij and d_ij the displacement stored in the row (anihip_aev_backward_flux) -- the
        virial term of the heat flux when ``vectors`` are the velocities.  Rows outside nbrs.lo..nbrs.hi are zero.  Nothing is
        scattered: no global atomics; a fixed order and the same bits run to run on the tuned grids (a general grid adds a row's
        angular terms with LDS float atomics of one wave, whose order was observed to repeat, not guaranteed to).
        shard_rows / slab_mask as for ``backward`` (every term is an own
        term of its row, so the flags, which qualify what is read of other rows, are not needed)."""
        _require_cuda(species, grad_aev, vectors, slab_mask)
        n = species.numel()
        assert grad_aev.dtype == torch.float32 and grad_aev.is_contiguous()
        assert grad_aev.numel() == ((nbrs.hi - nbrs.lo) if shard_rows else n) * self.L
        assert vectors.dtype == torch.float32 and vectors.is_contiguous() and vectors.numel() == 3 * n
        if slab_mask is not None:
            assert slab_mask.dtype == torch.int32 and slab_mask.numel() == n and slab_mask.is_contiguous()
        alloc = torch.empty if (nbrs.lo == 0 and nbrs.hi == n) else torch.zeros
        out = alloc((n, 3), dtype=torch.float32, device=species.device)
        _lib.check(_lib.lib().anihip_aev_backward_flux(
            _stream(), C.byref(self.params), _ptr(self.table(species.device)), n, nbrs.lo, nbrs.hi, _ptr(species),
            _ptr(nbrs.meta), _ptr(nbrs.ent), _row_ptr(grad_aev, nbrs.lo if shard_rows else 0, self.L), _ptr(slab_mask), 0,
            _ptr(vectors), _ptr(out), _ptr(nbrs.status)))
        return out


FIXED_SCALE = 2.0 ** -32


def fixed_to_float(acc: Tensor) -> Tensor:
    """int64 fixed-point accumulators (units of 2^-32) -> float32."""
    return (acc.to(torch.float64) * FIXED_SCALE).to(torch.float32)


def _pad32(x: int) -> int:
    return (x + 31) // 32 * 32


class VerletRows:
    """The reference's VerletCellList (neighbors.py:759-884) as an API-COMPATIBILITY SHIM.  The reference reuses a pair list
    built with cutoff Rcr + skin until an atom has moved skin / 2 because its pair search dominates a step; this engine's
    O(N) cell-list search is 5 % of a step and a refresh of skin rows (read the longer rows back, update, screen, re-sort)
    measured SLOWER than or equal to the plain rebuild at every size from 3 000 to 2.3 M atoms (profiles/r06_md_bench.txt,
    profiles/r05_md_bench.txt: 0.47 / 0.41 ms at 3 k atoms, 0.66 / 0.65 at 12 k, 1.13 / 1.09 at 47 k, 1.83 / 1.74 at 98 k,
    3.55 / 3.46 at 192 k, 13.59 / 13.11 at 786 k).  So ``neighborlist="verlet_cell_list"`` is accepted, gives the same rows
    and results, and by default simply rebuilds every step (``rebuild_above = 0``); the reuse machinery (anihip_nbr_refresh,
    host-synchronising displacement check like the reference's) stays for callers who want the reference's semantics and
    is switched on with ``rebuild_above = float("inf")`` (tests/test_gpu_md.py, tools/md_bench.py --force-verlet)."""

    # systems of at least this many atoms are rebuilt every step (cell mode); 0 = always (see the class docstring)
    rebuild_above = 0

    def __init__(self, skin: float = 1.0) -> None:
        if skin <= 0.0:
            raise ValueError("skin must be a positive float")
        self.skin = float(skin)
        self.reset_cached_values()
        self.n_builds = 0
        self.n_reuses = 0
        self.n_direct = 0   # steps that took the plain pair search (rebuild_above)

    def reset_cached_values(self) -> None:
        self._wide: tp.Optional[AevEngine] = None
        self._rows: tp.Optional[NeighborRows] = None
        self._coords0: tp.Optional[Tensor] = None
        self._cell0: tp.Optional[Tensor] = None
        self._key: tp.Optional[tuple] = None

    def _can_use_prev_list(self, coords: Tensor, cell: tp.Optional[Tensor], key: tuple) -> bool:
        if self._rows is None or self._key != key or self._coords0.shape != coords.shape:
            return False
        if (cell is None) != (self._cell0 is None) or (cell is not None and not torch.equal(cell, self._cell0)):
            return False
        moved2 = (coords - self._coords0).pow(2).sum(-1).max()
        return bool(moved2 < (0.5 * self.skin) ** 2)

    def rows(self, eng: AevEngine, species: Tensor, coords: Tensor, cell: tp.Optional[Tensor], pbc, lo: int, hi: int,
             mode: str, row_cap: int) -> NeighborRows:
        if species.numel() >= self.rebuild_above and mode == "cell":
            self.n_direct += 1
            return eng.neighbors(species, coords, cell, pbc, lo=lo, hi=hi, mode=mode, row_cap=row_cap)
        cell_d = None if cell is None else cell.detach().to(device=coords.device, dtype=torch.float32)
        key = (eng.consts, tuple(species.shape), None if pbc is None else tuple(bool(b) for b in pbc), mode)
        if not self._can_use_prev_list(coords, cell_d, key):
            if self._wide is None or self._key is None or self._key[0] != eng.consts:
                # every stored neighbor in the "far" class: rows may then hold up to 256 entries (include/anihip.h)
                self._wide = AevEngine(eng.consts._replace(Rcr=eng.consts.Rcr + self.skin, Rca=1e-3))
            self._rows = self._wide.neighbors(species, coords, cell, pbc, lo=0, hi=species.numel(), mode=mode,
                                              row_cap=_lib.MAX_RAD)
            self._coords0 = coords.clone()
            self._cell0 = None if cell_d is None else cell_d.clone()
            self._key = key
            self.n_builds += 1
        else:
            self.n_reuses += 1
        out = eng.refresh_rows(species, coords, self._coords0, self._rows, lo, hi, row_cap)
        # a Verlet row that overflowed would silently lose neighbors: surface it in the refreshed rows' status
        out.status.bitwise_or_(self._rows.status & (_lib.ST_ROW_OVERFLOW | _lib.ST_ENTRY_OVERFLOW))
        return out


_N_CUS: tp.Dict[int, int] = {}


def _n_cus(dev: torch.device) -> int:
    i = dev.index if dev.index is not None else torch.cuda.current_device()
    if i not in _N_CUS:
        _N_CUS[i] = int(torch.cuda.get_device_properties(i).multi_processor_count)
    return _N_CUS[i]


def species_column_map(num_species: int, radial_len: int, aev_len: int, order: tp.Sequence[int]) -> np.ndarray:
    """AEV column of the reference layout (aev/_computer.py: radial blocks by species, angular blocks by the triu index of
    the species pair) for every column of the SAME layout written with the species relabelled ``new = order.index(old)``:
    ``aev_relabelled[:, c] == aev_reference[:, map[c]]``.  Used to permute the input rows of the layer-0 weights when the
    engine numbers the species of a system "present ones first" (models.ANI.compact_species)."""
    S = num_species
    nr, pairs = radial_len // S, S * (S + 1) // 2
    nb = (aev_len - radial_len) // pairs
    assert nr * S == radial_len and radial_len + nb * pairs == aev_len and sorted(order) == list(range(S))

    def triu(a: int, b: int) -> int:   # index of the pair (a <= b) in row-major upper-triangular order
        return a * S - (a * (a - 1)) // 2 + (b - a)

    out = np.empty(aev_len, dtype=np.int64)
    for s_new in range(S):
        out[s_new * nr:(s_new + 1) * nr] = order[s_new] * nr + np.arange(nr)
    for a in range(S):
        for b in range(a, S):
            oa, ob = sorted((order[a], order[b]))
            out[radial_len + triu(a, b) * nb:radial_len + (triu(a, b) + 1) * nb] = radial_len + triu(oa, ob) * nb + np.arange(nb)
    return out


class PackedNetworks:
    """Ensemble parameters in the MFMA-friendly layout of include/anihip.h (members concatenated, widths
    padded to 32, transposed copies for the backward GEMMs); cf. BmmAtomicNetwork, nn/_infer.py:141-161."""

    # anihip_mlp_desc.flags (_lib.MLP_FLAG_*) of forward_backward: ``flags`` of an instance, else this class default
    # (0 = the library chooses from the problem size).  The library itself reads no environment variables.
    default_flags: int = 0
    flags: tp.Optional[int] = None
    pinned: int = 0   # live HIP graphs that captured this object's buffers (GraphedEnergiesForces)

    def __init__(self, weights: tp.Sequence[tp.Sequence[tp.Sequence[Tensor]]],
                 biases: tp.Sequence[tp.Sequence[tp.Sequence[Tensor]]], aev_len: int, celu_alpha: float,
                 device: torch.device, precision: str = "f16x3", radial_len: tp.Optional[int] = None,
                 activation: str = "celu") -> None:
        """weights[m][s][l]: [out, in] (torch.nn.Linear layout) of member m, species s, layer l.

        radial_len: length R of the radial part of the AEV; the layer-0 fp16 planes are then stored in slab
        order (include/anihip.h) so that forward_backward can skip all-zero AEV blocks given slab masks.
        Default: 16 S when aev_len has the ANI form 16 S + 32 S(S+1)/2, else plain order.

        precision: "fp32" (exact fp32 MFMA) or "f16x3" (split-fp16 three-product MFMA, ~4e-7 relative
        error per product, see include/anihip.h)."""
        if precision not in ("fp32", "f16x3"):
            raise ValueError(f"unknown MLP precision {precision!r}")
        if activation not in ("celu", "gelu"):
            raise ValueError(f"unknown activation {activation!r}: the network kernels have celu and gelu")
        # (GELU: inference runs through the fused f16x3 kernel only -- anihip_mlp_forward_backward refuses an fp32 GELU pack --;
        # an fp32 GELU pack serves the TRAINING passes, which keep the pre-activations: train_forward, weight_grads,
        # tangent_weight_grads)
        self.precision = precision
        self.activation = activation
        M, S = len(weights), len(weights[0])
        nl = len(weights[0][0])
        if not (2 <= nl <= _lib.MAX_LAYERS):
            raise ValueError(f"networks must have 2..{_lib.MAX_LAYERS} Linear layers")
        if aev_len % 16 != 0:
            raise ValueError("AEV length must be a multiple of 16")
        self.M, self.S, self.nl, self.aev_len = M, S, nl, aev_len
        self.device = device
        self.shapes = [[tuple(weights[0][s][l].shape) for l in range(nl)] for s in range(S)]   # unpadded [out, in]
        # The layouts are produced by the library itself (anihip_mlp_pack, csrc/pack.hip): the same call a caller without
        # this package makes.  Parameters are handed over as contiguous fp32 tensors where they live (device or host).
        sh = _lib.MlpShape()
        sh.n_members, sh.num_species, sh.n_layers, sh.aev_len = M, S, nl, aev_len
        sh.aev_radial_len = -1 if radial_len is None else int(radial_len)
        sh.precision = _lib.MLP_F16X3 if precision == "f16x3" else _lib.MLP_FP32
        sh.activation = _lib.ACT_GELU if activation == "gelu" else _lib.ACT_CELU
        sh.celu_alpha = celu_alpha
        for s in range(S):
            if weights[0][s][nl - 1].shape[0] != 1:
                raise ValueError("final layer must have one output")
            for l in range(nl):
                sh.out_dims[s][l] = int(weights[0][s][l].shape[0])
        src, on_dev = [], None
        wp, bp = (C.c_void_p * (M * S * nl))(), (C.c_void_p * (M * S * nl))()
        for m in range(M):
            for s in range(S):
                for l in range(nl):
                    W = weights[m][s][l].detach().to(torch.float32).contiguous()
                    b = biases[m][s][l].detach().to(torch.float32).contiguous()
                    if tuple(W.shape) != self.shapes[s][l] or b.numel() != W.shape[0]:
                        raise ValueError("every member must have the same layer shapes")
                    if on_dev is None:
                        on_dev = W.is_cuda
                    if W.is_cuda != on_dev or b.is_cuda != on_dev:
                        raise ValueError("parameters must all live on the host or all on a device")
                    src += [W, b]
                    wp[(m * S + s) * nl + l], bp[(m * S + s) * nl + l] = W.data_ptr(), b.data_ptr()
        L = _lib.lib()
        need = L.anihip_mlp_pack_bytes(C.byref(sh))
        if need == 0:
            raise ValueError("libanihip: " + L.anihip_last_error().decode())
        self._buf = torch.empty(need, dtype=torch.uint8, device=device)
        d = _lib.MlpDesc()
        if on_dev:
            torch.cuda.current_stream(src[0].device).synchronize()   # (the library reads the parameters with blocking copies)
        stream = _stream() if self._buf.is_cuda else None
        _lib.check(L.anihip_mlp_pack(stream, C.byref(sh), wp, bp, 1 if on_dev else 0, _ptr(self._buf), need,
                                     1 if self._buf.is_cuda else 0, C.byref(d)))
        del src
        self.radial_len = d.aev_radial_len
        self.desc = d
        self._ws: tp.Optional[Tensor] = None
        self._train_ws: tp.Optional[Tensor] = None
        self._fast_training: tp.Optional[bool] = None
        self._second: tp.Optional[tp.Tuple[torch.cuda.Stream, torch.cuda.Event, torch.cuda.Event]] = None

    def _own_second_stream(self) -> None:
        """The second stream of the per-species launches with its fork / join events (anihip_mlp_desc.aux_stream, include/anihip.h):
        this pack's own, alive as long as the pack.  The library creates none; without them it keeps every launch on the caller's
        stream, which costs the 4 % of the step that the scheme buys (per-species launches) -- hence no silent fallback.
        (No copy of a pack can carry them along: ctypes refuses to copy or pickle the descriptor's pointers.)"""
        self._second = None
        self.desc.aux_stream = self.desc.fork_event = self.desc.join_event = None
        if torch.cuda.is_current_stream_capturing():
            return   # (nothing is created or recorded beside a capture: the library keeps a captured step on the caller's stream)
        stream = torch.cuda.Stream(device=self.device)
        fork, join = torch.cuda.Event(enable_timing=False), torch.cuda.Event(enable_timing=False)
        fork.record(stream)   # (torch creates an event's handle at its first record)
        join.record(stream)
        handles = (stream.cuda_stream, fork.cuda_event, join.cuda_event)
        if not all(handles):
            raise RuntimeError("torch handed out a NULL stream or event handle for the per-species launches")
        self._second = (stream, fork, join)
        self.desc.aux_stream, self.desc.fork_event, self.desc.join_event = handles

    def array(self, ptr: int, shape: tp.Sequence[int], dtype: torch.dtype = torch.float32) -> Tensor:
        """View of one packed array (a pointer of ``desc``) inside the buffer anihip_mlp_pack filled."""
        off = int(ptr) - self._buf.data_ptr()
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        assert 0 <= off and off + n <= self._buf.numel(), "pointer outside the packed buffer"
        return self._buf[off:off + n].view(dtype).view(*shape)

    def workspace(self, n_central: int, want_grad: bool = True) -> Tensor:
        """Scratch of one anihip_mlp_forward_backward call over n_central atoms: what the kernels that call runs touch
        (with the layer-0 backward inside the fused kernel ~100 B per atom: index lists, tile table, per-member energies;
        19.5 KB per atom for the layer-by-layer kernels of an ANI-2x pack)."""
        need = _lib.lib().anihip_mlp_forward_backward_workspace_bytes(C.byref(self.desc), n_central, int(want_grad))
        if self._ws is None or self._ws.numel() < need:
            if self.pinned and self._ws is not None:
                # a captured HIP graph replays into self._ws: never free or replace it; a larger eager call gets a
                # buffer of its own
                return torch.empty(need, dtype=torch.uint8, device=self.device)
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def forward_backward(self, species: Tensor, aev: Tensor, lo: int = 0, hi: tp.Optional[int] = None,
                         want_grad: bool = True, want_members: bool = False, chunk: tp.Optional[int] = None,
                         atomic_e: tp.Optional[Tensor] = None, grad_aev: tp.Optional[Tensor] = None,
                         slab_mask: tp.Optional[Tensor] = None, shard_rows: bool = False, tile_hint: int = 0,
                         plain_slabs: bool = False) -> tp.Tuple[Tensor, tp.Optional[Tensor], tp.Optional[Tensor]]:
        """Per-atom ensemble-mean energies [N], d e/d aev [N,L] (optional), member energies [M,N].

        slab_mask (int32 [N] from AevEngine.forward): the layer-0 GEMMs skip AEV slabs no atom of a row tile
        flags; grad_aev is then only defined inside the flagged slabs (all AevEngine.backward reads).  The flags must
        be in the order of this pack's layer-0 planes: the ANI slab order of the 16 / 32-column grids (radial_len > 0),
        or -- plain_slabs=True, general grids, radial_len == 0 -- the plain 32-column slabs of the row.
        shard_rows=True: aev (and the returned / given grad_aev) hold only the rows lo..hi.
        tile_hint: _lib.MLP_FLAG_SMALL_TILES / MLP_FLAG_BIG_TILES from a caller that knows the composition (used unless the
        instance / class flags already choose a layer-0 tiling)."""
        _require_cuda(species, aev, slab_mask)
        if slab_mask is not None:
            assert slab_mask.dtype == torch.int32 and slab_mask.numel() == species.numel()
            if (self.radial_len == 0) != plain_slabs or (plain_slabs and (self.aev_len > 1024 or self.precision != "f16x3")):
                slab_mask = None   # (flags in another order than the planes': multiply every slab)
        n = species.numel()
        hi = n if hi is None else hi
        rows = (hi - lo) if shard_rows else n
        rows0 = lo if shard_rows else 0
        assert aev.dtype == torch.float32 and aev.is_contiguous() and aev.numel() == rows * self.aev_len
        dev = aev.device
        full = (lo == 0 and hi == n) or shard_rows
        if atomic_e is None:
            atomic_e = (torch.empty if (lo == 0 and hi == n) else torch.zeros)(n, dtype=torch.float32, device=dev)
        if want_grad and grad_aev is None:
            grad_aev = (torch.empty if full else torch.zeros)((rows, self.aev_len), dtype=torch.float32, device=dev)
        if want_grad:
            assert grad_aev.dtype == torch.float32 and grad_aev.is_contiguous()
            assert grad_aev.numel() == rows * self.aev_len
        member_e = torch.zeros((self.M, n), dtype=torch.float32, device=dev) if want_members else None
        L = _lib.lib()
        # equal chunks (a short last chunk would leave most CUs idle in its tail), up to twice the preferred size when
        # that saves rounds of the 256-row layer-0 backward GEMM: its one-workgroup-per-CU tiles run in whole rounds
        # over the CUs (a rank's 292 k-atom shard of the 2.3 M-atom box: 2 chunks x 3 rounds -> 1 chunk x 5 rounds)
        nn_ = hi - lo
        n_cu = _n_cus(dev)
        fl = PackedNetworks.default_flags if self.flags is None else self.flags
        tiles = _lib.MLP_FLAG_SMALL_TILES | _lib.MLP_FLAG_BIG_TILES
        if not fl & tiles:
            fl |= tile_hint & tiles
        fl |= tile_hint & ~tiles   # (other switches a caller hands over with the hint, e.g. MLP_FLAG_BWD_TWO_PRODUCTS)
        self.desc.flags = fl   # (before the workspace queries: the flags choose the kernels)
        stream = _stream()
        # (lazily: member packs, training packs and small systems never see the flag and hold no stream.  torch hands streams out
        # of a pool: should the caller's be this pack's second one, the pack draws another)
        if fl & _lib.MLP_FLAG_SHAPED and (self._second is None or self.desc.aux_stream == stream):
            self._own_second_stream()
        if chunk is None:
            # ONE call when its scratch is small -- the fused kernel with the layer-0 backward inside keeps everything but
            # ~100 B per atom in LDS: one persistent launch and one tail instead of one per 2^20 atoms (-0.5 ms per step at
            # 2.34 M atoms) -- else launch groups of 2^20 atoms (19.5 KB of activations per atom for an ANI-2x pack)
            chunk = 1 << 20
            if nn_ > chunk and L.anihip_mlp_forward_backward_workspace_bytes(C.byref(self.desc), nn_, int(want_grad)) <= 512 * nn_:
                chunk = nn_

        def plan(nc: int) -> tp.Tuple[int, int]:
            st_ = max(1, -(-(-(-nn_ // nc)) // 256) * 256)
            return nc * -(-(st_ // 256 + self.S) // n_cu), st_

        nc_hi = max(1, -(-nn_ // chunk))
        cands = range(max(1, -(-nn_ // (2 * chunk))), nc_hi + 3) if want_grad and nn_ >= 65536 else (nc_hi,)
        nchunk = min(cands, key=lambda nc: (plan(nc)[0], nc))
        step = plan(nchunk)[1]
        for c0 in range(lo, hi, step):
            c1 = min(hi, c0 + step)
            ws = self.workspace(c1 - c0, want_grad)
            _lib.check(L.anihip_mlp_forward_backward(
                stream, C.byref(self.desc), n, c0, c1, _ptr(species), _row_ptr(aev, rows0, self.aev_len),
                _ptr(slab_mask), _ptr(ws), ws.numel(), _ptr(atomic_e),
                _row_ptr(grad_aev, rows0, self.aev_len) if want_grad else None, _ptr(member_e)))
        return atomic_e, (grad_aev if want_grad else None), member_e

    def refresh(self, weights, biases, fused_only: bool = False) -> None:
        """Re-read the parameter values (same shapes as at construction) into the packed arrays on the device
        (anihip_mlp_repack): w / wt / bias of an fp32 pack, every layout -- fp32 arrays, {hi, lo} fp16 planes, fragment
        orders, fused_bounds -- of an f16x3 pack (with the weight scales it was built with; ``scale_overflowed()`` tells,
        one call late, whether a weight has outgrown them)."""
        M, S, nl = self.M, self.S, self.nl
        ptrs = [t.data_ptr() for m in range(M) for s in range(S) for l in range(nl)
                for t in (weights[m][s][l], biases[m][s][l])]
        key = tuple(ptrs)
        if getattr(self, "_src_key", None) != key:
            for m in range(M):
                for s in range(S):
                    for l in range(nl):
                        W, b = weights[m][s][l], biases[m][s][l]
                        if (tuple(W.shape) != self.shapes[s][l] or W.dtype != torch.float32 or not W.is_contiguous()
                                or b.dtype != torch.float32 or not b.is_contiguous() or W.device != self.device):
                            raise ValueError("refresh() needs contiguous fp32 parameters of the packed shapes")
            self._src_tab = torch.tensor(ptrs, dtype=torch.int64, device=self.device)
            self._src_key = key
            self._out_in = np.asarray(self.shapes, dtype=np.int32).reshape(-1).copy()
        status = None
        if self.precision == "f16x3":
            if getattr(self, "_repack_status", None) is None:
                self._repack_status = torch.zeros(1, dtype=torch.int32, device=self.device)
                self._repack_poll = None
            status = self._repack_status
        # fused_only (f16x3): what the fused kernel and the fast training pass read; the layer-by-layer layouts go stale until
        # a full refresh (self.stale_layouts)
        flags = _lib.REPACK_FUSED_ONLY if (fused_only and self.precision == "f16x3") else 0
        self.stale_layouts = bool(flags)
        _lib.check(_lib.lib().anihip_mlp_repack(_stream(), C.byref(self.desc), _ptr(self._src_tab),
                                                self._out_in.ctypes.data, _ptr(status), flags))
        if status is not None and not torch.cuda.is_current_stream_capturing() and self._repack_poll is None:
            host = torch.empty(1, dtype=torch.int32, pin_memory=True)
            host.copy_(status, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._repack_poll = (host, ev)

    def scale_overflowed(self) -> bool:
        """Did a refresh find a weight outside the fp16 range of its layer's scale?  Reads what the PREVIOUS refresh queued
        (no wait unless the host runs a whole step ahead); the caller then packs again on the host (new scales)."""
        poll = getattr(self, "_repack_poll", None)
        if poll is None or torch.cuda.is_current_stream_capturing():
            return False
        host, ev = poll
        if not ev.query():
            return False
        self._repack_poll = None
        return bool(host[0])

    def fast_training(self) -> bool:
        """Do the training passes of this pack run through the fused network kernel?  The library's answer
        (anihip_mlp_fast_training: the rule its own training entry points apply), asked once: shapes and planes do not change
        after construction."""
        if self._fast_training is None:
            self._fast_training = bool(_lib.lib().anihip_mlp_fast_training(C.byref(self.desc)))
        return self._fast_training

    def _freshen_layouts(self, fused_route: bool) -> None:
        """A refresh(..., fused_only=True) leaves the layer-by-layer layouts (w / wt / wh / wth) at the parameters of the pack
        before it.  A call that the library serves layer by layer -- anything but the fused training pass without d Loss /
        d aev -- must not read them: run the full repack from the parameter table of the last refresh first.  Which route a
        pack takes is the library's answer (fast_training() = anihip_mlp_fast_training, the rule anihip_mlp_train_forward and
        anihip_mlp_weight_grads apply themselves), so this guard and the C side cannot drift apart."""
        if getattr(self, "stale_layouts", False) and not fused_route:
            _lib.check(_lib.lib().anihip_mlp_repack(_stream(), C.byref(self.desc), _ptr(self._src_tab),
                                                    self._out_in.ctypes.data, _ptr(getattr(self, "_repack_status", None)), 0))
            self.stale_layouts = False

    def train_forward(self, species: Tensor, aev: Tensor) -> tp.Tuple[Tensor, Tensor]:
        """First half of a training step: exact-fp32 forward that keeps the activations.  Returns (atomic_e [N],
        workspace) -- hand the workspace to weight_grads(..., workspace=ws) for the backward half."""
        _require_cuda(species, aev)
        self._freshen_layouts(self.fast_training())
        n = species.numel()
        assert aev.dtype == torch.float32 and aev.is_contiguous() and aev.numel() == n * self.aev_len
        L = _lib.lib()
        ws = torch.empty(L.anihip_mlp_train_workspace_bytes(C.byref(self.desc), n), dtype=torch.uint8,
                         device=aev.device)
        atomic_e = torch.zeros(n, dtype=torch.float32, device=aev.device)
        _lib.check(L.anihip_mlp_train_forward(_stream(), C.byref(self.desc), n, 0, n, _ptr(species), _ptr(aev),
                                              _ptr(ws), ws.numel(), _ptr(atomic_e)))
        return atomic_e, ws

    def _grad_buffers(self, dev):
        """One flat fp32 buffer holding every gradient array of anihip_species_grads + the ctypes pointer table."""
        M, S, nl, d = self.M, self.S, self.nl, self.desc
        sizes = []
        for s in range(S):
            dims = [d.net[s].dims[l] for l in range(nl + 1)]
            for l in range(nl):
                sizes += [M * dims[l] * dims[l + 1], M * dims[l + 1]]
        offs = np.concatenate([[0], np.cumsum([(x + 63) // 64 * 64 for x in sizes])])
        buf = torch.empty(int(offs[-1]), dtype=torch.float32, device=dev)
        sg = (_lib.SpeciesGrads * S)()
        q = 0
        for s in range(S):
            for l in range(nl):
                sg[s].gw[l] = buf.data_ptr() + 4 * int(offs[q])
                sg[s].gbias[l] = buf.data_ptr() + 4 * int(offs[q + 1])
                q += 2
        return buf, sg, sizes, offs

    def _unpack_grads(self, total: Tensor, sizes, offs):
        """Flat gradient buffer -> gw[m][s][l] [out, in], gb[m][s][l] [out] (views when the widths are unpadded)."""
        M, S, nl, d = self.M, self.S, self.nl, self.desc
        gw = [[[None] * nl for _ in range(S)] for _ in range(M)]
        gb = [[[None] * nl for _ in range(S)] for _ in range(M)]
        q = 0
        for s in range(S):
            dims = [d.net[s].dims[l] for l in range(nl + 1)]
            for l in range(nl):
                out, inn = self.shapes[s][l]
                w = total[int(offs[q]): int(offs[q]) + sizes[q]]
                b = total[int(offs[q + 1]): int(offs[q + 1]) + sizes[q + 1]]
                q += 2
                if l == nl - 1:
                    wv, bv = w.view(M, 1, dims[l]), b.view(M, 1)
                else:
                    wv, bv = w.view(M, dims[l + 1], dims[l]), b.view(M, dims[l + 1])   # nn.Linear layout
                for m in range(M):
                    gw[m][s][l] = wv[m, :out, :inn]
                    gb[m][s][l] = bv[m, :out]
        return gw, gb

    def tangent_weight_grads(self, species: Tensor, aev: Tensor, tangent: Tensor):
        """Second-order pass of force training (anihip_mlp_tangent_weight_grads): gradients with respect to every
        weight and bias of  S = sum_i tangent_i . d atomic_e[i] / d aev_i,  plus the per-atom terms of S [N]."""
        _require_cuda(species, aev, tangent)
        n = species.numel()
        dev = aev.device
        assert aev.dtype == torch.float32 and aev.is_contiguous() and aev.numel() == n * self.aev_len
        t = tangent.to(torch.float32).contiguous()
        assert t.numel() == n * self.aev_len
        buf, sg, sizes, offs = self._grad_buffers(dev)
        L = _lib.lib()
        ws = torch.empty(L.anihip_mlp_tangent_workspace_bytes(C.byref(self.desc), n), dtype=torch.uint8, device=dev)
        de = torch.zeros(n, dtype=torch.float32, device=dev)
        _lib.check(L.anihip_mlp_tangent_weight_grads(
            _stream(), C.byref(self.desc), n, 0, n, _ptr(species), _ptr(aev), _ptr(t), _ptr(ws), ws.numel(), sg,
            _ptr(de)))
        gw, gb = self._unpack_grads(buf, sizes, offs)
        return gw, gb, de

    def input_hvp(self, species: Tensor, aev: Tensor, tangent: Tensor) -> Tensor:
        """(1/M) sum_m H_m(aev_i) tangent[k, i]  [K, N, L]: input-space Hessian-vector products of the ensemble-mean atomic
        energies for K AEV-space tangents [K, N, L] (anihip_mlp_input_hvp; exact fp32, activations once per atom)."""
        _require_cuda(species, aev, tangent)
        n = species.numel()
        dev = aev.device
        a = aev.detach().to(torch.float32).contiguous()
        t = tangent.detach().to(torch.float32).contiguous()
        K = t.shape[0]
        assert a.numel() == n * self.aev_len and t.numel() == K * n * self.aev_len
        L = _lib.lib()
        ws = torch.empty(L.anihip_mlp_input_hvp_workspace_bytes(C.byref(self.desc), n, K), dtype=torch.uint8, device=dev)
        out = torch.empty((K, n, self.aev_len), dtype=torch.float32, device=dev)
        _lib.check(L.anihip_mlp_input_hvp(_stream(), C.byref(self.desc), n, _ptr(species), _ptr(a), K, _ptr(t), _ptr(ws),
                                          ws.numel(), _ptr(out)))
        return out

    def rows_hvp_row_bytes(self, n_atoms: int) -> int:
        """Workspace bytes one row of anihip_mlp_rows_hvp costs (the query is linear in the rows)."""
        L = _lib.lib()
        one = L.anihip_mlp_rows_hvp_workspace_bytes(C.byref(self.desc), n_atoms, 1)
        two = L.anihip_mlp_rows_hvp_workspace_bytes(C.byref(self.desc), n_atoms, 2)
        return max(int(two - one), 1)

    def rows_hvp_prepare(self, species: Tensor, aev: Tensor, max_rows: int) -> Tensor:
        """Workspace of rows_hvp for row sets of at most max_rows rows, with the exact-fp32 forward over the atoms run
        once and its activations kept (anihip_mlp_rows_hvp_prepare)."""
        _require_cuda(species, aev)
        n = species.numel()
        assert aev.dtype == torch.float32 and aev.is_contiguous() and aev.numel() == n * self.aev_len
        L = _lib.lib()
        ws = torch.empty(L.anihip_mlp_rows_hvp_workspace_bytes(C.byref(self.desc), n, max_rows), dtype=torch.uint8,
                         device=aev.device)
        _lib.check(L.anihip_mlp_rows_hvp_prepare(_stream(), C.byref(self.desc), n, _ptr(species), _ptr(aev), _ptr(ws),
                                                 ws.numel()))
        return ws

    def rows_hvp(self, species: Tensor, ws: Tensor, row_atom: Tensor, tangent: Tensor) -> Tensor:
        """(1/M) sum_m H_m(aev_{row_atom[q]}) tangent[q]  [R, L] over explicit rows, the rows of a species contiguous
        (anihip_mlp_rows_hvp; exact fp32; ws from rows_hvp_prepare)."""
        _require_cuda(species, ws, row_atom, tangent)
        n = species.numel()
        R = row_atom.numel()
        assert tangent.dtype == torch.float32 and tangent.is_contiguous() and tangent.numel() == R * self.aev_len
        out = torch.empty((R, self.aev_len), dtype=torch.float32, device=tangent.device)
        _lib.check(_lib.lib().anihip_mlp_rows_hvp(_stream(), C.byref(self.desc), n, _ptr(species), R, _ptr(row_atom),
                                                  _ptr(tangent), _ptr(ws), ws.numel(), _ptr(out)))
        return out

    def flat_grad_target(self, w_ptr, b_ptr, member_stride: int):
        """anihip_species_grads table for gradients that go straight into a flat buffer (torchani_amd.optim.Adam):
        w_ptr[s][l] / b_ptr[s][l] = device addresses of MEMBER 0's weight / bias gradient, member m's lie member_stride floats
        further on; accumulated into (the optimizer zeroes the buffer).  Needs unpadded widths."""
        sg = (_lib.SpeciesGrads * self.S)()
        for s in range(self.S):
            for l in range(self.nl):
                out, inn = self.shapes[s][l]
                if self.desc.net[s].dims[l] != inn or (l < self.nl - 1 and self.desc.net[s].dims[l + 1] != out):
                    raise ValueError("flat gradient targets need layer widths that are multiples of 32")
                sg[s].gw[l], sg[s].gbias[l] = int(w_ptr[s][l]), int(b_ptr[s][l])
            sg[s].member_stride, sg[s].accumulate = int(member_stride), 1
        return sg

    def weight_grads(self, species: Tensor, aev: Tensor, grad_atomic_e: Tensor,
                     want_grad_aev: bool = False, chunk: int = 1 << 16, workspace: tp.Optional[Tensor] = None,
                     target=None):
        """Training pass (anihip_mlp_weight_grads): gradients of  sum_i grad_atomic_e[i] * atomic_e[i]  with respect
        to every weight and bias, returned in torch.nn.Linear layout: gw[m][s][l] [out, in], gb[m][s][l] [out];
        plus atomic_e [N] and, optionally, d Loss / d aev [N, L].  Replaces torch autograd through
        nn/_core.py:146-149 / nn/_containers.py:377-421,608-636."""
        _require_cuda(species, aev, grad_atomic_e)
        self._freshen_layouts(self.fast_training() and not want_grad_aev)
        n = species.numel()
        dev = aev.device
        assert aev.dtype == torch.float32 and aev.is_contiguous() and aev.numel() == n * self.aev_len
        g_at = grad_atomic_e.to(torch.float32).contiguous().view(-1)
        assert g_at.numel() == n
        d = self.desc
        atomic_e = torch.zeros(n, dtype=torch.float32, device=dev)
        grad_aev = torch.zeros((n, self.aev_len), dtype=torch.float32, device=dev) if want_grad_aev else None
        L = _lib.lib()
        total = None
        if workspace is not None:
            chunk = max(n, 1)   # the forward half ran over all atoms at once (train_forward)
        for c0 in range(0, max(n, 1), chunk):
            c1 = min(n, c0 + chunk)
            if target is not None:   # (flat_grad_target: accumulated in place, nothing to unpack)
                buf, sg, sizes, offs = None, target, None, None
            else:
                buf, sg, sizes, offs = self._grad_buffers(dev)
            need = L.anihip_mlp_train_workspace_bytes(C.byref(d), c1 - c0)
            if workspace is not None:
                ws = workspace
                assert ws.numel() >= need
            else:
                if self._train_ws is None or self._train_ws.numel() < need:
                    self._train_ws = torch.empty(need, dtype=torch.uint8, device=dev)
                ws = self._train_ws
            _lib.check(L.anihip_mlp_weight_grads(
                _stream(), C.byref(d), n, c0, c1, _ptr(species), _ptr(aev), _ptr(g_at), _ptr(ws),
                ws.numel(), sg, _ptr(atomic_e), _ptr(grad_aev), 1 if workspace is not None else 0))
            if buf is not None:
                total = buf if total is None else total.add_(buf)
        if target is not None:
            return None, None, atomic_e, grad_aev
        gw, gb = self._unpack_grads(total, sizes, offs)
        return gw, gb, atomic_e, grad_aev


def energy_reduce(species: Tensor, atomic_e: Tensor, sae: tp.Optional[Tensor], lo: int = 0,
                  hi: tp.Optional[int] = None) -> Tensor:
    """Molecular energies [C] in float64 = sum over atoms lo..hi of (atomic_e + sae[species])."""
    _require_cuda(species, atomic_e, sae)
    Cn, A = species.shape
    n = Cn * A
    hi = n if hi is None else hi
    out = torch.empty(Cn, dtype=torch.float64, device=species.device)
    if sae is not None:
        assert sae.dtype == torch.float64
    _lib.check(_lib.lib().anihip_energy_reduce(
        _stream(), Cn, A, lo, hi, _ptr(species), _ptr(atomic_e), _ptr(sae), _ptr(out)))
    return out


def energy_forces_finish(species: Tensor, atomic_e: Tensor, sae: tp.Optional[Tensor], grad_coords: Tensor, lo: int = 0,
                         hi: tp.Optional[int] = None) -> Tensor:
    """energy_reduce, and ``grad_coords`` (float32, contiguous) negated IN PLACE into forces, in one launch for batches of
    small molecules (anihip_energy_forces_finish).  Returns the molecular energies [C] in float64."""
    _require_cuda(species, atomic_e, sae, grad_coords)
    Cn, A = species.shape
    hi = Cn * A if hi is None else hi
    assert grad_coords.dtype == torch.float32 and grad_coords.is_contiguous()
    if sae is not None:
        assert sae.dtype == torch.float64
    out = torch.empty(Cn, dtype=torch.float64, device=species.device)
    _lib.check(_lib.lib().anihip_energy_forces_finish(
        _stream(), Cn, A, lo, hi, _ptr(species), _ptr(atomic_e), _ptr(sae), _ptr(out), _ptr(grad_coords),
        grad_coords.numel()))
    return out
