"""Autograd helpers with the reference's names and behaviour (torchani/grad.py:42-399).

Hessians with respect to the coordinates (grad.py:86-150,239-260) come in two forms:

* ``hessians`` / ``forces_and_hessians``: through autograd like the reference -- one Hessian-vector product per force
  component.  Forces taken with ``create_graph=True`` from a model with FROZEN parameters are differentiable with respect to
  the coordinates: ``torch.autograd.grad((F * w).sum(), x) == -H w`` for any ``w``.  Each product runs the batched AEV JVP,
  the network input HVP and the second-order AEV backward of the HIP engine (include/anihip.h).
* ``energies_forces_and_hessians``: the batched path -- neighbor rows, AEVs and d E / d aev once, then the unit directions
  of all molecules in chunks of K (``hessian_chunk_size``, from a fixed memory budget) through the same three kernels.
* ``energies_forces_and_sparse_hessians``: the block-sparse path for large systems (``tuples.BlockHessian``) -- each unit
  direction is worked only on the central atoms whose AEV it moves, and only the blocks inside the cutoff pattern are kept.
* ``energies_forces_and_strain_hessians``: second derivatives with respect to the strain (x -> x S, cell -> cell S) -- the
  strain-strain block, the internal-strain tensor and the per-molecule virial, from 9 strain directions whatever the
  number of atoms; ``elastic_constants`` turns them into clamped- or relaxed-ion elastic constants.

The closed-form pair potentials (xTB repulsion, ZBL, Lennard-Jones, fixed-charge Coulomb / MNOK: ANI-2xr, ANI-r2s and
models built with ``add_pair_potential``) add their Hessian-vector products (anihip_pair_analytic_hvp) on both paths, and a
standalone pair potential may stand in for the model.  D3 dispersion (ANI-2dr) has no second derivative here: every Hessian
entry point raises NotImplementedError naming it.  ``vibrational_analysis`` and ``VibAnalysis`` (grad.py:153-236) are
host-side; ``sparse_vibrational_analysis`` finds the lowest modes of a ``BlockHessian`` on the device (anihip_block_hessian_spmm
under the solver of ``torchani_amd.modes``); unit conversions live in ``torchani_amd.units``.  NOT here: a numerical Hessian, the modules ``torchani.cutoffs``
(the cutoff envelopes live in the AEV kernels: ``AEVComputer(..., cutoff_fn="cosine" | "smooth")``,
``constants.cutoff_kernel_name``) and ``torchani.sae`` (``nn.SelfEnergy`` is the energy shifter of the models).
"""
from __future__ import annotations

import math
import typing as tp

import torch
from torch import Tensor

from .tuples import HeatFlux
from .tuples import (BlockHessian, EnergiesForces, EnergiesForcesHessians, EnergiesForcesSparseHessians,
                     EnergiesForcesStrainHessians, ForcesHessians, SparseVibAnalysis, VibAnalysis)
from . import units as _units
from .utils import pbc_tuple


def forces(energies: Tensor, coordinates: Tensor, retain_graph: tp.Optional[bool] = None,
           create_graph: bool = False) -> Tensor:
    """forces = -d(sum energies)/d coordinates (grad.py:42-64)."""
    if not coordinates.requires_grad:
        raise ValueError("'coordinates' passed to `torchani.grad.forces` must require grad")
    if not coordinates.is_leaf:
        raise ValueError("'coordinates' passed to `torchani.grad` functions must be a 'leaf' Tensor"
                         "(i.e. must not have been modified prior to being used as an input).")
    (g,) = torch.autograd.grad([energies.sum()], [coordinates], retain_graph=retain_graph, create_graph=create_graph)
    return -g


def grads(scalars: Tensor, coords: Tensor, retain_graph: tp.Optional[bool] = None,
          create_graph: bool = False) -> Tensor:
    """Alias of forces with the sign flipped (grad.py:68-74)."""
    return -forces(scalars, coords, retain_graph, create_graph)


__all__ = ["single_point", "forces_for_training", "energies_and_forces", "forces", "grads", "calc_forces", "calc_grads",
           "hessians", "forces_and_hessians", "energies_forces_and_hessians", "calc_hessians", "calc_forces_and_hessians",
           "vibrational_analysis"]

calc_forces = forces
calc_grads = grads


def forces_for_training(energies: Tensor, coordinates: Tensor) -> Tensor:
    """Forces that can be differentiated again with respect to the parameters (grad.py:82-83): the engine's
    double-backward Functions answer with anihip_aev_jvp / anihip_mlp_tangent_weight_grads."""
    return forces(energies, coordinates, retain_graph=True, create_graph=True)


def _no_hessians(*args, **kwargs):
    # (single_point(hessians=True) is not wired up yet: use energies_forces_and_hessians / forces_and_hessians)
    raise NotImplementedError("single_point(hessians=True) is not available: use grad.energies_forces_and_hessians or "
                              "grad.forces_and_hessians")


def hessians(forces: Tensor, coordinates: Tensor, retain_graph: tp.Optional[bool] = None) -> Tensor:
    """d^2 E / d x^2 [C, 3A, 3A] from forces taken with create_graph=True (grad.py:108-145): one Hessian-vector product per
    force component through autograd.  Padding atoms give zero rows and columns."""
    if not coordinates.requires_grad:
        raise ValueError("'coordinates' passed to `torchani.grad.hessians` must require grad")
    if not coordinates.is_leaf:
        raise ValueError("'coordinates' passed to `torchani.grad` functions must be a 'leaf' Tensor"
                         "(i.e. must not have been modified prior to being used as an input).")
    if not forces.requires_grad:
        raise RuntimeError("these forces carry no graph: take them with create_graph=True (grad.forces_and_hessians)")
    C, A, D = forces.shape
    n = A * D
    flat = forces.reshape(C, n).unbind(dim=1)
    cols = []
    for j, comp in enumerate(flat):
        keep = retain_graph if j == n - 1 else True
        (gj,) = torch.autograd.grad([comp.sum()], [coordinates], retain_graph=keep, allow_unused=True)
        if gj is None:
            # (trainable parameters: the forces' second-order graph leads to the parameters, not to the coordinates)
            raise RuntimeError("these forces do not depend on the coordinates to second order: Hessians through autograd "
                               "need a model with frozen parameters (requires_grad_(False)); "
                               "grad.energies_forces_and_hessians serves any model")
        cols.append(gj.reshape(C, 1, n))
    return -torch.cat(cols, dim=1)


def forces_and_hessians(energies: Tensor, coordinates: Tensor, retain_graph: tp.Optional[bool] = None) -> ForcesHessians:
    """ForcesHessians(forces, hessians) through autograd (grad.py:86-103)."""
    f = forces(energies, coordinates, retain_graph=True, create_graph=True)
    return ForcesHessians(f, hessians(f, coordinates, retain_graph=retain_graph))


calc_hessians = hessians
calc_forces_and_hessians = forces_and_hessians

# device memory one chunk of directions of energies_forces_and_hessians may take
HESSIAN_BUDGET_BYTES = 1 << 30


def hessian_direction_bytes(n_rows: int, aev_len: int, hvp_row_bytes: int) -> int:
    """Device bytes one direction of energies_forces_and_hessians costs over n_rows = C * A atom rows: its tangent and
    output (3 floats each), J t and H_net J t (aev_len floats each), and the network HVP workspace of its rows."""
    return n_rows * (4 * 6 + 8 * aev_len + hvp_row_bytes)


def hessian_chunk_size(n_molecules: int, n_atoms: int, aev_len: int, hvp_row_bytes: int,
                       budget: int = HESSIAN_BUDGET_BYTES) -> int:
    """K: unit directions per chunk of energies_forces_and_hessians, from the fixed memory budget (never from a user
    option): as many as fit, at least 1, at most the 3A directions of a molecule."""
    per = hessian_direction_bytes(n_molecules * n_atoms, aev_len, hvp_row_bytes)
    return int(max(1, min(3 * n_atoms, budget // max(per, 1))))


def _pair_potentials_without_hessians(model) -> tp.List[str]:
    """Names of the enabled pair potentials of a model (or of a standalone potential) that have no second derivative
    with respect to the coordinates: TwoBodyDispersionD3 (its coordination-number coupling)."""
    from .potentials import _AnalyticPair, _Standalone

    if isinstance(model, _Standalone):
        pots = [model]
    else:
        pots = [p for name, p in getattr(model, "potentials", {}).items() if name != "nnp" and getattr(p, "_enabled", False)]
    return [type(p).__name__ for p in pots if not isinstance(p, _AnalyticPair)]


def _analytic_pair_rows(model, species32: Tensor, c32: Tensor, cell, pbc, aev_rows) -> tp.List[tuple]:
    """(potential, rows) of every enabled closed-form pair potential of a model, on the rows its forward uses: the AEV's
    rows, or the potential's own (model._pair_rows) when its cutoff is larger or infinite.  Overflowed rows raise."""
    out = []
    for name, pot in model.potentials.items():
        if name == "nnp" or not pot._enabled:
            continue
        rows = aev_rows
        if rows is None or pot.cutoff > model.aev_computer.radial.cutoff + 1e-6:
            rows = model._pair_rows(pot, species32, c32, cell, pbc)
            if rows.overflowed():
                raise RuntimeError(f"pair potential {name!r}: an atom has more than {rows.row_cap} neighbors inside its "
                                   f"cutoff ({pot.cutoff} A): its Hessian would be wrong")
        out.append((pot, rows))
    return out


class _SecondOrderInputs(tp.NamedTuple):
    ef: EnergiesForces
    species32: Tensor
    nnp: bool                             # the networks are enabled: eng, aev, packed and g are set
    nbrs: tp.Any                          # the AEV's neighbor rows (None: not built)
    eng: tp.Any
    aev: tp.Optional[Tensor]
    packed: tp.Any
    g: tp.Optional[Tensor]                # d E / d aev
    pairs: tp.List[tuple]                 # (potential, rows) of every closed-form pair term


def _second_order_inputs(model, species: Tensor, coordinates: Tensor, cell, pbc, what: str,
                         sparse: bool = False) -> _SecondOrderInputs:
    """What the Hessian and strain drivers compute before their direction loops.  D3 raises NotImplementedError (``what``
    names the derivatives); then energies and forces (grad.energies_and_forces), the neighbor rows, AEVs and d E / d aev
    of the networks, and the closed-form pair terms on the rows their forwards use (a standalone potential: itself on its
    own rows, overflow raises).  sparse: the rows are always built and the pair terms are _sparse_hessian_pairs's, on them
    (checked before any work)."""
    from .potentials import _Standalone

    pots = _pair_potentials_without_hessians(model)
    if pots:
        raise NotImplementedError(f"the pair potential(s) {', '.join(pots)} have no second derivative with respect to the "
                                  f"coordinates: {what} of this model are not available")
    sparse_pots = _sparse_hessian_pairs(model) if sparse else []
    ef = energies_and_forces(model, species, coordinates, cell, pbc, keep_vars=False)
    nnp, nbrs, eng, aev, packed, g = False, None, None, None, None, None
    with torch.no_grad():
        c32 = coordinates.detach().to(torch.float32).contiguous()
        if isinstance(model, _Standalone):
            species32 = model._to_elem_idxs(species, True).to(torch.int32).contiguous()
            rows = model._standalone_rows(species32, c32, cell, pbc)
            if rows.overflowed():
                wrong = "its Hessian" if what == "Hessians" else "its strain derivatives"
                raise RuntimeError(f"{type(model).__name__}: an atom has more than {rows.row_cap} neighbors inside the "
                                   f"cutoff ({model.cutoff} A): {wrong} would be wrong")
            return _SecondOrderInputs(ef, species32, nnp, nbrs, eng, aev, packed, g, [(model, rows)])
        species32 = model._elem_idxs(species).to(torch.int32).contiguous()
        nnp = model.potentials["nnp"]._enabled
        if nnp or sparse:
            aevc = model.aev_computer
            nbrs = aevc.neighbor_rows(species32, c32, cell, pbc_tuple(pbc))
            nbrs.raise_on_overflow()
            eng = aevc.engine()
        if nnp:
            aev = eng.forward(species32, nbrs)
            packed = model.neural_networks._pack(coordinates.device)
            _, g, _ = packed.forward_backward(species32, aev, want_grad=True)
        if sparse:
            pairs = [(pot, nbrs) for pot in sparse_pots]
        else:
            pairs = _analytic_pair_rows(model, species32, c32, cell, pbc, nbrs)
    return _SecondOrderInputs(ef, species32, nnp, nbrs, eng, aev, packed, g, pairs)


def energies_forces_and_hessians(model, species: Tensor, coordinates: Tensor, retain_graph: bool = False, *,
                                 cell: tp.Optional[Tensor] = None,
                                 pbc: tp.Optional[Tensor] = None) -> EnergiesForcesHessians:
    """EnergiesForcesHessians(energies, forces, hessians [C, 3A, 3A]) of a model, batched (grad.py:239-260 computes the
    same through 3A autograd products).  The neighbor rows, AEVs and d E / d aev are computed once; then unit direction j
    (atom j // 3, component j % 3 of EVERY molecule of the batch at once) runs through anihip_aev_jvp_batched,
    anihip_mlp_input_hvp, anihip_aev_backward_second and, per enabled closed-form pair potential,
    anihip_pair_analytic_hvp, in chunks of K = hessian_chunk_size(...) directions: ceil(3A / K) calls per stage.  A
    standalone pair potential (``torchani_amd.potentials``) may stand in for the model, on its own rows.  Energies and
    forces are those of grad.energies_and_forces.  Results are detached (any model: frozen or trainable parameters);
    ``retain_graph`` is accepted for the reference's signature."""
    inp = _second_order_inputs(model, species, coordinates, cell, pbc, "Hessians")
    H = _dense_hessian_columns(inp, coordinates.device)
    return EnergiesForcesHessians(inp.ef.energies, inp.ef.forces, H.to(coordinates.dtype))


def _dense_hessian_columns(inp: _SecondOrderInputs, device: torch.device) -> Tensor:
    """The direction loop of energies_forces_and_hessians on what _second_order_inputs computed: float32 [C, 3A, 3A], the
    unit directions in chunks of hessian_chunk_size(...) through the second-order kernels (shared with
    geomopt.SaddleOptimizer, which wants the Hessian at its own coordinates)."""
    _, species32, nnp, nbrs, eng, aev, packed, g, pairs = inp
    with torch.no_grad():
        Cn, A = species32.shape
        N = Cn * A
        if nnp:
            row_bytes = -(-_hvp_row_bytes(packed, N) // N)
            K = hessian_chunk_size(Cn, A, eng.L, row_bytes)
        else:
            K = hessian_chunk_size(Cn, A, 0, 0)
        n = 3 * A
        H = torch.zeros((Cn, n, n), dtype=torch.float32, device=device)
        mol0 = torch.arange(Cn, device=device) * A
        for j0 in range(0, n, K):
            j1 = min(n, j0 + K)
            k = torch.arange(j1 - j0, device=device)
            t = torch.zeros((j1 - j0, N, 3), dtype=torch.float32, device=device)
            jj = k + j0
            t[k.view(-1, 1), (mol0.view(1, -1) + (jj // 3).view(-1, 1)), (jj % 3).view(-1, 1)] = 1.0
            if nnp:
                daev = eng.jvp_batched(species32, nbrs, t)
                hv = packed.input_hvp(species32, aev, daev.view(j1 - j0, N, eng.L))
                del daev
                out = eng.backward_second(species32, nbrs, g, t, hv)   # [K, N, 3]: columns j0..j1 of every molecule
                del hv
            else:
                out = torch.zeros_like(t)
            for pot, rows in pairs:
                pot.hvp(species32, rows, t, out)
            H[:, :, j0:j1] = out.view(j1 - j0, Cn, n).permute(1, 2, 0)
    return H


def _sparse_hessian_pairs(model) -> tp.List[tp.Any]:
    """The enabled closed-form pair potentials of a model, for energies_forces_and_sparse_hessians: each must reach no
    further than the AEV radial cutoff (its pairs then sit in the AEV's rows and its Hessian in their pattern)."""
    rc = float(model.aev_computer.radial.cutoff)
    out = []
    for name, pot in model.potentials.items():
        if name == "nnp" or not pot._enabled:
            continue
        if math.isinf(pot.cutoff) or pot.cutoff > rc + 1e-6:
            raise ValueError(f"pair potential {name!r} ({type(pot).__name__}) has cutoff {pot.cutoff} A, beyond the AEV radial "
                             f"cutoff {rc} A: its Hessian is dense, use grad.energies_forces_and_hessians")
        out.append(pot)
    return out


def sparse_hessian_chunks(roff_host, n_rows_budget: int, max_atoms: int) -> tp.List[tp.Tuple[int, int]]:
    """Direction-atom ranges [n0, n1) of energies_forces_and_sparse_hessians: each holds at most n_rows_budget item rows
    (3 |R(a)| per atom a; at least one atom per chunk) and at most max_atoms atoms; ranges without rows are dropped."""
    import numpy as np

    cum = 3 * np.asarray(roff_host, dtype=np.int64)
    N = cum.size - 1
    out = []
    n0 = 0
    while n0 < N:
        n1 = int(np.searchsorted(cum, cum[n0] + n_rows_budget, side="right")) - 1
        n1 = max(n0 + 1, min(n1, n0 + max_atoms, N))
        if cum[n1] > cum[n0]:
            out.append((n0, n1))
        n0 = n1
    return out


def energies_forces_and_sparse_hessians(model, species: Tensor, coordinates: Tensor, *, cell: tp.Optional[Tensor] = None,
                                        pbc: tp.Optional[Tensor] = None) -> EnergiesForcesSparseHessians:
    """EnergiesForcesSparseHessians(energies, forces, hessians: BlockHessian) of a model: the Hessian with respect to the
    coordinates as 3 x 3 blocks over the pattern P(a) = U_{i in R(a)} R(i), R(i) = {i} U the neighbor row of i (ANI is
    local: no other block can be non-zero).  Unit direction (atom a, component c) is worked on the item rows (direction,
    i), i in R(a), only: anihip_aev_jvp_items, anihip_mlp_rows_hvp (activations computed once per call),
    anihip_aev_backward_second_items and anihip_pair_analytic_hvp_items scatter into a [K, N, 3] scratch zeroed once, and
    anihip_hess_sparse_extract moves each chunk's pattern blocks out and zeroes exactly those positions.  Chunks of
    direction atoms hold at most HESSIAN_BUDGET_BYTES of item-row buffers.  Energies and forces are those of
    grad.energies_and_forces; the blocks are float32 and agree with energies_forces_and_hessians to fp32 rounding.

    Covered: the networks plus closed-form pair potentials whose cutoff is at most the AEV radial cutoff (ANI-1x, ANI-2x,
    ANI-2xr), both envelopes, any AEV grid, PBC, batches.  A larger or infinite pair cutoff (ANI-r2s) raises ValueError;
    D3 (ANI-2dr) raises NotImplementedError; standalone pair potentials are not served."""
    import numpy as np

    from .engine import hessian_extract, hessian_items, hessian_pattern
    from .potentials import _Standalone

    if isinstance(model, _Standalone):
        raise NotImplementedError("sparse Hessians are not available for a standalone pair potential: use "
                                  "grad.energies_forces_and_hessians")
    ef, species32, nnp, nbrs, eng, aev, packed, g, pairs = _second_order_inputs(model, species, coordinates, cell, pbc,
                                                                                "Hessians", sparse=True)
    dev = coordinates.device
    with torch.no_grad():
        Cn, A = species32.shape
        N = Cn * A
        pat = hessian_pattern(species32, nbrs)
        per_row = 8
        if nnp:
            per_row += 8 * eng.L + packed.rows_hvp_row_bytes(N)
        max_r = int(np.diff(pat.roff_host).max()) if N else 0
        budget = max(HESSIAN_BUDGET_BYTES // per_row, 3 * max_r)
        chunks = sparse_hessian_chunks(pat.roff_host, budget, max(1, HESSIAN_BUDGET_BYTES // (36 * max(N, 1))))
        blocks = torch.zeros((pat.nnz, 3, 3), dtype=torch.float32, device=dev)
        if chunks:
            rows_max = max(3 * int(pat.roff_host[n1] - pat.roff_host[n0]) for n0, n1 in chunks)
            K = max(3 * (n1 - n0) for n0, n1 in chunks)
            scratch = torch.zeros((K, N, 3), dtype=torch.float32, device=dev)
            ws = packed.rows_hvp_prepare(species32, aev, rows_max) if nnp else None
            S = int(eng.params.num_species)
            for n0, n1 in chunks:
                row_atom, row_dir = hessian_items(species32, pat, S, n0, n1)
                if nnp:
                    daev = eng.jvp_items(species32, nbrs, row_atom, row_dir)
                    hv = packed.rows_hvp(species32, ws, row_atom, daev)
                    del daev
                    eng.backward_second_items(species32, nbrs, g, row_atom, row_dir, 3 * n0, hv, scratch)
                    del hv
                for pot, rows in pairs:
                    pot.hvp_items(species32, rows, row_atom, row_dir, 3 * n0, scratch)
                hessian_extract(pat, n0, n1, scratch, blocks)
    return EnergiesForcesSparseHessians(ef.energies, ef.forces, BlockHessian(pat.index, blocks, Cn, A))


def strain_hessian_chunk_atoms(aev_len: int, hvp_row_bytes: int, budget: int = HESSIAN_BUDGET_BYTES) -> int:
    """Atoms per chunk of energies_forces_and_strain_hessians (9 item rows each) from the memory budget: per row its
    row_atom / row_dir, J d', H_net J d' and the gathered d E / d aev (aev_len floats each) and the network HVP workspace."""
    return int(max(1, budget // (9 * (8 + 12 * aev_len + hvp_row_bytes))))


def energies_forces_and_strain_hessians(model, species: Tensor, coordinates: Tensor, *, cell: tp.Optional[Tensor] = None,
                                        pbc: tp.Optional[Tensor] = None) -> EnergiesForcesStrainHessians:
    """EnergiesForcesStrainHessians(energies, forces, virial, strain_hessians, internal_strain) of a model: the second
    derivatives of E(x S, cell S) with respect to the strain S (coordinates are row vectors; x -> x S, cell -> cell S) at
    S = I, per molecule:

    * virial [C, 3, 3] = d E_c / d S_ab;
    * strain_hessians [C, 3, 3, 3, 3] = d^2 E_c / d S_ab d S_pq, all 81 components (rotations included);
    * internal_strain [C, A, 3, 3, 3] = d^2 E_c / d x_iy d S_ab, x the unstrained coordinates.

    Only 9 directions, whatever the number of atoms: the item rows (k, i), k = 3 a + b in 0 .. 8 over every real atom i,
    run through anihip_aev_jvp_strain_items, anihip_mlp_rows_hvp (activations computed once per call) and
    anihip_aev_backward_second_strain_items, in chunks of atoms (rows of a species contiguous) holding at most
    HESSIAN_BUDGET_BYTES of row buffers; each enabled closed-form pair potential adds anihip_pair_analytic_hvp_strain on the
    rows its forward uses.  The kernels give the strained-frame mixed derivative K; internal_strain adds
    delta_ya (d E / d x_i)_b from the forces.  Molecules without a cell are allowed (S then scales the coordinates).  A
    standalone pair potential may stand in for the model.  Energies and forces are those of grad.energies_and_forces;
    results are detached, in the coordinates' dtype.  D3 (ANI-2dr) raises NotImplementedError."""
    ef, species32, nnp, nbrs, eng, aev, packed, g, pairs = _second_order_inputs(model, species, coordinates, cell, pbc,
                                                                                "strain second derivatives")
    dev = coordinates.device
    with torch.no_grad():
        Cn, A = species32.shape
        N = Cn * A
        out = torch.zeros((9, N, 3), dtype=torch.float32, device=dev)
        ss = torch.zeros((Cn, 9, 9), dtype=torch.float64, device=dev)
        vir = torch.zeros((Cn, 9), dtype=torch.float64, device=dev)
        if nnp and N:
            flat = species32.view(-1)
            real = torch.nonzero(flat >= 0).view(-1)
            atoms = real[torch.argsort(flat[real], stable=True)].to(torch.int32)   # (rows of a species contiguous)
            g = g.reshape(N, eng.L)
            chunk = strain_hessian_chunk_atoms(eng.L, packed.rows_hvp_row_bytes(N), HESSIAN_BUDGET_BYTES)
            n_real = atoms.numel()
            ws = packed.rows_hvp_prepare(species32, aev, 9 * min(chunk, max(n_real, 1)))
            dirs = torch.arange(9, dtype=torch.int32, device=dev)
            for a0 in range(0, n_real, chunk):
                at = atoms[a0:a0 + chunk]
                row_atom = at.repeat_interleave(9)
                row_dir = dirs.repeat(at.numel())
                daev = eng.jvp_strain_items(species32, nbrs, row_atom, row_dir)
                # d E_i / d S_k = g_i . d aev_i / d S_k: the per-molecule virial of the networks
                ra = row_atom.long()
                dE = (daev * g.index_select(0, ra)).sum(dim=1)
                vir.view(-1).index_add_(0, (ra // A) * 9 + row_dir.long(), dE.double())
                del dE
                hv = packed.rows_hvp(species32, ws, row_atom, daev)
                del daev
                eng.backward_second_strain_items(species32, nbrs, g, row_atom, row_dir, hv, out, ss)
                del hv
        for pot, rows in pairs:
            pot.hvp_strain(species32, rows, out, ss, vir)
        dt = coordinates.dtype
        K = out.view(3, 3, Cn, A, 3).permute(2, 3, 4, 0, 1).to(dt)   # [C, A, y, a, b]
        dEdx = -ef.forces.detach().to(dt)
        eye = torch.eye(3, dtype=dt, device=dev)
        internal = K + eye.view(1, 1, 3, 3, 1) * dEdx.view(Cn, A, 1, 1, 3)
        return EnergiesForcesStrainHessians(ef.energies, ef.forces, vir.view(Cn, 3, 3).to(dt),
                                            ss.view(Cn, 3, 3, 3, 3).to(dt), internal.contiguous())


# Voigt order of elastic_constants: xx, yy, zz, yz, xz, xy
VOIGT_PAIRS = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))


def voigt_projector(dtype: torch.dtype = torch.float64, device: tp.Optional[torch.device] = None) -> Tensor:
    """P [6, 9]: a symmetric strain in Voigt form (engineering shears, e_4 = 2 eps_yz) as the 9 components S_ab it moves,
    so that d^2 E / d e_I d e_J = P W P^T for W = d^2 E / d S d S [9, 9]."""
    P = torch.zeros((6, 9), dtype=dtype, device=device)
    for I, (a, b) in enumerate(VOIGT_PAIRS):
        if a == b:
            P[I, 3 * a + a] = 1.0
        else:
            P[I, 3 * a + b] = 0.5
            P[I, 3 * b + a] = 0.5
    return P


def _translations(active: Tensor) -> Tensor:
    """Orthonormal rigid translations [C, 3A, 3] over the active atoms [C, A] (zero on the others)."""
    Cn, A = active.shape
    w = active.to(torch.float64)
    w = w / w.sum(dim=1, keepdim=True).clamp(min=1.0).sqrt()
    T = torch.zeros((Cn, A, 3, 3), dtype=torch.float64, device=active.device)
    for y in range(3):
        T[:, :, y, y] = w
    return T.view(Cn, 3 * A, 3)


def elastic_constants(result: EnergiesForcesStrainHessians, cell: Tensor, *, hessians: tp.Optional[Tensor] = None,
                      relaxed: bool = False, unit: str = "GPa", pbc: tp.Optional[Tensor] = None) -> Tensor:
    """Elastic constants [C, 6, 6] in Voigt order xx, yy, zz, yz, xz, xy (engineering shears) from
    energies_forces_and_strain_hessians.  Full pbc only: a missing cell, or a ``pbc`` with a non-periodic direction, raises
    ValueError (``pbc`` None: the cell is taken as periodic in all three directions).

    Clamped-ion (Born) constants: (1/V) P W P^T with W = strain_hessians [9, 9] and P = voigt_projector().  With
    ``relaxed=True`` the internal relaxation is subtracted: C - Xi^T H^+ Xi / V, where Xi [3A, 6] is the strained-frame mixed
    derivative (internal_strain minus its force term delta_ya (d E / d x_i)_b) projected on symmetric strain and H is the
    dense Hessian [C, 3A, 3A] ``hessians`` (e.g. grad.energies_forces_and_hessians(...).hessians).  H^+ is the pseudo-inverse
    in fp64 on the complement of the three rigid translations of the atoms H or Xi touch (padding atoms are left out).

    These are second derivatives of the energy.  At a non-zero stress they differ from the stress-strain coefficients by
    terms in the stress, and a relaxed-ion value is only meaningful at a relaxed geometry (zero forces, H positive
    semidefinite on the complement of the translations).  unit: "GPa" or "Hartree/A^3"."""
    if cell is None:
        raise ValueError("elastic constants need a periodic cell")
    if pbc is not None and not bool(torch.as_tensor(pbc).all()):
        raise ValueError("elastic constants need periodic boundary conditions in all three directions")
    if unit == "GPa":
        scale = _units.HARTREE_PER_ANGSTROM3_TO_GPA
    elif unit in ("Hartree/A^3", "hartree/angstrom^3"):
        scale = 1.0
    else:
        raise ValueError(f"unknown unit {unit!r}: 'GPa' or 'Hartree/A^3'")
    W = result.strain_hessians.detach().to(torch.float64)
    Cn = W.shape[0]
    dev = W.device
    cell64 = cell.detach().to(device=dev, dtype=torch.float64)
    if cell64.dim() == 2:
        cell64 = cell64.unsqueeze(0).expand(Cn, 3, 3)
    V = torch.linalg.det(cell64).abs()
    if bool((V <= 0).any()):
        raise ValueError("the cell has zero volume")
    P = voigt_projector(torch.float64, dev)
    Wf = W.reshape(Cn, 9, 9)
    out = P @ Wf @ P.T / V.view(Cn, 1, 1)
    if relaxed:
        if hessians is None:
            raise ValueError("relaxed=True needs the dense Hessian: pass hessians=energies_forces_and_hessians(...).hessians")
        A = result.internal_strain.shape[1]
        H = hessians.detach().to(device=dev, dtype=torch.float64)
        if H.shape != (Cn, 3 * A, 3 * A):
            raise ValueError(f"hessians must be [{Cn}, {3 * A}, {3 * A}]")
        H = 0.5 * (H + H.transpose(1, 2))
        eye = torch.eye(3, dtype=torch.float64, device=dev)
        F = result.forces.detach().to(device=dev, dtype=torch.float64)
        K = result.internal_strain.detach().to(torch.float64) + eye.view(1, 1, 3, 3, 1) * F.view(Cn, A, 1, 1, 3)
        Xi = K.reshape(Cn, 3 * A, 9) @ P.T   # [C, 3A, 6]
        active = (H.view(Cn, A, 3, 3 * A).abs().sum(dim=(2, 3)) > 0) | (Xi.view(Cn, A, 18).abs().sum(dim=2) > 0)
        T = _translations(active)
        Pr = torch.eye(3 * A, dtype=torch.float64, device=dev).unsqueeze(0) - T @ T.transpose(1, 2)
        Hp = Pr @ H @ Pr
        lam, U = torch.linalg.eigh(Hp)
        big = lam.abs().amax(dim=1, keepdim=True)
        keep = lam.abs() > 1e-10 * big.clamp(min=torch.finfo(torch.float64).tiny)
        inv = torch.where(keep, 1.0 / torch.where(keep, lam, torch.ones_like(lam)), torch.zeros_like(lam))
        X = Pr @ Xi
        UX = U.transpose(1, 2) @ X
        out = out - (UX.transpose(1, 2) @ (inv.unsqueeze(2) * UX)) / V.view(Cn, 1, 1)
    return out * scale


def _hvp_row_bytes(packed, n_rows: int) -> int:
    """Workspace bytes of ONE direction of anihip_mlp_input_hvp over n_rows atoms (the query is linear in the directions)."""
    import ctypes

    from . import _lib

    L = _lib.lib()
    one = L.anihip_mlp_input_hvp_workspace_bytes(ctypes.byref(packed.desc), n_rows, 1)
    two = L.anihip_mlp_input_hvp_workspace_bytes(ctypes.byref(packed.desc), n_rows, 2)
    return max(int(two - one), 1)


def vibrational_analysis(masses: Tensor, hessian: Tensor, mode_kind: str = "mdu", unit: str = "cm^-1") -> VibAnalysis:
    """Harmonic frequencies, normal modes, force constants and reduced masses of ONE molecule (grad.py:153-236).

    masses [1, A] (amu), hessian [1, 3A, 3A] (Hartree / Angstrom^2).  The generalized eigenproblem H q = w^2 T q
    (T = the masses on the diagonal, three times each) is solved as the symmetric problem T^-1/2 H T^-1/2 q' = w^2 q'.
    mode_kind: "mdu" mass-deweighted unnormalized (ASE), "mdn" mass-deweighted normalized (Gaussian, ORCA), "mwn"
    mass-weighted normalized.  Imaginary frequencies come out negative.  Force constants (mDyne / Angstrom) and reduced
    masses (amu) as in Gaussian.  unit: "cm^-1" or "meV"."""
    to_unit = _freq_unit(unit)
    assert hessian.shape[0] == 1, "Currently only supporting computing one molecule a time"
    w = masses.sqrt().reciprocal().repeat_interleave(3, dim=1)   # [1, 3A]
    mh = hessian[0] * w[0].unsqueeze(0) * w[0].unsqueeze(1)
    evals, evecs = torch.linalg.eigh(mh)
    # (row k of evecs^T = mass-weighted mode k, orthonormal)
    freqs, modes, fconstants, rmasses = _modes_outputs(evals[None], evecs.transpose(0, 1)[None], w, mode_kind, to_unit)
    return VibAnalysis(freqs[0], modes[0].reshape(evals.numel(), -1, 3), fconstants[0], rmasses[0])


def _freq_unit(unit: str):
    """The conversion of sqrt(eigenvalue) / (2 pi) to the frequency unit "cm^-1" or "meV"."""
    if unit == "cm^-1":
        return _units.sqrt_mhessian2invcm
    if unit == "meV":
        return _units.sqrt_mhessian2milliev
    raise ValueError("Only meV and cm^-1 are supported right now")


SPARSE_MODES_SEED = 20261015   # start vectors of sparse_vibrational_analysis (fixed: results repeat exactly)


def _modes_outputs(evals: Tensor, mw: Tensor, w: Tensor, mode_kind: str, to_unit):
    """vibrational_analysis's outputs from eigenvalues [C, k] and mass-weighted unit modes mw [C, k, 3A]; w [C, 3A] = m^-1/2
    (0 on padding)."""
    md = mw * w.unsqueeze(1)
    inv_norm = md.norm(dim=2).reciprocal()
    rmasses = inv_norm ** 2
    fconstants = _units.mhessian2fconst(evals) * rmasses
    kind = mode_kind.lower()
    if kind in ("mdn", "mass-deweighted-normalized"):
        modes = md * inv_norm.unsqueeze(2)
    elif kind in ("mdu", "mass-deweighted-unnormalized"):
        modes = md
    elif kind in ("mwn", "mass-weighted-normalized"):
        modes = mw
    else:
        raise ValueError(f"Incorrect mode kind {mode_kind}")
    freqs = to_unit(evals.abs().sqrt() / (2 * math.pi) * torch.sign(evals))
    return freqs, modes, fconstants, rmasses


def _rigid_basis(masses: Tensor, real: Tensor, coordinates: tp.Optional[Tensor], rotations: bool) -> Tensor:
    """[C, 3A, 6 or 3] mass-weighted rigid-body motions over the real atoms: sqrt(m_a) e_x and sqrt(m_a) e_x x (r_a - com)."""
    C, A = masses.shape
    sm = torch.where(real, masses, torch.zeros_like(masses)).sqrt()                     # [C, A]
    eye = torch.eye(3, dtype=masses.dtype, device=masses.device)
    vecs = [sm[:, :, None] * eye[x] for x in range(3)]                                  # [C, A, 3] each
    if rotations:
        m = sm ** 2
        r = coordinates.to(masses.dtype)
        com = (m.unsqueeze(2) * r).sum(1, keepdim=True) / m.sum(1, keepdim=True).clamp_min(1e-300).unsqueeze(2)
        d = (r - com) * real.unsqueeze(2)
        vecs += [sm.unsqueeze(2) * torch.cross(eye[x].expand_as(d), d, dim=2) for x in range(3)]
    return torch.stack([v.reshape(C, 3 * A) for v in vecs], dim=2)


def sparse_vibrational_analysis(masses: Tensor, hessian: BlockHessian, n_modes: int = 20, *, mode_kind: str = "mdu",
                                unit: str = "cm^-1", project_rigid: bool = False, coordinates: tp.Optional[Tensor] = None,
                                pbc: tp.Optional[Tensor] = None, tol: float = 1e-6, max_iter: int = 1000,
                                check: bool = True) -> SparseVibAnalysis:
    """The n_modes lowest normal modes of each molecule of a block-sparse Hessian (grad.energies_forces_and_sparse_hessians):
    the eigenproblem of vibrational_analysis, A = M^-1/2 ((H + H^T) / 2) M^-1/2 over each molecule's real atoms, solved
    without forming A.  masses [C, A] (amu).  A padding atom is one without a diagonal block: it is excluded and its mode
    components are zero; a real atom whose mass is not positive and finite raises ValueError.

    anihip_block_hessian_prepare turns the blocks into the operator once (symmetrized, mass-weighted, the Gershgorin bound
    ||A||_G of each molecule); modes.lobpcg then touches A only through anihip_block_hessian_spmm, one product for all
    molecules.  A molecule with at most 3 (n_modes + guard) degrees of freedom is solved densely on the device
    (modes.dense_eigenpairs).  Every pair must reach ||A q - theta q|| <= tol ||A||_G; otherwise RuntimeError after
    max_iter iterations, or with check=False the unconverged pairs are returned.

    project_rigid=True removes the rigid-body motions in mass-weighted space: the 3 translations, and the 3 rotations about
    the centre of mass when no axis of pbc is periodic (they need coordinates [C, A, 3]); the modes returned are the lowest
    orthogonal to them.  The default keeps the spectrum of vibrational_analysis, which does not project.  Outputs:
    tuples.SparseVibAnalysis (fp64; freqs, modes, fconstants and rmasses as vibrational_analysis, mode_kind and unit
    alike)."""
    from . import modes as _modes
    from .engine import _require_cuda, block_hessian_prepare, block_hessian_spmm

    to_unit = _freq_unit(unit)
    if mode_kind.lower() not in ("mdn", "mass-deweighted-normalized", "mdu", "mass-deweighted-unnormalized", "mwn",
                                 "mass-weighted-normalized"):
        raise ValueError(f"Incorrect mode kind {mode_kind}")
    if not isinstance(hessian, BlockHessian):
        raise TypeError("hessian must be a tuples.BlockHessian (grad.vibrational_analysis takes dense Hessians)")
    C, A = hessian.n_molecules, hessian.n_atoms
    if tuple(masses.shape) != (C, A):
        raise ValueError(f"masses must be [C, A] = [{C}, {A}], got {list(masses.shape)}")
    if n_modes < 1:
        raise ValueError("n_modes must be at least 1")
    if not tol > 0 or max_iter < 1:
        raise ValueError("tol must be positive and max_iter at least 1")
    periodic = pbc is not None and bool(torch.as_tensor(pbc).any())
    if project_rigid and not periodic and (coordinates is None or tuple(coordinates.shape) != (C, A, 3)):
        raise ValueError("project_rigid=True without periodic axes removes rotations: pass coordinates [C, A, 3]")
    _require_cuda(masses, hessian.index, hessian.blocks, coordinates)
    dev = masses.device
    N = C * A
    index, blocks = hessian.index, hessian.blocks
    with torch.no_grad():
        if hessian.nnz > 1:
            key = index[1] * N + index[0]
            unsorted, crossing = torch.stack([(key[1:] <= key[:-1]).any(), (index[0] // A != index[1] // A).any()]).tolist()
            if crossing:
                raise ValueError("BlockHessian blocks couple different molecules")
            if unsorted:   # a hand-built Hessian: put it in column order once (the engine's own output already is)
                order = torch.argsort(key)
                index, blocks = index[:, order], blocks[order]
        m64 = masses.detach().to(torch.float64)
        op = block_hessian_prepare(index, blocks, m64.reshape(-1))
        real = (op.diag >= 0).view(C, A)
        bad = real & ~(torch.isfinite(m64) & (m64 > 0))
        w_atom = torch.where(real & ~bad, m64.clamp_min(1e-300).rsqrt(), torch.zeros_like(m64))
        w = w_atom.repeat_interleave(3, dim=1)                                          # [C, 3A]
        bound = op.gersh.view(C, A).amax(dim=1)
        dofmask = w > 0
        R = None
        if project_rigid:
            R = _rigid_basis(m64, real, None if coordinates is None else coordinates.detach(), not periodic)
            R, _, _ = _modes.svqb(R)
            R, _, vr = _modes.svqb(R)
            n_rigid = vr.sum(dim=1)
        else:
            n_rigid = torch.zeros(C, dtype=torch.int64, device=dev)
        avail = 3 * real.sum(dim=1) - n_rigid
        any_bad, avail_h = bool(bad.any()), avail.cpu()
        if any_bad:
            raise ValueError("masses must be positive and finite on every real atom (an atom with a diagonal block)")
        if n_modes > int(avail_h.min()):
            raise ValueError(f"n_modes = {n_modes} exceeds the {int(avail_h.min())} degrees of freedom of a molecule")
        k = n_modes + max(4, n_modes // 4)
        dense = avail_h <= 3 * k
        sel_d = torch.nonzero(dense).reshape(-1).tolist()
        sel_l = torch.nonzero(~dense).reshape(-1).tolist()

        def operator(sel):
            full = len(sel) == C
            sel_t = torch.tensor(sel, dtype=torch.int64, device=dev)
            Rs = None if R is None else R[sel_t]

            def project(V):
                return V - Rs @ (Rs.transpose(1, 2) @ V)

            def apply(V):
                outs = []
                for c0 in range(0, V.shape[2], _modes.MAX_VECTORS):
                    Vc = V[:, :, c0:c0 + _modes.MAX_VECTORS]
                    if full:
                        X = Vc.to(torch.float32).contiguous()
                    else:
                        X = torch.zeros((C, 3 * A, Vc.shape[2]), dtype=torch.float32, device=dev)
                        X[sel_t] = Vc.to(torch.float32)
                    Y = block_hessian_spmm(op, X)
                    outs.append((Y if full else Y[sel_t]).to(torch.float64))
                return torch.cat(outs, dim=2)

            if Rs is None:
                return apply, None, sel_t
            return (lambda V: project(apply(project(V)))), project, sel_t

        evals = torch.zeros((C, n_modes), dtype=torch.float64, device=dev)
        vecs = torch.zeros((C, 3 * A, n_modes), dtype=torch.float64, device=dev)
        res = torch.zeros((C, n_modes), dtype=torch.float64, device=dev)
        n_iter = 0
        if sel_d:
            apply, project, sel_t = operator(sel_d)
            mask = dofmask[sel_t]
            rank = torch.cumsum(mask.to(torch.int64), dim=1) - 1
            d = int(mask.sum(dim=1).max())
            E = torch.zeros((len(sel_d), 3 * A, d), dtype=torch.float64, device=dev)
            ci, ii = torch.nonzero(mask, as_tuple=True)
            E[ci, ii, rank[ci, ii]] = 1.0
            if project is not None:
                E = project(E)
            r = _modes.dense_eigenpairs(apply, E, n_modes, bound[sel_t])
            evals[sel_t], vecs[sel_t], res[sel_t] = r.eigenvalues, r.vectors, r.residuals
        if sel_l:
            apply, project, sel_t = operator(sel_l)
            g = torch.Generator(device=dev).manual_seed(SPARSE_MODES_SEED)
            X0 = torch.randn((len(sel_l), 3 * A, k), dtype=torch.float64, device=dev, generator=g)
            X0 = X0 * dofmask[sel_t].unsqueeze(2)
            r = _modes.lobpcg(apply, X0, n_modes, tol * bound[sel_t], bound[sel_t], max_iter, project=project)
            evals[sel_t], vecs[sel_t] = r.eigenvalues[:, :n_modes], r.vectors[:, :, :n_modes]
            res[sel_t] = r.residuals[:, :n_modes]
            n_iter = r.n_iter
        if check:
            rel = (res / bound.clamp_min(1e-300).unsqueeze(1)).max(dim=1).values
            worst = int(rel.argmax())
            if float(rel[worst]) > tol:
                raise RuntimeError(f"sparse_vibrational_analysis did not converge in max_iter = {max_iter} iterations: worst "
                                   f"residual {float(res[worst].max()):.3e} = {float(rel[worst]):.2e} ||A||_G in molecule "
                                   f"{worst} (tol {tol:g}); raise max_iter or pass check=False")
        mw = vecs.transpose(1, 2)
        freqs, modes, fconstants, rmasses = _modes_outputs(evals, mw, w, mode_kind, to_unit)
    return SparseVibAnalysis(freqs, modes.reshape(C, n_modes, A, 3), fconstants, rmasses, evals, res, n_iter)


def energies_and_forces(model, species: Tensor, coordinates: Tensor, cell: tp.Optional[Tensor] = None,
                        pbc: tp.Optional[Tensor] = None, retain_graph: tp.Optional[bool] = None,
                        create_graph: bool = False, charge: int = 0, atomic: bool = False,
                        ensemble_values: bool = False, keep_vars: bool = True) -> EnergiesForces:
    """``EnergiesForces(energies, forces)`` through torch.autograd, restoring coordinates.requires_grad: the signature, the
    leaf check and the result of the reference (grad.py:263-290) -- ``retain_graph`` / ``create_graph`` go to the force
    derivative (``create_graph=True``: forces that can be trained on, tools/training-aev-benchmark.py:139-140), the energies
    keep their graph like the reference's.  A standalone pair potential (``torchani_amd.potentials``) is called as
    ``model(species, coordinates, cell, pbc)``.  The keywords behind ``create_graph`` are extensions of this package:
    ``atomic`` / ``ensemble_values`` are handed to the model, ``keep_vars=False`` detaches the energies."""
    from .potentials import _Standalone

    saved = coordinates.requires_grad
    coordinates.requires_grad_(True)
    if not coordinates.is_leaf:
        raise ValueError("'coordinates' passed to `torchani.grad` functions must be a 'leaf' Tensor"
                         "(i.e. must not have been modified prior to being used as an input).")
    if isinstance(model, _Standalone):
        energies = model(species, coordinates, cell, pbc)
    elif atomic or ensemble_values:
        energies = model((species, coordinates), cell, pbc, atomic=atomic, ensemble_values=ensemble_values).energies
    else:
        energies = model((species, coordinates), cell, pbc).energies
    f = forces(energies, coordinates, retain_graph=retain_graph, create_graph=create_graph)
    coordinates.requires_grad_(saved)
    if not keep_vars:
        energies = energies.detach()
    return EnergiesForces(energies, f)


def heat_flux(model, species: Tensor, coordinates: Tensor, velocities: Tensor, masses: tp.Optional[Tensor] = None,
              cell: tp.Optional[Tensor] = None, pbc: tp.Optional[Tensor] = None,
              include_self_energies: bool = False) -> HeatFlux:
    """The heat flux of an ANI model at one phase-space point, ``HeatFlux(total, kinetic, convective, virial, atomic)`` in
    Hartree Angstrom / fs (velocities in Angstrom / fs, masses in amu, by default the standard atomic weights).

    With eps_i = 1/2 m_i |v_i|^2 + e_i, differentiating sum_i r_i eps_i along the equations of motion gives
    J = sum_i eps_i v_i - sum_i q_i,  q_i = sum_{j in row i} d_ij (dE_i/d d_ij . v_j): ``kinetic`` and ``convective`` are the two
    halves of the first sum, ``virial`` is the second with its sign and ``atomic`` holds the rows q_i.  ANI is strictly local
    (E_i depends on the displacements of row i alone), so this is exact, needs no absolute positions and holds under periodic
    boundaries.  e_i is the ensemble-mean network output.  ``include_self_energies=True`` adds the self energy c_{s_i} to e_i,
    i.e. sum_i c_{s_i} v_i to the flux: in a one-component system that is a constant times the conserved momentum, in a mixture
    it is a gauge choice (it changes the flux but not the conductivity of a converged Green-Kubo integral), so it is off by
    default.  One extra evaluation of the model (networks forward and backward), no forces.

    Raises RuntimeError, like ``energies_and_forces``, if an atom has more neighbors than a row holds (one host read, none
    where no row can overflow): the builder zeroes such a row and the flux would be silently wrong.

    Refused: models with pair potentials (ANI-2xr, ANI-2dr, anything added from ``potentials``), whose pair halves have no
    flux kernel yet, and a program with more than one rank in torch.distributed's default group (every rank would evaluate
    the whole system)."""
    from .md import default_masses

    if not hasattr(model, "heat_flux_terms"):
        raise NotImplementedError(f"heat flux: {type(model).__name__} has no flux kernel (standalone pair potentials are pair "
                                  "potentials: only ANI network models are supported)")
    model._refuse_heat_flux()
    if masses is None:
        masses = torch.where(species >= 0, default_masses(model, species).to(torch.float32), torch.ones((), device=species.device))
    J, q = model.heat_flux_terms(species, coordinates, velocities, masses, cell, pbc, include_self_energies)
    if not model._overflow_impossible(species, cell, pbc_tuple(pbc)):
        model.last_flux_neighbors.raise_on_overflow()
    return HeatFlux(J.sum(dim=1), J[:, 0], J[:, 1], J[:, 2], q)


def single_point(model, species: Tensor, coordinates: Tensor, cell: tp.Optional[Tensor] = None,
                 pbc: tp.Optional[Tensor] = None, charge: int = 0, forces: bool = False, hessians: bool = False,
                 atomic_energies: bool = False, atomic_charges: bool = False, atomic_charges_grad: bool = False,
                 ensemble_values: bool = False, keep_vars: bool = False) -> tp.Dict[str, Tensor]:
    """Properties of a batch of molecules as a dictionary (grad.py:293-399): energies, optional forces, atomic
    energies, and -- with ensemble_values -- the member values, their standard deviation and the QBC factors."""
    if hessians:
        _no_hessians()
    if atomic_charges_grad:
        raise NotImplementedError("atomic charges carry no gradient here (the charge networks run the inference kernels)")
    if forces and ensemble_values:
        raise NotImplementedError("forces of ensemble_values=True are not differentiable in the HIP engine")
    saved = coordinates.requires_grad
    if forces:
        coordinates.requires_grad_(True)
    result = model((species, coordinates), cell, pbc, atomic=atomic_energies, ensemble_values=ensemble_values)
    energies = result.energies
    out: tp.Dict[str, Tensor] = {}
    if atomic_charges:   # (ANIq models: models.ANImbis, models.simple_aniq)
        if not hasattr(result, "atomic_charges"):
            coordinates.requires_grad_(saved)
            raise ValueError("Model doesn't support atomic charges")
        out["atomic_charges"] = result.atomic_charges
    if ensemble_values:
        if atomic_energies:
            out["atomic_energies"] = energies.mean(dim=0)
            values = energies.sum(dim=-1)
        else:
            values = energies
        out["energies"] = values.mean(dim=0)
        single = values.shape[0] == 1
        out["ensemble_std"] = values.new_zeros(energies.shape) if single else values.std(dim=0, unbiased=True)
        out["ensemble_values"] = values
        qbc = values.new_zeros(values.shape).squeeze(0) if single else values.std(0, unbiased=True)
        out["qbcs"] = qbc / (species >= 0).sum(dim=1, dtype=energies.dtype).sqrt()
    elif atomic_energies:
        out["energies"] = energies.sum(dim=-1)
        out["atomic_energies"] = energies
    else:
        out["energies"] = energies
    if forces:
        out["forces"] = calc_forces(out["energies"], coordinates)
    coordinates.requires_grad_(saved)
    if not keep_vars:
        out = {k: v.detach() for k, v in out.items()}
    return out
