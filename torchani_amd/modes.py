"""Lowest eigenpairs of batched symmetric operators: the solver of grad.sparse_vibrational_analysis.

The operator is any callable ``op(X) -> A X`` on fp64 blocks of vectors ``X [C, n, m]`` (one symmetric A per molecule, the
molecules independent); on the HIP engine it is anihip_block_hessian_spmm, in the host tests a dense matrix.  ``lobpcg``
is the locally optimal block preconditioned conjugate gradient method (Knyazev 2001) in its orthogonal-basis form
(Hetmaniuk and Lehoucq 2006): the Rayleigh-Ritz step works on [X, W, P] with W and P orthonormalized against X and
each other, so the projected problem is a standard one.  Every molecule of the batch runs in the same fp64 batched matrices;
a direction that orthonormalization drops (a locked residual, a rank-deficient block) keeps its column as zeros and gets
a penalty on the projected diagonal above the spectrum (``bound``), so it is never selected and the shapes never change.

* Orthonormalization: SVQB (Stathopoulos and Wu 2002), twice, dropping singular values below 1e-7 of the largest.
* Soft locking: a pair whose residual is within tolerance adds no new direction but stays in the Rayleigh-Ritz basis.
* Convergence is checked on the host every ``check_every`` iterations, after A X is recomputed from X (the implicit update of
  A X drifts); the check is the only synchronization of an iteration.
* ``dense_eigenpairs`` is the route of molecules too small for a block method: Rayleigh-Ritz on the whole space.
"""
from __future__ import annotations

import typing as tp

import torch
from torch import Tensor

Op = tp.Callable[[Tensor], Tensor]
DROP = 1e-7          # SVQB: singular values below DROP x the largest are dropped (a Gram matrix resolves ~1e-8)
CHECK_EVERY = 5
SLAB = 4096          # rows per slab of the Gram products
MAX_VECTORS = 64     # columns per operator call (ANIHIP_BLOCK_HESSIAN_MAX_VECTORS)


def _bt(a: Tensor, b: Tensor) -> Tensor:
    """a^T b [C, p, q] of a [C, n, p], b [C, n, q]: for long n in slabs of SLAB rows, summed in a fixed order (a GEMM with
    a long inner dimension and a small output has little parallelism)."""
    C, n, p = a.shape
    if n <= 2 * SLAB:
        return a.transpose(1, 2) @ b
    nb = -(-n // SLAB)
    pad = nb * SLAB - n
    if pad:
        a = torch.nn.functional.pad(a, (0, 0, 0, pad))
        b = torch.nn.functional.pad(b, (0, 0, 0, pad))
    q = b.shape[2]
    return (a.reshape(C * nb, SLAB, p).transpose(1, 2) @ b.reshape(C * nb, SLAB, q)).view(C, nb, p, q).sum(dim=1)


def svqb(Z: Tensor, AZ: tp.Optional[Tensor] = None) -> tp.Tuple[Tensor, tp.Optional[Tensor], Tensor]:
    """Orthonormal columns spanning Z [C, n, p] (AZ transformed alike): (Z', AZ', valid [C, p]); dropped columns are zero."""
    M = _bt(Z, Z)
    d = torch.diagonal(M, dim1=1, dim2=2)
    dmax = d.amax(dim=1, keepdim=True)
    keep = d > (DROP * DROP) * dmax.clamp_min(1e-300)
    D = torch.where(keep, d.clamp_min(1e-300).rsqrt(), torch.zeros_like(d))
    lam, V = torch.linalg.eigh(M * D.unsqueeze(2) * D.unsqueeze(1))
    valid = lam > DROP * DROP * lam.amax(dim=1, keepdim=True).clamp_min(1e-300)
    s = torch.where(valid, lam.clamp_min(1e-300).rsqrt(), torch.zeros_like(lam))
    T = D.unsqueeze(2) * V * s.unsqueeze(1)
    return Z @ T, (None if AZ is None else AZ @ T), valid


def _orth_against(Z: Tensor, AZ: tp.Optional[Tensor], bases: tp.Sequence[tp.Tuple[Tensor, tp.Optional[Tensor]]]):
    for Q, AQ in bases:
        c = _bt(Q, Z)
        Z = Z - Q @ c
        if AZ is not None:
            AZ = AZ - AQ @ c
    return Z, AZ


def _rayleigh_ritz(S: Tensor, AS: Tensor, valid: Tensor, bound: Tensor, k: int):
    G = _bt(S, AS)
    G = 0.5 * (G + G.transpose(1, 2))
    pen = torch.where(valid, torch.zeros_like(G[:, :, 0]), (4.0 * bound + 1.0).unsqueeze(1).expand_as(valid))
    G = G + torch.diag_embed(pen)
    theta, Y = torch.linalg.eigh(G)
    return theta[:, :k], Y[:, :, :k]


class Result(tp.NamedTuple):
    eigenvalues: Tensor   # [C, k] fp64, ascending
    vectors: Tensor       # [C, n, k] fp64, orthonormal
    residuals: Tensor     # [C, k] ||A x - theta x||, from an explicit product
    n_iter: int


def dense_eigenpairs(op: Op, basis: Tensor, k: int, bound: Tensor, max_cols: int = MAX_VECTORS) -> Result:
    """The k lowest eigenpairs of A restricted to the span of basis [C, n, d] (orthonormalized here; A is applied in
    groups of max_cols columns)."""
    E, _, _ = svqb(basis)
    E, _, valid = svqb(E)
    AE = torch.cat([op(E[:, :, c:c + max_cols].contiguous()) for c in range(0, E.shape[2], max_cols)], dim=2)
    theta, Y = _rayleigh_ritz(E, AE, valid, bound, k)
    X, AX = E @ Y, AE @ Y
    X, AX = _fix_signs(X, AX)
    AX = op(X)
    return Result(theta, X, (AX - X * theta.unsqueeze(1)).norm(dim=1), 0)


def _fix_signs(X: Tensor, AX: Tensor) -> tp.Tuple[Tensor, Tensor]:
    """Each vector's largest component positive (the first of equal ones): the output does not depend on the start."""
    i = X.abs().argmax(dim=1, keepdim=True)
    s = torch.where(torch.gather(X, 1, i) < 0, -1.0, 1.0).to(X.dtype)
    return X * s, AX * s


def lobpcg(op: Op, X0: Tensor, n_want: int, tol: Tensor, bound: Tensor, max_iter: int, *,
           precond: tp.Optional[Op] = None, project: tp.Optional[Op] = None, check_every: int = CHECK_EVERY) -> Result:
    """The k = X0.shape[2] lowest eigenpairs of the operators (the first n_want of which must converge: the rest are guard
    vectors).  X0 [C, n, k] start vectors (zero where a molecule has no degrees of freedom), tol [C] the absolute residual
    tolerances, bound [C] an upper bound of |A| (the Gershgorin bound).  precond(R) and project(V) map [C, n, m] blocks:
    project restricts the search to a subspace that op preserves.  Returns after the first check at which the n_want lowest
    residuals are within tol, or after max_iter iterations (converged or not: the caller judges the residuals)."""
    k = X0.shape[2]
    tol = tol.to(X0.dtype)
    bound = bound.to(X0.dtype)
    X = X0 if project is None else project(X0)
    X, _, _ = svqb(X)
    X, _, vx = svqb(X)
    AX = op(X)
    theta, Y = _rayleigh_ritz(X, AX, vx, bound, k)
    X, AX = X @ Y, AX @ Y
    P = AP = None
    it = 0
    while True:
        R = AX - X * theta.unsqueeze(1)
        rn = R.norm(dim=1)
        if it % check_every == 0 or it >= max_iter:
            # X re-orthonormalized and its product made explicitly: the residuals checked are those of X itself
            X, _, vx = svqb(X)
            AX = op(X)
            theta, Y = _rayleigh_ritz(X, AX, vx, bound, k)
            X, AX = _fix_signs(X @ Y, AX @ Y)
            R = AX - X * theta.unsqueeze(1)
            rn = R.norm(dim=1)
            if it >= max_iter or bool((rn[:, :n_want] <= tol.unsqueeze(1)).all()):
                return Result(theta, X, rn, it)
        it += 1
        W = R * (rn > tol.unsqueeze(1)).unsqueeze(1).to(R.dtype)   # soft locking
        if precond is not None:
            W = precond(W)
        if project is not None:
            W = project(W)
        W, _ = _orth_against(W, None, [(X, None)])
        W, _, _ = svqb(W)
        W, _ = _orth_against(W, None, [(X, None)])
        W, _, vw = svqb(W)
        AW = op(W)
        if P is None:
            S, AS, valid = torch.cat([X, W], 2), torch.cat([AX, AW], 2), torch.cat([torch.ones_like(vx), vw], 1)
        else:
            P, AP = _orth_against(P, AP, [(X, AX), (W, AW)])
            P, AP, _ = svqb(P, AP)
            P, AP = _orth_against(P, AP, [(X, AX), (W, AW)])
            P, AP, vp = svqb(P, AP)
            S, AS = torch.cat([X, W, P], 2), torch.cat([AX, AW, AP], 2)
            valid = torch.cat([torch.ones_like(vx), vw, vp], 1)
        theta, Y = _rayleigh_ritz(S, AS, valid, bound, k)
        X, AX = S @ Y, AS @ Y
        P, AP = S[:, :, k:] @ Y[:, k:], AS[:, :, k:] @ Y[:, k:]
