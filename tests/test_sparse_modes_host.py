"""Host-side parts of the lowest normal modes of block-sparse Hessians (no GPU): the C declarations of the new entry points
against the ctypes symbol list, the solver of torchani_amd.modes on dense CPU operators with known spectra against
numpy.linalg.eigh, a torch reference of the operator's symmetrized, mass-weighted blocks on the hand-built batch with
padding of test_sparse_hessians_host.py, and the argument errors of grad.sparse_vibrational_analysis."""
import os
import re

import numpy as np
import pytest
import torch

from test_sparse_hessians_host import _hand_built

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("anihip_block_hessian_prepare", "anihip_block_hessian_spmm")


def test_header_declares_the_mode_entry_points():
    from torchani_amd import _lib

    with open(os.path.join(ROOT, "include", "anihip.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(anihip_\w+)\s*\(", src))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS
    assert "hess_modes.hip" in _lib.SOURCES
    assert _lib.ABI_VERSION == 13
    assert re.search(r"#define ANIHIP_BLOCK_HESSIAN_MAX_VECTORS (\d+)", src).group(1) == str(_lib.BLOCK_HESSIAN_MAX_VECTORS)


def reference_operator_blocks(index, blocks, masses):
    """Torch reference of anihip_block_hessian_prepare's blocks: entry p = (row j, column a) -> (B_ja + B_aj^T) / (2
    sqrt(m_j m_a)), with B_aj the stored block of the transposed entry."""
    N = masses.numel()
    key = index[0] * N + index[1]
    order = torch.argsort(key)
    pos = order[torch.searchsorted(key[order], index[1] * N + index[0])]
    m = masses.reshape(-1).to(torch.float64)
    w = (m[index[0]] * m[index[1]]).rsqrt().view(-1, 1, 1)
    return 0.5 * (blocks.double() + blocks.double()[pos].transpose(1, 2)) * w


def dense_operator(H, masses):
    """M^-1/2 ((H + H^T) / 2) M^-1/2 [C, 3A, 3A] of a BlockHessian (zero rows and columns on padding atoms)."""
    D = H.to_dense().double()
    D = 0.5 * (D + D.transpose(1, 2))
    m = masses.double()
    w = torch.where(m > 0, m.clamp_min(1e-300).rsqrt(), torch.zeros_like(m)).repeat_interleave(3, dim=1)
    return D * w.unsqueeze(2) * w.unsqueeze(1)


def test_reference_operator_blocks_hand_built():
    from torchani_amd.tuples import BlockHessian

    H, dense = _hand_built(4)
    # an asymmetric perturbation: the operator symmetrizes (H + H^T) / 2
    g = torch.Generator().manual_seed(5)
    blocks = H.blocks + 1e-2 * torch.randn(H.blocks.shape, generator=g)
    Hp = BlockHessian(H.index, blocks, H.n_molecules, H.n_atoms)
    masses = torch.tensor([[1.008, 12.0, 15.999, 14.007], [1.008, 32.06, 12.0, 0.0]])
    ab = reference_operator_blocks(Hp.index, Hp.blocks, masses)
    Aref = dense_operator(Hp, masses)
    Ab = BlockHessian(Hp.index, ab, 2, 4).to_dense()
    assert torch.allclose(Ab, Aref, rtol=0, atol=1e-12)
    assert torch.allclose(Ab, Ab.transpose(1, 2), rtol=0, atol=1e-12)
    assert torch.all(Ab[1, 9:] == 0) and torch.all(Ab[1, :, 9:] == 0)


def _known_spectra(n=240, seed=0):
    """Two molecules of n degrees of freedom, molecule 1 with its last 40 padding: molecule 0 has six zero eigenvalues,
    near-degenerate pairs and negative eigenvalues; molecule 1 a negative cluster and a spread above."""
    rng = np.random.default_rng(seed)
    lam0 = np.concatenate([[-3.0, -2.5, -2.5 + 1e-9, -1.0], np.zeros(6), [0.2, 0.2 + 1e-10, 0.5, 0.5 + 1e-8],
                           np.linspace(0.8, 1.5, 12), np.linspace(2.0, 40.0, n - 26)])
    lam1 = np.concatenate([[-0.7, -0.69, -0.68], np.linspace(0.1, 3.0, 30), np.linspace(4.0, 25.0, n - 40 - 33)])
    A = np.zeros((2, n, n))
    for c, lam, d in ((0, lam0, n), (1, lam1, n - 40)):
        Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
        A[c, :d, :d] = (Q * lam) @ Q.T
    A = 0.5 * (A + A.transpose(0, 2, 1))
    mask = np.ones((2, n), dtype=bool)
    mask[1, n - 40:] = False
    return A, mask


def _check_pairs(A, mask, res, n_want, tol):
    bound = np.abs(A).sum(axis=2).max(axis=1)
    for c in range(A.shape[0]):
        d = int(mask[c].sum())
        lam, V = np.linalg.eigh(A[c, :d, :d])
        th = res.eigenvalues[c, :n_want].numpy()
        X = res.vectors[c].numpy()
        assert np.abs(X[d:]).max(initial=0.0) == 0.0                       # padding untouched
        assert np.abs(th - lam[:n_want]).max() <= tol * bound[c]
        R = A[c] @ X[:, :n_want] - X[:, :n_want] * th
        assert np.linalg.norm(R, axis=0).max() <= tol * bound[c]
        assert np.abs(X[:, :n_want].T @ X[:, :n_want] - np.eye(n_want)).max() <= 1e-10
        for i in range(n_want):
            gap = min(abs(lam[i] - lam[i - 1]) if i else np.inf, abs(lam[i + 1] - lam[i]))
            if gap > 1e-3 * bound[c]:
                assert abs(V[:, i] @ X[:d, i]) >= 0.999


@pytest.mark.parametrize("n_want", [1, 8, 20])
def test_lobpcg_known_spectra(n_want):
    from torchani_amd import modes

    A, mask = _known_spectra()
    At = torch.from_numpy(A)
    bound = torch.from_numpy(np.abs(A).sum(axis=2).max(axis=1))
    tol = 1e-8
    k = n_want + max(4, n_want // 4)
    g = torch.Generator().manual_seed(1)
    X0 = torch.randn((2, A.shape[1], k), generator=g, dtype=torch.float64) * torch.from_numpy(mask).unsqueeze(2)
    res = modes.lobpcg(lambda X: At @ X, X0, n_want, tol * bound, bound, 2000)
    assert res.n_iter < 2000
    _check_pairs(A, mask, res, n_want, tol)
    again = modes.lobpcg(lambda X: At @ X, X0, n_want, tol * bound, bound, 2000)
    assert torch.equal(again.eigenvalues, res.eigenvalues) and torch.equal(again.vectors, res.vectors)


def test_lobpcg_stops_at_max_iter():
    from torchani_amd import modes

    A, mask = _known_spectra(seed=2)
    At = torch.from_numpy(A)
    bound = torch.from_numpy(np.abs(A).sum(axis=2).max(axis=1))
    X0 = torch.randn((2, A.shape[1], 12), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    res = modes.lobpcg(lambda X: At @ X, X0 * torch.from_numpy(mask).unsqueeze(2), 8, 1e-12 * bound, bound, 1)
    assert res.n_iter == 1
    assert (res.residuals[:, :8] > 1e-12 * bound.unsqueeze(1)).any()


def test_dense_eigenpairs_with_projection():
    from torchani_amd import modes

    A, mask = _known_spectra(n=100, seed=4)
    At = torch.from_numpy(A)
    bound = torch.from_numpy(np.abs(A).sum(axis=2).max(axis=1))
    # the complement of two fixed directions per molecule, inside the real degrees of freedom
    rng = np.random.default_rng(6)
    Rv = rng.standard_normal((2, 100, 2)) * mask[:, :, None]
    Rq = torch.from_numpy(np.stack([np.linalg.qr(Rv[c])[0] for c in range(2)]))

    def project(V):
        return V - Rq @ (Rq.transpose(1, 2) @ V)

    E = project(torch.diag_embed(torch.from_numpy(mask).double()))
    res = modes.dense_eigenpairs(lambda X: project(At @ project(X)), E, 5, bound)
    for c in range(2):
        d = int(mask[c].sum())
        Pc = np.eye(d) - Rq[c, :d].numpy() @ Rq[c, :d].numpy().T
        B = np.linalg.svd(Pc)[0][:, :d - 2]                     # orthonormal basis of the complement
        lam = np.linalg.eigvalsh(B.T @ A[c, :d, :d] @ B)
        assert np.abs(res.eigenvalues[c].numpy() - lam[:5]).max() <= 1e-10 * bound[c].item()
        assert np.abs(Rq[c].numpy().T @ res.vectors[c].numpy()).max() <= 1e-10


def test_sparse_vibrational_analysis_argument_errors():
    from torchani_amd import grad
    from torchani_amd.tuples import BlockHessian

    H, _ = _hand_built()
    masses = torch.tensor([[1.008, 12.0, 15.999, 14.007], [1.008, 32.06, 12.0, 0.0]])
    with pytest.raises(TypeError):
        grad.sparse_vibrational_analysis(masses, H.to_dense(), 2)
    with pytest.raises(ValueError, match="masses"):
        grad.sparse_vibrational_analysis(masses[:1], H, 2)
    with pytest.raises(ValueError, match="unit|meV"):
        grad.sparse_vibrational_analysis(masses, H, 2, unit="Hz")
    with pytest.raises(ValueError, match="mode kind"):
        grad.sparse_vibrational_analysis(masses, H, 2, mode_kind="xyz")
    with pytest.raises(ValueError, match="n_modes"):
        grad.sparse_vibrational_analysis(masses, H, 0)
    with pytest.raises(ValueError, match="coordinates"):
        grad.sparse_vibrational_analysis(masses, H, 2, project_rigid=True)
    with pytest.raises(ValueError, match="ROCm"):   # CPU tensors: no CPU fallback
        grad.sparse_vibrational_analysis(masses, H, 2)
    with pytest.raises(ValueError, match="ROCm"):
        grad.sparse_vibrational_analysis(masses, BlockHessian(H.index, H.blocks, 2, 4), 2, project_rigid=True,
                                         pbc=torch.tensor([True, True, True]))


def test_gram_products_in_slabs():
    from torchani_amd import modes

    g = torch.Generator().manual_seed(7)
    for n in (100, 2 * modes.SLAB + 1, 3 * modes.SLAB):
        a = torch.randn((2, n, 5), generator=g, dtype=torch.float64)
        b = torch.randn((2, n, 3), generator=g, dtype=torch.float64)
        assert torch.allclose(modes._bt(a, b), a.transpose(1, 2) @ b, rtol=1e-12, atol=1e-10)
