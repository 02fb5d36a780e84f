"""Host-side parts of the block-sparse Hessians (no GPU): the C declarations of the new entry points against the ctypes
symbol list, BlockHessian's conversions and products on hand-built blocks (a batch with padding atoms included), and the
chunking of the direction atoms."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("anihip_hess_sparse_rlist", "anihip_hess_sparse_pattern", "anihip_hess_sparse_items", "anihip_hess_sparse_extract",
       "anihip_aev_jvp_items", "anihip_aev_backward_second_items", "anihip_mlp_rows_hvp_workspace_bytes",
       "anihip_mlp_rows_hvp_prepare", "anihip_mlp_rows_hvp", "anihip_pair_analytic_hvp_items")


def test_header_declares_the_sparse_entry_points():
    from torchani_amd import _lib

    with open(os.path.join(ROOT, "include", "anihip.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(anihip_\w+)\s*\(", src))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS
    assert "hess_sparse.hip" in _lib.SOURCES
    assert _lib.ABI_VERSION == 13


def _hand_built(seed=0):
    """Two molecules of A = 4 atoms, atom 3 of molecule 1 padding; pattern: every pair of real atoms of a molecule except
    (0, 2) of molecule 0, by columns.  Returns the BlockHessian and its dense [C, 3A, 3A] twin built entry by entry."""
    from torchani_amd.tuples import BlockHessian

    g = torch.Generator().manual_seed(seed)
    C, A = 2, 4
    real = {0: [0, 1, 2, 3], 1: [0, 1, 2]}
    pairs = []
    for c, atoms in real.items():
        for a in atoms:
            for j in atoms:
                if c == 0 and {a, j} == {0, 2}:
                    continue
                pairs.append((c * A + j, c * A + a))   # (row, column), grouped by column
    index = torch.tensor(pairs, dtype=torch.int64).t().contiguous()
    blocks = torch.empty((index.shape[1], 3, 3))
    lookup = {}
    for p, (i, j) in enumerate(pairs):
        if (j, i) in lookup:
            blocks[p] = blocks[lookup[(j, i)]].t()
        else:
            r = torch.randn((3, 3), generator=g)
            blocks[p] = r + r.t() if i == j else r
        lookup[(i, j)] = p
    dense = torch.zeros((C, 3 * A, 3 * A))
    for p, (i, j) in enumerate(pairs):
        c, a, b = i // A, i % A, j % A
        dense[c, 3 * a:3 * a + 3, 3 * b:3 * b + 3] = blocks[p]
    return BlockHessian(index, blocks, C, A), dense


def test_block_hessian_to_dense():
    H, dense = _hand_built()
    D = H.to_dense()
    assert D.shape == (2, 12, 12) and D.dtype == torch.float32
    assert torch.equal(D, dense)
    assert torch.equal(D, D.transpose(1, 2))
    assert torch.all(D[1, 9:, :] == 0) and torch.all(D[1, :, 9:] == 0)   # the padding atom
    assert torch.all(D[0, 0:3, 6:9] == 0)                                # outside the pattern


def test_block_hessian_to_sparse_coo():
    H, dense = _hand_built(1)
    S = H.to_sparse_coo()
    assert S.is_sparse and S.shape == (24, 24) and S.is_coalesced()
    assert S._nnz() == 9 * H.nnz
    D = S.to_dense()
    assert torch.equal(D[:12, :12], dense[0]) and torch.equal(D[12:, 12:], dense[1])
    assert torch.all(D[:12, 12:] == 0) and torch.all(D[12:, :12] == 0)   # blocks never cross molecules


def test_block_hessian_matvec():
    H, dense = _hand_built(2)
    v = torch.randn((2, 4, 3), generator=torch.Generator().manual_seed(3))
    ref = torch.einsum("cij,cj->ci", dense.double(), v.double().reshape(2, 12)).reshape(2, 4, 3)
    out = H.matvec(v)
    assert out.shape == v.shape
    assert torch.allclose(out.double(), ref, rtol=1e-6, atol=1e-6)
    assert torch.allclose(H.matvec(v.reshape(2, 12)).reshape(2, 4, 3), out)
    with pytest.raises(ValueError):
        H.matvec(torch.zeros(5))


def test_block_hessian_shape_checks():
    from torchani_amd.tuples import BlockHessian

    with pytest.raises(ValueError):
        BlockHessian(torch.zeros((2, 3), dtype=torch.int64), torch.zeros((2, 3, 3)), 1, 2)


def test_sparse_hessian_chunks():
    from torchani_amd.grad import sparse_hessian_chunks

    rcnt = np.array([3, 0, 5, 2, 0, 0, 4, 1])   # |R(a)|; zeros are padding
    roff = np.concatenate([[0], np.cumsum(rcnt)])
    for budget, max_atoms in ((3, 8), (15, 8), (18, 2), (1000, 3), (1000, 100)):
        chunks = sparse_hessian_chunks(roff, budget, max_atoms)
        covered = [a for n0, n1 in chunks for a in range(n0, n1)]
        assert covered == sorted(set(covered))
        assert set(np.flatnonzero(rcnt)) <= set(covered)
        for n0, n1 in chunks:
            rows = 3 * int(roff[n1] - roff[n0])
            assert rows > 0 and n1 - n0 <= max_atoms
            assert rows <= budget or n1 - n0 == 1
