"""Host side of the strain second derivatives: the Voigt projection and the unit of grad.elastic_constants, the
relaxed-ion formula against direct minimisation, an analytic lattice, and the new entry points in the header and the
ctypes list (no GPU)."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("anihip_aev_jvp_strain_items", "anihip_aev_backward_second_strain_items", "anihip_pair_analytic_hvp_strain")


def _result(W, Xi=None, forces=None, A=1):
    """An EnergiesForcesStrainHessians with strain_hessians W [C, 9, 9], internal_strain Xi [C, A, 3, 9]."""
    from torchani_amd.tuples import EnergiesForcesStrainHessians

    C = W.shape[0]
    if Xi is None:
        Xi = torch.zeros((C, A, 3, 9), dtype=torch.float64)
    A = Xi.shape[1]
    if forces is None:
        forces = torch.zeros((C, A, 3), dtype=torch.float64)
    return EnergiesForcesStrainHessians(torch.zeros(C, dtype=torch.float64), forces, torch.zeros((C, 3, 3), dtype=torch.float64),
                                        W.reshape(C, 3, 3, 3, 3), Xi.reshape(C, A, 3, 3, 3))


def test_header_and_ctypes_list_the_strain_entry_points():
    from torchani_amd import _lib

    with open(os.path.join(ROOT, "include", "anihip.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS, name
    assert _lib.ABI_VERSION == 13


def test_unit_conversion():
    from torchani_amd import units

    # 1 Hartree = 4.3597447e-18 J; 1 A^3 = 1e-30 m^3
    assert abs(units.HARTREE_PER_ANGSTROM3_TO_GPA - 4359.74465) < 1e-3
    assert units.hartree_per_angstrom3_to_gpa(2.0) == 2.0 * units.HARTREE_PER_ANGSTROM3_TO_GPA


def test_voigt_projection():
    from torchani_amd import grad, units

    P = grad.voigt_projector()
    # a symmetric strain e in Voigt form (engineering shears) moves S by sum_I e_I P[I]
    e = torch.tensor([0.1, -0.2, 0.3, 0.04, -0.05, 0.06], dtype=torch.float64)
    eps = (e @ P).view(3, 3)
    want = torch.tensor([[0.1, 0.03, -0.025], [0.03, -0.2, 0.02], [-0.025, 0.02, 0.3]], dtype=torch.float64)
    assert torch.allclose(eps, want)
    # a quadratic energy E = 1/2 s^T W s over the 9 components: elastic_constants = P W P^T / V
    rs = np.random.RandomState(3)
    M = rs.normal(size=(9, 9))
    W = torch.from_numpy(M + M.T).unsqueeze(0)
    cell = torch.diag(torch.tensor([2.0, 3.0, 4.0], dtype=torch.float64))
    C = grad.elastic_constants(_result(W), cell, unit="Hartree/A^3")
    assert C.shape == (1, 6, 6)
    assert torch.allclose(C[0], P @ W[0] @ P.T / 24.0)
    assert torch.allclose(e @ C[0] @ e * 24.0, (e @ P) @ W[0] @ (e @ P))
    Cg = grad.elastic_constants(_result(W), cell)
    assert torch.allclose(Cg, C * units.HARTREE_PER_ANGSTROM3_TO_GPA)
    with pytest.raises(ValueError):
        grad.elastic_constants(_result(W), cell, unit="bar")
    with pytest.raises(ValueError):
        grad.elastic_constants(_result(W), None)
    with pytest.raises(ValueError):
        grad.elastic_constants(_result(W), cell, pbc=torch.tensor([True, True, False]))
    with pytest.raises(ValueError):
        grad.elastic_constants(_result(W), cell, relaxed=True)


def test_relaxed_ion_against_minimisation():
    """E(e, u) = 1/2 s^T W s + u^T K s + 1/2 u^T H u with s = e P (symmetric strain) and a translational null space in H and
    K: the relaxed constants are the Hessian of min_u E over e, found here by solving on the internal coordinates."""
    from torchani_amd import grad

    rs = np.random.RandomState(7)
    A = 5
    n = 3 * A
    # H: positive definite on the complement of the three translations, zero on them
    T = np.zeros((n, 3))
    for y in range(3):
        T[y::3, y] = 1.0 / np.sqrt(A)
    Q = np.eye(n) - T @ T.T
    B = rs.normal(size=(n, n))
    H = Q @ (B @ B.T + 0.5 * np.eye(n)) @ Q
    K = Q @ rs.normal(size=(n, 9))                    # (sum over the atoms vanishes: translation invariance)
    Wm = rs.normal(size=(9, 9))
    W = 30.0 * (Wm + Wm.T) + 400.0 * np.eye(9)
    # non-zero forces: internal_strain = K + delta_ya (dE/dx_i)_b; elastic_constants takes the force term back out
    F = Q @ rs.normal(size=n) * 0.1
    ist = K.reshape(A, 3, 3, 3).copy()
    for y in range(3):
        ist[:, y, y, :] += -F.reshape(A, 3)
    res = _result(torch.from_numpy(W).unsqueeze(0), torch.from_numpy(ist.reshape(1, A, 3, 9)),
                  torch.from_numpy(F.reshape(1, A, 3)))
    cell = torch.tensor([[4.0, 0.3, 0.0], [0.0, 5.0, 0.2], [0.1, 0.0, 6.0]], dtype=torch.float64)
    V = abs(np.linalg.det(cell.numpy()))
    P = grad.voigt_projector().numpy()
    Cr = grad.elastic_constants(res, cell, hessians=torch.from_numpy(H).unsqueeze(0), relaxed=True,
                                unit="Hartree/A^3")[0].numpy()
    Cc = grad.elastic_constants(res, cell, unit="Hartree/A^3")[0].numpy()
    # direct minimisation over u in the complement of the translations, column by column of the Voigt strains
    Z = np.linalg.svd(Q)[0][:, : n - 3]                # an orthonormal basis of the complement
    want = np.zeros((6, 6))
    for I in range(6):
        for J in range(6):
            def relaxed_energy(e):
                s = e @ P
                u = -Z @ np.linalg.solve(Z.T @ H @ Z, Z.T @ K @ s)
                return 0.5 * s @ W @ s + u @ K @ s + 0.5 * u @ H @ u
            h = 1e-3
            ei, ej = np.eye(6)[I] * h, np.eye(6)[J] * h
            want[I, J] = (relaxed_energy(ei + ej) - relaxed_energy(ei - ej) - relaxed_energy(-ei + ej)
                          + relaxed_energy(-ei - ej)) / (4 * h * h) / V
    assert np.abs(Cr - want).max() <= 1e-8 * np.abs(want).max()
    assert np.abs(Cc - P @ W @ P.T / V).max() <= 1e-12 * np.abs(Cc).max()
    assert (np.linalg.eigvalsh(Cc - Cr) > -1e-9).all()   # relaxing can only lower the energy


def test_simple_cubic_springs():
    """A simple cubic lattice (constant a) of nearest-neighbour harmonic springs k at rest length a, as a 2 x 2 x 2 periodic
    supercell: C11 = k / a, C12 = C44 = 0, and relaxed = clamped (a Bravais lattice: no internal strain)."""
    from torchani_amd import grad

    k, a, m = 0.7, 1.5, 2
    A = m ** 3
    pos = np.array([[i, j, l] for i in range(m) for j in range(m) for l in range(m)], dtype=np.float64) * a
    # per bond d (length a along an axis): W += k d_a d_p u_b u_q (the tension e'(r) = 0 at rest), summed over A x 3 bonds
    W = np.zeros((3, 3, 3, 3))
    H = np.zeros((3 * A, 3 * A))
    idx = {tuple(np.round(p / a).astype(int)): i for i, p in enumerate(pos)}
    for i, p in enumerate(pos):
        for ax in range(3):
            u = np.eye(3)[ax]
            d = a * u
            W += k * np.einsum("a,p,b,q->abpq", d, d, u, u)
            q = tuple((np.round(p / a).astype(int) + np.eye(3, dtype=int)[ax]) % m)
            j = idx[q]
            B = k * np.outer(u, u)
            H[3 * i:3 * i + 3, 3 * i:3 * i + 3] += B
            H[3 * j:3 * j + 3, 3 * j:3 * j + 3] += B
            H[3 * i:3 * i + 3, 3 * j:3 * j + 3] -= B
            H[3 * j:3 * j + 3, 3 * i:3 * i + 3] -= B
    res = _result(torch.from_numpy(W.reshape(1, 9, 9)), torch.zeros((1, A, 3, 9), dtype=torch.float64))
    cell = torch.eye(3, dtype=torch.float64) * (m * a)
    Cc = grad.elastic_constants(res, cell, unit="Hartree/A^3")[0]
    Cr = grad.elastic_constants(res, cell, hessians=torch.from_numpy(H).unsqueeze(0), relaxed=True, unit="Hartree/A^3")[0]
    want = torch.zeros((6, 6), dtype=torch.float64)
    for I in range(3):
        want[I, I] = k / a
    assert torch.allclose(Cc, want, atol=1e-14)
    assert torch.allclose(Cr, Cc, atol=1e-14)
