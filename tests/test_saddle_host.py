"""Host-side parts of the saddle-point search (no GPU): the fp64 reference of the GPU tests (tests/_saddle_ref.py) on the
four-atom Lennard-Jones cluster, its pieces against closed forms, the exported symbols, the workspace size of the Python layer
against the library's, and every refusal of SaddleOptimizer before any device work."""
import os
import re

import numpy as np
import pytest
import torch

from _saddle_ref import (LJ4_SADDLE, SaddleReference, bofill, lj4_diamond, lj_energy_forces, lj_hessian, oracle_lockstep,
                         relax_on_oracle, rfo_partitions, rigid_basis, rotatable_bonds, run_lj_reference)
from _util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lj_functions_against_finite_differences():
    x = lj4_diamond(0.05, 9)
    _, f = lj_energy_forces(x)
    H = lj_hessian(x)
    h = 1e-6
    for i in range(12):
        xp, xm = x.ravel().copy(), x.ravel().copy()
        xp[i] += h
        xm[i] -= h
        ep, fp = lj_energy_forces(xp.reshape(4, 3))
        em, fm = lj_energy_forces(xm.reshape(4, 3))
        assert abs(-(ep - em) / (2 * h) - f.ravel()[i]) < 1e-7
        assert np.abs(-(fp - fm).ravel() / (2 * h) - H[:, i]).max() < 1e-6


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_reference_finds_the_lj4_saddle_with_exact_hessians(seed):
    """From the planar diamond plus 0.002 sigma of noise, exact Hessians at every step: three steps reach the D2h saddle."""
    ref, x, e, f = run_lj_reference(lj4_diamond(0.002, seed), 1, 0.0, 3)
    assert ref.n_steps[0] == 3 and ref.n_rejected[0] == 0
    assert abs(e - LJ4_SADDLE) < 1e-9
    lam = np.linalg.eigvalsh(lj_hessian(x))
    assert lam[0] == pytest.approx(-0.465, abs=2e-3) and np.abs(lam[1:7]).max() < 1e-3 and lam[7] > 50.0
    assert lam[7:] == pytest.approx([55.4, 59.7, 119.4, 171.3, 178.1], abs=0.06)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_reference_converges_on_bofill_updates_alone(seed):
    """One exact Hessian, then Bofill updates only (hessian_every beyond the run): at most 11 accepted steps to fmax 1e-6."""
    ref, x, e, f = run_lj_reference(lj4_diamond(0.002, seed), 1000, 1e-6, 40)
    assert ref.converged[0] and ref.n_steps[0] <= 11
    assert abs(e - LJ4_SADDLE) < 1e-9 and np.sqrt((f ** 2).sum(-1)).max() < 1e-6


@pytest.mark.parametrize("seed", [1, 2])
def test_reference_climbs_away_from_a_start_without_negative_curvature(seed):
    """The limit of the method: with 0.01 sigma of noise (these seeds) the lowest vibrational mode of the start is positive,
    P-RFO climbs it and the cluster comes apart -- it does not arrive at the saddle next door."""
    x0 = lj4_diamond(0.01, seed)
    Q = rigid_basis(x0, None, True, True)
    P = np.eye(12) - Q @ Q.T
    lam = np.linalg.eigvalsh(P @ lj_hessian(x0) @ P)
    assert np.sort(lam[np.abs(lam) > 1e-9])[0] > 0.0
    ref, x, e, f = run_lj_reference(x0, 1, 1e-6, 60)
    far = np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1)).max()
    assert not ref.converged[0] and far > 3.0 and e > LJ4_SADDLE + 1.0


@pytest.mark.parametrize("hessian_every", [1, 4])
@pytest.mark.parametrize("base", ["rand_batch_ani2x", "water_pbc_ani2x"])
def test_lockstep_cases_have_a_defined_followed_mode(base, hessian_every):
    """The lock-step cases of tests/test_gpu_saddle.py rehearsed on the fp64 oracle's surface: the pairs the GPU test may skip
    (followed eigenvalue within 1e-6 relative of its neighbour) stay within its 10 % share by themselves.  Measured: none of
    the 48 pairs of the padded batch, none of the 8 of the periodic box, for either hessian_every."""
    pairs, degenerate = oracle_lockstep(load_golden(base), hessian_every, 8)
    assert pairs == 8 * load_golden(base)["species"].shape[0]
    assert degenerate <= 0.1 * pairs


@pytest.mark.parametrize("mol", [0, 13])
def test_seeded_weights_leave_no_torsion_to_scan(mol):
    """Why there is no ANI torsional-saddle test: the committed fixtures carry seeded random weights, whose surface has no
    chemistry.  The 13-atom molecules of cfg2_xyz13_28_ani2x start with four rotatable heavy-atom bonds; relaxed on the fp64
    oracle's surface (the first stage of relax, scan, search) they converge to geometries with atoms 0.1 to 0.2 A apart and
    no rotatable bond left (nine molecules were tried: 0, 1, 2, 3, 5, 8, 13, 21, 34), so no candidate reaches the scan."""
    symbols, x0, x, converged = relax_on_oracle(load_golden("cfg2_xyz13_28_ani2x"), mol)
    closest = lambda y: np.sqrt(((y[:, None] - y[None]) ** 2).sum(-1))[np.triu_indices(len(symbols), 1)].min()   # noqa: E731
    assert converged and closest(x0) > 1.0 and len(rotatable_bonds(symbols, x0)) == 4
    assert closest(x) < 0.5 and rotatable_bonds(symbols, x) == []


def test_rigid_basis_ranks():
    rs = np.random.RandomState(0)
    assert rigid_basis(rs.randn(1, 3), None, True, True).shape == (3, 3)        # one atom: no rotation
    line = np.outer(np.arange(3.0), [0.3, -0.5, 0.8]) + 0.1
    assert rigid_basis(line[:2], None, True, True).shape == (6, 5)              # linear: five rigid vectors
    assert rigid_basis(line, None, True, True).shape == (9, 5)
    x = rs.randn(5, 3)
    Q = rigid_basis(x, None, True, True)
    assert Q.shape == (15, 6) and np.abs(Q.T @ Q - np.eye(6)).max() < 1e-14
    shift = np.tile([0.2, -0.1, 0.4], 5)
    turn = np.cross([0.3, 0.1, -0.2], x - x.mean(0)).ravel()
    for v in (shift, turn):
        assert np.abs(v - Q @ (Q.T @ v)).max() < 1e-14
    assert rigid_basis(x, None, True, False).shape == (15, 3) and rigid_basis(x, None, False, False).shape == (15, 0)


def test_rfo_partitions_against_the_secular_equations():
    rs = np.random.RandomState(1)
    lam = np.sort(rs.randn(9) * 3)
    gt = rs.randn(9)
    gt[2] = 0.0           # a mode without a gradient component: no step along it
    for k in (0, 4):
        st = rfo_partitions(lam, gt, k)
        gp = 0.5 * (lam[k] + np.sqrt(lam[k] ** 2 + 4 * gt[k] ** 2))
        assert st[k] == pytest.approx(-gt[k] / (lam[k] - gp), rel=1e-12)
        others = [i for i in range(9) if i != k and gt[i] != 0.0]
        gm = (gt[others] * st[others]).sum()        # gm = sum g_i^2 / (gm - lam_i) with s_i = -g_i / (lam_i - gm)
        assert gm < min(0.0, lam[others].min())
        assert np.allclose(st[others], -gt[others] / (lam[others] - gm), rtol=1e-10, atol=0)
        assert st[2] == 0.0


def test_bofill_satisfies_the_secant_equation():
    rs = np.random.RandomState(2)
    M = rs.randn(7, 7)
    H = M + M.T
    s, y = rs.randn(7), rs.randn(7)
    H1 = bofill(H, s, y)
    assert np.abs(H1 @ s - y).max() < 1e-12 and np.abs(H1 - H1.T).max() < 1e-13
    assert bofill(H, np.zeros(7), y) is None and bofill(H, s, H @ s) is None


def test_reference_rejects_and_restores():
    """A quadratic model that lies about the energy: the step is rejected, the radius quartered, nothing else moves."""
    kind = np.ones((1, 2), dtype=int)
    ref = SaddleReference(kind, True, "lowest", 0.05, 0.15, 1e-4, 1e-7, 1e-9, coord_dtype=np.float64)
    H = np.diag([-1.0, 2.0, 3.0, 1.0, 4.0, 2.0])
    x = np.array([[[0.0, 0.0, 0.0], [1.0, 0.5, 0.2]]])
    f = np.array([[[0.3, -0.2, 0.1], [-0.1, 0.4, 0.2]]])
    dr = ref.propose(x, np.array([0.0]), f, H[None])
    assert np.linalg.norm(dr) == pytest.approx(0.05)
    ref.judge(np.array([10.0]), f, True)
    assert not ref.accepted[0] and ref.n_rejected[0] == 1 and ref.n_steps[0] == 0 and ref.trust[0] == pytest.approx(0.0125)
    assert np.array_equal(ref.H[0], H)


def test_library_exports_the_saddle_entry_points():
    from torchani_amd import _lib

    _lib.build()
    with open(os.path.join(ROOT, "include", "anihip.h")) as fh:
        declared = set(re.findall(r"\b(anihip_[a-z_0-9]+)\s*\(", fh.read()))
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    L = _lib.lib()
    for name in ("anihip_saddle_workspace_bytes", "anihip_saddle_project", "anihip_saddle_step", "anihip_saddle_accept"):
        assert name in declared and "saddle.hip" in _lib.SOURCES
        getattr(L, name)
    assert L.anihip_abi_version() == 13


def test_workspace_bytes_match_library_and_header_formula():
    from torchani_amd import _lib
    from torchani_amd.geomopt import SADDLE_MAX_COORDS, saddle_workspace_bytes

    _lib.build()
    L = _lib.lib()

    def header(C, A):   # q, b fp64 [C][6][n] | gproj, displacement, xi fp64 [C][n] | old coords fp32 [C][n] | scalars fp64 [C][8]
        n = 3 * A
        up = lambda b: (b + 255) // 256 * 256   # noqa: E731
        return 2 * up(C * 6 * n * 8) + 3 * up(C * n * 8) + up(C * n * 4) + up(C * 64)

    for C, A in [(1, 1), (5, 4), (6, 14), (256, 28), (3, 86), (1, 90), (2, SADDLE_MAX_COORDS // 3)]:
        assert L.anihip_saddle_workspace_bytes(C, A) == saddle_workspace_bytes(C, A) == header(C, A), (C, A)
    assert L.anihip_saddle_workspace_bytes(1, SADDLE_MAX_COORDS // 3 + 1) == 0 and b"atoms_per_mol" in L.anihip_last_error()
    assert L.anihip_saddle_workspace_bytes(0, 3) == 0
    with pytest.raises(ValueError):
        saddle_workspace_bytes(1, SADDLE_MAX_COORDS // 3 + 1)


def _cpu_inputs(A=3):
    return torch.zeros((2, A), dtype=torch.long), torch.zeros((2, A, 3))


@pytest.mark.parametrize("kw, error, match", [
    ({"constraints": object()}, NotImplementedError, "constraints"),
    ({"neighbors": object()}, NotImplementedError, "external neighbor"),
    ({"hessian_every": 0}, ValueError, "hessian_every"),
    ({"hessian_every": 2.5}, ValueError, "hessian_every"),
    ({"trust": 0.0}, ValueError, "trust"),
    ({"trust": float("nan")}, ValueError, "trust"),
    ({"max_trust": float("inf")}, ValueError, "max_trust"),
    ({"min_trust": -1e-4}, ValueError, "min_trust"),
    ({"trust": 0.5}, ValueError, "min_trust <= trust <= max_trust"),
    ({"mode": torch.zeros((2, 3))}, ValueError, "mode"),
    ({"mode": torch.zeros((3, 3))}, ValueError, "mode"),
    ({"fixed": torch.zeros(3, dtype=torch.bool)}, ValueError, "fixed"),
    ({"follow": "highest"}, ValueError, "follow"),
    ({"energy_floor": -1.0}, ValueError, "energy_floor"),
])
def test_bad_arguments_raise_before_device_work(kw, error, match):
    from torchani_amd.geomopt import SaddleOptimizer, optimize_saddle

    sp, x = _cpu_inputs()
    with pytest.raises(error, match=match):
        SaddleOptimizer(None, sp, x, **kw)
    with pytest.raises(error, match=match):
        optimize_saddle(None, sp, x, **kw)


def test_too_many_coordinates_shapes_and_cpu_tensors_raise():
    from torchani_amd.geomopt import SADDLE_MAX_COORDS, SaddleOptimizer, optimize_saddle

    sp, x = _cpu_inputs(SADDLE_MAX_COORDS // 3 + 1)
    with pytest.raises(ValueError, match="SADDLE_MAX_COORDS"):
        SaddleOptimizer(None, sp, x)
    sp, x = _cpu_inputs()
    with pytest.raises(ValueError, match=r"\[C, A, 3\]"):
        SaddleOptimizer(None, sp, x[:, :2])
    with pytest.raises(ValueError, match="ROCm"):
        SaddleOptimizer(None, sp, x)
    with pytest.raises(ValueError, match="fmax"):
        optimize_saddle(None, sp, x, fmax=-1.0)


def test_models_without_a_saddle_search_raise_on_the_host():
    from torchani_amd.geomopt import SaddleOptimizer
    from torchani_amd.models import ANI2dr, ANI2x

    sp, x = _cpu_inputs()
    with pytest.raises(NotImplementedError, match="TwoBodyDispersionD3"):
        SaddleOptimizer(ANI2dr(seed=0, n_members=2), sp, x)
    model = ANI2x(seed=0, n_members=2)
    model.requires_grad_(True)
    with pytest.raises(RuntimeError, match="frozen parameters"):
        SaddleOptimizer(model, sp, x)
