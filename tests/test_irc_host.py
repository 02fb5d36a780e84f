"""Reaction paths (torchani_amd.geomopt.ReactionPathFollower, anihip_irc_*) on the host: the fp64 reference of tests/_irc_ref.py
against the differential equation the LQA step solves and against exact cases, the reaction path of the four-atom
Lennard-Jones cluster rehearsed in fp64, the lock-step cases of tests/test_gpu_irc.py rehearsed on the fp64 oracle's surface,
the exports, the workspace formula and the refusals that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from _irc_ref import (ENERGY_ROSE, LOCKSTEP_STEP, MINIMUM, PATH_FULL, IrcReference, arc_length, lj4_saddle, lqa_step, oracle_lockstep,
                      rigid_basis_mw, run_lj_path)
from _saddle_ref import LJ4_SADDLE
from _util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the LQA step against the differential equation it solves --------------------------------------------------------------

def rk4_path(H, g, step, n_sub):
    """The curve of dq/dt = -(g + H q) from q = 0, parametrized by its own arc length, dq/ds = -G / |G|, and integrated by
    n_sub RK4 sub-steps to s = step: where the time integration arrives when it is stopped at that arc length."""
    q = np.zeros_like(g)
    h = step / n_sub

    def rhs(q):
        G = g + H @ q
        return -G / np.linalg.norm(G)

    for _ in range(n_sub):
        k1 = rhs(q)
        k2 = rhs(q + 0.5 * h * k1)
        k3 = rhs(q + 0.5 * h * k2)
        k4 = rhs(q + h * k3)
        q = q + h / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    return q


def _spectra():
    """(eigenvalues, gradient in the eigenbasis, step): a negative lowest mode; a positive spectrum over five orders of
    magnitude; one point after a saddle, where the gradient is tiny and lies mostly across the negative mode."""
    rs = np.random.RandomState(7)
    out = {}
    lam = np.sort(rs.uniform(0.5, 8.0, 9))
    lam[0] = -0.7
    out["negative lowest"] = (lam, rs.uniform(-0.3, 0.3, 9), 0.05)
    out["five orders"] = (np.logspace(-2, 3, 12), rs.uniform(-0.3, 0.3, 12), 0.05)
    lam = np.sort(rs.uniform(0.5, 8.0, 9))
    lam[0] = -0.5
    gt = 1e-3 * rs.uniform(-1, 1, 9)
    gt[0] = 1e-4
    out["near a saddle"] = (lam, gt, 0.05)
    return out


@pytest.mark.parametrize("name", ["negative lowest", "five orders", "near a saddle"])
def test_lqa_step_solves_its_differential_equation(name):
    """The reference's displacement against 8000 RK4 sub-steps, the error of those estimated from 4000.  Gate: 1e-8 of the
    largest component, plus twice the estimate.  Measured |LQA - RK4| / max |RK4| (estimate): negative lowest 1.3e-15
    (1.4e-15), five orders 2.0e-15 (2.3e-14), near a saddle 1.0e-9 (1.8e-8: the path turns by a right angle where the gradient
    is 1e-4, and RK4 in the arc length resolves that turn worst)."""
    lam, gt, step = _spectra()[name]
    U, _ = np.linalg.qr(np.random.RandomState(1).randn(lam.size, lam.size))
    H, g = (U * lam) @ U.T, U @ gt
    alpha, ds, landed, margin = lqa_step(lam, gt, step)
    assert not landed and ds == step and margin > 1e-2
    coarse, fine = rk4_path(H, g, step, 4000), rk4_path(H, g, step, 8000)
    scale = np.abs(fine).max()
    estimate = np.abs(coarse - fine).max() / scale
    err = np.abs(U @ alpha - fine).max() / scale
    print(f"{name}: |LQA - RK4| / max |RK4| = {err:.1e}, RK4 estimate {estimate:.1e}")
    assert err <= 1e-8 + 2.0 * estimate
    assert abs(arc_length(lam, gt, 0.0)) == 0.0


# ---- exact cases -----------------------------------------------------------------------------------------------------------

def test_one_moving_mode_moves_by_the_step():
    for lam0 in (-2.0, 0.0, 1e-12, 0.5, 30.0):
        lam = np.array([lam0, 1.0, 3.0])
        gt = np.array([0.2, 0.0, 0.0])
        if lam0 > 0 and 0.2 / lam0 < 0.05:   # the minimum of the model is nearer than the step: the landing
            alpha, ds, landed, margin = lqa_step(lam, gt, 0.05)
            assert landed and alpha[0] == -0.2 / lam0 and abs(ds - 0.2 / lam0) <= 1e-12 * ds
            assert margin == pytest.approx((0.05 - 0.2 / lam0) / 0.05, rel=1e-9)
            continue
        alpha, ds, landed, margin = lqa_step(lam, gt, 0.05)
        assert not landed and ds == 0.05
        assert alpha[0] < 0 and abs(abs(alpha[0]) - 0.05) <= 1e-12 * 0.05 and not alpha[1:].any()


def test_equal_eigenvalues_move_along_a_straight_line():
    lam = np.array([0.7, 0.7, 2.0, 5.0])
    gt = np.array([0.3, -0.4, 0.0, 0.0])
    alpha, ds, landed, _ = lqa_step(lam, gt, 0.05)
    assert not landed
    assert np.abs(alpha[:2] + 0.05 * gt[:2] / 0.5).max() <= 1e-12 * 0.05 and not alpha[2:].any()
    assert abs(np.linalg.norm(alpha) - 0.05) <= 1e-12 * 0.05


def test_small_lambda_t_limit_and_zero_gradient():
    """lam t -> 0: alpha -> -g~ t, a straight line down the gradient of length step, for eigenvalues far below 1 / t."""
    gt = np.array([0.1, -0.2, 0.05])
    for lam in (np.zeros(3), np.array([1e-13, -1e-13, 3e-14]), np.array([1e-300, 0.0, -1e-300])):
        alpha, ds, landed, _ = lqa_step(lam, gt, 0.05)
        assert not landed and ds == 0.05
        assert np.abs(alpha + 0.05 * gt / np.linalg.norm(gt)).max() <= 1e-11 * 0.05
    alpha, ds, landed, margin = lqa_step(np.array([1.0, 2.0]), np.zeros(2), 0.05)
    assert not alpha.any() and ds == 0.0 and not landed


def test_landing_on_the_minimum_of_the_model():
    lam = np.array([0.5, 2.0, 40.0])
    gt = np.array([0.01, -0.02, 0.3])
    alpha, ds, landed, margin = lqa_step(lam, gt, 0.05)
    assert landed and np.array_equal(alpha, -gt / lam)
    assert ds < 0.05 and ds >= np.linalg.norm(alpha) and margin == pytest.approx((0.05 - ds) / 0.05, rel=1e-12)
    # the same spectrum with a shorter step stops on the way
    alpha, ds, landed, margin = lqa_step(lam, gt, 0.01)
    assert not landed and ds == 0.01 and np.linalg.norm(alpha) < 0.01


def test_mass_weighted_rigid_basis():
    rs = np.random.RandomState(0)
    x, m = rs.randn(5, 3), rs.uniform(1.0, 40.0, 5)
    Q = rigid_basis_mw(x, m, True, True)
    assert Q.shape == (15, 6) and np.allclose(Q.T @ Q, np.eye(6), atol=1e-12)
    # a rigid motion dx = a + b x r in mass-weighted coordinates lies in the span
    dx = np.array([0.3, -0.2, 0.5]) + np.cross(np.array([0.1, 0.4, -0.3]), x)
    dq = (np.sqrt(m)[:, None] * dx).ravel()
    assert np.abs(dq - Q @ (Q.T @ dq)).max() < 1e-12
    assert rigid_basis_mw(x[:1], m[:1], True, True).shape == (3, 3)
    assert rigid_basis_mw(np.outer(np.arange(3.0), [0.3, -0.5, 0.8]), m[:3], True, True).shape == (9, 5)
    assert rigid_basis_mw(x, m, True, False).shape == (15, 3) and rigid_basis_mw(x, m, False, False).shape == (15, 0)


def test_reference_commit_branches():
    """Energy rose (nothing appended, done), append, MINIMUM by fmax, PATH_FULL."""
    kind = np.ones((4, 2), dtype=int)
    ref = IrcReference(kind, np.full((4, 2), 2.0), True, 0.05, 1e-3, 1e-7, 2, coord_dtype=np.float64)
    H = np.repeat(np.diag([1.0, 2.0, 3.0, 1.5, 4.0, 2.5])[None], 4, 0)
    x = np.zeros((4, 2, 3))
    f = np.repeat(np.array([[[0.3, -0.2, 0.1], [-0.1, 0.4, 0.2]]]), 4, 0)
    e = np.zeros(4)
    dr = ref.propose(x, e, f, H)
    assert np.abs(np.linalg.norm(np.sqrt(2.0) * dr.reshape(4, -1), axis=1) - 0.05).max() < 0.05   # (a curve: chord <= arc)
    f_small = 1e-4 * f
    ref.judge(np.array([1e-3, -1e-3, -1e-3, -1e-3]), np.stack([f[0], f[1], f_small[2], f[3]]), True)
    assert ref.reason.tolist() == [ENERGY_ROSE, 0, MINIMUM, 0] and ref.n_points.tolist() == [0, 1, 1, 1]
    assert ref.arc.tolist() == [0.0, 0.05, 0.05, 0.05]
    ref.propose(x + dr, np.full(4, -1e-3), f, None)
    assert ref.pending[0] is None and ref.pending[2] is None
    ref.judge(np.full(4, -2e-3), f, True)
    assert ref.reason.tolist() == [ENERGY_ROSE, PATH_FULL, MINIMUM, PATH_FULL] and ref.n_points.tolist() == [0, 2, 1, 2]


# ---- the four-atom Lennard-Jones cluster, rehearsed in fp64 with exact Hessians at every point -------------------------------

_LJ = {}


def _lj_paths(masses, step):
    key = (tuple(masses), step)
    if key not in _LJ:
        x0, e0, mode = lj4_saddle()
        _LJ[key] = (e0, [run_lj_path(x0, sign * mode, masses, step, fmax=1e-6) for sign in (1.0, -1.0)])
    return _LJ[key]


def test_lj4_saddle_of_the_rehearsal():
    x0, e0, mode = lj4_saddle()
    assert abs(e0 - LJ4_SADDLE) < 1e-9 and abs(np.linalg.norm(mode) - 1.0) < 1e-12


def test_lj4_path_at_step_0p05():
    """Both branches reach the tetrahedron (-6 eps) in 24 points, the energy falling at every one, path length 1.064."""
    e0, branches = _lj_paths((1.0, 1.0, 1.0, 1.0), 0.05)
    for ref in branches:
        assert ref.reason[0] == MINIMUM and ref.n_points[0] == 24
        assert abs(ref.path_e[0][-1] + 6.0) < 1e-9
        assert np.all(np.diff([e0] + ref.path_e[0]) < 0.0)
        assert ref.arc[0] == pytest.approx(1.064, abs=5e-4)


def test_lj4_path_length_converges():
    e0, branches = _lj_paths((1.0, 1.0, 1.0, 1.0), 0.0125)
    for ref in branches:
        assert ref.reason[0] == MINIMUM and abs(ref.path_e[0][-1] + 6.0) < 1e-9
        assert ref.arc[0] == pytest.approx(1.0316, abs=5e-5)


def test_lj4_path_with_unequal_masses():
    """Masses (1, 4, 9, 16): both branches reach -6 eps, path length 2.561 (54 points to fmax 1e-6; the last is a landing)."""
    e0, branches = _lj_paths((1.0, 4.0, 9.0, 16.0), 0.05)
    for ref in branches:
        assert ref.reason[0] == MINIMUM and ref.n_points[0] in (53, 54)
        assert abs(ref.path_e[0][-1] + 6.0) < 1e-9 and np.all(np.diff([e0] + ref.path_e[0]) < 0.0)
        assert ref.arc[0] == pytest.approx(2.561, abs=5e-4)


def test_lj4_step_too_long_ends_with_energy_rose():
    """The documented failure mode: at step 0.1 the LQA point overshoots the valley floor near the minimum; the run stops with
    ENERGY_ROSE after 10 points, 0.067 eps above the minimum.  There is no step-size control: halve the step."""
    e0, branches = _lj_paths((1.0, 1.0, 1.0, 1.0), 0.1)
    for ref in branches:
        assert ref.reason[0] == ENERGY_ROSE and ref.n_points[0] == 10
        assert ref.path_e[0][-1] + 6.0 == pytest.approx(0.067, abs=1e-3)


# ---- the lock-step cases of the GPU test, rehearsed on the oracle's surface ------------------------------------------------

@pytest.mark.parametrize("hessian_every", [1, 4])
@pytest.mark.parametrize("base", ["rand_batch_ani2x", "water_pbc_ani2x"])
def test_lockstep_cases_commit_points(base, hessian_every):
    """At LOCKSTEP_STEP every entry commits at least 4 of 8 points, and no step proposed comes within 1e-6 of the landing
    threshold (the pairs the GPU test may skip).  Measured at 0.05, the first value tried (0.025 gives the same): see REHEARSAL
    below."""
    g = load_golden(base)
    counts, reasons, margins = oracle_lockstep(g, hessian_every, 8, LOCKSTEP_STEP)
    print(f"{base}, hessian_every {hessian_every}, step {LOCKSTEP_STEP}: committed {counts}, reasons {reasons}, smallest "
          f"landing margin {min(margins):.2e}")
    assert len(counts) == g["species"].shape[0] and min(counts) >= 4
    assert min(margins) >= 1e-6
    assert (counts, reasons) == REHEARSAL[base]


# measured, for hessian_every 1 and 4 alike: every entry commits all 8 points and ends with PATH_FULL; on these random
# geometries a moving mode always has a negative eigenvalue, so no step has a landing threshold (all margins inf)
REHEARSAL = {"rand_batch_ani2x": ([8] * 6, [PATH_FULL] * 6), "water_pbc_ani2x": ([8], [PATH_FULL])}


# ---- the library and the refusals that need no device ----------------------------------------------------------------------

def test_library_exports_the_irc_entry_points():
    from torchani_amd import _lib

    _lib.build()
    with open(os.path.join(ROOT, "include", "anihip.h")) as fh:
        hdr = fh.read()
    declared = set(re.findall(r"\b(anihip_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    L = _lib.lib()
    for name in ("anihip_irc_workspace_bytes", "anihip_irc_project", "anihip_irc_step", "anihip_irc_commit"):
        assert name in declared and "irc.hip" in _lib.SOURCES
        getattr(L, name)
    for name, value in (("BAD_TABLE", _lib.IRC_BAD_TABLE), ("NONFINITE", _lib.IRC_NONFINITE), ("NO_ROOT", _lib.IRC_NO_ROOT),
                        ("MINIMUM", _lib.IRC_MINIMUM), ("ENERGY_ROSE", _lib.IRC_ENERGY_ROSE), ("PATH_FULL", _lib.IRC_PATH_FULL)):
        assert re.search(rf"#define\s+ANIHIP_IRC_{name}\s+{value}\b", hdr), name
    assert (MINIMUM, ENERGY_ROSE, PATH_FULL) == (_lib.IRC_MINIMUM, _lib.IRC_ENERGY_ROSE, _lib.IRC_PATH_FULL)
    assert ctypes.sizeof(_lib.Irc) == 4 * 4 + 3 * 8 + 16 * 8 + 8


def test_workspace_bytes_match_library_and_header_formula():
    from torchani_amd import _lib
    from torchani_amd.geomopt import SADDLE_MAX_COORDS, irc_workspace_bytes

    _lib.build()
    L = _lib.lib()

    def header(C, A):   # q, b fp64 [C][6][n] | gproj, w, displacement, xi fp64 [C][n] | old coords fp32 [C][n] | scalars [C][8]
        n = 3 * A
        up = lambda b: (b + 255) // 256 * 256   # noqa: E731
        return 2 * up(C * 6 * n * 8) + 4 * up(C * n * 8) + up(C * n * 4) + up(C * 64)

    for C, A in [(1, 1), (5, 4), (6, 14), (256, 28), (3, 86), (1, 90), (2, SADDLE_MAX_COORDS // 3)]:
        assert L.anihip_irc_workspace_bytes(C, A) == irc_workspace_bytes(C, A) == header(C, A), (C, A)
    assert L.anihip_irc_workspace_bytes(1, SADDLE_MAX_COORDS // 3 + 1) == 0 and b"atoms_per_mol" in L.anihip_last_error()
    assert L.anihip_irc_workspace_bytes(0, 3) == 0
    with pytest.raises(ValueError):
        irc_workspace_bytes(1, SADDLE_MAX_COORDS // 3 + 1)


def test_entry_points_refuse_bad_states_before_any_launch():
    """Null pointers and sizes out of range return nonzero with a message; nothing is launched (this runs without a device)."""
    from torchani_amd import _lib

    _lib.build()
    L = _lib.lib()
    buf = (ctypes.c_double * 4096)()
    p = ctypes.addressof(buf)

    def state(**kw):
        st = _lib.Irc(1, 2, 0, 4, 0.05, 1e-3, 1e-7, p, p, p, p, p, p, None, p, p, p, p, p, p, p, p, p, 1 << 20)
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    calls = (lambda st: L.anihip_irc_project(None, ctypes.byref(st), p), lambda st: L.anihip_irc_step(None, ctypes.byref(st), p, p),
             lambda st: L.anihip_irc_commit(None, ctypes.byref(st), p, p, 1))
    bad = [dict(masses=None), dict(path_coords=None), dict(reason=None), dict(workspace=None), dict(n_mol=0),
           dict(atoms_per_mol=0), dict(atoms_per_mol=_lib.SADDLE_MAX_COORDS // 3 + 1), dict(step=0.0), dict(step=float("nan")),
           dict(step=float("inf")), dict(max_points=0), dict(fmax=-1.0), dict(energy_floor=-1.0), dict(workspace_bytes=64)]
    for kw in bad:
        for call in calls:
            assert call(state(**kw)) != 0, kw
            assert L.anihip_last_error()
    assert L.anihip_irc_project(None, ctypes.byref(state()), None) != 0
    assert L.anihip_irc_step(None, ctypes.byref(state()), None, p) != 0 and L.anihip_irc_step(None, ctypes.byref(state()), p, None) != 0
    assert L.anihip_irc_commit(None, ctypes.byref(state()), None, p, 0) != 0
    assert L.anihip_irc_commit(None, ctypes.byref(state()), p, None, 0) != 0
    assert L.anihip_irc_project(None, None, p) != 0


def _cpu_inputs(A=3):
    return torch.zeros((2, A), dtype=torch.long), torch.zeros((2, A, 3))


@pytest.mark.parametrize("kw, error, match", [
    ({"constraints": object()}, NotImplementedError, "constraints"),
    ({"neighbors": object()}, NotImplementedError, "external neighbor"),
    ({"hessian_every": 0}, ValueError, "hessian_every"),
    ({"step": 0.0}, ValueError, "step"),
    ({"step": float("nan")}, ValueError, "step"),
    ({"step": float("inf")}, ValueError, "step"),
    ({"max_points": 0}, ValueError, "max_points"),
    ({"max_points": 2.5}, ValueError, "max_points"),
    ({"fmax": -1.0}, ValueError, "fmax"),
    ({"masses": torch.ones(3)}, ValueError, "masses"),
    ({"masses": torch.ones((2, 4))}, ValueError, "masses"),
    ({"direction": torch.zeros((2, 3))}, ValueError, "direction"),
    ({"fixed": torch.zeros(3, dtype=torch.bool)}, ValueError, "fixed"),
    ({"energy_floor": -1.0}, ValueError, "energy_floor"),
])
def test_bad_arguments_raise_before_device_work(kw, error, match):
    from torchani_amd.geomopt import ReactionPathFollower

    sp, x = _cpu_inputs()
    with pytest.raises(error, match=match):
        ReactionPathFollower(None, sp, x, **kw)


def test_too_many_coordinates_shapes_and_cpu_tensors_raise():
    from torchani_amd.geomopt import SADDLE_MAX_COORDS, ReactionPathFollower

    sp, x = _cpu_inputs(SADDLE_MAX_COORDS // 3 + 1)
    with pytest.raises(ValueError, match="SADDLE_MAX_COORDS"):
        ReactionPathFollower(None, sp, x)
    sp, x = _cpu_inputs()
    with pytest.raises(ValueError, match=r"\[C, A, 3\]"):
        ReactionPathFollower(None, sp, x[:, :2])
    with pytest.raises(ValueError, match="ROCm"):
        ReactionPathFollower(None, sp, x, masses=torch.ones((2, 3)))


def test_models_without_hessians_and_bad_saddles_raise_on_the_host():
    from torchani_amd.geomopt import ReactionPathFollower, follow_reaction_path
    from torchani_amd.models import ANI2dr, ANI2x
    from torchani_amd.tuples import OptimizedSaddles

    sp, x = _cpu_inputs()
    with pytest.raises(NotImplementedError, match="TwoBodyDispersionD3"):
        ReactionPathFollower(ANI2dr(seed=0, n_members=2), sp, x)
    model = ANI2x(seed=0, n_members=2)
    model.requires_grad_(True)
    with pytest.raises(RuntimeError, match="frozen parameters"):
        ReactionPathFollower(model, sp, x)
    z = torch.zeros(2)
    for converged, n_negative, entry in (([True, False], [1, 1], 1), ([True, True], [2, 1], 0), ([True, True], [1, 0], 1)):
        saddles = OptimizedSaddles(sp, x, z, x, torch.tensor(converged), z.int(), z, x.double(), torch.tensor(n_negative))
        with pytest.raises(ValueError, match=f"entry {entry} is not a first-order saddle"):
            follow_reaction_path(None, sp, saddles)
