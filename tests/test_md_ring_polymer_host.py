"""CPU checks of the ring-polymer integrator's definition (tests/_md_ring_polymer_ref.py, the fp64 restatement of
include/anihip.h that the GPU tests compare the kernels with): the mode matrix, the exact free propagation, the stationary law
of the thermostatted free ring polymer, the kinetic-energy estimators, and the declarations of the new entry points."""
import os
import re

import numpy as np
import pytest

import _md_ring_polymer_ref as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("P", [2, 3, 5, 8, 64])
def test_mode_matrix_is_orthogonal_and_diagonalizes_the_springs(P):
    Cm = rp.mode_matrix(P)
    assert np.abs(Cm.T @ Cm - np.eye(P)).max() <= 1e-13
    assert np.abs(Cm @ Cm.T - np.eye(P)).max() <= 1e-13
    # C^T K C = diag(omega_k^2) in units of omega_P = 1 (kT = hbar / P)
    om = rp.mode_frequencies(P, rp.HBAR / P)
    assert np.abs(Cm.T @ rp.spring_matrix(P) @ Cm - np.diag(om ** 2)).max() <= 1e-12
    # columns k > 0 sum to zero: the modes of the positions are the modes of the offsets from the centroid
    assert np.abs(Cm[:, 1:].sum(axis=0)).max() <= 1e-13


def _free_energy(x, v, mass, P, kT):
    """sum_j 1/2 m v_j^2 + 1/2 m omega_P^2 (q_j - q_j+1)^2 per polymer, amu A^2 / fs^2."""
    R = x.shape[0] // P
    q, vel = x.reshape(R, P, -1, 3), v.reshape(R, P, -1, 3)
    m = mass.reshape(R, P, -1)[:, :, :, None]
    wP = (P * kT / rp.HBAR)[:, None, None, None]
    return (0.5 * m * vel ** 2 + 0.5 * m * wP ** 2 * (q - np.roll(q, -1, axis=1)) ** 2).sum(axis=(1, 2, 3))


@pytest.mark.parametrize("P", [2, 5, 8])
def test_free_propagation_conserves_the_ring_polymer_energy(P):
    rs = np.random.RandomState(P)
    R, A = 2, 7
    x = np.repeat(rs.uniform(-5, 5, (R, 1, A, 3)), P, axis=1).reshape(R * P, A, 3) + rs.normal(0, 0.1, (R * P, A, 3))
    v = rs.normal(0, 0.02, (R * P, A, 3))
    mass = np.repeat(rs.choice([1.008, 12.011, 15.999], (R, A)), P, axis=0)
    kT = rp.KB_HARTREE * np.array([300.0, 120.0])
    active = np.ones((R * P, A), dtype=bool)
    zero = np.zeros_like(x)
    e0 = _free_energy(x, v, mass, P, kT)
    worst = 0.0
    for _ in range(1000):
        x, v = rp.drift(x, v, zero, active, mass, 0.7, P, kT)
        worst = max(worst, np.abs(_free_energy(x, v, mass, P, kT) / e0 - 1.0).max())
    print(f"ring polymer reference, P = {P}: 1000 free steps, max |E / E0 - 1| = {worst:.2e}")
    assert worst <= 1e-12


def _thermalized(R, P, A, T, dt, friction, lam, steps, seed):
    """The reference PILE step with zero forces from collapsed beads at rest; returns x, v, mass."""
    rs = np.random.RandomState(7)
    mass = np.repeat(rs.choice([1.008, 12.011, 15.999], (R, A)), P, axis=0)
    x = np.repeat(rs.uniform(-5, 5, (R, 1, A, 3)), P, axis=1).reshape(R * P, A, 3)
    v = np.zeros_like(x)
    kT = np.full(R, rp.KB_HARTREE * T)
    active = np.ones((R * P, A), dtype=bool)
    for s in range(steps):
        x, v = rp.drift(x, v, np.zeros_like(x), active, mass, dt, P, kT, True, np.full(R, friction), lam,
                        rp.noise(seed, s, R * P, A))
    return x, v, mass


@pytest.mark.parametrize("lam", [1.0, 0.5])
def test_thermostatted_free_ring_polymer_has_the_exact_mode_variances(lam):
    """O and A each preserve the Gaussian of the free ring polymer at any dt: <u_k^2> = P kT / (m omega_k^2) for k > 0.  300
    steps of 1 fs from collapsed beads (the slowest mode forgets its start as exp(-2 lam omega_1 t), omega_1 = 0.22 / fs); a
    mode has 3 A = 1800 samples, and the mean of u^2 / <u^2> has the standard error sqrt(2 / 1800)."""
    R, P, A, T = 1, 4, 600, 300.0
    x, v, mass = _thermalized(R, P, A, T, 1.0, 0.5, lam, 300, seed=5)
    Cm = rp.mode_matrix(P)
    u = x.reshape(P, A, 3).transpose(1, 2, 0) @ Cm          # [A, 3, P]
    om = rp.mode_frequencies(P, rp.KB_HARTREE * T)
    m = mass[0][:, None]
    for k in range(1, P):
        ratio = (u[..., k] ** 2 / (P * rp.KB_HARTREE * T * rp.ACC_UNIT / (m * om[k] ** 2))).mean()
        print(f"ring polymer reference, lambda {lam}: mode {k}  <u^2> / (P kT / m omega^2) = {ratio:.4f}")
        assert abs(ratio - 1.0) <= 5.0 * np.sqrt(2.0 / (3 * A))
    # and the bead velocities are Maxwell-Boltzmann at P T
    t_kin = (mass[..., None] * v ** 2).sum() / rp.ACC_UNIT / (3 * A * P * rp.KB_HARTREE) / (P * T)
    assert abs(t_kin - 1.0) <= 5.0 * np.sqrt(2.0 / (3 * A * P))


def test_both_kinetic_estimators_give_half_kT_per_component_on_a_free_particle():
    """Zero forces: the centroid-virial estimator is 3 N kT / 2 identically (W = 0), and the primitive one, 3 N P kT / 2 - S / P,
    averages to it; per component that is kT / 2, checked within 5 standard errors of the 1800 components' own scatter."""
    R, P, A, T = 1, 4, 600, 300.0
    x, v, mass = _thermalized(R, P, A, T, 1.0, 0.5, 1.0, 300, seed=9)
    kT = rp.KB_HARTREE * T
    active = np.ones((P, A), dtype=bool)
    S, W, _, _, cen = rp.estimators(x, np.zeros_like(x), active, mass, P, np.array([kT]))
    assert W[0] == 0.0
    assert np.allclose(cen[0], x.reshape(P, A, 3).mean(axis=0), rtol=0, atol=1e-13)
    q = x.reshape(P, A, 3)
    wP = P * kT / rp.HBAR
    s_comp = (0.5 * mass[0][None, :, None] * wP ** 2 * (q - np.roll(q, -1, axis=0)) ** 2).sum(axis=0) / rp.ACC_UNIT   # [A, 3]
    assert abs(s_comp.sum() / S[0] - 1.0) <= 1e-12
    prim = 0.5 * P * kT - s_comp / P
    mean, err = prim.mean(), prim.std(ddof=1) / np.sqrt(prim.size)
    print(f"ring polymer reference: primitive estimator per component / (kT / 2) = {mean / (0.5 * kT):.4f} +- {err / (0.5 * kT):.4f}")
    assert abs(mean - 0.5 * kT) <= 5.0 * err
    assert abs((1.5 * A * P * kT - S[0] / P) / (1.5 * A * kT) - 1.0) <= 5.0 * err / (0.5 * kT)


def test_free_ring_polymer_gates_hold_for_the_reference_with_the_gpu_tests_seed():
    """The stationary-law test of tests/test_gpu_md_ring_polymer.py, run on the fp64 reference with the same noise."""
    R, P, A, T, dt, friction, steps, seed = rp.FREE_CASE
    rs = np.random.RandomState(2)
    mass = np.repeat(np.array([1.008, 12.011, 14.007, 15.999, 32.06, 18.998, 35.45])[rs.randint(0, 7, (R, A))], P, axis=0)
    x, v = np.zeros((R * P, A, 3)), np.zeros((R * P, A, 3))
    active = np.ones((R * P, A), dtype=bool)
    kT = np.full(R, rp.KB_HARTREE * T)
    zero = np.zeros_like(x)
    for s in range(steps):
        x, vm = rp.drift(x, v, zero, active, mass, dt, P, kT, True, np.full(R, friction), 1.0, rp.noise(seed, s, R * P, A))
        v, ke = rp.kick(vm, zero, active, mass, dt)
    spread, se, t_ratio, t_gate = rp.free_polymer_figures(x, ke, mass, P, T)
    print(f"ring polymer reference, free polymer: spread {spread:.4f} (5 se = {5 * se:.4f}), T_bead / (P T) = {t_ratio:.4f} "
          f"(gate {t_gate:.4f})")
    assert abs(spread - 1.0) <= 5.0 * se and abs(t_ratio - 1.0) <= t_gate


def test_entry_points_are_declared_and_bound():
    from torchani_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "anihip.h")).read()
    declared = set(re.findall(r"\b(anihip_[a-z_0-9]+)\s*\(", hdr))
    for name in ("anihip_md_rp_drift", "anihip_md_rp_estimators"):
        assert name in declared and name in _lib.EXPORTED_SYMBOLS
    assert re.search(r"#define\s+ANIHIP_MD_HBAR\s+0\.024188843265857\b", hdr) and _lib.MD_HBAR == rp.HBAR == 0.024188843265857
    assert re.search(r"#define\s+ANIHIP_MD_RP_MAX_BEADS\s+64\b", hdr) and _lib.MD_RP_MAX_BEADS == 64
    from torchani_amd.md import BatchedDynamics, RingPolymerDynamics

    assert issubclass(RingPolymerDynamics, BatchedDynamics)
    # it overrides the drift and the draw of velocities, nothing else of the step
    for name in ("step", "run", "_kick", "_evaluate", "raise_on_overflow", "kinetic_energies", "temperatures"):
        assert name not in RingPolymerDynamics.__dict__
