"""fp64 numpy restatement of anihip_md_barostat (include/anihip.h has the definition): one move of isotropic stochastic cell
rescaling (Bernetti and Bussi 2020) per molecule, its noise word, and the ideal-gas dynamics that the statistical tests run
(drift, barostat, kick of tests/_md_ref.py with zero forces and a zero virial)."""
import numpy as np

import _md_ref as ref

BAROSTAT_STEP = 1 << 62                      # ANIHIP_MD_BAROSTAT_STEP
BAR_PER_HARTREE_ANGSTROM3 = 4.3597447222071e7   # what torchani_amd.md converts ``pressure`` with


def noise_word(step):
    """The Philox step word of the barostat's draw that goes with the drift of ``step``."""
    assert 0 <= step < BAROSTAT_STEP
    return BAROSTAT_STEP | step


def barostat_noise(seed, step, n_mol, replica_ids=None):
    """xi_b [C]: the xi_x of atom 0 of every molecule at the barostat's word."""
    return ref.noise(seed, noise_word(step), n_mol, 1, replica_ids)[:, 0, 0]


def volume(cell):
    """|det| of cell [C, 3, 3]."""
    return np.abs(np.linalg.det(np.asarray(cell, dtype=np.float64).reshape(-1, 3, 3)))


def barostat(x, v, cell, kinetic, virial, active, kT, pressure, beta_T, tau_p, dt, xi_b):
    """One move.  x, v [C, A, 3], cell [C, 3, 3], kinetic [C] (Hartree), virial [C, 3, 3] (Hartree, dE/d strain), active [C, A]
    bool, kT [C] (Hartree), pressure [C] (Hartree / Angstrom^3), beta_T (Angstrom^3 / Hartree), tau_p and dt (fs), xi_b [C].
    Returns the new (x, v, cell, kinetic) and mu [C]; inactive atoms keep x and v."""
    x, v = np.asarray(x, dtype=np.float64), np.asarray(v, dtype=np.float64)
    cell = np.asarray(cell, dtype=np.float64).reshape(-1, 3, 3)
    K, kT, p0 = (np.asarray(a, dtype=np.float64) for a in (kinetic, kT, pressure))
    V = volume(cell)
    p_int = (2.0 * K - np.trace(np.asarray(virial, dtype=np.float64).reshape(-1, 3, 3), axis1=1, axis2=2)) / (3.0 * V)
    deps = -(beta_T / tau_p) * (p0 - p_int) * dt + np.sqrt(2.0 * kT * beta_T * dt / (V * tau_p)) * np.asarray(xi_b, dtype=np.float64)
    mu = np.exp(deps / 3.0)
    act = np.asarray(active, dtype=bool)[..., None]
    m = mu[:, None, None]
    return np.where(act, m * x, x), np.where(act, v / m, v), m * cell, K / mu ** 2, mu


def ideal_gas_setup(n_mol=64, n_atoms=8):
    """The ideal gas of the statistical tests: 8 argon-like atoms per replica at 300 K, beta_T = 1 / P0, dt / tau_p = 0.02,
    gamma dt = 0.1, P0 chosen so that the mean volume (N + 1) kT / P0 is 1000 Angstrom^3.  The cell starts at the mean volume
    and the velocities at rest: the 400 steps dropped are 8 tau_p and 40 / gamma."""
    kT = ref.KB_HARTREE * 300.0
    v_unit = 1000.0 / (n_atoms + 1)          # kT / P0, Angstrom^3
    p0 = kT / v_unit
    return dict(n_mol=n_mol, n_atoms=n_atoms, kT=kT, p0=p0, beta_T=1.0 / p0, dt=1.0, tau_p=50.0, friction=0.1, mass=39.948,
                side=1000.0 ** (1.0 / 3.0), v_unit=v_unit)


def ideal_gas_ratios(volumes, setup, drop=400):
    """<V> / ((N + 1) kT / P0) and Var V / ((N + 1) (kT / P0)^2) over the replicas and the steps kept: both 1 for the
    Gamma(N + 1) law of the NPT ideal gas."""
    vol = np.asarray(volumes, dtype=np.float64)[drop:]
    n1 = setup["n_atoms"] + 1
    return vol.mean() / (n1 * setup["v_unit"]), vol.var() / (n1 * setup["v_unit"] ** 2)


def ideal_gas_volumes(seed, n_steps, setup):
    """Volumes [n_steps, C] of the reference dynamics with the Philox noise of (seed, step, replica = molecule index)."""
    Cn, A = setup["n_mol"], setup["n_atoms"]
    x, v = np.zeros((Cn, A, 3)), np.zeros((Cn, A, 3))
    zero, active = np.zeros((Cn, A, 3)), np.ones((Cn, A), dtype=bool)
    mass = np.full((Cn, A), setup["mass"])
    kT, p0, fr = np.full(Cn, setup["kT"]), np.full(Cn, setup["p0"]), np.full(Cn, setup["friction"])
    cell = np.tile(np.eye(3) * setup["side"], (Cn, 1, 1))
    K, W = np.zeros(Cn), np.zeros((Cn, 3, 3))
    out = np.empty((n_steps, Cn))
    for s in range(n_steps):
        x, v = ref.drift(x, v, zero, active, mass, setup["dt"], True, kT, fr, ref.noise(seed, s, Cn, A))
        x, v, cell, K, _ = barostat(x, v, cell, K, W, active, kT, p0, setup["beta_T"], setup["tau_p"], setup["dt"],
                                    barostat_noise(seed, s, Cn))
        v, K = ref.kick(v, zero, active, mass, setup["dt"])
        out[s] = volume(cell)
    return out
