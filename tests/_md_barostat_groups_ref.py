"""fp64 numpy restatement of anihip_md_group_terms and anihip_md_barostat_groups (include/anihip.h has the definition):
molecular cell rescaling, the barostat of tests/_md_barostat_ref.py with every constraint cluster of
tests/_md_constraints_ref.py moved as a rigid body, and the NPT ideal gas of rigid dimers that the statistical tests run."""
import numpy as np

import _md_barostat_ref as bref
import _md_constraints_ref as cref
import _md_ref as ref


def scaling_groups(active, mass, cons):
    """The clusters that move, as (molecule [G], atoms [G, n], m [G, n]) per cluster shape, and the mask [C, A] of the free
    atoms (active and in no cluster).  A cluster with an atom of w = 0 (an anchor) is left out of both."""
    active = np.asarray(active, dtype=bool)
    mass = np.asarray(mass, dtype=np.float64)
    free = active.copy()
    out = []
    for mol, atoms, _, _, _ in (cons.groups if cons is not None else []):
        m = mol[:, None]
        free[m, atoms] = False
        keep = (cons.w[m, atoms] != 0.0).all(axis=1)
        if keep.any():
            out.append((mol[keep], atoms[keep], mass[mol[keep][:, None], atoms[keep]]))
    return out, free


def centres(q, m, atoms, mol):
    """sum m q / sum m of every cluster: [G, 3]."""
    return (m[..., None] * q[mol[:, None], atoms]).sum(axis=1) / m.sum(axis=1)[:, None]


def group_terms(x, v, f, active, mass, cons):
    """K_mol [C] (Hartree): the free atoms' kinetic energy plus 1/2 M |V|^2 of every cluster; G [C] (Hartree): sum f . (x - X)
    over the atoms of every cluster.  x, v, f [C, A, 3], active [C, A] bool, mass [C, A] (amu), cons a cref.Constraints or None."""
    x, v, f = (np.asarray(a, dtype=np.float64) for a in (x, v, f))
    clusters, free = scaling_groups(active, mass, cons)
    K = 0.5 * (np.where(free, np.asarray(mass, dtype=np.float64), 0.0)[..., None] * v ** 2).sum(axis=(1, 2))
    G = np.zeros(x.shape[0])
    for mol, atoms, m in clusters:
        X, V = centres(x, m, atoms, mol), centres(v, m, atoms, mol)
        np.add.at(K, mol, 0.5 * m.sum(axis=1) * (V ** 2).sum(axis=1))
        np.add.at(G, mol, (f[mol[:, None], atoms] * (x[mol[:, None], atoms] - X[:, None])).sum(axis=(1, 2)))
    return K / ref.ACC_UNIT, G


def barostat_groups(x, v, cell, kinetic, kinetic_mol, virial, virial_mol, active, mass, cons, kT, pressure, beta_T, tau_p, dt, xi_b):
    """One move: ``bref.barostat`` with P_int = (2 K_mol - (tr W + G)) / (3 V), the free atoms rescaled and every cluster
    translated by (mu - 1) X, its velocities by (1 / mu - 1) V.  Returns the new (x, v, cell, kinetic, kinetic_mol) and mu [C]."""
    x, v = np.asarray(x, dtype=np.float64), np.asarray(v, dtype=np.float64)
    cell = np.asarray(cell, dtype=np.float64).reshape(-1, 3, 3)
    K, Km, G, kT, p0 = (np.asarray(a, dtype=np.float64) for a in (kinetic, kinetic_mol, virial_mol, kT, pressure))
    V = bref.volume(cell)
    p_int = (2.0 * Km - (np.trace(np.asarray(virial, dtype=np.float64).reshape(-1, 3, 3), axis1=1, axis2=2) + G)) / (3.0 * V)
    deps = -(beta_T / tau_p) * (p0 - p_int) * dt + np.sqrt(2.0 * kT * beta_T * dt / (V * tau_p)) * np.asarray(xi_b, dtype=np.float64)
    mu = np.exp(deps / 3.0)
    clusters, free = scaling_groups(active, mass, cons)
    s = mu[:, None, None]
    x1, v1 = np.where(free[..., None], s * x, x), np.where(free[..., None], v / s, v)
    for mol, atoms, m in clusters:
        X, Vc = centres(x, m, atoms, mol), centres(v, m, atoms, mol)
        x1[mol[:, None], atoms] = x[mol[:, None], atoms] + ((mu[mol] - 1.0)[:, None] * X)[:, None]
        v1[mol[:, None], atoms] = v[mol[:, None], atoms] + ((1.0 / mu[mol] - 1.0)[:, None] * Vc)[:, None]
    Km1 = Km / mu ** 2
    return x1, v1, s * cell, (K - Km) + Km1, Km1, mu


# ---- the NPT ideal gas of rigid bodies --------------------------------------------------------------------------------------

RIGID_GAS_PAIRS = [(0, 1), (2, 3), (4, 5)]   # three rigid dimers; atoms 6 and 7 are free: N_g = 5 scaling groups
RIGID_GAS_BOND = 1.0                         # Angstrom


def rigid_gas_setup():
    """``bref.ideal_gas_setup`` (64 replicas x 8 atoms) with kT / P0 = 1000 / (N_g + 1) Angstrom^3: the mean volume of the five
    groups is again 1000 Angstrom^3."""
    s = bref.ideal_gas_setup()
    s["n_groups"] = 5
    s["v_unit"] = 1000.0 / (s["n_groups"] + 1)
    s["p0"] = s["kT"] / s["v_unit"]
    s["beta_T"] = 1.0 / s["p0"]
    return s


def rigid_gas_state(setup):
    """x, pairs [C, 3, 2], lengths [C, 3]: every dimer along x, its first atom at the origin."""
    Cn, A = setup["n_mol"], setup["n_atoms"]
    x = np.zeros((Cn, A, 3))
    for _, j in RIGID_GAS_PAIRS:
        x[:, j, 0] = RIGID_GAS_BOND
    pairs = np.tile(np.array(RIGID_GAS_PAIRS, dtype=np.int64), (Cn, 1, 1))
    return x, pairs, np.full(pairs.shape[:2], RIGID_GAS_BOND)


def rigid_gas_ratios(volumes, setup, drop=400):
    """<V> / ((N_g + 1) kT / P0) and Var V / ((N_g + 1) (kT / P0)^2) over the replicas and the steps kept: both 1 for the
    Gamma(N_g + 1) law."""
    vol = np.asarray(volumes, dtype=np.float64)[drop:]
    n1 = setup["n_groups"] + 1
    return vol.mean() / (n1 * setup["v_unit"]), vol.var() / (n1 * setup["v_unit"] ** 2)


def rigid_gas_volumes(seed, n_steps, setup):
    """Volumes [n_steps, C] of constrained drift, ``barostat_groups``, constrained kick, ``group_terms`` with zero forces and a
    zero virial and the Philox noise of (seed, step, replica = molecule index)."""
    Cn, A = setup["n_mol"], setup["n_atoms"]
    x, pairs, lengths = rigid_gas_state(setup)
    v, zero, active = np.zeros((Cn, A, 3)), np.zeros((Cn, A, 3)), np.ones((Cn, A), dtype=bool)
    mass = np.full((Cn, A), setup["mass"])
    cons = cref.Constraints(pairs, lengths, active, mass)
    kT, p0, fr = np.full(Cn, setup["kT"]), np.full(Cn, setup["p0"]), np.full(Cn, setup["friction"])
    cell = np.tile(np.eye(3) * setup["side"], (Cn, 1, 1))
    K, W = np.zeros(Cn), np.zeros((Cn, 3, 3))
    Km, G = group_terms(x, v, zero, active, mass, cons)
    out = np.empty((n_steps, Cn))
    for s in range(n_steps):
        x, v = cref.drift(x, v, zero, active, mass, setup["dt"], cons, True, kT, fr, ref.noise(seed, s, Cn, A))
        x, v, cell, K, Km, _ = barostat_groups(x, v, cell, K, Km, W, G, active, mass, cons, kT, p0, setup["beta_T"], setup["tau_p"],
                                               setup["dt"], bref.barostat_noise(seed, s, Cn))
        v, K = cref.kick(x, v, zero, active, mass, setup["dt"], cons)
        Km, G = group_terms(x, v, zero, active, mass, cons)
        out[s] = bref.volume(cell)
    return out
