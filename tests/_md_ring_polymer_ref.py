"""fp64 numpy restatement of the ring-polymer integrator of csrc/md.hip (include/anihip.h has the definition): the normal-mode
matrix, the BAOAB-PILE drift over the beads of a batch and the estimators.  Noise and kick are those of _md_ref.py."""
import numpy as np

from _md_ref import ACC_UNIT, KB_HARTREE, kick, noise  # noqa: F401  (re-exported for the tests)

HBAR = 0.024188843265857   # Hartree fs


def mode_matrix(P):
    """C [P, P], y_j = sum_k C_jk u_k: 1 / sqrt(P); sqrt(2 / P) cos(2 pi j k / P) for 0 < k < P / 2; (-1)^j / sqrt(P) for k = P / 2;
    sqrt(2 / P) sin(2 pi j k / P) for k > P / 2."""
    j, k = np.arange(P)[:, None], np.arange(P)[None, :]
    Cm = np.where(2 * k < P, np.sqrt(2.0 / P) * np.cos(2 * np.pi * j * k / P), np.sqrt(2.0 / P) * np.sin(2 * np.pi * j * k / P))
    Cm[:, 0] = 1.0 / np.sqrt(P)
    if P % 2 == 0:
        Cm[:, P // 2] = (-1.0) ** np.arange(P) / np.sqrt(P)
    return Cm


def mode_frequencies(P, kT):
    """omega_k [..., P] = 2 omega_P sin(k pi / P), omega_P = P kT / hbar, for kT [...] in Hartree."""
    return 2.0 * (P * np.asarray(kT, dtype=np.float64)[..., None] / HBAR) * np.sin(np.arange(P) * np.pi / P)


def spring_matrix(P):
    """K [P, P] with sum_j (y_j - y_j+1)^2 = y^T K y."""
    K = 2.0 * np.eye(P)
    for j in range(P):
        K[j, (j + 1) % P] -= 1.0
        K[(j + 1) % P, j] -= 1.0
    return K


def free_step(u, w, omega, h):
    """A(h) on modes u, w [..., P] with omega [..., P] (omega_0 = 0)."""
    om = np.where(omega > 0, omega, 1.0)
    c, s = np.cos(omega * h), np.sin(omega * h)
    u1 = np.where(omega > 0, u * c + w / om * s, u + h * w)
    w1 = np.where(omega > 0, -u * om * s + w * c, w)
    return u1, w1


def ou_step(w, omega, gamma0, lam, dt, P, kT, im, xi):
    """O on mode velocities w [..., P]: c_k w + sqrt(P kT (1 - c_k^2) im) xi, gamma_0 = gamma0, gamma_k = 2 lam omega_k."""
    gamma = 2.0 * lam * omega
    gamma[..., 0] = gamma0
    c = np.exp(-gamma * dt)
    return c * w + np.sqrt(P * kT * (-np.expm1(-2.0 * gamma * dt)) * im) * xi


def drift(x, v, f, active, mass, dt, P, kT, langevin=False, friction=None, lam=1.0, xi=None):
    """anihip_md_rp_drift: x, v, f [R P, A, 3], active and mass [R P, A] (those of each polymer's first bead count), kT and
    friction [R] (the physical kT in Hartree), xi [R P, A, 3] with row r P + k driving mode k.  Returns the new (x, v)."""
    Cn, A = np.asarray(active).shape
    R = Cn // P
    sh = lambda a: np.asarray(a, dtype=np.float64).reshape(R, P, A, 3).transpose(0, 2, 3, 1)   # noqa: E731  [R, A, 3, P]
    act = np.asarray(active, dtype=bool).reshape(R, P, A)[:, 0][:, :, None, None]
    im = (ACC_UNIT / np.asarray(mass, dtype=np.float64).reshape(R, P, A)[:, 0])[:, :, None, None]
    q, vel, frc = sh(x), sh(v), sh(f)
    Cm = mode_matrix(P)
    om = mode_frequencies(P, kT)[:, None, None, :]     # [R, 1, 1, P]
    kTb = np.asarray(kT, dtype=np.float64)[:, None, None, None]
    vel = vel + 0.5 * dt * frc * im
    u, w = q @ Cm, vel @ Cm                              # u_k = sum_j C_jk y_j
    if langevin:
        u, w = free_step(u, w, om, 0.5 * dt)
        g0 = np.asarray(friction, dtype=np.float64)[:, None, None]
        w = ou_step(w, om * np.ones_like(w), g0, lam, dt, P, kTb, im, sh(xi))
        u, w = free_step(u, w, om, 0.5 * dt)
    else:
        u, w = free_step(u, w, om, dt)
    q1, v1 = np.where(act, u @ Cm.T, q), np.where(act, w @ Cm.T, 0.0)
    back = lambda a: a.transpose(0, 3, 1, 2).reshape(Cn, A, 3)   # noqa: E731
    return back(q1), back(v1)


def estimators(x, f, active, mass, P, kT):
    """anihip_md_rp_estimators: the spring energies S [R] and centroid-virial sums W [R] over the active atoms, the sums of
    the absolute values of their terms (the scale of a rounding-error gate), and the centroids [R, A, 3]."""
    Cn, A = np.asarray(active).shape
    R = Cn // P
    q = np.asarray(x, dtype=np.float64).reshape(R, P, A, 3)
    frc = np.asarray(f, dtype=np.float64).reshape(R, P, A, 3)
    act = np.asarray(active, dtype=bool).reshape(R, P, A)[:, :1, :, None]
    m = np.asarray(mass, dtype=np.float64).reshape(R, P, A)[:, :1, :, None]
    wP = (P * np.asarray(kT, dtype=np.float64) / HBAR)[:, None, None, None]
    cen = q.mean(axis=1)
    spring = np.where(act, 0.5 * m * wP ** 2 * (q - np.roll(q, -1, axis=1)) ** 2, 0.0) / ACC_UNIT
    vir = np.where(act, (q - cen[:, None]) * frc, 0.0)
    return spring.sum(axis=(1, 2, 3)), vir.sum(axis=(1, 2, 3)), np.abs(spring).sum(axis=(1, 2, 3)), np.abs(vir).sum(axis=(1, 2, 3)), cen


# The free ring polymer with zero forces under PILE, from collapsed beads at rest: (R, P, A, T in K, dt in fs, centroid
# friction in 1 / fs, steps, seed).  The fp64 reference passes both gates below with this seed (test_md_ring_polymer_host.py).
FREE_CASE = (4, 8, 64, 300.0, 1.0, 0.5, 200, 20240611)


def free_polymer_figures(x, ke, mass, P, T):
    """x [R P, A, 3], ke [R P] (Hartree), mass [R P, A] of a thermalized free ring polymer.  A and O each preserve the
    stationary law at any dt: per atom and component sum_j (q_j - qbar)^2 = sum_k>0 u_k^2 with independent Gaussian u_k of
    variance sigma_k^2 = P kT / (4 m omega_P^2 sin^2(k pi / P)), whose sum over k is (kT / (4 m omega_P^2)) (P^2 - 1) / 3 P.
    Returns the mean over all samples of that sum over its expectation, the standard error of that mean, 2 sum sigma_k^4 /
    (sum sigma_k^2)^2 / n under the root, the mean bead kinetic temperature over P T and its gate 5 sqrt(2 / (3 A C))."""
    Cn, A = mass.shape
    R = Cn // P
    q = np.asarray(x, dtype=np.float64).reshape(R, P, A, 3)
    kT = KB_HARTREE * T
    wP = P * kT / HBAR
    m = mass.reshape(R, P, A)[:, 0][:, :, None]
    expect = kT * ACC_UNIT / (4.0 * m * wP ** 2) * (P * P - 1) / 3.0 * P
    sample = ((q - q.mean(axis=1, keepdims=True)) ** 2).sum(axis=1) / expect     # [R, A, 3]
    s2 = 1.0 / np.sin(np.arange(1, P) * np.pi / P) ** 2
    se = np.sqrt(2.0 * (s2 ** 2).sum() / s2.sum() ** 2 / sample.size)
    t_ratio = (2.0 * np.asarray(ke) / (3 * A * KB_HARTREE)).mean() / (P * T)
    return sample.mean(), se, t_ratio, 5.0 * np.sqrt(2.0 / (3 * A * Cn))
