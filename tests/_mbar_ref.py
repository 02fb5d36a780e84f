"""fp64 numpy statement of the MBAR definitions of include/anihip.h (anihip_mbar_*): the reduced potential of a structured
problem, one self-consistent iteration exactly as defined there, a solver, the log weights, the asymptotic covariance in its
K x K form, the histogram of log weights, and an umbrella-sampling driver on Lennard-Jones dimers.  The GPU tests compare the
kernels and the class with it; the host tests check it against closed forms.  Every log-sum-exp is scipy's."""
import math

import numpy as np
from scipy.special import logsumexp

from _md_bias_ref import ACC_UNIT, DIHEDRAL, KB_HARTREE, dimer_free_energy, wrap


def reduced_potentials(beta, restraint, kinds, energy, cv):
    """u [K, N] = beta_k (E_n + sum_r 1/2 k e^2), e = max(0, |d| - hw), d = s - c (wrapped for a dihedral column), the sum
    over r in ascending order.  beta [K], restraint [K, R, 3], kinds [R], energy [N] or None, cv [N, R]."""
    beta, restraint = np.asarray(beta, dtype=np.float64), np.asarray(restraint, dtype=np.float64)
    K, R = restraint.shape[0], restraint.shape[1]
    N = cv.shape[0] if R else len(energy)
    bias = np.zeros((K, N))
    for r in range(R):
        d = cv[None, :, r] - restraint[:, None, r, 0]
        if kinds[r] == DIHEDRAL:
            d = wrap(d)
        e = np.maximum(0.0, np.abs(d) - restraint[:, None, r, 2])
        bias = bias + 0.5 * restraint[:, None, r, 1] * e * e
    E = np.zeros(N) if energy is None else np.asarray(energy, dtype=np.float64)
    return beta[:, None] * (E[None, :] + bias)


def denominators(u, n_k, f):
    """d_n = lse over the states with N_j > 0 of (ln N_j + f_j - u_j(x_n))."""
    on = n_k > 0
    return logsumexp(np.log(n_k[on])[:, None] + f[on, None] - u[on], axis=0)


def iterate(u, n_k, f):
    """One self-consistent iteration: (f', max |f' - f|), f'_k = -lse_n(-u_k(x_n) - d_n) shifted by f'_0."""
    d = denominators(u, n_k, f)
    new = -logsumexp(-u - d[None, :], axis=1)
    new = new - new[0]
    return new, np.abs(new - f).max()


def log_weights_all(u, n_k, f):
    """ln W [N, K] = f_k - u_k(x_n) - d_n."""
    return (f[:, None] - u - denominators(u, n_k, f)[None, :]).T


def log_weights(u, n_k, f, u_target):
    """ln W_n of a target state with reduced potential u_target [N], normalized over all samples."""
    a = -u_target - denominators(u, n_k, f)
    return a - logsumexp(a)


def solve(u, n_k, tolerance=1e-12, max_iterations=5000):
    """The converged f: Newton steps on the sampled states (the first of them pinned) while they lower the gradient norm, the
    self-consistent iteration otherwise; converged when an iteration moves f by less than ``tolerance``.  Returns (f,
    iterations)."""
    K = u.shape[0]
    on = np.flatnonzero(n_k > 0)
    free = on[1:]

    def gradient(f):
        return n_k * (np.exp(log_weights_all(u, n_k, f)).sum(axis=0) - 1.0)

    f = np.zeros(K)
    for it in range(1, max_iterations + 1):
        sci, delta = iterate(u, n_k, f)
        if delta < tolerance:
            return sci, it
        step = sci
        if free.size:
            W = np.exp(log_weights_all(u, n_k, f))
            g = n_k * (W.sum(axis=0) - 1.0)
            H = np.diag(n_k * W.sum(axis=0)) - (n_k[:, None] * (W.T @ W)) * n_k[None, :]
            try:
                nr = f.copy()
                nr[free] -= np.linalg.solve(H[np.ix_(free, free)], g[free])
                d = denominators(u, n_k, nr)   # (of the sampled states alone: the unsampled ones follow from it)
                off = n_k == 0
                nr[off] = -logsumexp(-u[off] - d[None, :], axis=1)
                nr = nr - nr[0]
                if np.all(np.isfinite(nr)) and np.linalg.norm(gradient(nr)) < np.linalg.norm(gradient(sci)):
                    step = nr
            except np.linalg.LinAlgError:
                pass
        f = step
    return f, max_iterations


def covariance(W, n_k):
    """Theta [K, K] of Shirts and Chodera (2008) from W^T W alone: with W^T W = V S^2 V^T,
    Theta = V S pinv(I - S V^T N V S) S V^T; eigenvalues of the inner matrix below 1e-10 of the largest count as zero."""
    s2, V = np.linalg.eigh(W.T @ W)
    S = np.sqrt(np.maximum(s2, 0.0))
    inner = np.eye(len(n_k)) - (S[:, None] * (V.T @ (n_k[:, None] * V))) * S[None, :]
    w, Q = np.linalg.eigh(0.5 * (inner + inner.T))
    inv = np.where(np.abs(w) > 1e-10 * np.abs(w).max(), 1.0 / np.where(w == 0.0, 1.0, w), 0.0)
    pinv = (Q * inv[None, :]) @ Q.T
    VS = V * S[None, :]
    return VS @ pinv @ VS.T


def uncertainties(W, n_k):
    """[K, K]: the standard error of f_i - f_j."""
    t = covariance(W, n_k)
    dg = np.diag(t)
    return np.sqrt(np.maximum(dg[:, None] + dg[None, :] - 2.0 * t, 0.0))


def histogram(log_w, cv, columns, lo, hi, bins):
    """(lse [prod bins], counts): the log-sum-exp of the log weights per bin.  In range: lo <= s < hi in every column; bin
    min(bins - 1, int((s - lo) * (bins / (hi - lo)))), the first column the slow index; -inf in an empty bin."""
    ok = ~np.isnan(log_w)
    idx = np.zeros(len(log_w), dtype=np.int64)
    for c, col in enumerate(columns):
        s = cv[:, col]
        with np.errstate(invalid="ignore"):
            ok &= (s >= lo[c]) & (s < hi[c])
            b = np.minimum(((np.where(ok, s, lo[c]) - lo[c]) * (bins[c] / (hi[c] - lo[c]))).astype(np.int64), bins[c] - 1)
        idx = idx * bins[c] + b
    B = int(np.prod(bins[:len(columns)]))
    out, counts = np.full(B, -np.inf), np.zeros(B, dtype=np.int64)
    for b in range(B):
        sel = ok & (idx == b)
        counts[b] = sel.sum()
        if counts[b]:
            out[b] = logsumexp(log_w[sel])
    return out, counts


def pmf(log_w, cv, columns, lo, hi, bins):
    """Free energy per bin in kT, the minimum at 0, inf in empty bins; and the counts."""
    lse, counts = histogram(log_w, cv, columns, lo, hi, bins)
    F = -lse
    return F - F[np.isfinite(F)].min(), counts


# ---- the harmonic case of the host and solver tests ----------------------------------------------------------------------------
HARMONIC_CENTERS = np.array([0.0, 0.6, 1.2, 1.8, 2.4, 1.0])
HARMONIC_K = np.array([4.0, 8.0, 16.0, 8.0, 4.0, 0.5])
HARMONIC_N = np.array([2000.0, 2000.0, 2000.0, 2000.0, 2000.0, 0.0])


def harmonic_case(seed):
    """Samples of the five sampled 1-D harmonic states u_k = 1/2 k_k (x - c_k)^2 at beta = 1: (restraint [6, 1, 3], n_k, cv
    [10000, 1], exact f of the five sampled states relative to state 0 = 1/2 ln(k_k / k_0))."""
    rs = np.random.RandomState(seed)
    x = np.concatenate([rs.normal(c, 1.0 / math.sqrt(k), int(n)) for c, k, n in zip(HARMONIC_CENTERS, HARMONIC_K, HARMONIC_N)])
    restraint = np.stack([HARMONIC_CENTERS, HARMONIC_K, np.zeros(6)], axis=1)[:, None, :]
    return restraint, HARMONIC_N.copy(), x[:, None], 0.5 * np.log(HARMONIC_K[:5] / HARMONIC_K[0])


# ---- umbrella sampling of a Lennard-Jones dimer -----------------------------------------------------------------------------------
UMBRELLA = dict(centers=np.arange(17) * 0.15 + 3.1, k=0.05, copies=64, eps=0.005, sigma=3.0, mass=12.011, T=300.0, dt=2.0,
                friction=0.05, steps=1000, every=10, discard=20, bins=48, lo=3.1, hi=5.5)


def dimer_umbrella(seed, p=UMBRELLA):
    """BAOAB as csrc/md.hip splits it, on copies x windows dimers from the window centres, the distance sampled after every
    ``every``-th step.  Returns (r [samples, entries], centre of each entry)."""
    rs = np.random.RandomState(seed)
    kT = KB_HARTREE * p["T"]
    c = np.repeat(p["centers"], p["copies"])
    n = len(c)
    x = np.zeros((n, 2, 3))
    x[:, 1, 0] = c
    mass, dt = p["mass"], p["dt"]
    v = rs.normal(size=(n, 2, 3)) * math.sqrt(kT * ACC_UNIT / mass)
    c1 = math.exp(-p["friction"] * dt)
    s_noise = math.sqrt(kT * (1.0 - c1 * c1) * ACC_UNIT / mass)

    def evaluate():
        d = x[:, 1] - x[:, 0]
        r = np.sqrt((d * d).sum(axis=1))
        q = (p["sigma"] / r) ** 6
        dU = 4.0 * p["eps"] * (-12.0 * q * q + 6.0 * q) / r + p["k"] * (r - c)
        f1 = -dU[:, None] * d / r[:, None]
        return r, np.stack([-f1, f1], axis=1)

    r, f = evaluate()
    series = []
    for step in range(1, p["steps"] + 1):
        v += 0.5 * dt * f * (ACC_UNIT / mass)
        x += 0.5 * dt * v
        v = c1 * v + s_noise * rs.normal(size=v.shape)
        x += 0.5 * dt * v
        r, f = evaluate()
        v += 0.5 * dt * f * (ACC_UNIT / mass)
        if step % p["every"] == 0:
            series.append(r.copy())
    return np.stack(series), c


def umbrella_error(r, centers_of_entries, p=UMBRELLA):
    """max |F_MBAR - F_exact| / kT over the bins, means removed, with the count of empty bins: the protocol of the GPU test
    (discard, one state per distinct centre, the PMF at the unbiased state on ``bins`` bins)."""
    kT = KB_HARTREE * p["T"]
    r = r[p["discard"]:]
    cv = r.reshape(-1, 1)
    centers = np.unique(centers_of_entries)
    n_k = np.array([(centers_of_entries == c).sum() * r.shape[0] for c in centers], dtype=np.float64)
    restraint = np.stack([centers, np.full(len(centers), p["k"]), np.zeros(len(centers))], axis=1)[:, None, :]
    beta = np.full(len(centers), 1.0 / kT)
    u = reduced_potentials(beta, restraint, [0], None, cv)
    f, _ = solve(u, n_k, tolerance=1e-10)
    lw = log_weights(u, n_k, f, np.zeros(cv.shape[0]))
    F, counts = pmf(lw, cv, [0], [p["lo"]], [p["hi"]], [p["bins"]])
    mid = p["lo"] + (np.arange(p["bins"]) + 0.5) * (p["hi"] - p["lo"]) / p["bins"]
    exact = dimer_free_energy(mid, p["eps"], p["sigma"], kT) / kT
    full = counts > 0
    err = np.abs((F[full] - F[full].mean()) - (exact[full] - exact[full].mean())).max()
    return err, int((~full).sum()), np.abs(exact - exact.mean()).max()
