"""fp64 numpy reference of the semantics of torchani_amd.geomopt: ASE's LBFGS without line search, a pair stored only if its
curvature s.y is positive, every molecule on its own.  The inverse-Hessian product is the two-loop recursion (Nocedal 1980),
deliberately not the compact representation of the HIP kernels, so agreement checks both."""
import numpy as np


def two_loop(g, pairs, alpha):
    """H g for the L-BFGS inverse Hessian of pairs [(s, y), ...] (oldest first) with H0 = I / alpha."""
    q = g.copy()
    a = []
    for s, y in reversed(pairs):
        ai = np.dot(s, q) / np.dot(y, s)
        q -= ai * y
        a.append(ai)
    z = q / alpha
    for (s, y), ai in zip(pairs, reversed(a)):
        b = np.dot(y, z) / np.dot(y, s)
        z += s * (ai - b)
    return z


class LbfgsReference:
    """The optimizer state of C molecules; ``step(x, f, active)`` returns the displacement [C, A, 3] of one step."""

    def __init__(self, n_mol, memory, maxstep, alpha, damping, fmax):
        self.memory, self.maxstep, self.alpha, self.damping, self.fmax = memory, maxstep, alpha, damping, fmax
        self.pairs = [[] for _ in range(n_mol)]
        self.x_prev = [None] * n_mol
        self.f_prev = [None] * n_mol
        self.converged = np.zeros(n_mol, dtype=bool)
        self.n_steps = np.zeros(n_mol, dtype=np.int64)
        self.rejected = np.zeros(n_mol, dtype=np.int64)   # pairs not stored: s.y <= 0

    def step(self, x, f, active):
        x = np.asarray(x, dtype=np.float64)
        f = np.where(np.asarray(active, dtype=bool)[..., None], np.asarray(f, dtype=np.float64), 0.0)
        dr = np.zeros_like(x)
        for c in range(x.shape[0]):
            if self.converged[c]:
                continue
            if np.sqrt((f[c] ** 2).sum(axis=-1)).max() < self.fmax:
                self.converged[c] = True
                continue
            xc, fc = x[c].ravel(), f[c].ravel()
            if self.x_prev[c] is not None:
                s, y = xc - self.x_prev[c], self.f_prev[c] - fc
                if np.dot(s, y) > 0:
                    self.pairs[c].append((s, y))
                    if len(self.pairs[c]) > self.memory:
                        self.pairs[c].pop(0)
                else:
                    self.rejected[c] += 1
            p = -two_loop(-fc, self.pairs[c], self.alpha)
            longest = np.sqrt((p.reshape(-1, 3) ** 2).sum(axis=-1)).max()
            if longest >= self.maxstep:
                p *= self.maxstep / longest
            dr[c] = (p * self.damping).reshape(-1, 3)
            self.x_prev[c], self.f_prev[c] = xc, fc
            self.n_steps[c] += 1
        return dr
