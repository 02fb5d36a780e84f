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
    """The optimizer state of C molecules; ``step(x, f, active)`` returns the displacement [C, A, 3] of one step.

    ``pair_dtype=np.float32`` mirrors the pair storage of k_lb_dots: s and y are formed in fp64, rounded to fp32 and taken back
    to fp64 before the curvature test and before they are stored; everything after that stays fp64.

    Book-keeping of the decisions taken (it changes no result): ``accepted``, ``rejected`` and, of the rejected pairs, those met
    with a full history (``rejected_full``; ``rejected_full_curved`` those of them with s.y < 0, a real negative curvature, and
    ``rejected_full_wrapped`` those of these met after a pair had been dropped, when the spare slot holds an older pair's row), with
    an empty one (``rejected_empty``) and those of a molecule that did not move (``rejected_still``: sum |s_i y_i| = 0, s or y
    zero bit for bit for the kernel too, so they have no margin and are left out of it); steps scaled to maxstep (``clipped``) and
    not (``unclipped``); ``converged_at`` the step() call at which a molecule was found converged (-1: not yet); ``direction``
    the unscaled p = -H g of the last step; ``margin`` the smallest relative distance of a decision from its threshold:
    |s.y| / sum |s_i y_i|, |max |f_i| - fmax| / fmax and |longest - maxstep| / maxstep."""

    def __init__(self, n_mol, memory, maxstep, alpha, damping, fmax, pair_dtype=None):
        self.memory, self.maxstep, self.alpha, self.damping, self.fmax = memory, maxstep, alpha, damping, fmax
        self.pair_dtype = pair_dtype
        self.pairs = [[] for _ in range(n_mol)]
        self.x_prev = [None] * n_mol
        self.f_prev = [None] * n_mol
        self.converged = np.zeros(n_mol, dtype=bool)
        self.n_steps = np.zeros(n_mol, dtype=np.int64)
        self.rejected = np.zeros(n_mol, dtype=np.int64)   # pairs not stored: s.y <= 0
        self.accepted = np.zeros(n_mol, dtype=np.int64)
        self.rejected_full = np.zeros(n_mol, dtype=np.int64)
        self.rejected_empty = np.zeros(n_mol, dtype=np.int64)
        self.rejected_full_curved = np.zeros(n_mol, dtype=np.int64)
        self.rejected_full_wrapped = np.zeros(n_mol, dtype=np.int64)
        self.rejected_still = np.zeros(n_mol, dtype=np.int64)
        self.clipped = np.zeros(n_mol, dtype=np.int64)
        self.unclipped = np.zeros(n_mol, dtype=np.int64)
        self.converged_at = np.full(n_mol, -1, dtype=np.int64)
        self.direction = [None] * n_mol
        self.margin = {"curvature": np.inf, "fmax": np.inf, "maxstep": np.inf}
        self.calls = 0

    def _near(self, key, distance, scale):
        if scale > 0:
            self.margin[key] = min(self.margin[key], distance / scale)

    def step(self, x, f, active):
        x = np.asarray(x, dtype=np.float64)
        f = np.where(np.asarray(active, dtype=bool)[..., None], np.asarray(f, dtype=np.float64), 0.0)
        dr = np.zeros_like(x)
        for c in range(x.shape[0]):
            if self.converged[c]:
                continue
            largest = np.sqrt((f[c] ** 2).sum(axis=-1)).max()
            self._near("fmax", abs(largest - self.fmax), self.fmax)
            if largest < self.fmax:
                self.converged[c] = True
                self.converged_at[c] = self.calls
                continue
            xc, fc = x[c].ravel(), f[c].ravel()
            if self.x_prev[c] is not None:
                s, y = xc - self.x_prev[c], self.f_prev[c] - fc
                if self.pair_dtype is not None:
                    s, y = s.astype(self.pair_dtype).astype(np.float64), y.astype(self.pair_dtype).astype(np.float64)
                self._near("curvature", abs(np.dot(s, y)), np.abs(s * y).sum())
                if np.dot(s, y) > 0:
                    self.accepted[c] += 1
                    self.pairs[c].append((s, y))
                    if len(self.pairs[c]) > self.memory:
                        self.pairs[c].pop(0)
                else:
                    self.rejected[c] += 1
                    self.rejected_full[c] += len(self.pairs[c]) == self.memory
                    self.rejected_empty[c] += len(self.pairs[c]) == 0
                    self.rejected_full_curved[c] += len(self.pairs[c]) == self.memory and np.dot(s, y) < 0
                    self.rejected_full_wrapped[c] += (len(self.pairs[c]) == self.memory and np.dot(s, y) < 0
                                                      and self.accepted[c] > self.memory)
                    self.rejected_still[c] += np.abs(s * y).sum() == 0
            p = -two_loop(-fc, self.pairs[c], self.alpha)
            self.direction[c] = p.copy()
            longest = np.sqrt((p.reshape(-1, 3) ** 2).sum(axis=-1)).max()
            self._near("maxstep", abs(longest - self.maxstep), self.maxstep)
            if longest >= self.maxstep:
                p *= self.maxstep / longest
                self.clipped[c] += 1
            else:
                self.unclipped[c] += 1
            dr[c] = (p * self.damping).reshape(-1, 3)
            self.x_prev[c], self.f_prev[c] = xc, fc
            self.n_steps[c] += 1
        self.calls += 1
        return dr
