"""fp64 numpy restatement of the constraint definitions of include/anihip.h (anihip_geom_constraints_*): the projection of the
forces onto the tangent space of internal-coordinate constraints and the Newton restore onto their targets, on the CVs of
tests/_md_bias_ref.py.  The linear systems are solved by a dense ``np.linalg.solve``, deliberately not the Cholesky
factorization of the HIP kernels, so agreement checks both; only the singularity rule (a Cholesky pivot <= 1e-12 x the largest
diagonal element) is the definition's own.  Also the reference optimizer (tests/_geomopt_ref.py plus project and restore, the
coordinates rounded to fp32 at every step), a Lennard-Jones cluster, and the SLSQP oracle.  Loops are plain: it is read, not
timed."""
import math

import numpy as np

from _geomopt_ref import LbfgsReference
from _md_bias_ref import DIHEDRAL, N_ATOMS, cv, wrap

MAX_CONSTRAINTS = 8
BAD_TABLE, SINGULAR, NOT_CONVERGED = 1, 2, 4
PIVOT = 1e-12


class Tables:
    """The tables of ``geomopt.build_constraint_tables`` (or hand-made arrays) as numpy."""

    def __init__(self, offset, kind, atoms, target):
        as_np = lambda t: t.numpy() if hasattr(t, "numpy") else np.asarray(t)   # noqa: E731
        self.offset, self.kind = as_np(offset).astype(np.int64), as_np(kind).astype(np.int64)
        self.atoms, self.target = as_np(atoms).astype(np.int64).reshape(-1, 4), as_np(target).astype(np.float64)

    def rows(self, c):
        return range(int(self.offset[c]), int(self.offset[c + 1]))


def table_is_broken(t, c, A):
    lo, hi = int(t.offset[c]), int(t.offset[c + 1])
    if lo < 0 or hi < lo or hi > t.kind.shape[0] or hi - lo > MAX_CONSTRAINTS:
        return True
    for r in range(lo, hi):
        if t.kind[r] not in N_ATOMS:
            return True
        at = t.atoms[r, :N_ATOMS[int(t.kind[r])]]
        if np.any(at < c * A) or np.any(at >= (c + 1) * A) or len(set(at.tolist())) != len(at):
            return True
    return False


def jacobian(t, c, x, active):
    """s [n] and J [n, Natoms * 3] (dense over the flat batch) of entry c at x [Natoms, 3], the columns of atoms with
    active == 0 zeroed."""
    rows = list(t.rows(c))
    s, J = np.zeros(len(rows)), np.zeros((len(rows), x.shape[0], 3))
    for k, r in enumerate(rows):
        at = t.atoms[r, :N_ATOMS[int(t.kind[r])]]
        s[k], g = cv(int(t.kind[r]), x[at])
        J[k, at] = g * (active[at] != 0)[:, None]
    return s, J.reshape(len(rows), 3 * x.shape[0])


def singular(G):
    """The definition's rule: Cholesky in the stored order, a pivot <= PIVOT x the largest diagonal element (or not finite)."""
    if not np.isfinite(G).all():
        return True
    n = G.shape[0]
    L = np.zeros_like(G)
    least = PIVOT * G.diagonal().max()
    for j in range(n):
        d = G[j, j] - L[j, :j] @ L[j, :j]
        if not d > least:
            return True
        L[j, j] = math.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (G[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return False


def project(t, x32, f32, active):
    """x32, f32 fp32 [C, A, 3], active [C, A].  Returns forces (fp32), jtl (fp64, J^T lambda per atom), multipliers and values
    (fp64 [N], NaN where not written), status [C], cond [C] (of G, 0 without constraints)."""
    Cn, A = x32.shape[:2]
    x, f = x32.astype(np.float64).reshape(-1, 3), f32.astype(np.float64).reshape(-1)
    act = np.asarray(active).reshape(-1)
    N = t.kind.shape[0]
    out = {"forces": f32.copy(), "jtl": np.zeros((Cn, A, 3)), "multipliers": np.full(N, np.nan), "values": np.full(N, np.nan),
           "status": np.zeros(Cn, dtype=np.int64), "cond": np.zeros(Cn)}
    fo = out["forces"].reshape(-1)
    for c in range(Cn):
        if table_is_broken(t, c, A):
            out["status"][c] = BAD_TABLE
            continue
        rows = list(t.rows(c))
        if not rows:
            continue
        with np.errstate(all="ignore"):
            s, J = jacobian(t, c, x, act)
            G = J @ J.T
        if singular(G):
            out["status"][c] = SINGULAR
            continue
        lam = np.linalg.solve(G, J @ f)
        jtl = J.T @ lam
        named = np.unique(t.atoms[rows][t.atoms[rows] >= 0])
        idx = (3 * named[:, None] + np.arange(3)).reshape(-1)
        fo[idx] = (f[idx] - jtl[idx]).astype(np.float32)
        out["jtl"].reshape(-1)[idx] = jtl[idx]
        out["multipliers"][rows], out["values"][rows], out["cond"][c] = lam, s, np.linalg.cond(G)
    return out


def residual(t, c, s):
    rows = list(t.rows(c))
    r = s - t.target[rows]
    dih = t.kind[rows] == DIHEDRAL
    r[dih] = wrap(r[dih])
    return r


def restore(t, x32, active, tolerance, max_iterations, first_correction=None):
    """Returns coords (fp32 [C, A, 3]), values (fp64 [N], at the fp32 coordinates returned; NaN where not written),
    iterations [C] and status [C].  ``first_correction``: a dict that receives {c: (dx, J)} of every entry's first iteration."""
    Cn, A = x32.shape[:2]
    act = np.asarray(active).reshape(-1)
    N = t.kind.shape[0]
    out = {"coords": x32.copy(), "values": np.full(N, np.nan), "iterations": np.zeros(Cn, dtype=np.int64),
           "status": np.zeros(Cn, dtype=np.int64)}
    for c in range(Cn):
        if table_is_broken(t, c, A):
            out["status"][c] = BAD_TABLE
            continue
        rows = list(t.rows(c))
        if not rows:
            continue
        x = x32.astype(np.float64).reshape(-1, 3).copy()
        it, status = 0, 0
        while True:
            with np.errstate(all="ignore"):
                s, J = jacobian(t, c, x, act)
                r = residual(t, c, s)
            if np.abs(r).max() <= tolerance:
                break
            if it == max_iterations:
                status = NOT_CONVERGED
                break
            with np.errstate(all="ignore"):
                G = J @ J.T
            if singular(G):
                status = SINGULAR
                break
            dx = J.T @ np.linalg.solve(G, r)
            if it == 0 and first_correction is not None:
                first_correction[c] = (dx.copy(), J.copy())
            x -= dx.reshape(-1, 3)
            it += 1
        out["status"][c] = status
        if status:
            continue
        if it > 0:
            named = np.unique(t.atoms[rows][t.atoms[rows] >= 0])
            out["coords"].reshape(-1, 3)[named] = x[named].astype(np.float32)
            s, _ = jacobian(t, c, out["coords"].astype(np.float64).reshape(-1, 3), act)
        out["values"][rows], out["iterations"][c] = s, it
    return out


def residual_bound(t, c, x32, tolerance):
    """What |s_k - t_k| of entry c can be at restored fp32 coordinates x32 [C, A, 3]: the fp64 iterate met ``tolerance``, and
    rounding it moved every atom by at most sqrt(3) / 2 of the fp32 spacing u at the largest |x| of the constraint, so to
    first order |ds_k| <= sum_i |grad_i s_k| sqrt(3) u / 2 (a distance: two unit gradients, 1.7 u; an angle or a dihedral: the
    same divided by its arms).  [n]"""
    x = x32.astype(np.float64).reshape(-1, 3)
    out = []
    for r in t.rows(c):
        at = t.atoms[r, :N_ATOMS[int(t.kind[r])]]
        g = cv(int(t.kind[r]), x[at])[1]
        u = float(np.spacing(np.float32(np.abs(x[at]).max())))
        out.append(tolerance + np.linalg.norm(g, axis=1).sum() * math.sqrt(3.0) / 2.0 * u)
    return np.array(out)


# ---- the reference optimizer ---------------------------------------------------------------------------------------------------

class ConstrainedReference:
    """GeometryOptimizer(constraints=...) on the host: LbfgsReference on the projected forces, the restore after every step,
    the coordinates fp32.  ``forces(x64 [C, A, 3]) -> (energies [C], forces [C, A, 3])`` is the model."""

    def __init__(self, forces, x, active, tables, memory=100, maxstep=0.2, alpha=70.0 / 27.211386024367243, damping=1.0,
                 fmax=1e-5, tolerance=1e-8, max_iterations=32):
        self.model, self.t, self.active = forces, tables, np.asarray(active)
        self.tol, self.max_it = tolerance, max_iterations
        self.lb = LbfgsReference(x.shape[0], memory, maxstep, alpha, damping, fmax)
        self.x = self._restore(np.asarray(x).astype(np.float32))
        self._evaluate()

    def _restore(self, x32):
        out = restore(self.t, x32, self.active, self.tol, self.max_it)
        assert not out["status"].any(), out["status"]
        return out["coords"]

    def _evaluate(self):
        self.energies, f = self.model(self.x.astype(np.float64))
        p = project(self.t, self.x, f.astype(np.float32), self.active)
        assert not p["status"].any(), p["status"]
        self.forces, self.multipliers, self.values = p["forces"], p["multipliers"], p["values"]

    def step(self):
        dr = self.lb.step(self.x, self.forces, self.active)
        self.x = self._restore((self.x.astype(np.float64) + dr).astype(np.float32))
        self._evaluate()

    def run(self, steps=1000):
        for _ in range(steps):
            self.step()
            if self.lb.converged.all():
                break
        return self


# ---- the Lennard-Jones cluster and the independent oracle -----------------------------------------------------------------------

LJ_EPS, LJ_SIGMA = 0.005, 3.0   # Hartree, Angstrom


def lj(x, eps=LJ_EPS, sigma=LJ_SIGMA):
    """E and forces [A, 3] of one cluster x [A, 3] (fp64)."""
    d = x[:, None, :] - x[None, :, :]
    r2 = (d * d).sum(-1)
    np.fill_diagonal(r2, np.inf)
    q = (sigma * sigma / r2) ** 3
    E = 2.0 * eps * (q * q - q).sum()
    dE = 4.0 * eps * (-12.0 * q * q + 6.0 * q) / r2   # (dE/dr) / r per pair
    return E, -(dE[:, :, None] * d).sum(axis=1)


def lj_batch(x):
    out = [lj(xc) for xc in x]
    return np.array([e for e, _ in out]), np.stack([f for _, f in out])


def bipyramid():
    """The LJ7 pentagonal bipyramid near its minimum, in units of sigma = 3 A: ring atoms 0 .. 4, apices 5 and 6."""
    t = 2 * np.pi * np.arange(5) / 5
    ring = np.stack([0.95 * np.cos(t), 0.95 * np.sin(t), np.zeros(5)], axis=1)
    return np.vstack([ring, [[0.0, 0.0, 0.59], [0.0, 0.0, -0.59]]]) * LJ_SIGMA


def lj_minimum():
    """The bipyramid minimized in fp64 (scipy BFGS to |g| <= 1e-10), centred."""
    from scipy.optimize import minimize

    x0 = bipyramid()
    res = minimize(lambda v: lj(v.reshape(-1, 3))[0], x0.ravel(), jac=lambda v: -lj(v.reshape(-1, 3))[1].ravel(), method="BFGS",
                   options={"gtol": 1e-10, "maxiter": 2000})
    x = res.x.reshape(-1, 3)
    return x - x.mean(axis=0)


def cv_value(kind, atoms, x):
    return cv(kind, x[list(atoms)])[0]


def slsqp(x0, constraints):
    """The energy minimum of the cluster under the equality constraints [(kind, atoms, target), ...], in fp64 by SLSQP: the
    independent oracle.  Returns (E, x)."""
    from scipy.optimize import minimize

    def make(kind, atoms, target):
        def fun(v):
            r = cv_value(kind, atoms, v.reshape(-1, 3)) - target
            return wrap(r) if kind == DIHEDRAL else r

        def jac(v):
            g = np.zeros((x0.shape[0], 3))
            g[list(atoms)] = cv(kind, v.reshape(-1, 3)[list(atoms)])[1]
            return g.ravel()

        return {"type": "eq", "fun": fun, "jac": jac}

    res = minimize(lambda v: lj(v.reshape(-1, 3))[0] / LJ_EPS, x0.ravel(), jac=lambda v: -lj(v.reshape(-1, 3))[1].ravel() / LJ_EPS,
                   method="SLSQP", constraints=[make(*c) for c in constraints], options={"ftol": 1e-15, "maxiter": 1000})
    assert res.success, res.message
    return res.fun * LJ_EPS, res.x.reshape(-1, 3)
