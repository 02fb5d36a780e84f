"""fp64 numpy reference of the semantics of torchani_amd.geomopt.ReactionPathFollower (include/anihip.h: anihip_irc): the
intrinsic reaction coordinate by the local quadratic approximation on a model Hessian with Bofill updates, every molecule on
its own.  Deliberately another formulation than the HIP kernels': it works on the active coordinates only (the kernels keep all
3A and push the others to mu), the mass-weighted rigid motions are orthonormalized by QR factorisations (the kernels:
Gram-Schmidt), the projected Hessian is formed as P H_q P + mu Q Q^T with dense products (the kernels: a rank-12 correction),
the arc length s(t) comes from the closed form of the speed on a scale-free grid of Gauss-Legendre panels over all of [0, t]
(the kernels: panels marched from a first width set by the spectrum) and t by bisection (the kernels: Newton).  Agreement
checks both."""
import numpy as np

from _saddle_ref import RANK_TOL, bofill, lj_energy_forces, lj_hessian

RUNNING, MINIMUM, ENERGY_ROSE, PATH_FULL = 0, 1, 2, 3
LANDING = 40.0
# The arc length of a point in the lock-step cases of tests/test_gpu_irc.py (Angstrom amu^1/2), chosen by the rehearsal of
# tests/test_irc_host.py::test_lockstep_cases_commit_points: from 0.05, halved until every entry commits at least 4 of 8 points.
LOCKSTEP_STEP = 0.05

_GL_X, _GL_W = np.polynomial.legendre.leggauss(24)
# [0, t] = [0, 2^-52 t] and 52 octaves, every octave in two panels of 24 nodes: the grid resolves e^(-lam tau) at every
# lam t up to 2^52 alike, and a panel never spans more than 0.35 of its distance from 0
_EDGES = np.concatenate([[0.0], 2.0 ** (np.arange(-104, 1) / 2.0)])
_MID, _HALF = 0.5 * (_EDGES[1:] + _EDGES[:-1]), 0.5 * (_EDGES[1:] - _EDGES[:-1])
_NODES = (_MID[:, None] + _HALF[:, None] * _GL_X[None]).ravel()
_WEIGHTS = (_HALF[:, None] * _GL_W[None]).ravel()


def arc_length(lam, gt, t):
    """s(t) = the integral over [0, t] of (sum g~_i^2 e^(-2 lam_i tau))^1/2."""
    tau = t * _NODES
    with np.errstate(over="ignore"):
        speed = np.sqrt(((gt * gt)[None] * np.exp(-2.0 * lam[None] * tau[:, None])).sum(axis=1))
    return float(t * (_WEIGHTS * speed).sum())


def lqa_step(lam, gt, step):
    """The LQA step in the eigenbasis.  Returns (alpha, ds, landed, margin): the displacement, the arc increment, whether the
    step landed on the minimum of the model, and the landing margin |s(T) - step| / step at T = 40 / min lam (inf when a
    moving mode has lam <= 0: the path never ends)."""
    lam, gt = np.asarray(lam, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    mv = gt != 0.0
    alpha = np.zeros_like(gt)
    if not mv.any():
        return alpha, 0.0, False, np.inf
    l, g = lam[mv], gt[mv]
    margin, T = np.inf, np.inf
    if l.min() > 0.0:
        T = LANDING / l.min()
        sT = arc_length(l, g, T)
        margin = abs(sT - step) / step
        if sT < step:
            alpha[mv] = -g / l
            return alpha, sT, True, margin
    hi = min(step / np.linalg.norm(g), T)
    while arc_length(l, g, hi) < step:
        hi = min(2.0 * hi, T)
    lo = 0.0
    while True:
        mid = 0.5 * (lo + hi)
        if not lo < mid < hi:
            break
        if arc_length(l, g, mid) < step:
            lo = mid
        else:
            hi = mid
    t = hi
    with np.errstate(divide="ignore", invalid="ignore"):
        alpha[mv] = np.where(l == 0.0, -g * t, g * np.expm1(-l * t) / l)
    return alpha, float(step), False, margin


def rigid_basis_mw(x, m, translations, rotations):
    """Orthonormal basis [3 n_free, r] of the mass-weighted rigid motions of the free atoms x [n_free, 3] of masses m (about
    their centre of mass)."""
    k = x.shape[0]
    if k == 0:
        return np.zeros((0, 0))
    sm = np.sqrt(m)
    raw = []
    if translations:
        for j in range(3):
            v = np.zeros((k, 3))
            v[:, j] = sm
            raw.append(v.ravel())
    if rotations:
        r = x - (m[:, None] * x).sum(axis=0) / m.sum()
        for j in range(3):
            raw.append((sm[:, None] * np.cross(np.eye(3)[j], r)).ravel())
    Q = np.zeros((3 * k, 0))
    for v in raw:
        norm = np.linalg.norm(v)
        if norm == 0.0:
            continue
        q, r = np.linalg.qr(np.column_stack([Q, v]))
        if abs(r[-1, -1]) > RANK_TOL * norm:   # independent of the ones kept
            Q = q
    return Q


class IrcReference:
    """The follower's state of C molecules.  ``propose(x, e, f, H_exact)`` makes the projection and the step and returns the
    displacement [C, A, 3]; ``judge(e_new, f_new, bofill)`` makes the commit.  kind [C, A]: 0 padding, 1 free, 2 fixed; masses
    [C, A]; direction [C, A, 3] or None.  coord_dtype=np.float32 rounds the displacement and the moved coordinates like the
    device does."""

    def __init__(self, kind, masses, periodic, step, fmax, energy_floor, max_points, direction=None, coord_dtype=np.float32):
        self.kind = np.asarray(kind)
        C, A = self.kind.shape
        self.masses = np.asarray(masses, dtype=np.float64)
        self.periodic, self.step, self.fmax, self.energy_floor = bool(periodic), float(step), fmax, energy_floor
        self.max_points = int(max_points)
        self.direction = None if direction is None else np.asarray(direction, dtype=np.float64).reshape(C, 3 * A)
        self.coord_dtype = coord_dtype
        self.H = np.zeros((C, 3 * A, 3 * A))
        self.n_points = np.zeros(C, dtype=np.int64)
        self.reason = np.zeros(C, dtype=np.int64)
        self.arc = np.zeros(C)
        self.margin = np.full(C, np.inf)    # the landing margin of the step last proposed
        self.landed = np.zeros(C, dtype=bool)
        self.ds = np.zeros(C)
        self.path_x = [[] for _ in range(C)]
        self.path_e = [[] for _ in range(C)]
        self.path_s = [[] for _ in range(C)]
        self.pending = [None] * C

    def active(self, c):
        return np.repeat(self.kind[c] == 1, 3)

    def propose(self, x, e, f, H_exact=None):
        x = np.asarray(x, dtype=np.float64)
        f = np.asarray(f, dtype=np.float64)
        C, A = self.kind.shape
        dr = np.zeros((C, A, 3))
        for c in range(C):
            self.pending[c] = None
            self.margin[c], self.landed[c], self.ds[c] = np.inf, False, 0.0
            if self.reason[c] != RUNNING:
                continue
            if H_exact is not None:
                self.H[c] = 0.5 * (H_exact[c] + H_exact[c].T)
            free = self.kind[c] == 1
            act = self.active(c)
            w = np.repeat(self.masses[c][free], 3) ** -0.5
            g = -f[c].ravel()[act] * w
            Hq = w[:, None] * self.H[c][np.ix_(act, act)] * w[None, :]
            no_fixed = not np.any(self.kind[c] == 2)
            Q = rigid_basis_mw(x[c][free], self.masses[c][free], no_fixed, no_fixed and not self.periodic)
            P = np.eye(g.size) - Q @ Q.T
            mu = 1.0 + (np.abs(Hq).sum(axis=1).max() if g.size else 0.0)
            lam, V = np.linalg.eigh(P @ Hq @ P + mu * (Q @ Q.T))
            if self.n_points[c] == 0 and self.direction is not None:
                ov = V[:, 0] @ (self.direction[c][act] / w)
                dq = (-self.step if ov < 0.0 else self.step) * V[:, 0]
                ds, zero = self.step, False
            else:
                gt = V.T @ (P @ g)
                alpha, ds, self.landed[c], self.margin[c] = lqa_step(lam, gt, self.step)
                dq = V @ alpha
                zero = not np.any(gt != 0.0)
            s = np.zeros(3 * A)
            s[act] = w * dq
            x0 = x[c].ravel().astype(self.coord_dtype)
            x1 = x0 + s.astype(self.coord_dtype)
            disp = x1.astype(np.float64) - x0.astype(np.float64)
            ds = max(ds, float(np.linalg.norm(disp[act] / w)))   # never below the chord between the stored points
            dr[c] = s.astype(self.coord_dtype).astype(np.float64).reshape(A, 3)
            self.ds[c] = ds
            self.pending[c] = (float(e[c]), -f[c].ravel(), disp, ds, zero, x1.astype(np.float64).reshape(A, 3))
        return dr

    def judge(self, e_new, f_new, update):
        f_new = np.asarray(f_new, dtype=np.float64)
        for c in range(self.kind.shape[0]):
            if self.pending[c] is None:
                continue
            e0, g0, disp, ds, zero, x1 = self.pending[c]
            if float(e_new[c]) > e0 + self.energy_floor:
                self.reason[c] = ENERGY_ROSE
                continue
            if update:
                act = self.active(c)
                new = bofill(self.H[c][np.ix_(act, act)], disp[act], (-f_new[c].ravel() - g0)[act])
                if new is not None:
                    self.H[c][np.ix_(act, act)] = new
            self.arc[c] += ds
            self.path_x[c].append(x1), self.path_e[c].append(float(e_new[c])), self.path_s[c].append(self.arc[c])
            self.n_points[c] += 1
            free = self.kind[c] == 1
            fm = np.sqrt((f_new[c][free] ** 2).sum(axis=-1)).max() if free.any() else 0.0
            if fm < self.fmax or zero:
                self.reason[c] = MINIMUM
            elif self.n_points[c] == self.max_points:
                self.reason[c] = PATH_FULL


# ---- the four-atom Lennard-Jones cluster in fp64 --------------------------------------------------------------------------

def lj4_saddle():
    """The D2h saddle of the LJ4 cluster in fp64 (Newton's iteration on the projected Hessian from the planar diamond) and its
    unit Cartesian mode of negative curvature."""
    from _saddle_ref import lj4_diamond, run_lj_reference

    _, x, e, f = run_lj_reference(lj4_diamond(0.0, 0), 1, 1e-13, 30)
    lam, V = np.linalg.eigh(lj_hessian(x))
    return x, e, V[:, 0].reshape(4, 3)


def run_lj_path(x0, direction, masses, step, max_points=400, fmax=1e-9, energy_floor=0.0, hessian_every=1):
    """One branch from the saddle x0 along ``direction`` on the fp64 Lennard-Jones surface, in fp64 coordinates, with the exact
    Hessian every ``hessian_every`` points (Bofill updates in between, as the follower makes them).  Returns the reference
    (path_x, path_e, path_s, reason, n_points of entry 0)."""
    ref = IrcReference(np.ones((1, 4), dtype=int), np.asarray(masses, dtype=np.float64)[None], False, step, fmax, energy_floor,
                       max_points, direction=np.asarray(direction)[None], coord_dtype=np.float64)
    x = x0.copy()
    e, f = lj_energy_forces(x)
    k = 0
    while ref.reason[0] == RUNNING:
        dr = ref.propose(x[None], np.array([e]), f[None], lj_hessian(x)[None] if k % hessian_every == 0 else None)[0]
        e1, f1 = lj_energy_forces(x + dr)
        ref.judge(np.array([e1]), f1[None], (k + 1) % hessian_every != 0)
        k += 1
        if ref.reason[0] != ENERGY_ROSE:
            x, e, f = x + dr, e1, f1
    return ref


# ---- the reference driven by the fp64 oracle (CPU rehearsals of the GPU cases) ---------------------------------------------

ATOMIC_MASS = {"H": 1.008, "C": 12.011, "N": 14.007, "O": 15.999, "F": 18.998, "S": 32.06, "Cl": 35.45}


def fixture_masses(g):
    """Masses [C, A] (amu) of a golden fixture whose species are element indices into g["symbols"]; padding gets 0."""
    table = np.array([ATOMIC_MASS[s] for s in g["symbols"]] + [0.0])
    return table[np.asarray(g["species"])]


def oracle_lockstep(g, hessian_every, n_calls, step, fmax=1e-4, energy_floor=1e-7):
    """The lock-step cases of tests/test_gpu_irc.py rehearsed on the CPU: the reference followed on the oracle's surface (fp32
    coordinates, as on the device; direction None, max_points = n_calls) for every molecule of fixture g.  Returns (committed
    points per molecule, reasons, the landing margins of all steps proposed)."""
    from _saddle_ref import OraclePES

    species = np.asarray(g["species"])
    masses = fixture_masses(g)
    periodic = g["cell"] is not None and bool(np.any(g["pbc"]))
    counts, reasons, margins = [], [], []
    for c in range(species.shape[0]):
        pes = OraclePES(g, c)
        kind = (species[c:c + 1] >= 0).astype(int)
        ref = IrcReference(kind, masses[c:c + 1], periodic, step, fmax, energy_floor, n_calls)
        x = np.asarray(g["coords"][c], dtype=np.float32).astype(np.float64)
        e, f = pes.energies_forces(x[None])
        for k in range(n_calls):
            if ref.reason[0] != RUNNING:
                break
            H = pes.hessian(x, richardson=False)[0][None] if k % hessian_every == 0 else None
            dr = ref.propose(x[None], e, f, H)
            margins.append(float(ref.margin[0]))
            x1 = (x.astype(np.float32) + dr[0].astype(np.float32)).astype(np.float64)
            e1, f1 = pes.energies_forces(x1[None])
            ref.judge(e1, f1, (k + 1) % hessian_every != 0)
            if ref.reason[0] != ENERGY_ROSE:
                x, e, f = x1, e1, f1
        counts.append(int(ref.n_points[0])), reasons.append(int(ref.reason[0]))
    return counts, reasons, margins
