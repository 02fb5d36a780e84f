"""Synthetic problems for the entry-point tests of anihip_lbfgs_step (tests/test_gpu_lbfgs_entry.py) and the host proof that they
reach what they are meant to reach (tests/test_lbfgs_cases_host.py).  No model: per molecule

    E(x) = d^T K d / 2 + sum_i q_i d_i^4 / 4 - b (u.d)^2 / 2 + c (u.d)^4 / 4,     d = x - x0 on the active coordinates, 0 elsewhere

with K = Q diag(lambda) Q^T, Q a seeded random orthogonal matrix, lambda log-spaced in [lo, hi] Ha / A^2, and the last two terms
(a ridge along the seeded unit vector u) only for molecules that must start where s.y <= 0.  Forces are evaluated in fp64 numpy
from the fp32 coordinates and cast to fp32; on inactive atoms (padding, fixed) the array holds garbage -- 1e6, or (NaN, 1e6, NaN) in
the cases that say so -- never zeros: the optimizer must take such a force as zero.

The cases are chosen for the quantities of lb_layout (csrc/lbfgs.hip), restated in layout() below; the `expect` column of CASES
is asserted against layout() by the host test, not trusted."""
import os
import typing as tp

import numpy as np

REPORT = os.environ.get("TORCHANI_AMD_GEOMOPT_REPORT")


def report(line):
    print(line)
    if not REPORT:
        return
    try:
        os.makedirs(os.path.dirname(REPORT) or ".", exist_ok=True)
        with open(REPORT, "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


LB_SLOTS = 4   # csrc/lbfgs.hip


class Layout(tp.NamedTuple):
    n: int
    n_pad: int
    V: int
    G: int
    R: int
    NV: int
    Gc: int
    M1: int
    offsets: tp.Dict[str, int]   # byte offset of every region of the workspace
    sizes: tp.Dict[str, int]     # bytes of one molecule's part of the region
    total: int


def layout(C, A, memory):
    """lb_layout of csrc/lbfgs.hip."""
    n = 3 * A
    n_pad = -(-n // 64) * 64
    V = 1
    while V < 16 and V < n_pad // 64:
        V *= 2
    G = -(-n_pad // (64 * V))
    M1 = memory + 1
    R = -(-M1 // LB_SLOTS)
    NV = 4 * M1 + 1
    Gc = -(-A // 64)
    per_mol = [("state", 4 * 4), ("coef", 2 * M1 * 8), ("rinv", M1 * M1 * 8), ("rinvt", M1 * M1 * 8), ("yy", M1 * M1 * 8),
               ("dd", M1 * 8), ("part", G * NV * 8), ("pmax", Gc * 8), ("p", n * 8), ("xprev", n_pad * 4), ("fprev", n_pad * 4),
               ("s", M1 * n_pad * 4), ("y", M1 * n_pad * 4)]
    offsets, o = {}, 0
    for name, b in per_mol:
        offsets[name] = o
        o += -(-C * b // 256) * 256
    return Layout(n, n_pad, V, G, R, NV, Gc, M1, offsets, dict(per_mol), o)


class Molecule:
    """One molecule's potential.  `quartic` is a scalar or one coefficient per coordinate; `soft` lists atoms taken out of K
    (their three coordinates get the curvature `soft_k` on the diagonal and couple to nothing); `ridge` = (b, c) adds the
    concave term along a seeded unit vector u of the active coordinates."""

    def __init__(self, rs, active, lo, hi, quartic, ridge=None, soft=(), soft_k=0.0):
        self.active = np.asarray(active, dtype=bool)
        A = self.active.size
        n = 3 * A
        self.mask = np.repeat(self.active, 3)
        self.x0 = rs.uniform(-2.0, 2.0, n).astype(np.float32).astype(np.float64)
        hard = np.ones(n, dtype=bool)
        for i in soft:
            hard[3 * i:3 * i + 3] = False
        m = int(hard.sum())
        Q, _ = np.linalg.qr(rs.standard_normal((m, m)))
        lam = np.logspace(np.log10(lo), np.log10(hi), m) if m > 1 else np.array([hi])
        self.K = np.zeros((n, n))
        self.K[np.ix_(hard, hard)] = (Q * lam) @ Q.T
        self.K[~hard, ~hard] = soft_k
        self.q = np.broadcast_to(np.asarray(quartic, dtype=np.float64), (n,)).copy()
        self.ridge = ridge
        u = rs.standard_normal(n) * self.mask
        self.u = u / np.linalg.norm(u) if self.mask.any() else u

    def forces(self, x):
        """fp64 [n] forces at the coordinates x [n]; 0 on inactive coordinates."""
        d = (np.asarray(x, dtype=np.float64) - self.x0) * self.mask
        f = -(self.K @ d) - self.q * d ** 3
        if self.ridge is not None:
            b, c = self.ridge
            t = self.u @ d
            f += (b * t - c * t ** 3) * self.u
        return f * self.mask

    def start(self, rs, amplitude, along_ridge=None, off_ridge=None):
        """fp32 [n] start: x0 + amplitude * uniform(-1, 1) on the active coordinates; with `off_ridge` its component along u is
        set to that; with `along_ridge` the start is x0 + along_ridge * u, on the ridge itself."""
        if along_ridge is not None:
            return (self.x0 + along_ridge * self.u).astype(np.float32)
        d = amplitude * rs.uniform(-1.0, 1.0, self.x0.size) * self.mask
        if off_ridge is not None:
            d += (off_ridge - self.u @ d) * self.u
        return (self.x0 + d).astype(np.float32)


class Problem:
    """The molecules of a case, their start coordinates and how garbage is put on the inactive atoms."""

    def __init__(self, case, molecules, x_start, nan_garbage, roles=None):
        self.case, self.molecules = case, molecules
        self.active = np.stack([m.active for m in molecules])                      # bool [C, A]
        self.x_start = np.stack(x_start).reshape(case.C, case.A, 3).astype(np.float32)
        self.nan_garbage = nan_garbage
        self.roles = roles

    def forces(self, x, only=None):
        """fp32 forces [C, A, 3] at the fp32 coordinates x [C, A, 3] (of molecule `only` alone: [1, A, 3] both)."""
        which = range(len(self.molecules)) if only is None else [only]
        out = np.empty((len(which), self.case.A, 3), dtype=np.float32)
        for k, c in enumerate(which):
            m = self.molecules[c]
            f = m.forces(np.asarray(x[k], dtype=np.float64).ravel()).astype(np.float32).reshape(-1, 3)
            f[~m.active] = (np.nan, 1e6, np.nan) if self.nan_garbage else 1e6
            out[k] = f
        return out

    def reference(self):
        """The fp64 two-loop reference with the kernel's fp32 pair storage."""
        from _geomopt_ref import LbfgsReference

        k = self.case
        return LbfgsReference(k.C, k.memory, k.maxstep, k.alpha, k.damping, k.fmax, pair_dtype=np.float32)


class Case(tp.NamedTuple):
    name: str
    C: int
    A: int
    memory: int
    steps: int
    fmax: float
    alpha: float      # Ha / A^2: H0 = 1 / alpha
    maxstep: float    # A
    damping: float
    expect: tp.Dict[str, int]   # V, G, Gc, R, n_pad the case is meant to have
    build: tp.Callable[["Case"], Problem]


def _plain(seed, lo, hi, quartic, amplitude, late_ridge=None):
    """Whole molecules on the convex potential.  `late_ridge` = (b, c, t0) puts a ridge under the last one and starts it t0 off
    the ridge: it stores pairs while its convex coordinates relax and t grows, and once the ring is full the fall off the ridge
    takes over the step: pairs with s.y < 0, s and y far from zero, rejected with the ring full.  Its large start amplitude keeps the
    first steps scaled to maxstep, so t grows slowly and the ring has wrapped by then: the spare slot that takes the rejected pair
    still has the row of R^-1 and Y^T Y of the pair it held before."""
    def build(case):
        rs = np.random.RandomState(seed)
        ridges = [None] * (case.C - 1) + [late_ridge and late_ridge[:2]]
        mols = [Molecule(rs, np.ones(case.A, dtype=bool), lo, hi, quartic, ridge=r) for r in ridges]
        amps = amplitude if isinstance(amplitude, (list, tuple)) else [amplitude] * case.C
        offs = [None] * (case.C - 1) + [late_ridge and late_ridge[2]]
        return Problem(case, mols, [m.start(rs, a, off_ridge=t) for m, a, t in zip(mols, amps, offs)], nan_garbage=False)
    return build


def _two_waves(case):
    """A = 65: atom 64 alone in the second wave of k_lb_direction / k_lb_update.  Molecule 0 whole; molecule 1 a padding tail
    (atoms 50 .. 64) and fixed atoms in the middle of the first wave; molecule 2 fixed atoms at 31, 32 and 63, atom 64 free."""
    rs = np.random.RandomState(65)
    act = np.ones((3, case.A), dtype=bool)
    act[1, 50:] = False
    act[1, [7, 21, 22, 40]] = False
    act[2, [31, 32, 63]] = False
    mols = [Molecule(rs, a, 0.5, 4.0, 2.0) for a in act]
    return Problem(case, mols, [m.start(rs, a) for m, a in zip(mols, (0.4, 0.05, 0.15))], nan_garbage=True)


SPLIT_ATOM = 341   # coordinate 1023 in chunk 0 of k_lb_dots<16>, 1024 and 1025 in chunk 1


def _split_atom(case):
    """A = 343, n = 1029.  Atom 341 couples to nothing and is all quartic, so its force falls slowly (a secant method converges
    linearly on d^4) while the rest converges fast: in molecule 0 it is the largest force when convergence is decided.  In
    molecule 1 the atom is fixed, in molecule 2 it is an atom like the others."""
    rs = np.random.RandomState(343)
    act = np.ones((3, case.A), dtype=bool)
    act[1, SPLIT_ATOM] = False
    q0 = np.full(3 * case.A, 2.0)
    q0[3 * SPLIT_ATOM:3 * SPLIT_ATOM + 3] = 400.0
    mols = [Molecule(rs, act[0], 1.0, 4.0, q0, soft=(SPLIT_ATOM,), soft_k=1e-3),
            Molecule(rs, act[1], 1.0, 4.0, 2.0),
            Molecule(rs, act[2], 1.0, 4.0, 2.0)]
    return Problem(case, mols, [m.start(rs, 0.2) for m in mols], nan_garbage=True)


def _concave(case):
    """Molecule 0 starts on the ridge itself (d along u): its first pairs are rejected with an empty history.  Molecule 1 starts
    off the ridge everywhere else and only just off it along u: pairs are stored while the convex coordinates relax, then the
    fall off the ridge dominates the step and pairs are rejected with a history.  Molecule 2: no ridge."""
    rs = np.random.RandomState(22)
    act = np.ones(case.A, dtype=bool)
    mols = [Molecule(rs, act, 0.5, 4.0, 2.0, ridge=(12.0, 40.0)), Molecule(rs, act, 0.5, 4.0, 2.0, ridge=(12.0, 40.0)),
            Molecule(rs, act, 0.5, 4.0, 2.0)]
    x1 = mols[1].start(rs, 0.3, off_ridge=1e-3)
    return Problem(case, mols, [mols[0].start(rs, 0.0, along_ridge=0.02), x1, mols[2].start(rs, 0.3)], nan_garbage=False)


ROLES = ("inactive", "minimum", "concave", "running")


def many_role(c):
    """Which state molecule c of `many_molecules` starts in."""
    return "inactive" if c % 5 == 0 else "minimum" if c % 4 == 0 else "concave" if c % 7 == 0 else "running"


def _many(case):
    rs = np.random.RandomState(257)
    mols, xs, roles = [], [], []
    for c in range(case.C):
        role = many_role(c)
        act = np.zeros(case.A, dtype=bool) if role == "inactive" else np.ones(case.A, dtype=bool)
        if role == "running" and c % 3 == 0:
            act[c % case.A] = False   # a fixed atom among the running ones
        m = Molecule(rs, act, 0.5, 4.0, 2.0, ridge=(12.0, 40.0) if role == "concave" else None)
        if role == "minimum":
            x = m.x0.astype(np.float32)
        elif role == "concave":
            x = m.start(rs, 0.0, along_ridge=0.02)
        else:
            x = m.start(rs, 0.05 + 0.25 * rs.uniform())
        mols.append(m), xs.append(x), roles.append(role)
    return Problem(case, mols, xs, nan_garbage=False, roles=roles)


def _e(V, G, Gc, R, n_pad):
    return dict(V=V, G=G, Gc=Gc, R=R, n_pad=n_pad)


# name, C, A, memory, steps, fmax, alpha, maxstep, damping, expected layout, problem (_plain: seed, lo, hi, q, start amplitudes).
# alpha is the stiffest curvature (the plain H0 = 1 / alpha step is stable), maxstep below the first steps and above the later ones.
# Where fmax is 0 the run goes on until the molecule no longer moves in fp32: from then on s = y = 0 exactly, every pair is rejected
# (s.y = 0) and the step repeats.  Those rejections say nothing about the spare slot, which then holds zeros; the rejections of real
# pairs with the ring full come from the late ridge under the last molecule of v1_full_group, v2_lone_slot and v4_three_groups.
CASES = [
    Case("one_atom", 3, 1, 1, 40, 0.0, 4.0, 0.05, 1.0, _e(1, 1, 1, 1, 64), _plain(1, 0.5, 4.0, 2.0, [0.3, 0.02, 0.1])),
    Case("v1_full_group", 2, 21, 3, 200, 0.0, 4.0, 0.05, 1.0, _e(1, 1, 1, 1, 64), _plain(21, 0.5, 4.0, 2.0, [0.3, 1.2], late_ridge=(6.0, 0.5, 1e-3))),
    Case("v2_lone_slot", 2, 22, 4, 200, 0.0, 4.0, 0.05, 1.0, _e(2, 1, 1, 2, 128), _plain(220, 0.5, 4.0, 2.0, [0.3, 1.2], late_ridge=(6.0, 0.5, 1e-3))),
    Case("v4_three_groups", 3, 43, 8, 250, 0.0, 4.0, 0.05, 1.0, _e(4, 1, 1, 3, 192), _plain(43, 0.5, 4.0, 2.0, [0.3, 0.1, 1.2], late_ridge=(6.0, 0.5, 1e-3))),
    Case("v4_two_waves", 3, 65, 8, 60, 1e-3, 4.0, 0.05, 1.0, _e(4, 1, 2, 3, 256), _two_waves),
    Case("v8", 2, 86, 16, 100, 0.0, 4.0, 0.05, 1.0, _e(8, 1, 2, 5, 320), _plain(86, 0.5, 4.0, 2.0, [0.3, 0.1])),
    Case("full_memory", 1, 171, 256, 330, 0.0, 400.0, 0.2, 1.0, _e(16, 1, 3, 65, 576), _plain(171, 0.02, 400.0, 50.0, 0.5)),
    Case("split_atom", 3, 343, 16, 120, 1e-4, 4.0, 0.05, 1.0, _e(16, 2, 6, 5, 1088), _split_atom),
    Case("concave_start", 3, 22, 4, 60, 0.0, 4.0, 0.05, 1.0, _e(2, 1, 1, 2, 128), _concave),
    Case("many_molecules", 257, 5, 2, 30, 1e-3, 4.0, 0.05, 1.0, _e(1, 1, 1, 1, 64), _many),
]
BY_NAME = {k.name: k for k in CASES}
# the molecules stepped alone (C = 1) and at their place in the batch: of `many_molecules` one that runs (converged at step 15), one
# that rejects pairs (a ridge start, the last of the batch to converge) and the first to converge (with a fixed atom)
SOLO = {"many_molecules": (1, 126, 159), "split_atom": (0, 1, 2)}

_PROBLEMS = {}


def problem(name):
    """The problem of a case, built once (K of `split_atom` is 3 x 1029^2 doubles)."""
    if name not in _PROBLEMS:
        _PROBLEMS[name] = BY_NAME[name].build(BY_NAME[name])
    return _PROBLEMS[name]


class Compact:
    """The algebra of csrc/lbfgs.hip for one molecule, restated in numpy: the compact representation of Byrd, Nocedal and Schnabel,
    R^-1 kept by column append, its trailing block kept when the oldest pair is dropped, pairs in fp32, the rest fp64."""

    def __init__(self, n, memory, alpha):
        self.memory, self.gamma = memory, 1.0 / alpha
        self.S, self.Y = np.zeros((n, 0)), np.zeros((n, 0))
        self.Rinv, self.YY, self.D = np.zeros((0, 0)), np.zeros((0, 0)), np.zeros(0)
        self.x_prev = self.f_prev = None

    def direction(self, x, f):
        """p = -H g at the coordinates x with forces f (inactive coordinates already zeroed): offers the pair, returns p."""
        if self.x_prev is not None:
            s = (x - self.x_prev).astype(np.float32).astype(np.float64)
            y = (self.f_prev - f).astype(np.float32).astype(np.float64)
            d = s @ y
            if d > 0:
                r, yy = self.S.T @ y, self.Y.T @ y
                if self.D.size == self.memory:
                    self.S, self.Y, self.Rinv, self.YY, self.D = self.S[:, 1:], self.Y[:, 1:], self.Rinv[1:, 1:], self.YY[1:, 1:], self.D[1:]
                    r, yy = r[1:], yy[1:]
                m = self.D.size
                Rinv = np.zeros((m + 1, m + 1))
                Rinv[:m, :m], Rinv[:m, m], Rinv[m, m] = self.Rinv, -(self.Rinv @ r) / d, 1.0 / d
                YY = np.zeros((m + 1, m + 1))
                YY[:m, :m], YY[:m, m], YY[m, :m], YY[m, m] = self.YY, yy, yy, y @ y
                self.Rinv, self.YY, self.D = Rinv, YY, np.append(self.D, d)
                self.S, self.Y = np.column_stack([self.S, s]), np.column_stack([self.Y, y])
        self.x_prev, self.f_prev = x.copy(), f.copy()
        g = -f
        a = self.Rinv @ (self.S.T @ g)
        w = self.D * a + self.gamma * (self.YY @ a) - self.gamma * (self.Y.T @ g)
        t = self.Rinv.T @ w
        return -(self.gamma * g + self.S @ t - self.gamma * (self.Y @ a))


def run_reference(prob, watch=None):
    """The case on the reference's own trajectory: every reference step applied to the coordinates in fp32, x <- x + fp32(dr) as
    k_lb_update does.  `watch(k, x, f, dr, ref)` is called after every step with the coordinates and forces it was given.
    Returns the reference."""
    ref = prob.reference()
    x = prob.x_start.copy()
    for k in range(prob.case.steps):
        f = prob.forces(x)
        dr = ref.step(x, f, prob.active)
        if watch is not None:
            watch(k, x, f, dr, ref)
        x = x + dr.astype(np.float32)
    return ref
