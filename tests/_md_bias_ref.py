"""fp64 numpy restatement of the biased-MD definitions of include/anihip.h (anihip_md_bias_*): collective variables with
their analytic gradients, the flat-bottom harmonic restraint, the sum over Gaussian hills with its derivative, the deposit,
and the per-atom force sum in CV order with the final fp32 rounding.  The GPU tests compare the kernels with it; the host
tests check it against autograd and finite differences.  Loops are plain: it is read, not timed."""
import math

import numpy as np

DISTANCE, ANGLE, DIHEDRAL = 0, 1, 2
N_ATOMS = {DISTANCE: 2, ANGLE: 3, DIHEDRAL: 4}
MAX_CVS = 16
TWO_PI = 2.0 * math.pi
KB_HARTREE = 3.166811563e-6


def wrap(d):
    """d shifted by a multiple of 2 pi into [-pi, pi)."""
    return d - TWO_PI * np.floor((d + math.pi) / TWO_PI)


def cv(kind, x):
    """(s, grad [n, 3]) of one CV at the positions x [n, 3] (fp64) of its atoms i, j(, k(, l))."""
    x = np.asarray(x, dtype=np.float64)
    if kind == DISTANCE:
        d = x[0] - x[1]
        s = math.sqrt(d @ d)
        return s, np.stack([d / s, -d / s])
    if kind == ANGLE:
        a, b = x[0] - x[1], x[2] - x[1]
        n = np.cross(a, b)
        nn = math.sqrt(n @ n)
        s = math.atan2(nn, a @ b)
        ga = np.cross(a, n) / ((a @ a) * nn)
        gb = np.cross(n, b) / ((b @ b) * nn)
        return s, np.stack([ga, -(ga + gb), gb])
    b1, b2, b3 = x[1] - x[0], x[2] - x[1], x[3] - x[2]
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    L2 = b2 @ b2
    L = math.sqrt(L2)
    s = math.atan2(L * (b1 @ n2), n1 @ n2)
    # Blondel and Karplus 1996: no 1 / sin, finite wherever the two planes exist
    gi = -L / (n1 @ n1) * n1
    gl = L / (n2 @ n2) * n2
    p, q = (b1 @ b2) / L2, (b3 @ b2) / L2
    gj = q * gl - (1.0 + p) * gi
    gk = p * gi - (1.0 + q) * gl
    return s, np.stack([gi, gj, gk, gl])


def restraint(kind, s, center, k, half_width):
    """(E, dE/ds) of the flat-bottom harmonic restraint."""
    d = s - center
    if kind == DIHEDRAL:
        d = wrap(d)
    e = max(0.0, abs(d) - half_width)
    return 0.5 * k * e * e, math.copysign(k * e, d)


def hills_sum(s, centers, heights, inv_sigma2, periodic):
    """V, dV/ds [2] of the hills (centers [2, n], heights [n]) at the CV values s [n_dim], and the sums of the absolute terms
    (the scale of the comparison's tolerance): n_dim = len(s) dimensions, periodic[d] wraps the difference."""
    n = heights.shape[0]
    nd = len(s)
    diff = np.zeros((2, n))
    for d in range(nd):
        dd = s[d] - centers[d, :n]
        diff[d] = wrap(dd) if periodic[d] else dd
    arg = sum(diff[d] ** 2 * inv_sigma2[d] for d in range(nd)) if nd else np.zeros(n)
    g = heights * np.exp(-0.5 * arg)
    terms = np.stack([g] + [-g * diff[d] * (inv_sigma2[d] if d < nd else 0.0) for d in range(2)])
    return terms[0].sum(), terms[1:].sum(axis=1), np.abs(terms).sum(axis=1)


def ulp32(v):
    """One unit in the last place of the fp32 values v."""
    v = np.abs(np.asarray(v, dtype=np.float32))
    return (np.nextafter(v, np.float32(np.inf)) - v).astype(np.float64)


class Bias:
    """The tables of ``md.build_bias_tables`` as numpy arrays plus the hill lists: what the kernels hold on the device."""

    def __init__(self, tables, capacity=None):
        t = tables
        self.cv_offset, self.kind, self.atoms = t.cv_offset.numpy(), t.kind.numpy(), t.atoms.numpy()
        self.restraint = t.restraint.numpy()
        self.meta_cv, self.inv_sigma2, self.height = t.meta_cv.numpy(), t.inv_sigma2.numpy(), t.height.numpy()
        self.list, self.rank, self.members = t.list.numpy(), t.rank_in_list.numpy(), t.members.numpy()
        self.bias_factor = t.bias_factor.numpy()
        G = self.members.shape[0]
        self.capacity = int(t.capacity if capacity is None else capacity)
        self.centers = np.zeros((G, 2, self.capacity))
        self.heights = np.zeros((G, self.capacity))
        self.used = t.used.numpy().astype(np.int64).copy()
        self.dropped = np.zeros(G, dtype=np.int64)
        n0 = t.centers.shape[2]
        self.centers[:, :, :n0], self.heights[:, :n0] = t.centers.numpy(), t.heights.numpy()

    def entry_hills(self, c, values):
        """V, dV [2], abs sums [3] of entry c's list at its own CV values (values: the CSR array of all CV values)."""
        g = self.list[c]
        if g < 0:
            return 0.0, np.zeros(2), np.zeros(3)
        lo = self.cv_offset[c]
        idx = [int(i) for i in self.meta_cv[c] if i >= 0]
        s = [values[lo + i] for i in idx]
        per = [self.kind[lo + i] == DIHEDRAL for i in idx]
        n = self.used[g]
        return hills_sum(s, self.centers[g][:, :n], self.heights[g][:n], self.inv_sigma2[c], per)

    def apply(self, x, forces):
        """x fp64 [C, A, 3] (coordinates + coordinates_lo, exactly), forces fp32 [C, A, 3].  Returns a dict: cv_values [Ncv],
        bias_energies [C], meta_energies [C], energy_scale [C] (sum of the absolute energy terms), forces fp32 (the incoming
        ones plus the bias force, rounded once) and bias_forces fp64."""
        Cn, A = x.shape[:2]
        xf = x.reshape(-1, 3)
        ncv = self.kind.shape[0]
        values, grads = np.zeros(ncv), np.zeros((ncv, 4, 3))
        for r in range(ncv):
            n = N_ATOMS[int(self.kind[r])]
            values[r], grads[r, :n] = cv(int(self.kind[r]), xf[self.atoms[r, :n]])
        e_bias, e_meta, scale = np.zeros(Cn), np.zeros(Cn), np.zeros(Cn)
        fb = np.zeros((Cn * A, 3))
        for c in range(Cn):
            lo, hi = self.cv_offset[c], self.cv_offset[c + 1]
            V, dV, absV = self.entry_hills(c, values)
            e_sum = 0.0
            for r in range(lo, hi):   # CV order: every atom's force is summed in it
                kind = int(self.kind[r])
                E, dE = restraint(kind, values[r], *self.restraint[r])
                for d in range(2):
                    if self.meta_cv[c, d] == r - lo:
                        dE += dV[d]
                e_sum += E
                scale[c] += abs(E)
                for a in range(N_ATOMS[kind]):
                    fb[self.atoms[r, a]] += -dE * grads[r, a]
            e_bias[c], e_meta[c] = e_sum + V, V
            scale[c] += absV[0]
        fb = fb.reshape(Cn, A, 3)
        out = (forces.astype(np.float64) + fb).astype(np.float32)
        return {"cv_values": values, "bias_energies": e_bias, "meta_energies": e_meta, "energy_scale": scale, "forces": out,
                "bias_forces": fb}

    def deposit(self, kT, values, meta_energies):
        """One round: every member of a list appends a hill at its CV values, in batch order within the list; a list that
        would overflow deposits nothing and counts its members as dropped.  kT fp32 [C]."""
        Cn = self.list.shape[0]
        for g in range(self.members.shape[0]):
            if self.used[g] + self.members[g] > self.capacity:
                self.dropped[g] += self.members[g]
        for c in range(Cn):
            g = self.list[c]
            if g < 0 or self.used[g] + self.members[g] > self.capacity:
                continue
            h = self.used[g] + self.rank[c]
            lo = self.cv_offset[c]
            for d in range(2):
                self.centers[g, d, h] = values[lo + self.meta_cv[c, d]] if self.meta_cv[c, d] >= 0 else 0.0
            w = self.height[c]
            if self.bias_factor[g] > 0.0:
                w = w * math.exp(-meta_energies[c] / ((self.bias_factor[g] - 1.0) * float(np.float32(kT[c]))))
            self.heights[g, h] = w
        for g in range(self.members.shape[0]):
            if self.used[g] + self.members[g] <= self.capacity:
                self.used[g] += self.members[g]


ACC_UNIT = 4.3597447222071e-18 / 1e-10 / 1.66053906660e-27 * 1e10 * 1e-30


def dimer_free_energy(r, eps, sigma, kT):
    """U_LJ(r) - 2 kT ln r: the free energy along the distance of a dimer in three dimensions, up to a constant."""
    q = (sigma / r) ** 6
    return 4.0 * eps * (q * q - q) - 2.0 * kT * np.log(r)


def dimer_metadynamics(seed, n=128, steps=1000, eps=0.005, sigma=3.0, T=300.0, dt=2.0, friction=0.05, mass=12.011,
                       wall=(4.25, 1.75, 0.05), sigma_cv=0.1, height_kT=0.02, gamma=6.0, pace=10, r0=None):
    """Multiple-walker well-tempered metadynamics of n Lennard-Jones dimers on one shared hill list, on the CPU: BAOAB as
    csrc/md.hip splits it, the bias on the distance, the deposit of include/anihip.h (after the kick of every ``pace``-th step,
    at the CV values and with the bias of that step's evaluation, acting from the next evaluation on).  Returns the hills
    (centers, heights)."""
    rs = np.random.RandomState(seed)
    kT = KB_HARTREE * T
    r0 = 2.0 ** (1.0 / 6.0) * sigma if r0 is None else r0
    x = np.zeros((n, 2, 3))
    x[:, 1, 0] = r0
    v = rs.normal(size=(n, 2, 3)) * math.sqrt(kT * ACC_UNIT / mass)
    c1 = math.exp(-friction * dt)
    s_noise = math.sqrt(kT * (1.0 - c1 * c1) * ACC_UNIT / mass)
    centers, heights = np.zeros(0), np.zeros(0)
    is2 = 1.0 / sigma_cv ** 2

    def evaluate():
        d = x[:, 1] - x[:, 0]
        r = np.sqrt((d * d).sum(axis=1))
        q = (sigma / r) ** 6
        dU = 4.0 * eps * (-12.0 * q * q + 6.0 * q) / r
        dd = r - wall[0]
        e = np.maximum(0.0, np.abs(dd) - wall[1])
        dU = dU + np.copysign(wall[2] * e, dd)
        diff = r[:, None] - centers[None, :]
        g = heights[None, :] * np.exp(-0.5 * diff * diff * is2)
        V = g.sum(axis=1)
        dU = dU - (g * diff).sum(axis=1) * is2
        f1 = -dU[:, None] * d / r[:, None]
        return r, V, np.stack([-f1, f1], axis=1)

    r, V, f = evaluate()
    for step in range(1, steps + 1):
        v += 0.5 * dt * f * (ACC_UNIT / mass)
        x += 0.5 * dt * v
        v = c1 * v + s_noise * rs.normal(size=v.shape)
        x += 0.5 * dt * v
        r, V, f = evaluate()
        v += 0.5 * dt * f * (ACC_UNIT / mass)
        if pace and step % pace == 0:
            centers = np.concatenate([centers, r])
            heights = np.concatenate([heights, height_kT * kT * np.exp(-V / ((gamma - 1.0) * kT))])
    return centers, heights


def free_energy_error(centers, heights, grid, eps, sigma, kT, sigma_cv, gamma):
    """max |F_metadynamics - F_exact| / kT on the grid, both with their mean removed; F_metadynamics = -gamma / (gamma - 1) V."""
    diff = grid[:, None] - centers[None, :]
    V = (heights[None, :] * np.exp(-0.5 * diff * diff / sigma_cv ** 2)).sum(axis=1)
    F = -gamma / (gamma - 1.0) * V
    exact = dimer_free_energy(grid, eps, sigma, kT)
    return np.abs((F - F.mean()) - (exact - exact.mean())).max() / kT
