"""fp64 numpy reference of the semantics of torchani_amd.geomopt.SaddleOptimizer (include/anihip.h: anihip_saddle): P-RFO on a
model Hessian with Bofill updates, every molecule on its own.  Deliberately another formulation than the HIP kernels': it
works on the active coordinates only (the kernels keep all 3A and push the others to mu), the rigid motions are
orthonormalized by QR factorisations (the kernels: Gram-Schmidt), the projected Hessian is formed as P H P + mu Q Q^T with
dense products (the kernels: a rank-12 correction), and the two RFO partitions are extreme eigenpairs of the augmented matrices
(the kernels: a closed form and a bisection on the secular equation).  Agreement checks both."""
import numpy as np

RANK_TOL = 1e-8


def rigid_basis(x, free, translations, rotations):
    """Orthonormal basis [3 n_free, r] of the rigid motions of the free atoms x [n_free, 3] (about their centroid)."""
    m = x.shape[0]
    raw = []
    if translations:
        for j in range(3):
            v = np.zeros((m, 3))
            v[:, j] = 1.0
            raw.append(v.ravel())
    if rotations:
        r = x - x.mean(axis=0)
        for j in range(3):
            raw.append(np.cross(np.eye(3)[j], r).ravel())
    Q = np.zeros((3 * m, 0))
    for v in raw:
        norm = np.linalg.norm(v)
        if norm == 0.0:
            continue
        q, r = np.linalg.qr(np.column_stack([Q, v]))
        if abs(r[-1, -1]) > RANK_TOL * norm:   # independent of the ones kept
            Q = q
    return Q


def rfo_partitions(lam, gt, k):
    """The P-RFO step in the eigenbasis: the highest eigenpair of [[lam_k, g_k], [g_k, 0]] along k, the lowest eigenpair of
    the bordered matrix of the other modes with a gradient component; step = v[:-1] / v[-1]."""
    st = np.zeros_like(gt)
    if gt[k] != 0.0:
        w, v = np.linalg.eigh(np.array([[lam[k], gt[k]], [gt[k], 0.0]]))
        st[k] = v[0, 1] / v[1, 1]
    idx = np.array([i for i in range(lam.size) if i != k and gt[i] != 0.0], dtype=int)
    if idx.size:
        M = np.zeros((idx.size + 1, idx.size + 1))
        M[np.arange(idx.size), np.arange(idx.size)] = lam[idx]
        M[-1, :-1] = M[:-1, -1] = gt[idx]
        w, v = np.linalg.eigh(M)
        st[idx] = v[:-1, 0] / v[-1, 0]
    return st


def bofill(H, s, y):
    """The Bofill update of H for the step s and the gradient change y (None: skipped)."""
    xi = y - H @ s
    xs, xx, ss = xi @ s, xi @ xi, s @ s
    if xx == 0.0 or ss == 0.0:
        return None
    phi = 0.0 if xs == 0.0 else xs * xs / (xx * ss)
    out = H + (1.0 - phi) * ((np.outer(xi, s) + np.outer(s, xi)) / ss - xs * np.outer(s, s) / ss ** 2)
    if xs != 0.0:
        out = out + phi * np.outer(xi, xi) / xs
    return out


class SaddleReference:
    """The optimizer state of C molecules.  ``propose(x, e, f, H_exact)`` makes step 1 to 7 of the issue and returns the
    displacement [C, A, 3]; ``judge(e_new, f_new, bofill)`` makes steps 9 and 10.  kind [C, A]: 0 padding, 1 free, 2 fixed.
    coord_dtype=np.float32 rounds the displacement and the moved coordinates like the device does."""

    def __init__(self, kind, periodic, follow, trust, max_trust, min_trust, energy_floor, fmax, mode=None,
                 coord_dtype=np.float32):
        self.kind = np.asarray(kind)
        C, A = self.kind.shape
        self.periodic, self.follow = bool(periodic), follow
        self.max_trust, self.min_trust, self.energy_floor, self.fmax = max_trust, min_trust, energy_floor, fmax
        self.coord_dtype = coord_dtype
        self.trust = np.full(C, float(trust))
        self.H = np.zeros((C, 3 * A, 3 * A))
        self.modes = np.zeros((C, 3 * A)) if mode is None else np.asarray(mode, dtype=np.float64).reshape(C, 3 * A).copy()
        self.have_mode = mode is not None
        self.calls = 0
        self.converged = np.zeros(C, dtype=bool)
        self.accepted = np.zeros(C, dtype=bool)
        self.n_steps = np.zeros(C, dtype=np.int64)
        self.n_rejected = np.zeros(C, dtype=np.int64)
        self.eigenvalues = np.zeros(C)
        self.gap = np.full(C, np.inf)       # relative distance of the followed eigenvalue to its nearest neighbour
        self.pending = [None] * C

    def active(self, c):
        return np.repeat(self.kind[c] == 1, 3)

    def propose(self, x, e, f, H_exact=None):
        x = np.asarray(x, dtype=np.float64)
        f = np.asarray(f, dtype=np.float64)
        C, A = self.kind.shape
        dr = np.zeros((C, A, 3))
        use_overlap = self.have_mode and (self.calls == 0 or self.follow == "overlap")
        for c in range(C):
            self.pending[c] = None
            if self.converged[c]:
                continue
            free = self.kind[c] == 1
            if H_exact is not None:
                self.H[c] = 0.5 * (H_exact[c] + H_exact[c].T)
            fnorm = np.sqrt((f[c][free] ** 2).sum(axis=-1))
            if fnorm.size == 0 or fnorm.max() < self.fmax:
                self.converged[c] = True
                continue
            act = self.active(c)
            g = -f[c].ravel()[act]
            Ha = self.H[c][np.ix_(act, act)]
            no_fixed = not np.any(self.kind[c] == 2)
            Q = rigid_basis(x[c][free], free, no_fixed, no_fixed and not self.periodic)
            P = np.eye(g.size) - Q @ Q.T
            mu = 1.0 + np.abs(self.H[c]).sum(axis=1).max()
            lam, V = np.linalg.eigh(P @ Ha @ P + mu * (Q @ Q.T))
            gt = V.T @ (P @ g)
            k = 0
            if use_overlap:
                ov = np.abs(V.T @ self.modes[c][act])
                ov[lam >= 0.5 * mu] = -1.0
                k = int(np.argmax(ov))
            near = np.abs(np.delete(lam, k) - lam[k]).min() if lam.size > 1 else np.inf
            self.gap[c] = near / max(abs(lam[k]), 1e-300)
            st = rfo_partitions(lam, gt, k)
            norm = np.linalg.norm(st)
            if norm > self.trust[c]:
                st *= self.trust[c] / norm
                norm = self.trust[c]
            pred = float(gt @ st + 0.5 * (lam * st * st).sum())
            s = np.zeros(3 * A)
            s[act] = V @ st
            x0 = x[c].ravel().astype(self.coord_dtype)
            x1 = x0 + s.astype(self.coord_dtype)
            disp = x1.astype(np.float64) - x0.astype(np.float64)
            dr[c] = s.astype(self.coord_dtype).astype(np.float64).reshape(A, 3)
            self.eigenvalues[c] = lam[k]
            self.modes[c] = 0.0
            self.modes[c][act] = V[:, k]
            self.pending[c] = (float(e[c]), -f[c].ravel(), pred, norm, disp)
        self.have_mode = self.have_mode or self.follow == "overlap"
        self.calls += 1
        return dr

    def judge(self, e_new, f_new, update):
        f_new = np.asarray(f_new, dtype=np.float64)
        for c in range(self.kind.shape[0]):
            self.accepted[c] = False
            if self.pending[c] is None:
                continue
            e0, g0, pred, norm, disp = self.pending[c]
            radius = self.trust[c]
            ok = True
            if abs(pred) >= self.energy_floor and pred != 0.0:
                dev = abs((float(e_new[c]) - e0) / pred - 1.0)
                if dev > 1.0:
                    ok = False
                    radius = max(radius / 4, self.min_trust)
                elif dev < 0.25 and norm >= 0.99 * radius:
                    radius = min(2 * radius, self.max_trust)
                elif dev > 0.75:
                    radius = max(radius / 2, self.min_trust)
            self.trust[c] = radius
            if not ok:
                self.n_rejected[c] += 1
                continue
            self.accepted[c] = True
            self.n_steps[c] += 1
            if update:
                act = self.active(c)
                new = bofill(self.H[c][np.ix_(act, act)], disp[act], (-f_new[c].ravel() - g0)[act])
                if new is not None:
                    self.H[c][np.ix_(act, act)] = new


# ---- the four-atom Lennard-Jones cluster in fp64 (eps = sigma = 1) -------------------------------------------------------

LJ4_SADDLE = -5.0734208585   # the planar D2h rhombus (the literature's -5.07342)


def lj_energy_forces(x):
    d = x[:, None, :] - x[None, :, :]
    r2 = (d ** 2).sum(-1)
    np.fill_diagonal(r2, 1.0)
    i6 = r2 ** -3
    e = 4.0 * (i6 * i6 - i6)
    np.fill_diagonal(e, 0.0)
    w = 24.0 * (2.0 * i6 * i6 - i6) / r2      # -dE/dr / r
    np.fill_diagonal(w, 0.0)
    return 0.5 * e.sum(), (w[:, :, None] * d).sum(axis=1)


def lj_hessian(x):
    n = x.shape[0]
    H = np.zeros((n, 3, n, 3))
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            d = x[i] - x[j]
            r2 = d @ d
            i6 = r2 ** -3
            a = -24.0 * (2.0 * i6 * i6 - i6) / r2                    # E' / r
            b = (4.0 * (156.0 * i6 * i6 - 42.0 * i6) / r2 - a) / r2   # (E'' - E' / r) / r^2
            blk = a * np.eye(3) + b * np.outer(d, d)
            H[i, :, i, :] += blk
            H[i, :, j, :] -= blk
    return H.reshape(3 * n, 3 * n)


def lj4_diamond(noise, seed):
    """Two equilateral triangles of side 1.12 sharing an edge, in the plane, plus Gaussian noise."""
    a = 1.12
    h = a * np.sqrt(3.0) / 2
    x = np.array([[0.0, a / 2, 0.0], [0.0, -a / 2, 0.0], [h, 0.0, 0.0], [-h, 0.0, 0.0]])
    return x + noise * np.random.RandomState(seed).randn(4, 3)


def run_lj_reference(x0, hessian_every, fmax, steps, trust=0.05, max_trust=0.15, min_trust=1e-4, energy_floor=1e-7):
    """The reference driven by the fp64 Lennard-Jones functions above, in fp64 coordinates, for one cluster.  Returns the
    reference and the final (x, e, f)."""
    ref = SaddleReference(np.ones((1, x0.shape[0]), dtype=int), False, "lowest", trust, max_trust, min_trust, energy_floor, fmax,
                          coord_dtype=np.float64)
    x = x0.copy()
    e, f = lj_energy_forces(x)
    for k in range(steps):
        H = lj_hessian(x)[None] if k % hessian_every == 0 else None
        dr = ref.propose(x[None], np.array([e]), f[None], H)[0]
        if ref.converged[0]:
            break
        e1, f1 = lj_energy_forces(x + dr)
        ref.judge(np.array([e1]), f1[None], (k + 1) % hessian_every != 0)
        if ref.accepted[0]:
            x, e, f = x + dr, e1, f1
    return ref, x, e, f


# ---- the reference driven by the fp64 oracle (CPU rehearsals of the GPU cases) ---------------------------------------------

class OraclePES:
    """Energies, forces and central-difference Hessians of the seeded ANI model of a golden fixture from the fp64 oracle,
    one molecule (species [A], padding -1) at a time."""

    def __init__(self, g, c=0):
        from _util import oracle_networks, oracle_params
        from oracle.oracle import Oracle

        self.orc = Oracle("f64")
        self.dims, self.flat, self.sae = oracle_networks(g["kind"], g["n_members"], g["seed"])
        self.p = oracle_params(g["kind"], g["cutoff_fn"])
        self.n_members = g["n_members"]
        self.species = np.asarray(g["species"][c], dtype=np.int64)
        self.cell = None if g["cell"] is None else np.asarray(g["cell"], dtype=np.float64)
        self.pbc = g["pbc"]

    def energies_forces(self, x):
        """x [K, A, 3] -> energies [K], forces [K, A, 3]."""
        x = np.asarray(x, dtype=np.float64)
        sp = np.repeat(self.species[None], x.shape[0], axis=0)
        out = self.orc.energy_forces(self.p, sp, x, self.dims, self.flat, self.n_members, sae=self.sae, cell=self.cell,
                                     pbc=self.pbc)
        return out["energies"], out["forces"]

    def hessian(self, x, h=1e-4, richardson=True):
        """(H [3A, 3A], spread): Richardson-extrapolated central differences of the forces at steps h and 2h, symmetrized,
        and the largest |D(h) - D(2h)|, the noise floor of an element (as tests/_second_order_ref.py measures it).
        richardson=False: the differences at h alone (half the evaluations), spread None."""
        x = np.asarray(x, dtype=np.float64)
        n = x.size
        e = np.eye(n).reshape(n, *x.shape)
        d = []
        for s in (h, 2 * h) if richardson else (h,):
            fp = self.energies_forces(x[None] + s * e)[1].reshape(n, n)
            fm = self.energies_forces(x[None] - s * e)[1].reshape(n, n)
            d.append(-(fp - fm) / (2 * s))
        if not richardson:
            return 0.5 * (d[0] + d[0].T), None
        H = (4.0 * d[0] - d[1]) / 3.0
        return 0.5 * (H + H.T), float(np.abs(d[0] - d[1]).max())


def oracle_lockstep(g, hessian_every, n_steps, fmax=1e-4, trust=0.05, max_trust=0.15, min_trust=1e-4, energy_floor=1e-7):
    """The lock-step cases of tests/test_gpu_saddle.py rehearsed on the CPU: the reference stepped on the oracle's surface
    (fp32 coordinates, as on the device) for every molecule of fixture g.  Returns (pairs, degenerate): the (molecule, step)
    pairs that moved and those among them whose followed eigenvalue lies within 1e-6 relative of its neighbour."""
    species = np.asarray(g["species"])
    periodic = g["cell"] is not None and bool(np.any(g["pbc"]))
    pairs = degenerate = 0
    for c in range(species.shape[0]):
        pes = OraclePES(g, c)
        kind = (species[c:c + 1] >= 0).astype(int)
        ref = SaddleReference(kind, periodic, "lowest", trust, max_trust, min_trust, energy_floor, fmax)
        x = np.asarray(g["coords"][c], dtype=np.float32).astype(np.float64)
        e, f = pes.energies_forces(x[None])
        for k in range(n_steps):
            H = pes.hessian(x, richardson=False)[0][None] if k % hessian_every == 0 else None
            dr = ref.propose(x[None], e, f, H)
            if ref.pending[0] is None:
                break
            pairs += 1
            degenerate += ref.gap[0] <= 1e-6
            x1 = (x.astype(np.float32) + dr[0].astype(np.float32)).astype(np.float64)
            e1, f1 = pes.energies_forces(x1[None])
            ref.judge(e1, f1, (k + 1) % hessian_every != 0)
            if ref.accepted[0]:
                x, e, f = x1, e1, f1
    return pairs, int(degenerate)


def relax_on_oracle(g, c, steps=400):
    """Molecule c of fixture g (its real atoms) relaxed by the L-BFGS reference on the oracle's surface to the default fmax,
    in fp32 coordinates.  Returns (atomic symbols, start x, relaxed x, converged)."""
    from _geomopt_ref import LbfgsReference

    A = int((np.asarray(g["species"][c]) >= 0).sum())
    one = dict(g, species=np.asarray(g["species"])[c:c + 1, :A], coords=np.asarray(g["coords"])[c:c + 1, :A])
    pes = OraclePES(one, 0)
    x0 = one["coords"][0].astype(np.float64)
    x = x0.copy()
    lb = LbfgsReference(1, 100, 0.2, 70.0 / 27.211386024367243, 1.0, 0.05 / 27.211386024367243)
    for _ in range(steps):
        dr = lb.step(x[None], pes.energies_forces(x[None])[1], np.ones((1, A), dtype=bool))
        if lb.converged[0]:
            break
        x = (x.astype(np.float32) + dr[0].astype(np.float32)).astype(np.float64)
    return [g["symbols"][s] for s in one["species"][0]], x0, x, bool(lb.converged[0])


def rotatable_bonds(symbols, x):
    """Bonds j-k between heavy atoms that each carry another neighbour and are in no ring (geomopt.fragment_mask's bonds)."""
    import torch

    from torchani_amd.geomopt import fragment_mask

    number = {"H": 1, "C": 6, "N": 7, "O": 8, "F": 9, "S": 16, "Cl": 17}
    z = torch.tensor([number[s] for s in symbols])
    xt = torch.from_numpy(np.asarray(x, dtype=np.float64))
    out = []
    for j in range(len(symbols)):
        for k in range(j + 1, len(symbols)):
            if z[j] == 1 or z[k] == 1:
                continue
            try:
                side_k, side_j = fragment_mask(z, xt, j, k), fragment_mask(z, xt, k, j)
            except ValueError:
                continue
            # (a bond: k's side does not hold j only if the two are bonded; both sides need a further atom)
            d = float((xt[j] - xt[k]).norm())
            if d < 2.0 and int(side_k.sum()) > 1 and int(side_j.sum()) > 1 and int(side_k.sum()) + int(side_j.sum()) == len(symbols):
                out.append((j, k))
    return out
