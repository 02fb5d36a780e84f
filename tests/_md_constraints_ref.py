"""fp64 numpy restatement of the bond-length constraints of csrc/md.hip (include/anihip.h has the definition): cluster finding,
``project_v`` by a dense linear solve per cluster, ``move`` (SHAKE with the directions of the start of the move) by Newton's
method on the multipliers down to 1e-13, and the constrained drift and kick built on ``_md_ref.drift`` / ``_md_ref.kick``.
Clusters of one shape (the same local constraint list) are solved together as one batch of small dense systems."""
import numpy as np

import _md_ref as ref


def find_clusters(pairs):
    """pairs [C, K, 2] (padded with -1) -> a list of (molecule, atoms ascending, [(slot a, slot b, k)] in the order of
    ``pairs``), the connected components of each molecule's constraint graph ordered by molecule and smallest atom."""
    out = []
    for c, mol in enumerate(np.asarray(pairs)):
        parent = {}

        def find(i):
            while parent.setdefault(i, i) != i:
                parent[i] = parent[parent[i]]
                i = parent[i]
            return i

        valid = [(k, int(i), int(j)) for k, (i, j) in enumerate(mol) if i >= 0]
        for _, i, j in valid:
            parent[max(find(i), find(j))] = min(find(i), find(j))
        comps = {}
        for i in parent:
            comps.setdefault(find(i), []).append(i)
        for root in sorted(comps):
            atoms = sorted(comps[root])
            bonds = [(atoms.index(i), atoms.index(j), k) for k, i, j in valid if find(i) == root]
            out.append((c, atoms, bonds))
    return out


class Constraints:
    """pairs [C, K, 2], lengths [C, K] (Angstrom), active [C, A] bool, mass [C, A] (amu): w = ACC_UNIT / m of an active atom and
    0 of any other; ``groups`` batches the clusters of one shape: (molecule [G], atoms [G, n], a [nb], b [nb], d [G, nb])."""

    def __init__(self, pairs, lengths, active, mass):
        self.clusters = find_clusters(pairs)
        active = np.asarray(active, dtype=bool)
        self.w = np.where(active, ref.ACC_UNIT / np.asarray(mass, dtype=np.float64), 0.0)
        self.owned = np.zeros(active.shape, dtype=bool)
        self.per_molecule = (np.asarray(pairs)[..., 0] >= 0).sum(axis=1)
        shapes = {}
        for c, atoms, bonds in self.clusters:
            self.owned[c, atoms] = True
            key = (len(atoms), tuple((a, b) for a, b, _ in bonds))
            shapes.setdefault(key, []).append((c, atoms, [lengths[c][k] for _, _, k in bonds]))
        self.owned &= active
        self.groups = []
        for (n, ab), members in shapes.items():
            self.groups.append((np.array([m[0] for m in members]), np.array([m[1] for m in members]),
                                np.array([a for a, _ in ab]), np.array([b for _, b in ab]),
                                np.array([m[2] for m in members], dtype=np.float64)))


def _directions(r, w, a, b):
    """W J^T of a batch of clusters: G [g, n, 3, nb] with G[., a_k, :, k] = w_a r_k and G[., b_k, :, k] = -w_b r_k."""
    G = np.zeros(w.shape + (3, len(a)))
    for k in range(len(a)):
        G[:, a[k], :, k] += w[:, a[k], None] * r[:, k]
        G[:, b[k], :, k] -= w[:, b[k], None] * r[:, k]
    return G


def project_v(x, v, cons):
    """v' = v - W J^T mu with r . (v'_a - v'_b) = 0 for every constraint, r = x_a - x_b."""
    v = np.array(v, dtype=np.float64)
    for mol, atoms, a, b, _ in cons.groups:
        m = mol[:, None]
        xc, vc, w = x[m, atoms], v[m, atoms], cons.w[m, atoms]
        r = xc[:, a] - xc[:, b]
        G = _directions(r, w, a, b)
        M = np.einsum("gkc,gkcl->gkl", r, G[:, a] - G[:, b])
        rhs = (r * (vc[:, a] - vc[:, b])).sum(axis=-1)
        v[m, atoms] = vc - np.einsum("gnck,gk->gnc", G, np.linalg.solve(M, rhs[..., None])[..., 0])
    return v


def move(x, v, h, cons, tol=1e-13, max_newton=50):
    """x' = x + h v + W J(x)^T lambda with |x'_a - x'_b| = d (relative residual of d^2 below ``tol``) and v' = (x' - x) / h, for
    the atoms of clusters; every other atom keeps x and v."""
    x0, v = np.asarray(x, dtype=np.float64), np.array(v, dtype=np.float64)
    x1 = x0.copy()
    for mol, atoms, a, b, d in cons.groups:
        m = mol[:, None]
        xc, w = x0[m, atoms], cons.w[m, atoms]
        G = _directions(xc[:, a] - xc[:, b], w, a, b)
        free = xc + h * v[m, atoms]
        lam = np.zeros(d.shape)
        for _ in range(max_newton):
            xn = free + np.einsum("gnck,gk->gnc", G, lam)
            s = xn[:, a] - xn[:, b]
            g = (s * s).sum(axis=-1) - d * d
            if (np.abs(g) <= tol * d * d).all():
                break
            jac = 2.0 * np.einsum("gkc,gkcl->gkl", s, G[:, a] - G[:, b])
            lam = lam - np.linalg.solve(jac, g[..., None])[..., 0]
        else:
            raise RuntimeError("the reference SHAKE did not converge")
        x1[m, atoms] = xn
        v[m, atoms] = (xn - xc) / h
    return x1, v


def residuals(x, cons):
    """The largest | |x_a - x_b| / d - 1 | over all constraints."""
    worst = 0.0
    for mol, atoms, a, b, d in cons.groups:
        xc = np.asarray(x, dtype=np.float64)[mol[:, None], atoms]
        worst = max(worst, np.abs(np.linalg.norm(xc[:, a] - xc[:, b], axis=-1) / d - 1.0).max())
    return worst


def velocity_residuals(x, v, cons):
    """Per cluster group: |r_hat . (v_a - v_b)| [G, nb] and the largest |v| component of each cluster [G]."""
    out = []
    for mol, atoms, a, b, _ in cons.groups:
        xc, vc = np.asarray(x, dtype=np.float64)[mol[:, None], atoms], np.asarray(v, dtype=np.float64)[mol[:, None], atoms]
        r = xc[:, a] - xc[:, b]
        rv = (r * (vc[:, a] - vc[:, b])).sum(axis=-1) / np.linalg.norm(r, axis=-1)
        out.append((np.abs(rv), np.abs(vc).max(axis=(1, 2))))
    return out


def drift(x, v, f, active, mass, dt, cons, langevin=False, kT=None, friction=None, xi=None):
    """``_md_ref.drift`` for the atoms outside clusters; for those inside, B, then move(dt) (NVE) or move(dt/2), O, move(dt/2)."""
    act = np.asarray(active, dtype=bool)[..., None]
    x = np.asarray(x, dtype=np.float64)
    x_free, v_free = ref.drift(x, v, f, active, mass, dt, langevin, kT, friction, xi)
    w = cons.w[..., None]
    v1 = np.where(act, np.asarray(v, dtype=np.float64) + 0.5 * dt * np.asarray(f, dtype=np.float64) * w, 0.0)
    if langevin:
        c1 = np.exp(-np.asarray(friction, dtype=np.float64) * dt)[:, None, None]
        sigma = np.sqrt(np.asarray(kT, dtype=np.float64)[:, None, None] * (1.0 - c1 * c1) * w)
        xa, va = move(x, v1, 0.5 * dt, cons)
        xb, vb = move(xa, np.where(act, c1 * va + sigma * xi, 0.0), 0.5 * dt, cons)
    else:
        xb, vb = move(x, v1, dt, cons)
    own = cons.owned[..., None]
    return np.where(own, xb, x_free), np.where(own, vb, v_free)


def kick(x, v, f, active, mass, dt, cons):
    """B and project_v at x; returns the new v and the kinetic energies [C] (Hartree)."""
    v1, _ = ref.kick(v, f, active, mass, dt)
    v1 = project_v(np.asarray(x, dtype=np.float64), v1, cons)
    m = np.where(np.asarray(active, dtype=bool), np.asarray(mass, dtype=np.float64), 0.0)[..., None]
    return v1, 0.5 * (m * v1 ** 2).sum(axis=(1, 2)) / ref.ACC_UNIT
