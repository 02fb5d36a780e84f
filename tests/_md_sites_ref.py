"""fp64 numpy restatement of the group CVs of include/anihip.h (anihip_md_sites_*): the centre of a group, the switching
function of the coordination number with its derivative, the minimum image, the two-float split of a site's position, the
2^-64 floor of the value site, and the spread of the site forces back to the atoms with the fp32 site force and the final fp32
rounding.  Everything after the gather is tests/_md_bias_ref.py on the extended arrays.  Loops are plain: it is read, not
timed (a pair sum is one numpy row per atom, one atom against a group)."""
import math

import numpy as np

import _md_bias_ref as br

NONE, CENTER, ANCHOR, VALUE = 0, 1, 2, 3
ROLE_CENTER, ROLE_A, ROLE_B = 0, 1, 2
FLOOR = 2.0 ** -64
MAX_SITES = 64


def split(x):
    """(hi, lo) fp32 with hi = (float)x, lo = (float)(x - hi)."""
    hi = np.float32(x)
    return hi, np.float32(np.float64(x) - np.float64(hi))


def base(r, r0, d0, n):
    """1 / (1 + x^n), x = max(r - d0, 0) / r0, x^n by repeated multiplication."""
    x = max(r - d0, 0.0) / r0
    p = x
    for _ in range(2, n):
        p = p * x
    return 1.0 / (1.0 + p * x)


def switch(r, r0, d0, r_max, n):
    """(sw, dsw/dr) at r, a number or an array; r_max = inf: no cut."""
    r = np.asarray(r, dtype=np.float64)
    b = 0.0 if math.isinf(r_max) else base(r_max, r0, d0, n)
    x = np.maximum(r - d0, 0.0) / r0
    p = x   # x^(n - 1)
    for _ in range(2, n):
        p = p * x
    q = 1.0 + p * x
    inside = r < r_max
    sw = np.where(inside, (1.0 / q - b) / (1.0 - b), 0.0)
    dsw = np.where(inside & (r > d0), -n * p / (r0 * (q * q)) / (1.0 - b), 0.0)
    return sw, dsw


def mic(d, cell, pbc):
    """d [..., 3] - rint(d cell^-1) cell along the periodic directions; rows of cell are the lattice vectors."""
    if cell is None or not any(pbc):
        return d
    n = np.rint(d @ np.linalg.inv(cell)) * np.asarray(pbc, dtype=np.float64)
    return d - n @ cell


def center(x, atoms, w):
    """(sum_i w_i x_i in ascending atom order, the sum of the absolute terms) of the rows ``atoms`` of x [N, 3]."""
    s, scale = np.zeros(3), np.zeros(3)
    for i, wi in zip(atoms, w):
        s = s + wi * x[i]
        scale = scale + np.abs(wi * x[i])
    return s, scale


def pair_terms(x, i, others, p, cell, pbc):
    """Atom i against the atoms ``others`` (i itself skipped): sum of sw, sum of dsw/dr (x_i - x_j)_mic / r [3] with the terms
    of dsw/dr = 0 left out, and the sums of their absolute values.  One numpy row per call."""
    others = np.asarray(others)
    others = others[others != i]
    d = mic(x[i] - x[others], cell, pbc)
    r = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    sw, dsw = switch(r, *p)
    on = dsw != 0.0
    t = dsw[on, None] * (d[on] / r[on, None])
    return sw.sum(), np.abs(sw).sum(), t.sum(axis=0), np.abs(t).sum(axis=0)


def coordination(x, group_a, group_b, p, cell=None, pbc=(0, 0, 0)):
    """(s, sum of |terms|, ds/dx [N, 3]) of the coordination number of two groups of rows of x [N, 3]; p = (r0, d0, r_max, n)."""
    s, sa = 0.0, 0.0
    grad = np.zeros_like(x)
    for i in group_a:
        si, sai, g, _ = pair_terms(x, i, group_b, p, cell, pbc)
        s, sa = s + si, sa + sai
        grad[i] += g
    for i in group_b:   # the mirrored sum
        grad[i] += pair_terms(x, i, group_a, p, cell, pbc)[2]
    return s, sa, grad


class Sites:
    """The tables of ``md.build_site_tables`` as numpy arrays."""

    def __init__(self, tables, n_atoms):
        t = tables
        self.A, self.V = n_atoms, t.max_sites
        self.kind, self.ref = t.site_kind.numpy(), t.site_ref.numpy()
        self.group_offset, self.group_atoms, self.group_weights = (a.numpy() for a in (t.group_offset, t.group_atoms,
                                                                                       t.group_weights))
        self.coord, self.coord_params = t.coord.numpy(), t.coord_params.numpy()
        self.member_offset, self.member_site, self.member_weight = (a.numpy() for a in (t.member_offset, t.member_site,
                                                                                        t.member_weight))
        self.pbc = tuple(t.pbc)
        self.cell = np.array(t.cell).reshape(3, 3) if any(t.pbc) else None

    def group(self, g):
        lo, hi = self.group_offset[g], self.group_offset[g + 1]
        return self.group_atoms[lo:hi], self.group_weights[lo:hi]

    def row(self, q):
        """(group A, group B, (r0, d0, r_max, n)) of coordination row q, global atom indices."""
        r0, d0, r_max, _ = self.coord_params[q]
        return self.group(self.coord[q, 1])[0], self.group(self.coord[q, 2])[0], (r0, d0, r_max, int(self.coord[q, 4]))

    def gather(self, x, forces, ext=None):
        """x fp64 [C, A, 3] (coordinates + coordinates_lo), forces fp32 [C, A, 3]; ``ext``: the three extended arrays fp32
        [C, A + V, 3] to write into (zeros if None: slots of no site keep what they hold).  Returns a dict: coords, coords_lo,
        forces (the extended arrays), sites fp64 [C, V, 3] (the positions before the split; s before the floor for a value
        site) and scale [C, V, 3] (the sums of the absolute terms)."""
        Cn, A, V = x.shape[0], self.A, self.V
        xf = x.reshape(-1, 3)
        hi, lo, f = (np.zeros((Cn, A + V, 3), dtype=np.float32) for _ in range(3)) if ext is None else (e.copy() for e in ext)
        xs = x.astype(np.float32)
        hi[:, :A], lo[:, :A], f[:, :A] = xs, (x - xs.astype(np.float64)).astype(np.float32), forces
        sites, scale = np.zeros((Cn, V, 3)), np.zeros((Cn, V, 3))
        for c in range(Cn):
            for v in range(V):
                k = self.kind[c, v]
                if k == NONE:
                    continue
                pos = np.zeros(3)
                if k == CENTER:
                    pos, scale[c, v] = center(xf, *self.group(self.ref[c, v]))
                    sites[c, v] = pos
                elif k == VALUE:
                    ga, gb, p = self.row(self.ref[c, v])
                    s, sa = 0.0, 0.0
                    for i in ga:
                        si, sai, _, _ = pair_terms(xf, i, gb, p, self.cell, self.pbc)
                        s, sa = s + si, sa + sai
                    sites[c, v, 0], scale[c, v, 0] = s, sa
                    pos = np.array([max(s, FLOOR), 0.0, 0.0])
                for d in range(3):
                    hi[c, A + v, d], lo[c, A + v, d] = split(pos[d])
                f[c, A + v] = 0.0
        return {"coords": hi, "coords_lo": lo, "forces": f, "sites": sites, "scale": scale}

    def spread(self, x, forces_ext, rounded=True):
        """The forces [C, A, 3] of the real atoms from the extended forces [C, A + V, 3]: fp32 in, fp64 sums through every
        atom's rows of the inverse table in order, one fp32 rounding (``rounded=False``: fp64 throughout, for the all-fp64
        reference).  Returns (forces, scale): scale fp64 [C, A, 3] the sums of the absolute terms."""
        Cn, A, V = x.shape[0], self.A, self.V
        xf = x.reshape(-1, 3)
        fe = forces_ext.astype(np.float64)
        out, scale = fe[:, :A].copy(), np.abs(fe[:, :A])
        for c in range(Cn):
            for i in range(A):
                gi = c * A + i
                for m in range(self.member_offset[gi], self.member_offset[gi + 1]):
                    v, role = self.member_site[m]
                    if role == ROLE_CENTER:
                        out[c, i] = out[c, i] + self.member_weight[m] * fe[c, A + v]
                        scale[c, i] += np.abs(self.member_weight[m] * fe[c, A + v])
                    else:
                        ga, gb, p = self.row(self.ref[c, v])
                        _, _, g, gabs = pair_terms(xf, gi, gb if role == ROLE_A else ga, p, self.cell, self.pbc)
                        out[c, i] = out[c, i] + fe[c, A + v, 0] * g
                        scale[c, i] += abs(fe[c, A + v, 0]) * gabs
        return (out.astype(np.float32) if rounded else out), scale

    def apply(self, bias, x, forces):
        """The whole chain on a ``_md_bias_ref.Bias`` of the extended tables.  Returns the dict of ``Bias.apply`` with ``forces``
        fp32 [C, A, 3] (the site forces rounded to fp32 as the kernels leave them), plus ``forces64`` (fp64 throughout),
        ``force_scale`` (|model force| + sum |bias terms| per component), ``gather`` and ``forces_ext``."""
        g = self.gather(x, forces)
        x_ext = g["coords"].astype(np.float64) + g["coords_lo"].astype(np.float64)
        out = bias.apply(x_ext, g["forces"])
        f32, _ = self.spread(x, out["forces"])
        exact = g["forces"].astype(np.float64) + out["bias_forces"]
        f64, scale = self.spread(x, exact, rounded=False)
        # (the spread started its scale from |model + bias| of the atom itself: |model| + |bias| instead)
        A = self.A
        scale += np.abs(g["forces"][:, :A].astype(np.float64)) + np.abs(out["bias_forces"][:, :A]) - np.abs(exact[:, :A])
        out.update(forces_ext=out["forces"], forces=f32, forces64=f64, force_scale=scale, gather=g)
        return out


def ulps32(a, b):
    """|a - b| in units of the last place of the fp32 values b."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.maximum(br.ulp32(b), 2.0 ** -149)
