"""fp64 numpy statements of the observables of torchani_amd.md (include/anihip.h: anihip_md_rdf_accumulate and
anihip_md_corr_accumulate), written from the definitions, not from the kernels."""
import itertools

import numpy as np


def pair_distances(x, cell=None, pbc=(False, False, False), r_cut=0.0):
    """Every ordered pair (i, j, image) of one entry with 0 < r <= r_cut, periodic images and an atom's own image included:
    (i [n], j [n], r [n]) in fp64.  x [A, 3]; cell rows are the lattice vectors."""
    x = np.asarray(x, dtype=np.float64)
    shifts = np.zeros((1, 3))
    if cell is not None and any(pbc):
        cell = np.asarray(cell, dtype=np.float64)
        inv = np.linalg.inv(cell)
        # images needed along vector k: r_cut over the perpendicular width
        reach = [int(np.ceil(r_cut * np.linalg.norm(inv[:, k]))) if pbc[k] else 0 for k in range(3)]
        # atoms need not lie inside the cell: one more image covers any offset of up to a lattice vector
        frac = x @ inv
        extra = [int(np.ceil(np.ptp(frac[:, k]))) if pbc[k] else 0 for k in range(3)]
        n = [range(-(reach[k] + extra[k]), reach[k] + extra[k] + 1) for k in range(3)]
        shifts = np.array([np.array(s, dtype=np.float64) @ cell for s in itertools.product(*n)])
    ii, jj, rr = [], [], []
    for s in shifts:
        d = x[None, :, :] + s[None, None, :] - x[:, None, :]   # d[i, j] = x_j + s - x_i
        r = np.sqrt((d * d).sum(-1))
        keep = (r <= r_cut) & ((r > 0) | np.any(s != 0))
        if not np.any(s != 0):
            keep &= ~np.eye(x.shape[0], dtype=bool)
        i, j = np.nonzero(keep)
        ii.append(i), jj.append(j), rr.append(r[i, j])
    return np.concatenate(ii), np.concatenate(jj), np.concatenate(rr)


def rdf_counts(species, coords, pairs, r_max, bins, cell=None, pbc=(False, False, False), per_entry=False, margin=0.0):
    """counts [C, P, bins] (or [P, bins]) of the definition: row entries (i -> j) with species_i = a_p, species_j = b_p,
    floor(r / delta) = b, r < r_max; species [C, A] (negative: padding), coords [C, A, 3], pairs [(a, b)] of species values.
    With ``margin`` > 0 also returns near [C, P, bins + 1] (or [P, bins + 1]): the pairs whose distance lies within ``margin`` of
    edge e delta (e = bins: r_max), which may fall on either side."""
    species, coords = np.asarray(species), np.asarray(coords, dtype=np.float64)
    Cn, P = species.shape[0], len(pairs)
    delta = r_max / bins
    counts = np.zeros((Cn, P, bins), dtype=np.int64)
    near = np.zeros((Cn, P, bins + 1), dtype=np.int64)
    for c in range(Cn):
        real = np.nonzero(species[c] >= 0)[0]
        i, j, r = pair_distances(coords[c][real], cell, pbc, r_max + margin)
        si, sj = species[c][real][i], species[c][real][j]
        for p, (a, b) in enumerate(pairs):
            rp = r[(si == a) & (sj == b)]
            inside = rp[rp < r_max]
            counts[c, p] = np.bincount(np.minimum(np.floor(inside / delta).astype(np.int64), bins - 1), minlength=bins)
            if margin > 0:
                e = np.rint(rp / delta).astype(np.int64)
                close = (np.abs(rp - e * delta) <= margin) & (e >= 1) & (e <= bins)
                near[c, p] = np.bincount(e[close], minlength=bins + 1)
    if not per_entry:
        counts, near = counts.sum(0), near.sum(0)
    return (counts, near) if margin > 0 else counts


class Correlation:
    """Multiple time origins over the last M samples: S[c, s, l] and the origins n_l, sample by sample.  kind "msd":
    sum |y(k) - y(k - l)|^2; "vacf": sum y(k) . y(k - l).  species [C, A] (negative: padding) take the values
    0 .. n_species - 1; ``abs_sums`` keeps sum |terms| (the scale of the rounding error of a signed sum)."""

    def __init__(self, kind, species, n_species, lags):
        assert kind in ("msd", "vacf")
        self.kind, self.species, self.S, self.M = kind, np.asarray(species), int(n_species), int(lags)
        Cn = self.species.shape[0]
        self.sums = np.zeros((Cn, self.S, self.M))
        self.abs_sums = np.zeros((Cn, self.S, self.M))
        self.origins = np.zeros(self.M, dtype=np.int64)
        self.history = []   # the last M samples, newest last
        self.k = 0

    def add(self, y):
        y = np.asarray(y, dtype=np.float64)
        self.history.append(y)
        if len(self.history) > self.M:
            self.history.pop(0)
        onehot = (self.species[:, :, None] == np.arange(self.S)[None, None, :]).astype(np.float64)   # [C, A, S]
        for l in range(min(self.k, self.M - 1) + 1):   # noqa: E741
            old = self.history[-1 - l]
            term = ((y - old) ** 2).sum(-1) if self.kind == "msd" else (y * old).sum(-1)   # [C, A]
            size = term if self.kind == "msd" else np.abs(y * old).sum(-1)
            self.sums[:, :, l] += np.einsum("ca,cas->cs", term, onehot)
            self.abs_sums[:, :, l] += np.einsum("ca,cas->cs", size, onehot)
            self.origins[l] += 1
        self.k += 1

    def atom_counts(self):
        return np.stack([(self.species == s).sum(1) for s in range(self.S)], axis=1)

    def mean(self):
        """S / (n_l N_cs): NaN where a lag has no origin or a species no atom."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.sums / (self.origins[None, None, :] * self.atom_counts()[:, :, None].astype(np.float64))
