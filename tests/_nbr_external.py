"""Host constructions for the entry points of csrc/nbr.hip that take or give somebody else's list (numpy only): the
reference-style half list of a case, the LAMMPS-style full list over the local atoms and their ghosts, moved coordinates for
the Verlet refresh, and synthetic rows with their half list.  Each is made from a case of tests/_nbr_cases.py and the fp64
oracle's full list (oracle64.neighbors(..., cutoff, cell_list=False) on the case's fp32 coordinates).
tests/test_nbr_external_host.py asserts what they promise on the CPU; tests/test_gpu_neighbors_external.py holds the kernels to
them.

Two shell cases are new here, both open, centre = atom 0, every shell 0.5 A or more from a cutoff:
  * skin_crowd_open: 200 atoms within Rcr and 156 between Rcr and Rcr + 1 -- a skin half list offers the centre 100 candidates
    more than a row holds; they are screened before they count, so the row must not overflow.
  * skin_over_open: 200 atoms within Rcr and 60 between Rcr and Rcr + skin -- the true row fits, the Verlet row (260) does not.
No wide row (Rcr + skin, every entry in the far group) of the other shell cases run without the outer shell exceeds 256 entries
or 255 of one species apart from the rows meant to overflow (the largest is 218), so no shell had to be thinned.
"""
from __future__ import annotations

import typing as tp

import numpy as np

import _nbr_cases as nc
from _nbr_rows import IMG_SPAN, pair_keys

SKIN = 1.0
MOVE_RANDOM = 0.28    # |delta| <= 0.28 sqrt(3) = 0.485 < skin / 2
MOVE_SHELL = 0.10     # relative motion <= 0.2 sqrt(3) = 0.35 < the 0.5 A margins of the shells
# refresh: the stored displacement's error plus the fp32 roundings of d0 + (xj - xj0) - (xi - xi0), each at most half a
# spacing of a number below Rcr + skin; the band is 2 sqrt(3) times that, rounded up
REFRESH_GATE = nc.DISP_GATE + 4.0 * float(np.spacing(np.float32(nc.RCR + SKIN)))
REFRESH_BAND = float(np.ceil(2.0 * np.sqrt(3.0) * REFRESH_GATE * 1e6) / 1e6)
SCAN_TWICE_N = 262144 + 1024 + 5   # k_scan_sums sums 256 blocks of 1024 atoms per turn of its loop


def skin_crowd_case() -> nc.NbrCase:
    return nc._shell_case("skin_crowd", [(100, 2.6, None), (100, 4.4, None), (156, 5.6, None)], 256,
                          ("356 candidates within Rcr + 1, 200 within Rcr",), False, False)


def skin_over_case() -> nc.NbrCase:
    # (overflow_rows stays empty: the plain builders and the external lists give a clean row)
    return nc._shell_case("skin_over", [(100, 2.6, None), (100, 4.4, None), (60, 5.6, None)], 256,
                          ("true row 200, Verlet row 260",), False, False)


def shell_cases() -> tp.List[nc.NbrCase]:
    """The chunk and limit cases without the outer shell (it only steers the cell kernels), open and periodic."""
    return [c for c in nc.chunk_cases() + nc.limit_cases() if not c.name.endswith("_outer")]


def sweep() -> tp.List[nc.NbrCase]:
    return nc.random_cases() + shell_cases()


def move_amplitude(case: nc.NbrCase) -> float:
    return MOVE_RANDOM if case.centre is None else MOVE_SHELL


def oracle_list(oracle64, case: nc.NbrCase, cutoff: float, coords: tp.Optional[np.ndarray] = None, species=None):
    x = case.coords if coords is None else coords
    return oracle64.neighbors(case.species if species is None else species, np.asarray(x, dtype=np.float64), cutoff,
                              case.cell, case.pbc, cell_list=False)


def unpadded_species(case: nc.NbrCase) -> np.ndarray:
    """The case's species with every padding atom turned into species 0: the oracle then lists the pairs that touch it."""
    return np.where(case.species < 0, 0, case.species).astype(np.int32)


def flat_pairs(case: nc.NbrCase, olist, cutoff: float, coords: tp.Optional[np.ndarray] = None):
    """(i, j, d, r, image) of the oracle's ordered pairs within cutoff."""
    start, j, d, r = olist
    n = case.n_atoms
    i = np.repeat(np.arange(n), np.diff(start))
    sel = r <= cutoff
    i, j, d, r = i[sel], j[sel].astype(np.int64), d[sel].astype(np.float64), r[sel].astype(np.float64)
    xw = nc.wrap_f64(case if coords is None else case._replace(coords=coords))
    cell = case.cell.astype(np.float64) if case.periodic else None
    _, img = pair_keys(i, j, d, xw, cell, n)
    return i, j, d, r, img


def first_nonzero_positive(v: np.ndarray) -> np.ndarray:
    """Per row of v [P, 3]: is its first non-zero component positive (all zero: False)."""
    return (v[:, 0] > 0) | ((v[:, 0] == 0) & ((v[:, 1] > 0) | ((v[:, 1] == 0) & (v[:, 2] > 0))))


class HalfList(tp.NamedTuple):
    idx: np.ndarray      # [2, P] int64
    diff: np.ndarray     # [P, 3] float32 = r_idx0 - r_idx1 (+ image shift)
    image: np.ndarray    # [P, 3] image index of the ordered pair (idx0 -> idx1)


def half_list(case: nc.NbrCase, olist, cutoff: float) -> HalfList:
    """The reference-style half list: of the ordered pairs within cutoff those with j > i, and of an atom's own images the
    one whose image index has its first non-zero component positive; diff = -(d) in fp32."""
    i, j, d, _, img = flat_pairs(case, olist, cutoff)
    keep = (j > i) | ((j == i) & first_nonzero_positive(img))
    return HalfList(np.stack([i[keep], j[keep]]), (-d[keep]).astype(np.float32), img[keep])


def shuffled_swapped(h: HalfList, seed: int) -> HalfList:
    """The same pairs in a seeded random order, a random half of them the other way round (a <-> b, diff negated)."""
    rs = np.random.RandomState(seed)
    order = rs.permutation(h.idx.shape[1])
    idx, diff, img = h.idx[:, order].copy(), h.diff[order].copy(), h.image[order].copy()
    swap = rs.uniform(size=order.size) < 0.5
    idx[:, swap] = idx[::-1][:, swap]
    diff[swap] = -diff[swap]
    img[swap] = -img[swap]
    return HalfList(idx, diff, img)


class Expanded(tp.NamedTuple):
    """The open system of a case's local atoms followed by their ghosts, and a LAMMPS-style full list over it."""
    species: np.ndarray      # [1, M] int32
    coords: np.ndarray       # [1, M, 3] float32
    n_local: int
    ghost_j: np.ndarray      # [M - n_local]: the local atom a ghost is an image of
    ghost_image: np.ndarray  # [M - n_local, 3]
    ilist: np.ndarray        # int32, permuted
    numneigh: np.ndarray     # int32, per listed atom
    jlist: np.ndarray        # int32
    has_row: np.ndarray      # [M] bool: listed, numneigh > 0 and a real atom -- every other row must come back empty
    n_candidates: np.ndarray  # [M]: candidates the list offers (padding entries included), 0 where unlisted

    def as_case(self, base: nc.NbrCase) -> nc.NbrCase:
        return base._replace(name=base.name + "+ghosts", species=self.species, coords=self.coords, cell=None, pbc=None)


def expand_ghosts(case: nc.NbrCase, olist, cutoff: float, seed: int = 5, unlisted_every: tp.Optional[int] = 7,
                  empty_every: tp.Optional[int] = 11) -> Expanded:
    """olist: the oracle's list out to `cutoff` (Rcr + 1: the candidates).  Ghost g = n + k for the k-th distinct (j, image
    != 0) of that list, at fp32(x_j + image @ cell) with the species of j.  The full list gives every listed local atom its
    candidates (local index or ghost), its own index and three seeded indices from outside its candidates, shuffled; local
    atoms i = 3 mod unlisted_every are not listed, i = 5 mod empty_every are listed with numneigh = 0; ilist is permuted."""
    n = case.n_atoms
    rs = np.random.RandomState(seed)
    i, j, _, _, img = flat_pairs(case, olist, cutoff)
    xw = nc.wrap_f64(case)
    sp = case.species.reshape(-1)
    is_ghost = np.any(img != 0, axis=1)
    span = IMG_SPAN
    gkey = ((j * span + img[:, 0] + span // 2) * span + img[:, 1] + span // 2) * span + img[:, 2] + span // 2
    uniq, first, inverse = np.unique(gkey[is_ghost], return_index=True, return_inverse=True)
    ghost_j = j[is_ghost][first]
    ghost_image = img[is_ghost][first]
    target = j.copy()
    target[is_ghost] = n + inverse
    m = n + uniq.size
    cell = case.cell.astype(np.float64) if case.periodic else np.zeros((3, 3))
    coords = np.concatenate([xw, xw[ghost_j] + ghost_image.astype(np.float64) @ cell]).astype(np.float32)
    species = np.concatenate([sp, sp[ghost_j]]).astype(np.int32)
    local = np.arange(n)
    listed = np.ones(n, dtype=bool) if unlisted_every is None else local % unlisted_every != 3
    empty = np.zeros(n, dtype=bool) if empty_every is None else local % empty_every == 5
    start = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=n))])
    ilist = rs.permutation(local[listed]).astype(np.int32)
    if ilist.size > 1 and np.all(np.diff(ilist) > 0):
        ilist = ilist[::-1].copy()
    rows, numneigh = [], []
    n_cand = np.zeros(m, dtype=np.int64)
    for a in ilist:
        if empty[a]:
            numneigh.append(0)
            continue
        cand = target[start[a]:start[a + 1]]
        extra = rs.randint(0, m, 3)
        extra = extra[~np.isin(extra, cand) & (extra != a)]   # (all within the candidates' cutoff are candidates already)
        row = np.concatenate([cand, [a], extra])
        rows.append(rs.permutation(row))
        numneigh.append(row.size)
        n_cand[a] = row.size
    has_row = np.zeros(m, dtype=bool)
    has_row[:n] = listed & ~empty & (sp >= 0)
    jlist = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, dtype=np.int32)
    return Expanded(species.reshape(1, m), coords.reshape(1, m, 3), n, ghost_j, ghost_image, ilist,
                    np.asarray(numneigh, dtype=np.int32), jlist, has_row, n_cand)


def moved(case: nc.NbrCase, amplitude: float, seed: int) -> np.ndarray:
    """The case's coordinates displaced per component by a uniform +-amplitude, fp32 [1, N, 3]."""
    rs = np.random.RandomState(seed)
    delta = rs.uniform(-amplitude, amplitude, case.coords.shape).astype(np.float32)
    return (case.coords + delta).astype(np.float32)


# ---- synthetic rows and their half list --------------------------------------------------------------------------------------

class Synthetic(tp.NamedTuple):
    meta: np.ndarray   # [n, 6] uint32
    ent: np.ndarray    # [3 n, 4] float32
    n: int


def synthetic_rows(n: int, seed: int) -> Synthetic:
    """Rows in the format of include/anihip.h, row capacity 3, 0 to 3 entries per atom: j uniform over all atoms (both sides
    of i), one entry in sixteen an own image (j = i) whose displacement has its leading components zeroed at random, so that
    each branch of the own-image rule decides, with either sign.  Displacement components are multiples of 1/8 below 5: the
    squares and their sum are exact in fp32 whatever the order or fusing of the operations."""
    rs = np.random.RandomState(seed)
    cnt = rs.randint(0, 4, n)
    meta = np.zeros((n, 6), dtype=np.uint32)
    meta[:, 0] = 3 * np.arange(n)
    nA = cnt // 2
    meta[:, 1] = nA | ((cnt - nA) << 16)
    j = rs.randint(0, n, (n, 3))
    own = rs.uniform(size=(n, 3)) < 1.0 / 16.0
    j[own] = np.broadcast_to(np.arange(n)[:, None], (n, 3))[own]
    k = rs.randint(1, 40, (n, 3, 3)) * rs.choice([-1, 1], (n, 3, 3))
    lead = rs.randint(0, 3, (n, 3))            # own images: this many leading components are zero
    for q in range(2):
        k[..., q][own & (lead > q)] = 0
    sp = rs.randint(0, 4, (n, 3))
    ent = np.zeros((n, 3, 4), dtype=np.float32)
    ent[..., :3] = k.astype(np.float32) / 8.0
    ent[..., 3] = (j.astype(np.uint32) | (sp.astype(np.uint32) << 28)).view(np.float32)
    return Synthetic(meta, ent.reshape(3 * n, 4), n)


def numpy_half_keep(i: np.ndarray, j: np.ndarray, d: np.ndarray) -> np.ndarray:
    """half_keep of csrc/nbr.hip restated: j > i, and of an atom's own images the displacement whose first non-zero component
    is positive."""
    return np.where(j != i, j > i, first_nonzero_positive(d))


def synthetic_half(s: Synthetic, lo: int, hi: int):
    """(idx [2, P], diff [P, 3], dist [P]) that anihip_nbr_rows_to_half must give for the rows lo..hi: the kept entries in row
    order, offsets by an exclusive cumsum of the per-atom counts."""
    m = s.meta[lo:hi].astype(np.int64)
    cnt = (m[:, 1] & 0xFFFF) + (m[:, 1] >> 16)
    i = np.repeat(np.arange(lo, hi), cnt)
    first = np.cumsum(cnt) - cnt
    e = s.ent[np.repeat(m[:, 0], cnt) + np.arange(int(cnt.sum())) - np.repeat(first, cnt)]
    j = (np.ascontiguousarray(e[:, 3]).view(np.uint32) & 0x0FFFFFFF).astype(np.int64)
    keep = numpy_half_keep(i, j, e[:, :3])
    per_atom = np.bincount(i[keep] - lo, minlength=hi - lo)
    offs = np.cumsum(per_atom) - per_atom
    d = e[keep, :3]
    dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).astype(np.float32))
    assert int(offs[-1] + per_atom[-1]) == int(keep.sum())
    return np.stack([i[keep], j[keep]]), -d, dist
