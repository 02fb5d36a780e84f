"""Seeded geometries for the neighbor-builder sweep (numpy only): skewed, thin and uneven cells, partial periodicity, empty
and crowded bins, and rows exactly at / one over the three row limits.  tests/test_neighbor_cases_host.py holds the fp64
oracle to them on the CPU, tests/test_gpu_neighbors.py the HIP builders pair for pair, and
tests/golden/gen_golden_nbr_sweep.py writes the reference's counts for some of them.

Every case: species [1, N] int32, coords [1, N, 3] float32, cell (3, 3) float32 or None, pbc or None, the two cutoffs, a row
capacity, and the regimes it is meant to reach.  `kernel` says which of the two cell kernels must take its bins
("bin": none left to the per-atom kernel, "atom": all, "both": strictly between, None: not pinned); grid_model() below
predicts that from the documented grid rule, so that a case which does not land where it should fails on the CPU.

Departures from the sizes first sketched for this sweep, each because the case did not reach its regime otherwise:
  * ortho is diag(41.5, 20.6, 15.5), not diag(41, 23, 17): with 5.1 / 5.75 / 5.67 A bins a stencil holds about 450 atoms,
    so about half of the bins went over the 448 candidates of the per-bin kernel and "none left over" did not hold.
  * wide (diag 20.6) runs with max_cells = 8: floor(20.6 / 5.1) = 4 bins per axis, and it is the coarsening to 2 x 2 x 2
    that gives the 10.3 A bins and ~2 900 candidates per stencil that send every bin to the per-atom kernel.
  * the outer shell of the shell families has 560 atoms, not 300: a 9 A sphere sticks out of the centre's stencil (half-width
    8.2 A), 73 % of it is inside, and 64 + 0.73 * 300 candidates stay under 448.
"""
from __future__ import annotations

import typing as tp

import numpy as np

from _nbr_rows import wrap_coords

RCR = 5.1
RCA = 3.5
NUM_SPECIES = 4
DENSITY = 0.1
# |d - d_ref| gate of the row comparison (A) and the borderline band that follows from it: a pair whose fp64 distance is
# within BAND of a cutoff may fall on either side of it (2 * sqrt(3) * 5e-6 = 1.73e-5, rounded up)
DISP_GATE = 5e-6
BAND = 2e-5
BAND_SHARE = 1e-3
MAX_ANG = 128
MAX_PER_SPECIES = 255
CAND_CAP = 448      # candidates the per-bin kernel stages
STENCIL_CAP = 64    # stencil bins it resolves
BATCH_MAX_ATOMS = 1300


class NbrCase(tp.NamedTuple):
    name: str
    species: np.ndarray
    coords: np.ndarray
    cell: tp.Optional[np.ndarray]
    pbc: tp.Optional[tp.Tuple[bool, bool, bool]]
    regimes: tp.Tuple[str, ...]
    row_cap: int = 256
    rcr: float = RCR
    rca: float = RCA
    max_cells: tp.Optional[int] = None
    kernel: tp.Optional[str] = None            # "bin" | "atom" | "both" | None
    overflow_rows: tp.Tuple[int, ...] = ()     # rows that must come back zeroed with ANIHIP_ST_ROW_OVERFLOW set
    centre: tp.Optional[int] = None            # shell families: the central atom
    limits: tp.Optional[tp.Tuple[int, int, int]] = None   # shell families: (row, angular, per species) limit in force
    coarsened: bool = False                    # ANIHIP_ST_GRID_OVERFLOW expected
    golden: tp.Optional[str] = None            # tests/golden/nbrsweep_<golden>.npz holds the reference's counts

    @property
    def n_atoms(self) -> int:
        return int(self.species.shape[1])

    @property
    def periodic(self) -> bool:
        return self.cell is not None and self.pbc is not None and any(self.pbc)


def _cell(rows) -> np.ndarray:
    return np.asarray(rows, dtype=np.float32).reshape(3, 3)


def _diag(a, b, c) -> np.ndarray:
    return _cell([[a, 0, 0], [0, b, 0], [0, 0, c]])


def _random_in_cell(seed: int, cell: np.ndarray, n: tp.Optional[int] = None, outside: bool = False):
    """Uniform random fractional coordinates in `cell` at DENSITY; `outside`: a fifth of the atoms get integer lattice offsets
    in -3..3 before the cast to fp32."""
    rs = np.random.RandomState(seed)
    c64 = cell.astype(np.float64)
    if n is None:
        n = int(round(DENSITY * abs(np.linalg.det(c64))))
    frac = rs.uniform(0.0, 1.0, (n, 3))
    if outside:
        pick = rs.permutation(n)[: n // 5]
        frac[pick] += rs.randint(-3, 4, (pick.size, 3))
    species = rs.randint(0, NUM_SPECIES, n).astype(np.int32)
    return species.reshape(1, n), (frac @ c64).astype(np.float32).reshape(1, n, 3)


ORTHO_CELL = _diag(41.5, 20.6, 15.5)
SKEW_CELL = _cell([[30, 0, 0], [14, 22, 0], [-9, 11, 19]])
SLAB_CELL = _cell([[3.9, 0, 0], [0.5, 33, 0], [0.2, 3, 28]])
ROD_CELL = _diag(4.4, 4.6, 60)
TINY_CELL = _cell([[2.9, 0, 0], [0.3, 3.1, 0], [0.1, 0.2, 3.3]])
WIDE_CELL = _diag(20.6, 20.6, 20.6)
BIG_CELL = _diag(60, 60, 60)
TTT, TTF, TFF, FFF = (True, True, True), (True, True, False), (True, False, False), (False, False, False)


def _pbc_tag(pbc) -> str:
    return "".join("T" if b else "F" for b in pbc)


def random_cases() -> tp.List[NbrCase]:
    out = []
    sp, x = _random_in_cell(11, ORTHO_CELL, outside=True)
    out.append(NbrCase("ortho", sp, x, ORTHO_CELL, TTT, ("unequal bin counts per axis", "outside atoms"), kernel="bin",
                       golden="ortho"))
    sp_s, x_s = _random_in_cell(12, SKEW_CELL, outside=True)
    for pbc in (TTT, TTF, TFF, FFF):
        out.append(NbrCase("skew_" + _pbc_tag(pbc), sp_s, x_s, SKEW_CELL, pbc,
                           ("triclinic bins", "bounding-box axes", "outside atoms"), golden="skew_" + _pbc_tag(pbc)))
    sp, x = _random_in_cell(13, SLAB_CELL)
    out.append(NbrCase("slab", sp, x, SLAB_CELL, TTT, ("one bin and half-width 2 on one axis", "self images"), golden="slab"))
    sp, x = _random_in_cell(14, ROD_CELL)
    out.append(NbrCase("rod", sp, x, ROD_CELL, TTT, ("stencil of 75 bins",), kernel="atom", golden="rod"))
    sp, x = _random_in_cell(15, TINY_CELL, n=3)
    out.append(NbrCase("tiny", sp, x, TINY_CELL, TTT, ("125-bin stencil", "many self images"), kernel="atom", golden="tiny"))
    sp, x = _random_in_cell(16, WIDE_CELL)
    out.append(NbrCase("wide", sp, x, WIDE_CELL, TTT, ("10.3 A bins", "thousands of candidates per stencil"), max_cells=8,
                       kernel="atom", coarsened=True))
    # droplet: 600 atoms in a 9 A ball at the middle of the big cell, 300 spread over the rest
    rs = np.random.RandomState(17)
    v = rs.normal(size=(600, 3))
    v *= (9.0 * rs.uniform(0.0, 1.0, 600) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]
    xd = np.concatenate([v + 30.0, rs.uniform(0.0, 60.0, (300, 3))]).astype(np.float32).reshape(1, 900, 3)
    spd = rs.randint(0, NUM_SPECIES, 900).astype(np.int32).reshape(1, 900)
    out.append(NbrCase("droplet_TTT", spd, xd, BIG_CELL, TTT, ("empty bins", "crowded beside sparse", "both kernels"),
                       kernel="both"))
    out.append(NbrCase("droplet_none", spd, xd, None, None, ("empty bins", "crowded beside sparse", "both kernels"),
                       kernel="both"))
    o = out[0]
    for mc in (8, 1):
        out.append(o._replace(name=f"coarse_{mc}", max_cells=mc, kernel=None, coarsened=True, golden=None,
                              regimes=("grid coarsening",)))
    sp_p = sp_s.copy()
    sp_p[0, ::7] = -1
    out.append(NbrCase("padded", sp_p, x_s, SKEW_CELL, TTF, ("padding atoms in no bin", "empty rows")))
    rs = np.random.RandomState(18)
    xc = rs.uniform(0.0, 1.0, (900, 3)) * np.array([33.0, 21.0, 13.0]) - 4.0
    out.append(NbrCase("cluster", rs.randint(0, NUM_SPECIES, 900).astype(np.int32).reshape(1, 900),
                       xc.astype(np.float32).reshape(1, 900, 3), None, None, ("bounding-box grid",)))
    return out


# ---- shell families --------------------------------------------------------------------------------------------------------

def fibonacci_sphere(n: int, radius: float, phase: float = 0.0) -> np.ndarray:
    """n evenly spread points on a sphere (golden-angle spiral)."""
    k = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * (np.pi * (3.0 - np.sqrt(5.0))) + phase
    s = np.sqrt(1.0 - z * z)
    return radius * np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1)


OUTER_SHELL_ATOMS = 560
OUTER_SHELL_RADIUS = 9.0


def _shell_case(name, shells, row_cap, regimes, pbc, outer, over=False, limits=(256, MAX_ANG, MAX_PER_SPECIES)):
    """Central atom (index 0) at the middle of the big cell + shells [(count, radius, species or None = cycling 0..3)]."""
    pts, sps = [np.zeros((1, 3))], [np.array([1], dtype=np.int32)]
    for q, (cnt, radius, species) in enumerate(shells):
        pts.append(fibonacci_sphere(cnt, radius, phase=0.7 * q))
        sps.append(np.full(cnt, species, dtype=np.int32) if species is not None
                   else (np.arange(cnt) % NUM_SPECIES).astype(np.int32))
    if outer:
        pts.append(fibonacci_sphere(OUTER_SHELL_ATOMS, OUTER_SHELL_RADIUS, phase=0.3))
        sps.append((np.arange(OUTER_SHELL_ATOMS) % NUM_SPECIES).astype(np.int32))
    x = (np.concatenate(pts) + 30.0).astype(np.float32)
    sp = np.concatenate(sps)
    n = sp.shape[0]
    tag = ("_pbc" if pbc else "_open") + ("_outer" if outer else "")
    return NbrCase(name + tag, sp.reshape(1, n), x.reshape(1, n, 3), BIG_CELL if pbc else None, TTT if pbc else None,
                   tuple(regimes) + (("past 448 candidates: per-atom kernel",) if outer else ()), row_cap=row_cap,
                   kernel="both" if outer else None, overflow_rows=(0,) if over else (), centre=0, limits=limits)


CHUNK_COUNTS = (63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)


def chunk_cases() -> tp.List[NbrCase]:
    """k neighbors of the centre across the 64-hit chunk boundaries of the row writers; no row may overflow."""
    out = []
    for k in CHUNK_COUNTS:
        near = min(100, k // 2)
        for pbc in (True, False):
            for outer in (False, True):
                out.append(_shell_case(f"chunk{k}", [(near, 2.6, None), (k - near, 4.4, None)], 256,
                                       (f"{k} hits: chunk boundary",), pbc, outer))
    return out


def limit_cases() -> tp.List[NbrCase]:
    """Each row limit exactly reached (clean build) and one over (the centre's row zeroed, the flag set, all else intact)."""
    out = []
    for pbc in (True, False):
        for outer in (False, True):
            for over in (0, 1):
                t = "over" if over else "at"
                a = (pbc, outer, bool(over))
                out.append(_shell_case(f"cap64_{t}", [(64 + over, 4.4, None)], 64, ("row capacity 64",), *a,
                                       limits=(64, MAX_ANG, MAX_PER_SPECIES)))
                out.append(_shell_case(f"ang128_{t}", [(128 + over, 3.0, None)], 256, ("angular limit 128",), *a))
                out.append(_shell_case(f"spec255_{t}", [(255 + over, 4.5, 0)], 256, ("8-bit per-species count",), *a))
                # all of them in the far group: the far count itself reaches 256
                out.append(_shell_case(f"rad256_{t}", [(256 + over, 4.5, None)], 256, ("radial limit 256",), *a))
    return out


def edge_cases() -> tp.List[NbrCase]:
    """Pairs along the first lattice axis at Rcr -+ 1e-3 and Rca -+ 1e-3, coordinates exactly representable in fp32 (multiples
    of 2^-10 A; the cutoffs 5.1 and 3.5 are taken as the fp32 kernels see them), nothing excused.  Each pair sits in a
    corner of the cell of its own, far from the others; once inside the cell, once across the periodic boundary."""
    q = 1.0 / 1024.0
    gaps = [np.floor((RCR - 1e-3) / q) * q, np.ceil((RCR + 1e-3) / q) * q, np.floor((RCA - 1e-3) / q) * q,
            np.ceil((RCA + 1e-3) / q) * q]
    out = []
    for across in (False, True):
        pts = []
        for m, gap in enumerate(gaps):
            y, z = 10.0 + 20.0 * (m % 2), 10.0 + 20.0 * (m // 2)
            x0 = 60.0 - 2.0 if across else 20.0
            pts += [[x0, y, z], [x0 + gap - (60.0 if across else 0.0), y, z]]
        x = np.asarray(pts, dtype=np.float32)
        assert np.array_equal(x.astype(np.float64), np.asarray(pts)), "edge coordinates must be exact in fp32"
        sp = (np.arange(8) % NUM_SPECIES).astype(np.int32)
        out.append(NbrCase("edge_across" if across else "edge_inside", sp.reshape(1, 8), x.reshape(1, 8, 3), BIG_CELL, TTT,
                           ("pairs 1e-3 A inside / outside each cutoff",)))
    return out


# what the four pairs of an edge case must be: (in the row at all, in the angular group)
EDGE_EXPECT = ((True, False), (False, False), (True, True), (True, False))


def all_cases() -> tp.List[NbrCase]:
    return random_cases() + chunk_cases() + limit_cases() + edge_cases()


def case_by_name(name: str) -> NbrCase:
    for c in all_cases():
        if c.name == name:
            return c
    raise KeyError(name)


GOLDEN_CASES = tuple(c.name for c in random_cases() if c.golden)


# ---- plain references ------------------------------------------------------------------------------------------------------

def wrap_f64(case: NbrCase) -> np.ndarray:
    """The case's fp32 coordinates mapped into the cell along the periodic axes, in fp64 (frac -= floor(frac))."""
    return wrap_coords(case.coords, case.cell if case.periodic else None, case.pbc)


def image_repeats(case: NbrCase, cutoff: float) -> np.ndarray:
    if not case.periodic:
        return np.zeros(3, dtype=np.int64)
    inv = np.linalg.inv(case.cell.astype(np.float64))
    return np.where(case.pbc, np.ceil(cutoff * np.linalg.norm(inv, axis=0)), 0).astype(np.int64)


def numpy_pairs(case: NbrCase, cutoff: float):
    """Every ordered (i, j, image) with |x_j + image @ cell - x_i| <= cutoff by plain enumeration: (i, j, image [P, 3], r)."""
    x = wrap_f64(case)
    real = case.species.reshape(-1) >= 0
    rep = image_repeats(case, cutoff)
    c = case.cell.astype(np.float64) if case.periodic else np.eye(3)
    oi, oj, om, orr = [], [], [], []
    idx = np.arange(x.shape[0])
    for n0 in range(-rep[0], rep[0] + 1):
        for n1 in range(-rep[1], rep[1] + 1):
            for n2 in range(-rep[2], rep[2] + 1):
                img = np.array([n0, n1, n2])
                xs = x + img.astype(np.float64) @ c
                # (an image whose bounding box is further than the cutoff from the atoms' own holds no pair)
                gap = np.maximum(0.0, np.maximum(xs[real].min(0) - x[real].max(0), x[real].min(0) - xs[real].max(0)))
                if np.linalg.norm(gap) > cutoff:
                    continue
                d = xs[None, :, :] - x[:, None, :]
                r = np.sqrt((d * d).sum(-1))
                hit = (r <= cutoff) & real[:, None] & real[None, :]
                if n0 == 0 and n1 == 0 and n2 == 0:
                    hit[idx, idx] = False
                i, j = np.nonzero(hit)
                oi.append(i)
                oj.append(j)
                orr.append(r[i, j])
                om.append(np.broadcast_to(img, (i.size, 3)))
    return np.concatenate(oi), np.concatenate(oj), np.concatenate(om), np.concatenate(orr)


def grid_model(case: NbrCase, max_cells: tp.Optional[int] = None):
    """The grid anihip_nbr_build_cell lays over a case, from its documented rule: along a periodic axis floor(height /
    Rcr) bins and a stencil half-width of ceil(Rcr / bin width); along any other axis the bounding box of the atoms cut
    into bins no narrower than Rcr, half-width 1; the longest axis halved until the grid fits max_cells.  Returns (bins
    per axis, stencil bins, number of occupied bins, number of occupied bins whose stencil holds more than CAND_CAP
    candidates or has more than STENCIL_CAP bins)."""
    n = case.n_atoms
    if max_cells is None:
        max_cells = case.max_cells if case.max_cells is not None else max(4096, 2 * n)
    real = case.species.reshape(-1) >= 0
    x = case.coords.reshape(-1, 3).astype(np.float64)[real]
    c = case.cell.astype(np.float64) if case.periodic else np.eye(3)
    pbc = np.asarray(case.pbc if case.periodic else (False,) * 3)
    inv = np.linalg.inv(c)
    h = 1.0 / np.linalg.norm(inv, axis=0)
    f = x @ inv
    f -= np.floor(f) * pbc
    f0 = np.where(pbc, 0.0, f.min(axis=0))
    span = np.where(pbc, 1.0, f.max(axis=0) - f.min(axis=0) + 2e-4 / h)
    nb = np.maximum(1, np.floor(span * h / case.rcr).astype(np.int64))
    while nb.prod() > max_cells:
        k = int(np.argmax(nb))
        nb[k] = (nb[k] + 1) // 2
    rng = np.where(pbc, np.ceil(case.rcr / (span * h / nb)), 1).astype(np.int64)
    b = np.clip(np.floor((f - f0) / span * nb).astype(np.int64), 0, nb - 1)
    cnt = np.zeros(tuple(nb), dtype=np.int64)
    np.add.at(cnt, (b[:, 0], b[:, 1], b[:, 2]), 1)
    cand = np.zeros_like(cnt)
    for o0 in range(-rng[0], rng[0] + 1):
        for o1 in range(-rng[1], rng[1] + 1):
            for o2 in range(-rng[2], rng[2] + 1):
                sh = cnt
                for k, o in enumerate((o0, o1, o2)):
                    if pbc[k]:
                        sh = np.roll(sh, -o, axis=k)
                    elif o:
                        z = np.zeros_like(sh)
                        src = [slice(None)] * 3
                        dst = [slice(None)] * 3
                        src[k] = slice(o, None) if o > 0 else slice(None, o)
                        dst[k] = slice(None, -o) if o > 0 else slice(-o, None)
                        z[tuple(dst)] = sh[tuple(src)]
                        sh = z
                cand += sh
    stencil = int(np.prod(2 * rng + 1))
    occupied = cnt > 0
    left = occupied & ((cand > CAND_CAP) | (stencil > STENCIL_CAP))
    return tuple(int(v) for v in nb), stencil, int(occupied.sum()), int(left.sum())
