"""Seeded geometries whose neighbor rows are 65 to 256 entries long, for the AEV kernels (numpy only).  The kernels of
csrc/aev.hip and csrc/aev_generic.hip walk a row in 64-entry chunks and have code that only a long row reaches;
tests/test_aev_cases_host.py proves on the CPU which case reaches which of those paths, tests/test_gpu_aev_long_rows.py holds
the kernels to the fp64 oracle on every case.

The geometries are the shell families of tests/_nbr_cases.py (a centre atom inside Fibonacci shells, open boundaries; one
periodic and one with the outer shell that sends bins to the per-atom neighbor kernel), two shell cases of the same kind
with 65 and 127 angular neighbors, and two cases with many long rows: the 9 x 9 x 9 jittered lattice and a dense core
inside a thin shell.  The species labelling decides the block and group structure of a row, so every geometry comes with
one or more labellings:

  built  the four species cycling, as _nbr_cases builds them
  one    every atom the same species: one same-species angular block (ang128: 8128 pairs), one radial group of up to 255
  seven  the seven ANI-2x species cycling: 28 angular blocks, dealt in batches
  lone   one atom of species 0 inside the centre's angular shell, every other atom species 1: blocks with cj = 1 (no
         same-species pair of that species, 1 x n mixed blocks)
  pad    255 neighbors of the centre whose seven per-species counts are 33, 33, 33, 33, 41, 41, 41 (all = 1 mod 8): the
         largest padded radial list k_aev_fwd3 can see, 255 + 49 slots

images12_pbc is a periodic cell smaller than the cutoffs: every atom sits in every row several times through its images,
in the angular and in the far group, so in different 64-entry chunks of a row (tests/_second_order_ref.py).
"""
from __future__ import annotations

import functools
import typing as tp

import numpy as np

import _nbr_cases as nc

RCR = nc.RCR
RCA = nc.RCA
MAX_RAD = 256
MAX_ANG = nc.MAX_ANG
MAX_PER_SPECIES = nc.MAX_PER_SPECIES
PAD_COUNTS = (33, 33, 33, 33, 41, 41, 41)


class AevCase(tp.NamedTuple):
    name: str
    species: np.ndarray                    # [1, N] int32
    coords: np.ndarray                     # [1, N, 3] float32
    cell: tp.Optional[np.ndarray]
    pbc: tp.Optional[tp.Tuple[bool, bool, bool]]
    num_species: int                       # 4 or 7: the AEV constants the labelling needs
    centre: tp.Optional[int] = None        # shell families: the atom with the long row
    over: bool = False                     # the centre's row is one over a limit: zeroed, ANIHIP_ST_ROW_OVERFLOW set
    variants: tp.Tuple[str, ...] = ()      # also run with: "1x" (4 x 8 grid), "smooth", "bent" (unequally spaced shifts)
    general: bool = False                  # also run on a general grid (csrc/aev_generic.hip)

    @property
    def n_atoms(self) -> int:
        return int(self.species.shape[1])

    @property
    def periodic(self) -> bool:
        return self.cell is not None and self.pbc is not None and any(self.pbc)


def long_row_lattice():
    """9 x 9 x 9 atoms on a cubic lattice of spacing 1.5 A, each coordinate jittered by +-0.1 A, the seven ANI-2x species
    at random: an inner atom has about 170 neighbors inside the radial and 56 inside the angular cutoff."""
    rs = np.random.RandomState(7)
    k = np.arange(9) * 1.5
    x = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3) + rs.uniform(-0.1, 0.1, (729, 3))
    return rs.randint(0, 7, (1, 729)).astype(np.int64), x.astype(np.float32)[None]


DENSE_SPACING = 1.0
DENSE_CORE_RADIUS = 3.0
DENSE_SHELL = (96, 4.9)


def dense_cluster():
    """A dense core inside a thin shell: a cubic lattice of spacing 1.0 A jittered by +-0.08 A per coordinate and cut to a
    ball of 3.0 A, inside 96 atoms spread over a sphere of 4.9 A; the seven species at random.  Fewer than 257 atoms in all, so
    no row can pass 256 entries, while every atom of the inner core has 65 to 128 neighbors within 3.5 A (a uniform density
    cannot do that: (5.1 / 3.5)^3 = 3.1 radial neighbors per angular one)."""
    rs = np.random.RandomState(41)
    m = int(np.ceil(DENSE_CORE_RADIUS / DENSE_SPACING)) + 1
    k = (np.arange(-m, m + 1) + 0.5) * DENSE_SPACING
    g = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)
    g = g[np.linalg.norm(g, axis=1) <= DENSE_CORE_RADIUS]
    g = g + rs.uniform(-0.08, 0.08, g.shape)
    x = np.concatenate([g, nc.fibonacci_sphere(DENSE_SHELL[0], DENSE_SHELL[1], phase=0.4)]) + 10.0
    n = x.shape[0]
    return rs.randint(0, 7, (1, n)).astype(np.int32), x.astype(np.float32).reshape(1, n, 3)


def _relabel(species: np.ndarray, how: str, coords: np.ndarray, centre: int) -> np.ndarray:
    n = species.shape[1]
    if how == "built":
        return species.copy()
    if how == "one":
        return np.full_like(species, 2)
    if how == "seven":
        return (np.arange(n, dtype=np.int32) % 7).reshape(1, n)
    if how == "lone":
        out = np.ones_like(species)
        # the first atom after the centre lies on the innermost shell: inside the angular cutoff of the centre
        lone = 1 if centre == 0 else 0
        assert np.linalg.norm(coords[0, lone].astype(np.float64) - coords[0, centre].astype(np.float64)) < RCA - 0.4
        out[0, lone] = 0
        return out
    raise ValueError(how)


def _from_nbr(base: nc.NbrCase, how: str, **kw) -> AevCase:
    sp = _relabel(base.species, how, base.coords, base.centre)
    return AevCase(f"{base.name}/{how}", sp, base.coords, base.cell, base.pbc, 7 if how == "seven" else 4,
                   centre=base.centre, over=bool(base.overflow_rows), **kw)


def _shell(name: str, shells, outer: bool = False, pbc: bool = False) -> nc.NbrCase:
    return nc._shell_case(name, shells, 256, (), pbc, outer)


def _pad_case() -> AevCase:
    """chunk255's geometry (100 atoms at 2.6 A, 155 at 4.4 A) with the labels of PAD_COUNTS dealt at random."""
    base = nc.case_by_name("chunk255_open")
    labels = np.repeat(np.arange(7, dtype=np.int32), PAD_COUNTS)
    np.random.RandomState(3).shuffle(labels)
    sp = base.species.copy()
    sp[0, 0] = 5
    sp[0, 1:] = labels
    return AevCase("chunk255_open/pad", sp, base.coords, None, None, 7, centre=0, general=True)


IMAGES_CELL = nc._cell([[3.7, 0, 0], [0.3, 3.6, 0], [0.1, 0.2, 5.5]])


def _images_case() -> AevCase:
    """12 atoms on a jittered 2 x 2 x 3 grid of a 3.7 x 3.6 x 5.5 A triclinic cell, the four species cycling: about 100
    entries per row, each atom about eight times."""
    rs = np.random.RandomState(23)
    k = np.stack(np.meshgrid(np.arange(2), np.arange(2), np.arange(3), indexing="ij"), axis=-1).reshape(-1, 3)
    frac = (k + 0.5) / np.array([2.0, 2.0, 3.0]) + rs.uniform(-0.06, 0.06, (12, 3))
    x = (frac @ IMAGES_CELL.astype(np.float64)).astype(np.float32)
    sp = (np.arange(12, dtype=np.int32) % 4).reshape(1, 12)
    return AevCase("images12_pbc/built", sp, x.reshape(1, 12, 3), IMAGES_CELL, nc.TTT, 4)


@functools.lru_cache(maxsize=1)
def all_cases() -> tp.Tuple[AevCase, ...]:
    nbr = {c.name: c for c in nc.chunk_cases() + nc.limit_cases()}
    # two shell cases that _nbr_cases does not have: 65 and 127 angular neighbors (odd lengths above 64)
    nbr["ang65_open"] = _shell("ang65", [(65, 2.6, None), (100, 4.4, None)])
    nbr["ang127_open"] = _shell("ang127", [(127, 3.0, None), (128, 4.5, None)])
    out = []
    for k in nc.CHUNK_COUNTS:
        out.append(_from_nbr(nbr[f"chunk{k}_open"], "built", variants=("1x", "smooth", "bent") if k == 193 else ()))
    out.append(_from_nbr(nbr["ang128_at_open"], "built", variants=("1x", "bent"), general=True))
    out.append(_from_nbr(nbr["spec255_at_open"], "built"))
    out.append(_from_nbr(nbr["rad256_at_open"], "built"))
    out.append(_from_nbr(nbr["ang65_open"], "built"))
    out.append(_from_nbr(nbr["ang127_open"], "built", variants=("smooth",)))
    out.append(_from_nbr(nbr["chunk129_pbc"], "built"))
    out.append(_from_nbr(nbr["ang128_at_open"], "one", variants=("smooth", "bent"), general=True))
    out.append(_from_nbr(nbr["chunk255_open"], "one", variants=("1x",)))
    out.append(_from_nbr(nbr["ang127_open"], "one"))
    out.append(_from_nbr(nbr["ang128_at_open"], "seven", variants=("smooth",), general=True))
    out.append(_from_nbr(nbr["chunk256_open"], "seven", variants=("bent",), general=True))
    out.append(_from_nbr(nbr["rad256_at_open_outer"], "seven"))
    out.append(_from_nbr(nbr["ang65_open"], "seven"))
    out.append(_from_nbr(nbr["chunk193_open"], "lone"))
    out.append(_from_nbr(nbr["ang128_at_open"], "lone", variants=("1x",)))
    out.append(_pad_case())
    sp, x = long_row_lattice()
    out.append(AevCase("lattice", sp.astype(np.int32), x, None, None, 7))
    sp, x = dense_cluster()
    out.append(AevCase("dense", sp, x, None, None, 7, variants=("smooth", "bent")))
    out.append(_images_case())
    for name in ("ang128_over_open", "spec255_over_open", "rad256_over_open"):
        out.append(_from_nbr(nbr[name], "built"))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def case_by_name(name: str) -> AevCase:
    for c in all_cases():
        if c.name == name:
            return c
    raise KeyError(name)


CASE_NAMES = tuple(c.name for c in all_cases() if not c.over)
OVER_NAMES = tuple(c.name for c in all_cases() if c.over)
VARIANT_NAMES = tuple((c.name, v) for c in all_cases() for v in c.variants)
GENERAL_NAMES = tuple(c.name for c in all_cases() if c.general)


def moved(case: AevCase, seed: int = 19, step: float = 0.05) -> np.ndarray:
    """The case's coordinates with every atom moved by a seeded displacement of at most `step` A."""
    rs = np.random.RandomState(seed)
    v = rs.normal(size=(case.n_atoms, 3))
    v *= (step * rs.uniform(0.0, 1.0, case.n_atoms) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]
    return (case.coords.astype(np.float64) + v[None]).astype(np.float32)


def split_ranges(case: AevCase) -> tp.Tuple[tp.Tuple[int, int], ...]:
    """Disjoint ranges of central atoms that cover the case.  Shell families: the centre (atom 0) is in the first range,
    all but seven of its neighbors are in the others."""
    n = case.n_atoms
    if case.centre is not None:
        return (0, 8), (8, 8 + (n - 8) // 2), (8 + (n - 8) // 2, n)
    return (0, n // 3), (n // 3, n)


# ---- what a row looks like to the kernels --------------------------------------------------------------------------------

class RowStats(tp.NamedTuple):
    rad: np.ndarray      # [N] entries of the row (neighbors within Rcr)
    ang: np.ndarray      # [N] of them within Rca
    cnt_a: np.ndarray    # [N, S] per-species counts of the angular group
    cnt_f: np.ndarray    # [N, S] per-species counts of the far group
    banded: int          # pairs within nc.BAND of a cutoff (either side): fp32 builders may place them differently


def row_stats(case: AevCase, num_species: int, rcr: float = RCR, rca: float = RCA, coords: tp.Optional[np.ndarray] = None,
              margin: float = 0.0) -> RowStats:
    """Row lengths and per-species counts from fp64 distances of the fp32 coordinates (plain enumeration of the images).
    margin: added to both cutoffs (-+ nc.BAND: the rows without / with every pair an fp32 builder may place either way)."""
    c = case if coords is None else case._replace(coords=coords)
    i, j, _, r = nc.numpy_pairs(nc.NbrCase(c.name, c.species, c.coords, c.cell, c.pbc, ()), rcr + nc.BAND)
    banded = int((np.abs(r - rcr) <= nc.BAND).sum() + (np.abs(r - rca) <= nc.BAND).sum())
    rcr, rca = rcr + margin, rca + margin
    keep = r <= rcr
    i, j, r = i[keep], j[keep], r[keep]
    n = c.n_atoms
    sp = c.species.reshape(-1)[j]
    cnt = np.zeros((n, 2, num_species), dtype=np.int64)
    np.add.at(cnt, (i, (r > rca).astype(np.int64), sp), 1)
    return RowStats(cnt.sum(axis=(1, 2)), cnt[:, 0].sum(axis=1), cnt[:, 0], cnt[:, 1], banded)


def within_limits(st: RowStats, rows=slice(None)) -> bool:
    return bool(st.rad[rows].max() <= MAX_RAD and st.ang[rows].max() <= MAX_ANG
                and (st.cnt_a + st.cnt_f)[rows].max() <= MAX_PER_SPECIES)


def block_pairs(cnt_a: np.ndarray) -> tp.List[int]:
    """Pairs per angular block of one row, blocks in the kernel's order (species pairs tj <= tk, row-major); 0 = absent."""
    S = cnt_a.shape[0]
    return [int(cnt_a[a] * (cnt_a[a] - 1) // 2 if a == b else cnt_a[a] * cnt_a[b]) for a in range(S) for b in range(a, S)]


def pair_dealing(cnt_a: np.ndarray) -> tp.Tuple[int, int, int]:
    """How k_aev_fwd3 deals the pairs of one row to its 64 slots: (I, slots at I, slots at I + 1).
    Restated from csrc/aev.hip:
        block_slots(np, I) = (ceil(np / I) + 3) & ~3          // slots of a block: its pairs, I per slot, padded to 4
        T = nA (nA - 1) / 2,  I = ceil(T / 64)
        if sum_b block_slots(np_b, I) > 64:                    // padding pushed the blocks over the wave
            if sum_b block_slots(np_b, I + 1) <= 64: I += 1    // one more iteration
            else: batches of blocks, I iterations each"""
    nA = int(cnt_a.sum())
    T = nA * (nA - 1) // 2
    I = max(1, -(-T // 64))
    blocks = [p for p in block_pairs(cnt_a) if p > 0]
    slots = lambda it: sum(((-(-p // it)) + 3) & ~3 for p in blocks)   # noqa: E731
    return I, slots(I), slots(I + 1)


def expected_slabs(st: RowStats, num_species: int) -> np.ndarray:
    """Slab flags [N] of the tuned layout (include/anihip.h): bit j < ceil(S / 2) radial slab of species 2j, 2j + 1; then one
    bit per species pair tj <= tk, set when the angular group holds a pair of that block."""
    S = num_species
    n = st.rad.shape[0]
    tot = st.cnt_a + st.cnt_f
    bits = np.zeros(n, dtype=np.int64)
    rs = (S + 1) // 2
    for j in range(rs):
        present = tot[:, 2 * j] > 0
        if 2 * j + 1 < S:
            present |= tot[:, 2 * j + 1] > 0
        bits |= present.astype(np.int64) << j
    P = 0
    for a in range(S):
        for b in range(a, S):
            have = (st.cnt_a[:, a] >= 2) if a == b else ((st.cnt_a[:, a] >= 1) & (st.cnt_a[:, b] >= 1))
            bits |= have.astype(np.int64) << (rs + P)
            P += 1
    return bits


REGIMES = (
    "radial 65..128", "radial 129..192", "radial 193..256",
    "angular 64", "angular 65", "angular 127", "angular 128",
    "angular even > 64", "angular odd > 64",
    "one-species block >= 2016 pairs",
    "pairs dealt with I + 1 iterations",
    "pairs dealt in batches of blocks",
    "species group > 64 entries",
    "padded radial list of 255 + 49",
)


def regimes_of(st: RowStats) -> tp.Set[str]:
    """The regimes of REGIMES that some row of the case reaches."""
    out = set()
    for lo, hi in ((65, 128), (129, 192), (193, 256)):
        if np.any((st.rad >= lo) & (st.rad <= hi)):
            out.add(f"radial {lo}..{hi}")
    for k in (64, 65, 127, 128):
        if np.any(st.ang == k):
            out.add(f"angular {k}")
    long_ang = st.ang[(st.ang > 64) & (st.ang <= MAX_ANG)]
    if np.any(long_ang % 2 == 0):
        out.add("angular even > 64")
    if np.any(long_ang % 2 == 1):
        out.add("angular odd > 64")
    ok = (st.ang <= MAX_ANG) & (st.rad <= MAX_RAD)
    if np.any((st.cnt_a.max(axis=1) >= 64) & ok):   # 64 * 63 / 2 = 2016
        out.add("one-species block >= 2016 pairs")
    if np.any(((st.cnt_a + st.cnt_f).max(axis=1) > 64) & ok):
        out.add("species group > 64 entries")
    for row in np.nonzero(ok & (st.ang >= 2))[0]:
        _, s0, s1 = pair_dealing(st.cnt_a[row])
        if s0 > 64:
            out.add("pairs dealt with I + 1 iterations" if s1 <= 64 else "pairs dealt in batches of blocks")
    tot = st.cnt_a + st.cnt_f
    if np.any(ok & (st.rad == 255) & np.all(tot % 8 == 1, axis=1) & (tot.shape[1] == 7)):
        out.add("padded radial list of 255 + 49")
    return out
