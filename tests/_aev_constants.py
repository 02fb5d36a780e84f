"""Constant sets off the published models' for the tuned AEV kernels, and small geometries to run them on (numpy only).
k_aev_fwd3, k_aev_bwd and k_aev_jvp of csrc/aev.hip are picked from the grid SIZES alone (16 radial shifts, an 8 x 4 or a
4 x 8 angular grid); every other constant is free, and AEVComputer.from_constants hands it to them.  What depends on the
constants is decided by anihip_aev_table_pack: it admits the forward's Gaussian recurrence over ShfA (ANIHIP_AEV_UNIFORM_SHFA,
flag 1) and the backward's recurrences over ShfR and ShfA (ANIHIP_AEV_REC_BWD, flag 2) by inequalities on the exponents the
kernels can meet, and the kernels clamp those exponents to match.  The quantities are restated here in fp64 from the fp32
constants (admission()):

  forward            xm = qA max(|Rca - ShfA[c]|, ShfA[c]), c = nA / 2 - 1, qA = sqrt(EtaA log2 e), D = qA (ShfA[1] - ShfA[0]):
                     max(xm^2, 2 D xm) < 100
  backward angular   max((nA / 2) 2 D_A xa, (nA / 2)^2 D_A^2) < 110, xa = xm, D_A = qA (ShfA[-1] - ShfA[0]) / (nA - 1)
  backward radial    2 D_R xr + 16 D_R^2 < 110, xr = qR max(|Rcr - ShfR[9]|, ShfR[9]), D_R = qR (ShfR[15] - ShfR[0]) / 15

The flag of the backward needs both of its inequalities and both shift arrays equally spaced, the forward's only ShfA.

SETS is the named table (each entry: what it reaches, the flags the packer must give it, the geometries it runs on); the
boundary sets are the ANI-2x constants with the largest two-digit EtaA or EtaR that keeps a flag and the smallest that
clears it (tests/test_aev_constants_host.py finds the same numbers by asking the packer).  sweep() is a seeded sweep of 24
trials over the free constants.  tests/test_aev_constants_host.py proves the flags, the row shapes and that fp32 can hold
the gates on these inputs; tests/test_gpu_aev_constants.py holds the kernels to the fp64 oracle on them."""
from __future__ import annotations

import functools
import math
import typing as tp

import numpy as np

import _aev_cases as ac
import _nbr_cases as nc

LOG2E = float(np.float32(1.4426950408889634))   # csrc/anihip_common.h LOG2E: a float
FWD_BOUND = 100.0
BWD_BOUND = 110.0
MIN_DIST = 0.75
GEOMS = ("cluster40", "tric60", "batch3x14")
LONG_ROW_CASE = "chunk129_open/built"   # tests/_aev_cases.py: a row of 129 entries, two 64-entry chunk seams


def _f32(v) -> float:
    return float(np.float32(v))


def _f32s(v) -> tp.Tuple[float, ...]:
    return tuple(float(x) for x in np.asarray(v, dtype=np.float32))


def _ani_linspace(start: float, stop: float, steps: int) -> tp.Tuple[float, ...]:
    """The end-point-excluding linspace of the published shifts (torchani_amd/constants.py: linspace)."""
    return tuple(start + ((stop - start) / steps) * j for j in range(steps))


class ConstSet(tp.NamedTuple):
    """One set of AEV constants; every float is an fp32 value held in a Python float, so that the engine, the oracle and
    the reference's from_constants see the same numbers."""
    name: str
    num_species: int
    Rcr: float
    Rca: float
    EtaR: float
    ShfR: tp.Tuple[float, ...]
    EtaA: float
    Zeta: float
    ShfA: tp.Tuple[float, ...]
    ShfZ: tp.Tuple[float, ...]
    cutoff_fn: str
    flags: int                                 # what anihip_aev_table_pack must give (bits 1 and 2)
    reaches: str
    near: tp.Optional[tp.Tuple[str, str]] = None   # boundary sets: (inequality group, "inside" | "outside")
    geoms: tp.Tuple[str, ...] = GEOMS
    long_row: bool = False                     # also on LONG_ROW_CASE
    vjp_reg: bool = True                       # the fp32 oracle's VJP stays under half of VJP_REG_REL: that gate applies

    @property
    def grid(self) -> tp.Tuple[int, int]:
        return len(self.ShfA), len(self.ShfZ)

    @property
    def out_dim(self) -> int:
        S = self.num_species
        return 16 * S + S * (S + 1) // 2 * 32

    def aev_constants(self):
        from torchani_amd.constants import AEVConstants

        return AEVConstants(self.num_species, self.Rcr, self.Rca, self.EtaR, self.ShfR, self.EtaA, self.Zeta, self.ShfA,
                            self.ShfZ, self.cutoff_fn)

    def oracle_params(self):
        from oracle import oracle as orc

        return orc.make_params(self.num_species, self.Rcr, self.Rca, self.EtaR, self.EtaA, self.Zeta, self.ShfR, self.ShfA,
                               self.ShfZ, self.cutoff_fn)


def make_set(name, S, Rcr, Rca, EtaR, ShfR, EtaA, Zeta, ShfA, ShfZ, cutoff_fn, flags, reaches, **kw) -> ConstSet:
    assert len(ShfR) == 16 and (len(ShfA), len(ShfZ)) in ((8, 4), (4, 8)), "tuned grid sizes only"
    return ConstSet(name, S, _f32(Rcr), _f32(Rca), _f32(EtaR), _f32s(ShfR), _f32(EtaA), _f32(Zeta), _f32s(ShfA), _f32s(ShfZ),
                    cutoff_fn, flags, reaches, **kw)


# ---- the admission inequalities, restated ----------------------------------------------------------------------------------

class Admission(tp.NamedTuple):
    fwd: float          # max(xm^2, 2 D xm): the flag needs < FWD_BOUND
    bwd_ang: float      # max((nA / 2) 2 D_A xa, (nA / 2)^2 D_A^2): < BWD_BOUND
    bwd_rad: float      # 2 D_R xr + 16 D_R^2: < BWD_BOUND
    uniform_a: bool     # ShfA equally spaced (to 1e-5 of the spacing, the tighter of the packer's two tests)
    uniform_r: bool

    @property
    def flags(self) -> int:
        fwd = self.uniform_a and self.fwd < FWD_BOUND
        bwd = self.uniform_a and self.uniform_r and self.bwd_ang < BWD_BOUND and self.bwd_rad < BWD_BOUND
        return (1 if fwd else 0) | (2 if bwd else 0)

    def of(self, group: str) -> tp.Tuple[float, float]:
        """(quantity, bound) of an inequality group."""
        return {"forward": (self.fwd, FWD_BOUND), "backward angular": (self.bwd_ang, BWD_BOUND),
                "backward radial": (self.bwd_rad, BWD_BOUND)}[group]


def _uniform(s: np.ndarray) -> bool:
    D = (s[-1] - s[0]) / (s.size - 1)
    return bool(D > 0 and np.all(np.abs((s - s[0]) - np.arange(s.size) * D) < 1e-5 * D))


def admission(c: ConstSet) -> Admission:
    """The three quantities of the module header in fp64 from the fp32 constants (nothing taken from the packer)."""
    shfa, shfr = np.asarray(c.ShfA, dtype=np.float64), np.asarray(c.ShfR, dtype=np.float64)
    na = shfa.size
    ca = na // 2 - 1
    qa, qr = math.sqrt(c.EtaA * LOG2E), math.sqrt(c.EtaR * LOG2E)
    xa = qa * max(abs(c.Rca - shfa[ca]), abs(shfa[ca]))
    D1 = qa * (shfa[1] - shfa[0])
    DA = qa * (shfa[-1] - shfa[0]) / (na - 1)
    DR = qr * (shfr[-1] - shfr[0]) / 15
    xr = qr * max(abs(c.Rcr - shfr[9]), abs(shfr[9]))
    return Admission(max(xa * xa, 2.0 * D1 * xa), max((na // 2) * 2.0 * DA * xa, (na // 2) ** 2 * DA * DA),
                     2.0 * DR * xr + 16.0 * DR * DR, _uniform(shfa), _uniform(shfr))


# ---- the table -------------------------------------------------------------------------------------------------------------

SHFR_2X = _ani_linspace(0.8, 5.1, 16)
SHFA_2X = _ani_linspace(0.8, 3.5, 8)
SHFZ_2X = _ani_linspace(math.pi / 8, math.pi + math.pi / 8, 4)
SHFR_1X = _ani_linspace(0.9, 5.2, 16)
SHFA_1X = _ani_linspace(0.9, 3.5, 4)
SHFZ_1X = _ani_linspace(math.pi / 16, math.pi + math.pi / 16, 8)
# the boundary values of EtaA / EtaR with the ANI-2x shifts and cutoffs (EtaA 12.5, EtaR 19.7 are the published ones):
# (group, last value that keeps the group's flag, first that clears it)
BOUNDARY_ETAS = {"backward angular": ("EtaA", 15.0, 16.0), "forward": ("EtaA", 21.0, 22.0),
                 "backward radial": ("EtaR", 26.0, 27.0)}


def _2x(name, S, flags, reaches, EtaR=19.7, EtaA=12.5, **kw) -> ConstSet:
    return make_set(name, S, 5.1, 3.5, EtaR, SHFR_2X, EtaA, 14.1, SHFA_2X, SHFZ_2X, "cosine", flags, reaches, **kw)


def _sets() -> tp.Tuple[ConstSet, ...]:
    out = [
        # -- boundary sets: ANI-2x shifts, one Eta moved to the edge of an admission inequality --
        _2x("bwd_ang_in", 4, 3, "EtaA 15: backward angular recurrence at 106 / 110, both recurrences run", EtaA=15.0,
            near=("backward angular", "inside"), long_row=True),
        _2x("bwd_ang_out", 3, 1, "EtaA 16: backward angular bound passed, direct Gaussians in the backward only", EtaA=16.0,
            near=("backward angular", "outside")),
        _2x("fwd_in", 5, 1, "EtaA 21: forward recurrence at 99.5 / 100 with equally spaced ShfA", EtaA=21.0,
            near=("forward", "inside")),
        _2x("fwd_out", 2, 0, "EtaA 22: forward bound passed with equally spaced shifts, every Gaussian direct", EtaA=22.0,
            near=("forward", "outside")),
        _2x("bwd_rad_in", 7, 3, "EtaR 26: backward radial recurrence at 108 / 110", EtaR=26.0,
            near=("backward radial", "inside"), long_row=True),
        _2x("bwd_rad_out", 6, 1, "EtaR 27: backward radial bound passed", EtaR=27.0, near=("backward radial", "outside")),
        # -- off-model sets --
        make_set("g48_zeta1", 3, 6.0, 4.0, 16.0, SHFR_1X, 4.0, 1.0, SHFA_1X, SHFZ_1X, "cosine", 3,
                 "4 x 8 grid, Zeta = 1 (exp2(0 log2|h|) in the backward), EtaA = 4, Rcr = 6.0, Rca = 4.0; odd species count"),
        _2x("g84_zeta64", 5, 3, "8 x 4 grid, Zeta = 64; odd species count: half-filled last radial slab; the fp32 oracle's "
            "VJP is 2.7e-6 off here, so the 5e-6 gate is not asked")._replace(Zeta=64.0, vjp_reg=False),
        make_set("rca_eq_rcr", 2, 4.0, 4.0, 19.7, _ani_linspace(0.8, 4.0, 16), 12.5, 14.1, _ani_linspace(0.8, 4.0, 8), SHFZ_2X,
                 "cosine", 1, "Rca = Rcr = 4.0: the far part of every row is empty; backward angular bound passed (115 / 110)"),
        _2x("shfz_bent", 6, 3, "ShfZ unequally spaced (the recurrences run over ShfA and ShfR only)")._replace(
            ShfZ=_f32s([z + (0.11 if k % 2 else -0.07) for k, z in enumerate(SHFZ_2X)])),
        make_set("shift_half", 1, 5.1, 3.5, 19.7, _ani_linspace(0.5, 5.1, 16), 12.5, 14.1, _ani_linspace(0.5, 3.5, 8), SHFZ_2X,
                 "cosine", 3, "shifts starting at 0.5 A (below the 0.75 A closest pair); one species"),
        make_set("g48_smooth", 4, 5.2, 3.5, 16.0, SHFR_1X, 8.0, 32.0, SHFA_1X, SHFZ_1X, "smooth", 3,
                 "smooth envelope on the 4 x 8 grid"),
        make_set("xr_cosine", 7, 5.2, 3.5, 19.7, _ani_linspace(0.9, 5.2, 16), 12.5, 14.1, _ani_linspace(0.9, 3.5, 8), SHFZ_2X,
                 "cosine", 3, "cosine envelope on the shifts of the 2xr (simple) set"),
    ]
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


SETS = _sets()
SET_NAMES = tuple(c.name for c in SETS)
BOUNDARY_NAMES = tuple(c.name for c in SETS if c.near is not None)
LONG_ROW_SETS = tuple(c.name for c in SETS if c.long_row)
SECOND_ORDER_SETS = ("bwd_ang_in", "g48_zeta1")   # backward_second: one boundary set and the Zeta = 1 set
PUSHED_SETS = ("bwd_ang_in", "bwd_rad_in")        # rows that are not symmetric (rows_from_full)
# tests/golden/tuned_<set>.npz: the reference's own numbers for (set, geometry)
GOLDEN_RUNS = (("bwd_ang_in", "mol10"), ("g48_zeta1", "mol10"), ("rca_eq_rcr", "pbc16"))


def set_by_name(name: str) -> ConstSet:
    for c in SETS + sweep_sets():
        if c.name == name:
            return c
    raise KeyError(name)


# ---- the random sweep ------------------------------------------------------------------------------------------------------

SWEEP_SEED = 0
SWEEP_TRIALS = 24


class Trial(tp.NamedTuple):
    cset: ConstSet
    geom: str      # a name geometry() understands


def _draw_sweep(seed: int) -> tp.Tuple[Trial, ...]:
    rs = np.random.RandomState(seed)
    out = []
    for k in range(SWEEP_TRIALS):
        S = int(rs.randint(1, 8))
        na, nz = ((8, 4), (4, 8))[int(rs.randint(0, 2))]
        Rcr = float(rs.uniform(4.0, 6.0))
        Rca = float(rs.uniform(2.5, Rcr))
        EtaR, EtaA = float(rs.uniform(4.0, 40.0)), float(rs.uniform(4.0, 24.0))
        Zeta = float(rs.choice([1.0, 8.0, 14.1, 32.0]))
        ShfR = np.linspace(rs.uniform(0.5, 1.0), Rcr - rs.uniform(0.2, 0.6), 16)
        ShfA = np.linspace(rs.uniform(0.5, 1.0), Rca - rs.uniform(0.2, 0.6), na)
        ShfZ = (np.arange(nz) + 0.5) * np.pi / nz
        cut = "smooth" if rs.rand() < 0.4 else "cosine"
        kind = ("cluster", "pbc", "batch")[int(rs.randint(0, 3))]
        atoms = int(rs.choice([2, 30, 40])) if kind == "cluster" else (60 if kind == "pbc" else 14)
        c = make_set(f"sweep{k:02d}", S, Rcr, Rca, EtaR, ShfR, EtaA, Zeta, ShfA, ShfZ, cut, 0, "random sweep")
        c = c._replace(flags=admission(c).flags, reaches=f"random sweep, trial {k}: {na} x {nz}, S = {S}, {cut}")
        out.append(Trial(c, f"{kind}:{atoms}:{1000 + k}"))
    return tuple(out)


@functools.lru_cache(maxsize=1)
def sweep() -> tp.Tuple[Trial, ...]:
    """24 seeded trials shaped like test_general_grids_random_sweep of tests/test_gpu_parity.py: EtaR 4 .. 40, EtaA 4 .. 24,
    Zeta of {1, 8, 14.1, 32}, Rcr 4 .. 6, Rca 2.5 .. Rcr, the first shift 0.5 .. 1.0 A and the last 0.2 .. 0.6 A inside its
    cutoff, 1 .. 7 species, both grids, both envelopes; a cluster of 2, 30 or 40 atoms, a 60-atom periodic box or a padded
    3 x 14 batch.  SWEEP_SEED is the first seed from 0 on with which each of the flag values 0, 1 and 3 occurs at least four
    times (tests/test_aev_constants_host.py::test_sweep_flag_counts)."""
    return _draw_sweep(SWEEP_SEED)


def sweep_sets() -> tp.Tuple[ConstSet, ...]:
    return tuple(t.cset for t in sweep())


def flag_counts(trials: tp.Sequence[Trial]) -> tp.Dict[int, int]:
    out = {0: 0, 1: 0, 2: 0, 3: 0}
    for t in trials:
        out[t.cset.flags] += 1
    return out


def first_good_seed() -> int:
    seed = 0
    while True:
        n = flag_counts(_draw_sweep(seed))
        if min(n[0], n[1], n[3]) >= 4:
            return seed
        seed += 1


# ---- geometries ------------------------------------------------------------------------------------------------------------

class Geom(tp.NamedTuple):
    name: str
    species: np.ndarray                    # [C, A] int32, -1 = padding
    coords: np.ndarray                     # [C, A, 3] float32
    cell: tp.Optional[np.ndarray]
    pbc: tp.Optional[tp.Tuple[bool, bool, bool]]

    @property
    def n_atoms(self) -> int:
        return int(self.species.size)

    @property
    def periodic(self) -> bool:
        return self.cell is not None

    def molecule(self, m: int) -> ac.AevCase:
        return ac.AevCase(f"{self.name}[{m}]", self.species[m:m + 1], self.coords[m:m + 1], self.cell, self.pbc, 7)


TRIC_CELL = nc._cell([[9.2, 0, 0], [1.1, 9.6, 0], [-0.7, 0.9, 10.1]])


def _spread(rs, n: int, box: float, cell: tp.Optional[np.ndarray] = None) -> np.ndarray:
    """n points, uniform in a cube of edge `box` (or in `cell`), no two closer than MIN_DIST (images included)."""
    pts: tp.List[np.ndarray] = []
    shifts = np.zeros((1, 3))
    if cell is not None:
        k = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
        shifts = k.astype(np.float64) @ cell.astype(np.float64)
    while len(pts) < n:
        q = rs.uniform(0.0, box, 3) if cell is None else rs.uniform(0.0, 1.0, 3) @ cell.astype(np.float64)
        if all(np.linalg.norm(q + shifts - p, axis=1).min() > MIN_DIST + 1e-3 for p in pts):
            pts.append(q)
    return np.asarray(pts)


GOLD_CELL = nc._cell([[8.4, 0, 0], [0.6, 8.8, 0], [0.3, -0.5, 9.1]])
# name: (kind, atoms, seed, cube edge, cell)
GEOM_SPECS = {"cluster40": ("cluster", 40, 11, 4.6, None), "tric60": ("pbc", 60, 12, 0.0, TRIC_CELL),
              "batch3x14": ("batch", 14, 13, 3.5, None),
              # the fixtures of tests/golden/gen_golden_tuned_constants.py (small: a fixture holds whole fp64 rows)
              "mol10": ("cluster", 10, 14, 2.8, None), "pbc16": ("pbc", 16, 15, 0.0, GOLD_CELL)}


@functools.lru_cache(maxsize=None)
def geometry(name: str, num_species: int) -> Geom:
    """cluster40: 40 atoms in a 4.6 A cube, open; tric60: 60 atoms in the triclinic TRIC_CELL (9.2 x 9.6 x 10.1 A: smaller
    than twice the cutoffs, so rows hold several images of the cell), periodic; batch3x14: three 14-atom molecules in 3.5 A
    cubes, the second with three padding atoms; mol10, pbc16: 10 atoms in a 2.8 A cube, 16 in GOLD_CELL (at least twice
    every cutoff it is used with).  No two atoms closer than 0.75 A; the species are seeded per species count.
    "<kind>:<atoms>:<seed>": the sweep's own (cluster, pbc or batch)."""
    kind, atoms, seed, box, cell = GEOM_SPECS.get(name) or _sweep_geom(name)
    rs = np.random.RandomState(seed)
    C = 3 if kind == "batch" else 1
    x = np.stack([_spread(rs, atoms, box, cell) for _ in range(C)]).astype(np.float32)
    sp = np.random.RandomState(100 * seed + num_species).randint(0, num_species, (C, atoms)).astype(np.int32)
    if kind == "batch":
        sp[1, atoms - 3:] = -1
    return Geom(name, sp, x, cell, (True, True, True) if kind == "pbc" else None)


def _sweep_geom(name: str):
    kind, atoms, seed = name.split(":")
    rs = np.random.RandomState(int(seed))
    box = float(rs.uniform(3.5, 5.5)) if int(atoms) > 2 else 1.6
    return kind, int(atoms), int(seed), (3.5 if kind == "batch" else box), (TRIC_CELL if kind == "pbc" else None)


def long_row_geometry() -> Geom:
    c = ac.case_by_name(LONG_ROW_CASE)
    return Geom(LONG_ROW_CASE, c.species.astype(np.int32), c.coords, c.cell, c.pbc)


def runs() -> tp.Tuple[tp.Tuple[str, str], ...]:
    """(set, geometry) of the table."""
    out = [(c.name, g) for c in SETS for g in c.geoms]
    out += [(c.name, LONG_ROW_CASE) for c in SETS if c.long_row]
    return tuple(out)


def sweep_runs() -> tp.Tuple[tp.Tuple[str, str], ...]:
    return tuple((t.cset.name, t.geom) for t in sweep())


def geometry_of(run: tp.Tuple[str, str]) -> Geom:
    cset = set_by_name(run[0])
    if run[1] == LONG_ROW_CASE:
        g = long_row_geometry()
        assert int(g.species.max()) < cset.num_species
        return g
    return geometry(run[1], cset.num_species)


def run_id(run) -> str:
    return f"{run[0]}-{run[1].replace(':', '_').replace('/', '_')}"


def displaced(geom: Geom, seed: int = 19, step: float = 0.05) -> np.ndarray:
    """The coordinates with a third of the atoms (every third) moved by a seeded displacement of at most `step` A."""
    rs = np.random.RandomState(seed)
    n = geom.n_atoms
    v = rs.normal(size=(n, 3))
    v *= (step * rs.uniform(0.0, 1.0, n) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]
    v[np.arange(n) % 3 != 0] = 0.0
    return (geom.coords.astype(np.float64) + v.reshape(geom.coords.shape)).astype(np.float32)


def central_range(geom: Geom) -> tp.Tuple[int, int]:
    """A range of central atoms strictly inside the system."""
    n = geom.n_atoms
    return n // 3, max(2 * n // 3, n // 3 + 1)


# ---- rows ------------------------------------------------------------------------------------------------------------------

def row_stats(geom: Geom, cset: ConstSet, coords: tp.Optional[np.ndarray] = None, margin: float = 0.0) -> ac.RowStats:
    """_aev_cases.row_stats molecule by molecule, under the set's cutoffs (padding atoms: empty rows)."""
    parts = []
    for m in range(geom.species.shape[0]):
        mol = geom.molecule(m)
        parts.append(ac.row_stats(mol, cset.num_species, cset.Rcr, cset.Rca,
                                  coords=None if coords is None else coords[m:m + 1], margin=margin))
    return ac.RowStats(*[np.concatenate([getattr(p, f) for p in parts]) for f in ("rad", "ang", "cnt_a", "cnt_f")],
                       sum(p.banded for p in parts))


def closest_pair(geom: Geom) -> float:
    out = np.inf
    for m in range(geom.species.shape[0]):
        mol = geom.molecule(m)
        _, _, _, r = nc.numpy_pairs(nc.NbrCase(mol.name, mol.species, mol.coords, mol.cell, mol.pbc, ()), 2.0)
        out = min(out, float(r.min()) if r.size else np.inf)
    return out


def reach(geom: Geom, cset: ConstSet) -> Admission:
    """The admission quantities with the distances the geometry really has in place of the worst case 0 .. Rc: the largest
    exponents the recurrences (would) meet on it.  Below admission(cset) by what no geometry reaches: pairs closer than
    MIN_DIST, and pairs at the cutoff itself."""
    shfa, shfr = np.asarray(cset.ShfA, dtype=np.float64), np.asarray(cset.ShfR, dtype=np.float64)
    na = shfa.size
    qa, qr = math.sqrt(cset.EtaA * LOG2E), math.sqrt(cset.EtaR * LOG2E)
    D1 = qa * (shfa[1] - shfa[0])
    DA = qa * (shfa[-1] - shfa[0]) / (na - 1)
    DR = qr * (shfr[-1] - shfr[0]) / 15
    xa = xr = 0.0
    for m in range(geom.species.shape[0]):
        mol = geom.molecule(m)
        i, _, _, r = nc.numpy_pairs(nc.NbrCase(mol.name, mol.species, mol.coords, mol.cell, mol.pbc, ()), cset.Rcr)
        if r.size:
            xr = max(xr, float(qr * np.abs(r - shfr[9]).max()))
        for c in np.unique(i):
            ra = np.sort(r[(i == c) & (r <= cset.Rca)])
            if ra.size >= 2:   # the mean distances of the row's pairs span (ra[0] + ra[1]) / 2 .. (ra[-2] + ra[-1]) / 2
                ends = np.array([ra[0] + ra[1], ra[-2] + ra[-1]]) / 2.0
                xa = max(xa, float(qa * np.abs(ends - shfa[na // 2 - 1]).max()))
    return Admission(max(xa * xa, 2.0 * D1 * xa), max((na // 2) * 2.0 * DA * xa, (na // 2) ** 2 * DA * DA),
                     2.0 * DR * xr + 16.0 * DR * DR, _uniform(shfa), _uniform(shfr))


def full_list(geom: Geom):
    """A LAMMPS-style full list of an open one-molecule geometry: every atom lists every other atom (the row builder screens
    them by distance): (ilist, jlist, numneigh) int32."""
    assert geom.species.shape[0] == 1 and not geom.periodic
    n = geom.n_atoms
    ilist = np.arange(n, dtype=np.int32)
    jlist = np.concatenate([np.delete(ilist, i) for i in range(n)]).astype(np.int32)
    return ilist, jlist, np.full(n, n - 1, dtype=np.int32)


# ---- references ------------------------------------------------------------------------------------------------------------

class Ref(tp.NamedTuple):
    aev: np.ndarray      # [N, L]
    w: np.ndarray        # [N, L] float32: the cotangent
    vjp: np.ndarray      # [N, 3]
    virial: np.ndarray   # [3, 3]
    t: np.ndarray        # [N, 3]: the direction
    jvp: np.ndarray      # [N, L]


@functools.lru_cache(maxsize=2)
def _oracle(kind: str):
    from oracle.oracle import Oracle

    return Oracle(kind)


def cotangent(geom: Geom, cset: ConstSet) -> np.ndarray:
    return np.random.RandomState(1000).uniform(-1.0, 1.0, (geom.n_atoms, cset.out_dim)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(run: tp.Tuple[str, str], kind: str = "f64", x_key: tp.Optional[str] = None) -> Ref:
    """The oracle (kind "f64": the reference; "f32": the same sums rounded to fp32) on a run: AEV rows, the VJP of the seeded
    cotangent with its virial, and J t along tests/_util.fgrad_direction.  x_key "displaced": at displaced(geom)."""
    from _util import fgrad_direction

    cset, geom = set_by_name(run[0]), geometry_of(run)
    p = cset.oracle_params()
    n = geom.n_atoms
    w = cotangent(geom, cset)
    t = fgrad_direction(geom.species)
    x64 = (displaced(geom) if x_key == "displaced" else geom.coords).astype(np.float64)
    o = _oracle(kind)
    aev, vjp, vir = o.aev(p, geom.species, x64, geom.cell, geom.pbc, grad_aev=w.astype(np.float64), want_virial=True)
    _, jt = o.aev_jvp(p, geom.species, x64, t, geom.cell, geom.pbc)
    return Ref(aev.reshape(n, -1).astype(np.float64), w, vjp.reshape(n, 3).astype(np.float64), np.asarray(vir, dtype=np.float64),
               t.reshape(n, 3), jt.reshape(n, -1).astype(np.float64))


class Second(tp.NamedTuple):
    t: np.ndarray        # [K, N, 3] float32: the directions
    dgrad: np.ndarray    # [K, N, L] float32
    curv: np.ndarray     # [K, N, 3]: (D_t J^T) w, Richardson central difference of the oracle's VJP
    spread: np.ndarray   # [K]: largest |D(h) - D(2h)|
    lin: np.ndarray      # [K, N, 3]: J^T dgrad[k]
    h: np.ndarray        # [K]


@functools.lru_cache(maxsize=None)
def second_reference(run: tp.Tuple[str, str]) -> Second:
    """out[k] = J^T dgrad[k] + (D_{t[k]} J^T) w of AevEngine.backward_second along three directions (tests/_util's
    fgrad_direction, a unit vector on the atom with the longest row, a seeded sign vector), from tests/_second_order_ref.py:
    fd_until takes the first step whose spread is below a hundredth of the gate."""
    import _second_order_ref as so
    from _util import fgrad_direction

    cset, geom = set_by_name(run[0]), geometry_of(run)
    assert geom.species.shape[0] == 1
    p = cset.oracle_params()
    n = geom.n_atoms
    w = cotangent(geom, cset).astype(np.float64)
    x = geom.coords.astype(np.float64)
    o = _oracle("f64")

    def vjp(cot, xx):
        return o.aev(p, geom.species, xx, geom.cell, geom.pbc, grad_aev=cot)[1].reshape(n, 3)

    t = np.zeros((3, n, 3))
    t[0] = fgrad_direction(geom.species)[0]
    t[1, int(np.argmax(row_stats(geom, cset).rad)), 2] = 1.0
    t[2] = np.random.RandomState(1004).choice([-1.0, 1.0], (n, 3))
    dgrad = np.random.RandomState(1001).uniform(-1.0, 1.0, (3, n, cset.out_dim)).astype(np.float32)
    lin = [vjp(dgrad[k].astype(np.float64), x) for k in range(3)]
    fds = [so.fd_until(lambda h, k=k: vjp(w, x + h * t[k][None]), so.second_ok(lin[k])) for k in range(3)]
    return Second(t.astype(np.float32), dgrad, np.stack([f.value for f in fds]), np.array([f.spread.max() for f in fds]),
                  np.stack(lin), np.array([f.h for f in fds]))
