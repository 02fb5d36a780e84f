"""Cases, potentials and gates of the pair-virial tests (numpy only).

The virial W = dE / d(strain) [3, 3] of a pair potential is what constant-pressure dynamics, pressures() and the ASE stress
consume.  tests/golden/gen_golden_pair_virials.py evaluates it with the reference's own classes in fp64 on the cases below,
tests/test_pair_virials_host.py proves on the CPU that the fixtures and the gates tell a wrong kernel from a right one, and
tests/test_gpu_pair_virials.py holds k_pair<KIND>, k_d3_pair + k_d3_cngrad and the ANI-2xr / ANI-2dr sums to them.

Inputs are loaded by name from where they already live; only the two own-image cells are defined here.

  case                 atoms  pbc  why
  water_pbc_ani2x         30  TTT  the fixture every other pair test uses; D3's 8 A cutoff equals the cell edge
  water_ttf               30  TTF  the same coordinates, partial periodicity on the same rows
  triclinic_pbc_ani2x     20  TTF  off-diagonal cell; large repulsive terms that cancel
  chunk129_pbc/built     130  TTT  rows of 129 entries at 8 A: the second pass of the ``k += WAVE`` lane loops
  own4                     4  TTT  a cell smaller than every cutoff: a quarter of the pairs are an atom and its own image;
                                   D3 with a 7.5 A cutoff here (d3_r75): at 8 A its rows would hold 284 to 286 entries, and
                                   a neighbor row holds 256 -- the engine refuses that, which the GPU test asserts as well
  own1                     1  TTT  one atom in a skewed 2.3 to 2.6 A cell: the forces are zero, W is own images alone

Gates.  |W - W_ref|max <= rel x A with A = sum over pairs of |dE / d d_p| |d_p| (the sum without cancellation, stored with
every fixture).  rel per family = 4 x the largest error of the REFERENCE's own float32 evaluation over the counted cases,
rounded up to one digit, and capped by the relative force gate the same loop is already held to
(profiles/pair_virial_tests.txt has the numbers).  A (potential, case) counts when max |W_ref| >= 100 x its gate; the
others are listed in EXCLUDED with the reason.
"""
from __future__ import annotations

import os
import typing as tp

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ANI2X_SYMBOLS = ("H", "C", "N", "O", "S", "F", "Cl")

OWN4_CELL = ((3.1, 0.0, 0.0), (0.4, 3.3, 0.0), (0.2, -0.3, 3.0))
OWN4_FRAC = ((0.1, 0.1, 0.1), (0.55, 0.45, 0.2), (0.3, 0.8, 0.6), (0.8, 0.2, 0.75))
OWN4_SPECIES = (3, 0, 0, 1)   # O H H C
OWN1_CELL = ((2.4, 0.0, 0.0), (0.5, 2.3, 0.0), (0.3, -0.6, 2.5))
OWN1_FRAC = ((0.1, 0.1, 0.1),)
OWN1_SPECIES = (3,)


class PairVirialCase(tp.NamedTuple):
    name: str
    symbols: tp.Tuple[str, ...]
    species: np.ndarray                    # [1, N] int64, indices into symbols
    coords: np.ndarray                     # [1, N, 3] float32
    cell: np.ndarray                       # [3, 3] float32
    pbc: tp.Tuple[bool, bool, bool]

    @property
    def n_atoms(self) -> int:
        return int(self.species.shape[1])

    @property
    def file_name(self) -> str:
        return self.name.replace("/", "_")


def _golden(name, pbc=None, rename=None):
    with np.load(os.path.join(GOLDEN_DIR, name + ".npz")) as z:
        sym = tuple(str(s) for s in z["symbols"])
        return PairVirialCase(rename or name, sym, z["species"].astype(np.int64), z["coords"].astype(np.float32),
                              z["cell"].astype(np.float32), tuple(bool(b) for b in (z["pbc"] if pbc is None else pbc)))


def _long_row(name):
    import _aev_cases as ac

    c = ac.case_by_name(name)
    return PairVirialCase(name, ANI2X_SYMBOLS, c.species.astype(np.int64), c.coords.astype(np.float32),
                          np.asarray(c.cell, dtype=np.float32), tuple(bool(b) for b in c.pbc))


def _own(name, cell, frac, species):
    cell = np.asarray(cell, dtype=np.float32)
    x = (np.asarray(frac, dtype=np.float64) @ cell.astype(np.float64)).astype(np.float32)
    return PairVirialCase(name, ANI2X_SYMBOLS, np.asarray([species], dtype=np.int64), x[None], cell, (True, True, True))


_BUILDERS: tp.Dict[str, tp.Callable[[], PairVirialCase]] = {
    "water_pbc_ani2x": lambda: _golden("water_pbc_ani2x"),
    "water_ttf": lambda: _golden("water_pbc_ani2x", pbc=(True, True, False), rename="water_ttf"),
    "triclinic_pbc_ani2x": lambda: _golden("triclinic_pbc_ani2x"),
    "chunk129_pbc/built": lambda: _long_row("chunk129_pbc/built"),
    "own4": lambda: _own("own4", OWN4_CELL, OWN4_FRAC, OWN4_SPECIES),
    "own1": lambda: _own("own1", OWN1_CELL, OWN1_FRAC, OWN1_SPECIES),
}
CASE_NAMES = tuple(_BUILDERS)
OWN_IMAGE_CASES = ("own4", "own1", "triclinic_pbc_ani2x")   # cases with pairs (i, i): the "own images dropped" mutation
_cache: tp.Dict[str, PairVirialCase] = {}


def case_by_name(name: str) -> PairVirialCase:
    if name not in _cache:
        _cache[name] = _BUILDERS[name]()
    return _cache[name]


# ---- potentials: key -> family; the constructor arguments are those of gen_golden_pairs2.cases / the older fixtures -----
ANALYTIC_KEYS = ("zbl", "zbl_cos", "lj", "lj_rep", "lj_disp", "coulomb", "mnok")
FAMILY = dict({k: "analytic" for k in ANALYTIC_KEYS}, xtb="xtb", xtb_cos="xtb", d3="d3", d3_b973c="d3", d3_r75="d3")
XTB_KW = {"xtb": dict(cutoff=5.2, cutoff_fn="smooth"), "xtb_cos": dict(cutoff=5.1, cutoff_fn="cosine")}
D3_KW = {"d3": dict(functional="wb97x", cutoff=8.0, cutoff_fn="smooth"),
         "d3_b973c": dict(functional="b973c", cutoff=8.0, cutoff_fn="smooth"),
         "d3_r75": dict(functional="wb97x", cutoff=7.5, cutoff_fn="smooth")}   # own4: rows of 222 to 227 entries
OWN4_D3_CUTOFF = 7.5   # also the cutoff of ANI-2dr's dispersion term on own4 (8 A everywhere else)


def keys_of(case_name: str) -> tp.Tuple[str, ...]:
    extra = case_name == "water_pbc_ani2x"
    return (("xtb",) + (("xtb_cos",) if extra else ()) + ANALYTIC_KEYS + (d3_key_of(case_name),)
            + (("d3_b973c",) if extra else ()))


def d3_key_of(case_name: str) -> str:
    return "d3_r75" if case_name == "own4" else "d3"


# element constants of tests/golden/gen_golden_pairs2.py, which loads the reference on import and so cannot be imported by
# a test: the generator and tests/test_pair_virials_host.py (from that file's text) assert that the copies are the same
CHARGES = {"H": 0.35, "C": -0.15, "N": -0.45, "O": -0.70, "S": -0.20, "F": -0.25, "Cl": -0.10}
ETA = {"H": 0.47, "C": 0.37, "N": 0.53, "O": 0.45, "S": 0.30, "F": 0.52, "Cl": 0.34}
EPS = {"H": 2.5e-5, "C": 1.4e-4, "N": 2.7e-4, "O": 3.3e-4, "S": 4.0e-4, "F": 1.0e-4, "Cl": 4.2e-4}
SIGMA = {"H": 1.49, "C": 1.91, "N": 1.82, "O": 1.66, "S": 1.98, "F": 1.75, "Cl": 1.95}


def analytic_kwargs(symbols: tp.Sequence[str]) -> tp.Dict[str, tp.Tuple[str, dict]]:
    """key -> (class name, keyword arguments): the same for the reference's classes and for torchani_amd.potentials."""
    q = tuple(CHARGES[s] for s in symbols)
    return {
        "zbl": ("RepulsionZBL", dict(cutoff=5.2, cutoff_fn="smooth")),
        "zbl_cos": ("RepulsionZBL", dict(k=0.4685, cutoff=4.0, cutoff_fn="cosine")),
        "lj": ("LennardJones", dict(eps=tuple(EPS[s] for s in symbols), sigma=tuple(SIGMA[s] for s in symbols), cutoff=7.5,
                                    cutoff_fn="smooth")),
        "lj_rep": ("RepulsionLJ", dict(cutoff=5.2, cutoff_fn="smooth")),
        "lj_disp": ("DispersionLJ", dict(cutoff=7.5, cutoff_fn="smooth")),
        "coulomb": ("FixedCoulomb", dict(charges=q, dielectric=1.3, cutoff=7.5, cutoff_fn="smooth")),
        "mnok": ("FixedMNOK", dict(charges=q, eta=tuple(ETA[s] for s in symbols), cutoff=7.5, cutoff_fn="smooth")),
    }


# ---- gates ---------------------------------------------------------------------------------------------------------------
# The reference's float32 evaluation is off by at most 1.74e-6 A (xtb, triclinic_pbc_ani2x), 7.37e-6 A (lj,
# triclinic_pbc_ani2x: one pair at 0.9 sigma) and 1.91e-5 A (d3, chunk129_pbc/built: the Gaussian reference weights amplify
# the rounding of the coordination numbers).  4 x that is 7e-6, 3e-5 and 8e-5: every family is held to its CAP, the relative
# force gate of the same loop.  The host test recomputes all this from the fixtures.
GATE_CAP = {"xtb": 5e-6, "analytic": 1e-5, "d3": 2e-5}
GATE_REL = {"xtb": 5e-6, "analytic": 1e-5, "d3": 2e-5}
# (potential key, case) below 100 x its gate: none -- every potential counts on every case, own1's cell included
EXCLUDED: tp.Dict[tp.Tuple[str, str], str] = {}


def gate_from_f32(worst: float, cap: float) -> float:
    """4 x worst rounded UP to one significant digit, at most cap."""
    v = 4.0 * worst
    e = int(np.floor(np.log10(v)))
    m = int(np.ceil(v / 10.0 ** e - 1e-9))
    return min(cap, m * 10.0 ** e)


def load_virials(case_name: str) -> tp.Dict[str, np.ndarray]:
    with np.load(os.path.join(GOLDEN_DIR, f"pairs_virial_{case_by_name(case_name).file_name}.npz")) as z:
        return {k: z[k] for k in z.files}


# ---- the ANI-2xr family ---------------------------------------------------------------------------------------------------
# (kind, case, seed); water_pbc_ani2x carries the seed of tests/golden/x2r_<kind>_water_pbc_ani2x.npz, whose energies and
# forces the new files must repeat.  ANI-r2s has no periodic case: its repulsion has no cutoff, which neither the reference's
# neighbor list nor the engine's rows accept together with a cell.
MODEL_CASES = tuple((kind, case, seed) for kind in ("ani2xr", "ani2dr")
                    for case, seed in (("water_pbc_ani2x", 22), ("water_ttf", 26), ("triclinic_pbc_ani2x", 27), ("own4", 28)))
MODEL_PAIR_TERMS = {"ani2xr": (("repulsion_xtb", "xtb"),), "ani2dr": (("repulsion_xtb", "xtb"), ("dispersion_d3", "d3"))}
NETWORK_VIRIAL_TOL = 1e-4   # x max(1, max |W_ref|) Ha: VIRIAL_TOL of tests/test_gpu_aev_long_rows.py


def load_model_virials(kind: str, case_name: str) -> tp.Dict[str, np.ndarray]:
    with np.load(os.path.join(GOLDEN_DIR, f"x2r_virial_{kind}_{case_by_name(case_name).file_name}.npz")) as z:
        return {k: z[k] for k in z.files}
