"""The neighbor-builder sweep of tests/_nbr_cases.py on the CPU: the fp64 oracle's brute-force list, the reference that
tests/test_gpu_neighbors.py holds the HIP builders to, is itself held to the oracle's cell list, to a plain numpy enumeration
of the periodic images, and to the reference's AllPairs (per-atom counts and distance sums, tests/golden/nbrsweep_*.npz from
gen_golden_nbr_sweep.py).  The generator's own promises are asserted from the oracle alone: the borderline band's share, the
margins of the shell families, which of the two cell kernels a case must reach."""
import os

import numpy as np
import pytest

import _nbr_cases as nc
from _nbr_rows import IMG_SPAN, pair_keys

CASES = nc.all_cases()
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def oracle_list(oracle64, case, cutoff, cell_list=False):
    return oracle64.neighbors(case.species, case.coords.astype(np.float64), cutoff, case.cell, case.pbc,
                              cell_list=cell_list)


def list_keys(case, lst):
    start, j, d, _ = lst
    n = case.n_atoms
    i = np.repeat(np.arange(n), np.diff(start))
    cell = case.cell.astype(np.float64) if case.periodic else None
    return pair_keys(i, j.astype(np.int64), d.astype(np.float64), nc.wrap_f64(case), cell, n)[0]


def row_stats(case, lst):
    """Per atom: neighbors, neighbors within Rca, and the largest per-species count of either group."""
    start, j, _, r = lst
    n = case.n_atoms
    i = np.repeat(np.arange(n), np.diff(start))
    sp = case.species.reshape(-1)[j]
    cls = np.zeros((n, 2, nc.NUM_SPECIES), dtype=np.int64)
    np.add.at(cls, (i, (r > case.rca).astype(np.int64), sp), 1)
    return np.diff(start), cls[:, 0].sum(axis=1), cls.max(axis=(1, 2))


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_oracle_lists_agree(oracle64, case):
    """Brute force == cell list == plain numpy enumeration, as sets of (i, j, image)."""
    brute = list_keys(case, oracle_list(oracle64, case, case.rcr))
    assert np.unique(brute).size == brute.size
    binned = list_keys(case, oracle_list(oracle64, case, case.rcr, cell_list=True))
    assert np.array_equal(np.sort(brute), np.sort(binned)), f"{case.name}: the oracle's two lists differ"
    if case.n_atoms <= nc.BATCH_MAX_ATOMS:
        i, j, img, _ = nc.numpy_pairs(case, case.rcr)
        key = i.astype(np.int64) * case.n_atoms + j
        for q in range(3):
            key = key * IMG_SPAN + (img[:, q] + IMG_SPAN // 2)
        assert np.array_equal(np.sort(brute), np.sort(key)), f"{case.name}: oracle {brute.size} pairs, numpy {key.size}"


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_conditions(oracle64, case):
    lst = oracle_list(oracle64, case, case.rcr + nc.BAND)
    r = lst[3]
    inside = r <= case.rcr
    banded = int((np.abs(r - case.rcr) <= nc.BAND).sum() + (np.abs(r - case.rca) <= nc.BAND).sum())
    assert banded <= nc.BAND_SHARE * max(int(inside.sum()), 1), f"{case.name}: {banded} of {int(inside.sum())} pairs in the band"
    start, j, d, _ = lst
    keep = np.repeat(np.arange(case.n_atoms), np.diff(start))[inside]
    exact = (np.concatenate([[0], np.cumsum(np.bincount(keep, minlength=case.n_atoms))]), j[inside], d[inside], r[inside])
    rows, ang, per_species = row_stats(case, exact)
    pad = case.species.reshape(-1) < 0
    assert np.all(rows[pad] == 0)
    if case.centre is None:
        # prototypes of the random cases: rows up to 133 (droplet), 55 within Rca, 40 of one species
        assert rows.max() <= case.row_cap and ang.max() <= nc.MAX_ANG and per_species.max() <= nc.MAX_PER_SPECIES
    else:
        cap, amax, smax = case.limits
        others = np.arange(case.n_atoms) != case.centre
        assert rows[others].max() <= cap - 8 and ang[others].max() <= amax - 8 and per_species[others].max() <= smax - 8
        c = case.centre
        rc = r[inside][keep == c]
        # (0.5 A nominally -- the 3.0 A shell -- less the fp32 rounding of coordinates near 30 A)
        assert np.all(np.abs(rc - case.rcr) >= 0.5 - 1e-5) and np.all(np.abs(rc - case.rca) >= 0.5 - 1e-5)
        over = rows[c] > cap or ang[c] > amax or per_species[c] > smax
        assert over == (case.overflow_rows == (c,))
        if over:
            assert max(rows[c] - cap, ang[c] - amax, per_species[c] - smax) == 1, "one over the limit, no more"
        elif case.name.startswith(("cap64", "ang128", "spec255", "rad256")):
            assert rows[c] == cap or ang[c] == amax or per_species[c] == smax, "exactly at the limit"
    nb, stencil, occupied, left = nc.grid_model(case)
    if case.kernel == "bin":
        assert left == 0
    elif case.kernel == "atom":
        assert left == occupied == int(np.prod(nb))
    elif case.kernel == "both":
        assert 0 < left < int(np.prod(nb))
    if case.coarsened:
        assert int(np.prod(nc.grid_model(case, max_cells=1 << 29)[0])) > case.max_cells


@pytest.mark.parametrize("name", nc.GOLDEN_CASES)
def test_oracle_matches_reference_all_pairs(oracle64, name):
    """Per-atom neighbor counts and sums of neighbor distances of the reference's AllPairs on the same fp32 coordinates."""
    case = nc.case_by_name(name)
    with np.load(os.path.join(GOLDEN_DIR, f"nbrsweep_{case.golden}.npz")) as z:
        g = {k: z[k] for k in z.files}
    assert g["count"].shape == (case.n_atoms,), "the fixture is of another case: rerun tests/golden/gen_golden_nbr_sweep.py"
    start, _, _, r = oracle_list(oracle64, case, case.rcr)
    cnt = np.diff(start)
    assert np.array_equal(cnt, g["count"].astype(np.int64)), f"{name}: per-atom neighbor counts differ from AllPairs"
    i = np.repeat(np.arange(case.n_atoms), cnt)
    sums = np.bincount(i, weights=r, minlength=case.n_atoms)
    assert np.all(np.abs(sums - g["dist_sum"]) <= 1e-9 * np.maximum(cnt, 1)), np.abs(sums - g["dist_sum"]).max()
