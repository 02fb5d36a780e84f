"""The references of tests/test_gpu_second_order_long_rows.py on the CPU: how long the rows of the existing second-order
fixtures are (the gap the long-row cases close), that every finite-difference reference of tests/_second_order_ref.py has
converged to a hundredth of the gate it is used with, which case reaches which long-row path of the second-order kernels, and
that the references reproduce fixtures of the reference project (one Hessian, one set of strain derivatives -- the latter
also proves the index convention of out and ss)."""
import os

import numpy as np
import pytest

import _aev_cases as ac
import _second_order_ref as so
from _util import GOLDEN_DIR, load_golden

RUN_IDS = [so.run_id(r) for r in so.RUNS]
HESSIAN_FIXTURES = ("ch4_ani1x", "rand_batch_ani2x", "water_pbc_ani2x", "water_pbc_smooth_ani2x", "triclinic_pbc_ani2x",
                    "small_ani2x", "dense90_ani2x")
PAIR_HESSIAN_BASES = ("rand_batch_ani2x", "water_pbc_ani2x", "triclinic_pbc_ani2x")   # tests/golden/hess_pairs_*.npz
PAIR_CUTOFFS = (4.0, 5.2, 7.5)   # the cutoffs of tests/golden/gen_golden_pairs2.py: cases
# longest row within 5.2 / 7.5 / 8.0 A (AEV and short pair cutoffs / long pair cutoffs / D3)
EXPECTED_ROWS = {
    "ch4_ani1x": (4,), "rand_batch_ani2x": (13,), "water_pbc_ani2x": (41, 116, 148), "water_pbc_smooth_ani2x": (41, 116, 148),
    "triclinic_pbc_ani2x": (61, 133, 156), "small_ani2x": (71, 143, 149), "dense90_ani2x": (89,),
}


def report(line):
    print(line)   # (pytest -rP shows the lines of passing tests)


def longest_row(g, cutoff):
    """Longest row of a golden case within cutoff, over its molecules (fp64 enumeration of the images)."""
    pbc = None if g["pbc"] is None else tuple(bool(b) for b in g["pbc"])
    return max(int(so.row_lengths(so.rows_of(g["species"][m], g["coords"][m], g["cell"], pbc, cutoff)).max())
               for m in range(g["species"].shape[0]))


def test_fixture_rows():
    """No second-order fixture has a row above 128 within 5.2 A (89 is the longest), no hess_pairs_* base one above 192 at
    any cutoff of gen_golden_pairs2.cases (133), no first-order pair or D3 fixture one above 156: the table of the rows."""
    report(f"{'fixture':26s} {'<= 5.2 A':>9s} {'<= 7.5 A':>9s} {'<= 8.0 A':>9s}")
    for name in HESSIAN_FIXTURES:
        g = load_golden(name)
        got = tuple(longest_row(g, rc) for rc in (5.2, 7.5, 8.0)[:len(EXPECTED_ROWS[name])])
        report(f"{name:26s} " + " ".join(f"{v:9d}" for v in got))
        assert got == EXPECTED_ROWS[name], (name, got)
        assert got[0] <= 128
    for name in PAIR_HESSIAN_BASES:
        g = load_golden(name)
        longest = max(longest_row(g, rc) for rc in PAIR_CUTOFFS)
        report(f"hess_pairs_{name}: longest row at the cutoffs {PAIR_CUTOFFS}: {longest}")
        assert longest <= 192


def test_pair_rows_of_the_long_row_fixtures():
    """The rows of the two long-row cases of the pair fixtures (pairs_, pairs2_, d3_, hess_pairs_<case>.npz) at every pair
    cutoff, D3's 8 A included (an infinite cutoff on the open case: all other atoms): none above 256; chunk256_open/seven
    has rows of 193..256 entries at 5.2 A and beyond (the fourth 64-entry round of k_pair_hvp, k_pair and the D3 passes),
    at 5.2 A only the centre's (so its Hessian rows are among the stored ones); chunk129_pbc/built has 130 atoms in a 60 A
    cell, so its longest row is 129 at every cutoff: no periodic case puts the pair kernels on a row above 192 entries."""
    longest = {}
    for name in ("chunk256_open/seven", "chunk129_pbc/built"):
        c = ac.case_by_name(name)
        for rc in PAIR_CUTOFFS + (8.0,) + (() if c.periodic else (1.0e3,)):
            longest[name, rc] = int(so.row_lengths(so.rows_of(c.species, c.coords, c.cell, c.pbc, rc)).max())
            report(f"{name} within {rc} A: longest row {longest[name, rc]}")
    assert max(longest.values()) <= 256
    assert all(193 <= longest["chunk256_open/seven", rc] <= 256 for rc in (5.2, 7.5, 8.0, 1.0e3))
    assert all(longest["chunk129_pbc/built", rc] == 129 for rc in (5.2, 7.5, 8.0))
    c = ac.case_by_name("chunk256_open/seven")
    at52 = so.row_lengths(so.rows_of(c.species, c.coords, None, None, 5.2))
    assert np.nonzero(at52 > 192)[0].tolist() == [0] and int(at52[1:].max()) <= 192


def second_lines(label, sec):
    """Per direction: the spread |D(h) - D(2h)| against a hundredth of the gate, without and with the first-order term."""
    ok = True
    for k in range(sec.curv.shape[0]):
        tol = 0.01 * so.GATE * min(so.mag(sec.curv[k]), so.mag(sec.curv[k] + sec.lin[k]))
        report(f"{label} direction {k}: h {sec.h[k]:.0e} |D(h) - D(2h)| {sec.spread[k]:.2e} (gate / 100 = {tol:.2e}; max|ref| "
               f"{np.abs(sec.curv[k]).max():.1f})")
        ok &= bool(sec.spread[k] < tol)
    return ok


@pytest.mark.parametrize("run", so.RUNS, ids=RUN_IDS)
def test_differences_have_converged(run):
    """Dense directions and item slabs of every run: |ref(h) - ref(2h)| below a hundredth of the gate of that direction,
    without and with its first-order term."""
    ok = second_lines(f"{so.run_id(run)} dense", so.dense_ref(*run))
    for it in so.items_ref(*run):
        ok &= second_lines(f"{so.run_id(run)} items of atom {it.atom} (|R| {len(it.R)})", it.second)
    assert ok


@pytest.mark.parametrize("run", so.STRAIN_RUNS, ids=[so.run_id(r) for r in so.STRAIN_RUNS])
def test_strain_differences_have_converged(run):
    ref = so.strain_ref(*run)
    tag = so.run_id(run)
    ok = True
    for k in range(9):
        tol = 0.01 * so.GATE * min(so.mag(ref.curv[k]), so.mag(ref.curv[k] + ref.lin[k]))
        jtol = 0.01 * so.JVP_TOL * np.maximum(1.0, np.abs(ref.jvp[k]).max(axis=1))
        report(f"{tag} strain direction {k}: h {ref.h[k]:.0e} out spread {ref.curv_spread[k]:.2e} (gate / 100 = {tol:.2e}); J rows "
               f"spread / (row gate / 100), worst {float((ref.jvp_spread[k] / jtol).max()):.2e}")
        ok &= bool(ref.curv_spread[k] < tol) and bool(np.all(ref.jvp_spread[k] < jtol))
    stol = 0.01 * so.SS_GATE * min(np.abs(ref.ss).max(), np.abs(ref.ss + ref.ss_lin).max())
    report(f"{tag} ss spread {ref.ss_spread:.2e} (gate / 100 = {stol:.2e}; max|ss| {np.abs(ref.ss).max():.1f})")
    assert ok and ref.ss_spread < stol


@pytest.mark.parametrize("name", so.MODEL_CASES)
def test_model_differences_have_converged(name):
    cols, ref = so.model_ref(name)
    for q, col in enumerate(cols):
        tol = 0.01 * so.GATE * so.mag(ref.value[q])
        report(f"{name} model column {col}: |D(h) - D(2h)| {ref.spread[q].max():.2e} (gate / 100 = {tol:.2e}; max|ref| "
               f"{np.abs(ref.value[q]).max():.2f})")
        assert ref.spread[q].max() < tol


def test_every_regime_has_a_case():
    """Which case of the GPU file drives which long-row path of the second-order kernels; the controls drive none."""
    names = [n for n in dict.fromkeys([r[0] for r in so.RUNS] + list(so.PATTERN_CASES))]
    table = {r: [] for r in so.SO_REGIMES}
    for n in names:
        for r in so.so_regimes_of(n):
            table[r].append(n)
    for r in so.SO_REGIMES:
        report(f"regime {r:52s} {len(table[r]):2d} cases: {', '.join(table[r])}")
    assert all(table[r] for r in so.SO_REGIMES)
    for n in so.CONTROLS:
        assert not so.so_regimes_of(n), n
    for n in so.LONG:
        assert so.so_regimes_of(n), n
    by = {n: ac.row_stats(ac.case_by_name(n), ac.case_by_name(n).num_species) for n in names}
    assert by["ang128_at_open/one"].cnt_a[0].max() == 128                       # 8128 pairs in one block
    assert (by["spec255_at_open/built"].cnt_a + by["spec255_at_open/built"].cnt_f)[0].max() == 255
    assert by["chunk256_open/seven"].rad[0] == 256 and by["chunk129_pbc/built"].rad[0] == 129
    assert so.DUP_CASE in table["atom twice in a row, in different 64-entry pieces"]
    assert so.DUP_CASE in so.PATTERN_CASES and so.DUP_CASE in [r[0] for r in so.STRAIN_RUNS]
    # the structure is compared exactly: no pair may sit where an fp32 builder could place it either way
    for n in so.PATTERN_CASES:
        assert so.case_rows(n).banded == 0, n
    assert any(ac.case_by_name(r[0]).periodic for r in so.STRAIN_RUNS) and any(not ac.case_by_name(r[0]).periodic
                                                                               for r in so.STRAIN_RUNS)


def test_reference_pinned_to_a_hessian_fixture():
    """Four rows of tests/golden/hess_dense90_ani2x.npz (the reference project's fp64 Hessian; H is symmetric, a row is a
    column) from hessian_columns, to float32 resolution of the largest entry."""
    g = load_golden("dense90_ani2x")
    with np.load(os.path.join(GOLDEN_DIR, "hess_dense90_ani2x.npz")) as z:
        rows, hess = z["hess_rows"], z["hess"][0]
    pick = [0, 9, 20, 31]
    ref = so.hessian_columns(g["kind"], g["seed"], g["species"][0], g["coords"][0], [int(rows[q]) for q in pick],
                             cutoff_fn=g["cutoff_fn"], n_members=g["n_members"])
    err = np.abs(ref.value - hess[pick]).max()
    tol = float(np.finfo(np.float32).eps) * np.abs(hess[pick]).max()
    report(f"dense90 rows {[int(rows[q]) for q in pick]}: |fd - fixture| {err:.2e} (float32 resolution {tol:.2e}, max|H| "
           f"{np.abs(hess[pick]).max():.3f}); spread {ref.spread.max():.2e}")
    assert err <= tol


def test_strain_convention_reproduces_a_fixture():
    """strain_second -- the code that makes the references of out and ss -- on the whole model's gradient and virial
    reproduces tests/golden/hess_strain_water_pbc_ani2x.npz (the reference project's fp64 double autograd, the fixture of
    tests/test_gpu_strain_hessians.py): virial[a, b], strain_hessians[x, y, a, b] = ss[3 x + y][3 a + b] and
    internal_strain[i, y, a, b] = out[3 a + b][i][y] + delta_ya (d E / d x_i)_b."""
    g = load_golden("water_pbc_ani2x")
    with np.load(os.path.join(GOLDEN_DIR, "hess_strain_water_pbc_ani2x.npz")) as z:
        fx = {k: z[k] for k in ("virial", "strain_hessians", "internal_strain")}
    pbc = tuple(bool(b) for b in g["pbc"])
    curv, ss, V0, F = so.model_strain(g["kind"], g["seed"], g["species"][0], g["coords"][0], g["cell"], pbc,
                                      cutoff_fn=g["cutoff_fn"], n_members=g["n_members"])
    A = g["species"].shape[1]
    internal = curv.value.reshape(3, 3, A, 3).transpose(2, 3, 0, 1).copy()   # [i, y, a, b]
    for a in range(3):
        internal[:, a, a, :] += -F
    errs = {"virial": np.abs(V0 - fx["virial"][0]).max() / np.abs(fx["virial"]).max(),
            "strain_hessians": np.abs(ss.value.reshape(3, 3, 3, 3) - fx["strain_hessians"][0]).max()
            / np.abs(fx["strain_hessians"]).max(),
            "internal_strain": np.abs(internal - fx["internal_strain"][0]).max() / np.abs(fx["internal_strain"]).max()}
    report("water_pbc strain fixture, |fd - fixture| / max|fixture|: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    # a wrong index convention is an error of order 1; a tenth of the 2e-5 the fixture is compared at on the MI355X
    assert all(v <= 0.1 * so.SS_GATE for v in errs.values()), errs
