"""Host-side proof that the pair-virial fixtures and gates can tell a wrong kernel from a right one (no GPU, no reference;
tests/_pair_virial_cases.py, tests/golden/gen_golden_pair_virials.py).

* the gates follow from the error of the reference's own float32 evaluation (4 x, rounded up, capped by the relative force
  gate of the same loop) -- printed per (potential, case); profiles/pair_virial_tests.txt keeps the table: worst 1.74e-6 A
  (xtb), 7.37e-6 A (lj) and 1.91e-5 A (d3), so the three gates are their caps 5e-6, 1e-5 and 2e-5;
* every (potential, case) has max |W_ref| >= 100 x its gate (smallest: mnok on water_pbc_ani2x, 158 x) -- nothing excluded;
  D3 on own4 is the entry d3_r75 with a 7.5 A cutoff, the one the GPU test runs (8 A rows do not fit the engine's 256);
* the mistakes a virial kernel can make each move W by at least 10 x the gate on every one of them: own images dropped
  (smallest 31 x, lj_rep on own4), xz and yz swapped (54 x), (0, 1) written without (1, 0) (49 x), a missing 1/2 (158 x);
* the new fixtures repeat the energies and forces of the older fixtures of the same cases, and the model virials are the
  network part plus the pair fixtures of their terms.
"""
import os

import numpy as np
import pytest

import _pair_virial_cases as pv

GOLDEN = pv.GOLDEN_DIR
COUNT_FACTOR, MUTATION_FACTOR = 100.0, 10.0


def entries():
    for case in pv.CASE_NAMES:
        z = pv.load_virials(case)
        for key in pv.keys_of(case):
            yield case, key, z


def gate(key, z):
    return pv.GATE_REL[pv.FAMILY[key]] * float(z[key + "_abs"])


def counted(case, key):
    return (key, case) not in pv.EXCLUDED


def test_case_table():
    assert len(pv.CASE_NAMES) == 6
    for name in pv.CASE_NAMES:
        c = pv.case_by_name(name)
        assert c.n_atoms <= 130 and c.coords.dtype == np.float32 and c.cell.dtype == np.float32
        assert c.species.shape == (1, c.n_atoms) and c.coords.shape == (1, c.n_atoms, 3) and any(c.pbc)
    w, t = pv.case_by_name("water_pbc_ani2x"), pv.case_by_name("water_ttf")
    assert np.array_equal(w.coords, t.coords) and np.array_equal(w.cell, t.cell) and t.pbc == (True, True, False)
    assert pv.case_by_name("chunk129_pbc/built").n_atoms == 130
    # the own-image cells: as many pairs and own images as the reference listed, the shortest distance of own4
    z4, z1 = pv.load_virials("own4"), pv.load_virials("own1")
    assert tuple(z4["lj_pairs"]) == (449, 116) and tuple(z4["d3_r75_pairs"]) == (449, 116)
    assert pv.d3_key_of("own4") == "d3_r75" and "d3" not in pv.keys_of("own4")   # (8 A: rows of 286 entries, refused)
    assert pv.D3_KW["d3_r75"]["cutoff"] == pv.OWN4_D3_CUTOFF < pv.D3_KW["d3"]["cutoff"]
    o4 = pv.case_by_name("own4")
    x, cell = o4.coords[0].astype(np.float64), o4.cell.astype(np.float64)
    sh = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), -1).reshape(-1, 3) @ cell
    d = np.linalg.norm(x[:, None, None] - x[None, :, None] - sh[None, None], axis=-1)
    assert abs(d[d > 0].min() - 1.488) < 5e-3   # (H .. H through the cell's second vector: no pair on a repulsive wall)
    for key in pv.keys_of("own1"):
        n, own = z1[key + "_pairs"]
        assert n == own > 0, key
        assert np.array_equal(z1[key + "_forces"], np.zeros((1, 1, 3))), key   # the two images of a pair cancel exactly
        assert np.allclose(z1[key + "_virial"], z1[key + "_virial_self"], rtol=0, atol=1e-9 * float(z1[key + "_abs"]))
    # chunk129_pbc/built at 8 A: rows of 129 entries (8015 pairs of 130 atoms = 123.3 per atom, every atom sees all others)
    assert int(pv.load_virials("chunk129_pbc/built")["d3_pairs"][0]) > 64 * 130 // 2


def test_fixtures_are_complete_and_symmetric():
    for case, key, z in entries():
        a = float(z[key + "_abs"])
        w, ws, w32 = z[key + "_virial"], z[key + "_virial_self"], z[key + "_virial_f32"]
        assert w.shape == ws.shape == w32.shape == (3, 3) and w.dtype == np.float64 and a > 0
        assert np.abs(w - w.T).max() <= 1e-10 * a and np.abs(ws - ws.T).max() <= 1e-10 * a
        assert np.abs(w).max() <= a and np.abs(ws).max() <= a
        if int(z[key + "_pairs"][1]) == 0:
            assert not ws.any()
    # the water cell is 8 A wide: D3's cutoff reaches an atom's own image there, the other potentials' do not
    zw = pv.load_virials("water_pbc_ani2x")
    assert zw["d3_pairs"][1] == 90 and zw["lj_pairs"][1] == 0


def test_gates_follow_from_the_fp32_reference():
    worst = {f: (0.0, None) for f in pv.GATE_CAP}
    print()
    for case, key, z in entries():
        a = float(z[key + "_abs"])
        rel = float(np.abs(z[key + "_virial_f32"] - z[key + "_virial"]).max()) / a
        print(f"fp32 reference  {case:20s} {key:8s} |W_f32 - W|max / A = {rel:.2e}   max|W| / A = "
              f"{np.abs(z[key + '_virial']).max() / a:.3f}   A = {a:.3e} Ha")
        if counted(case, key) and rel > worst[pv.FAMILY[key]][0]:
            worst[pv.FAMILY[key]] = (rel, (case, key))
    for fam, (rel, where) in worst.items():
        want = pv.gate_from_f32(rel, pv.GATE_CAP[fam])
        print(f"gate  {fam:8s} worst fp32 reference {rel:.2e} at {where}: 4 x = {4 * rel:.1e}, rounded up and capped at "
              f"{pv.GATE_CAP[fam]:.0e} -> {want:.0e}")
        assert pv.GATE_REL[fam] == want and pv.GATE_REL[fam] <= pv.GATE_CAP[fam]
    assert pv.gate_from_f32(1.2e-7, 1.0) == pytest.approx(5e-7) and pv.gate_from_f32(2.5e-7, 1.0) == pytest.approx(1e-6)
    assert pv.gate_from_f32(1.0e-7, 1.0) == pytest.approx(4e-7) and pv.gate_from_f32(1.0, 2e-5) == 2e-5


def test_counting_condition():
    assert len(pv.EXCLUDED) <= 2 and not [k for k in pv.EXCLUDED if k[1] == "own4"]
    low = []
    for case, key, z in entries():
        ratio = float(np.abs(z[key + "_virial"]).max()) / gate(key, z)
        low.append((ratio, key, case))
        if counted(case, key):
            assert ratio >= COUNT_FACTOR, (key, case, ratio)
        else:
            assert ratio < COUNT_FACTOR, f"{key} on {case} counts ({ratio:.0f} x its gate): take it out of EXCLUDED"
    for k in pv.EXCLUDED:
        assert k[1] in pv.CASE_NAMES and k[0] in pv.keys_of(k[1])
    print("\nsmallest max|W_ref| / gate:", ", ".join(f"{k} on {c} {r:.0f}" for r, k, c in sorted(low)[:3]))


def mutations(w, w_self):
    swap = w.copy()
    swap[0, 2], swap[2, 0], swap[1, 2], swap[2, 1] = w[1, 2], w[2, 1], w[0, 2], w[2, 0]
    anti = w.copy()
    anti[1, 0] = 0.0
    return {"own images dropped": w - w_self, "xz and yz swapped": swap, "(0, 1) without (1, 0)": anti, "missing 1/2": 2.0 * w}


def test_mutations_are_seen():
    smallest = {}
    qualifying_own = []
    for case, key, z in entries():
        if not counted(case, key):
            continue
        w, g = z[key + "_virial"], gate(key, z)
        for what, wm in mutations(w, z[key + "_virial_self"]).items():
            moved = float(np.abs(wm - w).max()) / g
            if what == "own images dropped":
                if case not in ("own4", "own1"):
                    if case in pv.OWN_IMAGE_CASES and moved >= MUTATION_FACTOR:   # (triclinic: where it qualifies)
                        qualifying_own.append(key)
                    continue
            assert moved >= MUTATION_FACTOR, f"{what}: {key} on {case} moves W by {moved:.1f} gates only"
            if moved < smallest.get(what, (np.inf,))[0]:
                smallest[what] = (moved, key, case)
    print()
    for what, (moved, key, case) in smallest.items():
        print(f"mutation  {what:24s} moves W by >= {moved:8.1f} gates (smallest: {key} on {case})")
    print("own images of triclinic_pbc_ani2x are visible for", qualifying_own)
    assert set(qualifying_own) >= {"coulomb", "mnok", "d3"}


def test_element_constants_are_the_generators():
    """CHARGES, ETA, EPS, SIGMA of the case table against the text of gen_golden_pairs2.py (importing it loads the reference)."""
    src = open(os.path.join(GOLDEN, "gen_golden_pairs2.py")).read()
    ns: dict = {}
    exec("CHARGES = " + src.split("def cases(symbols):")[0].split("CHARGES = ")[1], ns)
    for name in ("CHARGES", "ETA", "EPS", "SIGMA"):
        assert ns[name] == getattr(pv, name), name


def _sum(path, key):
    with np.load(os.path.join(GOLDEN, path)) as z:
        return float(z[key].sum())


def test_energies_repeat_the_older_fixtures():
    for case in ("water_pbc_ani2x", "triclinic_pbc_ani2x", "chunk129_pbc/built"):
        z, fn = pv.load_virials(case), case.replace("/", "_")
        old = {"xtb": _sum(f"pairs_{fn}.npz", "energies"), "d3": _sum(f"d3_{fn}.npz", "energies")}
        old.update({k: _sum(f"pairs2_{fn}.npz", k + "_atomic") for k in pv.ANALYTIC_KEYS})
        if case == "water_pbc_ani2x":
            old["xtb_cos"] = _sum("pairs_cos_water_pbc_ani2x.npz", "energies")
            old["d3_b973c"] = _sum("d3_b973c_water_pbc_ani2x.npz", "energies")
        assert set(old) == set(pv.keys_of(case))
        for key, e in old.items():
            assert abs(float(z[key + "_energy"]) - e) <= 1e-10 * max(1.0, abs(e)), (case, key)


@pytest.mark.parametrize("kind,case,seed", pv.MODEL_CASES)
def test_model_fixtures(kind, case, seed):
    m = pv.load_model_virials(kind, case)
    c = pv.case_by_name(case)
    sym = [str(s) for s in m["symbols"]]
    assert int(m["seed"]) == seed and str(m["kind"]) == kind
    assert [sym[k] for k in m["species"][0]] == [c.symbols[k] for k in c.species[0]]
    assert np.array_equal(m["coords"], c.coords) and np.array_equal(m["cell"], c.cell) and tuple(m["pbc"]) == c.pbc
    wt, wn = m["virial_total"], m["virial_nnp"]
    assert np.abs(wt - wt.T).max() <= 1e-10 * max(1.0, np.abs(wt).max()) and np.abs(wn - wn.T).max() <= 1e-10
    # the pair part is the pair fixtures' (same recipe: xTB up to 5.2 A, smooth; D3 with the B97-3c constants on water_pbc)
    z = pv.load_virials(case)
    pair = z["xtb_virial"].copy()
    assert abs(float(m["abs_repulsion_xtb"]) - float(z["xtb_abs"])) <= 1e-9 * float(z["xtb_abs"])
    if kind == "ani2dr":
        assert float(m["d3_cutoff"]) == (pv.OWN4_D3_CUTOFF if case == "own4" else 8.0)
        if case != "water_pbc_ani2x":
            # (the model's D3 has the B97-3c constants, the pair fixtures of these cases the wB97X ones: nothing to add up
            # here; the generator asserts total = network part + pairwise sums of the model's own terms for every file)
            return
        pair += z["d3_b973c_virial"]
        assert abs(float(m["abs_dispersion_d3"]) - float(z["d3_b973c_abs"])) <= 1e-9 * float(z["d3_b973c_abs"])
    assert np.abs(wt - wn - pair).max() <= 1e-9 * float(z["xtb_abs"])
    if case == "water_pbc_ani2x":   # an older fixture has the same case, kind and seed
        with np.load(os.path.join(GOLDEN, f"x2r_{kind}_{case}.npz")) as old:
            assert int(old["seed"]) == seed
            assert np.abs(old["energies"] - m["energies"]).max() <= 1e-9
            assert np.abs(old["forces"] - m["forces"]).max() <= 1e-9
