"""The long-row cases of tests/_aev_cases.py on the CPU: every row inside the three row limits (under every set of constants
the case runs with), every long-row path of the AEV kernels reached by some case, and the fp32 build of the oracle against
the fp64 one on every case -- the figures the gates of tests/test_gpu_aev_long_rows.py are to be read against."""
import numpy as np
import pytest

import _aev_cases as ac
from _util import fgrad_direction
from oracle import oracle as orc
from oracle.oracle import Oracle

CASES = ac.all_cases()
IDS = [c.name for c in CASES]
# the gates the kernels are held to (tests/test_gpu_parity.py): the fp32 build of the SAME sums must sit inside them, or
# they could not be asked of an fp32 kernel
AEV_TOL = 2e-5
VJP_TOL = 2e-5


def report(line):
    print(line)   # (pytest -rP shows the lines of passing tests)


def constants_of(case, variant=None):
    """(Rcr, Rca, number of species) the case runs with."""
    return (5.2, 3.5, 4) if variant == "1x" else (ac.RCR, ac.RCA, case.num_species)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rows_within_limits(case):
    """At most 128 angular neighbors, 256 entries and 255 of one species in every row of a case not marked over, with the
    ANI-2x cutoffs and with the ANI-1x ones where the case runs on the 4 x 8 grid, before and after the move of the
    forward_update test; an over case is one over exactly one limit in the centre's row and inside them elsewhere."""
    for variant in (None,) + tuple(v for v in case.variants if v == "1x"):
        rcr, rca, S = constants_of(case, variant)
        assert int(case.species.max()) < S
        for coords in (None,) if case.over else (None, ac.moved(case)):
            st = ac.row_stats(case, S, rcr, rca, coords=coords)
            tot = st.cnt_a + st.cnt_f
            if not case.over:
                assert ac.within_limits(st), (case.name, variant, int(st.rad.max()), int(st.ang.max()), int(tot.max()))
                continue
            c = case.centre
            others = np.arange(case.n_atoms) != c
            assert ac.within_limits(st, others)
            excess = (int(st.rad[c]) - ac.MAX_RAD, int(st.ang[c]) - ac.MAX_ANG, int(tot[c].max()) - ac.MAX_PER_SPECIES)
            assert max(excess) == 1, excess
    if case.centre is not None:
        # the shells keep the centre's neighbors 0.5 A away from both cutoffs: its row is the same in fp32 and in fp64
        x = case.coords[0].astype(np.float64)
        r = np.linalg.norm(x - x[case.centre], axis=1)
        r = r[(r > 0) & (r < 6.0)]
        assert np.all(np.abs(r - ac.RCR) >= 0.5 - 1e-5) and np.all(np.abs(r - ac.RCA) >= 0.5 - 1e-5)


def test_every_regime_has_a_case():
    """Which case drives which long-row path, from the fp64 distances; a path without a case fails."""
    table = {r: [] for r in ac.REGIMES}
    for case in CASES:
        if case.over:
            continue
        st = ac.row_stats(case, case.num_species)
        for r in ac.regimes_of(st):
            table[r].append(case.name)
    for r in ac.REGIMES:
        report(f"regime {r:36s} {len(table[r]):2d} cases: {', '.join(table[r][:4])}{' ...' if len(table[r]) > 4 else ''}")
    missing = [r for r in ac.REGIMES if not table[r]]
    assert not missing, missing
    # the labellings do what they are for
    by = {c.name: ac.row_stats(c, c.num_species) for c in CASES if not c.over}
    c0 = lambda name: by[name].cnt_a[0]   # noqa: E731
    assert ac.block_pairs(c0("ang128_at_open/one")).count(8128) == 1 and sum(ac.block_pairs(c0("ang128_at_open/one"))) == 8128
    assert sum(p > 0 for p in ac.block_pairs(c0("ang128_at_open/seven"))) == 28
    lone = c0("chunk193_open/lone")
    assert lone[0] == 1 and lone[1] == 95 and ac.block_pairs(lone)[:2] == [0, 95]
    pad = by["chunk255_open/pad"]
    assert sorted((pad.cnt_a + pad.cnt_f)[0]) == sorted(ac.PAD_COUNTS)
    assert int((((pad.cnt_a + pad.cnt_f)[0] + 7) & ~7).sum()) == 255 + 49
    dense = by["dense"]
    assert int(((dense.ang >= 65) & (dense.ang <= 128)).sum()) >= 20 and dense.rad.max() <= 256
    assert by["lattice"].rad.max() > 128


@pytest.fixture(scope="module")
def oracle32():
    return Oracle("f32")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp32_oracle_against_fp64(oracle64, oracle32, case):
    """The fp32 build of the oracle -- the same sums, every operation rounded to fp32 -- against the fp64 build: AEV rows
    (per row, relative to max(1, largest entry of the row)), the VJP of a seeded cotangent, its virial and a JVP."""
    p = orc.params_2x() if case.num_species == 7 else orc.make_params(4, *_2x_tail())
    L = case.num_species * 16 + case.num_species * (case.num_species + 1) // 2 * 32
    w = np.random.RandomState(1000).uniform(-1.0, 1.0, (1, case.n_atoms, L)).astype(np.float32).astype(np.float64)
    t = fgrad_direction(case.species)
    x64 = case.coords.astype(np.float64)
    a64, g64, v64 = oracle64.aev(p, case.species, x64, case.cell, case.pbc, grad_aev=w, want_virial=True)
    a32, g32, v32 = oracle32.aev(p, case.species, x64, case.cell, case.pbc, grad_aev=w, want_virial=True)
    _, j64 = oracle64.aev_jvp(p, case.species, x64, t, case.cell, case.pbc)
    _, j32 = oracle32.aev_jvp(p, case.species, x64, t, case.cell, case.pbc)
    row_max = np.maximum(1.0, np.abs(a64[0]).max(axis=1))
    aerr = (np.abs(a32[0].astype(np.float64) - a64[0]).max(axis=1) / row_max).max()
    gmag, jmag, vmag = np.abs(g64).max(), np.abs(j64).max(), np.abs(v64).max()
    gerr = np.abs(g32.astype(np.float64) - g64).max() / max(1.0, gmag)
    jerr = np.abs(j32.astype(np.float64) - j64).max() / max(1.0, jmag)
    verr = np.abs(v32 - v64).max() / max(1.0, vmag)
    report(f"f32 oracle {case.name:28s} aev {aerr:.2e} x row max (largest entry {np.abs(a64).max():.1f})   vjp {gerr:.2e} x "
           f"{max(1.0, gmag):.1f}   virial {verr:.2e} x {max(1.0, vmag):.1f}   jvp {jerr:.2e} x {max(1.0, jmag):.1f}")
    assert aerr <= AEV_TOL and gerr <= VJP_TOL and jerr <= VJP_TOL


def _2x_tail():
    """ANI-2x constants behind the number of species, as oracle.params_2x passes them to make_params."""
    import math

    return (5.1, 3.5, 19.7, 12.5, 14.1, orc.linspace(0.8, 5.1, 16), orc.linspace(0.8, 3.5, 8),
            orc.linspace(math.pi / 8, math.pi + math.pi / 8, 4), "cosine")
