"""The constant sets of tests/_aev_constants.py on the CPU: the flags anihip_aev_table_pack gives every set, the admission
quantities recomputed in fp64 (every boundary set within 5 % of its bound on the stated side, and its Eta the very
two-digit value at which the packer's flag flips; their geometries reach at least 80 % of the exponents the bounds are
stated for), the sweep's flag counts, the shape of the rows (which sets have an
empty far part, a half-filled last radial slab, every species count 1 .. 7), the fp32 build of the oracle against the fp64
one on every set and geometry -- the figures the gates of tests/test_gpu_aev_constants.py are to be read against: a set on
which fp32 cannot hold HALF of a gate is replaced, not gated more loosely -- and the convergence of the finite differences
behind the second-order references."""
import os

import numpy as np
import pytest

import _aev_cases as ac
import _aev_constants as kc

RUNS = kc.runs()
RUN_IDS = [kc.run_id(r) for r in RUNS]
SWEEP_RUNS = kc.sweep_runs()
# the gates the kernels are held to (tests/test_gpu_parity.py, tests/test_gpu_aev_long_rows.py)
AEV_TOL = 2e-5
VJP_TOL = 2e-5
VJP_REG_REL = 5e-6
JVP_TOL = 2e-5
VIRIAL_TOL = 1e-4
GATE = 2e-5   # tests/_second_order_ref.py


def report(line):
    print(line)   # (pytest -rP shows the lines of passing tests)


def packer_flags(cset):
    from torchani_amd.engine import AevEngine

    eng = AevEngine(cset.aev_constants())
    eng.host_table()
    assert eng.tuned
    return eng.params.flags & 3


@pytest.fixture(scope="module", autouse=True)
def lib():
    from torchani_amd import _lib

    _lib.build()
    return _lib.lib()


@pytest.mark.parametrize("cset", kc.SETS, ids=kc.SET_NAMES)
def test_packer_gives_the_stated_flags(cset):
    """anihip_aev_table_pack on the set: the flags the table states, which are also the flags of the inequalities restated
    in fp64 (admission)."""
    a = kc.admission(cset)
    got = packer_flags(cset)
    report(f"{cset.name:12s} {cset.grid[0]} x {cset.grid[1]} S={cset.num_species} {cset.cutoff_fn:6s} flags {got}: forward "
           f"{a.fwd:6.1f} / 100, backward angular {a.bwd_ang:6.1f} / 110, radial {a.bwd_rad:6.1f} / 110  -- {cset.reaches}")
    assert got == cset.flags == a.flags
    assert a.uniform_a and a.uniform_r   # (unequally spaced ShfA / ShfR: test_aev_with_unequally_spaced_shifts)


@pytest.mark.parametrize("group", sorted(kc.BOUNDARY_ETAS))
def test_boundary_values_are_where_the_packer_flips(group):
    """With the ANI-2x shifts and cutoffs, the packer asked for every two-digit Eta from 10 to 99: the flag of the group is
    kept up to the value of the "inside" set and cleared from the value of the "outside" set on, and those two are
    neighbors.  Each of the two sets lies within 5 % of its bound, on its side."""
    field, last_in, first_out = kc.BOUNDARY_ETAS[group]
    bit = 1 if group == "forward" else 2
    inside, outside = (next(c for c in kc.SETS if c.near == (group, side)) for side in ("inside", "outside"))
    assert getattr(inside, field) == last_in and getattr(outside, field) == first_out == last_in + 1.0
    base = inside._replace(EtaA=float(np.float32(12.5)), EtaR=float(np.float32(19.7)))   # the ANI-2x constants
    kept = [bool(packer_flags(base._replace(**{field: float(v)})) & bit) for v in range(10, 100)]
    flips = [v for v, (a, b) in zip(range(11, 100), zip(kept[:-1], kept[1:])) if a != b]
    assert kept[0] and flips == [int(first_out)], (group, flips)
    for cset, side in ((inside, "inside"), (outside, "outside")):
        q, bound = kc.admission(cset).of(group)
        report(f"{group}: {cset.name} {field} = {getattr(cset, field):.0f}: {q:.2f} / {bound:.0f} ({side})")
        assert (0.95 * bound <= q < bound) if side == "inside" else (bound <= q <= 1.05 * bound)
        assert bool(packer_flags(cset) & bit) == (side == "inside")
        # nothing but the one Eta differs from ANI-2x
        assert cset._replace(**{field: getattr(base, field)})[2:11] == base[2:11]


def test_sweep_flag_counts():
    """The sweep's flags from the restated inequalities are the packer's, trial by trial; each of 0, 1 and 3 occurs at least
    four times; SWEEP_SEED is the first seed that does that; the trials cover both grids, both envelopes, every Zeta."""
    trials = kc.sweep()
    assert len(trials) == kc.SWEEP_TRIALS == 24
    for t in trials:
        assert packer_flags(t.cset) == t.cset.flags, t.cset.name
    n = kc.flag_counts(trials)
    report(f"sweep seed {kc.SWEEP_SEED}: flags 0 x {n[0]}, 1 x {n[1]}, 2 x {n[2]}, 3 x {n[3]}")
    assert min(n[0], n[1], n[3]) >= 4
    assert kc.first_good_seed() == kc.SWEEP_SEED
    sets = [t.cset for t in trials]
    assert {c.grid for c in sets} == {(8, 4), (4, 8)} and {c.cutoff_fn for c in sets} == {"cosine", "smooth"}
    assert {round(c.Zeta, 1) for c in sets} == {1.0, 8.0, 14.1, 32.0}
    assert {t.geom.split(":")[0] for t in trials} == {"cluster", "pbc", "batch"}
    for c in sets:
        assert 4.0 <= c.Rcr <= 6.0 and 2.5 <= c.Rca <= c.Rcr and 4.0 <= c.EtaR <= 40.0 and 4.0 <= c.EtaA <= 24.0
        assert c.ShfR[-1] < c.Rcr and c.ShfA[-1] < c.Rca


def test_table_covers_what_it_is_for():
    """Every species count 1 .. 7, both grids and both envelopes in the table; flags 1 with equally spaced ShfA; the sets the
    issue names, with their constants."""
    assert {c.num_species for c in kc.SETS} == set(range(1, 8))
    assert {c.grid for c in kc.SETS} == {(8, 4), (4, 8)} and {c.cutoff_fn for c in kc.SETS} == {"cosine", "smooth"}
    assert any(c.flags == 1 and kc.admission(c).uniform_a for c in kc.SETS)
    by = {c.name: c for c in kc.SETS}
    z1 = by["g48_zeta1"]
    assert (z1.grid, z1.Zeta, z1.EtaA, z1.Rcr, z1.Rca) == ((4, 8), 1.0, 4.0, 6.0, 4.0)
    assert by["g84_zeta64"].grid == (8, 4) and by["g84_zeta64"].Zeta == 64.0
    assert by["rca_eq_rcr"].Rca == by["rca_eq_rcr"].Rcr == 4.0
    dz = np.diff(by["shfz_bent"].ShfZ)
    assert dz.max() - dz.min() > 0.1
    assert by["shift_half"].ShfR[0] == by["shift_half"].ShfA[0] == 0.5
    assert (by["g48_smooth"].grid, by["g48_smooth"].cutoff_fn) == ((4, 8), "smooth")
    from torchani_amd.constants import aev_constants_simple
    xr, simple = by["xr_cosine"], aev_constants_simple()
    assert xr.cutoff_fn == "cosine" and simple.cutoff_fn == "smooth"
    assert np.allclose(xr.ShfR, simple.ShfR, atol=1e-6) and np.allclose(xr.ShfA, simple.ShfA, atol=1e-6)
    assert set(kc.SECOND_ORDER_SETS) <= set(kc.SET_NAMES) and by[kc.SECOND_ORDER_SETS[0]].near is not None
    assert len(kc.LONG_ROW_SETS) == 2 and all(by[n].near is not None and by[n].flags == 3 for n in kc.LONG_ROW_SETS)
    assert all(by[n].flags & 2 for n in kc.PUSHED_SETS)
    # no set repeats a published one
    from torchani_amd.constants import aev_constants_1x, aev_constants_2x
    for c in kc.SETS:
        for pub in (aev_constants_2x(c.num_species), aev_constants_1x(c.num_species), aev_constants_simple(c.num_species)):
            same = (np.float32(pub.Rcr), np.float32(pub.Rca), np.float32(pub.EtaR), np.float32(pub.EtaA),
                    np.float32(pub.Zeta)) == (c.Rcr, c.Rca, c.EtaR, c.EtaA, c.Zeta) and pub.cutoff_fn == c.cutoff_fn \
                and len(pub.ShfA) == len(c.ShfA) and np.allclose(pub.ShfR, c.ShfR, atol=1e-6) \
                and np.allclose(pub.ShfA, c.ShfA, atol=1e-6) and np.allclose(pub.ShfZ, c.ShfZ, atol=1e-6)
            assert not same, c.name


@pytest.mark.parametrize("run", RUNS + SWEEP_RUNS, ids=RUN_IDS + [kc.run_id(r) for r in SWEEP_RUNS])
def test_rows(run):
    """Rows inside the three limits before and after the displacement of the forward_update test, no pair closer than
    0.75 A, no pair within _nbr_cases.BAND of a cutoff (so the slab flags are decided); the far part of every row empty
    exactly where Rca = Rcr; the last radial slab half filled exactly where the species count is odd; the long-row case
    crosses a 64-entry chunk seam."""
    cset, geom = kc.set_by_name(run[0]), kc.geometry_of(run)
    st = kc.row_stats(geom, cset)
    moved = kc.row_stats(geom, cset, coords=kc.displaced(geom))
    for s in (st, moved):
        assert ac.within_limits(s), (run, int(s.rad.max()), int(s.ang.max()))
    assert kc.closest_pair(geom) >= kc.MIN_DIST
    assert int(geom.species.max()) < cset.num_species
    assert st.banded == 0 and moved.banded == 0
    if run in RUNS:
        assert (int(st.cnt_f.sum()) == 0) == (cset.Rca == cset.Rcr)
    real = geom.species.reshape(-1) >= 0
    if geom.n_atoms > 2:
        assert np.all(st.rad[real] > 0)
    assert np.all(st.rad[~real] == 0)
    if cset.Rca == cset.Rcr:
        assert np.array_equal(st.rad, st.ang) and int(st.ang.max()) < 128
    if run[1] == kc.LONG_ROW_CASE:
        assert int(st.rad.max()) == 129 and int(st.ang.max()) >= 64
    lo, hi = kc.central_range(geom)
    assert 0 < lo < hi < geom.n_atoms or geom.n_atoms <= 2
    n_moved = int((kc.displaced(geom) != geom.coords).any(axis=-1).sum())
    assert n_moved == -(-geom.n_atoms // 3)
    report(f"{kc.run_id(run):36s} N={geom.n_atoms:3d} S={cset.num_species} longest row {int(st.rad.max()):3d}, angular "
           f"{int(st.ang.max()):3d}, far entries {int(st.cnt_f.sum()):5d}, radial slabs {(cset.num_species + 1) // 2}"
           f"{' (last half filled)' if cset.num_species % 2 else ''}")


@pytest.mark.parametrize("run", [r for r in RUNS if r[0] in kc.BOUNDARY_NAMES], ids=lambda r: kc.run_id(r))
def test_geometries_reach_the_admitted_exponents(run):
    """The bounds are stated for distances 0 .. Rc; a geometry cannot have a pair closer than 0.75 A, and a pair at the cutoff
    has no weight.  What the boundary sets' geometries do reach -- the same three quantities from their own distances -- is
    at least 80 % of the worst case the packer admits by, for each of the three groups."""
    cset, geom = kc.set_by_name(run[0]), kc.geometry_of(run)
    a, got = kc.admission(cset), kc.reach(geom, cset)
    report(f"{kc.run_id(run):36s} reached / admitted by: forward {got.fwd:6.1f} / {a.fwd:6.1f}, backward angular "
           f"{got.bwd_ang:6.1f} / {a.bwd_ang:6.1f}, radial {got.bwd_rad:6.1f} / {a.bwd_rad:6.1f}")
    for g, w in zip(got[:3], a[:3]):
        assert 0.8 * w <= g <= w


def test_fixture_geometry_of_rca_eq_rcr():
    """tests/golden/grid_tuned_rca_eq_rcr.npz was written with Rca one fp32 step below Rcr (the reference refuses
    Rca = Rcr): no pair of its geometry lies between the two, and its cell is at least twice the cutoff."""
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid_tuned_rca_eq_rcr.npz")) as z:
        rca, rcr, cell = float(z["Rca"]), float(z["Rcr"]), z["cell"].astype(np.float64)
    cset = kc.set_by_name("rca_eq_rcr")
    assert rcr == cset.Rcr and rca == float(np.nextafter(np.float32(rcr), np.float32(0.0)))
    geom = kc.geometry_of(("rca_eq_rcr", "pbc16"))
    st = kc.row_stats(geom, cset._replace(Rca=rca))
    assert int(st.cnt_f.sum()) == 0 and st.banded == 0
    heights = abs(np.linalg.det(cell)) / np.linalg.norm(np.cross(cell[[1, 2, 0]], cell[[2, 0, 1]]), axis=1)
    assert heights.min() >= 2.0 * rcr


@pytest.mark.parametrize("run", RUNS + SWEEP_RUNS, ids=RUN_IDS + [kc.run_id(r) for r in SWEEP_RUNS])
def test_fp32_oracle_holds_half_of_every_gate(run):
    """The fp32 build of the oracle -- the same sums, every operation rounded to fp32, plain evaluation of every Gaussian --
    against the fp64 build: AEV rows (per row, relative to max(1, largest entry of the row)), the VJP of the seeded
    cotangent, its virial and J t, each under HALF of the gate the kernels are held to; VJP_REG_REL only where the table
    says it applies.  Worst over the table: rows 3.1e-6, VJP 2.7e-6 (g84_zeta64; 1.2e-6 elsewhere), J t 1.8e-6, virial
    1.8e-6."""
    cset = kc.set_by_name(run[0])
    r64, r32 = kc.reference(run), kc.reference(run, "f32")
    row_max = np.maximum(1.0, np.abs(r64.aev).max(axis=1))
    aerr = float((np.abs(r32.aev - r64.aev).max(axis=1) / row_max).max())
    gmag, jmag, vmag = (max(1.0, float(np.abs(v).max())) for v in (r64.vjp, r64.jvp, r64.virial))
    gerr = float(np.abs(r32.vjp - r64.vjp).max()) / gmag
    jerr = float(np.abs(r32.jvp - r64.jvp).max()) / jmag
    verr = float(np.abs(r32.virial - r64.virial).max()) / vmag
    report(f"f32 oracle {kc.run_id(run):36s} flags {cset.flags} aev {aerr:.2e} x row max (largest entry "
           f"{np.abs(r64.aev).max():.1f})   vjp {gerr:.2e} x {gmag:.1f}   virial {verr:.2e} x {vmag:.1f}   jvp {jerr:.2e} x "
           f"{jmag:.1f}")
    assert aerr <= 0.5 * AEV_TOL and gerr <= 0.5 * VJP_TOL and jerr <= 0.5 * JVP_TOL and verr <= 0.5 * VIRIAL_TOL
    if cset.vjp_reg:
        assert gerr <= 0.5 * VJP_REG_REL, "the table applies VJP_REG_REL to this set"
    # the inputs do something: every part of the row is exercised
    assert np.abs(r64.aev).max() > 0.1 and gmag > 0.0


def test_vjp_reg_is_waived_only_where_fp32_cannot_hold_it():
    """A set with vjp_reg = False has a geometry on which the fp32 oracle's VJP is more than half of VJP_REG_REL off."""
    for cset in kc.SETS:
        if cset.vjp_reg:
            continue
        worst = 0.0
        for g in cset.geoms:
            r64, r32 = kc.reference((cset.name, g)), kc.reference((cset.name, g), "f32")
            worst = max(worst, float(np.abs(r32.vjp - r64.vjp).max()) / max(1.0, float(np.abs(r64.vjp).max())))
        assert worst > 0.5 * VJP_REG_REL, (cset.name, worst)


@pytest.mark.parametrize("name", kc.SECOND_ORDER_SETS)
def test_second_order_differences_have_converged(name):
    """The 1 / 100-of-gate rule of tests/test_second_order_cases_host.py for the references of backward_second: per
    direction |D(h) - D(2h)| below a hundredth of GATE x max(1, largest entry), without and with the first-order term."""
    import _second_order_ref as so

    assert so.GATE == GATE
    sec = kc.second_reference((name, "cluster40"))
    ok = True
    for k in range(sec.curv.shape[0]):
        tol = 0.01 * GATE * min(so.mag(sec.curv[k]), so.mag(sec.curv[k] + sec.lin[k]))
        report(f"{name} direction {k}: h {sec.h[k]:.0e} |D(h) - D(2h)| {sec.spread[k]:.2e} (gate / 100 = {tol:.2e}; max|ref| "
               f"{np.abs(sec.curv[k]).max():.1f})")
        ok &= bool(sec.spread[k] < tol)
    assert ok
