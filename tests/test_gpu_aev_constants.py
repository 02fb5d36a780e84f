"""The tuned AEV kernels -- k_aev_fwd3, k_aev_bwd, k_aev_jvp of csrc/aev.hip, and k_aev_bwd2 of csrc/aev_hess.hip -- on constants
OFF the published models', against the fp64 oracle.  The kernels are picked from the grid sizes alone (16 radial shifts, 8 x 4
or 4 x 8 angular terms); EtaR, EtaA, Zeta, the cutoffs, the shift values, ShfZ, the species count and the envelope are free,
and what depends on them is where the cleverness is: anihip_aev_table_pack admits the Gaussian recurrences of the forward and
of the backward by inequalities on the exponents, the kernels clamp those exponents to match, the recurrences multiply
chains of exp2 values, Zeta and Zeta - 1 go through exp2(. log2|h|), the radial slabs are dealt two species at a time.  The
sets are those of tests/_aev_constants.py: the ANI-2x shifts with EtaA or EtaR at the last two-digit value inside each
admission bound and at the first outside it, the 4 x 8 grid with Zeta = 1, Zeta = 64, Rca = Rcr, unequal ShfZ, shifts from
0.5 A, the envelopes swapped between the grids, every species count 1 .. 7, and a seeded sweep of 24 trials; on 40-atom
clusters, a 60-atom triclinic box smaller than twice the cutoff, a padded 3 x 14 batch and, for two boundary sets, a row of 129
entries.  tests/test_aev_constants_host.py proves on the CPU which flags each set gets and that fp32 can hold the gates on
these inputs; tests/test_oracle_golden.py pins the oracle to the reference on three of the sets.

Every comparison asserts first that the engine took the tuned kernels with the flags the table states.

Gates, none of them new: AEV rows 2e-5 x max(1, largest entry of the ROW) (AEV_TOL of tests/test_gpu_parity.py, per row as in
tests/test_gpu_aev_long_rows.py); VJP 2e-5 (VJP_TOL) and, on the sets whose fp32-oracle error is under half of it, 5e-6
(VJP_REG_REL of tests/test_gpu_parity.py) x max(1, largest entry); J t 2e-5 x max(1, largest entry)
(tests/test_gpu_training.py::test_aev_jvp_matches_reference); virial 1e-4 Ha x max(1, largest entry)
(tests/test_gpu_md.py::test_virial_matches_reference_stress); second order 2e-5 x max(1, largest entry) per direction (GATE of
tests/_second_order_ref.py).

Measured on the MI355X (profiles/aev_constants_tests.txt, per set), worst over the table and the sweep, next to what the fp32
build of the oracle -- the same sums with every Gaussian evaluated directly -- makes of the same inputs:

                     kernels     fp32 oracle
  AEV rows           5.3e-6      3.1e-6     (both on g84_zeta64; 2.6e-6 / 1.9e-6 elsewhere)
  VJP                3.1e-6      2.7e-6     (g84_zeta64, where the 5e-6 gate is not asked; 2.9e-6 / 1.3e-6 elsewhere)
  virial             4.6e-6      1.9e-6     (of max(1, largest entry); the gate is 1e-4)
  J t                2.2e-6      1.8e-6
  second order       1.1e-6      -

The boundary sets are no worse than the others: inside the admission bounds the recurrences hold the gates with the margin
of the published sets (bwd_ang_in VJP 2.3e-6, bwd_rad_in 2.2e-6, fwd_in rows 2.1e-6).  With t[TAB_RECA] scaled by 1 + 1e-4
in a scratch build, test_backward fails on every set with flag 2 (bwd_ang_in: 7e-4 .. 1.2e-3 of max|vjp|) and passes on
every set without it."""
import functools

import numpy as np
import pytest
import torch

import _aev_cases as ac
import _aev_constants as kc
from test_gpu_parity import report

pytestmark = pytest.mark.gpu

AEV_TOL = 2e-5        # tests/test_gpu_parity.py
VJP_TOL = 2e-5        # tests/test_gpu_aev_long_rows.py
VJP_REG_REL = 5e-6    # tests/test_gpu_parity.py: the regression gate of test_aev_forward_and_backward
JVP_TOL = 2e-5        # tests/test_gpu_training.py::test_aev_jvp_matches_reference
VIRIAL_TOL = 1e-4     # tests/test_gpu_md.py::test_virial_matches_reference_stress, "assert err < 1e-4" (Ha)
GATE = 2e-5           # tests/_second_order_ref.py GATE (tests/test_gpu_hessians.py), per direction

RUNS = kc.runs()
RUN_IDS = [kc.run_id(r) for r in RUNS]
SWEEP_RUNS = kc.sweep_runs()
SWEEP_IDS = [kc.run_id(r) for r in SWEEP_RUNS]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from torchani_amd import _lib

    _lib.lib()  # fail loudly if the native library is missing
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def engine(set_name):
    from torchani_amd.engine import AevEngine

    eng = AevEngine(kc.set_by_name(set_name).aev_constants())
    eng.host_table()   # (anihip_aev_table_pack sets the flags)
    return eng


class Ctx:
    """One set of constants on one geometry, on the device."""

    def __init__(self, run, dev):
        self.run, self.tag = run, kc.run_id(run)
        self.cset, self.geom = kc.set_by_name(run[0]), kc.geometry_of(run)
        self.eng = engine(run[0])
        self.ref = kc.reference(run)
        self.stats = kc.row_stats(self.geom, self.cset)
        self.dev, self.n = dev, self.geom.n_atoms
        self.sp32 = torch.from_numpy(self.geom.species.astype(np.int32)).to(dev).contiguous()
        self.x = torch.from_numpy(self.geom.coords).to(dev).contiguous()
        self.cell = None if self.geom.cell is None else torch.from_numpy(self.geom.cell).to(dev)
        self.w = torch.from_numpy(self.ref.w).to(dev).contiguous()
        self.t = torch.from_numpy(self.ref.t.astype(np.float32)).to(dev).contiguous()
        self.modes = ("batch", "cell") if self.geom.species.shape[0] == 1 else ("batch",)

    def tuned_with_stated_flags(self):
        """The engine runs the tuned kernels, with the flags the table states for the set."""
        assert self.eng.tuned and self.eng.L == self.cset.out_dim
        assert (self.eng.params.flags & 3) == self.cset.flags, (self.tag, self.eng.params.flags, self.cset.flags)

    def rows(self, mode, lo=0, hi=None, x=None):
        nbrs = self.eng.neighbors(self.sp32, self.x if x is None else x, self.cell, self.geom.pbc, lo=lo, hi=hi, mode=mode,
                                  row_cap=256)
        torch.cuda.synchronize()
        nbrs.raise_on_overflow()
        return nbrs

    def shape_line(self):
        st = self.stats
        return (f"flags {self.cset.flags} S={self.cset.num_species} N={self.n} longest row {int(st.rad.max())}, angular "
                f"{int(st.ang.max())}")


def where_in_row(cset, col):
    R = 16 * cset.num_species
    if col < R:
        return f"radial part, species {col // 16}, shift {col % 16}"
    pairs = [(a, b) for a in range(cset.num_species) for b in range(a, cset.num_species)]
    return f"angular block of species pair {pairs[(col - R) // 32]}, term {(col - R) % 32}"


def check_aev_rows(ctx, got, ref, stats, label):
    """Every row against the oracle's, each relative to max(1, its own largest entry)."""
    ctx.tuned_with_stated_flags()
    err = np.abs(got.astype(np.float64) - ref)
    row_max = np.maximum(1.0, np.abs(ref).max(axis=1))
    rel = err.max(axis=1) / row_max
    k = int(np.argmax(rel))
    col = int(np.argmax(err[k]))
    assert rel[k] <= AEV_TOL, (f"{ctx.tag} {label}: row {k} ({int(stats.rad[k])} entries, {int(stats.ang[k])} angular) off by "
                               f"{err[k, col]:.2e} = {rel[k]:.2e} x its maximum {row_max[k]:.2f} in column {col}: "
                               f"{where_in_row(ctx.cset, col)} (reference {ref[k, col]:.6f})")
    return float(rel[k]), float(row_max[k])


def check_slab_flags(ctx, aev, mask, coords=None):
    """As test_slab_masks_flag_exactly_the_nonzero_blocks (tests/test_gpu_parity.py): a block outside the flags is identically
    zero, and the flags are exactly the blocks the fp64 rows have (no pair of these geometries lies within _nbr_cases.BAND of
    a cutoff: tests/test_aev_constants_host.py).  An odd species count leaves the last radial slab half filled."""
    eng, S = ctx.eng, ctx.cset.num_species
    R, rs = 16 * S, (S + 1) // 2
    a = aev.cpu().numpy()
    mk = mask.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    assert eng.n_slabs == rs + S * (S + 1) // 2
    for j in range(eng.n_slabs):
        blk = a[:, 32 * j:min(32 * j + 32, R)] if j < rs else a[:, R + 32 * (j - rs):R + 32 * (j - rs) + 32]
        flagged = (mk >> j) & 1 == 1
        assert np.all(blk[~flagged] == 0), f"{ctx.tag} slab {j}: non-zero AEV entries outside the mask"
    assert np.all(mk >> eng.n_slabs == 0)
    must = ac.expected_slabs(kc.row_stats(ctx.geom, ctx.cset, coords=coords, margin=-ac.nc.BAND), S)
    may = ac.expected_slabs(kc.row_stats(ctx.geom, ctx.cset, coords=coords, margin=+ac.nc.BAND), S)
    assert np.array_equal(must, may)
    bad = np.nonzero(mk != must)[0]
    assert bad.size == 0, f"{ctx.tag}: flags of atom {int(bad[0])}: {mk[bad[0]]:#x}, expected {must[bad[0]]:#x}"


def check_vjp(ctx, got, ref, label):
    ctx.tuned_with_stated_flags()
    mag = max(1.0, float(np.abs(ref).max()))
    err = np.abs(got.astype(np.float64) - ref).max(axis=1)
    k = int(np.argmax(err))
    msg = (f"{ctx.tag} {label}: atom {k} ({int(ctx.stats.rad[k])} entries, {int(ctx.stats.ang[k])} angular) off by {err[k]:.2e} "
           f"= {err[k] / mag:.2e} x max|vjp| {mag:.1f}")
    assert err[k] < VJP_TOL * mag, msg
    if ctx.cset.vjp_reg:   # (the fp32 oracle is under half of it on this set: tests/test_aev_constants_host.py)
        assert err[k] <= VJP_REG_REL * mag, "regression gate: " + msg
    return float(err[k] / mag), mag


def check_jvp(ctx, got, label):
    ctx.tuned_with_stated_flags()
    ref = ctx.ref.jvp
    mag = max(1.0, float(np.abs(ref).max()))
    err = np.abs(got.astype(np.float64) - ref)
    k = int(np.argmax(err.max(axis=1)))
    col = int(np.argmax(err[k]))
    assert err[k, col] < JVP_TOL * mag, (f"{ctx.tag} {label}: row {k} off by {err[k, col]:.2e} = {err[k, col] / mag:.2e} x "
                                         f"max|J t| {mag:.2f} in column {col}: {where_in_row(ctx.cset, col)}")
    return float(err[k, col] / mag), mag


# ---- forward ---------------------------------------------------------------------------------------------------------------

def forward_checked(ctx, mode):
    nbrs = ctx.rows(mode)
    mask = torch.full((ctx.n,), -1, dtype=torch.int32, device=ctx.dev)
    aev = ctx.eng.forward(ctx.sp32, nbrs, slab_mask=mask)
    torch.cuda.synchronize()
    rel, row_max = check_aev_rows(ctx, aev.cpu().numpy(), ctx.ref.aev, ctx.stats, f"{mode} forward")
    check_slab_flags(ctx, aev, mask)
    pad = ctx.geom.species.reshape(-1) < 0
    assert np.all(aev.cpu().numpy()[pad] == 0) and np.all(mask.cpu().numpy()[pad] == 0)
    return nbrs, aev, rel, row_max


@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
def test_forward(dev, run):
    """AevEngine.forward row by row against the oracle; the slab flags exactly the non-zero blocks (odd species counts: a
    half-filled last radial slab)."""
    ctx = Ctx(run, dev)
    for mode in ctx.modes:
        _, _, rel, row_max = forward_checked(ctx, mode)
        report(f"kfwd  {ctx.tag:36s} {mode:5s} {ctx.shape_line()}; max row err {rel:.2e} x row max {row_max:.2f}")


@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
def test_forward_update(dev, run):
    """Rows kept by forward_update and updated in place after a third of the atoms moved by up to 0.05 A: against the oracle
    at the moved coordinates at the gate of the forward, equal to a fresh forward there, the new flags exact."""
    ctx = Ctx(run, dev)
    eng, sp32, n = ctx.eng, ctx.sp32, ctx.n
    x_moved_np = kc.displaced(ctx.geom)
    x_moved = torch.from_numpy(x_moved_np).to(dev).contiguous()
    ref_moved = kc.reference(run, "f64", "displaced")
    st_moved = kc.row_stats(ctx.geom, ctx.cset, coords=x_moved_np)
    for mode in ctx.modes:
        eng.release_rows()
        first, _ = eng.forward_update(sp32, ctx.rows(mode), shard_rows=False)
        first = first.clone()
        nb_moved = ctx.rows(mode, x=x_moved)
        kept, kept_mask = eng.forward_update(sp32, nb_moved, shard_rows=False)
        m2 = torch.zeros(n, dtype=torch.int32, device=dev)
        fresh = eng.forward(sp32, nb_moved, slab_mask=m2)
        torch.cuda.synchronize()
        rel, row_max = check_aev_rows(ctx, kept.cpu().numpy(), ref_moved.aev, st_moved, f"{mode} forward_update")
        d = (kept - fresh).abs().cpu().numpy().astype(np.float64).max(axis=1) / np.maximum(1.0, np.abs(ref_moved.aev).max(axis=1))
        assert d.max() <= AEV_TOL, f"{ctx.tag} {mode}: updated rows differ from fresh ones by {d.max():.2e} x row max"
        assert torch.equal(kept_mask, m2), f"{ctx.tag} {mode}: flags of the updated rows differ from a fresh forward's"
        check_slab_flags(ctx, kept, kept_mask, coords=x_moved_np)
        assert not torch.equal(kept, first), "the move changed nothing"
        report(f"kupd  {ctx.tag:36s} {mode:5s} after the move: max row err {rel:.2e} x row max {row_max:.2f}; from a fresh "
               f"forward {d.max():.2e}")
        eng.release_rows()


# ---- backward --------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def range_vjp(run):
    """The oracle's VJP of the cotangent zeroed outside the central range of the run."""
    cset, geom = kc.set_by_name(run[0]), kc.geometry_of(run)
    lo, hi = kc.central_range(geom)
    w = np.zeros((geom.n_atoms, cset.out_dim))
    w[lo:hi] = kc.reference(run).w[lo:hi]
    _, g = kc._oracle("f64").aev(cset.oracle_params(), geom.species, geom.coords.astype(np.float64), geom.cell, geom.pbc,
                                 grad_aev=w)
    return g.reshape(geom.n_atoms, 3)


@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
def test_backward(dev, run):
    """AevEngine.backward of a seeded cotangent in [-1, 1] against the oracle: the float path, the fixed-point path (two calls
    bit-equal), the virial, and a range of central atoms inside the system (the gather and the push side of the pairs that
    cross its ends) against the oracle's VJP of the cotangent zeroed outside the range."""
    from torchani_amd.engine import fixed_to_float

    ctx = Ctx(run, dev)
    eng, sp32, n, w = ctx.eng, ctx.sp32, ctx.n, ctx.w
    vref = ctx.ref.virial
    vgate = VIRIAL_TOL * max(1.0, float(np.abs(vref).max()))
    lo, hi = kc.central_range(ctx.geom)
    for mode in ctx.modes:
        nbrs = ctx.rows(mode)
        g = eng.backward(sp32, nbrs, w)
        torch.cuda.synchronize()
        rel, mag = check_vjp(ctx, g.cpu().numpy(), ctx.ref.vjp, f"{mode} backward")
        acc = [eng.backward(sp32, nbrs, w, grad_coords=torch.zeros((n, 3), dtype=torch.int64, device=dev), fixed_point=True)
               for _ in range(2)]
        assert torch.equal(acc[0], acc[1]), f"{ctx.tag} {mode}: two fixed-point backward calls differ"
        rel_fx, _ = check_vjp(ctx, fixed_to_float(acc[0]).cpu().numpy(), ctx.ref.vjp, f"{mode} fixed-point backward")
        vir = torch.zeros((3, 3), dtype=torch.float64, device=dev)
        g_v = eng.backward(sp32, nbrs, w, virial=vir)
        check_vjp(ctx, g_v.cpu().numpy(), ctx.ref.vjp, f"{mode} backward with virial")
        verr = float(np.abs(vir.cpu().numpy() - vref).max())
        assert verr < vgate, f"{ctx.tag} {mode}: virial off by {verr:.2e} Ha, gate {vgate:.2e}"
        part = ctx.rows(mode, lo, hi)
        g_p = eng.backward(sp32, part, w[lo:hi].contiguous(), shard_rows=True)
        torch.cuda.synchronize()
        rel_p, _ = check_vjp(ctx, g_p.cpu().numpy(), range_vjp(run), f"{mode} backward of the central atoms {lo}..{hi}")
        report(f"kbwd  {ctx.tag:36s} {mode:5s} vjp err {rel:.2e}, fixed point {rel_fx:.2e}, atoms {lo}..{hi} {rel_p:.2e} x "
               f"max|vjp| {mag:.1f}; virial err {verr:.2e} Ha (gate {vgate:.1e}, max|virial| {np.abs(vref).max():.1f})")


@pytest.mark.parametrize("name", kc.PUSHED_SETS)
def test_backward_pushes_on_full_rows(dev, name):
    """Rows from a full list (AevEngine.rows_from_full: not symmetric, every radial term pushed to its neighbor) of the
    40-atom cluster, on the two boundary sets whose backward runs both recurrences."""
    run = (name, "cluster40")
    ctx = Ctx(run, dev)
    ilist, jlist, numneigh = (torch.from_numpy(a).to(dev) for a in kc.full_list(ctx.geom))
    rows = ctx.eng.rows_from_full(ctx.sp32, ctx.x, ilist, jlist, numneigh, row_cap=256)
    torch.cuda.synchronize()
    assert rows.symmetric is False and not rows.overflowed()
    g = ctx.eng.backward(ctx.sp32, rows, ctx.w)
    aev = ctx.eng.forward(ctx.sp32, rows)
    torch.cuda.synchronize()
    check_aev_rows(ctx, aev.cpu().numpy(), ctx.ref.aev, ctx.stats, "forward on rows from a full list")
    rel, mag = check_vjp(ctx, g.cpu().numpy(), ctx.ref.vjp, "backward on rows from a full list")
    report(f"kpush {ctx.tag:36s} push path: vjp err {rel:.2e} x max|vjp| {mag:.1f}")


# ---- JVP -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
def test_jvp(dev, run):
    """AevEngine.jvp and jvp_batched (two directions: t and -2 t) against the oracle's J t."""
    ctx = Ctx(run, dev)
    for mode in ctx.modes:
        nbrs = ctx.rows(mode)
        one = ctx.eng.jvp(ctx.sp32, nbrs, ctx.t)
        many = ctx.eng.jvp_batched(ctx.sp32, nbrs, torch.stack([ctx.t, -2.0 * ctx.t]))
        torch.cuda.synchronize()
        assert many.shape == (2, ctx.n, ctx.eng.L)
        rel, mag = check_jvp(ctx, one.cpu().numpy(), f"{mode} jvp")
        rel_b, _ = check_jvp(ctx, many[0].cpu().numpy(), f"{mode} jvp_batched, first direction")
        rel_c, _ = check_jvp(ctx, -0.5 * many[1].cpu().numpy(), f"{mode} jvp_batched, second direction")
        report(f"kjvp  {ctx.tag:36s} {mode:5s} J t err {rel:.2e}, batched {max(rel_b, rel_c):.2e} x max|J t| {mag:.2f}")


# ---- second order ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", kc.SECOND_ORDER_SETS)
def test_backward_second(dev, name):
    """AevEngine.backward_second along three directions, without and with a seeded dgrad, against the Richardson central
    difference of the oracle's VJP (tests/_second_order_ref.py fd; converged to a hundredth of the gate:
    tests/test_aev_constants_host.py), per direction."""
    run = (name, "cluster40")
    ctx = Ctx(run, dev)
    ref = kc.second_reference(run)
    t = torch.from_numpy(ref.t).to(dev)
    dg = torch.from_numpy(ref.dgrad).to(dev)
    for mode in ctx.modes:
        nbrs = ctx.rows(mode)
        ctx.tuned_with_stated_flags()
        worst = []
        for got, want, what in ((ctx.eng.backward_second(ctx.sp32, nbrs, ctx.w, t), ref.curv, "(D_t J^T) w"),
                                (ctx.eng.backward_second(ctx.sp32, nbrs, ctx.w, t, dg), ref.curv + ref.lin, "with dgrad")):
            got = got.cpu().numpy().astype(np.float64)
            assert got.shape == want.shape
            e = 0.0
            for k in range(want.shape[0]):
                m = max(1.0, float(np.abs(want[k]).max()))
                err = float(np.abs(got[k] - want[k]).max())
                e = max(e, err / m)
                assert err <= GATE * m, f"{ctx.tag} {mode} {what}: direction {k} off by {err:.2e} = {err / m:.2e} x {m:.1f}"
            worst.append(e)
        report(f"kso   {ctx.tag:36s} {mode:5s} err / max(1, max|ref|) per direction, worst: {worst[0]:.2e}, with dgrad "
               f"{worst[1]:.2e}; max|ref| {np.abs(ref.curv).max():.1f}")


# ---- the sweep -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("run", SWEEP_RUNS, ids=SWEEP_IDS)
def test_sweep(dev, run):
    """The 24 seeded trials of _aev_constants.sweep (every free constant drawn, both grids, both envelopes, 1 .. 7 species;
    flags 0, 1 and 3 at least four times each): forward rows with their flags, and the VJP."""
    ctx = Ctx(run, dev)
    for mode in ctx.modes:
        nbrs, _, rel, row_max = forward_checked(ctx, mode)
        g = ctx.eng.backward(ctx.sp32, nbrs, ctx.w)
        torch.cuda.synchronize()
        vrel, mag = check_vjp(ctx, g.cpu().numpy(), ctx.ref.vjp, f"{mode} backward")
        c = ctx.cset
        report(f"kswp  {ctx.tag:24s} {mode:5s} {c.grid[0]}x{c.grid[1]} {c.cutoff_fn:6s} Rcr {c.Rcr:.2f} Rca {c.Rca:.2f} EtaR "
               f"{c.EtaR:4.1f} EtaA {c.EtaA:4.1f} Zeta {c.Zeta:4.1f} {ctx.shape_line()}; max row err {rel:.2e} x {row_max:.2f}; "
               f"vjp err {vrel:.2e} x {mag:.1f}")
