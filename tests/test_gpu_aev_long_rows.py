"""The AEV kernels on neighbor rows of 65 to 256 entries against the fp64 oracle: k_aev_fwd3, k_aev_bwd and k_aev_jvp of
csrc/aev.hip and the general-grid kernels of csrc/aev_generic.hip walk a row in 64-entry chunks, and each has code that only
a long row runs (chunks fetched on the spot, the padded radial list, pairs dealt in batches of blocks, the one-part
tournament of the backward, 8-bit per-species counts).  The cases are those of tests/_aev_cases.py;
tests/test_aev_cases_host.py proves on the CPU which case reaches which path and prints what the fp32 build of the oracle
makes of them (AEV rows up to 3.3e-6 x row maximum, VJP about 5e-7, virial up to 1.6e-6, JVP up to 5.3e-6 of the largest
entry; the kernels measure 3.9e-6, 1.5e-6, 2.5e-6 and 2.1e-6: profiles/aev_long_rows_tests.txt).

Gates, none of them new: AEV rows 2e-5 x max(1, largest entry of the ROW) (tests/test_gpu_parity.py AEV_TOL; per row, so that
the centre's large entries cannot hide an error in a short row); VJP 2e-5 (parity) and 5e-6 (regression, VJP_REG_REL) x
max(1, largest entry); JVP 2e-5 x max(1, largest entry) (test_aev_jvp_matches_reference); virial 1e-4 Ha x max(1, largest
entry) (test_virial_matches_reference_stress)."""
import functools
import os
import typing as tp

import numpy as np
import pytest
import torch

import _aev_cases as ac
from _util import fgrad_direction, oracle_networks, oracle_params, seeded_state
from test_gpu_parity import report

pytestmark = pytest.mark.gpu

AEV_TOL = 2e-5        # tests/test_gpu_parity.py
VJP_TOL = 2e-5
VJP_REG_REL = 5e-6    # tests/test_gpu_parity.py: the regression gate of test_aev_forward_and_backward
JVP_TOL = 2e-5        # tests/test_gpu_training.py::test_aev_jvp_matches_reference
VIRIAL_TOL = 1e-4     # tests/test_gpu_md.py::test_virial_matches_reference_stress, "assert err < 1e-4" (Ha)
E_ATOM_REG = 1e-6     # tests/test_gpu_parity.py
F_REG = 5e-6
MODES = ("batch", "cell")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from torchani_amd import _lib

    _lib.lib()  # fail loudly if the native library is missing
    return torch.device("cuda:0")


# ---- constants, engines, references (each computed once and shared) ------------------------------------------------------

BENT_A = tuple(0.8 + 0.3375 * k + 0.05 * (k % 3) for k in range(8))   # test_aev_with_unequally_spaced_shifts


def constants(num_species, variant=None):
    from torchani_amd.constants import AEVConstants, aev_constants_1x, aev_constants_2x

    if variant == "1x":
        return aev_constants_1x(4)
    if variant == "general":   # the 5 / 3 x 5 grid of tests/golden/grid_r5_a3z5_dense.npz (GRID_CASES), seven species
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid_r5_a3z5_dense.npz")) as z:
            return AEVConstants(7, float(z["Rcr"]), float(z["Rca"]), float(z["EtaR"]), tuple(z["ShfR"].tolist()),
                                float(z["EtaA"]), float(z["Zeta"]), tuple(z["ShfA"].tolist()), tuple(z["ShfZ"].tolist()),
                                str(z["cutoff_fn"]))
    c = aev_constants_2x(num_species=num_species, cutoff_fn="smooth" if variant == "smooth" else "cosine")
    return c._replace(ShfA=BENT_A) if variant == "bent" else c


@functools.lru_cache(maxsize=None)
def engine(num_species, variant=None):
    from torchani_amd.engine import AevEngine

    eng = AevEngine(constants(num_species, variant))
    eng.host_table()   # (anihip_aev_table_pack sets the flags)
    assert eng.tuned == (variant != "general")
    if variant == "bent":    # neither the forward's nor the backward's Gaussian recurrence: every Gaussian evaluated directly
        assert (eng.params.flags & 3) == 0
    elif variant != "general":
        assert (eng.params.flags & 3) == 3
    return eng


@functools.lru_cache(maxsize=1)
def oracle64():
    from oracle.oracle import Oracle

    return Oracle("f64")


class Ref(tp.NamedTuple):
    aev: np.ndarray      # [N, L]
    w: np.ndarray        # [N, L] float32: the cotangent
    vjp: np.ndarray      # [N, 3]
    virial: np.ndarray   # [3, 3]
    t: np.ndarray        # [N, 3]: the direction
    jvp: np.ndarray      # [N, L]
    stats: ac.RowStats


@functools.lru_cache(maxsize=None)
def reference(name, variant=None):
    from oracle import oracle as orc

    case = ac.case_by_name(name)
    c = constants(case.num_species, variant)
    p = orc.make_params(c.num_species, c.Rcr, c.Rca, c.EtaR, c.EtaA, c.Zeta, c.ShfR, c.ShfA, c.ShfZ, c.cutoff_fn)
    n = case.n_atoms
    w = np.random.RandomState(1000).uniform(-1.0, 1.0, (n, c.out_dim)).astype(np.float32)
    t = fgrad_direction(case.species)
    x64 = case.coords.astype(np.float64)
    aev, vjp, vir = oracle64().aev(p, case.species, x64, case.cell, case.pbc, grad_aev=w.astype(np.float64), want_virial=True)
    _, jt = oracle64().aev_jvp(p, case.species, x64, t, case.cell, case.pbc)
    return Ref(aev.reshape(n, -1), w, vjp.reshape(n, 3), vir, t.reshape(n, 3), jt.reshape(n, -1),
               ac.row_stats(case, c.num_species, c.Rcr, c.Rca))


class Ctx:
    """One case on the device with one set of constants."""

    def __init__(self, name, dev, variant=None):
        self.case = ac.case_by_name(name)
        self.variant = variant
        self.tag = name if variant is None else f"{name} [{variant}]"
        self.eng = engine(self.case.num_species, variant)
        self.ref = reference(name, variant)
        self.dev = dev
        self.n = self.case.n_atoms
        self.sp32 = torch.from_numpy(self.case.species.astype(np.int32)).to(dev).contiguous()
        self.x = torch.from_numpy(self.case.coords).to(dev).contiguous()
        self.cell = None if self.case.cell is None else torch.from_numpy(self.case.cell).to(dev)
        self.pbc = self.case.pbc
        self.w = torch.from_numpy(self.ref.w).to(dev).contiguous()
        self.t = torch.from_numpy(self.ref.t.astype(np.float32)).to(dev).contiguous()

    def rows(self, mode, lo=0, hi=None, x=None, check=True):
        nbrs = self.eng.neighbors(self.sp32, self.x if x is None else x, self.cell, self.pbc, lo=lo, hi=hi, mode=mode,
                                  row_cap=256)
        if check:
            torch.cuda.synchronize()
            nbrs.raise_on_overflow()
        return nbrs

    def shape_line(self):
        st = self.ref.stats
        return (f"N={self.n} longest radial row {int(st.rad.max())}, angular {int(st.ang.max())}, largest group "
                f"{int((st.cnt_a + st.cnt_f).max())}")


def where_in_row(c, col):
    """Which part of an AEV row of constants c the column belongs to."""
    R, per = c.radial_len, len(c.ShfA) * len(c.ShfZ)
    if col < R:
        return f"radial part, species {col // len(c.ShfR)}, shift {col % len(c.ShfR)}"
    P = (col - R) // per
    pairs = [(a, b) for a in range(c.num_species) for b in range(a, c.num_species)]
    return f"angular block of species pair {pairs[P]}, term {(col - R) % per}"


def check_aev_rows(ctx, got, rows=None, label="aev"):
    """Every row against the oracle's, each relative to max(1, its own largest entry); returns the report figures."""
    ref = ctx.ref.aev
    rows = np.arange(ctx.n) if rows is None else rows
    err = np.abs(got[rows].astype(np.float64) - ref[rows])
    row_max = np.maximum(1.0, np.abs(ref[rows]).max(axis=1))
    rel = err.max(axis=1) / row_max
    k = int(np.argmax(rel))
    col = int(np.argmax(err[k]))
    st = ctx.ref.stats
    msg = (f"{ctx.tag} {label}: row {int(rows[k])} ({int(st.rad[rows[k]])} entries, {int(st.ang[rows[k]])} angular) off by "
           f"{err[k, col]:.2e} = {rel[k]:.2e} x its maximum {row_max[k]:.2f} in column {col}: "
           f"{where_in_row(ctx.eng.consts, col)} (reference {ref[rows[k], col]:.6f})")
    assert rel[k] <= AEV_TOL, msg
    return float(rel[k]), float(row_max[k])


def check_slab_flags(ctx, aev, mask):
    """Tuned layout: a block outside the flags is identically zero, and the flags are the blocks the fp64 rows have (a pair
    within _nbr_cases.BAND of a cutoff may count or not)."""
    eng, c = ctx.eng, ctx.eng.consts
    S, R = c.num_species, c.radial_len
    rs = (S + 1) // 2
    a = aev.cpu().numpy()
    mk = mask.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    for j in range(eng.n_slabs):
        blk = a[:, 32 * j:min(32 * j + 32, R)] if j < rs else a[:, R + 32 * (j - rs):R + 32 * (j - rs) + 32]
        flagged = (mk >> j) & 1 == 1
        assert np.all(blk[~flagged] == 0), f"{ctx.tag} slab {j}: non-zero AEV entries outside the mask"
    assert np.all(mk >> eng.n_slabs == 0)
    must = ac.expected_slabs(ac.row_stats(ctx.case, S, c.Rcr, c.Rca, margin=-ac.nc.BAND), S)
    may = ac.expected_slabs(ac.row_stats(ctx.case, S, c.Rcr, c.Rca, margin=+ac.nc.BAND), S)
    bad = np.nonzero(((must & ~mk) != 0) | ((mk & ~may) != 0))[0]
    assert bad.size == 0, f"{ctx.tag}: flags of atom {int(bad[0])}: {mk[bad[0]]:#x}, expected {must[bad[0]]:#x} .. {may[bad[0]]:#x}"


def check_vjp(ctx, got, label):
    ref = ctx.ref.vjp
    mag = max(1.0, float(np.abs(ref).max()))
    err = np.abs(got.astype(np.float64) - ref).max(axis=1)
    k = int(np.argmax(err))
    st = ctx.ref.stats
    msg = (f"{ctx.tag} {label}: atom {k} ({int(st.rad[k])} entries, {int(st.ang[k])} angular) off by {err[k]:.2e} = "
           f"{err[k] / mag:.2e} x max|vjp| {mag:.1f}")
    assert err[k] < VJP_TOL * mag, msg
    assert err[k] <= VJP_REG_REL * mag, "regression gate: " + msg
    return float(err[k] / mag), mag


def check_jvp(ctx, got, label):
    ref = ctx.ref.jvp
    mag = max(1.0, float(np.abs(ref).max()))
    err = np.abs(got.astype(np.float64) - ref)
    k = int(np.argmax(err.max(axis=1)))
    col = int(np.argmax(err[k]))
    assert err[k, col] < JVP_TOL * mag, (f"{ctx.tag} {label}: row {k} off by {err[k, col]:.2e} = {err[k, col] / mag:.2e} x "
                                         f"max|J t| {mag:.2f} in column {col}: {where_in_row(ctx.eng.consts, col)}")
    return float(err[k, col] / mag), mag


# ---- forward ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ac.CASE_NAMES)
def test_forward_rows(dev, name):
    """AevEngine.forward row by row against the oracle, the slab flags, sub-ranges of central atoms (shard_rows) bit-equal to
    the same rows of the whole-range call, and rows updated in place (forward_update) bit-equal to fresh ones after every
    atom moved by up to 0.05 A.  Both neighbor builders: they order the entries inside a group differently."""
    ctx = Ctx(name, dev)
    eng, sp32, n = ctx.eng, ctx.sp32, ctx.n
    x_moved = torch.from_numpy(ac.moved(ctx.case)).to(dev).contiguous()
    for mode in MODES:
        nbrs = ctx.rows(mode)
        mask = torch.full((n,), -1, dtype=torch.int32, device=dev)
        aev = eng.forward(sp32, nbrs, slab_mask=mask)
        torch.cuda.synchronize()
        rel, row_max = check_aev_rows(ctx, aev.cpu().numpy())
        report(f"fwd   {name:28s} {mode:5s} {ctx.shape_line()}; max row err {rel:.2e} x row max {row_max:.2f}")
        check_slab_flags(ctx, aev, mask)
        for lo, hi in ac.split_ranges(ctx.case):
            part = ctx.rows(mode, lo, hi)
            a_part = eng.forward(sp32, part, shard_rows=True)
            assert a_part.shape == (hi - lo, eng.L)
            assert torch.equal(a_part, aev[lo:hi]), (name, mode, lo, hi, float((a_part - aev[lo:hi]).abs().max()))
        eng.release_rows()
        eng.forward_update(sp32, nbrs, shard_rows=False)
        nb_moved = ctx.rows(mode, x=x_moved)
        kept, kept_mask = eng.forward_update(sp32, nb_moved, shard_rows=False)
        m2 = torch.zeros(n, dtype=torch.int32, device=dev)
        fresh = eng.forward(sp32, nb_moved, slab_mask=m2)
        assert torch.equal(kept, fresh), (name, mode, float((kept - fresh).abs().max()))
        assert torch.equal(kept_mask, m2)
        assert not torch.equal(fresh, aev), "the move changed nothing"
        eng.release_rows()


# ---- backward --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ac.CASE_NAMES)
def test_backward(dev, name):
    """AevEngine.backward of a seeded cotangent in [-1, 1] against the oracle at the parity and at the regression gate: the
    float path, the fixed-point path (two calls bit-equal), the virial (bound: tests/test_gpu_md.py,
    test_virial_matches_reference_stress, "assert err < 1e-4", here x max(1, largest entry of the reference virial)), with
    the forward's slab flags and the cotangent zeroed outside them, and summed over disjoint ranges of central atoms (the
    gather and the push side of a pair whose atoms lie in different ranges), virial included."""
    from torchani_amd.engine import fixed_to_float

    ctx = Ctx(name, dev)
    eng, sp32, n, w = ctx.eng, ctx.sp32, ctx.n, ctx.w
    vref = ctx.ref.virial
    vgate = VIRIAL_TOL * max(1.0, float(np.abs(vref).max()))
    for mode in MODES:
        nbrs = ctx.rows(mode)
        g = eng.backward(sp32, nbrs, w)
        torch.cuda.synchronize()
        rel, mag = check_vjp(ctx, g.cpu().numpy(), f"{mode} backward")
        reg = VJP_REG_REL * mag
        # fixed point
        acc = [eng.backward(sp32, nbrs, w, grad_coords=torch.zeros((n, 3), dtype=torch.int64, device=dev), fixed_point=True)
               for _ in range(2)]
        assert torch.equal(acc[0], acc[1]), f"{ctx.tag} {mode}: two fixed-point backward calls differ"
        rel_fx, _ = check_vjp(ctx, fixed_to_float(acc[0]).cpu().numpy(), f"{mode} fixed-point backward")
        # virial
        vir = torch.zeros((3, 3), dtype=torch.float64, device=dev)
        g_v = eng.backward(sp32, nbrs, w, virial=vir)
        check_vjp(ctx, g_v.cpu().numpy(), f"{mode} backward with virial")
        verr = float(np.abs(vir.cpu().numpy() - vref).max())
        report(f"bwd   {name:28s} {mode:5s} vjp err {rel:.2e}, fixed point {rel_fx:.2e} x max|vjp| {mag:.1f}; virial err "
               f"{verr:.2e} Ha (gate {vgate:.1e}, max|virial| {np.abs(vref).max():.1f})")
        assert verr < vgate, f"{ctx.tag} {mode}: virial off by {verr:.2e} Ha, gate {vgate:.2e}"
        # slab flags of the forward; the cotangent zeroed outside the flagged blocks
        mask = torch.zeros(n, dtype=torch.int32, device=dev)
        eng.forward(sp32, nbrs, slab_mask=mask)
        g_m = eng.backward(sp32, nbrs, zero_outside_flags(ctx, w, mask), slab_mask=mask)
        d = float((g_m - g).abs().max())
        assert d <= reg, f"{ctx.tag} {mode}: backward with slab flags differs by {d:.2e} (gate {reg:.2e})"
        # disjoint ranges of central atoms add up
        tot = torch.zeros((n, 3), dtype=torch.float32, device=dev)
        vtot = torch.zeros((3, 3), dtype=torch.float64, device=dev)
        for lo, hi in ac.split_ranges(ctx.case):
            part = ctx.rows(mode, lo, hi)
            vpart = torch.zeros((3, 3), dtype=torch.float64, device=dev)
            eng.backward(sp32, part, w[lo:hi].contiguous(), grad_coords=tot, shard_rows=True, virial=vpart)
            vtot += vpart
        d = float((tot - g).abs().max())
        assert d <= reg, f"{ctx.tag} {mode}: ranges add up to something {d:.2e} off the whole (gate {reg:.2e})"
        check_vjp(ctx, tot.cpu().numpy(), f"{mode} backward summed over ranges")
        dv = float((vtot - vir).abs().max())
        assert dv < vgate, f"{ctx.tag} {mode}: virials of the ranges add up to something {dv:.2e} Ha off the whole"


def zero_outside_flags(ctx, w, mask):
    """w with every block of every row zeroed whose slab flag is clear (tuned layout)."""
    c = ctx.eng.consts
    S, R = c.num_species, c.radial_len
    rs = (S + 1) // 2
    out = w.clone()
    mk = mask.to(torch.int64) & 0xFFFFFFFF
    for j in range(ctx.eng.n_slabs):
        cols = slice(32 * j, min(32 * j + 32, R)) if j < rs else slice(R + 32 * (j - rs), R + 32 * (j - rs) + 32)
        out[:, cols] *= ((mk >> j) & 1).to(out.dtype).view(-1, 1)
    return out


# ---- JVP -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ac.CASE_NAMES)
def test_jvp(dev, name):
    """AevEngine.jvp and jvp_batched (one direction) against the oracle's J t at the bound of test_aev_jvp_matches_reference:
    the tangent kernel on rows of up to 128 angular neighbors and on single-species blocks."""
    ctx = Ctx(name, dev)
    for mode in MODES:
        nbrs = ctx.rows(mode)
        one = ctx.eng.jvp(ctx.sp32, nbrs, ctx.t)
        many = ctx.eng.jvp_batched(ctx.sp32, nbrs, ctx.t[None])
        torch.cuda.synchronize()
        assert many.shape == (1, ctx.n, ctx.eng.L)
        rel, mag = check_jvp(ctx, one.cpu().numpy(), f"{mode} jvp")
        rel_b, _ = check_jvp(ctx, many[0].cpu().numpy(), f"{mode} jvp_batched")
        report(f"jvp   {name:28s} {mode:5s} J t err {rel:.2e}, batched {rel_b:.2e} x max|J t| {mag:.2f}")


# ---- other constants: the 4 x 8 grid, the smooth cutoff, unequally spaced shifts, a general grid ----------------------------

def forward_backward_jvp(ctx, mode, label):
    eng, sp32 = ctx.eng, ctx.sp32
    nbrs = ctx.rows(mode)
    mask = torch.full((ctx.n,), -1, dtype=torch.int32, device=ctx.dev)
    aev = eng.forward(sp32, nbrs, slab_mask=mask)
    g = eng.backward(sp32, nbrs, ctx.w)
    jt = eng.jvp(sp32, nbrs, ctx.t)
    torch.cuda.synchronize()
    rel, row_max = check_aev_rows(ctx, aev.cpu().numpy())
    if eng.tuned:
        check_slab_flags(ctx, aev, mask)
    vrel, vmag = check_vjp(ctx, g.cpu().numpy(), f"{mode} backward")
    jrel, jmag = check_jvp(ctx, jt.cpu().numpy(), f"{mode} jvp")
    report(f"{label:5s} {ctx.tag:38s} {mode:5s} {ctx.shape_line()}; max row err {rel:.2e} x row max {row_max:.2f}; vjp err "
           f"{vrel:.2e} x {vmag:.1f}; J t err {jrel:.2e} x {jmag:.2f}")


@pytest.mark.parametrize("name,variant", ac.VARIANT_NAMES, ids=[f"{n}-{v}" for n, v in ac.VARIANT_NAMES])
def test_other_constants(dev, name, variant):
    """The 4 x 8 instantiations (ANI-1x constants), the smooth cutoff, and unequally spaced angular shifts (no Gaussian
    recurrence in either kernel: anihip_aev_table_pack clears both flags) on long rows: forward rows, flags, backward and
    JVP against the oracle with the gates of the tests above."""
    ctx = Ctx(name, dev, variant)
    for mode in MODES:
        forward_backward_jvp(ctx, mode, "var")


@pytest.mark.parametrize("name", ac.GENERAL_NAMES)
def test_general_grid(dev, name):
    """csrc/aev_generic.hip strides rows by 64 as well: the 5 / 3 x 5 grid of GRID_CASES' r5_a3z5_dense (seven species) on
    ang128 in three labellings, chunk256 with seven species and the pad case."""
    ctx = Ctx(name, dev, "general")
    for mode in MODES:
        forward_backward_jvp(ctx, mode, "grid")


# ---- rows that overflow ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ac.OVER_NAMES)
def test_overflowing_row(dev, name):
    """One over a row limit (129 angular neighbors, 256 of one species, 257 entries): the builder zeroes the centre's row and
    sets ANIHIP_ST_ROW_OVERFLOW; the forward leaves the centre's AEV row all zero, and every other row -- the centre is still
    their neighbor -- matches the oracle's."""
    ctx = Ctx(name, dev)
    c = ctx.case.centre
    others = np.arange(ctx.n) != c
    for mode in MODES:
        nbrs = ctx.rows(mode, check=False)
        aev = ctx.eng.forward(ctx.sp32, nbrs)
        torch.cuda.synchronize()
        assert nbrs.overflowed()
        got = aev.cpu().numpy()
        assert np.all(got[c] == 0), f"{name} {mode}: the overflowed row is not zero"
        assert np.abs(ctx.ref.aev[c]).max() > 0.1   # (the zero row is not what the oracle has there)
        rel, row_max = check_aev_rows(ctx, got, rows=np.nonzero(others)[0])
        report(f"over  {name:28s} {mode:5s} centre row zero; other rows: max row err {rel:.2e} x row max {row_max:.2f}")


# ---- one whole model -------------------------------------------------------------------------------------------------------

_models = {}


@pytest.mark.parametrize("name", ["dense", "ang128_at_open/seven"])
def test_whole_model(dev, name):
    """energies_and_forces of a seeded ANI-2x ensemble against the oracle: the slab flags of long rows through the network
    stage.  E_ATOM_REG and F_REG of tests/test_gpu_parity.py x max(1, largest reference value)."""
    from torchani_amd.models import ANI2x

    seed = 31
    case = ac.case_by_name(name)
    dims, flat, _ = oracle_networks("ani2x", 8, seed)
    ref = oracle64().energy_forces(oracle_params("ani2x"), case.species, case.coords.astype(np.float64), dims, flat, 8, sae=None)
    emag = max(1.0, float(np.abs(ref["atomic_energies"]).max()))
    fmag = max(1.0, float(np.abs(ref["forces"]).max()))
    sp = torch.from_numpy(case.species.astype(np.int64)).to(dev)
    x = torch.from_numpy(case.coords).to(dev)
    for mode in MODES:
        if mode not in _models:
            _models[mode] = ANI2x(state_dict=seeded_state("ani2x", 8, seed), device=dev, periodic_table_index=False,
                                  neighborlist=mode, row_capacity=256)
        out = _models[mode].energies_and_forces(sp, x, check_overflow=True)
        torch.cuda.synchronize()
        ea = float(np.abs(out.atomic_energies.cpu().numpy() - ref["atomic_energies"]).max())
        fe = float(np.abs(out.forces.cpu().numpy() - ref["forces"]).max())
        report(f"model {name:28s} {mode:5s} max|e_atom err| = {ea:.2e} (max {emag:.2f})  |F err| = {fe:.2e} (max {fmag:.2f})")
        assert ea <= E_ATOM_REG * emag and fe <= F_REG * fmag
