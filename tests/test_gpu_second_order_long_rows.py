"""The second-order kernels on neighbor rows of 65 to 256 entries against the fp64 oracle: k_aev_bwd2<Dense | Item | Strain>
(csrc/aev_hess.hip), the item and strain forms of the general JVP kernel (k_aev_fwd_gen<true, Dir::Item | Dir::Strain>,
csrc/aev_generic.hip), k_hs_rlist / k_hs_pattern (csrc/hess_sparse.hip) and, through two whole models, the dense and the
block-sparse Hessian drivers.  Each walks a row in 64-entry pieces and has code only a long row runs: rows staged in LDS with
lane-strided loops, 8-bit per-species counts, the triangular pair decode with up to 255 atoms of one species, thousands of
fp32 LDS atomics onto one neighbor, duplicates removed across 64-lane ballots.  The cases are those of tests/_aev_cases.py
(two controls inside the first piece, then 65 to 256 entries, one-species blocks, periodic images, a cell smaller than the
cutoff); the references are central differences of the oracle's analytic first-order quantities
(tests/_second_order_ref.py), and tests/test_second_order_cases_host.py proves on the CPU that they have converged and which
case reaches which path.

Gates, none of them new and each applied PER DIRECTION (or slab, or row), so that a large block cannot hide an error in a
small one: second-order outputs 2e-5 x max(1, largest |entry| of the reference of that direction) (GATE of
tests/test_gpu_hessians.py); item and strain JVP rows 2e-5 x max(1, largest entry of the row) (JVP_TOL of
tests/test_gpu_aev_long_rows.py); ss 2e-5 x max |ss_ref| (REF_GATE of tests/test_gpu_strain_hessians.py); sparse against
dense 1e-6 x max |H| (DENSE_GATE of tests/test_gpu_sparse_hessians.py); the structure is compared exactly.  Measured:
profiles/second_order_long_rows_tests.txt."""
import functools

import numpy as np
import pytest
import torch

import _aev_cases as ac
import _second_order_ref as so
from _util import seeded_state
from test_gpu_parity import report

pytestmark = pytest.mark.gpu

RUN_IDS = [so.run_id(r) for r in so.RUNS]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from torchani_amd import _lib

    _lib.lib()  # fail loudly if the native library is missing
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def engine(num_species, variant=None):
    from torchani_amd.engine import AevEngine

    eng = AevEngine(so.constants(num_species, variant))
    eng.host_table()
    assert eng.tuned == (variant != "general")
    return eng


class Ctx:
    """One run on the device: the case, its constants and the seeded inputs of its reference."""

    def __init__(self, run, dev):
        name, variant = run
        self.tag = so.run_id(run)
        self.cr = cr = so.case_ref(name, variant)
        self.case = cr.case
        self.eng = engine(self.case.num_species, variant)
        assert self.eng.L == cr.L
        self.dev, self.n = dev, cr.n
        self.sp32 = torch.from_numpy(self.case.species.astype(np.int32)).to(dev).contiguous()
        self.x = torch.from_numpy(self.case.coords).to(dev).contiguous()
        self.cell = None if self.case.cell is None else torch.from_numpy(self.case.cell).to(dev)
        self.g = torch.from_numpy(cr.g).to(dev).contiguous()
        self.lens = so.row_lengths(cr.rows)
        # one long case on the rows of both builders (they order the entries inside a group differently)
        own = so.mode_of(self.case)
        self.modes = (own, "cell" if own == "batch" else "batch") if (name == so.BOTH_MODES and variant is None) else (own,)

    def rows(self, mode, lo=0, hi=None):
        nbrs = self.eng.neighbors(self.sp32, self.x, self.cell, self.case.pbc, lo=lo, hi=hi, mode=mode, row_cap=256)
        torch.cuda.synchronize()
        nbrs.raise_on_overflow()
        return nbrs

    def shape_line(self):
        return f"N={self.n} longest row {int(self.lens.max())}"


def slab_errors(ctx, got, ref, what):
    """Every direction (slab) of got [K, N, 3] against ref, each relative to max(1, its own largest |entry|): (largest
    error / gate magnitude over the slabs, the failure messages)."""
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    worst, bad = 0.0, []
    for k in range(ref.shape[0]):
        m = so.mag(ref[k])
        err = np.abs(got[k] - ref[k]).max(axis=1)
        a = int(np.argmax(err))
        worst = max(worst, float(err[a] / m))
        if not err[a] <= so.GATE * m:
            bad.append(f"{ctx.tag} {what}: direction {k}, atom {a} (row of {int(ctx.lens[a])}) off by {err[a]:.2e} = "
                       f"{err[a] / m:.2e} x max(1, max|ref|) = {m:.1f}")
    return worst, bad


def row_errors(ctx, got, ref, atoms, what):
    """JVP rows got [R, L] against ref [R, L] (row q belongs to central atom atoms[q]), each relative to max(1, its own
    largest entry)."""
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    m = np.maximum(1.0, np.abs(ref).max(axis=1))
    rel = np.abs(got - ref).max(axis=1) / m
    q = int(np.argmax(rel))
    bad = [] if rel[q] <= so.JVP_TOL else [
        f"{ctx.tag} {what}: row {q} (atom {int(atoms[q])}, row of {int(ctx.lens[atoms[q]])}) off by {rel[q]:.2e} x max(1, row "
        f"max) = {m[q]:.2f}"]
    return float(rel[q]), bad


# ---- dense directions ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("run", so.RUNS, ids=RUN_IDS)
def test_dense_second_backward(dev, run):
    """AevEngine.backward_second along four directions (the fgrads direction, a unit vector on the centre, one on an atom
    of the outer shell, a seeded sign vector) without and with a seeded dgrad, then the same call over disjoint ranges of
    central atoms, which must add up to the whole."""
    ctx = Ctx(run, dev)
    cr, eng = ctx.cr, ctx.eng
    ref = so.dense_ref(*run)
    t = torch.from_numpy(cr.t).to(dev)
    dg = torch.from_numpy(cr.dgrad).to(dev)
    for mode in ctx.modes:
        nbrs = ctx.rows(mode)
        e0, bad = slab_errors(ctx, eng.backward_second(ctx.sp32, nbrs, ctx.g, t), ref.curv, f"{mode} (D_t J^T) g")
        whole = eng.backward_second(ctx.sp32, nbrs, ctx.g, t, dg)
        e1, b = slab_errors(ctx, whole, ref.curv + ref.lin, f"{mode} with dgrad")
        bad += b
        tot = torch.zeros_like(whole)
        for lo, hi in ac.split_ranges(ctx.case):
            tot += eng.backward_second(ctx.sp32, ctx.rows(mode, lo, hi), ctx.g, t, dg)
        e2, b = slab_errors(ctx, tot, ref.curv + ref.lin, f"{mode} summed over ranges")
        bad += b
        e3, b = slab_errors(ctx, tot, whole.cpu().numpy().astype(np.float64), f"{mode} ranges against the whole call")
        bad += b
        report(f"so dense  {ctx.tag:30s} {mode:5s} {ctx.shape_line()}; err / max(1, max|ref|) per direction, worst: "
               f"{e0:.2e}, with dgrad {e1:.2e}, over ranges {e2:.2e} (ranges vs whole {e3:.2e}); max|ref| "
               f"{np.abs(ref.curv).max():.1f}")
        assert not bad, "\n".join(bad)


# ---- item rows -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("run", so.RUNS, ids=RUN_IDS)
def test_item_rows(dev, run):
    """jvp_items and backward_second_items on exactly the rows the sparse path hands them: hessian_pattern and
    hessian_items for the direction atoms centre (dir0 = 0), first shell and outer (dir0 = 3 a > 0).  The rows must be
    {(3 a + c, i): i in R(a)}; every JVP row and every slab is compared."""
    from torchani_amd.engine import hessian_items, hessian_pattern

    ctx = Ctx(run, dev)
    cr, eng = ctx.cr, ctx.eng
    table = torch.from_numpy(cr.dg_item).to(dev)
    for mode in ctx.modes:
        nbrs = ctx.rows(mode)
        pat = hessian_pattern(ctx.sp32, nbrs)
        for it in so.items_ref(*run):
            a = it.atom
            row_atom, row_dir = hessian_items(ctx.sp32, pat, int(eng.params.num_species), a, a + 1)
            ra, rd = row_atom.cpu().numpy().astype(np.int64), row_dir.cpu().numpy().astype(np.int64)
            assert sorted(zip(rd.tolist(), ra.tolist())) == sorted((3 * a + c, i) for c in range(3) for i in it.R), \
                f"{ctx.tag} {mode}: the item rows of atom {a} are not 3 x R(a)"
            ej, bad = row_errors(ctx, eng.jvp_items(ctx.sp32, nbrs, row_atom, row_dir), it.jvp[rd - 3 * a, ra], ra,
                                 f"{mode} jvp_items of atom {a}")
            dgrad = table[row_dir.long() - 3 * a, row_atom.long()].contiguous()
            errs = []
            for dg, want, what in ((torch.zeros_like(dgrad), it.second.curv, "items"),
                                   (dgrad, it.second.curv + it.second.lin, "items with dgrad")):
                out = torch.zeros((3, ctx.n, 3), dtype=torch.float32, device=dev)
                eng.backward_second_items(ctx.sp32, nbrs, ctx.g, row_atom, row_dir, 3 * a, dg, out)
                e, b = slab_errors(ctx, out, want, f"{mode} {what} of atom {a}")
                errs.append(e)
                bad += b
            report(f"so items  {ctx.tag:30s} {mode:5s} atom {a:3d} |R| {len(it.R):3d} dir0 {3 * a:3d}: J rows {ej:.2e} x row "
                   f"max; slabs {errs[0]:.2e}, with dgrad {errs[1]:.2e} x max(1, max|ref|) (max|ref| "
                   f"{np.abs(it.second.curv).max():.1f})")
            assert not bad, "\n".join(bad)


# ---- strain rows -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("run", so.STRAIN_RUNS, ids=[so.run_id(r) for r in so.STRAIN_RUNS])
def test_strain_rows(dev, run):
    """jvp_strain_items and backward_second_strain_items over the nine strain directions of every atom, the rows ordered
    as grad.energies_forces_and_strain_hessians orders them (a species' rows contiguous): every JVP row, the nine slabs
    of out and ss, without and with a seeded dgrad."""
    ctx = Ctx(run, dev)
    cr, eng = ctx.cr, ctx.eng
    ref = so.strain_ref(*run)
    flat = ctx.sp32.view(-1)
    atoms = torch.argsort(flat, stable=True).to(torch.int32)
    row_atom = atoms.repeat_interleave(9)
    row_dir = torch.arange(9, dtype=torch.int32, device=dev).repeat(atoms.numel())
    ra, rd = row_atom.cpu().numpy().astype(np.int64), row_dir.cpu().numpy().astype(np.int64)
    dgrad = torch.from_numpy(cr.dg_strain).to(dev)[row_dir.long(), row_atom.long()].contiguous()
    for mode in ctx.modes:
        nbrs = ctx.rows(mode)
        ej, bad = row_errors(ctx, eng.jvp_strain_items(ctx.sp32, nbrs, row_atom, row_dir), ref.jvp[rd, ra], ra,
                             f"{mode} jvp_strain_items")
        errs = []
        for dg, want, want_ss, what in ((torch.zeros_like(dgrad), ref.curv, ref.ss, "strain"),
                                        (dgrad, ref.curv + ref.lin, ref.ss + ref.ss_lin, "strain with dgrad")):
            out = torch.zeros((9, ctx.n, 3), dtype=torch.float32, device=dev)
            ss = torch.zeros((1, 9, 9), dtype=torch.float64, device=dev)
            eng.backward_second_strain_items(ctx.sp32, nbrs, ctx.g, row_atom, row_dir, dg, out, ss)
            e, b = slab_errors(ctx, out, want, f"{mode} {what}: out")
            bad += b
            d = np.abs(ss[0].cpu().numpy() - want_ss)
            es = float(d.max() / np.abs(want_ss).max())
            if not es <= so.SS_GATE:
                x, k = np.unravel_index(int(np.argmax(d)), d.shape)
                bad.append(f"{ctx.tag} {mode} {what}: ss[{x}][{k}] off by {d.max():.2e} = {es:.2e} x max|ss_ref| "
                           f"{np.abs(want_ss).max():.1f}")
            errs += [e, es]
        report(f"so strain {ctx.tag:30s} {mode:5s} {ctx.shape_line()}: J rows {ej:.2e} x row max; out {errs[0]:.2e}, with dgrad "
               f"{errs[2]:.2e} x max(1, max|ref|); ss {errs[1]:.2e}, with dgrad {errs[3]:.2e} x max|ss_ref| "
               f"{np.abs(ref.ss).max():.1f}")
        assert not bad, "\n".join(bad)


# ---- structure -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", so.PATTERN_CASES)
def test_pattern(dev, name):
    """hessian_pattern against the sets of the enumerated rows, exactly: R(a) starts with a, holds no atom twice and equals
    the set; P(a) is sorted and equals U_{i in R(a)} R(i); the status word is 0 (hessian_pattern raises otherwise)."""
    from torchani_amd.engine import hessian_pattern

    ctx = Ctx((name, None), dev)
    R = ctx.cr.R
    P = so.p_sets(R)
    for mode in ctx.modes:
        pat = hessian_pattern(ctx.sp32, ctx.rows(mode))
        roff, poff = pat.roff_host, pat.poff_host
        rlist = pat.rlist.cpu().numpy()
        index = pat.index.cpu().numpy()
        assert roff.shape == (ctx.n + 1,) and poff.shape == (ctx.n + 1,)
        for a in range(ctx.n):
            mine = rlist[roff[a]:roff[a + 1]].tolist()
            assert mine[0] == a and len(set(mine)) == len(mine) and set(mine) == R[a], f"{name} {mode}: R({a})"
            col = index[:, poff[a]:poff[a + 1]]
            assert np.all(col[1] == a) and col[0].tolist() == sorted(P[a]), f"{name} {mode}: P({a})"
        report(f"so pattern {name:29s} {mode:5s} N={ctx.n}: sum |R| {int(roff[-1])}, largest |R| {int(np.diff(roff).max())}, nnz "
               f"{pat.nnz}, largest |P| {int(np.diff(poff).max())}: equal to the sets")


# ---- whole models ----------------------------------------------------------------------------------------------------------

_models = {}


@pytest.mark.parametrize("name", so.MODEL_CASES)
def test_whole_model(dev, name):
    """grad.energies_forces_and_hessians of a seeded ANI-2x ensemble on six columns (the components of the centre and of
    the outer atom) against central differences of the oracle's forces, and energies_forces_and_sparse_hessians against the
    dense result."""
    from torchani_amd import grad
    from torchani_amd.models import ANI2x

    case = ac.case_by_name(name)
    cols, ref = so.model_ref(name)
    mode = so.mode_of(case)
    if mode not in _models:
        _models[mode] = ANI2x(state_dict=seeded_state("ani2x", 8, so.MODEL_SEED), device=dev, periodic_table_index=False,
                              neighborlist=mode, row_capacity=256)
    sp = torch.from_numpy(case.species.astype(np.int64)).to(dev)
    x = torch.from_numpy(case.coords).to(dev)
    dense = grad.energies_forces_and_hessians(_models[mode], sp, x)
    sparse = grad.energies_forces_and_sparse_hessians(_models[mode], sp, x)
    torch.cuda.synchronize()
    H = dense.hessians[0].double().cpu().numpy()
    worst, bad = 0.0, []
    for q, col in enumerate(cols):
        m = so.mag(ref.value[q])
        err = float(np.abs(H[:, col] - ref.value[q]).max())
        worst = max(worst, err / m)
        if not err <= so.GATE * m:
            bad.append(f"{name}: column {col} off by {err:.2e} = {err / m:.2e} x max(1, max|ref|) = {m:.2f}")
    spread = float(np.abs(sparse.hessians.to_dense()[0].double().cpu().numpy() - H).max() / np.abs(H).max())
    report(f"so model  {name:30s} {mode:5s} N={case.n_atoms}: six columns {worst:.2e} x max(1, max|ref|) (max|ref| "
           f"{np.abs(ref.value).max():.2f}); sparse against dense {spread:.2e} x max|H| {np.abs(H).max():.2f}")
    assert not bad, "\n".join(bad)
    assert spread <= so.DENSE_GATE
