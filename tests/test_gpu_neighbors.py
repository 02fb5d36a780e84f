"""The neighbor builders of csrc/nbr.hip pair for pair against the fp64 oracle's brute-force list, on the sweep of
tests/_nbr_cases.py: skewed, thin and uneven cells, partial periodicity, atoms outside the cell, empty and crowded bins, a
coarsened grid, padding atoms, partial central ranges, the 64-hit chunk boundaries of the row writers and the three row
limits exactly reached and one over.  Every case runs through AevEngine.neighbors in mode "cell"; cases of at most 1 300
atoms also in mode "batch".  tests/test_neighbor_cases_host.py holds the oracle itself to these geometries on the CPU.

Per build (tests/_nbr_rows.py compare_rows): the (j, image) set of every row equals the oracle's outside the borderline band
(a pair within BAND = 2e-5 A of Rcr may be present or absent, within BAND of Rca in either group: 2 sqrt(3) times the
displacement gate, at most 1e-3 of a case's pairs, asserted on the CPU); group split, species order, packed counts;
displacements within 5e-6 A -- in batch mode, where the wrapped position is held in absolute fp32, within max(5e-6, 4 ulp of
the largest wrapped coordinate); no overflow bit except in the one-over cases; and which of the two cell kernels took the
bins, from status[2] (bins) and status[3] (bins left to the per-atom kernel).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _nbr_cases as nc
from _nbr_rows import compare_rows, decode_rows, pair_keys
from test_gpu_parity import report, unpack_rows
from torchani_amd import _lib
from torchani_amd.constants import aev_constants_2x

pytestmark = pytest.mark.gpu

SWEEP = nc.random_cases() + nc.chunk_cases() + nc.limit_cases()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.lib()  # fail loudly if the native library is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def eng():
    from torchani_amd.engine import AevEngine

    consts = aev_constants_2x(num_species=nc.NUM_SPECIES)
    assert consts.Rcr == nc.RCR and consts.Rca == nc.RCA
    return AevEngine(consts)


def to_dev(case, dev):
    sp = torch.from_numpy(case.species).to(dev).contiguous()
    x = torch.from_numpy(case.coords).to(dev).contiguous()
    cell = None if case.cell is None else torch.from_numpy(case.cell).to(dev)
    return sp, x, cell, case.pbc


def oracle_list(oracle64, case):
    """The reference: brute force in fp64 on the case's fp32 coordinates, out to Rcr + BAND so that the band is seen."""
    return oracle64.neighbors(case.species, case.coords.astype(np.float64), case.rcr + nc.BAND, case.cell, case.pbc,
                              cell_list=False)


def disp_gate(case, mode, xw):
    if mode == "cell":
        return nc.DISP_GATE
    # batch mode keeps the wrapped position in absolute fp32: the bound comes from the input
    return max(nc.DISP_GATE, 4.0 * float(np.spacing(np.float32(np.abs(xw).max()))))


def modes_of(case):
    return ["cell", "batch"] if case.n_atoms <= nc.BATCH_MAX_ATOMS else ["cell"]


def build(eng, case, dev, mode, lo=0, hi=None):
    sp, x, cell, pbc = to_dev(case, dev)
    kw = {"max_cells": case.max_cells} if mode == "cell" else {}
    nbrs = eng.neighbors(sp, x, cell, pbc, lo=lo, hi=hi, mode=mode, row_cap=case.row_cap, **kw)
    torch.cuda.synchronize()
    return nbrs


def check_build(case, mode, nbrs, ref, lo=0, hi=None, quiet=False):
    """All per-build assertions of the module header; returns the status words."""
    n = case.n_atoms
    hi = n if hi is None else hi
    tag = f"{case.name}/{mode}"
    status = nbrs.status.cpu().numpy().view(np.uint32)
    meta, ent = unpack_rows(nbrs, n)
    xw = nc.wrap_f64(case)
    cell64 = case.cell.astype(np.float64) if case.periodic else None
    skip = tuple(i for i in case.overflow_rows if lo <= i < hi)
    flagged = bool(status[0] & (_lib.ST_ROW_OVERFLOW | _lib.ST_ENTRY_OVERFLOW))
    assert flagged == bool(skip), f"{tag}: status[0] = {status[0]}, rows expected to overflow: {skip}"
    for i in skip:
        assert np.all(meta[i, 1:6] == 0), f"{tag}: the overflowing row {i} must come back zeroed"
    assert np.array_equal(meta[lo:hi, 0].astype(np.int64), (np.arange(lo, hi) - lo) * nbrs.row_cap)
    res = compare_rows(tag, meta, ent, lo, hi, case.species, ref, xw, cell64, case.rcr, case.rca, band_rcr=nc.BAND,
                       band_rca=nc.BAND, skip_rows=skip)
    gate = disp_gate(case, mode, xw)
    bins, left = int(status[2]), int(status[3])
    if not quiet:
        report(f"nbrs  {case.name:24s} {mode:5s} atoms {n:5d} pairs {res.pairs:6d} bins {bins if mode == 'cell' else 0:5d} "
               f"left to per-atom kernel {left if mode == 'cell' else 0:4d} excused {res.excused:3d} "
               f"max|d - d_ref| = {res.worst:.2e} A (gate {gate:.1e})")
    assert res.worst <= gate, f"{tag}: displacement error {res.worst:.2e} A over {gate:.1e}"
    if mode == "cell":
        # (the grid rule of include/anihip.h, restated in tests/_nbr_cases.py grid_model)
        max_cells = case.max_cells if case.max_cells is not None else max(4096, 2 * n)
        coarsened = int(np.prod(nc.grid_model(case, max_cells=1 << 29)[0])) > max_cells
        assert coarsened or not case.coarsened
        assert bool(status[0] & _lib.ST_GRID_OVERFLOW) == coarsened, f"{tag}: grid coarsening flag"
        assert bins <= max_cells
        if case.periodic and all(case.pbc):
            assert bins == int(np.prod(nc.grid_model(case)[0])), f"{tag}: {bins} bins"
        if lo == 0 and hi == n:
            if case.kernel == "bin":
                assert left == 0, f"{tag}: {left} of {bins} bins went to the per-atom kernel, none expected"
            elif case.kernel == "atom":
                assert left == bins, f"{tag}: only {left} of {bins} bins went to the per-atom kernel"
            elif case.kernel == "both":
                assert 0 < left < bins, f"{tag}: {left} of {bins} bins went to the per-atom kernel, both kernels expected"
    return status


@pytest.mark.parametrize("case", SWEEP, ids=[c.name for c in SWEEP])
def test_rows_match_oracle(dev, eng, oracle64, case):
    ref = oracle_list(oracle64, case)
    for mode in modes_of(case):
        check_build(case, mode, build(eng, case, dev, mode), ref)


def raw_cell_build(eng, case, dev, lo, hi, fill):
    """anihip_nbr_build_cell into buffers pre-filled with a pattern, so that what the build leaves alone can be seen."""
    sp, x, cell, pbc = to_dev(case, dev)
    n = case.n_atoms
    mask = sum((1 << k) for k in range(3) if pbc is not None and pbc[k]) if cell is not None else 0
    cell_t = cell.contiguous() if mask else None
    meta = torch.full((n, _lib.META_WORDS), fill, dtype=torch.int32, device=dev)
    ent = torch.full(((hi - lo) * case.row_cap, 4), fill, dtype=torch.int32, device=dev)
    status = torch.zeros(_lib.STATUS_WORDS, dtype=torch.int32, device=dev)
    L = _lib.lib()
    max_cells = max(4096, 2 * n)
    ws = torch.empty(L.anihip_nbr_workspace_bytes(n, max_cells), dtype=torch.uint8, device=dev)
    _lib.check(L.anihip_nbr_build_cell(
        torch.cuda.current_stream().cuda_stream, C.byref(eng.params), n, sp.data_ptr(), x.data_ptr(),
        None if cell_t is None else cell_t.data_ptr(), mask, lo, hi, max_cells, ws.data_ptr(), ws.numel(),
        meta.data_ptr(), ent.data_ptr(), (hi - lo) * case.row_cap, status.data_ptr()))
    torch.cuda.synchronize()
    return meta.cpu().numpy(), ent.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("name", ["ortho", "skew_TTT", "droplet_TTT", "droplet_none"])
def test_central_range(dev, eng, oracle64, name):
    """lo, hi = the middle third: exactly those atoms' rows, identical to the full build's, and nothing else written -- no
    other atom's metadata, no entry past the end of a row."""
    case = nc.case_by_name(name)
    n = case.n_atoms
    lo, hi = n // 3, 2 * n // 3
    ref = oracle_list(oracle64, case)
    for mode in modes_of(case):
        part = build(eng, case, dev, mode, lo, hi)
        check_build(case, mode, part, ref, lo, hi, quiet=True)
        full = build(eng, case, dev, mode)
        mp, ep = unpack_rows(part, n)
        mf, ef = unpack_rows(full, n)
        assert np.array_equal(mp[lo:hi, 1:], mf[lo:hi, 1:]), f"{name}/{mode}: metadata of a partial build differs"
        rp, rf = decode_rows(mp, ep, lo, hi), decode_rows(mf, ef, lo, hi)
        assert np.array_equal(rp.j, rf.j) and np.array_equal(rp.d, rf.d), f"{name}/{mode}: rows of a partial build differ"
    fill = 0x7FC0DEAD   # (a NaN pattern no entry holds)
    meta, ent, status = raw_cell_build(eng, case, dev, lo, hi, fill)
    assert not (int(status[0]) & (_lib.ST_ROW_OVERFLOW | _lib.ST_ENTRY_OVERFLOW))
    assert np.all(meta[:lo] == fill) and np.all(meta[hi:] == fill), f"{name}: a build of {lo}..{hi} wrote other atoms' metadata"
    m = meta.view(np.uint32)[lo:hi].astype(np.int64)
    cnt = (m[:, 1] & 0xFFFF) + (m[:, 1] >> 16)
    ent_rows = ent.reshape(hi - lo, case.row_cap, 4)
    past = np.arange(case.row_cap)[None, :] >= cnt[:, None]
    assert np.all(ent_rows[past] == fill), f"{name}: entries past the end of a row were written"
    assert not np.any(np.all(ent_rows[~past] == fill, axis=-1))
    report(f"nbrs  {name:24s} range {lo}..{hi}: rows identical to the full build's, nothing else written")


@pytest.mark.parametrize("name", ["ortho", "skew_TTT"])
def test_rows_to_half(dev, eng, oracle64, name):
    """rows_to_half of the rows: every unordered pair of the oracle once -- half its ordered pairs."""
    from torchani_amd.engine import rows_to_half

    case = nc.case_by_name(name)
    n = case.n_atoms
    start, j, d, r = oracle_list(oracle64, case)
    nbrs = build(eng, case, dev, "cell")
    idx, dist, diff = rows_to_half(nbrs, n)
    torch.cuda.synchronize()
    idx, diff = idx.cpu().numpy(), diff.cpu().numpy().astype(np.float64)
    xw = nc.wrap_f64(case)
    cell64 = case.cell.astype(np.float64)
    oi = np.repeat(np.arange(n), np.diff(start))
    okey, _ = pair_keys(oi, j.astype(np.int64), d.astype(np.float64), xw, cell64, n)
    must = okey[r <= case.rcr - nc.BAND]
    # diff = r_i - r_j (+ shift): the ordered pair (i, j) has displacement -diff, its mirror (j, i) has +diff
    fwd, _ = pair_keys(idx[0], idx[1], -diff, xw, cell64, n)
    bwd, _ = pair_keys(idx[1], idx[0], diff, xw, cell64, n)
    both = np.concatenate([fwd, bwd])
    assert np.unique(both).size == both.size, f"{name}: an unordered pair is listed twice"
    assert np.all(np.isin(must, both)) and np.all(np.isin(both, okey))
    n_exact = int((r <= case.rcr).sum())
    n_band = int((np.abs(r - case.rcr) <= nc.BAND).sum())
    assert n_exact % 2 == 0 and abs(2 * idx.shape[1] - n_exact) <= n_band
    if n_band == 0:
        assert 2 * idx.shape[1] == n_exact
    assert np.abs(np.linalg.norm(diff, axis=1) - dist.cpu().numpy()).max() < 1e-5
    report(f"nbrs  {name:24s} rows_to_half: {idx.shape[1]} pairs, oracle {n_exact} ordered pairs")


@pytest.mark.parametrize("case", nc.edge_cases(), ids=[c.name for c in nc.edge_cases()])
def test_cutoff_edges(dev, eng, oracle64, case):
    """Pairs 1e-3 A inside and outside each cutoff, along a lattice axis, inside the cell and across its boundary: in / out
    and angular / far, nothing excused."""
    ref = oracle_list(oracle64, case)
    assert np.all(np.abs(ref[3] - case.rcr) > 5e-4) and np.all(np.abs(ref[3] - case.rca) > 5e-4)
    for mode in modes_of(case):
        nbrs = build(eng, case, dev, mode)
        check_build(case, mode, nbrs, ref)
        meta, ent = unpack_rows(nbrs, case.n_atoms)
        rows = decode_rows(meta, ent, 0, case.n_atoms)
        for p, (present, angular) in enumerate(nc.EDGE_EXPECT):
            for a, b in ((2 * p, 2 * p + 1), (2 * p + 1, 2 * p)):
                hit = (rows.i == a) & (rows.j == b)
                assert int(hit.sum()) == int(present), f"{case.name}/{mode}: pair {p} ({a}, {b})"
                assert int((rows.i == a).sum()) == int(present)
                if present:
                    assert bool(rows.ang[hit][0]) == angular, f"{case.name}/{mode}: pair {p} in the wrong group"
