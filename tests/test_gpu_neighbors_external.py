"""The entry points of csrc/nbr.hip that take or give somebody else's list, pair for pair against the fp64 oracle:
anihip_nbr_from_half (k_half_scatter, k_half_finish), anihip_nbr_from_full (k_nbr_full), anihip_nbr_refresh (k_nbr_refresh)
and anihip_nbr_rows_to_half (k_half_count, k_scan_blocks, k_scan_sums, k_half_write), and the consumers' paths for rows that
are not symmetric (k_aev_bwd pushing its radial terms, k_pair with ANIHIP_PAIR_PUSH).  Cases: the random cases of
tests/_nbr_cases.py and its chunk and limit families without the outer shell, open and periodic; the host constructions are
those of tests/_nbr_external.py, which tests/test_nbr_external_host.py holds to the oracle on the CPU.

Per build (tests/_nbr_rows.py compare_rows): the (j, image) set of every row, group split, species order, packed counts; no
overflow bit except where a case names overflow_rows, those rows zeroed and every other row intact.  Gates: rows from a half
list DISP_GATE (the list's fp32 diff is the oracle's displacement rounded once); rows from a full list batch mode's
max(DISP_GATE, 4 ulp of the largest coordinate); refreshed rows REFRESH_GATE = DISP_GATE + 4 spacing(fp32(Rcr + skin)) against
the oracle at the moved coordinates, with the band 2 sqrt(3) times that.

Round trip rows -> half list -> rows: the half list carries one displacement per pair, so the row of the pair's other atom
gets its exact negative, while a builder computes that entry on its own (with an image shift, (x_j + s) - x_i and
(x_i - s) - x_j round differently).  So every row must hold the kept entries bit for bit and the mirrored ones within twice
DISP_GATE; for the open case built in batch mode (d = x_j - x_i straight from the coordinates, and fl(a - b) = -fl(b - a)) and
for a second trip from the rows of the first, every row is the same multiset of entries bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _nbr_cases as nc
import _nbr_external as nx
from _nbr_rows import compare_rows, pair_keys
from test_gpu_neighbors import build, modes_of, to_dev
from test_gpu_parity import report, unpack_rows
from torchani_amd import _lib
from torchani_amd.constants import aev_constants_2x

pytestmark = pytest.mark.gpu

SWEEP = nx.sweep()
IDS = [c.name for c in SWEEP]
FILL = 0x7FC0DEAD   # (a NaN pattern no entry holds)
OVER = _lib.ST_ROW_OVERFLOW | _lib.ST_ENTRY_OVERFLOW


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


_lists = {}


def ref_list(oracle64, case, cutoff, coords=None, species=None, tag=""):
    """The oracle's list of a case, computed once per (case, cutoff, variant) and left unchanged."""
    key = (case.name, round(cutoff, 9), tag)
    if key not in _lists:
        _lists[key] = nx.oracle_list(oracle64, case, cutoff, coords=coords, species=species)
    return _lists[key]


def raw_rows(meta, ent, lo, hi):
    """The used entries of rows lo..hi as they lie in memory: (i, j, fp32 displacement [E, 3])."""
    m = meta[lo:hi].astype(np.int64)
    cnt = (m[:, 1] & 0xFFFF) + (m[:, 1] >> 16)
    i = np.repeat(np.arange(lo, hi), cnt)
    k = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    e = ent[np.repeat(m[:, 0], cnt) + k]
    j = (np.ascontiguousarray(e[:, 3]).view(np.uint32) & 0x0FFFFFFF).astype(np.int64)
    return i, j, np.ascontiguousarray(e[:, :3]), np.ascontiguousarray(e[:, 3]).view(np.uint32)


def row_bytes(nbrs, n, lo=None, hi=None):
    """Everything rows lo..hi say, byte for byte: the metadata words past the offset and the used entries in order."""
    meta, ent = unpack_rows(nbrs, n)
    lo = nbrs.lo if lo is None else lo
    hi = nbrs.hi if hi is None else hi
    i, _, d, w = raw_rows(meta, ent, lo, hi)
    return meta[lo:hi, 1:].copy(), i, d.view(np.uint32).copy(), w.copy()


def same_rows(a, b):
    """Are two row_bytes results identical?"""
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def records(i, j, d):
    """One sortable record per entry: (i, j, bits of the fp32 displacement with -0 taken as +0)."""
    bits = (d.astype(np.float32) + np.float32(0.0)).view(np.uint32).astype(np.int64)
    rec = np.concatenate([i[:, None], j[:, None], bits], axis=1).astype(np.int64)
    return np.ascontiguousarray(rec).view([("f%d" % q, np.int64) for q in range(5)]).reshape(-1)


def check_rows(entry, case, nbrs, ref, gate, lo=0, hi=None, band=nc.BAND, coords=None, over=None, only=None, note="",
               quiet=False):
    """The per-build assertions of the module header for rows lo..hi of `case` (at `coords` if given).  only: bool [n], the
    atoms that must have rows -- every other row lo..hi must be empty.  Returns the RowReport."""
    n = case.n_atoms
    hi = n if hi is None else hi
    tag = f"{entry} {case.name} {note}".strip()
    status = nbrs.status.cpu().numpy().view(np.uint32)
    meta, ent = unpack_rows(nbrs, n)
    at = case if coords is None else case._replace(coords=coords)
    xw = nc.wrap_f64(at)
    cell64 = case.cell.astype(np.float64) if case.periodic else None
    over = case.overflow_rows if over is None else over
    skip = tuple(i for i in over if lo <= i < hi)
    flagged = bool(status[0] & OVER)
    assert flagged == bool(skip), f"{tag}: status[0] = {status[0]}, rows expected to overflow: {skip}"
    for i in skip:
        assert np.all(meta[i, 1:6] == 0), f"{tag}: the overflowing row {i} must come back zeroed"
    has = np.ones(n, dtype=bool) if only is None else only
    rng = np.arange(lo, hi)
    assert np.array_equal(meta[rng[has[lo:hi]], 0].astype(np.int64), (rng[has[lo:hi]] - lo) * nbrs.row_cap), f"{tag}: row offsets"
    empty = rng[~has[lo:hi]]
    assert np.all(meta[empty, 1:6] == 0), f"{tag}: an atom that must have no row has one"
    res = compare_rows(tag, meta, ent, lo, hi, case.species, ref, xw, cell64, case.rcr, case.rca, band_rcr=band,
                       band_rca=band, skip_rows=skip + tuple(empty.tolist()))
    if not quiet:
        report(f"nbrx  {entry:9s} {case.name:18s} {note:12s} atoms {n:5d} rows {lo:4d}..{hi:<5d} pairs {res.pairs:6d} excused "
               f"{res.excused:3d} max|d - d_ref| = {res.worst:.2e} A (gate {gate:.1e})")
    assert res.worst <= gate, f"{tag}: displacement error {res.worst:.2e} A over {gate:.1e}"
    return res


# ---- rows from a half list -------------------------------------------------------------------------------------------------

def half_rows(eng, case, h, dev, lo=0, hi=None):
    sp = torch.from_numpy(case.species).to(dev).contiguous()
    nbrs = eng.rows_from_half(sp, torch.from_numpy(h.idx).to(dev), torch.from_numpy(h.diff).to(dev), lo=lo, hi=hi,
                              row_cap=case.row_cap)
    torch.cuda.synchronize()
    return nbrs


def raw_from_half(eng, case, h, dev, lo, hi):
    """anihip_nbr_from_half into buffers pre-filled with a pattern, so that what the call leaves alone can be seen."""
    n = case.n_atoms
    sp = torch.from_numpy(case.species).to(dev).contiguous()
    idx = torch.from_numpy(h.idx).to(dev).contiguous()
    diff = torch.from_numpy(h.diff).to(dev).contiguous()
    meta = torch.full((n, _lib.META_WORDS), FILL, dtype=torch.int32, device=dev)
    ent = torch.full(((hi - lo) * case.row_cap, 4), FILL, dtype=torch.int32, device=dev)
    status = torch.zeros(_lib.STATUS_WORDS, dtype=torch.int32, device=dev)
    L = _lib.lib()
    ws = torch.empty(L.anihip_nbr_half_workspace_bytes(hi - lo), dtype=torch.uint8, device=dev)
    _lib.check(L.anihip_nbr_from_half(
        torch.cuda.current_stream().cuda_stream, C.byref(eng.params), n, sp.data_ptr(), idx.shape[1], idx.data_ptr(),
        diff.data_ptr(), lo, hi, ws.data_ptr(), ws.numel(), meta.data_ptr(), ent.data_ptr(), (hi - lo) * case.row_cap,
        status.data_ptr()))
    torch.cuda.synchronize()
    return meta.cpu().numpy(), ent.cpu().numpy(), status.cpu().numpy()


def band_rows(case, ref, band=nc.BAND):
    """bool [n]: the rows that hold a pair within `band` of Rcr (such a pair may be present or absent)."""
    start, _, _, r = ref
    i = np.repeat(np.arange(case.n_atoms), np.diff(start))
    out = np.zeros(case.n_atoms, dtype=bool)
    out[i[np.abs(r - case.rcr) <= band]] = True
    return out


HALF_SWEEP = SWEEP + [nx.skin_crowd_case()]


@pytest.mark.parametrize("case", HALF_SWEEP, ids=[c.name for c in HALF_SWEEP])
def test_rows_from_half(dev, eng, oracle64, case):
    """The exact list, the same pairs shuffled and half of them swapped, and the skin list cut at Rcr + 1 (for `padded` with
    the pairs that touch a padding atom left in): each against the oracle, all byte-identical to each other (a row with a
    pair inside the band at Rcr excepted for the skin lists: there the fp64 cut of the exact list and the kernel's fp32
    screen may differ), two runs of one list byte-identical, every displacement plus or minus a diff that was passed in; then
    the middle third through the raw entry point: those rows the full call's, nothing else written."""
    n = case.n_atoms
    ref = ref_list(oracle64, case, case.rcr + nc.BAND)
    wide = ref_list(oracle64, case, case.rcr + 1.0)
    exact = nx.half_list(case, wide, case.rcr)
    lists = {"exact": exact, "shuffled": nx.shuffled_swapped(exact, seed=7),
             "skin": nx.shuffled_swapped(nx.half_list(case, wide, case.rcr + 1.0), seed=8)}
    if np.any(case.species < 0):
        padded = ref_list(oracle64, case, case.rcr + 1.0, species=nx.unpadded_species(case), tag="unpadded")
        lists["skin+padding"] = nx.shuffled_swapped(nx.half_list(case, padded, case.rcr + 1.0), seed=9)
        assert lists["skin+padding"].idx.shape[1] > lists["skin"].idx.shape[1]
    got = {}
    for key, h in lists.items():
        nbrs = half_rows(eng, case, h, dev)
        assert nbrs.symmetric
        check_rows("from_half", case, nbrs, ref, nc.DISP_GATE, note=key)
        got[key] = row_bytes(nbrs, n)
    clear = ~band_rows(case, ref)
    assert same_rows(got["exact"], got["shuffled"]), f"{case.name}: the order of the list shows in the rows"
    for key in lists:
        if key.startswith("skin"):
            assert same_rows_on(got["exact"], got[key], clear), f"{case.name}: rows from the {key} list differ"
    again = row_bytes(half_rows(eng, case, lists["skin"], dev), n)
    assert same_rows(again, got["skin"]), f"{case.name}: two runs of one list differ"
    # every displacement is one that was passed in, or its negative
    h = lists["skin"]
    offered = np.concatenate([records(h.idx[0], h.idx[1], -h.diff), records(h.idx[1], h.idx[0], h.diff)])
    _, i, d, w = got["skin"]
    mine = records(i, (w & 0x0FFFFFFF).astype(np.int64), d.view(np.float32))
    assert np.all(np.isin(mine, offered)), f"{case.name}: a displacement is not plus or minus the diff passed in"
    # the middle third, raw
    lo, hi = n // 3, max(2 * n // 3, n // 3 + 1)
    part = half_rows(eng, case, lists["skin"], dev, lo, hi)
    check_rows("from_half", case, part, ref, nc.DISP_GATE, lo, hi, note="skin, range")
    assert same_rows(row_bytes(part, n), row_bytes_of(got["skin"], lo, hi)), f"{case.name}: rows of a partial call differ"
    meta, ent, status = raw_from_half(eng, case, lists["skin"], dev, lo, hi)
    assert not (int(status[0]) & OVER)
    assert np.all(meta[:lo] == FILL) and np.all(meta[hi:] == FILL), f"{case.name}: a call for {lo}..{hi} wrote other atoms' metadata"
    m = meta.view(np.uint32)[lo:hi].astype(np.int64)
    cnt = (m[:, 1] & 0xFFFF) + (m[:, 1] >> 16)
    ent_rows = ent.reshape(hi - lo, case.row_cap, 4)
    past = np.arange(case.row_cap)[None, :] >= cnt[:, None]
    assert np.all(ent_rows[past] == FILL), f"{case.name}: entries past the end of a row were written"
    assert not np.any(np.all(ent_rows[~past] == FILL, axis=-1))


def same_rows_on(a, b, rows):
    """row_bytes results of whole-range calls (lo = 0) identical on the rows flagged in `rows`."""
    ka, kb = rows[a[1]], rows[b[1]]
    return (np.array_equal(a[0][rows], b[0][rows]) and np.array_equal(a[2][ka], b[2][kb])
            and np.array_equal(a[3][ka], b[3][kb]))


def row_bytes_of(rb, lo, hi):
    """The rows lo..hi of a whole-range row_bytes result."""
    k = (rb[1] >= lo) & (rb[1] < hi)
    return rb[0][lo:hi], rb[1][k], rb[2][k], rb[3][k]


def test_skin_candidates_do_not_overflow(dev, eng, oracle64):
    """The centre of skin_crowd_open is offered 356 candidates, 100 more than a row holds, of which 200 are within Rcr: the
    longer ones are screened before they take a slot."""
    case = nx.skin_crowd_case()
    wide = ref_list(oracle64, case, case.rcr + 1.0)
    h = nx.half_list(case, wide, case.rcr + 1.0)
    assert int(((h.idx[0] == 0) | (h.idx[1] == 0)).sum()) == 356
    nbrs = half_rows(eng, case, h, dev)
    assert not nbrs.overflowed()
    meta, _ = unpack_rows(nbrs, case.n_atoms)
    assert int(meta[0, 1] & 0xFFFF) + int(meta[0, 1] >> 16) == 200


# ---- rows from a full list -------------------------------------------------------------------------------------------------

def full_rows(eng, ex, dev, row_cap, ilist=None, numneigh=None, jlist=None):
    sp = torch.from_numpy(ex.species).to(dev).contiguous()
    x = torch.from_numpy(ex.coords).to(dev).contiguous()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    nbrs = eng.rows_from_full(sp, x, t(ex.ilist if ilist is None else ilist), t(ex.jlist if jlist is None else jlist),
                              t(ex.numneigh if numneigh is None else numneigh), row_cap=row_cap)
    torch.cuda.synchronize()
    return nbrs


def full_gate(ex):
    return max(nc.DISP_GATE, 4.0 * float(np.spacing(np.float32(np.abs(ex.coords).max()))))


@pytest.mark.parametrize("case", SWEEP, ids=IDS)
def test_rows_from_full(dev, eng, oracle64, case):
    """The local atoms and their ghosts as an open system with a LAMMPS-style list (candidates out to Rcr + 1, the atom
    itself and three far atoms mixed in, a permuted ilist, every seventh atom unlisted, some with numneigh = 0): the rows of
    the listed atoms are the oracle's all-pairs rows of that system, every other row is empty, the rows are marked as not
    symmetric."""
    wide = ref_list(oracle64, case, case.rcr + 1.0)
    ex = nx.expand_ghosts(case, wide, case.rcr + 1.0)
    ecase = ex.as_case(case)
    eref = ref_list(oracle64, ecase, case.rcr + nc.BAND)
    nbrs = full_rows(eng, ex, dev, case.row_cap)
    assert nbrs.symmetric is False and (nbrs.lo, nbrs.hi) == (0, ecase.n_atoms)
    m = ecase.n_atoms
    res = check_rows("from_full", ecase, nbrs, eref, full_gate(ex), only=ex.has_row,
                     note=f"{m - ex.n_local} ghosts")
    kept = int(sum(np.diff(eref[0])[ex.has_row]))
    offered = int(ex.n_candidates[ex.has_row].sum())
    assert offered > kept and res.pairs <= kept, f"{case.name}: nothing for the screen to drop"
    assert np.array_equal(row_bytes(full_rows(eng, ex, dev, case.row_cap), m)[2], row_bytes(nbrs, m)[2])


def test_full_list_indices_out_of_range(dev, eng, oracle64):
    """What include/anihip.h now states: a jlist entry outside 0 .. n_atoms is skipped like a far atom (the row is what it is
    without it, no flag); an ilist entry outside 0 .. n_atoms sets ANIHIP_ST_ENTRY_OVERFLOW and every other row is built."""
    case = nc.case_by_name("chunk65_open")
    wide = ref_list(oracle64, case, case.rcr + 1.0)
    ex = nx.expand_ghosts(case, wide, case.rcr + 1.0)
    m = ex.species.shape[1]
    base = full_rows(eng, ex, dev, 256)
    assert not base.overflowed()
    first = np.cumsum(ex.numneigh) - ex.numneigh
    owner = np.repeat(ex.ilist, ex.numneigh)
    assert owner.size == ex.jlist.size and first.size == ex.ilist.size
    jl = ex.jlist.copy()
    selfs = np.nonzero(jl == owner)[0]
    assert selfs.size == int((ex.numneigh > 0).sum())
    jl[selfs[0::3]] = m
    jl[selfs[1::3]] = -1
    jl[selfs[2::3]] = 2 ** 31 - 1
    got = full_rows(eng, ex, dev, 256, jlist=jl)
    assert not got.overflowed() and int(got.status[0]) == 0
    assert same_rows(row_bytes(got, m), row_bytes(base, m)), "an out-of-range jlist entry changed a row"
    il = np.concatenate([ex.ilist[:5], [m], ex.ilist[5:], [-1]]).astype(np.int32)
    nn = np.concatenate([ex.numneigh[:5], [0], ex.numneigh[5:], [0]]).astype(np.int32)
    assert il.size <= m
    got = full_rows(eng, ex, dev, 256, ilist=il, numneigh=nn)
    assert int(got.status[0]) & OVER == _lib.ST_ENTRY_OVERFLOW
    assert same_rows(row_bytes(got, m), row_bytes(base, m)), "an out-of-range ilist entry changed another atom's row"


# ---- Verlet refresh ---------------------------------------------------------------------------------------------------------

REFRESH_SWEEP = SWEEP + [nx.skin_over_case()]


@pytest.mark.parametrize("case", REFRESH_SWEEP, ids=[c.name for c in REFRESH_SWEEP])
def test_refresh(dev, eng, oracle64, case):
    """VerletRows with the reuse switched on: rows at the build point, then rows refreshed after every atom moved by up to
    0.28 A (random cases) or 0.10 A (shell families) per component, against the oracle at the moved coordinates; one build, one
    reuse; a sub-range call byte-identical to the full call's rows; the one-over cases -- and skin_over_open, whose true row
    fits while its Verlet row does not -- flagged through the status, the centre's row zeroed."""
    from torchani_amd.engine import VerletRows

    n = case.n_atoms
    sp, x0, cell, pbc = to_dev(case, dev)
    x1_np = nx.moved(case, nx.move_amplitude(case), seed=3)
    x1 = torch.from_numpy(x1_np).to(dev).contiguous()
    ref0 = ref_list(oracle64, case, case.rcr + nx.REFRESH_BAND)
    ref1 = ref_list(oracle64, case, case.rcr + nx.REFRESH_BAND, coords=x1_np, tag="moved")
    over = (0,) if case.name == "skin_over_open" else case.overflow_rows
    for mode in modes_of(case):
        ver = VerletRows(skin=nx.SKIN)
        ver.rebuild_above = float("inf")
        r0 = ver.rows(eng, sp, x0, cell, pbc, 0, n, mode, case.row_cap)
        torch.cuda.synchronize()
        assert (ver.n_builds, ver.n_reuses, ver.n_direct) == (1, 0, 0)
        assert int((ver._rows.meta[:, 1] & 0xFFFF).max()) == 0, "a Verlet row has entries in the angular group"
        check_rows("refresh", case, r0, ref0, nx.REFRESH_GATE, band=nx.REFRESH_BAND, over=over, note=f"{mode}, built",
                   quiet=True)
        r1 = ver.rows(eng, sp, x1, cell, pbc, 0, n, mode, case.row_cap)
        torch.cuda.synchronize()
        assert (ver.n_builds, ver.n_reuses, ver.n_direct) == (1, 1, 0)
        check_rows("refresh", case, r1, ref1, nx.REFRESH_GATE, band=nx.REFRESH_BAND, coords=x1_np, over=over,
                   note=f"{mode}, moved")
        stored = ver._rows.meta.cpu().numpy().view(np.uint32)[:, 1] >> 16
        if case.centre is not None and not over:
            assert int(stored[case.centre]) == int(np.diff(ref0[0])[case.centre]), "the centre's Verlet row"
        lo, hi = n // 3, max(2 * n // 3, n // 3 + 1)
        part = eng.refresh_rows(sp, x1, ver._coords0, ver._rows, lo, hi, case.row_cap)
        torch.cuda.synchronize()
        assert same_rows(row_bytes(part, n), row_bytes_of(row_bytes(r1, n), lo, hi)), f"{case.name}/{mode}: sub-range refresh"


# ---- rows to a half list ---------------------------------------------------------------------------------------------------

TO_HALF = ("slab", "tiny", "rod", "skew_TTF", "padded", "droplet_none", "chunk256_pbc")


def sorted_records(nbrs, n):
    meta, ent = unpack_rows(nbrs, n)
    i, j, d, _ = raw_rows(meta, ent, 0, n)
    return np.sort(records(i, j, d)), (i, j, d)


@pytest.mark.parametrize("name", TO_HALF)
def test_rows_to_half_cases(dev, eng, oracle64, name):
    """rows_to_half on thin cells, self images, padding, an open system and a 256-entry row: every unordered pair of the
    oracle once; of an atom's own images the one with the positive image index; a sub-range's export is the rows lo..hi of
    the full export, in order; and the round trip back to rows (module header)."""
    from torchani_amd.engine import rows_to_half

    case = nc.case_by_name(name)
    n = case.n_atoms
    start, j, d, r = ref_list(oracle64, case, case.rcr + nc.BAND)
    nbrs = build(eng, case, dev, "cell")
    assert not nbrs.overflowed()
    idx_t, dist_t, diff_t = rows_to_half(nbrs, n)
    torch.cuda.synchronize()
    idx, diff32 = idx_t.cpu().numpy(), diff_t.cpu().numpy()
    diff = diff32.astype(np.float64)
    xw = nc.wrap_f64(case)
    cell64 = case.cell.astype(np.float64) if case.periodic else None
    oi = np.repeat(np.arange(n), np.diff(start))
    okey, oimg = pair_keys(oi, j.astype(np.int64), d.astype(np.float64), xw, cell64, n)
    must = okey[r <= case.rcr - nc.BAND]
    fwd, fimg = pair_keys(idx[0], idx[1], -diff, xw, cell64, n)
    bwd, _ = pair_keys(idx[1], idx[0], diff, xw, cell64, n)
    both = np.concatenate([fwd, bwd])
    assert np.unique(both).size == both.size, f"{name}: an unordered pair is listed twice"
    assert np.all(np.isin(must, both)) and np.all(np.isin(both, okey))
    n_exact = int((r <= case.rcr).sum())
    n_band = int((np.abs(r - case.rcr) <= nc.BAND).sum())
    assert n_exact % 2 == 0 and abs(2 * idx.shape[1] - n_exact) <= n_band
    if n_band == 0:
        assert 2 * idx.shape[1] == n_exact
    assert np.abs(np.linalg.norm(diff, axis=1) - dist_t.cpu().numpy()).max() < 1e-5
    # own images: exactly the one the reference keeps
    own = idx[0] == idx[1]
    n_own = int(((oi == j) & (r <= case.rcr - nc.BAND)).sum())
    assert np.all(idx[1] >= idx[0]) and np.all(nx.first_nonzero_positive(fimg[own]))
    assert 2 * int(own.sum()) >= n_own and (n_own > 0) == (name in ("slab", "tiny", "rod"))
    # a sub-range
    lo, hi = n // 3, max(2 * n // 3, n // 3 + 1)
    sub = rows_to_half(nbrs._replace(lo=lo, hi=hi), n)
    sel = (idx[0] >= lo) & (idx[0] < hi)
    assert np.array_equal(sub[0].cpu().numpy(), idx[:, sel]) and np.array_equal(sub[2].cpu().numpy(), diff32[sel])
    assert np.array_equal(sub[1].cpu().numpy(), dist_t.cpu().numpy()[sel])
    # round trip
    sp = torch.from_numpy(case.species).to(dev).contiguous()
    back = eng.rows_from_half(sp, idx_t, diff_t, row_cap=case.row_cap)
    torch.cuda.synchronize()
    assert not back.overflowed()
    rec0, (i0, j0, d0) = sorted_records(nbrs, n)
    rec1, (i1, j1, d1) = sorted_records(back, n)
    assert rec0.size == rec1.size and np.array_equal(np.bincount(i0, minlength=n), np.bincount(i1, minlength=n))
    kept = nx.numpy_half_keep(i0, j0, d0)
    assert np.all(np.isin(records(i0[kept], j0[kept], d0[kept]), rec1)), f"{name}: a kept entry changed on the round trip"
    mirrored = records(j0[kept], i0[kept], -d0[kept])
    assert np.array_equal(np.sort(np.concatenate([records(i0[kept], j0[kept], d0[kept]), mirrored])), rec1)
    k0, _ = pair_keys(i0, j0, d0.astype(np.float64), xw, cell64, n)
    k1, _ = pair_keys(i1, j1, d1.astype(np.float64), xw, cell64, n)
    o0, o1 = np.argsort(k0), np.argsort(k1)
    assert np.array_equal(k0[o0], k1[o1]), f"{name}: the round trip changes a row's (j, image) set"
    worst = float(np.abs(d0[o0].astype(np.float64) - d1[o1]).max())
    assert worst <= 2 * nc.DISP_GATE
    if not case.periodic:   # (batch mode, no image shift: d = x_j - x_i straight from the coordinates)
        plain = build(eng, case, dev, "batch")
        idx_b, _, diff_b = rows_to_half(plain, n)
        back_b = eng.rows_from_half(sp, idx_b, diff_b, row_cap=case.row_cap)
        torch.cuda.synchronize()
        assert np.array_equal(sorted_records(plain, n)[0], sorted_records(back_b, n)[0]), \
            f"{name}: open system, the round trip changes an entry"
    idx2, _, diff2 = rows_to_half(back, n)
    again = eng.rows_from_half(sp, idx2, diff2, row_cap=case.row_cap)
    torch.cuda.synchronize()
    assert np.array_equal(sorted_records(again, n)[0], rec1), f"{name}: a second round trip changes an entry"
    report(f"nbrx  to_half   {name:18s} {idx.shape[1]} pairs ({int(own.sum())} own images), oracle {n_exact} ordered pairs; range "
           f"{lo}..{hi} in order; round trip: kept entries bit for bit, mirrored within {worst:.1e} A")


def raw_to_half(meta, ent, n, lo, hi, capacity, guard=64):
    """anihip_nbr_rows_to_half with `capacity` into outputs followed by `guard` pattern-filled elements."""
    dev = meta.device
    L = _lib.lib()
    ws = torch.empty(L.anihip_nbr_rows_to_half_workspace_bytes(hi - lo), dtype=torch.uint8, device=dev)
    npairs = torch.full((1,), -1, dtype=torch.int64, device=dev)
    idx = torch.full((2 * capacity + guard,), -7, dtype=torch.int64, device=dev)
    dist = torch.full((capacity + guard,), -7.0, dtype=torch.float32, device=dev)
    diff = torch.full((3 * capacity + guard,), -7.0, dtype=torch.float32, device=dev)
    _lib.check(L.anihip_nbr_rows_to_half(
        torch.cuda.current_stream().cuda_stream, n, lo, hi, meta.data_ptr(), ent.data_ptr(), ws.data_ptr(), ws.numel(), capacity,
        idx.data_ptr() if capacity else None, dist.data_ptr() if capacity else None, diff.data_ptr() if capacity else None,
        npairs.data_ptr()))
    torch.cuda.synchronize()
    return int(npairs.item()), idx.cpu().numpy(), dist.cpu().numpy(), diff.cpu().numpy()


def test_rows_to_half_synthetic(dev):
    """263 173 atoms with 0 to 3 entries each (k_scan_sums turns its loop twice), lo = 0 and lo = 777: the count call
    returns P, idx / diff / dist equal the numpy restatement exactly, order included; with capacity = P - 7 the first
    capacity pairs are written and nothing behind them."""
    n = nx.SCAN_TWICE_N
    s = nx.synthetic_rows(n, seed=2)
    meta = torch.from_numpy(s.meta.view(np.int32)).to(dev).contiguous()
    ent = torch.from_numpy(s.ent).to(dev).contiguous()
    for lo in (0, 777):
        e_idx, e_diff, e_dist = nx.synthetic_half(s, lo, n)
        P = e_idx.shape[1]
        assert raw_to_half(meta, ent, n, lo, n, 0)[0] == P, "the count call"
        for cap in (P, P - 7):
            got_p, idx, dist, diff = raw_to_half(meta, ent, n, lo, n, cap)
            assert got_p == P
            assert np.array_equal(idx[:2 * cap].reshape(2, cap), e_idx[:, :cap]), f"lo = {lo}, capacity {cap}: idx"
            assert np.array_equal(diff[:3 * cap].reshape(cap, 3), e_diff[:cap]), f"lo = {lo}, capacity {cap}: diff"
            assert np.array_equal(dist[:cap], e_dist[:cap]), f"lo = {lo}, capacity {cap}: dist"
            assert np.all(idx[2 * cap:] == -7) and np.all(dist[cap:] == -7.0) and np.all(diff[3 * cap:] == -7.0), \
                f"lo = {lo}, capacity {cap}: something was written behind the outputs"
        report(f"nbrx  to_half   synthetic {n} atoms, rows {lo}..{n}: {P} pairs, equal to the numpy half list; capacity "
               f"{P - 7}: the first {P - 7} written, nothing else")


# ---- the consumers on rows that are not symmetric ---------------------------------------------------------------------------

CONSUMER_CASES = ("chunk129_open", "chunk256_open", "ang128_at_open")
VJP_TOL = 2e-5        # tests/test_gpu_aev_long_rows.py
VJP_REG_REL = 5e-6


def listed_everything(oracle64, case, cutoff):
    wide = ref_list(oracle64, case, cutoff + 1.0)
    ex = nx.expand_ghosts(case, wide, cutoff + 1.0, unlisted_every=None, empty_every=None)
    assert ex.species.shape[1] == case.n_atoms and np.all(ex.has_row)
    return ex


@pytest.mark.parametrize("name", CONSUMER_CASES)
def test_aev_backward_pushes_on_full_rows(dev, eng, oracle64, name):
    """AevEngine.backward on rows from a full list (no ANIHIP_BWD_SYMMETRIC: every radial term pushed to its neighbor) with a
    seeded cotangent against the oracle's vector-Jacobian product, at the parity and the regression gate of
    tests/test_gpu_aev_long_rows.py."""
    from oracle import oracle as orc

    case = nc.case_by_name(name)
    n = case.n_atoms
    c = eng.consts
    p = orc.make_params(c.num_species, c.Rcr, c.Rca, c.EtaR, c.EtaA, c.Zeta, c.ShfR, c.ShfA, c.ShfZ, c.cutoff_fn)
    w = np.random.RandomState(1000).uniform(-1.0, 1.0, (n, c.out_dim)).astype(np.float32)
    _, ref = oracle64.aev(p, case.species, case.coords.astype(np.float64), None, None, grad_aev=w.astype(np.float64))
    ref = ref.reshape(n, 3)
    ex = listed_everything(oracle64, case, case.rcr)
    rows = full_rows(eng, ex, dev, 256)
    assert rows.symmetric is False and not rows.overflowed()
    sp = torch.from_numpy(case.species).to(dev).contiguous()
    wt = torch.from_numpy(w).to(dev).contiguous()
    g = eng.backward(sp, rows, wt)
    g_sym = eng.backward(sp, build(eng, case, dev, "batch"), wt)
    torch.cuda.synchronize()
    mag = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(g.cpu().numpy().astype(np.float64) - ref).max())
    dsym = float((g - g_sym).abs().max())
    report(f"nbrx  aev_bwd   {name:18s} push path: vjp err {err / mag:.2e} x max|vjp| {mag:.1f} (gates {VJP_TOL:.0e}, "
           f"{VJP_REG_REL:.0e}); from the gather path on symmetric rows {dsym / mag:.2e}")
    assert err < VJP_TOL * mag and err <= VJP_REG_REL * mag, f"{name}: vjp off by {err / mag:.2e} x {mag:.1f}"


@pytest.mark.parametrize("name", CONSUMER_CASES)
def test_pair_potential_pushes_on_full_rows(dev, oracle64, name):
    """RepulsionZBL.accumulate (ANIHIP_PAIR_PUSH) on rows from a full list: per-atom halves and gradient against the
    reference's own class in fp64 (tests/golden/gen_golden_pairs2.py, PUSH_ROWS) at the gates of
    test_analytic_pair_potentials_match_reference; with the 5.2 A smooth and the 4.0 A cosine envelope."""
    import _aev_cases as ac
    from torchani_amd import potentials as P
    from torchani_amd.engine import AevEngine

    case = nc.case_by_name(name)
    n = case.n_atoms
    twin = ac.case_by_name(name + "/built")   # (what the fixture was written from)
    assert np.array_equal(twin.species, case.species) and np.array_equal(twin.coords, case.coords)
    ref = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"pairs2_{name}_built.npz")))
    symbols = ["H", "C", "N", "O", "S", "F", "Cl"]
    pots = {"zbl": P.RepulsionZBL(symbols, cutoff=5.2, cutoff_fn="smooth"),
            "zbl_cos": P.RepulsionZBL(symbols, k=0.4685, cutoff=4.0, cutoff_fn="cosine")}
    sp = torch.from_numpy(case.species).to(dev).contiguous()
    x = torch.from_numpy(case.coords).to(dev).contiguous()
    for key, pot in pots.items():
        pot = pot.to(dev)
        e = AevEngine(aev_constants_2x(7)._replace(Rcr=pot.cutoff, Rca=1e-3))
        ex = listed_everything(oracle64, case, pot.cutoff)
        rows = full_rows(e, ex, dev, 256)
        assert rows.symmetric is False and not rows.overflowed()
        out = []
        for r in (rows, e.neighbors(sp, x, mode="batch", row_cap=256)):
            ae = torch.zeros(n, dtype=torch.float32, device=dev)
            gc = torch.zeros((n, 3), dtype=torch.float32, device=dev)
            pot.accumulate(sp, r, ae, gc)
            torch.cuda.synchronize()
            out.append((ae.cpu().numpy(), gc.cpu().numpy()))
        ea_ref, f_ref = ref[key + "_atomic"].reshape(n), ref[key + "_forces"].reshape(n, 3)
        escale, fscale = max(1e-3, np.abs(ea_ref).max()), max(1e-3, np.abs(f_ref).max())
        ea = float(np.abs(out[0][0] - ea_ref).max())
        fe = float(np.abs(-out[0][1] - f_ref).max())
        report(f"nbrx  pair_push {name:18s} {key:8s} max|e_atom err| = {ea:.2e} (scale {escale:.1e})  |F err| = {fe:.2e} (scale "
               f"{fscale:.1e}); from symmetric rows: e_atom {np.abs(out[0][0] - out[1][0]).max():.2e}, grad "
               f"{np.abs(out[0][1] - out[1][1]).max():.2e}")
        assert ea < 5e-6 * escale and fe < 1e-5 * fscale, key
