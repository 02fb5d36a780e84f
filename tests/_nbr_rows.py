"""Decoder of the engine's neighbor rows (format: include/anihip.h) and their comparison with the oracle's full list, shared
by tests/test_gpu_parity.py and tests/test_gpu_neighbors.py.  numpy only."""
from __future__ import annotations

import typing as tp

import numpy as np

IMG_SPAN = 33   # image indices -16..16 per axis fit a key


def wrap_coords(coords, cell, pbc) -> np.ndarray:
    """fp64 copy of coords [n, 3] mapped into the cell along its periodic axes (frac -= floor(frac)); cell None: unchanged."""
    x = np.asarray(coords, dtype=np.float64).reshape(-1, 3)
    if cell is None or pbc is None or not any(pbc):
        return x
    c = np.asarray(cell, dtype=np.float64)
    f = x @ np.linalg.inv(c)
    f -= np.floor(f) * np.asarray(pbc, dtype=np.float64)
    return f @ c


class Rows(tp.NamedTuple):
    """The rows lo..hi flattened: entry e belongs to central atom i[e], sits at place k[e] of its row (angular-range group
    first: ang[e]), names neighbor j[e] of species sp[e] at displacement d[e]."""
    i: np.ndarray
    k: np.ndarray
    ang: np.ndarray
    j: np.ndarray
    sp: np.ndarray
    d: np.ndarray
    nA: np.ndarray      # per atom of lo..hi
    nF: np.ndarray
    cntA: np.ndarray    # [hi - lo, 8] packed per-species counts of the two groups
    cntF: np.ndarray


def decode_rows(meta: np.ndarray, ent: np.ndarray, lo: int, hi: int) -> Rows:
    m = meta[lo:hi].astype(np.int64)
    nA, nF = m[:, 1] & 0xFFFF, m[:, 1] >> 16
    cnt = nA + nF
    i = np.repeat(np.arange(lo, hi), cnt)
    first = np.concatenate([[0], np.cumsum(cnt)])[:-1]
    k = np.arange(int(cnt.sum())) - np.repeat(first, cnt)
    e = ent[np.repeat(m[:, 0], cnt) + k]
    w = np.ascontiguousarray(e[:, 3]).view(np.uint32)
    sh = 8 * np.arange(4)
    cntA = np.concatenate([(m[:, 2:3] >> sh) & 255, (m[:, 3:4] >> sh) & 255], axis=1)
    cntF = np.concatenate([(m[:, 4:5] >> sh) & 255, (m[:, 5:6] >> sh) & 255], axis=1)
    return Rows(i, k, k < np.repeat(nA, cnt), (w & 0x0FFFFFFF).astype(np.int64), (w >> 28).astype(np.int64),
                e[:, :3].astype(np.float64), nA, nF, cntA, cntF)


def pair_keys(i, j, d, xw, cell, n_atoms):
    """One integer per (i, j, periodic image): the image is read off the displacement, d - (xw[j] - xw[i]) = image @ cell."""
    if cell is None:
        img = np.zeros((i.shape[0], 3), dtype=np.int64)
    else:
        fr = (d - (xw[j] - xw[i])) @ np.linalg.inv(cell)
        img = np.rint(fr).astype(np.int64)
        assert i.size == 0 or np.abs(fr - img).max() < 1e-3, "a displacement is not a lattice image of its pair"
        assert i.size == 0 or np.abs(img).max() <= IMG_SPAN // 2
    key = i.astype(np.int64) * n_atoms + j
    for q in range(3):
        key = key * IMG_SPAN + (img[:, q] + IMG_SPAN // 2)
    return key, img


class RowReport(tp.NamedTuple):
    pairs: int       # oracle pairs of the compared rows within Rcr
    excused: int     # of the oracle's pairs, those inside a borderline band
    worst: float     # max |d - d_ref| over the matched entries


def compare_rows(tag, meta, ent, lo, hi, species, oracle_list, xw, cell, rcr, rca, band_rcr=0.0, band_rca=1e-5,
                 skip_rows=()) -> RowReport:
    """Rows lo..hi of the engine against the oracle's full list (start, j, d, r).  With band_rcr > 0 the oracle's list must
    have been built with cutoff rcr + band_rcr.

    * every row's (j, image) set equals the oracle's; a pair with |r - rcr| <= band_rcr may be present or absent;
    * neighbor species as in `species`; angular-range group first, a pair with |r - rca| > band_rca in the right group
      and the fp32 lengths of the row itself on the right side of rca within 1e-5; each group sorted by species; the packed
      per-species counts;
    * rows in skip_rows (zeroed on purpose) are left out.
    Returns the pair count, the excused count and the worst displacement error; the caller gates the latter."""
    species = np.asarray(species).reshape(-1)
    n = species.shape[0]
    start, oj, od, orr = oracle_list
    rows = decode_rows(meta, ent, lo, hi)
    keep_row = np.ones(n, dtype=bool)
    keep_row[list(skip_rows)] = False
    # ---- the rows by themselves ----
    assert np.all((rows.j >= 0) & (rows.j < n)), f"{tag}: neighbor index out of range"
    assert np.array_equal(rows.sp, species[rows.j]), f"{tag}: species bits of an entry differ from the neighbor's species"
    rr = np.linalg.norm(rows.d, axis=1)
    assert np.all(rr[rows.ang] <= rca + 1e-5) and np.all(rr[~rows.ang] >= rca - 1e-5), f"{tag}: angular / far split"
    same = (rows.i[1:] == rows.i[:-1]) & (rows.ang[1:] == rows.ang[:-1])
    assert np.all(np.diff(rows.sp)[same] >= 0), f"{tag}: a group is not sorted by species"
    assert np.all(np.diff(rows.ang.astype(np.int64))[rows.i[1:] == rows.i[:-1]] <= 0), f"{tag}: far entry before angular"
    cA = np.zeros((hi - lo, 8), dtype=np.int64)
    cF = np.zeros((hi - lo, 8), dtype=np.int64)
    np.add.at(cA, (rows.i[rows.ang] - lo, rows.sp[rows.ang]), 1)
    np.add.at(cF, (rows.i[~rows.ang] - lo, rows.sp[~rows.ang]), 1)
    assert np.array_equal(cA, rows.cntA) and np.array_equal(cF, rows.cntF), f"{tag}: packed per-species counts"
    # ---- against the oracle ----
    oi = np.repeat(np.arange(n), np.diff(start))
    sel = (oi >= lo) & (oi < hi) & keep_row[oi]
    oi, oj, od, orr = oi[sel], oj[sel].astype(np.int64), od[sel].astype(np.float64), orr[sel].astype(np.float64)
    gsel = keep_row[rows.i]
    gi, gj, gd, gang = rows.i[gsel], rows.j[gsel], rows.d[gsel], rows.ang[gsel]
    okey, oimg = pair_keys(oi, oj, od, xw, cell, n)
    gkey, gimg = pair_keys(gi, gj, gd, xw, cell, n)
    assert np.unique(okey).size == okey.size, f"{tag}: the oracle lists a pair twice"
    if np.unique(gkey).size != gkey.size:
        u, c = np.unique(gkey, return_counts=True)
        e = int(np.nonzero(gkey == u[c > 1][0])[0][0])
        raise AssertionError(f"{tag}: atom {gi[e]} lists neighbor {gj[e]} image {gimg[e].tolist()} {int(c.max())} times")
    in_band = np.abs(orr - rcr) <= band_rcr
    must = orr <= rcr - band_rcr if band_rcr > 0 else orr <= rcr
    assert np.all(must | in_band), f"{tag}: the oracle's list reaches past rcr + band"
    missing = must & ~np.isin(okey, gkey)
    if missing.any():
        e = int(np.nonzero(missing)[0][0])
        raise AssertionError(f"{tag}: {int(missing.sum())} pairs missing; first: atom {oi[e]} lacks neighbor {oj[e]} image "
                             f"{oimg[e].tolist()} at r = {orr[e]:.6f} (row has {int((gi == oi[e]).sum())} entries, oracle "
                             f"{int((oi == oi[e]).sum())})")
    extra = ~np.isin(gkey, okey)
    if extra.any():
        e = int(np.nonzero(extra)[0][0])
        raise AssertionError(f"{tag}: {int(extra.sum())} pairs too many; first: atom {gi[e]} lists neighbor {gj[e]} image "
                             f"{gimg[e].tolist()} at |d| = {np.linalg.norm(gd[e]):.6f}")
    order = np.argsort(okey)
    at = order[np.searchsorted(okey[order], gkey)]
    worst = float(np.abs(od[at] - gd).max()) if gkey.size else 0.0
    r_ref = orr[at]
    wrong = (gang != (r_ref <= rca)) & (np.abs(r_ref - rca) > band_rca)
    if wrong.any():
        e = int(np.nonzero(wrong)[0][0])
        raise AssertionError(f"{tag}: atom {gi[e]} has neighbor {gj[e]} at r = {r_ref[e]:.6f} in the "
                             f"{'angular' if gang[e] else 'far'} group")
    excused = int(in_band.sum() + (np.abs(orr - rca) <= band_rca).sum()) if band_rcr > 0 else 0
    return RowReport(int((orr <= rcr).sum()), excused, worst)
