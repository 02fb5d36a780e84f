"""What tests/test_gpu_neighbors_external.py rests on, on the CPU: the host constructions of tests/_nbr_external.py held to
the fp64 oracle, the borderline bands' shares at the built and at the moved coordinates, the regimes each entry point of
csrc/nbr.hip must reach (from fp64 distances), the sizes of the Verlet rows, and the synthetic rows' expectation."""
import numpy as np
import pytest

import _nbr_cases as nc
import _nbr_external as nx
from _nbr_rows import pair_keys

SWEEP = nx.sweep() + [nx.skin_crowd_case(), nx.skin_over_case()]
IDS = [c.name for c in SWEEP]


def counts(case, olist, cutoff, rca=None, coords=None):
    """Per atom: pairs within cutoff, of them within rca, and the largest per-species count of either group."""
    i, j, _, r, _ = nx.flat_pairs(case, olist, cutoff, coords=coords)
    n = case.n_atoms
    rca = case.rca if rca is None else rca
    cls = np.zeros((n, 2, nc.NUM_SPECIES), dtype=np.int64)
    np.add.at(cls, (i, (r > rca).astype(np.int64), case.species.reshape(-1)[j]), 1)
    return cls.sum(axis=(1, 2)), cls[:, 0].sum(axis=1), cls.max(axis=(1, 2))


def band_share(r, cutoffs, band):
    return sum(int((np.abs(r - c) <= band).sum()) for c in cutoffs)


@pytest.mark.parametrize("case", SWEEP, ids=IDS)
def test_bands_and_verlet_rows(oracle64, case):
    """The band's share at the built and at the moved coordinates (a pair inside it may fall on either side), the margins
    of the shell families at the moved coordinates, and the Verlet rows' sizes."""
    wide = case.rcr + nx.SKIN
    lst = nx.oracle_list(oracle64, case, wide + nc.BAND)
    r = lst[3]
    pairs = max(int((r <= case.rcr).sum()), 1)
    assert band_share(r, (case.rcr, case.rca, wide), nc.BAND) <= nc.BAND_SHARE * pairs
    x1 = nx.moved(case, nx.move_amplitude(case), seed=3)
    assert np.abs(x1 - case.coords).max() <= nx.move_amplitude(case) + 1e-5
    assert np.sqrt(((x1.astype(np.float64) - case.coords) ** 2).sum(-1)).max() < 0.5 * nx.SKIN
    lst1 = nx.oracle_list(oracle64, case, case.rcr + nx.REFRESH_BAND, coords=x1)
    assert band_share(lst1[3], (case.rcr, case.rca), nx.REFRESH_BAND) <= nc.BAND_SHARE * pairs
    # every pair of the moved coordinates was within Rcr + skin where the Verlet rows were built
    k0 = set(pair_keys(*nx.flat_pairs(case, lst, wide)[:3], nc.wrap_f64(case),
                       case.cell.astype(np.float64) if case.periodic else None, case.n_atoms)[0].tolist()) \
        if not case.periodic else None
    if k0 is not None:
        i1, j1, d1, _, _ = nx.flat_pairs(case, lst1, case.rcr, coords=x1)
        k1 = pair_keys(i1, j1, d1, x1.reshape(-1, 3).astype(np.float64), None, case.n_atoms)[0]
        assert set(k1.tolist()) <= k0
    # Verlet rows: Rcr + skin, every entry in the far group (Rca = 1e-3)
    rows_w, _, spec_w = counts(case, lst, wide, rca=1e-3)
    rows, ang, spec = counts(case, lst, case.rcr)
    rows1, ang1, spec1 = counts(case, lst1, case.rcr, coords=x1)
    if case.centre is None:
        assert rows_w.max() <= 256 and spec_w.max() <= nc.MAX_PER_SPECIES
        assert rows1.max() <= case.row_cap and ang1.max() <= nc.MAX_ANG and spec1.max() <= nc.MAX_PER_SPECIES
        return
    c = case.centre
    others = np.arange(case.n_atoms) != c
    assert rows_w[others].max() <= 256 and spec_w[others].max() <= nc.MAX_PER_SPECIES
    cap, amax, smax = case.limits
    assert rows1[others].max() <= cap and ang1[others].max() <= amax and spec1[others].max() <= smax
    # the centre keeps its counts under the move, each pair 0.15 A or more from a cutoff
    assert (rows1[c], ang1[c], spec1[c]) == (rows[c], ang[c], spec[c])
    i1, _, _, r1, _ = nx.flat_pairs(case, lst1, case.rcr + nx.REFRESH_BAND, coords=x1)
    rc = r1[i1 == c]
    assert np.all(np.abs(rc - case.rcr) >= 0.15) and np.all(np.abs(rc - case.rca) >= 0.15)
    over = rows[c] > cap or ang[c] > amax or spec[c] > smax
    assert over == (case.overflow_rows == (c,))
    wide_over = rows_w[c] > 256 or spec_w[c] > nc.MAX_PER_SPECIES
    if case.name == "skin_over_open":
        assert rows[c] == 200 and rows_w[c] == 260 and not over and wide_over
    elif case.name == "skin_crowd_open":
        i0, _, _, r0, _ = nx.flat_pairs(case, lst, case.rcr + 1.0)
        assert rows[c] == 200 and int((i0 == c).sum()) == 356 and not over
    else:
        # a Verlet row overflows only where the true row does, or where all 256 are of one species in the far group
        assert wide_over == (over and not case.name.startswith(("cap64", "ang128")))


def test_every_regime_has_a_case(oracle64):
    """From fp64 distances: rows in each chunk interval, every limit at and one over, self images, padding."""
    got = {}
    for case in nx.shell_cases():
        rows, ang, spec = counts(case, nx.oracle_list(oracle64, case, case.rcr), case.rcr)
        got[case.name] = (int(rows[case.centre]), int(ang[case.centre]), int(spec[case.centre]))
    for tag in ("_open", "_pbc"):
        longest = sorted(v[0] for k, v in got.items() if k.startswith("chunk") and k.endswith(tag))
        assert any(65 <= v <= 128 for v in longest) and any(129 <= v <= 192 for v in longest)
        assert any(193 <= v <= 256 for v in longest) and 256 in longest
        assert got["cap64_at" + tag][0] == 64 and got["cap64_over" + tag][0] == 65
        assert got["ang128_at" + tag][1] == 128 and got["ang128_over" + tag][1] == 129
        assert got["spec255_at" + tag][2] == 255 and got["spec255_over" + tag][2] == 256
        assert got["rad256_at" + tag][:2] == (256, 0) and got["rad256_over" + tag][:2] == (257, 0)
    for name in ("slab", "tiny"):
        case = nc.case_by_name(name)
        i, j, _, _, img = nx.flat_pairs(case, nx.oracle_list(oracle64, case, case.rcr), case.rcr)
        assert np.any(i == j), f"{name}: no atom sees its own image"
    assert np.any(nc.case_by_name("padded").species < 0)
    # the consumers' cases: more than 64 pushed radial terms and a full angular group
    assert got["chunk129_open"][0] == 129 and got["chunk256_open"][0] == 256 and got["ang128_at_open"][1] == 128


@pytest.mark.parametrize("case", SWEEP, ids=IDS)
def test_half_list(oracle64, case):
    """Each unordered pair once: the list and its mirror are the oracle's ordered pairs, none twice; own images kept by the
    sign of the image index; the skin list holds the exact one; the padded variant adds only pairs that touch padding."""
    n = case.n_atoms
    lst = nx.oracle_list(oracle64, case, case.rcr + 1.0)
    xw = nc.wrap_f64(case)
    cell = case.cell.astype(np.float64) if case.periodic else None
    i, j, d, _, _ = nx.flat_pairs(case, lst, case.rcr)
    okey = pair_keys(i, j, d, xw, cell, n)[0]
    keys = {}
    for tag, cutoff in (("exact", case.rcr), ("skin", case.rcr + 1.0)):
        h = nx.half_list(case, lst, cutoff)
        a, b = h.idx
        assert np.all((b > a) | ((b == a) & nx.first_nonzero_positive(h.image)))
        fwd = pair_keys(a, b, -h.diff.astype(np.float64), xw, cell, n)[0]
        bwd = pair_keys(b, a, h.diff.astype(np.float64), xw, cell, n)[0]
        both = np.concatenate([fwd, bwd])
        assert np.unique(both).size == both.size == 2 * a.size
        keys[tag] = both
        s = nx.shuffled_swapped(h, seed=7)
        fs = pair_keys(s.idx[0], s.idx[1], -s.diff.astype(np.float64), xw, cell, n)[0]
        bs = pair_keys(s.idx[1], s.idx[0], s.diff.astype(np.float64), xw, cell, n)[0]
        assert np.array_equal(np.sort(np.concatenate([fs, bs])), np.sort(both))
        assert not np.array_equal(s.idx, h.idx) or a.size < 2
    assert np.array_equal(np.sort(keys["exact"]), np.sort(okey))
    assert np.all(np.isin(keys["exact"], keys["skin"])) and keys["skin"].size >= keys["exact"].size
    if case.centre is None and case.n_atoms > 100:
        assert keys["skin"].size > keys["exact"].size
    if np.any(case.species < 0):
        lp = nx.oracle_list(oracle64, case, case.rcr, species=nx.unpadded_species(case))
        hp = nx.half_list(case, lp, case.rcr)
        pad = case.species.reshape(-1) < 0
        touches = pad[hp.idx[0]] | pad[hp.idx[1]]
        assert touches.any() and int((~touches).sum()) == keys["exact"].size // 2


GHOST_NAMES = ("ortho", "skew_TTT", "skew_TFF", "slab", "rod", "tiny", "padded", "droplet_TTT", "chunk129_pbc", "chunk256_open")


@pytest.mark.parametrize("name", GHOST_NAMES)
def test_expand_ghosts(oracle64, name):
    """The expanded open system's all-pairs rows of the local atoms are the periodic oracle's rows under ghost -> (j, image);
    the full list offers every pair within Rcr + 1, the atom itself and nothing twice inside the cutoff."""
    case = nc.case_by_name(name)
    n = case.n_atoms
    lst = nx.oracle_list(oracle64, case, case.rcr + 1.0)
    ex = nx.expand_ghosts(case, lst, case.rcr + 1.0)
    m = ex.species.shape[1]
    assert ex.n_local == n and (m > n) == (name not in ("chunk129_pbc", "chunk256_open", "skew_FFF"))
    assert np.any(np.any(ex.ghost_image != 0, axis=1)) or m == n
    ecase = ex.as_case(case)
    start, ej, ed, er = nx.oracle_list(oracle64, ecase, case.rcr + nc.BAND)
    ei = np.repeat(np.arange(m), np.diff(start))
    loc = ei < n
    ei, ej, ed, er = ei[loc], ej[loc].astype(np.int64), ed[loc], er[loc]
    g = ej >= n
    back_j = np.where(g, ex.ghost_j[np.where(g, ej - n, 0)] if m > n else ej, ej)
    img = np.zeros((ej.size, 3), dtype=np.int64)
    if m > n:
        img[g] = ex.ghost_image[ej[g] - n]
    span = nx.IMG_SPAN
    ekey = ei * n + back_j
    for q in range(3):
        ekey = ekey * span + (img[:, q] + span // 2)
    xw = nc.wrap_f64(case)
    cell = case.cell.astype(np.float64) if case.periodic else None
    i, j, d, r, _ = nx.flat_pairs(case, lst, case.rcr + nc.BAND)
    okey = pair_keys(i, j, d, xw, cell, n)[0]
    assert np.unique(ekey).size == ekey.size
    assert np.all(np.isin(okey[r <= case.rcr - nc.BAND], ekey[er <= case.rcr])), f"{name}: the expansion loses a pair"
    assert np.all(np.isin(ekey[er <= case.rcr - nc.BAND], okey[r <= case.rcr])), f"{name}: the expansion adds a pair"
    # the list itself
    assert np.array_equal(np.sort(ex.ilist), np.nonzero(np.arange(n) % 7 != 3)[0])
    assert not np.array_equal(ex.ilist, np.sort(ex.ilist))
    assert (np.any(ex.numneigh == 0) or n < 6) and int(ex.numneigh.sum()) == ex.jlist.size
    first = np.cumsum(ex.numneigh) - ex.numneigh
    x = ex.coords.reshape(-1, 3).astype(np.float64)
    for q in np.random.RandomState(1).permutation(ex.ilist.size)[:40]:
        a = int(ex.ilist[q])
        row = ex.jlist[first[q]:first[q] + ex.numneigh[q]].astype(np.int64)
        if ex.numneigh[q] == 0:
            assert a % 11 == 5 and not ex.has_row[a]
            continue
        assert a in row and row.min() >= 0 and row.max() < m
        dist = np.linalg.norm(x[row] - x[a], axis=1)
        inside = row[(dist <= case.rcr + 0.5) & (row != a) & (ex.species.reshape(-1)[row] >= 0)]
        assert np.unique(inside).size == inside.size, f"{name}: atom {a} is offered a neighbor twice"
        want = ej[(ei == a) & (er <= case.rcr)]
        assert np.all(np.isin(want, row)), f"{name}: the list of atom {a} lacks a neighbor"
        assert np.any(dist > case.rcr + nc.BAND) or name == "tiny"


def test_synthetic_rows_expectation():
    """The count the synthetic table's half list must have: the kept entries, about half of all, and the same whichever way
    it is counted; a sub-range's list is a slice of the whole one's."""
    n = 5000
    s = nx.synthetic_rows(n, seed=2)
    m = s.meta.astype(np.int64)
    cnt = (m[:, 1] & 0xFFFF) + (m[:, 1] >> 16)
    assert cnt.min() == 0 and cnt.max() == 3 and np.array_equal(m[:, 0], 3 * np.arange(n))
    idx, diff, dist = nx.synthetic_half(s, 0, n)
    P = idx.shape[1]
    e = s.ent.reshape(n, 3, 4)
    j = (np.ascontiguousarray(e[..., 3]).view(np.uint32) & 0x0FFFFFFF).astype(np.int64)
    used = np.arange(3)[None, :] < cnt[:, None]
    i = np.broadcast_to(np.arange(n)[:, None], (n, 3))
    own = used & (j == i)
    pos = nx.first_nonzero_positive(e[..., :3].reshape(-1, 3)).reshape(n, 3)
    assert P == int((used & (j > i)).sum() + (own & pos).sum())
    assert own.sum() > 100 and 0.3 < (own & pos).sum() / own.sum() < 0.7
    # each branch of the own-image rule decides somewhere, with either sign
    d = e[..., :3][own]
    for lead in range(3):
        at = np.all(d[:, :lead] == 0, axis=1) & (d[:, lead] != 0)
        assert np.any(d[at, lead] > 0) and np.any(d[at, lead] < 0)
    assert np.all(idx[1] >= idx[0]) and np.any(idx[1] == idx[0]) and np.any(j[used] < i[used])
    assert np.array_equal(dist.astype(np.float64) ** 2, (diff.astype(np.float64) ** 2).sum(axis=1)) or \
        np.allclose(dist.astype(np.float64), np.sqrt((diff.astype(np.float64) ** 2).sum(axis=1)), rtol=6e-8, atol=0)
    lo, hi = 777, 4000
    sub = nx.synthetic_half(s, lo, hi)
    sel = (idx[0] >= lo) & (idx[0] < hi)
    assert np.array_equal(sub[0], idx[:, sel]) and np.array_equal(sub[1], diff[sel]) and np.array_equal(sub[2], dist[sel])
    assert nx.SCAN_TWICE_N > 256 * 1024


def test_gates():
    assert abs(nx.REFRESH_GATE - (5e-6 + 4 * 4.76837158203125e-07)) < 1e-12
    assert nx.REFRESH_BAND >= 2.0 * np.sqrt(3.0) * nx.REFRESH_GATE and nx.REFRESH_BAND < 2.5e-5
