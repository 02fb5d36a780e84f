"""fp64 numpy reference of the heat flux on the existing oracle (nothing in oracle/ changes), and the kernel cases that
tests/test_heat_flux_host.py and tests/test_gpu_heat_flux.py share.

For a cotangent w the oracle's VJP with only row i non-zero is the gradient of the scalar w_i . aev_i alone: on atom j != i it
is g_ij = d (w_i . aev_i) / d d_ij as long as the pair has a single image (open, or every periodic height >= 2 Rcr), and
q_i = sum_j d_ij (g_ij . v_j) with d_ij the fp64 minimum image.  One oracle call per row.  A cell too small for that is
replicated k_a x k_b x k_c times with replicated vectors until it is not: the rows of the first replica are the rows of the
cell, and J(supercell) = k_a k_b k_c J(cell).
"""
from __future__ import annotations

import functools
import math
import os
import typing as tp

import numpy as np

import _aev_cases as ac
import _aev_constants as akc

ACC_UNIT = 4.3597447222071e-18 / 1e-10 / 1.66053906660e-27 * 1e10 * 1e-30   # torchani_amd.md.ACC_UNIT, CODATA 2018
ROW_TOL = 2e-5      # per-centre rows: the VJP gate (tests/test_gpu_parity.py), x max(1, largest |entry| of the reference [N, 3])
SUM_TOL = 1e-4      # per-entry sums: the virial gate (tests/test_gpu_md.py), x max(1, largest entry)


@functools.lru_cache(maxsize=2)
def oracle(kind: str = "f64"):
    from oracle.oracle import Oracle

    return Oracle(kind)


def heights(cell: np.ndarray) -> np.ndarray:
    """Perpendicular widths of a cell [3, 3] (rows = lattice vectors)."""
    cell = np.asarray(cell, dtype=np.float64)
    vol = abs(np.linalg.det(cell))
    return np.array([vol / np.linalg.norm(np.cross(cell[(a + 1) % 3], cell[(a + 2) % 3])) for a in range(3)])


def replication(cell, pbc, rcr: float) -> tp.Tuple[int, int, int]:
    if cell is None or pbc is None:
        return (1, 1, 1)
    h = heights(cell)
    return tuple(int(math.ceil(2.0 * rcr / h[a] - 1e-12)) if pbc[a] else 1 for a in range(3))


def supercell(x: np.ndarray, cell, reps) -> tp.Tuple[np.ndarray, np.ndarray, int]:
    """(coordinates [K N, 3] with the first replica first, cell of the supercell, K)."""
    cell = np.asarray(cell, dtype=np.float64)
    shifts = [(a, b, c) for a in range(reps[0]) for b in range(reps[1]) for c in range(reps[2])]
    xs = np.concatenate([x + np.asarray(s, dtype=np.float64) @ cell for s in shifts])
    return xs, cell * np.asarray(reps, dtype=np.float64)[:, None], len(shifts)


def min_image(d: np.ndarray, cell, pbc) -> np.ndarray:
    if cell is None or pbc is None:
        return d
    cell = np.asarray(cell, dtype=np.float64)
    f = d @ np.linalg.inv(cell)
    f -= np.round(f) * np.asarray(pbc, dtype=np.float64)
    return f @ cell


def flux_rows(p, species, coords, w, v, cell=None, pbc=None, rows=None, kind: str = "f64") -> np.ndarray:
    """q [N, 3] fp64 of ONE system: species [N], coords [N, 3], cotangent w [N, L], vectors v [N, 3]; rows not in ``rows`` stay
    zero.  kind "f32": the oracle's own sums in fp32 (its g_ij), the contraction with d and v still in fp64."""
    o = oracle(kind)
    species = np.asarray(species, dtype=np.int32).reshape(-1)
    n = species.shape[0]
    x = np.asarray(coords, dtype=np.float64).reshape(n, 3)
    v = np.asarray(v, dtype=np.float64).reshape(n, 3)
    w = np.asarray(w, dtype=np.float64).reshape(n, -1)
    reps = replication(cell, pbc, float(p.Rcr))
    K = 1
    if reps != (1, 1, 1):
        x, cell, K = supercell(x, cell, reps)
    sp_s, v_s = np.tile(species, K), np.tile(v, (K, 1))
    q = np.zeros((n, 3))
    for i in (range(n) if rows is None else rows):
        if species[i] < 0:
            continue
        wi = np.zeros((K * n, w.shape[1]))
        wi[i] = w[i]
        _, g = o.aev(p, sp_s[None], x[None], cell, pbc, grad_aev=wi)
        g = np.asarray(g, dtype=np.float64).reshape(K * n, 3)
        g[i] = 0.0
        g[sp_s < 0] = 0.0
        d = min_image(x - x[i], cell, pbc)
        q[i] = ((g * v_s).sum(axis=1)[:, None] * d).sum(axis=0)
    return q


def flux_rows_batch(p, species, coords, w, v, cell=None, pbc=None, rows=None, kind: str = "f64") -> np.ndarray:
    """flux_rows molecule by molecule: species [C, A], coords / v [C, A, 3], w [C A, L]; rows: flat atom indices."""
    species = np.asarray(species)
    Cn, A = species.shape
    w = np.asarray(w).reshape(Cn, A, -1)
    out = np.zeros((Cn, A, 3))
    for c in range(Cn):
        r = None if rows is None else [k - c * A for k in rows if c * A <= k < (c + 1) * A]
        out[c] = flux_rows(p, species[c], coords[c], w[c], np.asarray(v).reshape(Cn, A, 3)[c], cell, pbc, r, kind)
    return out.reshape(Cn * A, 3)


def flux_sums(species, masses, energies, v, q) -> np.ndarray:
    """J [C, 3, 3] fp64: kinetic convective, potential convective, virial term, over the atoms with species >= 0."""
    species = np.asarray(species)
    Cn, A = species.shape
    real = (species >= 0)[..., None]
    v = np.asarray(v, dtype=np.float64).reshape(Cn, A, 3)
    ke = 0.5 * np.asarray(masses, dtype=np.float64).reshape(Cn, A) * (v * v).sum(axis=-1) / ACC_UNIT
    out = np.zeros((Cn, 3, 3))
    out[:, 0] = (ke[..., None] * v * real).sum(axis=1)
    out[:, 1] = (np.asarray(energies, dtype=np.float64).reshape(Cn, A, 1) * v * real).sum(axis=1)
    out[:, 2] = -(np.asarray(q, dtype=np.float64).reshape(Cn, A, 3) * real).sum(axis=1)
    return out


def model_flux(p, dims, flat, n_members, species, coords, v, masses, cell=None, pbc=None, sae=None) -> tp.Tuple[np.ndarray, np.ndarray]:
    """(J [C, 3, 3], q [C, A, 3]) of a model given as oracle networks: w from Oracle.mlp(want_grad=True), e_i its ensemble-mean
    atomic energies (plus sae[species] if given)."""
    o = oracle("f64")
    species = np.asarray(species)
    Cn, A = species.shape
    x = np.asarray(coords, dtype=np.float64)
    aev = o.aev(p, species, x, cell, pbc)
    ae, g, _ = o.mlp(species, aev, dims, flat, n_members=n_members)
    ae = np.asarray(ae, dtype=np.float64).reshape(Cn, A)
    if sae is not None:
        ae = ae + np.where(species >= 0, np.asarray(sae, dtype=np.float64)[np.clip(species, 0, None)], 0.0)
    q = flux_rows_batch(p, species, x, g, v, cell, pbc)
    return flux_sums(species, masses, ae, v, q), q.reshape(Cn, A, 3)


# ---- correlation and conductivity (numpy) ------------------------------------------------------------------------------------
def hfacf_ref(J: np.ndarray, lags: int) -> tp.Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(sums [C, M], origins [M], sum of |terms| [C, M]) of a series J [n, C, 3]: every sample k paired with k - l,
    l = 0 .. min(k, M - 1)."""
    n, Cn, _ = J.shape
    S, A = np.zeros((Cn, lags)), np.zeros((Cn, lags))
    for l in range(min(lags, n)):   # noqa: E741
        t = J[l:] * J[:n - l]
        S[:, l] = t.sum(axis=(0, 2))
        A[:, l] = np.abs(t).sum(axis=(0, 2))
    return S, np.maximum(n - np.arange(lags), 0), A


def trapezoid(h: np.ndarray, dt: float) -> np.ndarray:
    """Running trapezoid integral of h [..., M] sampled every dt: out[..., l] = int_0^{l dt}."""
    out = np.zeros_like(h)
    out[..., 1:] = np.cumsum(0.5 * (h[..., 1:] + h[..., :-1]), axis=-1) * dt
    return out


# ---- kernel cases -------------------------------------------------------------------------------------------------------------
class FluxCase(tp.NamedTuple):
    name: str
    species: np.ndarray                    # [C, A] int32, -1 = padding
    coords: np.ndarray                     # [C, A, 3] float32
    cell: tp.Optional[np.ndarray]
    pbc: tp.Optional[tp.Tuple[bool, bool, bool]]
    grids: tp.Tuple[str, ...]              # "2x" (8 x 4), "1x" (4 x 8), "general", or the name of a sweep set
    rows: tp.Optional[tp.Tuple[int, ...]]  # flat indices of the rows the reference computes (None: all)
    sub: tp.Optional[tp.Tuple[int, int]] = None   # also run the central range lo..hi alone

    @property
    def n_atoms(self) -> int:
        return int(self.species.size)


def _cluster(seed: int, n: int, box: float, S: int, dmin: float = 0.8) -> tp.Tuple[np.ndarray, np.ndarray]:
    rs = np.random.RandomState(seed)
    pts: tp.List[np.ndarray] = []
    while len(pts) < n:
        c = rs.uniform(0.0, box, 3)
        if all(np.linalg.norm(c - q) >= dmin for q in pts):
            pts.append(c)
    return rs.randint(0, S, n).astype(np.int32), np.asarray(pts, dtype=np.float32)


def _radial_only() -> FluxCase:
    """Five atoms on a bent chain 4.2 A apart: every neighbor lies between Rca = 3.5 and Rcr >= 5.1, so no row has an angular
    neighbor and every term is a radial-only push; plus a tight triple 20 A away whose rows have both kinds."""
    chain = np.array([[0, 0, 0], [4.2, 0, 0], [8.4, 0.3, 0], [12.5, 1.0, 0.4], [16.6, 1.2, 1.0]], dtype=np.float32)
    triple = np.array([[0, 20, 0], [1.1, 20.2, 0.1], [0.3, 21.2, 0.4], [4.3, 20.5, 0.2]], dtype=np.float32)
    sp = np.array([[0, 1, 2, 3, 0, 1, 0, 3, 2]], dtype=np.int32)
    return FluxCase("radial_only", sp, np.concatenate([chain, triple])[None], None, None, ("2x", "1x", "general"), None)


def _batch3() -> FluxCase:
    """Three molecules of 11, 6 and 1 atoms in one batch: padding atoms, and an atom without neighbors."""
    A = 11
    sp = np.full((3, A), -1, dtype=np.int32)
    x = np.zeros((3, A, 3), dtype=np.float32)
    for c, (n, seed) in enumerate(((11, 5), (6, 6), (1, 7))):
        s, p = _cluster(seed, n, 3.2, 4)
        sp[c, :n], x[c, :n] = s, p
    x[sp < 0] = 0.0
    return FluxCase("batch3", sp, x, None, None, ("2x", "1x", "general"), None, sub=(3, 15))


def _from_aev(name: str, grids, rows=None, sub=None) -> FluxCase:
    c = ac.case_by_name(name)
    n = c.n_atoms
    if rows == "centre+":   # the long row and eight seeded others
        rs = np.random.RandomState(3)
        rows = tuple(sorted({int(c.centre)} | set(int(k) for k in rs.choice(n, 8, replace=False))))
    return FluxCase(name, c.species.astype(np.int32), c.coords, c.cell, c.pbc, grids, rows, sub)


def _sweep_case(set_name: str) -> FluxCase:
    run = next(r for r in akc.sweep_runs() if r[0] == set_name)
    g = akc.geometry_of(run)
    return FluxCase(f"{set_name}:{run[1]}", g.species.astype(np.int32), g.coords, g.cell, g.pbc, (set_name,), None)


SWEEP_SMOOTH = "sweep17"   # smooth cutoff, 8 x 4, six species, both recurrences, a triclinic cell
SWEEP_NO_REC = "sweep00"   # cosine cutoff, 4 x 8, five species, neither recurrence, a batch of three


@functools.lru_cache(maxsize=1)
def cases() -> tp.Tuple[FluxCase, ...]:
    one = FluxCase("single_atom", np.array([[2]], dtype=np.int32), np.zeros((1, 1, 3), dtype=np.float32), None, None,
                   ("2x", "1x", "general"), None)
    out = (
        _radial_only(),
        one,
        _batch3(),
        _from_aev("chunk63_open/built", ("2x", "1x", "general"), sub=(10, 40)),    # rows of <= 64 entries
        _from_aev("chunk65_open/built", ("2x", "1x", "general")),                  # 65 entries: the second radial chunk
        _from_aev("ang65_open/built", ("2x", "1x", "general"), rows="centre+"),             # 65 angular: the one-part tournament
        _from_aev("images12_pbc/built", ("2x", "1x", "general")),                  # an atom's own image: supercell reference
        _sweep_case(SWEEP_SMOOTH),
        _sweep_case(SWEEP_NO_REC),
    )
    assert akc.set_by_name(SWEEP_SMOOTH).cutoff_fn == "smooth" and akc.set_by_name(SWEEP_NO_REC).flags == 0
    return out


def case_by_name(name: str) -> FluxCase:
    return next(c for c in cases() if c.name == name)


def runs() -> tp.Tuple[tp.Tuple[str, str], ...]:
    return tuple((c.name, g) for c in cases() for g in c.grids)


def run_id(run) -> str:
    return f"{run[0]}-{run[1]}".replace("/", "_").replace(":", "_")


def constants(grid: str):
    """AEVConstants of a grid name, with seven species for "2x" / "general" and four for "1x"."""
    from torchani_amd.constants import AEVConstants, aev_constants_1x, aev_constants_2x

    if grid == "2x":
        return aev_constants_2x(7)
    if grid == "1x":
        return aev_constants_1x(4)
    if grid == "general":
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid_r5_a3z5_dense.npz")) as z:
            return AEVConstants(7, float(z["Rcr"]), float(z["Rca"]), float(z["EtaR"]), tuple(z["ShfR"].tolist()),
                                float(z["EtaA"]), float(z["Zeta"]), tuple(z["ShfA"].tolist()), tuple(z["ShfZ"].tolist()),
                                str(z["cutoff_fn"]))
    return akc.set_by_name(grid).aev_constants()


def oracle_params_of(c):
    from oracle import oracle as orc

    return orc.make_params(c.num_species, c.Rcr, c.Rca, c.EtaR, c.EtaA, c.Zeta, c.ShfR, c.ShfA, c.ShfZ, c.cutoff_fn)


class Ref(tp.NamedTuple):
    w: np.ndarray       # [N, L] float32: the cotangent
    v: np.ndarray       # [N, 3] float32: the vectors, uniform in [-1, 1]
    q: np.ndarray       # [N, 3] fp64 (zero outside ``rows``)
    rows: np.ndarray    # the rows computed


def inputs(run) -> tp.Tuple[np.ndarray, np.ndarray]:
    case, c = case_by_name(run[0]), constants(run[1])
    rs = np.random.RandomState(1000)
    w = rs.uniform(-1.0, 1.0, (case.n_atoms, c.out_dim)).astype(np.float32)
    v = rs.uniform(-1.0, 1.0, (case.n_atoms, 3)).astype(np.float32)
    return w, v


@functools.lru_cache(maxsize=None)
def reference(run, kind: str = "f64") -> Ref:
    case = case_by_name(run[0])
    p = oracle_params_of(constants(run[1]))
    w, v = inputs(run)
    q = flux_rows_batch(p, case.species, case.coords.astype(np.float64), w, v, case.cell, case.pbc, case.rows, kind)
    rows = np.arange(case.n_atoms) if case.rows is None else np.asarray(case.rows)
    return Ref(w, v, q, rows)


def row_gate(ref: Ref) -> float:
    return ROW_TOL * max(1.0, float(np.abs(ref.q).max()))


def sum_gate(total: np.ndarray) -> float:
    return SUM_TOL * max(1.0, float(np.abs(total).max()))
