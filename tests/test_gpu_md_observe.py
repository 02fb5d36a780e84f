"""The MD observers (csrc/md_observe.hip, torchani_amd/md_observe.py) on the MI355X against the fp64 reference of
tests/_md_observe_ref.py: the two entry points through the C ABI on synthetic states, then the observers through
``BatchedDynamics`` and its subclasses on a standalone Lennard-Jones potential.

Gates, derived and not measured.  RDF counts are integers and must equal the reference's on the fp32-rounded coordinates, but for
pairs whose fp64 distance lies within 2e-5 A of a bin edge or of r_max (a few fp32 ulps of coordinates below 32 A, 1.9e-6 A
each, in the engine's fp32 difference): a bin may differ by the number of such pairs at its two edges, and they must be at most
1 % of the pairs of the case.  MSD: 1e-10 relative (an fp64 sum of up to 1e5 non-negative terms gives about 1e-11); VACF: 1e-10
of the sum of the absolute terms; two runs bit-identical; guard words around every buffer untouched."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _md_observe_ref as obr
from test_gpu_md_device import SEED, _stream
from test_gpu_md_replica_exchange import _lj_replicas

pytestmark = pytest.mark.gpu

GUARD = 16
EDGE_MARGIN = 2e-5     # Angstrom
EDGE_SHARE = 0.01
SUM_GATE = 1e-10
ACC_UNIT = 4.3597447222071e-18 / 1e-10 / 1.66053906660e-27 * 1e10 * 1e-30


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from torchani_amd import _lib

    _lib.lib()
    return torch.device("cuda:0")


def _guarded(dev, shape, dtype, fill):
    """A zeroed tensor of ``shape`` between two runs of GUARD elements of ``fill``: (the view, the whole buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    buf[GUARD:GUARD + n] = 0
    return buf[GUARD:GUARD + n].view(*shape), buf


def _guards_intact(buf, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


# ---- anihip_md_rdf_accumulate ----------------------------------------------------------------------------------------------

def _random_box(rs, Cn, A, box, n_species, n_real=None):
    sp = rs.randint(0, n_species, (Cn, A)).astype(np.int64)
    if n_real is not None:
        for c, n in enumerate(n_real):
            sp[c, n:] = -1
    x = rs.uniform(0.0, box, (Cn, A, 3)).astype(np.float32)
    return sp, x


ALL_PAIRS_3 = [(a, b) for a in range(3) for b in range(3)][:8]   # eight of the nine ordered pairs: (2, 2) is unwanted
RDF_CASES = {
    # name: (C, A, real atoms, box, cell, species, pairs, r_max, bins, rows' cutoff or None for r_max)
    "one_atom_no_pairs": (3, 1, None, 1.0, None, 1, [(0, 0)], 3.0, 8, None),
    "rows_of_65_to_256": (1, 150, None, 7.0, None, 1, [(0, 0)], 6.0, 120, None),
    "two_entries_with_padding": (2, 40, (40, 23), 5.0, None, 2, [(0, 1), (1, 1)], 4.0, 64, None),
    "257_entries_of_3": (257, 3, None, 2.0, None, 2, [(0, 0), (0, 1), (1, 0)], 3.0, 32, None),
    "entries_change_between_rounds": (5, 8, (8, 5, 8, 1, 7), 3.0, None, 2, [(0, 0), (1, 0)], 3.0, 16, None),
    "one_bin_one_pair_of_three_species": (1, 60, None, 6.0, None, 3, [(2, 0)], 4.0, 1, None),
    "1024_bins_in_a_14A_cell": (1, 300, None, 14.0, 14.0, 1, [(0, 0)], 6.0, 1024, None),
    "eight_pairs_of_three_species": (2, 70, (70, 64), 6.0, None, 3, ALL_PAIRS_3, 5.0, 120, None),
    "6A_cell_5A_reach": (1, 20, None, 6.0, 6.0, 2, [(0, 0), (0, 1), (1, 1)], 5.0, 100, None),
    "own_image_in_a_4p43A_cell": (1, 14, None, 4.43, (4.43, 6.1, 6.47), 1, [(0, 0)], 5.0, 100, None),
    "r_max_below_the_rows_cutoff": (2, 50, (50, 31), 6.0, None, 2, [(0, 0), (1, 0)], 3.5, 70, 6.0),
    "cell_list_rows_of_520_atoms": (1, 520, None, 16.0, 16.0, 2, [(0, 1), (1, 1)], 5.0, 200, None),
}


_RDF_REFERENCE = {}


@pytest.mark.parametrize("per_entry", [False, True], ids=["summed", "per_entry"])
@pytest.mark.parametrize("case", list(RDF_CASES))
def test_rdf_accumulate_counts_what_the_reference_counts(dev, case, per_entry):
    from torchani_amd import _lib
    from torchani_amd.constants import aev_constants_2x
    from torchani_amd.engine import AevEngine

    Cn, A, n_real, box, cell, n_sp, pairs, r_max, bins, r_rows = RDF_CASES[case]
    rs = np.random.RandomState(sum(map(ord, case)))
    sp, x = _random_box(rs, Cn, A, box, n_sp, n_real)
    pbc = (False,) * 3
    cell_np = cell_t = None
    if cell is not None:
        cell_np = np.diag(np.broadcast_to(np.asarray(cell, dtype=np.float64), (3,)))
        x = (x * (np.diag(cell_np) / box)).astype(np.float32) if np.ndim(cell) else x
        cell_t, pbc = torch.from_numpy(cell_np).to(dev), (True,) * 3
    if case not in _RDF_REFERENCE:   # (once per case: the summed counts are the per-entry ones added up)
        _RDF_REFERENCE[case] = obr.rdf_counts(sp, x, pairs, r_max, bins, cell_np, pbc, per_entry=True, margin=EDGE_MARGIN)
    want, near = _RDF_REFERENCE[case] if per_entry else tuple(t.sum(0) for t in _RDF_REFERENCE[case])
    n_pairs_case = int(want.sum())
    if case != "one_atom_no_pairs":
        assert n_pairs_case > 0
    share = near.sum() / max(n_pairs_case, 1)
    assert share <= EDGE_SHARE, f"{case}: {share:.2%} of the pairs lie on an edge"

    species32 = torch.from_numpy(sp).to(device=dev, dtype=torch.int32).contiguous()
    coords = torch.from_numpy(x).to(dev).contiguous()
    engine = AevEngine(aev_constants_2x(max(n_sp, 1))._replace(Rcr=float(r_rows or r_max), Rca=1e-3))
    mode = "cell" if (Cn == 1 and A > 512) else "batch"
    rows = engine.neighbors(species32, coords, cell_t, pbc, mode=mode, row_cap=_lib.MAX_RAD)
    assert not rows.overflowed()
    if case == "rows_of_65_to_256":
        longest = int(((rows.meta[:, 1] & 0xFFFF) + ((rows.meta[:, 1] >> 16) & 0xFFFF)).max())
        assert 64 < longest <= 256, longest
    table = (C.c_int8 * 64)(*([-1] * 64))
    for p, (a, b) in enumerate(pairs):
        table[8 * a + b] = p
    shape = (Cn, len(pairs), bins) if per_entry else (len(pairs), bins)
    fill = -(1 << 40)
    counts, whole = _guarded(dev, shape, torch.int64, fill)
    params = _lib.MdParams(Cn, A, 0, 0, 1.0, 0, 0)
    for _ in range(2):   # two samples of the same state: twice the counts
        _lib.check(_lib.lib().anihip_md_rdf_accumulate(
            _stream(), C.byref(params), len(pairs), bins, r_max, int(per_entry), table, species32.data_ptr(),
            rows.meta.data_ptr(), rows.ent.data_ptr(), rows.ent.shape[0], counts.data_ptr()))
    torch.cuda.synchronize()
    assert _guards_intact(whole, fill)
    got = counts.cpu().numpy()
    assert (got % 2 == 0).all()
    diff = np.abs(got // 2 - want)
    allowed = near[..., :-1] + near[..., 1:]   # (edge 0 is r = 0: no pair)
    print(f"md observe, rdf {case} ({'per entry' if per_entry else 'summed'}): {n_pairs_case} pairs, {int(near.sum())} within "
          f"{EDGE_MARGIN:g} A of an edge ({share:.3%}), {int(diff.sum())} counted on the other side, rows up to "
          f"{int(((rows.meta[:, 1] & 0xFFFF) + ((rows.meta[:, 1] >> 16) & 0xFFFF)).max())} entries")
    assert (diff <= allowed).all(), (case, np.argwhere(diff > allowed)[:5], diff.max())
    assert abs(int(got.sum()) // 2 - n_pairs_case) <= int(near[..., -1].sum())   # (only r_max lets a pair in or out)


# ---- anihip_md_corr_accumulate ---------------------------------------------------------------------------------------------

CORR_CASES = {
    # name: (C, A, species, lags, padding)
    "one_atom": (2, 1, 1, 2, False),
    "63_atoms_one_lag": (2, 63, 1, 1, False),
    "64_atoms_7_species": (1, 64, 7, 2, False),
    "65_atoms_64_lags_padding": (3, 65, 7, 64, True),
    "255_atoms_65_lags": (2, 255, 2, 65, False),
    "256_atoms": (2, 256, 2, 3, False),
    "257_atoms_two_chunks_padding": (2, 257, 7, 3, True),
    "257_entries_of_3_padding": (257, 3, 2, 2, True),
}


class CorrAbi:
    """One correlation through the C ABI: the gather tables of the observer's builder, ring, sums and workspace between guards."""

    def __init__(self, dev, kind, species, lags):
        from torchani_amd import _lib, md

        self.L, self.kind, self.lags = _lib.lib(), kind, lags
        _, gather, gather_species, _ = md.MeanSquaredDisplacement(lags=lags, every=1)._tables(torch.from_numpy(species))
        self.Cn, self.A = species.shape
        self.G, self.S = gather.shape[1], int(species.max()) + 1
        self.gather, self.gather_species = gather.to(dev), gather_species.to(dev)
        msd = kind == _lib.MD_CORR_MSD
        self.ring, self.ring_whole = _guarded(dev, (lags, self.Cn, 3, self.G), torch.float64 if msd else torch.float32, -7.0)
        self.sums, self.sums_whole = _guarded(dev, (self.Cn, self.S, lags), torch.float64, -7.0)
        nbytes = self.L.anihip_md_corr_workspace_bytes(self.Cn, self.G, lags, self.S)
        assert nbytes == self.Cn * -(-self.G // 256) * self.S * lags * 8
        self.ws, self.ws_whole = _guarded(dev, (nbytes // 8,), torch.float64, -7.0)
        self.params = _lib.MdParams(self.Cn, self.A, 0, 0, 1.0, 0, 0)
        self.k = 0

    def add(self, x, x_lo=None):
        from torchani_amd import _lib

        _lib.check(self.L.anihip_md_corr_accumulate(
            _stream(), C.byref(self.params), self.kind, self.lags, self.S, self.G, self.k, self.gather.data_ptr(),
            self.gather_species.data_ptr(), x.data_ptr(), None if x_lo is None else x_lo.data_ptr(), self.ring.data_ptr(),
            self.sums.data_ptr(), self.ws.data_ptr(), self.ws.numel() * 8))
        self.k += 1

    def intact(self):
        return all(_guards_intact(b, -7.0) for b in (self.ring_whole, self.sums_whole, self.ws_whole))


@pytest.mark.parametrize("kind", ["msd", "vacf"])
@pytest.mark.parametrize("case", list(CORR_CASES))
def test_corr_accumulate_sums_what_the_reference_sums(dev, case, kind):
    from torchani_amd import _lib

    Cn, A, S, M, padding = CORR_CASES[case]
    rs = np.random.RandomState(sum(map(ord, case)))
    species = rs.randint(0, S, (Cn, A)).astype(np.int64)
    species[0, :min(S, A)] = np.arange(min(S, A))   # (every species is there)
    if padding:   # (the tail of the last entry and, where every species stays, the last atom of the first)
        species[-1, A - max(A // 3, 1):] = -1
        if A > S:
            species[0, -1] = -1
    n_samples = 2 * M + 3
    steps = rs.normal(size=(n_samples, Cn, A, 3)) * 0.05
    xs = 3.0 + np.cumsum(steps, axis=0) if kind == "msd" else steps * 4.0
    hi = xs.astype(np.float32)
    lo = ((xs - hi) if kind == "msd" else np.zeros_like(xs)).astype(np.float32)
    exact = hi.astype(np.float64) + lo.astype(np.float64)   # what the kernel forms
    ref = obr.Correlation(kind, species, S, M)
    runs = [CorrAbi(dev, _lib.MD_CORR_MSD if kind == "msd" else _lib.MD_CORR_VACF, species, M) for _ in range(2)]
    check_at = sorted({max(M - 1, 1), M, n_samples})   # fewer samples than lags (where there can be), exactly M, wrapped
    worst = 0.0
    for k in range(n_samples):
        ref.add(exact[k])
        h, l = torch.from_numpy(hi[k]).to(dev), torch.from_numpy(lo[k]).to(dev)   # noqa: E741
        for run in runs:
            run.add(h, l if kind == "msd" else None)
        if k + 1 in check_at:
            got = runs[0].sums.cpu().numpy()
            assert torch.equal(runs[0].sums, runs[1].sums) and torch.equal(runs[0].ring, runs[1].ring)
            n_l = np.maximum(k + 1 - np.arange(M), 0)
            assert np.array_equal(ref.origins, n_l)
            assert (got[:, :, n_l == 0] == 0.0).all()
            if kind == "msd":
                assert (got[:, :, 0] == 0.0).all()
                err = np.abs(got - ref.sums) / np.where(ref.sums > 0, ref.sums, 1.0)
            else:
                err = np.abs(got - ref.sums) / np.where(ref.abs_sums > 0, ref.abs_sums, 1.0)
            worst = max(worst, float(err.max()))
            assert err.max() <= SUM_GATE, (case, kind, k + 1, err.max())
    assert all(run.intact() for run in runs)
    print(f"md observe, {kind} {case}: C = {Cn}, A = {A}, {S} species, {M} lags, {n_samples} samples: worst error "
          f"{worst:.1e} of {'the sum' if kind == 'msd' else 'sum |terms|'} (gate {SUM_GATE:g}); two runs bit-identical")


# ---- through the dynamics ---------------------------------------------------------------------------------------------------

def _all_five(md, every, lags=4):
    return [md.TimeSeries(("potential", "kinetic", "total", "temperature"), every=every, capacity=8),
            md.Trajectory(every=every, capacity=8, velocities=True),
            md.RadialDistribution([("H", "H")], r_max=3.0, bins=32, every=every, per_entry=True),
            md.MeanSquaredDisplacement(lags=lags, every=every), md.VelocityAutocorrelation(lags=lags, every=every)]


@pytest.mark.parametrize("on_full", ["raise", "wrap"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_series_and_frames_are_the_accessors_at_the_sampled_steps(dev, dtype, on_full):
    from torchani_amd import md

    lj, sp, x, mass = _lj_replicas(dev)
    dyn = md.BatchedDynamics(lj, sp, x, dt=1.0, masses=mass, temperature=120.0, friction=0.05, seed=SEED)
    dyn.set_temperature(120.0)
    names = ("potential", "kinetic", "total", "temperature")
    ts = dyn.attach(md.TimeSeries(names, every=2, capacity=3, on_full=on_full))
    trj = dyn.attach(md.Trajectory(every=2, capacity=3, velocities=True, dtype=dtype, on_full=on_full))
    assert isinstance(ts, md.TimeSeries) and isinstance(trj, md.Trajectory)
    kept = []
    for s in range(6 if on_full == "raise" else 9):
        dyn.step()
        if dyn.steps_done % 2 == 0:
            frame = dyn.coordinates.clone() if dtype == torch.float32 else dyn.coordinates.double() + dyn.coordinates_lo.double()
            kept.append((dyn.steps_done, [dyn.potential_energies.clone(), dyn.kinetic_energies(), dyn.total_energies(),
                                          dyn.temperatures()], frame, dyn.velocities.clone()))
    if on_full == "raise":
        dyn.step()
        with pytest.raises(RuntimeError, match="is full: 3 samples"):
            dyn.step()
    kept = kept[-3:]
    assert ts.steps().tolist() == trj.steps().tolist() == [k[0] for k in kept]
    for q, name in enumerate(names):
        got = ts.values(name)
        assert got.dtype == torch.float64 and torch.equal(got, torch.stack([k[1][q] for k in kept])), name
    assert trj.frames().dtype == dtype and torch.equal(trj.frames(), torch.stack([k[2] for k in kept]))
    assert torch.equal(trj.velocity_frames(), torch.stack([k[3] for k in kept]))
    with pytest.raises(ValueError, match="bias="):
        dyn.attach(md.TimeSeries(("cv",), 1, 2))
    with pytest.raises(ValueError, match="ReplicaExchange"):
        dyn.attach(md.TimeSeries(("rung",), 1, 2))


def test_samples_do_not_synchronize(dev):
    from torchani_amd import md

    lj, sp, x, mass = _lj_replicas(dev)
    dyn = md.BatchedDynamics(lj, sp, x, dt=1.0, masses=mass, temperature=120.0, friction=0.05, seed=SEED)
    dyn.set_temperature(120.0)
    observers = [dyn.attach(o) for o in _all_five(md, every=2)]
    for _ in range(2):   # (the first sample of every observer loads its kernels)
        dyn.step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(8):
            dyn.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert dyn.steps_done == 10 and [o.n_samples for o in observers] == [5] * 5
    dyn.run(2)   # (the periodic host checks read the observers' status)
    assert int(observers[2].counts().sum()) > 0 and float(observers[4].vacf()[:, :, 0].min()) > 0.0


def test_without_observers_the_parent_path_runs_bit_for_bit(dev):
    """No observer, and observers that are never due, against a dynamics whose ``step()`` is the body it had before there were
    observers (``_advance`` alone)."""
    from torchani_amd import md

    lj, sp, x, mass = _lj_replicas(dev)
    kw = dict(dt=1.0, masses=mass, temperature=120.0, friction=0.05, seed=SEED)
    new = [md.BatchedDynamics(lj, sp, x, **kw), md.BatchedDynamics(lj, sp, x, **kw)]
    idle = [new[1].attach(o) for o in _all_five(md, every=100)]
    assert new[0]._observers == []

    class Before(md.BatchedDynamics):
        step = md.BatchedDynamics._advance

    old = Before(lj, sp, x, **kw)
    for d in new + [old]:
        d.set_temperature(120.0)
        d.run(8)
    assert [o.n_samples for o in idle] == [0] * 5
    for d in new:
        for name in ("coordinates", "coordinates_lo", "velocities", "forces", "potential_energies"):
            assert torch.equal(getattr(d, name), getattr(old, name)), name


def test_free_flight_gives_ballistic_msd_and_constant_vacf(dev):
    from torchani_amd import md
    from torchani_amd.potentials import LennardJones

    lj = LennardJones(("H",), eps=(0.002,), sigma=(1.0,), cutoff=3.0).to(dev)
    grid = np.stack(np.meshgrid(np.arange(2), np.arange(2), np.arange(2), indexing="ij"), -1).reshape(-1, 3) * 12.0
    x = torch.from_numpy(np.tile(grid.astype(np.float32), (2, 1, 1))).to(dev)
    sp = torch.ones((2, 8), dtype=torch.int64, device=dev)
    dyn = md.BatchedDynamics(lj, sp, x, dt=0.5, masses=torch.full((2, 8), 12.011, device=dev), seed=SEED)   # NVE
    dyn.set_temperature(300.0)
    v = dyn.velocities.double().clone()
    every, lags = 3, 16
    msd = dyn.attach(md.MeanSquaredDisplacement(lags=lags, every=every))
    vac = dyn.attach(md.VelocityAutocorrelation(lags=lags, every=every))
    dyn.run(every * (2 * lags + 3), check_every=50)
    assert float(dyn.forces.abs().max()) == 0.0 and torch.equal(dyn.velocities.double(), v)
    v2 = v.pow(2).sum(dim=-1).mean(dim=1)   # [C]
    t = msd.times().to(dev)
    assert msd.times().tolist() == [l * every * 0.5 for l in range(lags)] and msd.species_values.tolist() == [1]
    got, want = msd.msd()[:, 0, 1:], v2.view(-1, 1) * t[1:] ** 2
    rel = ((got - want).abs() / want).max().item()
    flat = ((vac.vacf()[:, 0] - v2.view(-1, 1)).abs() / v2.view(-1, 1)).max().item()
    print(f"md observe, free flight: MSD within {rel:.1e} of <|v|^2> t^2 (gate 1e-5), VACF constant to {flat:.1e} (gate 1e-10)")
    assert float(msd.msd()[:, 0, 0].abs().max()) == 0.0 and rel <= 1e-5 and flat <= 1e-10
    assert torch.allclose(msd.total(), msd.msd()[:, 0], rtol=1e-14, equal_nan=True)
    d = msd.diffusion_coefficients(fit=(lags // 2, lags))   # (a parabola's slope over t0 .. t1 is <|v|^2> (t0 + t1))
    assert torch.allclose(d[:, 0] * 6.0, v2 * (t[lags // 2] + t[lags - 1]), rtol=1e-4)


def test_fixed_simple_cubic_lattice_has_its_shells(dev):
    from torchani_amd import md
    from torchani_amd.potentials import LennardJones

    a, n = 2.0, 3
    lj = LennardJones(("H",), eps=(0.002,), sigma=(1.0,), cutoff=3.0).to(dev)
    grid = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(1, -1, 3) * a + 0.3
    x = torch.from_numpy(grid.astype(np.float32)).to(dev)
    sp = torch.ones((1, n ** 3), dtype=torch.int64, device=dev)
    cell = torch.eye(3, device=dev) * (n * a)
    dyn = md.BatchedDynamics(lj, sp, x, cell, (True, True, True), dt=0.5, masses=torch.full((1, n ** 3), 12.011, device=dev),
                             fixed=torch.ones((1, n ** 3), dtype=torch.bool, device=dev), seed=SEED)
    bins, r_max = 25, 3.75   # (bins of 0.15 A: the shells at a, sqrt(2) a and sqrt(3) a sit well inside bins 13, 18 and 23)
    rdf = dyn.attach(md.RadialDistribution([("H", "H")], r_max=r_max, bins=bins, every=2))
    dyn.run(6)
    assert rdf.n_samples == 3 and tuple(rdf.counts().shape) == (1, bins)
    cn = rdf.coordination_numbers()[0]
    steps = torch.diff(cn, prepend=cn.new_zeros(1))
    assert {int(b): float(steps[b]) for b in steps.nonzero().view(-1)} == {13: 6.0, 18: 12.0, 23: 8.0}
    assert rdf.counts()[0].cpu().numpy().astype(np.int64).sum() == 3 * 27 * 26
    edges = rdf.edges().to(dev)
    shell = 4.0 * math.pi / 3.0 * (edges[1:] ** 3 - edges[:-1] ** 3)
    back = torch.cumsum(rdf.g()[0] * (27.0 / float(dyn.volumes())) * shell, 0)
    assert torch.allclose(back, cn, rtol=1e-12, atol=0.0)
    rdf.reset()
    assert rdf.n_samples == 0 and int(rdf.counts().cpu().numpy().astype(np.int64).sum()) == 0
    open_dyn = md.BatchedDynamics(lj, sp, x, dt=0.5, masses=torch.full((1, n ** 3), 12.011, device=dev))
    free = open_dyn.attach(md.RadialDistribution([("H", "H")], r_max=r_max, bins=bins, every=1))
    open_dyn.run(1)
    assert float(free.coordination_numbers()[0, -1]) < 26.0   # (no images: the faces have fewer neighbors)
    with pytest.raises(ValueError, match="coordination_numbers"):
        free.g()


def test_an_overflowing_row_raises_at_the_periodic_check(dev):
    from torchani_amd import md
    from torchani_amd.potentials import LennardJones

    rs = np.random.RandomState(5)
    lj = LennardJones(("H",), eps=(1e-6,), sigma=(0.1,), cutoff=0.3).to(dev)
    x = torch.from_numpy(rs.uniform(0.0, 5.0, (1, 300, 3)).astype(np.float32)).to(dev)
    sp = torch.ones((1, 300), dtype=torch.int64, device=dev)
    dyn = md.BatchedDynamics(lj, sp, x, dt=0.5, masses=torch.full((1, 300), 12.011, device=dev),
                             fixed=torch.ones((1, 300), dtype=torch.bool, device=dev))
    dyn.attach(md.RadialDistribution([("H", "H")], r_max=9.0, bins=10, every=1))   # 299 neighbors: a row holds 256
    with pytest.raises(RuntimeError, match="lower r_max"):
        dyn.run(2, check_every=1)


def test_dimers_vibrate_at_the_harmonic_frequency(dev):
    from torchani_amd import md
    from torchani_amd.potentials import LennardJones

    eps, sigma, mass, dt, every = 0.002, 1.0, 12.011, 2.0, 4
    omega = math.sqrt(57.146 * eps * ACC_UNIT / (sigma ** 2 * (mass / 2.0)))   # 1 / fs
    lags = int(round(math.pi / (0.02 * omega) / (every * dt)))   # one frequency bin pi / (lags every dt) = 2 % of omega
    lj = LennardJones(("H",), eps=(eps,), sigma=(sigma,)).to(dev)
    x = torch.zeros((64, 2, 3), dtype=torch.float32, device=dev)
    x[:, 1, 0] = 2.0 ** (1.0 / 6.0) * sigma + 0.01 * sigma
    dyn = md.BatchedDynamics(lj, torch.ones((64, 2), dtype=torch.int64, device=dev), x, dt=dt,
                             masses=torch.full((64, 2), mass, device=dev))
    vac = dyn.attach(md.VelocityAutocorrelation(lags=lags, every=every))
    dyn.run(every * (lags + 120), check_every=10_000)
    wn, density = vac.spectrum()
    assert tuple(density.shape) == (64, 1, lags)
    peak = wn[density[:, 0].argmax(dim=-1)]
    want = omega / (2.0 * math.pi * 2.99792458e-5)
    print(f"md observe, LJ dimers: harmonic {want:.1f} 1/cm, spectrum peak {float(peak[0]):.1f} 1/cm, one bin {float(wn[1]):.1f} 1/cm "
          f"({float(wn[1]) / want:.2%} of it), {lags} lags")
    assert abs(float(wn[1]) / want - 0.02) < 1e-3
    assert float((peak - want).abs().max()) <= float(wn[1])


def test_replica_exchange_is_sampled_after_the_attempt(dev):
    from torchani_amd import md

    lj, sp, x, mass = _lj_replicas(dev)
    T = md.temperature_ladder(100.0, 130.0, 5)
    dyn = md.ReplicaExchangeDynamics(lj, sp, x, dt=1.0, masses=mass, temperature=T, friction=0.02, exchange_every=2, seed=7)
    dyn.set_temperature(T)
    ts = dyn.attach(md.TimeSeries(("rung", "temperature"), every=2, capacity=16))
    trj = dyn.attach(md.Trajectory(every=2, capacity=16, velocities=True))
    rungs, velocities = [], []
    for s in range(16):
        dyn.step()
        if (s + 1) % 2 == 0:
            rungs.append(dyn.rungs())
            velocities.append(dyn.velocities.clone())
    assert dyn.attempts_done == 8 and int(dyn.exchange_accepts.sum()) > 0, "no swap: nothing was rescaled"
    series = ts.values("rung")
    assert series.dtype == torch.float64 and torch.equal(series.to(torch.int32), torch.stack(rungs))
    assert len({tuple(r.tolist()) for r in rungs}) > 1
    assert torch.equal(trj.velocity_frames(), torch.stack(velocities))   # the rescaled ones


def test_ring_polymers_take_the_rdf_and_refuse_the_correlations(dev):
    from torchani_amd import md

    lj, sp, x, mass = _lj_replicas(dev, Cn=2)
    dyn = md.RingPolymerDynamics(lj, sp, x, beads=4, temperature=100.0, dt=0.5, masses=mass, seed=3)
    dyn.set_temperature(100.0)
    rdf = dyn.attach(md.RadialDistribution([("H", "H")], r_max=3.0, bins=30, every=1))
    ts = dyn.attach(md.TimeSeries(("potential",), every=1, capacity=4))
    trj = dyn.attach(md.Trajectory(every=2, capacity=4))
    for cls in (md.MeanSquaredDisplacement, md.VelocityAutocorrelation):
        with pytest.raises(ValueError, match="beads are not trajectories"):
            dyn.attach(cls(lags=4, every=1))
    dyn.run(4)
    assert rdf.n_samples == 4 and ts.n_samples == 4 and trj.n_samples == 2 and tuple(trj.frames().shape) == (2, 8, 8, 3)
    # every bead is an entry of 8 atoms with all 56 ordered pairs within 3 A of a 1.15 A cube
    assert int(rdf.counts().cpu().numpy().astype(np.int64).sum()) == 4 * 8 * 56


def test_barostat_cells_volumes_and_the_refused_msd(dev):
    """27 Lennard-Jones atoms in a 7.5 A cell under the barostat: the cell of every frame, the volume and pressure series, g(r)
    normalized with the mean volume of the samples, and no MSD."""
    from torchani_amd import md
    from torchani_amd.potentials import LennardJones

    rs = np.random.RandomState(4)
    grid = np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing="ij"), -1).reshape(-1, 3) * 2.5
    x = torch.from_numpy((grid + rs.uniform(-0.2, 0.2, grid.shape)).astype(np.float32)).to(dev).unsqueeze(0)
    cell = (torch.eye(3) * 7.5).to(dev)
    sp = torch.ones((1, 27), dtype=torch.int64, device=dev)
    lj = LennardJones(("H",), eps=(0.002,), sigma=(2.4,), cutoff=5.0).to(dev)
    dyn = md.BatchedDynamics(lj, sp, x, cell, (True, True, True), masses=torch.full((1, 27), 12.011, device=dev),
                             temperature=100.0, pressure=1.0, seed=SEED)
    dyn.set_temperature(100.0)
    with pytest.raises(ValueError, match="barostat"):
        dyn.attach(md.MeanSquaredDisplacement(lags=4, every=1))
    ts = dyn.attach(md.TimeSeries(("volume", "pressure"), every=1, capacity=4))
    trj = dyn.attach(md.Trajectory(every=1, capacity=4, dtype=torch.float64))
    rdf = dyn.attach(md.RadialDistribution([("H", "H")], r_max=3.5, bins=35, every=1))
    vac = dyn.attach(md.VelocityAutocorrelation(lags=2, every=1))
    cells, volumes, pressures = [], [], []
    for _ in range(4):
        dyn.step()
        cells.append(dyn.cell64.clone().view(3, 3)), volumes.append(dyn.volumes()), pressures.append(dyn.pressures())
    assert torch.equal(trj.cells(), torch.stack(cells)) and len({float(v) for v in volumes}) == 4
    assert torch.equal(ts.values("volume"), torch.stack(volumes)) and torch.equal(ts.values("pressure"), torch.stack(pressures))
    mean_v = torch.stack(volumes).sum(dim=0) / 4.0   # (summed in sample order, as the observer does)
    edges = rdf.edges().to(dev)
    shell = 4.0 * math.pi / 3.0 * (edges[1:] ** 3 - edges[:-1] ** 3)
    counts = torch.from_numpy(rdf.counts().cpu().numpy().astype(np.int64)).to(dev).double()
    assert int(counts.sum()) > 0 and torch.allclose(rdf.g(), counts * mean_v / (4 * 27.0 * 27.0 * shell), rtol=1e-14, atol=0.0)
    assert vac.n_samples == 4 and vac.origins().tolist() == [4, 3]


def test_series_of_the_bias_and_its_cvs(dev):
    from torchani_amd import md

    lj, sp, x, mass = _lj_replicas(dev)
    window = torch.linspace(1.0, 1.4, 5, dtype=torch.float64)
    dyn = md.BatchedDynamics(lj, sp, x, dt=1.0, masses=mass, temperature=120.0, friction=0.05, seed=SEED,
                             bias=[md.Restraint(md.distance(0, 7), window, 0.05), md.Restraint(md.angle(0, 1, 2), 1.5, 0.01)])
    dyn.set_temperature(120.0)
    ts = dyn.attach(md.TimeSeries(("bias", "cv", "total"), every=3, capacity=2, on_full="wrap"))
    kept = []
    for _ in range(9):
        dyn.step()
        if dyn.steps_done % 3 == 0:
            kept.append((dyn.bias_energies.clone(), dyn.collective_variables(), dyn.total_energies()))
    assert ts.steps().tolist() == [6, 9] and tuple(ts.values("cv").shape) == (2, 5, 2)
    for q, name in enumerate(("bias", "cv", "total")):
        assert torch.equal(ts.values(name), torch.stack([k[q] for k in kept[-2:]])), name
    assert float(ts.values("bias").min()) > 0.0
