"""CPU checks of the MD observers (torchani_amd/md_observe.py): the fp64 reference of tests/_md_observe_ref.py (what the GPU
tests compare the kernels with) on answers known in closed form, the host-side results of the observers fed with the
reference's sums, the origin counts, every refusal at ``attach``, the ``on_full`` behaviors, and the declarations of the C ABI."""
import ctypes as C
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import _md_observe_ref as obr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeDynamics:
    """What an observer reads of a dynamics, on the host: CPU tensors and the accessors of ``BatchedDynamics``."""

    barostat = False
    _bias = None

    def __init__(self, species, dt=0.5, cell=None, pbc=None):
        self.species = torch.as_tensor(species)
        Cn, A = self.species.shape
        self.dt, self.cell, self.pbc, self.steps_done = dt, cell, pbc, 0
        self.coordinates = torch.zeros((Cn, A, 3), dtype=torch.float32)
        self.coordinates_lo = torch.zeros_like(self.coordinates)
        self.velocities = torch.zeros_like(self.coordinates)
        self.potential_energies = torch.zeros(Cn, dtype=torch.float64)
        self.model = types.SimpleNamespace(symbols=("H", "O"))

    def kinetic_energies(self):
        return self.potential_energies + 1.0

    def advance(self):
        self.steps_done += 1
        self.coordinates += 1.0
        self.coordinates_lo += 0.25
        self.velocities -= 1.0
        self.potential_energies += 2.0


# ---- the reference on known answers ---------------------------------------------------------------------------------------

def test_reference_rdf_counts_the_shells_of_a_simple_cubic_lattice():
    a, n = 2.0, 3
    grid = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(1, -1, 3) * a
    species = np.zeros((1, n ** 3), dtype=np.int64)
    cell, bins, r_max = np.eye(3) * (n * a), 25, 3.75   # (bins of 0.15 A: no shell sits on an edge)
    counts = obr.rdf_counts(species, grid + 0.3, [(0, 0)], r_max, bins, cell, (True, True, True))
    per_atom = counts[0] / n ** 3
    delta = r_max / bins
    shells = {int(math.floor(a * f / delta)): m for f, m in ((1.0, 6), (math.sqrt(2.0), 12), (math.sqrt(3.0), 8))}
    assert {int(b): int(v) for b, v in zip(np.nonzero(per_atom)[0], per_atom[np.nonzero(per_atom)[0]])} == shells
    # a cell of one lattice constant: an atom's own images are its six neighbors
    one = obr.rdf_counts(np.zeros((1, 1), dtype=np.int64), np.zeros((1, 1, 3)), [(0, 0)], 2.5, 5, np.eye(3) * a, (True,) * 3)
    assert one.tolist() == [[0, 0, 0, 0, 6]]
    # ordered pairs, padding, per entry and the boundary pairs
    sp = np.array([[0, 1, 1, -1], [1, 0, -1, -1]])
    x = np.array([[[0, 0, 0], [1.0, 0, 0], [0, 1.5, 0], [0.1, 0, 0]], [[0, 0, 0], [0, 0, 1.0], [0, 0, 0.5], [0, 0, 0.6]]])
    c, near = obr.rdf_counts(sp, x, [(0, 1), (1, 0), (1, 1)], 2.0, 4, per_entry=True, margin=1e-6)
    assert c[0].tolist() == [[0, 0, 1, 1], [0, 0, 1, 1], [0, 0, 0, 2]] and c[1].tolist() == [[0, 0, 1, 0], [0, 0, 1, 0], [0] * 4]
    assert near[0].tolist() == [[0, 0, 1, 1, 0], [0, 0, 1, 1, 0], [0] * 5] and int(near[1].sum()) == 2


def test_reference_correlations_of_straight_lines_and_cosines():
    rs = np.random.RandomState(0)
    Cn, A, M, dt = 2, 5, 8, 0.5
    species = rs.randint(0, 2, (Cn, A))
    species[1, 4] = -1
    v, x0 = rs.normal(size=(Cn, A, 3)), rs.normal(size=(Cn, A, 3))
    msd, vac = obr.Correlation("msd", species, 2, M), obr.Correlation("vacf", species, 2, M)
    for k in range(2 * M + 3):
        msd.add(x0 + v * (k * dt))
        vac.add(v)
    with np.errstate(invalid="ignore"):   # (a species without atoms in an entry: NaN on both sides)
        v2 = np.stack([((v ** 2).sum(-1) * (species == s)).sum(1) / (species == s).sum(1) for s in range(2)], 1)
    t = np.arange(M) * dt
    assert np.isfinite(v2).sum() >= 3
    assert np.allclose(msd.mean(), v2[:, :, None] * t ** 2, rtol=1e-12, atol=1e-14, equal_nan=True)
    assert np.allclose(vac.mean(), v2[:, :, None] * np.ones(M), rtol=1e-12, equal_nan=True)
    # a cosine velocity: averaged over the origins of whole periods, <v(t) v(t + tau)> = cos(omega tau) / 2
    M, period = 64, 16
    cos = obr.Correlation("vacf", np.zeros((1, 1), dtype=np.int64), 1, M)
    for k in range(M - 1 + 40 * period):
        cos.add(np.array([[[math.cos(2 * math.pi * k / period), 0.0, 0.0]]]))
    # (lag l has n - l origins: whole periods but for the last l, which leave an O(period / n) remainder)
    assert np.abs(cos.mean()[0, 0] - 0.5 * np.cos(2 * math.pi * np.arange(M) / period)).max() < 0.03


def test_origin_counts_before_and_after_the_ring_wraps():
    from torchani_amd import md_observe

    M = 5
    ref = obr.Correlation("vacf", np.zeros((1, 2), dtype=np.int64), 1, M)
    for k in range(2 * M + 3):
        assert md_observe.origins(k, M).tolist() == ref.origins.tolist()
        ref.add(np.ones((1, 2, 3)))
    assert md_observe.origins(3, M).tolist() == [3, 2, 1, 0, 0]          # fewer samples than lags
    assert md_observe.origins(M, M).tolist() == [5, 4, 3, 2, 1]          # the ring is full
    assert md_observe.origins(2 * M + 3, M).tolist() == [13, 12, 11, 10, 9]   # wrapped: every sample pairs with M - 1 before it


# ---- the host side of the observers ------------------------------------------------------------------------------------------

def test_correlation_results_from_the_reference_sums():
    from torchani_amd import md

    rs = np.random.RandomState(1)
    species = np.array([[8, 1, 1, -1, 8, 1], [1, 1, 8, 8, 8, -1]])
    dyn = FakeDynamics(species, dt=0.25)
    msd = md.MeanSquaredDisplacement(lags=6, every=4)
    msd._attach(dyn)
    assert msd.species_values.tolist() == [1, 8] and msd.atom_counts.tolist() == [[3, 2], [2, 3]]
    # the gather table: real atoms sorted by species, stable, -1 past them
    assert msd._gather.tolist() == [[1, 2, 5, 0, 4], [0, 1, 2, 3, 4]] and msd._gather_species.tolist() == [[0, 0, 0, 1, 1], [0, 0, 1, 1, 1]]
    index = np.where(species == 1, 0, np.where(species == 8, 1, -1))
    ref = obr.Correlation("msd", index, 2, 6)
    v, x0 = rs.normal(size=(2, 6, 3)), rs.normal(size=(2, 6, 3))
    for k in range(4):
        ref.add(x0 + v * k)
    msd._sums.copy_(torch.from_numpy(ref.sums))
    msd.n_samples = 4
    got = msd.msd().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ref.mean())) and np.isnan(got[..., 4:]).all() and not np.isnan(got[..., :4]).any()
    assert np.allclose(got[..., :4], ref.mean()[..., :4], rtol=1e-14)
    assert msd.times().tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0] and msd.origins().tolist() == [4, 3, 2, 1, 0, 0]
    total = ref.sums.sum(1)[:, :4] / (ref.origins[:4] * 5.0)
    assert np.allclose(msd.total().numpy()[:, :4], total, rtol=1e-14)
    # a straight line: MSD = |v|^2 t^2, whose least-squares slope over the lags 1, 2, 3 (t = 1, 2, 3) is 4 |v|^2
    v2 = np.stack([((v ** 2).sum(-1) * (index == s)).sum(1) / (index == s).sum(1) for s in range(2)], 1)
    assert np.allclose(msd.diffusion_coefficients(fit=(1, 4)).numpy(), 4.0 * v2 / 6.0, rtol=1e-12)
    with pytest.raises(ValueError, match="fit"):
        msd.diffusion_coefficients(fit=(3, 7))
    msd.reset()
    assert msd.n_samples == 0 and float(msd._sums.abs().max()) == 0.0


def test_spectrum_puts_a_cosine_in_its_bin():
    from torchani_amd import md, md_observe

    L, dt, j0 = 256, 2.0, 37
    omega = math.pi * j0 / (L * dt)
    t = torch.arange(L, dtype=torch.float64) * dt
    wn, dens = md_observe.cosine_spectrum(torch.cos(omega * t).view(1, 1, L), dt)
    assert tuple(dens.shape) == (1, 1, L) and int(dens[0, 0].argmax()) == j0
    assert abs(float(wn[j0]) - omega / (2 * math.pi * md_observe.LIGHT_SPEED_CM_PER_FS)) < 1e-9 * float(wn[j0])
    assert abs(float(wn[1]) - 1.0 / (2 * L * dt * 2.99792458e-5)) < 1e-9   # one bin is 1 / (2 c L dt)
    _, flat = md_observe.cosine_spectrum(torch.cos(omega * t), dt, window=None)
    assert int(flat.argmax()) == j0 and float(flat[j0]) == pytest.approx((L - 1) * dt, rel=1e-9)   # dt (1 + 2 (L / 2 - 1))
    with pytest.raises(ValueError, match="window"):
        md_observe.cosine_spectrum(torch.cos(omega * t), dt, window="blackman")
    # through the observer: the lags with an origin only
    dyn = FakeDynamics(np.zeros((1, 1), dtype=np.int64), dt=0.5)
    vac = md.VelocityAutocorrelation(lags=L + 8, every=4)
    vac._attach(dyn)
    vac.n_samples = L
    vac._sums[0, 0, :L] = torch.cos(omega * t) * md_observe.origins(L, L).double()
    wn2, dens2 = vac.spectrum()
    assert torch.equal(wn2, wn) and torch.allclose(dens2, dens, rtol=1e-12, atol=1e-12)


def test_radial_distribution_results_from_the_reference_counts():
    from torchani_amd import md

    rdf = md.RadialDistribution([("O", "O"), ("O", "H")], r_max=4.0, bins=8, every=2)
    # (filled by hand: ``_allocate`` builds an engine, which the GPU tests cover)
    rdf._dyn, rdf.n_samples, rdf._full_pbc = object(), 4, True
    rdf._counts = torch.zeros((2, 8), dtype=torch.int64)
    rdf._counts[0, 3], rdf._counts[1, 1], rdf._counts[1, 7] = 40, 16, 64
    rdf._n_a, rdf._n_b = torch.tensor([[2.0, 2.0], [3.0, 3.0]]), torch.tensor([[2.0, 4.0], [3.0, 6.0]])
    rdf._volume_sum = torch.tensor([4 * 1000.0], dtype=torch.float64)
    cn = rdf.coordination_numbers()
    assert cn[0].tolist() == [0, 0, 0, 2, 2, 2, 2, 2] and cn[1].tolist() == [0, 0.8, 0.8, 0.8, 0.8, 0.8, 0.8, 4.0]
    g = rdf.g()
    shell = 4 * math.pi / 3 * (2.0 ** 3 - 1.5 ** 3)
    assert float(g[0, 3]) == pytest.approx(40 * 1000.0 / (4 * (4 + 9) * shell), rel=1e-14) and float(g[0].sum()) == float(g[0, 3])
    # g integrates back to the coordination number: sum_b g rho_b shell = counts / (n_samples N_a) for one entry
    assert rdf.counts().dtype == torch.uint64 and rdf.edges().tolist() == [0.5 * k for k in range(9)]
    rdf._full_pbc = False
    with pytest.raises(ValueError, match="coordination_numbers"):
        rdf.g()


# ---- refusals and the rings ------------------------------------------------------------------------------------------------

def test_constructors_refuse():
    from torchani_amd import md

    for make, match in (
            (lambda: md.TimeSeries(("potential", "enthalpy"), 1, 4), "unknown quantity"),
            (lambda: md.TimeSeries((), 1, 4), "at least one"),
            (lambda: md.TimeSeries(("potential", "potential"), 1, 4), "each once"),
            (lambda: md.TimeSeries(("potential",), 0, 4), "every"),
            (lambda: md.TimeSeries(("potential",), 1, 0), "capacity"),
            (lambda: md.TimeSeries(("potential",), 1, 4, on_full="drop"), "on_full"),
            (lambda: md.Trajectory(1, 4, dtype=torch.float16), "dtype"),
            (lambda: md.RadialDistribution([], 5.0, 10, 1), "pairs"),
            (lambda: md.RadialDistribution([("O", "O")] * 2, 5.0, 10, 1), "twice"),
            (lambda: md.RadialDistribution([("O", str(k)) for k in range(9)], 5.0, 10, 1), "pairs"),
            (lambda: md.RadialDistribution([("O", "O")], 5.0, 1025, 1), "bins"),
            (lambda: md.RadialDistribution([("O", "O")], 5.0, 0, 1), "bins"),
            (lambda: md.RadialDistribution([("O", "O")], 0.0, 10, 1), "r_max"),
            (lambda: md.MeanSquaredDisplacement(lags=0, every=1), "lags"),
            (lambda: md.VelocityAutocorrelation(lags=4, every=1.5), "every")):
        with pytest.raises(ValueError, match=match):
            make()


def test_attach_refuses_on_the_host():
    from torchani_amd import md

    dyn = FakeDynamics(np.array([[1, 8, 8, -1]] * 3))
    for q, match in (("bias", "bias="), ("cv", "bias="), ("volume", "cell"), ("pressure", "pressure="), ("rung", "ReplicaExchange")):
        with pytest.raises(ValueError, match=match):
            md.TimeSeries((q,), 1, 4)._attach(dyn)
    with pytest.raises(ValueError, match="not an element of the model"):
        md.RadialDistribution([("O", "C")], 5.0, 10, 1)._attach(dyn)
    # the ring: 7 lags x 3 entries x 3 components x 3 atoms of fp64, one byte too many
    need = 7 * 3 * 3 * 3 * 8
    with pytest.raises(ValueError, match=rf"takes {need} bytes.*fewer lags"):
        md.MeanSquaredDisplacement(lags=7, every=1, max_bytes=need - 1)._attach(dyn)
    with pytest.raises(ValueError, match=rf"takes {need // 2} bytes.*fewer lags"):
        md.VelocityAutocorrelation(lags=7, every=1, max_bytes=need // 2 - 1)._attach(dyn)
    ok = md.MeanSquaredDisplacement(lags=7, every=1, max_bytes=need)
    ok._attach(dyn)
    with pytest.raises(ValueError, match="attached already"):
        ok._attach(dyn)
    dyn.barostat = True
    with pytest.raises(ValueError, match="barostat"):
        md.MeanSquaredDisplacement(lags=7, every=1)._attach(dyn)
    md.VelocityAutocorrelation(lags=7, every=1)._attach(dyn)   # (velocities are not rescaled into displacements)
    beads = object.__new__(md.RingPolymerDynamics)
    beads.barostat, beads.species = False, dyn.species
    for cls in (md.MeanSquaredDisplacement, md.VelocityAutocorrelation):
        with pytest.raises(ValueError, match="beads are not trajectories"):
            cls(lags=7, every=1)._attach(beads)
    with pytest.raises(ValueError, match="1 .. 8 species"):
        md.VelocityAutocorrelation(lags=2, every=1)._attach(FakeDynamics(np.arange(9).reshape(1, 9)))
    with pytest.raises(ValueError, match="takes an observer"):
        md.BatchedDynamics.attach(dyn, object())
    for obs in (md.Trajectory(1, 2), md.MeanSquaredDisplacement(2, 1), md.RadialDistribution([("O", "O")], 3.0, 4, 1)):
        with pytest.raises(ValueError, match="attach the observer"):
            (obs.frames if isinstance(obs, md.Trajectory) else obs.sums if hasattr(obs, "sums") else obs.counts)()


@pytest.mark.parametrize("on_full", ["raise", "wrap"])
def test_rings_keep_time_order_and_fill_as_asked(on_full):
    from torchani_amd import md

    dyn = FakeDynamics(np.array([[1, 8], [8, -1]]))
    ts = md.TimeSeries(("potential", "kinetic"), every=2, capacity=3, on_full=on_full)
    trj = md.Trajectory(every=2, capacity=3, velocities=True, dtype=torch.float64, on_full=on_full)
    for o in (ts, trj):
        o._attach(dyn)
    want = []
    for _ in range(6):   # samples at steps 2, 4, 6: the rings are exactly full
        dyn.advance()
        if dyn.steps_done % 2 == 0:
            ts._sample(dyn), trj._sample(dyn)
            want.append((dyn.steps_done, dyn.potential_energies.clone(), dyn.coordinates.double() + dyn.coordinates_lo.double(),
                         dyn.velocities.clone()))
    assert ts.steps().tolist() == trj.steps().tolist() == [2, 4, 6]
    assert torch.equal(ts.values("potential"), torch.stack([w[1] for w in want]))
    assert torch.equal(ts.values("kinetic"), torch.stack([w[1] + 1.0 for w in want]))
    assert trj.frames().dtype == torch.float64 and torch.equal(trj.frames(), torch.stack([w[2] for w in want]))
    assert torch.equal(trj.velocity_frames(), torch.stack([w[3] for w in want]))
    dyn.advance(), dyn.advance()
    if on_full == "raise":
        for o in (ts, trj):
            with pytest.raises(RuntimeError, match="is full: 3 samples"):
                o._sample(dyn)
            assert o.n_samples == 3 and o.steps().tolist() == [2, 4, 6]
    else:
        ts._sample(dyn), trj._sample(dyn)
        want.append((dyn.steps_done, dyn.potential_energies.clone(), dyn.coordinates.double() + dyn.coordinates_lo.double(), None))
        assert ts.n_samples == 4 and ts.steps().tolist() == trj.steps().tolist() == [4, 6, 8]
        assert torch.equal(ts.values("potential"), torch.stack([w[1] for w in want[1:]]))
        assert torch.equal(trj.frames(), torch.stack([w[2] for w in want[1:]]))
    with pytest.raises(ValueError, match="not recorded"):
        ts.values("total")
    with pytest.raises(ValueError, match="velocities=True"):
        plain = md.Trajectory(1, 2)
        plain._attach(dyn)
        plain.velocity_frames()
    with pytest.raises(ValueError, match="needs a cell"):
        plain.cells()
    ts.reset()
    assert ts.n_samples == 0 and ts.steps().numel() == 0 and ts.values("potential").shape[0] == 0


def test_step_is_split_and_observers_are_exported():
    from torchani_amd import md

    for name in ("TimeSeries", "Trajectory", "RadialDistribution", "MeanSquaredDisplacement", "VelocityAutocorrelation"):
        assert issubclass(getattr(md, name), md.Observer)
    # replica exchange attempts inside the part of the step that observers sample after
    assert "_advance" in md.ReplicaExchangeDynamics.__dict__ and "step" not in md.ReplicaExchangeDynamics.__dict__
    assert "_advance" in md.BatchedDynamics.__dict__ and "attach" in md.BatchedDynamics.__dict__


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------

def test_abi_is_declared_and_bound():
    from torchani_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "anihip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(anihip_[a-z_0-9]+)\s*\(", code))
    L = _lib.lib()
    names = ("anihip_md_rdf_accumulate", "anihip_md_corr_workspace_bytes", "anihip_md_corr_accumulate")
    for name in names:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and getattr(L, name) is not None
        args = re.search(rf"\b{name}\s*\(([^)]*)\)", code).group(1)
        assert len(args.split(",")) == len(getattr(L, name).argtypes), name
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    assert "md_observe.hip" in _lib.SOURCES
    assert re.search(r"#define\s+ANIHIP_ABI_VERSION\s+13\b", hdr) and _lib.ABI_VERSION == 13 and L.anihip_abi_version() == 13
    for name, value in (("MD_CORR_MSD", 0), ("MD_CORR_VACF", 1), ("MD_RDF_MAX_PAIRS", 8), ("MD_RDF_MAX_BINS", 1024)):
        assert re.search(rf"#define\s+ANIHIP_{name}\s+{value}\b", hdr), name
        assert getattr(_lib, name) == value
    assert L.anihip_md_corr_workspace_bytes.restype is C.c_size_t
    # the workspace: n_mol x chunks of 256 gather slots x species x lags doubles
    assert L.anihip_md_corr_workspace_bytes(3, 257, 5, 2) == 3 * 2 * 2 * 5 * 8
    assert L.anihip_md_corr_workspace_bytes(3, 0, 5, 2) == 0 and b"must be >= 1" in L.anihip_last_error()


def test_calls_refuse_what_the_host_can_see():
    from torchani_amd import _lib

    L = _lib.lib()
    params = _lib.MdParams(2, 6, 0, 0, 1.0, 0, 0)
    one = C.c_void_p(8)   # (never followed: the calls return first)
    table = (C.c_int8 * 64)(*([-1] * 64))
    rdf = lambda P=1, bins=4, r=3.0, t=table, sp=one: L.anihip_md_rdf_accumulate(  # noqa: E731
        None, C.byref(params), P, bins, r, 0, t, sp, one, one, 12, one)
    for call, message in ((lambda: rdf(P=9), b"n_pairs must be in 1 .. 8"), (lambda: rdf(bins=1025), b"bins in 1 .. 1024"),
                          (lambda: rdf(r=0.0), b"r_max must be > 0"), (lambda: rdf(sp=None), b"null pointer")):
        assert call() != 0 and message in L.anihip_last_error()
    table[9] = 1
    assert rdf() != 0 and b"pair_slot[9] = 1 is not a pair below 1" in L.anihip_last_error()
    corr = lambda kind=0, lags=4, S=2, G=6, k=0, ws=one, nb=2 * 1 * 2 * 4 * 8: L.anihip_md_corr_accumulate(  # noqa: E731
        None, C.byref(params), kind, lags, S, G, k, one, one, one, None, one, one, ws, nb)
    for call, message in ((lambda: corr(kind=2), b"unknown correlation kind 2"), (lambda: corr(lags=0), b"lags must be in"),
                          (lambda: corr(S=9), b"n_species in 1 .. 8"), (lambda: corr(G=7), b"max_atoms = 7 exceeds"),
                          (lambda: corr(k=-1), b"sample >= 0"), (lambda: corr(nb=127), b"workspace holds 127 bytes, 128 needed")):
        assert call() != 0 and message in L.anihip_last_error()
