"""CPU checks of MBAR: the reference of tests/_mbar_ref.py (the fp64 statement of include/anihip.h that the GPU tests compare
the kernels with) against closed forms, the validation of ``md.ThermodynamicStates`` and ``md.MBAR``, what ``from_dynamics``
builds and refuses (on stub dynamics: the classes cannot be built without a device), and the C ABI: header and bindings agree,
and every entry point refuses what the host can see before it launches anything."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import _mbar_ref as mr
from torchani_amd import _lib, md
from torchani_amd.md_bias import build_bias_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference against closed forms --------------------------------------------------------------------------------------

def test_reference_recovers_harmonic_free_energies():
    """Six 1-D harmonic states, 2000 samples from each of the first five: f_k - f_0 = 1/2 ln(k_k / k_0) within 5 of the
    reference's own standard errors (seeds 0 .. 4 gave at most 2.7; seed 0 is the one kept: 1.6)."""
    restraint, n_k, cv, exact = mr.harmonic_case(0)
    u = mr.reduced_potentials(np.ones(6), restraint, [0], None, cv)
    f, iterations = mr.solve(u, n_k)
    assert iterations < 50
    plain = np.zeros(6)
    for _ in range(400):
        plain, delta = mr.iterate(u, n_k, plain)
    assert delta < 1e-10 and np.abs(plain - f).max() < 1e-8   # the plain iteration ends at the same point
    W = np.exp(mr.log_weights_all(u, n_k, f))
    assert np.abs(W.sum(axis=0) - 1.0).max() < 1e-10
    assert np.abs((W * n_k[None, :]).sum(axis=1) - 1.0).max() < 1e-10
    se = mr.uncertainties(W, n_k)
    z = (f[1:5] - exact[1:]) / se[0, 1:5]
    print(f"mbar reference, harmonic states: f = {np.array2string(f, precision=4)}, z = {np.array2string(z, precision=2)}")
    assert np.abs(z).max() <= 5.0
    assert np.all(se[0, 1:5] > 0.005) and np.all(se[0, 1:5] < 0.1) and np.abs(np.diag(se)).max() < 1e-7
    # the unsampled state: predicted from the others, with a larger error bar
    assert abs(f[5] - 0.5 * np.log(0.5 / 4.0)) <= 5.0 * se[0, 5] and se[0, 5] > se[0, 1]
    # weights of the unsampled state reproduce its mean and variance
    lw = mr.log_weights(u, n_k, f, u[5])
    mean = (np.exp(lw) * cv[:, 0]).sum()
    assert abs(np.exp(lw).sum() - 1.0) < 1e-12 and abs(mean - 1.0) < 0.15


def test_reference_histogram_edges_and_empty_bins():
    cv = np.array([[0.0], [0.25], [0.5], [1.0], [-0.1], [0.49999], [np.nan]])
    lw = np.log(np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]))
    lse, counts = mr.histogram(lw, cv, [0], [0.0], [1.0], [4])
    assert counts.tolist() == [1, 2, 1, 0]   # on an edge: the bin on the right; hi itself and below lo: out
    assert np.allclose(np.exp(lse[:3]), [1.0, 8.0, 3.0]) and np.isneginf(lse[3])
    F, _ = mr.pmf(lw, cv, [0], [0.0], [1.0], [4])
    assert F.min() == 0.0 and np.isposinf(F[3])


def test_reference_wraps_dihedral_columns():
    from _md_bias_ref import DIHEDRAL

    cv = np.array([[3.141], [-3.141]])
    rows = np.array([[[-3.14, 2.0, 0.0]]])
    u = mr.reduced_potentials([1.0], rows, [DIHEDRAL], None, cv)
    assert np.allclose(u[0], [0.5 * 2.0 * (2 * np.pi - 6.281) ** 2, 0.5 * 2.0 * 0.001 ** 2])


# ---- ThermodynamicStates and MBAR --------------------------------------------------------------------------------------------

def test_thermodynamic_states_layout_and_validation():
    s = md.ThermodynamicStates(300.0, [3.1, 3.25, 3.4], 0.05)
    assert s.n_states == 3 and s.n_columns == 1 and s.kinds.tolist() == [_lib.MD_CV_DISTANCE]
    assert torch.allclose(s.beta, torch.full((3,), 1.0 / (md.KB_HARTREE * 300.0), dtype=torch.float64))
    assert s.restraint[:, 0].tolist() == [[3.1, 0.05, 0.0], [3.25, 0.05, 0.0], [3.4, 0.05, 0.0]]
    s = md.ThermodynamicStates(torch.tensor([100.0, 200.0]), [[1.0, 0.5]], [0.1, 0.2], 0.01, kinds=("distance", "dihedral"))
    assert s.n_states == 2 and s.restraint.shape == (2, 2, 3) and s.kinds.tolist() == [0, 2]
    assert s.restraint[1].tolist() == [[1.0, 0.1, 0.01], [0.5, 0.2, 0.01]]
    ladder = md.ThermodynamicStates([15.0, 30.0, 60.0])
    assert ladder.n_states == 3 and ladder.n_columns == 0
    for bad, match in ((lambda: md.ThermodynamicStates(-1.0), "temperature must be > 0"),
                       (lambda: md.ThermodynamicStates([1.0, 2.0], [1.0, 2.0, 3.0], 1.0), "temperature holds 2 states"),
                       (lambda: md.ThermodynamicStates(300.0, [1.0]), "centers without k"),
                       (lambda: md.ThermodynamicStates(300.0, k=1.0), "pass centers too"),
                       (lambda: md.ThermodynamicStates(300.0, [1.0], -1.0), ">= 0"),
                       (lambda: md.ThermodynamicStates(300.0, [1.0], 1.0, -0.1), ">= 0"),
                       (lambda: md.ThermodynamicStates(300.0, [1.0], [1.0, 2.0, 3.0]), "k must broadcast"),
                       (lambda: md.ThermodynamicStates(300.0, [1.0], 1.0, kinds=["torsion"]), "unknown CV kind"),
                       (lambda: md.ThermodynamicStates(300.0, [1.0], 1.0, kinds=["distance", "angle"]), "kinds must name 1"),
                       (lambda: md.ThermodynamicStates(300.0, torch.zeros(2, 17), 1.0), "more than 16"),
                       (lambda: md.ThermodynamicStates(300.0, [float("nan")], 1.0), "finite")):
        with pytest.raises(ValueError, match=match):
            bad()


def test_mbar_validation_needs_no_device():
    s = md.ThermodynamicStates(300.0, [3.1, 3.25], 0.05)
    cv = torch.zeros((10, 1), dtype=torch.float64)
    for bad, match in ((lambda: md.MBAR("states", [5, 5], cv), "ThermodynamicStates"),
                       (lambda: md.MBAR(s, [5, 5, 0], cv), "one count per state"),
                       (lambda: md.MBAR(s, [5.5, 4.5], cv), "integers >= 0"),
                       (lambda: md.MBAR(s, [-5, 15], cv), "integers >= 0"),
                       (lambda: md.MBAR(s, [0, 0], cv), "no state was sampled"),
                       (lambda: md.MBAR(s, [5, 5]), "needs samples"),
                       (lambda: md.MBAR(s, [5, 5], energies=torch.zeros(10)), "cv .* is needed"),
                       (lambda: md.MBAR(s, [5, 5], torch.zeros(10, 2)), "cv must have shape"),
                       (lambda: md.MBAR(s, [5, 5], cv, torch.zeros(9)), "energies must have shape"),
                       (lambda: md.MBAR(s, [5, 4], cv), "n_k sums to 9"),
                       (lambda: md.MBAR(md.ThermodynamicStates([100.0, 200.0], [[1.0]], 1.0), [5, 5], cv), "need the potential energies"),
                       (lambda: md.MBAR(s, [5, 5], cv), "ROCm device"),
                       (lambda: md.MBAR.from_reduced_potentials(torch.zeros(10), [10]), "shape \\[K, N\\]"),
                       (lambda: md.MBAR.from_reduced_potentials(torch.zeros(2, 10), [5, 4]), "n_k sums to 9"),
                       (lambda: md.MBAR.from_reduced_potentials(torch.zeros(2, 10), [5, 5]), "ROCm device")):
        with pytest.raises(ValueError, match=match):
            bad()


# ---- from_dynamics on stub dynamics ------------------------------------------------------------------------------------------

class _Series:
    """What from_dynamics reads of a TimeSeries."""

    def __init__(self, dyn, n, capacity=None, **values):
        self._dyn, self.n_samples, self.capacity = dyn, n, n if capacity is None else capacity
        self.quantities, self._values = tuple(values), values

    def values(self, name):
        return self._values[name]


def _stub(cls, temperature, bias=None, ladders=None, **attrs):
    """An object of the class with the attributes from_dynamics reads (no device, no model)."""
    Cn = len(temperature)
    dyn = object.__new__(cls)
    species = torch.ones((Cn, 2), dtype=torch.int64)
    dyn.species, dyn.coordinates = species, torch.zeros((Cn, 2, 3))
    dyn.temperature, dyn.barostat, dyn.langevin = torch.as_tensor(temperature, dtype=torch.float32), False, True
    dyn._bias = None
    if bias is not None:
        tables = build_bias_tables(species, None, bias, temperature)
        dyn._bias = types.SimpleNamespace(tables=tables, n_lists=int(tables.members.numel()))
    if ladders is not None:
        lad = md.build_ladders(ladders, dyn.temperature)
        dyn.n_ladders, dyn._slot, dyn.rung_temperatures = lad.slot.shape[0], lad.slot, lad.rung_temperatures
    for name, value in attrs.items():
        setattr(dyn, name, value)
    return dyn


def _tables(dyn, series, discard=0, stride=1, ladder=0):
    return md.MBAR._tables_from_dynamics(dyn, series, discard, stride, ladder)


def test_from_dynamics_pools_identical_entries_into_states():
    centers = torch.tensor([3.1, 3.4, 3.1, 3.25, 3.4, 3.1], dtype=torch.float64)
    dyn = _stub(md.BatchedDynamics, [300.0] * 6, [md.Restraint(md.distance(0, 1), centers, 0.05)])
    cv = torch.arange(10 * 6, dtype=torch.float64).view(10, 6, 1)
    states, n_k, samples, energy, entries = _tables(dyn, _Series(dyn, 10, cv=cv), discard=2, stride=2)
    assert states.restraint[:, 0, 0].tolist() == [3.1, 3.4, 3.25]   # in the order of their first entry
    assert n_k.tolist() == [3 * 4, 2 * 4, 1 * 4] and energy is None and entries.tolist() == list(range(6))
    assert torch.equal(samples, cv[2::2].reshape(-1, 1))
    # two temperatures: the states split again and the potential is needed
    dyn = _stub(md.BatchedDynamics, [300.0, 300.0, 320.0, 300.0, 300.0, 320.0], [md.Restraint(md.distance(0, 1), centers, 0.05)])
    with pytest.raises(ValueError, match='must record "potential"'):
        _tables(dyn, _Series(dyn, 10, cv=cv))
    pot = torch.arange(60, dtype=torch.float64).view(10, 6)
    states, n_k, samples, energy, _ = _tables(dyn, _Series(dyn, 10, cv=cv, potential=pot))
    assert states.n_states == 4 and n_k.tolist() == [10, 20, 20, 10] and torch.equal(energy, pot.reshape(-1))
    assert states.temperature.tolist() == [300.0, 300.0, 320.0, 300.0] and states.restraint[:, 0, 0].tolist() == [3.1, 3.4, 3.1, 3.25]
    # no bias at all: states by temperature, no columns
    dyn = _stub(md.BatchedDynamics, [100.0, 200.0, 100.0])
    states, n_k, samples, energy, _ = _tables(dyn, _Series(dyn, 4, potential=torch.zeros(4, 3, dtype=torch.float64)))
    assert states.n_columns == 0 and n_k.tolist() == [8, 4] and samples is None and energy.shape == (12,)


def test_from_dynamics_counts_the_samples_of_every_rung():
    T = md.temperature_ladder(15.0, 60.0, 3).repeat(2)
    dyn = _stub(md.ReplicaExchangeDynamics, T.tolist(), [md.Restraint(md.distance(0, 1), 1.1, 0.01)],
                ladders=torch.arange(6).view(2, 3))
    rung = torch.tensor([[0, 1, 2, 0, 1, 2], [1, 0, 2, 0, 2, 1], [1, 2, 0, 2, 0, 1], [2, 1, 0, 2, 0, 1]], dtype=torch.float64)
    cv = torch.rand(4, 6, 1, dtype=torch.float64)
    pot = torch.rand(4, 6, dtype=torch.float64)
    series = _Series(dyn, 4, cv=cv, potential=pot, rung=rung)
    states, n_k, samples, energy, entries = _tables(dyn, series, ladder=1)
    assert entries.tolist() == [3, 4, 5] and states.n_states == 3 and n_k.tolist() == [4, 4, 4]
    assert torch.allclose(states.temperature, T[:3].float().double()) and torch.equal(energy, pot[:, 3:].reshape(-1))
    assert torch.equal(samples, cv[:, 3:].reshape(-1, 1)) and states.restraint[:, 0].tolist() == [[1.1, 0.01, 0.0]] * 3
    states, n_k, _, _, _ = _tables(dyn, series, discard=1, ladder=0)
    assert n_k.tolist() == [3, 3, 3]
    with pytest.raises(ValueError, match='must record "rung"'):
        _tables(dyn, _Series(dyn, 4, cv=cv, potential=pot))
    with pytest.raises(ValueError, match="ladder must be an integer in 0 .. 1"):
        _tables(dyn, series, ladder=2)


def test_from_dynamics_refusals():
    r = md.distance(0, 1)
    centers = torch.tensor([3.1, 3.4], dtype=torch.float64)
    cv = torch.zeros(4, 2, 1, dtype=torch.float64)
    plain = _stub(md.BatchedDynamics, [300.0, 300.0], [md.Restraint(r, centers, 0.05)])
    meta = _stub(md.BatchedDynamics, [300.0, 300.0], [md.Restraint(r, centers, 0.05), md.Metadynamics(r, 0.1, 1e-4, 10)])
    with pytest.raises(ValueError, match="Metadynamics: a time-dependent bias"):
        _tables(meta, _Series(meta, 4, cv=cv))
    with pytest.raises(ValueError, match="has wrapped"):
        _tables(plain, _Series(plain, 9, capacity=4, cv=cv))
    bad = cv.clone()
    bad[2, 1, 0] = float("nan")
    with pytest.raises(ValueError, match="NaN in a CV column"):
        _tables(plain, _Series(plain, 4, cv=bad))
    partial = _stub(md.BatchedDynamics, [300.0, 300.0], [md.Restraint(md.distance(torch.tensor([0, -1]), 1), centers, 0.05)])
    with pytest.raises(ValueError, match="entry 1 does not have CV column 0 \\(a NaN in the series\\)"):
        _tables(partial, _Series(partial, 4, cv=cv))
    beads = _stub(md.RingPolymerDynamics, [300.0, 300.0])
    with pytest.raises(ValueError, match="ring polymers"):
        _tables(beads, _Series(beads, 4, cv=cv))
    baro = _stub(md.BatchedDynamics, [300.0, 300.0], barostat=True)
    with pytest.raises(ValueError, match="barostat"):
        _tables(baro, _Series(baro, 4, cv=cv))
    lad = _stub(md.ReplicaExchangeDynamics, [100.0, 200.0], [md.Restraint(r, centers, 0.05)], ladders=torch.arange(2).view(1, 2))
    with pytest.raises(ValueError, match="ladder 0 hold different restraints"):
        _tables(lad, _Series(lad, 4, cv=cv, potential=cv[..., 0], rung=cv[..., 0]))
    with pytest.raises(ValueError, match='must record "cv"'):
        _tables(plain, _Series(plain, 4, potential=cv[..., 0]))
    with pytest.raises(ValueError, match="not attached to this dynamics"):
        _tables(plain, _Series(meta, 4, cv=cv))
    with pytest.raises(ValueError, match="leaves none"):
        _tables(plain, _Series(plain, 4, cv=cv), discard=4)
    nve = _stub(md.BatchedDynamics, [0.0, 0.0], langevin=False)
    with pytest.raises(ValueError, match="needs a thermostat"):
        _tables(nve, _Series(nve, 4, potential=cv[..., 0]))


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------

MBAR_SYMBOLS = ("anihip_mbar_workspace_bytes", "anihip_mbar_iterate", "anihip_mbar_log_weights",
                "anihip_mbar_histogram_workspace_bytes", "anihip_mbar_histogram")


def test_abi_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "anihip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(anihip_[a-z_0-9]+)\s*\(", code))
    L = _lib.lib()
    for name in MBAR_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and getattr(L, name) is not None
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    assert "mbar.hip" in _lib.SOURCES and re.search(r"#define\s+ANIHIP_ABI_VERSION\s+13\b", hdr) and _lib.ABI_VERSION == 13
    for name, value in (("MBAR_BAD_COUNTS", 1), ("MBAR_BAD_SAMPLES", 2), ("MBAR_BAD_STATES", 4), ("MBAR_MAX_BINS", 4096)):
        assert re.search(rf"#define\s+ANIHIP_{name}\s+{value}\b", hdr), name
        assert getattr(_lib, name) == value
    assert re.search(r"#define\s+ANIHIP_MBAR_TARGET_EXTERNAL\s+\(-1\)", hdr) and _lib.MBAR_TARGET_EXTERNAL == -1
    assert re.search(r"#define\s+ANIHIP_MBAR_TARGET_ALL\s+\(-2\)", hdr) and _lib.MBAR_TARGET_ALL == -2
    body = re.search(r"typedef struct \{([^}]*)\} anihip_mbar;", code).group(1)
    names = re.findall(r"\*?\b([a-z_A-Z0-9]+)\s*[,;]", body)
    assert names == [n for n, _ in _lib.Mbar._fields_]
    assert C.sizeof(_lib.Mbar) == 8 + 2 * 4 + 8 * C.sizeof(C.c_void_p) and _lib.Mbar.beta.offset == 16
    text = open(os.path.join(ROOT, "torchani_amd", "csrc", "mbar.hip")).read()
    assert '#include "md_cv.h"' in text and "cv_wrap(" in text and "atomicAdd(a.counts" in text
    assert not re.search(r"atomicAdd\([^)]*(double|float)", text) and "asm" not in text


def _problem(**change):
    fake = 4096   # never followed: every call below is refused first
    fields = dict(n_samples=100, n_states=3, n_cvs=2, beta=fake, n_k=fake, restraint=fake, cv_kind=fake, energy=fake, cv=fake,
                  u_kn=None, status=fake)
    fields.update(change)
    return _lib.Mbar(*(fields[n] for n, _ in _lib.Mbar._fields_))


BAD_PROBLEMS = (("n_states must be >= 1", dict(n_states=0)), ("n_cvs must be in 0 .. 16", dict(n_cvs=17)),
                ("n_cvs must be in 0 .. 16", dict(n_cvs=-1)), ("n_samples must be >= 1", dict(n_samples=-5)),
                ("n_samples must be >= 1", dict(n_samples=0)), ("n_k and status", dict(n_k=None)), ("n_k and status", dict(status=None)),
                ("needs beta", dict(beta=None)), ("needs restraint, cv_kind and cv", dict(cv=None)),
                ("needs restraint, cv_kind and cv", dict(restraint=None)), ("needs restraint, cv_kind and cv", dict(cv_kind=None)))


def test_error_returns_fire_before_any_launch():
    L = _lib.lib()
    err = lambda: L.anihip_last_error().decode()   # noqa: E731
    fake = 4096
    for match, change in BAD_PROBLEMS:
        p = _problem(**change)
        assert L.anihip_mbar_workspace_bytes(C.byref(p)) == 0 and match in err(), match
        assert L.anihip_mbar_iterate(None, C.byref(p), fake, 1, fake, fake, fake, 1 << 40) == 1 and match in err(), match
        assert L.anihip_mbar_log_weights(None, C.byref(p), fake, 0, None, None, None, 0, 10, fake, fake, 1 << 40) == 1
        assert match in err(), match
    assert L.anihip_mbar_workspace_bytes(None) == 0 and "null pointer" in err()
    good = _problem()
    need = L.anihip_mbar_workspace_bytes(C.byref(good))
    # ln N, two f buffers, the raw f, d, the raw weights, 1 chunk of 1536 samples x K pairs, 1 chunk of 1024 pairs, ln Z
    assert need == 8 * (4 * 3 + 2 * 100 + 1 * 3 * 2 + 1 * 2 + 1)
    dense = _problem(u_kn=fake, beta=None, restraint=None, cv_kind=None, cv=None, energy=None)
    assert L.anihip_mbar_workspace_bytes(C.byref(dense)) == need
    big = _problem(n_samples=1 << 20, n_states=256, n_cvs=1)
    assert L.anihip_mbar_workspace_bytes(C.byref(big)) == 8 * (4 * 256 + 2 * (1 << 20) + 512 * 256 * 2 + 1024 * 2 + 1)
    for args, match in (((None, 1, fake, fake, fake, need), "null pointer"), ((fake, 1, None, fake, fake, need), "null pointer"),
                        ((fake, 1, fake, None, fake, need), "null pointer"), ((fake, 0, fake, fake, fake, need), "n_iter must be >= 1"),
                        ((fake, 1, fake, fake, None, need), "workspace holds"), ((fake, 1, fake, fake, fake, need - 1), "workspace holds")):
        assert L.anihip_mbar_iterate(None, C.byref(good), *args) == 1 and match in err(), match
    for args, match in (((None, 0, None, None, None, 0, 10, fake, fake, need), "null pointer"),
                        ((fake, 0, None, None, None, 0, 10, None, fake, need), "null pointer"),
                        ((fake, 3, None, None, None, 0, 10, fake, fake, need), "target must be a state below 3"),
                        ((fake, -3, None, None, None, 0, 10, fake, fake, need), "target must be a state below 3"),
                        ((fake, 0, None, None, None, -1, 10, fake, fake, need), "does not lie in the 100 samples"),
                        ((fake, 0, None, None, None, 95, 10, fake, fake, need), "does not lie in the 100 samples"),
                        ((fake, 0, None, None, None, 0, 0, fake, fake, need), "does not lie in the 100 samples"),
                        ((fake, -1, None, fake, None, 0, 10, fake, fake, need), "needs target_beta and target_restraint"),
                        ((fake, -1, fake, None, None, 0, 10, fake, fake, need), "needs target_beta and target_restraint"),
                        ((fake, -2, None, None, None, 0, 10, fake, fake, need - 1), "workspace holds")):
        assert L.anihip_mbar_log_weights(None, C.byref(good), *args) == 1 and match in err(), match
    assert L.anihip_mbar_log_weights(None, C.byref(dense), fake, -1, None, None, None, 0, 10, fake, fake, need) == 1
    assert "needs target_u" in err()
    # the histogram
    i2, d2 = C.c_int32 * 2, C.c_double * 2
    assert L.anihip_mbar_histogram_workspace_bytes(0, 10) == 0 and L.anihip_mbar_histogram_workspace_bytes(10, 4097) == 0
    assert L.anihip_mbar_histogram_workspace_bytes(10, 0) == 0 and "n_bins in 1 .. 4096" in err()
    assert L.anihip_mbar_histogram_workspace_bytes(100, 48) == 2 * 48 * 8
    assert L.anihip_mbar_histogram_workspace_bytes(1 << 20, 48) == (512 + 1) * 48 * 8

    def hist(n=100, w=fake, cv=fake, stride=2, m=1, cols=(0, 0), lo=(0.0, 0.0), hi=(1.0, 1.0), bins=(48, 1), out=fake, counts=fake,
             ws=fake, nbytes=2 * 48 * 8):
        return L.anihip_mbar_histogram(None, n, w, cv, stride, m, i2(*cols), d2(*lo), d2(*hi), i2(*bins), out, counts, ws, nbytes)

    for kw, match in ((dict(w=None), "null pointer"), (dict(cv=None), "null pointer"), (dict(out=None), "null pointer"),
                      (dict(counts=None), "null pointer"), (dict(n=0), "n_samples must be in 1"), (dict(n=-1), "n_samples must be in 1"),
                      (dict(m=0), "one or two columns"), (dict(m=3), "one or two columns"), (dict(stride=0), "cv_stride must be >= 1"),
                      (dict(cols=(2, 0)), "column 2 is outside 0 .. 1"), (dict(cols=(-1, 0)), "column -1 is outside"),
                      (dict(bins=(0, 1)), "bins must be in 1 .. 4096"), (dict(bins=(4097, 1)), "bins must be in 1 .. 4096"),
                      (dict(lo=(1.0, 0.0)), "need lo < hi"), (dict(hi=(float("nan"), 1.0)), "need lo < hi"),
                      (dict(m=2, bins=(100, 100)), "10000 bins in all"), (dict(ws=None), "workspace holds"),
                      (dict(nbytes=2 * 48 * 8 - 1), "workspace holds")):
        assert hist(**kw) == 1 and match in err(), match
