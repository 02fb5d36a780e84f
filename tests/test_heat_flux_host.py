"""CPU checks of the heat flux: the fp64 reference of tests/_heat_flux_ref.py (what the GPU tests compare the kernels with) on
answers known in closed form, the correlation observer fed with synthetic series through ``_push`` on CPU tensors, the unit
factor, every refusal, the declarations of the C ABI, and what the fp32 build of the oracle makes of every kernel case (it has
to land under a quarter of the gate the kernels are held to; the ratios are printed and kept in
profiles/heat_flux_tests.txt)."""
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import _heat_flux_ref as hf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.environ.get("HEAT_FLUX_REPORT")


def report(line):
    print(line)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(line + "\n")


# ---- the reference on closed forms ---------------------------------------------------------------------------------------
def _radial_sum(p, wts, r):
    """sum_k w_k 0.25 exp(-EtaR (r - ShfR_k)^2) fc(r) and its derivative: the radial AEV terms of one neighbor, written out
    (with the oracle's constants, which are the fp32 values of the published ones)."""
    s, eta, rcr = np.array([p.ShfR[k] for k in range(p.nR)], dtype=np.float64), float(p.EtaR), float(p.Rcr)
    fc, dfc = 0.5 * math.cos(math.pi * r / rcr) + 0.5, -0.5 * math.pi / rcr * math.sin(math.pi * r / rcr)
    e = 0.25 * np.exp(-eta * (r - s) ** 2)
    return float((wts * e).sum() * fc), float((wts * e * (-2.0 * eta * (r - s))).sum() * fc + (wts * e).sum() * dfc)


def test_reference_two_body_closed_form():
    """E_1 = E_2 = phi(r) / 2 through a synthetic cotangent: -(q_1 + q_2) = -(phi' / 2) d_12 (u . (v_1 + v_2))."""
    c = hf.constants("2x")
    p = hf.oracle_params_of(c)
    # a Lennard-Jones-like phi: repulsive weights on the short shifts, attractive on the longer ones
    wts = np.where(np.arange(16) < 5, 3.0, -1.0) * np.linspace(1.0, 0.2, 16)
    x = np.array([[0.1, -0.2, 0.3], [1.3, 0.9, -0.4]])
    d = x[1] - x[0]
    r = float(np.linalg.norm(d))
    w = np.zeros((2, c.out_dim))
    w[:, 16 * 1:16 * 2] = wts          # both atoms of species 1: the radial block of a neighbor of species 1
    v = np.array([[0.3, -0.7, 0.2], [-0.5, 0.1, 0.9]])
    half_phi, half_dphi = _radial_sum(p, wts, r)
    aev = hf.oracle().aev(p, np.array([[1, 1]]), x[None])
    assert abs(float((w * aev.reshape(2, -1)).sum()) - 2.0 * half_phi) < 1e-12 * max(1.0, abs(half_phi))
    q = hf.flux_rows(p, [1, 1], x, w, v)
    want = -half_dphi * d * float((d / r) @ (v[0] + v[1]))
    assert abs(half_dphi) > 1e-3
    assert np.abs(-q.sum(axis=0) - want).max() < 1e-12 * max(1.0, np.abs(want).max()), (-q.sum(axis=0), want)


def test_reference_against_oracle_virial():
    """With a constant vector c, sum_i q_i = W^T c of the oracle's virial W = sum_ij g_ij (x) d_ij."""
    for name, grid in (("batch3", "2x"), ("images12_pbc/built", "2x"), ("radial_only", "general")):
        case, c = hf.case_by_name(name), hf.constants(grid)
        p = hf.oracle_params_of(c)
        w, _ = hf.inputs((name, grid))
        cv = np.array([0.3, -0.8, 0.5])
        v = np.broadcast_to(cv, (case.n_atoms, 3))
        q = hf.flux_rows_batch(p, case.species, case.coords.astype(np.float64), w, v, case.cell, case.pbc)
        _, _, W = hf.oracle().aev(p, case.species, case.coords.astype(np.float64), case.cell, case.pbc,
                                  grad_aev=w.astype(np.float64), want_virial=True)
        want = W.T @ cv
        assert np.abs(q.sum(axis=0) - want).max() < 1e-10 * max(1.0, np.abs(want).max()), (name, q.sum(axis=0), want)


def test_reference_supercell_identity():
    """A cell large enough for single images against its own 2 x 2 x 2 supercell with replicated vectors: the rows of the first
    replica are the rows of the cell, J(supercell) = 8 J(cell)."""
    c = hf.constants("2x")
    p = hf.oracle_params_of(c)
    sp, x = hf._cluster(11, 24, 10.6, 4)
    cell, pbc = np.diag([10.6, 10.9, 11.3]), (True, True, True)
    assert hf.replication(cell, pbc, c.Rcr) == (1, 1, 1)
    rs = np.random.RandomState(2)
    w, v = rs.uniform(-1, 1, (24, c.out_dim)), rs.uniform(-1, 1, (24, 3))
    q = hf.flux_rows(p, sp, x, w, v, cell, pbc)
    xs, cell_s, K = hf.supercell(x.astype(np.float64), cell, (2, 2, 2))
    qs = hf.flux_rows(p, np.tile(sp, K), xs, np.tile(w, (K, 1)), np.tile(v, (K, 1)), cell_s, pbc)
    scale = max(1.0, np.abs(q).max())
    assert np.abs(qs[:24] - q).max() < 1e-11 * scale
    assert np.abs(qs.sum(axis=0) - 8.0 * q.sum(axis=0)).max() < 1e-10 * scale
    # and the replication the reference does by itself, for a cell smaller than the cutoffs
    small = hf.case_by_name("images12_pbc/built")
    assert max(hf.replication(small.cell, small.pbc, c.Rcr)) >= 2
    assert np.abs(hf.reference(("images12_pbc/built", "2x")).q).max() > 1e-3


def test_flux_sums_and_kinetic_unit():
    from torchani_amd import md

    assert hf.ACC_UNIT == md.ACC_UNIT
    sp = np.array([[0, 3, -1]])
    m, e = np.array([[1.008, 15.999, 7.0]]), np.array([[0.5, -0.25, 9.0]])
    v = np.array([[[1.0, 0, 0], [0, 2.0, 0], [5.0, 5.0, 5.0]]])
    q = np.array([[[0.1, 0.2, 0.3], [0.0, -1.0, 0.5], [7.0, 7.0, 7.0]]])
    J = hf.flux_sums(sp, m, e, v, q)
    assert np.allclose(J[0, 0], [0.5 * 1.008 / md.ACC_UNIT, 0.5 * 15.999 * 4.0 * 2.0 / md.ACC_UNIT, 0.0], rtol=1e-15)
    assert np.allclose(J[0, 1], [0.5, -0.5, 0.0], rtol=1e-15)
    assert np.allclose(J[0, 2], [-0.1, 0.8, -0.8], rtol=1e-15)


# ---- the correlation observer on synthetic series --------------------------------------------------------------------------
def _observer(lags, every, n_entries, dt):
    from torchani_amd import md

    ob = md.HeatFluxAutocorrelation(lags, every)
    ob._init_buffers(n_entries, torch.device("cpu"), dt)
    return ob


def test_hfacf_exponential_sequence_exact_sums_and_origins_across_the_wrap():
    """J_k = rho^k e: S_l = rho^l (1 - rho^(2 (n - l))) / (1 - rho^2) |e|^2, over 2 M + 3 samples (the ring wraps twice)."""
    M, rho = 7, 0.9
    n = 2 * M + 3
    e = np.array([[1.0, -2.0, 0.5], [0.3, 0.3, -0.1]])
    ob = _observer(M, 2, 2, 0.25)
    J = np.stack([rho ** k * e for k in range(n)])
    for k in range(n):
        ob._push(torch.from_numpy(J[k]))
    l = np.arange(M)   # noqa: E741
    exact = rho ** l * (1.0 - rho ** (2 * (n - l))) / (1.0 - rho * rho) * (e * e).sum(axis=1)[:, None]
    assert np.abs(ob._sums.numpy() - exact).max() < 1e-13 * np.abs(exact).max()
    S, n_l, A = hf.hfacf_ref(J, M)
    assert np.abs(ob._sums.numpy() - S).max() <= 1e-10 * A.max()
    assert ob.origins().tolist() == n_l.tolist() == [n - k for k in range(M)]
    assert np.abs(ob.hfacf().numpy() - exact / n_l).max() < 1e-13 * np.abs(exact).max()
    assert np.allclose(ob.times().numpy(), l * 2 * 0.25, rtol=0, atol=0)


def test_conductivity_of_a_cosine_is_the_sine():
    from torchani_amd import md, units

    M, dt, every, omega = 40, 0.5, 2, 0.01
    step = dt * every
    ob = _observer(M, every, 1, dt)
    for k in range(3 * M):
        ob._push(torch.tensor([[math.cos(omega * k * step), math.sin(omega * k * step), 0.0]], dtype=torch.float64))
    t = np.arange(M) * step
    assert np.abs(ob.hfacf().numpy()[0] - np.cos(omega * t)).max() < 1e-13
    T, V = 300.0, 1234.5
    kappa = ob.thermal_conductivity(temperature=T, volume=V).numpy()[0]
    pref = units.HARTREE_PER_ANGSTROM_FS_KELVIN_TO_WATT_PER_METER_KELVIN / (3.0 * V * md.KB_HARTREE * T * T)
    trap = np.sin(omega * t) * 0.5 * step / math.tan(0.5 * omega * step)     # the trapezoid rule on a cosine, exactly
    assert np.abs(kappa - pref * trap).max() < 1e-12 * pref * np.abs(trap).max()
    assert np.abs(kappa - pref * hf.trapezoid(np.cos(omega * t), step)).max() < 1e-12 * pref * np.abs(trap).max()
    # against the integral itself: the trapezoid rule is off by (omega step)^2 / 12 of it
    sine = np.sin(omega * t) / omega
    assert np.abs(kappa / pref - sine).max() < 1.01 * (omega * step) ** 2 / 12.0 * np.abs(sine).max()


def test_hfacf_is_nan_without_origins():
    ob = _observer(5, 1, 2, 0.5)
    assert torch.isnan(ob.hfacf()).all() and ob.origins().tolist() == [0] * 5
    ob._push(torch.ones((2, 3), dtype=torch.float64))
    ob._push(torch.ones((2, 3), dtype=torch.float64))
    h = ob.hfacf()
    assert torch.equal(h[:, :2], torch.full((2, 2), 3.0, dtype=torch.float64)) and torch.isnan(h[:, 2:]).all()
    assert torch.isnan(ob.thermal_conductivity(temperature=300.0, volume=1000.0)[:, 2:]).all()
    ob.reset()
    assert ob.n_samples == 0 and torch.isnan(ob.hfacf()).all()
    with pytest.raises(ValueError, match="attach the observer"):
        __import__("torchani_amd").md.HeatFluxAutocorrelation(4, 1).hfacf()


def test_conductivity_defaults_of_a_thermostatted_and_of_an_nve_run():
    """Without arguments T is the thermostat's target (Langevin) or the mean sampled temperature (NVE), V the cell's volume:
    the same numbers as the call that is given them."""
    rs = np.random.RandomState(4)
    target, mean, vol = torch.tensor([250.0, 350.0]), torch.tensor([290.0, 310.0], dtype=torch.float64), torch.tensor([777.0])
    for langevin in (True, False):
        ob = _observer(6, 1, 2, 0.5)
        ob._dyn = types.SimpleNamespace(langevin=langevin, temperature=target, volumes=lambda: vol.double())
        ob._temp_sum = torch.zeros(2, dtype=torch.float64)
        for k in range(9):
            ob._temp_sum += mean
            ob._push(torch.from_numpy(rs.uniform(-1.0, 1.0, (2, 3))))
        assert torch.equal(ob.mean_temperatures(), mean)
        T = target.double() if langevin else mean
        kappa = ob.thermal_conductivity()
        assert torch.equal(kappa, ob.thermal_conductivity(temperature=T, volume=777.0))
        assert bool(torch.isfinite(kappa).all()) and float(kappa[:, 1:].abs().min()) > 0.0
        # per entry: 1 / T^2
        one = ob.thermal_conductivity(temperature=300.0, volume=777.0)
        assert torch.allclose(kappa * (T * T).view(2, 1), one * 300.0 ** 2, rtol=1e-14, atol=0.0)


def test_unit_factor_against_codata():
    from torchani_amd import md, units

    hartree_j, amu_kg, kb_j = 4.3597447222071e-18, 1.66053906660e-27, 1.380649e-23   # CODATA 2018
    f = units.HARTREE_PER_ANGSTROM_FS_KELVIN_TO_WATT_PER_METER_KELVIN
    assert abs(f - hartree_j / (1e-10 * 1e-15)) <= 1e-15 * f and abs(f - 4.3597447222071e7) < 1e-6
    # the constants the integral is built from are md.py's: k_B in Hartree / K, and the kinetic energy's amu A^2 / fs^2 -> Ha
    assert abs(md.KB_HARTREE * hartree_j / kb_j - 1.0) < 1e-9
    assert abs(md.ACC_UNIT - hartree_j / (amu_kg * 1e10)) < 1e-15


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _fake_dyn(**kw):
    model = types.SimpleNamespace(heat_flux_terms=None, _refuse_heat_flux=lambda: None)
    base = dict(_clusters=None, _bias=None, barostat=False, cell=torch.eye(3) * 12.0, pbc=(True, True, True), model=model,
                _model_eval=types.SimpleNamespace(standalone=False))
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_every_refusal_at_attach():
    from torchani_amd import md
    from torchani_amd.models import ANI

    for make in (lambda: md.HeatFlux(1, 4), lambda: md.HeatFluxAutocorrelation(4, 1)):
        name = type(make()).__name__
        rp = object.__new__(md.RingPolymerDynamics)
        with pytest.raises(ValueError, match=f"{name} is not available on RingPolymerDynamics"):
            make()._attach(rp)
        with pytest.raises(ValueError, match=f"{name} is not available with constraints: the constraint forces carry a heat flux"):
            make()._attach(_fake_dyn(_clusters=object()))
        with pytest.raises(ValueError, match=f"{name} is not available with a bias: the bias forces carry a heat flux"):
            make()._attach(_fake_dyn(_bias=object()))
        with pytest.raises(ValueError, match="is a pair potential, and the pair halves have no flux kernel"):
            make()._attach(_fake_dyn(_model_eval=types.SimpleNamespace(standalone=True)))
        pairs = types.SimpleNamespace(potentials={"nnp": types.SimpleNamespace(_enabled=True),
                                                  "repulsion_xtb": types.SimpleNamespace(_enabled=True)})
        pairs.heat_flux_terms, pairs._refuse_heat_flux = None, lambda: ANI._refuse_heat_flux(pairs)
        with pytest.raises(ValueError, match=rf"{name}: heat flux: the model has pair potentials \(repulsion_xtb\), whose pair "
                                             "halves have no flux kernel yet"):
            make()._attach(_fake_dyn(model=pairs))
    with pytest.raises(ValueError, match="HeatFluxAutocorrelation is not available with a barostat"):
        md.HeatFluxAutocorrelation(4, 1)._attach(_fake_dyn(barostat=True))
    for kw in (dict(cell=None, pbc=None), dict(pbc=(True, True, False))):
        with pytest.raises(ValueError, match="HeatFluxAutocorrelation needs a cell that is periodic in all three directions"):
            md.HeatFluxAutocorrelation(4, 1)._attach(_fake_dyn(**kw))
    # HeatFlux itself takes an open molecule (the allocation is all that is left to do: it needs species and coordinates)
    ob = md.HeatFlux(1, 4)
    ob._check(_fake_dyn(cell=None, pbc=None))
    with pytest.raises(ValueError, match="must be an integer >= 1"):
        md.HeatFluxAutocorrelation(0, 1)
    with pytest.raises(ValueError, match='on_full must be "raise" or "wrap"'):
        md.HeatFlux(1, 4, on_full="drop")


def test_refusals_of_the_model(monkeypatch):
    from torchani_amd import grad
    from torchani_amd.models import ANI

    plain = types.SimpleNamespace(potentials={"nnp": types.SimpleNamespace(_enabled=True),
                                              "dispersion_d3": types.SimpleNamespace(_enabled=False)})
    ANI._refuse_heat_flux(plain)   # (a disabled pair potential does not count)
    plain.potentials["dispersion_d3"]._enabled = True
    with pytest.raises(NotImplementedError, match=r"pair potentials \(dispersion_d3\), whose pair halves have no flux kernel yet"):
        ANI._refuse_heat_flux(plain)
    plain.potentials["dispersion_d3"]._enabled = False
    ANI._refuse_heat_flux(plain)   # (no process group: one rank)
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 1)
    ANI._refuse_heat_flux(plain)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="more than one rank is not supported"):
        ANI._refuse_heat_flux(plain, group=object())
    with pytest.raises(NotImplementedError, match="more than one rank is not supported"):   # the default group of the program
        ANI._refuse_heat_flux(plain)
    real = types.SimpleNamespace(heat_flux_terms=None, _refuse_heat_flux=lambda: ANI._refuse_heat_flux(plain))
    with pytest.raises(NotImplementedError, match="more than one rank is not supported"):   # what grad.heat_flux reaches
        grad.heat_flux(real, torch.zeros((1, 2), dtype=torch.long), torch.zeros((1, 2, 3)), torch.zeros((1, 2, 3)))
    from torchani_amd import md

    with pytest.raises(ValueError, match="HeatFlux: heat flux: more than one rank is not supported"):   # and the observers
        md.HeatFlux(1, 4)._attach(_fake_dyn(model=real))
    monkeypatch.undo()
    with pytest.raises(NotImplementedError, match="has no flux kernel"):
        grad.heat_flux(types.SimpleNamespace(), torch.zeros((1, 2), dtype=torch.long), torch.zeros((1, 2, 3)), torch.zeros((1, 2, 3)))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_abi_declarations():
    from torchani_amd import _lib

    with open(os.path.join(ROOT, "include", "anihip.h")) as f:
        header = f.read()
    L = _lib.lib()
    for name in ("anihip_aev_backward_flux", "anihip_md_heat_flux_workspace_bytes", "anihip_md_heat_flux"):
        assert re.search(r"\b" + name + r"\(", header) and name in _lib.EXPORTED_SYMBOLS and getattr(L, name) is not None
    assert L.anihip_abi_version() == _lib.ABI_VERSION
    # null pointers and bad ranges come back nonzero before any launch (no device is touched: this runs without one)
    from torchani_amd.engine import AevEngine

    eng = AevEngine(hf.constants("2x"))
    tab = eng.host_table()
    import ctypes as C

    buf = (C.c_float * 64)()
    args = lambda **kw: [kw.get(k, d) for k, d in (("stream", None), ("p", C.byref(eng.params)), ("table", tab.ctypes.data),   # noqa: E731
                                                   ("n", 4), ("lo", 0), ("hi", 4), ("species", C.addressof(buf)),
                                                   ("meta", C.addressof(buf)), ("ent", C.addressof(buf)),
                                                   ("grad_aev", C.addressof(buf)), ("slab_mask", None), ("flags", 0),
                                                   ("vectors", C.addressof(buf)), ("flux_atoms", C.addressof(buf)),
                                                   ("status", None))]
    for bad in (dict(vectors=None), dict(flux_atoms=None), dict(grad_aev=None), dict(species=None), dict(lo=3, hi=2),
                dict(hi=5), dict(lo=-1)):
        assert L.anihip_aev_backward_flux(*args(**bad)) != 0, bad
        assert _lib.last_error() if hasattr(_lib, "last_error") else True
    assert L.anihip_md_heat_flux_workspace_bytes(0, 5) == 0 and L.anihip_md_heat_flux_workspace_bytes(3, 700) == 3 * 3 * 9 * 8
    assert L.anihip_md_heat_flux(None, None, None, None, None, None, None, None, None, 0) != 0


# ---- what fp32 makes of the kernel cases ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", hf.runs(), ids=hf.run_id)
def test_fp32_oracle_lands_under_a_quarter_of_the_gates(run):
    """The oracle's own sums in fp32 against fp64, per-centre rows and their sum, relative to the gates of the GPU test."""
    ref, low = hf.reference(run), hf.reference(run, "f32")
    row_err = float(np.abs(low.q - ref.q).max())
    sum_err = float(np.abs(low.q.sum(axis=0) - ref.q.sum(axis=0)).max())
    rg, sg = hf.row_gate(ref), hf.sum_gate(ref.q.sum(axis=0))
    report(f"fp32 oracle {hf.run_id(run):44s} rows {len(ref.rows):4d} max|q| {np.abs(ref.q).max():9.3f}  row err {row_err:.2e} = "
           f"{row_err / rg:.3f} x gate {rg:.2e}   sum err {sum_err:.2e} = {sum_err / sg:.3f} x gate {sg:.2e}")
    assert row_err < 0.25 * rg and sum_err < 0.25 * sg
