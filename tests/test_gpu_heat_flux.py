"""The heat flux on the device against the fp64 reference of tests/_heat_flux_ref.py: anihip_aev_backward_flux entry by entry on
the tuned 8 x 4 and 4 x 8 grids and the general grid, anihip_md_heat_flux, ``grad.heat_flux`` on ANI-2x x 8, the flux as the
time derivative of sum_i r_i eps_i (independent of the formula: sign, units, kinetic term), and the two observers through
``BatchedDynamics``.

Gates, none of them new: per-centre rows 2e-5 x max(1, largest |entry| of the reference [N, 3]) (the VJP gate of
tests/test_gpu_parity.py: the rows are the gradients the VJP pushes, weighted by d and by |v| <= 1), per-entry sums 1e-4 x
max(1, largest entry) (the virial gate of tests/test_gpu_md.py), the correlation sums 1e-10 of sum |terms|.
tests/test_heat_flux_host.py holds the fp32 build of the oracle under a quarter of the first two on every case."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _heat_flux_ref as hf
import _second_order_ref as so
from _util import load_golden, oracle_networks, oracle_params, seeded_state
from test_gpu_parity import report

pytestmark = pytest.mark.gpu

GUARD = 16
SENTINEL = -12345.5
MASS_BY_INDEX = np.array([1.008, 12.011, 14.007, 15.999, 32.06, 18.998, 35.45])
CORR_GATE = 1e-10


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from torchani_amd import _lib

    _lib.lib()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def engine(grid):
    from torchani_amd.engine import AevEngine

    eng = AevEngine(hf.constants(grid))
    eng.host_table()
    assert eng.tuned == (grid != "general")
    return eng


def _reduce(dev, species, q, masses=None, energies=None, v=None):
    """anihip_md_heat_flux on [C, A] inputs (zeros where not given): J [C, 3, 3] fp64."""
    from torchani_amd import _lib
    from torchani_amd.engine import _stream

    Cn, A = species.shape
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)   # noqa: E731
    masses = z(Cn, A) if masses is None else masses
    energies = z(Cn, A, dt=torch.float64) if energies is None else energies
    v = z(Cn, A, 3) if v is None else v
    out = torch.full((Cn, 3, 3), float("nan"), dtype=torch.float64, device=dev)
    ws = torch.empty(_lib.lib().anihip_md_heat_flux_workspace_bytes(Cn, A), dtype=torch.uint8, device=dev)
    params = _lib.MdParams(Cn, A, 0, 0, 1.0, 0, 0)
    _lib.check(_lib.lib().anihip_md_heat_flux(_stream(), C.byref(params), masses.data_ptr(), energies.data_ptr(),
                                              species.data_ptr(), v.data_ptr(), q.contiguous().data_ptr(), out.data_ptr(),
                                              ws.data_ptr(), ws.numel()))
    return out


# ---- anihip_aev_backward_flux ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", hf.runs(), ids=hf.run_id)
def test_flux_rows_match_the_reference(dev, run):
    """Per-centre rows and their per-entry sums ("batch" rows, and "cell" rows for a single system), two runs bit-identical,
    rows of padding atoms and of atoms without neighbors zero, a sub-range of central atoms bit-equal to the same rows of the
    whole range with everything outside it untouched (guard words), and with constant vectors c: -sum q = -W^T c of
    anihip_aev_backward_virial on the same rows."""
    from torchani_amd import _lib
    from torchani_amd.engine import _ptr, _stream

    case, ref, eng = hf.case_by_name(run[0]), hf.reference(run), engine(run[1])
    Cn, A = case.species.shape
    n = Cn * A
    sp32 = torch.from_numpy(case.species.astype(np.int32)).to(dev).contiguous()
    x = torch.from_numpy(case.coords).to(dev).contiguous()
    cell = None if case.cell is None else torch.from_numpy(np.asarray(case.cell, dtype=np.float32)).to(dev)
    w, v = torch.from_numpy(ref.w).to(dev).contiguous(), torch.from_numpy(ref.v).to(dev).contiguous()
    rows = torch.from_numpy(ref.rows).to(dev)
    in_rows = torch.zeros(n, dtype=torch.bool, device=dev)
    in_rows[rows] = True
    real = case.species.reshape(-1) >= 0
    sums_ref = -(ref.q.reshape(Cn, A, 3) * real.reshape(Cn, A, 1)).sum(axis=1)
    rg, sg = hf.row_gate(ref), hf.sum_gate(sums_ref)
    for mode in (("batch", "cell") if Cn == 1 and A > 1 else ("batch",)):
        nbrs = eng.neighbors(sp32, x, cell, case.pbc, mode=mode, row_cap=256)
        torch.cuda.synchronize()
        nbrs.raise_on_overflow()
        q = eng.backward_flux(sp32, nbrs, w, v)
        q2 = eng.backward_flux(sp32, nbrs, w, v)
        torch.cuda.synchronize()
        assert q.shape == (n, 3) and torch.equal(q, q2), "two runs differ"
        got = q.cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all()
        assert np.all(got[~real] == 0.0), "rows of padding atoms must be zero"
        err = np.abs(got - ref.q)[ref.rows]
        k = int(np.argmax(err.max(axis=1)))
        J = _reduce(dev, sp32, torch.where(in_rows[:, None], q, torch.zeros_like(q)).view(Cn, A, 3))
        torch.cuda.synchronize()
        Jn = J.cpu().numpy()
        assert np.all(Jn[:, :2] == 0.0)
        serr = float(np.abs(Jn[:, 2] - sums_ref).max())
        report(f"flux  {hf.run_id(run):44s} {mode:5s} N={n:4d} rows {len(ref.rows):4d}  row err {err.max():.2e} = "
               f"{err.max() / rg:.3f} x gate {rg:.2e}   sum err {serr:.2e} = {serr / sg:.3f} x gate {sg:.2e}")
        assert err.max() < rg, f"{run} {mode}: row {int(ref.rows[k])} off by {err[k]} (reference {ref.q[ref.rows[k]]})"
        assert serr < sg, f"{run} {mode}: sums {Jn[:, 2]} against {sums_ref}"
        # constant vectors: the virial of the force backward on the same rows
        cv = torch.tensor([0.3, -0.8, 0.5], device=dev)
        qc = eng.backward_flux(sp32, nbrs, w, cv.expand(n, 3).contiguous())
        W = torch.empty((3, 3), dtype=torch.float64, device=dev)
        eng.backward(sp32, nbrs, w, virial=W)
        want = -(W.t() @ cv.double())
        have = _reduce(dev, sp32, qc.view(Cn, A, 3))[:, 2].sum(dim=0)
        torch.cuda.synchronize()
        assert float((have - want).abs().max()) < hf.sum_gate(want.cpu().numpy()), (run, mode, have, want)
        if case.sub is not None:
            lo, hi = case.sub
            part = eng.neighbors(sp32, x, cell, case.pbc, lo=lo, hi=hi, mode=mode, row_cap=256)
            buf = torch.full((3 * n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
            out = buf[GUARD:GUARD + 3 * n].view(n, 3)
            _lib.check(_lib.lib().anihip_aev_backward_flux(
                _stream(), C.byref(eng.params), _ptr(eng.table(dev)), n, lo, hi, _ptr(sp32), _ptr(part.meta), _ptr(part.ent),
                _ptr(w), None, 0, _ptr(v), out.data_ptr(), _ptr(part.status)))
            torch.cuda.synchronize()
            assert torch.equal(out[lo:hi], q[lo:hi]), (run, mode, "the rows of a sub-range differ from the whole range's")
            assert bool((out[:lo] == SENTINEL).all()) and bool((out[hi:] == SENTINEL).all()), "rows outside lo..hi were written"
            assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())
            via = eng.backward_flux(sp32, part, w[lo:hi].contiguous(), v, shard_rows=True)
            assert torch.equal(via[lo:hi], q[lo:hi]) and bool((via[:lo] == 0).all()) and bool((via[hi:] == 0).all())


def test_reduction_sums_what_the_reference_sums(dev):
    """anihip_md_heat_flux on padded entries of one chunk and of several (A = 700: three chunks and the second launch), against
    the fp64 sums; bit-identical run to run."""
    rs = np.random.RandomState(5)
    for Cn, A in ((3, 7), (2, 700), (1, 1)):
        sp = rs.randint(0, 4, (Cn, A)).astype(np.int32)
        sp[-1, A // 2 + 1:] = -1
        m = rs.uniform(1.0, 30.0, (Cn, A)).astype(np.float32)
        e = rs.uniform(-1.0, 1.0, (Cn, A))
        v = rs.uniform(-1.0, 1.0, (Cn, A, 3)).astype(np.float32)
        q = rs.uniform(-1.0, 1.0, (Cn, A, 3)).astype(np.float32)
        t = lambda a: torch.from_numpy(a).to(dev).contiguous()   # noqa: E731
        J = _reduce(dev, t(sp), t(q), t(m), t(e), t(v))
        J2 = _reduce(dev, t(sp), t(q), t(m), t(e), t(v))
        torch.cuda.synchronize()
        want = hf.flux_sums(sp, m, e, v, q)
        assert torch.equal(J, J2)
        assert np.abs(J.cpu().numpy() - want).max() < 1e-12 * max(1.0, np.abs(want).max()), (Cn, A)


# ---- grad.heat_flux on ANI-2x x 8 ------------------------------------------------------------------------------------------
def _model(dev, deterministic=False):
    """deterministic: forces summed in fixed point, so that two trajectories can be compared bit for bit."""
    from torchani_amd.models import ANI2x

    model = ANI2x(state_dict=seeded_state("ani2x", 8, 7), device=dev, periodic_table_index=False, row_capacity=256)
    model.deterministic_forces = deterministic
    return model


@functools.lru_cache(maxsize=None)
def model_case(name):
    """(species [C, A] int64, coords fp32, cell, pbc, velocities fp32 in Angstrom / fs, masses fp32)."""
    if name == "ch4":
        g = load_golden("ch4_ani1x")
        sp, x, cell, pbc = g["species"].astype(np.int64), g["coords"], None, None
    elif name == "cfg2_13_28":   # one 13- and one 28-atom molecule of config 2 in one batch
        g = load_golden("cfg2_xyz13_28_ani2x")
        count = (g["species"] >= 0).sum(axis=1)
        pick = [int(np.nonzero(count == 13)[0][0]), int(np.nonzero(count == 28)[0][0])]
        sp, x, cell, pbc = g["species"][pick].astype(np.int64), g["coords"][pick], None, None
    else:
        g = load_golden("water_pbc_ani2x")
        sp, x = g["species"].astype(np.int64), g["coords"]
        cell, pbc = g["cell"].astype(np.float32), tuple(bool(b) for b in g["pbc"])
    rs = np.random.RandomState(77)
    v = (rs.uniform(-1.0, 1.0, x.shape) * 0.02).astype(np.float32)
    v[sp < 0] = 0.0
    m = np.where(sp >= 0, MASS_BY_INDEX[np.clip(sp, 0, 6)], 1.0).astype(np.float32)
    return sp, x.astype(np.float32), cell, pbc, v, m


@functools.lru_cache(maxsize=None)
def model_reference(name):
    sp, x, cell, pbc, v, m = model_case(name)
    dims, flat, _ = oracle_networks("ani2x", 8, 7)
    return hf.model_flux(oracle_params("ani2x"), dims, flat, 8, sp, x, v, m, cell, pbc)


def _heat_flux(dev, model, name, x=None, **kw):
    from torchani_amd import grad

    sp, x0, cell, pbc, v, m = model_case(name)
    t = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    return grad.heat_flux(model, t(sp), t(x0 if x is None else x), t(v), masses=t(m),
                          cell=None if cell is None else t(cell), pbc=pbc, **kw)


@pytest.mark.parametrize("name", ["ch4", "cfg2_13_28", "water_pbc"])
def test_heat_flux_of_a_model_matches_the_reference(dev, name):
    model = _model(dev)
    J_ref, q_ref = model_reference(name)
    out = _heat_flux(dev, model, name)
    torch.cuda.synchronize()
    assert out.total.dtype == torch.float64 and out.total.shape == J_ref[:, 0].shape and out.atomic.shape == q_ref.shape
    assert torch.equal(out.total, out.kinetic + out.convective + out.virial)
    rg = hf.ROW_TOL * max(1.0, float(np.abs(q_ref).max()))
    qerr = float(np.abs(out.atomic.cpu().numpy() - q_ref).max())
    line = f"model {name:12s} rows {qerr:.2e} = {qerr / rg:.3f} x gate"
    assert qerr < rg
    for k, (field, part) in enumerate((("kinetic", out.kinetic), ("convective", out.convective), ("virial", out.virial))):
        gate = hf.sum_gate(J_ref[:, k])
        err = float(np.abs(part.cpu().numpy() - J_ref[:, k]).max())
        line += f"  {field} {err:.2e} = {err / gate:.3f} x gate (max {np.abs(J_ref[:, k]).max():.2e})"
        assert err < gate, (name, field, part, J_ref[:, k])
    tot = J_ref.sum(axis=1)
    assert float(np.abs(out.total.cpu().numpy() - tot).max()) < hf.sum_gate(tot)
    # The velocities of a thermal molecule are ~0.02 Angstrom / fs, so J is ~1e-3 and the floor of 1 in the gates above is most of
    # them: the same two relative gates without the floor, on the magnitudes this case has
    assert qerr < hf.ROW_TOL * float(np.abs(q_ref).max())
    for k, part in enumerate((out.kinetic, out.convective, out.virial)):
        assert float(np.abs(part.cpu().numpy() - J_ref[:, k]).max()) < hf.SUM_TOL * float(np.abs(J_ref[:, k]).max()), k
    report(line)
    again = _heat_flux(dev, model, name)
    assert all(torch.equal(a, b) for a, b in zip(out, again)), "two evaluations differ"


def test_heat_flux_with_self_energies(dev):
    """include_self_energies=True adds sum_i c_{s_i} v_i to the potential convective term and leaves the other terms alone."""
    model = _model(dev)
    sp, x, cell, pbc, v, m = model_case("cfg2_13_28")
    dims, flat, sae = oracle_networks("ani2x", 8, 7)
    J_ref, _ = hf.model_flux(oracle_params("ani2x"), dims, flat, 8, sp, x, v, m, cell, pbc, sae=sae)
    J_plain, _ = model_reference("cfg2_13_28")
    assert np.abs(J_ref[:, 1] - J_plain[:, 1]).max() > 10.0 * np.abs(J_plain[:, 1]).max(), "the self energies do not show"
    out, plain = _heat_flux(dev, model, "cfg2_13_28", include_self_energies=True), _heat_flux(dev, model, "cfg2_13_28")
    torch.cuda.synchronize()
    err = float(np.abs(out.convective.cpu().numpy() - J_ref[:, 1]).max())
    report(f"model cfg2_13_28 with self energies: convective {err:.2e} at max {np.abs(J_ref[:, 1]).max():.2e}")
    assert err < hf.SUM_TOL * float(np.abs(J_ref[:, 1]).max())
    assert torch.equal(out.kinetic, plain.kinetic) and torch.equal(out.virial, plain.virial)
    assert torch.equal(out.atomic, plain.atomic) and torch.equal(out.total, out.kinetic + out.convective + out.virial)


def test_heat_flux_raises_on_an_overflowing_row(dev):
    """A neighbor row over row_capacity is zeroed by the builder: grad.heat_flux raises as energies_and_forces does."""
    from torchani_amd.models import ANI2x

    small = ANI2x(state_dict=seeded_state("ani2x", 8, 7), device=dev, periodic_table_index=False, row_capacity=8)
    with pytest.raises(RuntimeError, match="neighbor row overflow"):
        _heat_flux(dev, small, "water_pbc")
    with pytest.raises(RuntimeError, match="neighbor row overflow"):   # (27 neighbors in an open molecule of 28)
        _heat_flux(dev, small, "cfg2_13_28")
    _heat_flux(dev, small, "ch4")   # (five atoms: no row can overflow, nothing is read)


def test_heat_flux_does_not_change_under_lattice_shifts(dev):
    """Every atom of the water box shifted by its own lattice vector.  No absolute position enters: the potential convective and
    the virial term agree within the relative gates without their floor of 1 (the terms are ~1e-3), the kinetic term bit for
    bit.  The engine wraps the shifted fp32 coordinates, whose last bits then differ; on coordinates snapped to a grid of 2^-10
    Angstrom in the 8 Angstrom cubic cell, shift and wrap are exact in fp32, the wrapped coordinates are the same bits, and so is
    every term."""
    model = _model(dev)
    sp, x, cell, pbc, v, m = model_case("water_pbc")
    J_ref, _ = model_reference("water_pbc")
    n_cells = np.random.RandomState(9).randint(-2, 3, x.shape).astype(np.float32)
    shifts = n_cells @ cell
    base, moved = _heat_flux(dev, model, "water_pbc"), _heat_flux(dev, model, "water_pbc", x=(x + shifts).astype(np.float32))
    torch.cuda.synchronize()
    for k, field in enumerate(("kinetic", "convective", "virial")):
        a, b = getattr(base, field), getattr(moved, field)
        assert float((a - b).abs().max()) < hf.sum_gate(J_ref[:, k]), field
        assert float((a - b).abs().max()) < hf.SUM_TOL * float(np.abs(J_ref[:, k]).max()), field
    assert float((base.atomic - moved.atomic).abs().max()) < hf.ROW_TOL * float(base.atomic.abs().max())
    assert torch.equal(base.kinetic, moved.kinetic)
    # exact in fp32: a cubic cell of 8 = 2^3 Angstrom, coordinates on a grid of 2^-10 Angstrom, shifts of whole cells
    assert np.array_equal(cell, np.diag([8.0, 8.0, 8.0]).astype(np.float32))
    xs = (np.round(x * 1024.0) / 1024.0).astype(np.float32)
    xm = (xs + shifts).astype(np.float32)
    wrap = lambda a: a - np.float32(8.0) * np.floor(a / np.float32(8.0))   # noqa: E731
    assert np.array_equal(xm - shifts, xs) and np.array_equal(wrap(xm), wrap(xs)) and not np.array_equal(xm, xs)
    base, moved = _heat_flux(dev, model, "water_pbc", x=xs), _heat_flux(dev, model, "water_pbc", x=xm)
    torch.cuda.synchronize()
    assert float(base.convective.abs().max()) > 1e-4 and float(base.virial.abs().max()) > 1e-5
    for field in ("kinetic", "convective", "virial", "total", "atomic"):
        assert torch.equal(getattr(base, field), getattr(moved, field)), f"{field} changed under an exact lattice shift"


def test_heat_flux_is_the_time_derivative_of_the_energy_moment(dev):
    """R = sum_i r_i eps_i along r(+-h) = r +- h v + 1/2 h^2 a, v(+-h) = v +- h a with the oracle's fp64 energies and forces:
    (R(+h) - R(-h)) / 2h, Richardson over h and 2h, is J.  Gate: 10 x the spread |D(h) - D(2h)| plus the model-level gate."""
    model = _model(dev)
    sp, x, _, _, v, m = model_case("ch4")
    dims, flat, _ = oracle_networks("ani2x", 8, 7)
    p, o = oracle_params("ani2x"), hf.oracle()
    x64, v64, m64 = x.astype(np.float64), v.astype(np.float64), m.astype(np.float64)
    f0 = o.energy_forces(p, sp, x64, dims, flat, 8)["forces"].astype(np.float64)
    acc = f0 * hf.ACC_UNIT / m64[..., None]

    def moment(h):
        r, u = x64 + h * v64 + 0.5 * h * h * acc, v64 + h * acc
        ae, _, _ = o.mlp(sp, o.aev(p, sp, r), dims, flat, n_members=8, want_grad=False)
        eps = 0.5 * m64 * (u * u).sum(axis=-1) / hf.ACC_UNIT + np.asarray(ae, dtype=np.float64).reshape(sp.shape)
        return (r * eps[..., None]).sum(axis=1)

    J_ref, _ = model_reference("ch4")
    gate = hf.sum_gate(J_ref.sum(axis=1))
    fd = so.fd_until(moment, lambda r: float(r.spread.max()) < 0.1 * gate)
    out = _heat_flux(dev, model, "ch4")
    torch.cuda.synchronize()
    err = np.abs(out.total.cpu().numpy() - fd.value)
    report(f"d/dt sum r eps: h = {fd.h:g} fs, spread {fd.spread.max():.2e}, J {np.abs(fd.value).max():.3e}, "
           f"device - FD {err.max():.2e}, reference - FD {np.abs(J_ref.sum(axis=1) - fd.value).max():.2e}")
    assert np.abs(fd.value).max() > 1e-5, "the case has no flux to speak of"
    assert np.all(err < 10.0 * fd.spread + gate), (out.total, fd.value, fd.spread)
    # (|J| is 3e-4 here, below the floor of that gate: the same relative gate without the floor, which a wrong factor in any
    # of the three terms -- the kinetic one is half of J -- cannot pass)
    assert np.all(err < 10.0 * fd.spread + hf.SUM_TOL * np.abs(fd.value).max()), (out.total, fd.value, fd.spread)


# ---- through the dynamics ----------------------------------------------------------------------------------------------------
def _water_dynamics(dev, model, cls=None, **kw):
    from torchani_amd import md

    sp, x, cell, pbc, _, m = model_case("water_pbc")
    t = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    dyn = (cls or md.BatchedDynamics)(model, t(sp), t(x), t(cell), pbc, dt=0.5, masses=t(m), seed=3, **kw)
    dyn.set_temperature(300.0)
    return dyn


def test_observers_record_the_flux_and_only_read(dev):
    """HeatFlux values bit-equal to grad.heat_flux at the same state; HeatFluxAutocorrelation over 2 M + 3 samples against the
    numpy sums of the recorded series; no host synchronization inside step(); the trajectory bit-identical with and without the
    observers, and to the step as it was before there were observers (``_advance`` alone)."""
    from torchani_amd import grad, md

    M = 3
    n = 2 * M + 3
    model = _model(dev, deterministic=True)
    watched = _water_dynamics(dev, model)
    flux = watched.attach(md.HeatFlux(every=1, capacity=n))
    corr = watched.attach(md.HeatFluxAutocorrelation(lags=M, every=1))
    for _ in range(3):   # (kernels loaded)
        watched.step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(n - 3):
            watched.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert flux.n_samples == corr.n_samples == n and flux.steps().tolist() == list(range(1, n + 1))
    now = grad.heat_flux(model, watched.species, watched.coordinates, watched.velocities, masses=watched.masses,
                         cell=watched.cell, pbc=watched.pbc)
    vals = flux.values()
    assert vals.shape == (n, 1, 3, 3) and vals.dtype == torch.float64
    assert torch.equal(vals[-1, :, 0], now.kinetic) and torch.equal(vals[-1, :, 1], now.convective)
    assert torch.equal(vals[-1, :, 2], now.virial) and torch.equal(flux.total()[-1], vals[-1].sum(dim=1))
    S, n_l, A = hf.hfacf_ref(flux.total().cpu().numpy(), M)
    assert corr.origins().tolist() == n_l.tolist()
    assert np.abs(corr._sums.cpu().numpy() - S).max() <= CORR_GATE * A.max()
    h = corr.hfacf().cpu().numpy()
    assert np.abs(h - S / n_l).max() <= CORR_GATE * A.max() and float(h[0, 0]) > 0.0
    kappa = corr.thermal_conductivity()
    assert kappa.shape == (1, M) and float(kappa[0, 0]) == 0.0 and bool(torch.isfinite(kappa).all())
    assert abs(float(corr.mean_temperatures()[0]) / 300.0 - 1.0) < 0.5
    # the defaults of an NVE run are the mean sampled temperature and the cell's volume
    assert torch.equal(kappa, corr.thermal_conductivity(temperature=corr.mean_temperatures(), volume=watched.volumes()))
    assert abs(float(watched.volumes()[0]) - 512.0) < 1e-9
    from torchani_amd.md import KB_HARTREE
    from torchani_amd.units import HARTREE_PER_ANGSTROM_FS_KELVIN_TO_WATT_PER_METER_KELVIN as TO_SI

    T = float(corr.mean_temperatures()[0])
    want = hf.trapezoid(h, 0.5) * TO_SI / (3.0 * 512.0 * KB_HARTREE * T * T)
    assert np.abs(kappa.cpu().numpy() - want).max() <= 1e-12 * np.abs(want).max()

    class Before(md.BatchedDynamics):
        step = md.BatchedDynamics._advance

    plain, before = _water_dynamics(dev, _model(dev, True)), _water_dynamics(dev, _model(dev, True), cls=Before)
    for d in (plain, before):
        for _ in range(n):
            d.step()
    torch.cuda.synchronize()
    for name in ("coordinates", "coordinates_lo", "velocities", "forces", "potential_energies"):
        assert torch.equal(getattr(plain, name), getattr(before, name)), f"without observers: {name}"
        assert torch.equal(getattr(watched, name), getattr(plain, name)), f"with observers: {name}"


def test_heat_flux_observer_on_open_molecules(dev):
    """HeatFlux on a batch of open molecules with padding (no cell); the correlation observer refuses it."""
    from torchani_amd import md

    sp, x, _, _, v, m = model_case("cfg2_13_28")
    t = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    model = _model(dev)
    dyn = md.BatchedDynamics(model, t(sp), t(x), dt=0.25, masses=t(m), seed=1)
    dyn.set_velocities(t(v))
    with pytest.raises(ValueError, match="needs a cell that is periodic"):
        dyn.attach(md.HeatFluxAutocorrelation(4, 1))
    flux = dyn.attach(md.HeatFlux(every=2, capacity=2, on_full="wrap"))
    dyn.run(6)
    assert flux.n_samples == 3 and flux.steps().tolist() == [4, 6]
    assert flux.values().shape == (2, 2, 3, 3) and bool(torch.isfinite(flux.values()).all())
    assert float(flux.total().abs().max()) > 0.0
