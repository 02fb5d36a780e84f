"""The stochastic-cell-rescaling barostat of the device integrator (anihip_md_barostat in csrc/md.hip, ``pressure=`` of
torchani_amd.md.BatchedDynamics) on the MI355X against the fp64 restatement of tests/_md_barostat_ref.py: the move with the
kinetic energy and the virial given, the NPT ideal gas, whole NPT steps on ANI-2x in lock-step with the reference,
``pressures()`` against a finite difference of the energy in the volume, and the behaviour of the Python layer.

Shapes as in test_gpu_md_device.py: C = 3, A = 70 (more than a wave, no multiple of 64, padding in the middle molecule, fixed
atoms, permuted replica ids) and C = 2, A = 300 (more than one 256-atom chunk per molecule)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _md_barostat_ref as bref
import _md_ref as ref
from _util import load_golden
from test_gpu_md_device import MASS_BY_INDEX, SEED, STEP0, _ani_case, _assert_close, _noise
from test_md_barostat_host import IDEAL_GAS_SEED

pytestmark = pytest.mark.gpu

BAR = bref.BAR_PER_HARTREE_ANGSTROM3
# The largest |cell64 - cell_ref| / max |cell_ref| of the three lock-step NPT steps, as measured (profiles/md_barostat_tests.txt):
# the device draws xi_b in fp32 and the reference in fp64.  The gate is ten times that.
CELL_DIFF_MEASURED = {"water_pbc_ani2x": 2.45e-10, "triclinic_pbc_ani2x": 3.64e-10}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from torchani_amd import _lib

    _lib.lib()
    return torch.device("cuda:0")


def _stream():
    from torchani_amd.engine import _stream as s

    return s()


class Kernels:
    """The C ABI on a state made from numpy arrays: x (fp64, split into the two-float pair), v [C, A, 3], active [C, A] (0, 1 or
    2), mass [C, A], cell [C, 3, 3]; zero forces for drift and kick."""

    def __init__(self, dev, x, v, active, mass, cell, dt, kT, friction, beta_T, tau_p, p0, rid=None, seed=SEED, langevin=True):
        from torchani_amd import _lib

        self.lib, self._lib = _lib.lib(), _lib
        Cn, A = active.shape
        up = lambda a, dt_: torch.from_numpy(np.ascontiguousarray(a, dtype=dt_)).to(dev)   # noqa: E731
        hi = np.asarray(x, dtype=np.float64).astype(np.float32)
        self.x, self.lo = up(hi, np.float32), up(np.asarray(x, dtype=np.float64) - hi.astype(np.float64), np.float32)
        self.v, self.active, self.mass = up(v, np.float32), up(active, np.uint8), up(mass, np.float32)
        self.inv_mass = (ref.ACC_UNIT / self.mass.double()).float()
        self.kT, self.friction = up(kT, np.float32), up(friction, np.float32)
        self.rid = None if rid is None else torch.as_tensor(rid, dtype=torch.int64).to(dev)
        self.P = _lib.MdParams(Cn, A, _lib.MD_LANGEVIN if langevin else 0, 0, dt, seed, 0)
        self.ws = torch.empty(self.lib.anihip_md_workspace_bytes(Cn, A), dtype=torch.uint8, device=dev)
        self.kinetic = torch.zeros(Cn, dtype=torch.float64, device=dev)
        self.virial = torch.zeros((Cn, 9), dtype=torch.float64, device=dev)
        self.cell64 = up(np.asarray(cell).reshape(Cn, 9), np.float64)
        self.cell32 = torch.zeros((Cn, 9), dtype=torch.float32, device=dev)
        self.scale = torch.zeros(Cn, dtype=torch.float64, device=dev)
        self.p0 = up(p0, np.float64)
        self.beta_T, self.tau_p = beta_T, tau_p
        self.zero = torch.zeros((Cn, A, 3), dtype=torch.float32, device=dev)

    def _rid(self):
        return None if self.rid is None else self.rid.data_ptr()

    def drift(self, step):
        self.P.step = step
        self._lib.check(self.lib.anihip_md_drift(
            _stream(), C.byref(self.P), self.active.data_ptr(), self.inv_mass.data_ptr(), self.kT.data_ptr(),
            self.friction.data_ptr(), self._rid(), self.x.data_ptr(), self.lo.data_ptr(), self.v.data_ptr(), self.zero.data_ptr()))

    def barostat_rc(self, step, beta_T=None, tau_p=None, **null):
        """The status of the call; ``null``: argument names to pass as NULL."""
        self.P.step = step
        ptr = lambda name, t: None if name in null else t.data_ptr()   # noqa: E731
        return self.lib.anihip_md_barostat(
            _stream(), C.byref(self.P), self.beta_T if beta_T is None else beta_T, self.tau_p if tau_p is None else tau_p,
            ptr("active", self.active), ptr("kT", self.kT), ptr("pressure", self.p0), self._rid(), ptr("virial", self.virial),
            ptr("kinetic", self.kinetic), ptr("cell64", self.cell64), ptr("cell32", self.cell32), ptr("coords", self.x),
            ptr("coords_lo", self.lo), ptr("velocities", self.v), ptr("scale", self.scale))

    def barostat(self, step):
        self._lib.check(self.barostat_rc(step))

    def kick(self):
        self._lib.check(self.lib.anihip_md_kick(
            _stream(), C.byref(self.P), self.active.data_ptr(), self.mass.data_ptr(), self.v.data_ptr(), self.zero.data_ptr(),
            self.kinetic.data_ptr(), self.ws.data_ptr(), self.ws.numel()))

    def pair(self):
        return self.x.double().cpu().numpy() + self.lo.double().cpu().numpy()


def _state(Cn, A, seed=5):
    """Positions in fp64 with |x| <= 20 A (the two-float pair holds them to 20 * 2^-47 A), velocities, triclinic cells, and an
    active mask with padding in the middle molecule, two fixed atoms and two atoms marked as owned by a constraint cluster."""
    rs = np.random.RandomState(seed)
    x = rs.uniform(-20.0, 20.0, (Cn, A, 3))
    hi = x.astype(np.float32)
    x = hi.astype(np.float64) + (x - hi).astype(np.float32).astype(np.float64)   # exactly a pair of floats
    v = rs.normal(0.0, 0.01, (Cn, A, 3)).astype(np.float32).astype(np.float64)
    mass = MASS_BY_INDEX[rs.randint(0, 7, (Cn, A))].astype(np.float32).astype(np.float64)
    active = np.ones((Cn, A), dtype=np.uint8)
    active[Cn // 2, A - 9:] = 0               # padding
    active[0, 5] = active[Cn - 1, A - 1] = 0   # fixed
    active[0, 7] = active[Cn - 1, 2] = 2       # ANIHIP_MD_ATOM_CLUSTER: scaled like a free atom
    cell = np.tile(np.diag([41.0, 39.0, 43.0]), (Cn, 1, 1)) + rs.uniform(-4.0, 4.0, (Cn, 3, 3))
    return x, v, mass, active, cell


# ---- the move with K, W, kT and P0 given ------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cn, A", [(3, 70), (2, 300)])
def test_barostat_move_matches_reference(dev, Cn, A):
    """Gates: the pair coords + coords_lo within 1e-10 A (the constraints' gate; the pair resolves 20 * 2^-47 = 1.4e-13 A),
    velocities within one fp32 ulp of the largest |v|, cell64, kinetic and scale to 1e-13 relative, cell32 = (float)cell64,
    inactive atoms untouched bit for bit.  xi_b is, by definition, the fp32 variate of anihip_md_noise widened to fp64: the
    reference is fed the device's own draw at the barostat's word, and that draw is held against the fp64 Philox restatement
    at the gate of test_noise_matches_reference (2e-5)."""
    x, v, mass, active, cell = _state(Cn, A)
    v[active == 0] = 0.123   # (what an inactive atom holds is none of the barostat's business)
    rs = np.random.RandomState(8)
    rid = [5, 0, 3][:Cn]
    kT = (ref.KB_HARTREE * np.array([250.0, 300.0, 350.0])[:Cn]).astype(np.float32).astype(np.float64)
    p0 = np.array([1.0, 1000.0, -500.0])[:Cn] / BAR
    beta_T, tau_p, dt = 4.57e-5 * BAR, 20.0, 0.5
    K, W = rs.uniform(0.2, 0.4, Cn), rs.normal(0.0, 0.3, (Cn, 3, 3))
    k = Kernels(dev, x, v, active, mass, cell, dt, kT, np.full(Cn, 0.01), beta_T, tau_p, p0, rid)
    k.kinetic.copy_(torch.from_numpy(K))
    k.virial.copy_(torch.from_numpy(W.reshape(Cn, 9)))
    x_before, lo_before, v_before = k.x.clone(), k.lo.clone(), k.v.clone()
    k.barostat(STEP0)
    xi = _noise(dev, SEED, bref.noise_word(STEP0), Cn, 1, rid)[:, 0, 0].astype(np.float64)
    d_xi = np.abs(xi - bref.barostat_noise(SEED, STEP0, Cn, rid)).max()
    assert d_xi <= 2e-5
    x1, v1, cell1, K1, mu = bref.barostat(x, v, cell, K, W, active != 0, kT, p0, beta_T, tau_p, dt, xi)
    got_mu, got_K = k.scale.cpu().numpy(), k.kinetic.cpu().numpy()
    got_cell, got_cell32 = k.cell64.cpu().numpy().reshape(Cn, 3, 3), k.cell32.cpu().numpy().reshape(Cn, 3, 3)
    got_v = k.v.cpu().numpy()
    err_x = np.abs(k.pair() - x1).max()
    ulp_v = np.spacing(np.float32(np.abs(v1[active != 0]).max()))
    err_v = np.abs(got_v.astype(np.float64) - v1).max()
    err_mu, err_K = np.abs(got_mu / mu - 1.0).max(), np.abs(got_K / K1 - 1.0).max()
    err_cell = (np.abs(got_cell - cell1).max(axis=(1, 2)) / np.abs(cell1).max(axis=(1, 2))).max()
    print(f"md barostat move [{Cn}][{A}]: mu - 1 = {', '.join(f'{m:.3e}' for m in mu - 1.0)}  |d pair| {err_x:.2e} A  |dv| "
          f"{err_v / ulp_v:.2f} ulp of max |v|  d mu {err_mu:.1e}  d K {err_K:.1e}  d cell {err_cell:.1e}  |xi - xi_ref| {d_xi:.1e}")
    assert np.abs(mu - 1.0).min() > 1e-6   # (a move worth comparing)
    assert err_x <= 1e-10
    assert err_v <= ulp_v
    assert err_mu <= 1e-13 and err_K <= 1e-13 and err_cell <= 1e-13
    assert np.array_equal(got_cell32, got_cell.astype(np.float32))
    off = torch.from_numpy(active == 0).to(dev)
    assert torch.equal(k.x[off], x_before[off]) and torch.equal(k.lo[off], lo_before[off]) and torch.equal(k.v[off], v_before[off])
    # coords is the fp32 nearest to the pair
    assert np.array_equal(k.pair().astype(np.float32), k.x.cpu().numpy())


def test_barostat_argument_checks(dev):
    x, v, mass, active, cell = _state(2, 70)
    args = (dev, x, v, active, mass, cell, 0.5, np.full(2, 1e-3), np.full(2, 0.01), 2000.0, 100.0, np.zeros(2))
    k = Kernels(*args)
    before = k.cell64.clone()
    err = lambda: k.lib.anihip_last_error().decode()   # noqa: E731
    assert k.barostat_rc(0, beta_T=0.0) != 0 and "beta_T" in err()
    assert k.barostat_rc(0, tau_p=-1.0) != 0 and "tau_p" in err()
    assert k.barostat_rc(1 << 62) != 0 and "2^62" in err()
    for name in ("active", "kT", "pressure", "virial", "kinetic", "cell64", "cell32", "coords", "coords_lo", "velocities", "scale"):
        assert k.barostat_rc(0, **{name: True}) != 0 and "null" in err(), name
    k.P.dt = 0.0
    assert k.barostat_rc(0) != 0 and "dt" in err()
    nve = Kernels(*args, langevin=False)
    assert nve.barostat_rc(0) != 0 and "Langevin" in err()
    assert torch.equal(k.cell64, before)   # a refused call launches nothing


# ---- the NPT ideal gas ------------------------------------------------------------------------------------------------------

def _ideal_gas(dev, seed, n_steps, rid=None):
    """drift / barostat / kick with zero forces and a zero virial on the setup of the reference; returns the cells of every
    step [n_steps, C, 9] (one device copy per step, read at the end) and the kernels."""
    s = bref.ideal_gas_setup()
    Cn, A = s["n_mol"], s["n_atoms"]
    zero = np.zeros((Cn, A, 3))
    k = Kernels(dev, zero, zero, np.ones((Cn, A), dtype=np.uint8), np.full((Cn, A), s["mass"]),
                np.tile(np.eye(3) * s["side"], (Cn, 1, 1)), s["dt"], np.full(Cn, s["kT"]), np.full(Cn, s["friction"]),
                s["beta_T"], s["tau_p"], np.full(Cn, s["p0"]), rid, seed)
    cells = torch.empty((n_steps, Cn, 9), dtype=torch.float64, device=dev)
    for step in range(n_steps):
        k.drift(step)
        k.barostat(step)
        k.kick()
        cells[step].copy_(k.cell64)
    return cells, k, s


def test_device_samples_the_npt_ideal_gas(dev):
    """The setup and the gates of test_reference_samples_the_npt_ideal_gas (3 % on the mean volume, 15 % on its variance), with
    the seed at which the reference sits inside half of each gate (1.0011 and 0.981).  kT is rounded to fp32 on the device,
    6e-8 relative, far below either gate."""
    cells, k, s = _ideal_gas(dev, IDEAL_GAS_SEED, 4000)
    vol = bref.volume(cells.cpu().numpy().reshape(-1, 3, 3)).reshape(4000, s["n_mol"])
    mean, var = bref.ideal_gas_ratios(vol, s, drop=400)
    print(f"md barostat device, ideal gas seed {IDEAL_GAS_SEED}: <V> / ((N+1) kT/P0) = {mean:.4f}, "
          f"Var V / ((N+1) (kT/P0)^2) = {var:.4f}")
    assert np.isfinite(k.pair()).all()
    assert abs(mean - 1.0) <= 0.03
    assert abs(var - 1.0) <= 0.15


def test_volume_path_is_bit_identical_and_follows_the_replica_id(dev):
    runs = [_ideal_gas(dev, 3, 50) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1].x, runs[1][1].x) and torch.equal(runs[0][1].lo, runs[1][1].lo)
    assert torch.equal(runs[0][1].v, runs[1][1].v)
    rid = list(range(64))
    rid[1], rid[7], rid[63] = 7, 1, 1000
    other, _, _ = _ideal_gas(dev, 3, 50, rid)
    same = [c for c in range(64) if c not in (1, 7, 63)]
    assert torch.equal(other[:, same], runs[0][0][:, same])
    assert torch.equal(other[:, 1], runs[0][0][:, 7]) and torch.equal(other[:, 7], runs[0][0][:, 1])   # a replica, wherever it sits
    assert not torch.equal(other[:, 63], runs[0][0][:, 63])                                            # another id, another path


# ---- whole NPT steps on a model ---------------------------------------------------------------------------------------------

def _npt_case(base, dev, **kw):
    """BatchedDynamics with a barostat on a fixture (periodic in all three directions: the triclinic fixture's own pbc leaves
    z open, which the barostat refuses) and what the reference needs."""
    from torchani_amd.md import BatchedDynamics

    model, sp, x, cell, _ = _ani_case(base, dev)
    spn = sp.cpu().numpy()
    mass = MASS_BY_INDEX[np.clip(spn, 0, 6)].astype(np.float32).astype(np.float64)
    par = dict(dt=0.5, temperature=300.0, friction=0.05, replica_ids=torch.tensor([11]), seed=SEED, pressure=2000.0,
               compressibility=4.57e-5, barostat_time=200.0)
    par.update(kw)
    bd = BatchedDynamics(model, sp, x, cell, (True, True, True), masses=torch.from_numpy(mass).to(dev), **par)
    return bd, model, sp, x, cell, mass, par


def _reference_step(bd, mass, par, step):
    """One step of ``bd`` in lock-step with the reference, which is fed the device's forces and virial: returns what the
    reference makes of the state before the step, (x, v, kinetic, cell), given the forces of the device after it."""
    active = (bd.species >= 0).cpu().numpy()
    Cn, A = active.shape
    rid = bd._replica_ids.cpu().numpy()
    x0 = bd.coordinates.double().cpu().numpy() + bd.coordinates_lo.double().cpu().numpy()
    v0, f0 = bd.velocities.double().cpu().numpy(), bd.forces.double().cpu().numpy()
    K0, W0 = bd.kinetic_energies().cpu().numpy(), bd._model_eval.virial.cpu().numpy().reshape(1, 3, 3)
    cell0 = bd.cell64.cpu().numpy().reshape(1, 3, 3)
    kT = (bd.temperature.cpu().numpy() * np.float32(ref.KB_HARTREE)).astype(np.float64)   # (the device forms k_B T in fp32)
    fr = bd.friction.double().cpu().numpy()
    p0 = bd.pressure.cpu().numpy() / BAR
    bd.step()
    x1, vm = ref.drift(x0, v0, f0, active, mass, par["dt"], True, kT, fr, ref.noise(SEED, step, Cn, A, rid))
    x2, v2, cell1, _, mu = bref.barostat(x1, vm, cell0, K0, W0, active, kT, p0, par["compressibility"] * BAR, par["barostat_time"],
                                         par["dt"], bref.barostat_noise(SEED, step, Cn, rid))
    v3, ke = ref.kick(v2, bd.forces.double().cpu().numpy(), active, mass, par["dt"])
    return x2, v3, ke, cell1, mu


@pytest.mark.parametrize("base", ["water_pbc_ani2x", "triclinic_pbc_ani2x"])
def test_npt_steps_on_ani2x_match_reference(dev, base):
    """Three steps of drift, barostat, evaluation, kick on ANI-2x x 8 with the gates of
    test_langevin_steps_on_ani2x_match_reference; the cell within ten times the difference measured (CELL_DIFF_MEASURED).
    The pressure moves by several hundred bar from one evaluation to the next here, so a move made with the virial of the
    new evaluation shifts mu by (beta_T / tau_p) dP dt / 3 ~ 2e-5 and the coordinates by ~7e-5 A, tens of times their gate; a
    kinetic energy taken after the drift instead of before it showed as 1.6e-5 A; another step word redraws xi_b (1e-3 in mu)."""
    bd, model, sp, x, cell, mass, par = _npt_case(base, dev)
    bd.set_temperature(300.0)   # (the kinetic energy is stale at the first move: refreshed on the device)
    assert bd.cell is not cell and bd.cell.dtype == torch.float32 and bd.cell64.dtype == torch.float64
    worst, moves = 0.0, []
    for s in range(3):
        assert bd.steps_done == s
        x2, v3, ke, cell1, mu = _reference_step(bd, mass, par, s)
        _assert_close(bd.coordinates.double().cpu().numpy(), bd.velocities.double().cpu().numpy(),
                      bd.kinetic_energies().cpu().numpy(), x2, v3, ke)
        got = bd.cell64.cpu().numpy().reshape(1, 3, 3)
        worst = max(worst, np.abs(got - cell1).max() / np.abs(cell1).max())
        moves.append(float(mu[0]) - 1.0)
        assert abs(bd.barostat_scale.item() / mu[0] - 1.0) <= 1e-6
        assert torch.equal(bd.cell, bd.cell64.float())
        assert np.allclose(bd.volumes().cpu().numpy(), bref.volume(got), rtol=1e-14)
    print(f"md barostat NPT steps on {base}: mu - 1 = {', '.join(f'{m:.3e}' for m in moves)}, largest |cell64 - cell_ref| "
          f"/ max |cell_ref| = {worst:.2e}, P = {bd.pressures().item():.4e} bar, V = {bd.volumes().item():.3f} A^3")
    assert min(abs(m) for m in moves) > 1e-5   # (moves that a wrong ordering would show in)
    assert worst <= 10.0 * CELL_DIFF_MEASURED[base]
    # the forces and the virial held are the model's at the coordinates and the cell held
    out = model.energies_and_forces(sp, bd.coordinates, bd.cell, bd.pbc, stress=True)
    assert (out.forces - bd.forces).abs().max().item() <= 1e-5 * max(1.0, out.forces.abs().max().item())
    assert (out.virial - bd._model_eval.virial).abs().max().item() <= 1e-5 * max(1.0, out.virial.abs().max().item())
    # the caller's cell is not the one that moved
    assert np.array_equal(cell.cpu().numpy(), load_golden(base)["cell"])


# ---- pressures() ------------------------------------------------------------------------------------------------------------

def _fd_pressure(energy, x, cell, h):
    """-(E(V (1 + h)) - E(V (1 - h))) / (2 h V) under isotropic scaling of coordinates and cell, Hartree / Angstrom^3."""
    V = float(bref.volume(cell.double().cpu().numpy())[0])
    e = [energy((x.double() * s).float(), (cell.double() * s).float()) for s in ((1.0 + h) ** (1.0 / 3.0), (1.0 - h) ** (1.0 / 3.0))]
    return -(e[0] - e[1]) / (2.0 * h * V)


def _check_pressure(name, bd, model, sp, x, cell, atomic_e):
    """pressures() at rest (K = 0: the configurational part) against central differences of the energy in the volume.

    Noise of one energy: dE = 8 * 2^-24 sqrt(N) max |e_i| (every atomic energy is an fp32 number at the end of a chain of fp32
    sums: 8 half-ulps each, adding at random over the atoms) + 2^-24 max |x| |F|_2 (the scaled coordinates are rounded to fp32)
    + 2^-24 |W|_F (so is the scaled cell).  Truncation: for pair energies falling as r^-6 .. r^-12, E ~ V^-2 .. V^-4 and
    V^3 E''' = 12 .. 30 times V E'; with 20, FD(h) is off by h^2 20 |V E'| / (6 V) ~ 1.1 h^2 |tr W| / V, the noise is
    dE / (h V), and the sum is smallest at h = (dE / (2 |tr W|))^(1/3), capped at 0.02.  The gate does not rest on that factor
    of 20: the truncation is taken from the differences themselves, FD(2h) - FD(h) = 3 times that of FD(h), so
    gate = |FD(2h) - FD(h)| / 3 + 1.5 dE / (h V) (the noise of FD(h), and a third of that of FD(2h) - FD(h))."""
    from torchani_amd.geomopt import ModelEvaluator

    N = int((sp >= 0).sum())
    W = bd._model_eval.virial.cpu().numpy()
    V = bd.volumes().item()
    dE = (8.0 * 2.0 ** -24 * np.sqrt(N) * float(atomic_e.abs().max()) + 2.0 ** -24 * float(x.abs().max()) * float(bd.forces.double().norm())
          + 2.0 ** -24 * float(np.linalg.norm(W)))
    h = min(0.02, (dE / (2.0 * abs(np.trace(W)))) ** (1.0 / 3.0))
    energy = lambda xs, cs: ModelEvaluator(model, sp, cs, bd.pbc)(xs.contiguous())[0].item()   # noqa: E731
    fd1, fd2 = _fd_pressure(energy, x, cell, h), _fd_pressure(energy, x, cell, 2.0 * h)
    gate = abs(fd2 - fd1) / 3.0 + 1.5 * dE / (h * V)
    p = bd.pressures().item()
    print(f"md barostat pressures() on {name}: P = {p:.6e} bar, finite difference {fd1 * BAR:.6e} bar at h = {h:.2e} "
          f"({fd2 * BAR:.6e} at 2h), |dP| = {abs(p - fd1 * BAR):.2e} bar, gate {gate * BAR:.2e} bar (energy noise {dE:.1e} Ha)")
    assert bd.kinetic_energies().item() == 0.0
    assert abs(p - (-np.trace(W) / (3.0 * V)) * BAR) <= 1e-12 * abs(p)
    assert abs(p / BAR - fd1) <= gate
    assert gate <= 0.05 * abs(p / BAR)   # (a comparison that says something)


def test_pressures_match_finite_differences_on_water(dev):
    bd, model, sp, x, cell, mass, par = _npt_case("water_pbc_ani2x", dev)
    out = model.energies_and_forces(sp, x, cell, bd.pbc)
    _check_pressure("water_pbc_ani2x", bd, model, sp, x, cell, out.atomic_energies)
    # with kinetic energy: the ideal-gas term on top
    bd.set_temperature(300.0)
    ke = bd.kinetic_energies().item()
    p_conf = -bd._model_eval.virial.diagonal().sum().item() / (3.0 * bd.volumes().item())
    assert abs(bd.pressures().item() / BAR - (p_conf + 2.0 * ke / (3.0 * bd.volumes().item()))) <= 1e-12 * abs(p_conf)


def test_pressures_of_a_standalone_pair_potential(dev):
    """ModelEvaluator(stress=True) on a standalone potential (the ``virial=`` argument of ``accumulate``): 27 atoms on a
    jittered 2.5 A grid in a 7.5 A cell, Lennard-Jones with a 5 A cutoff."""
    from torchani_amd.md import BatchedDynamics
    from torchani_amd.potentials import LennardJones

    rs = np.random.RandomState(4)
    grid = np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing="ij"), -1).reshape(-1, 3) * 2.5
    x = torch.from_numpy((grid + rs.uniform(-0.2, 0.2, grid.shape)).astype(np.float32)).to(dev).unsqueeze(0)
    cell = (torch.eye(3) * 7.5).to(dev)
    sp = torch.ones((1, 27), dtype=torch.int64, device=dev)
    lj = LennardJones(("H",), eps=(0.002,), sigma=(2.4,), cutoff=5.0).to(dev)
    bd = BatchedDynamics(lj, sp, x, cell, (True, True, True), masses=torch.full((1, 27), 12.011, device=dev), temperature=100.0,
                         pressure=1.0)
    atomic_e = lj(sp, x, cell, (True, True, True), atomic=True)
    _check_pressure("Lennard-Jones 27", bd, lj, sp, x, cell, atomic_e)
    bd.run(3)
    assert bd.steps_done == 3 and bool(torch.isfinite(bd.cell64).all()) and bd.volumes().item() != 7.5 ** 3


# ---- behaviour of the Python layer ------------------------------------------------------------------------------------------

def test_npt_step_does_not_synchronize_and_pressure_is_read(dev):
    bd, model, sp, x, cell, mass, par = _npt_case("water_pbc_ani2x", dev)
    bd.set_temperature(300.0)
    for _ in range(3):
        bd.step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            bd.step()
        bd.set_velocities(0.5 * bd.velocities)   # (a stale kinetic energy is refreshed without a host read)
        bd.step()
        bd.volumes(), bd.pressures(), bd.kinetic_energies(), bd.temperatures()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bd.steps_done == 7
    bd.run(3, check_every=2)
    assert bd.steps_done == 10
    # the user's write to ``pressure`` is read by the next step: 2e5 bar more shrinks the box by
    # (beta_T / tau_p) dP dt / 3 = 4.57e-5 * 2e5 * 0.5 / 200 / 3 = 7.6e-3 in mu against the reference fed the old pressure
    bd.pressure.fill_(2.0e5 + par["pressure"])
    x2, v3, ke, cell1, mu = _reference_step(bd, mass, par, 10)
    got = bd.cell64.cpu().numpy().reshape(1, 3, 3)
    measured, diff = CELL_DIFF_MEASURED["water_pbc_ani2x"], np.abs(got - cell1).max() / np.abs(cell1).max()
    print(f"md barostat, pressure overwritten: mu - 1 = {mu[0] - 1.0:.3e}, |cell64 - cell_ref| / max |cell_ref| = {diff:.2e}")
    assert diff <= 10.0 * measured
    old = mu[0] * np.exp(par["compressibility"] * 2.0e5 * par["dt"] / par["barostat_time"] / 3.0)   # mu at the old pressure
    assert abs(bd.barostat_scale.item() / mu[0] - 1.0) <= 1e-6 and abs(bd.barostat_scale.item() / old - 1.0) > 5e-3
    _assert_close(bd.coordinates.double().cpu().numpy(), bd.velocities.double().cpu().numpy(),
                  bd.kinetic_energies().cpu().numpy(), x2, v3, ke)


def test_barostat_argument_errors(dev):
    from torchani_amd.md import BatchedDynamics, BondConstraints

    model, sp, x, cell, _ = _ani_case("water_pbc_ani2x", dev)
    pbc = (True, True, True)
    mass = torch.from_numpy(MASS_BY_INDEX.astype(np.float32)).to(dev)[sp.clamp(min=0)]
    ok = dict(masses=mass, temperature=300.0, pressure=1.0)
    make = lambda *a, **kw: BatchedDynamics(model, *a, **{**ok, **kw})   # noqa: E731
    with pytest.raises(ValueError, match="Langevin"):
        make(sp, x, cell, pbc, temperature=None)
    with pytest.raises(ValueError, match="C = 1"):
        make(sp.repeat(2, 1), x.repeat(2, 1, 1), cell, pbc, masses=mass.repeat(2, 1))
    with pytest.raises(ValueError, match="periodic in all three"):
        make(sp, x, None, None)
    with pytest.raises(ValueError, match="periodic in all three"):
        make(sp, x, cell, (True, True, False))
    fixed = torch.zeros(sp.shape, dtype=torch.bool, device=dev)
    fixed[0, 2] = True
    with pytest.raises(ValueError, match="fixed atoms"):
        make(sp, x, cell, pbc, fixed=fixed)
    with pytest.raises(ValueError, match="constraints"):
        make(sp, x, cell, pbc, constraints=BondConstraints(torch.tensor([[[0, 1]]])))
    with pytest.raises(ValueError, match="compressibility"):
        make(sp, x, cell, pbc, compressibility=0.0)
    with pytest.raises(ValueError, match="barostat_time"):
        make(sp, x, cell, pbc, barostat_time=-1.0)
    with pytest.raises(ValueError, match="pressure must be"):
        make(sp, x, cell, pbc, pressure=torch.zeros(2))
    # no barostat: no new attribute is needed, and the observable that needs the virial says so
    nvt = make(sp, x, cell, pbc, pressure=None)
    assert not nvt.barostat and nvt.cell is cell and abs(nvt.volumes().item() - 512.0) < 1e-9
    with pytest.raises(ValueError, match="pressure="):
        nvt.pressures()
    # all-padding constraints and an all-False mask are no constraints and no fixed atoms
    make(sp, x, cell, pbc, fixed=torch.zeros_like(fixed), constraints=BondConstraints(torch.full((1, 1, 2), -1)))
