"""The on-device MD integrator (csrc/md.hip, torchani_amd.md.BatchedDynamics) on the MI355X against the fp64 reference of
tests/_md_ref.py: the Philox / Box-Muller noise, drift and kick with the forces given, the two-float coordinates, the thermostat
on a temperature ladder, whole Langevin steps on ANI-2x and NVE against the host driver MolecularDynamics.

Shapes: C = 3, A = 70 (more than a wave per molecule, no multiple of 64, padding in the middle molecule, two fixed atoms, permuted
replica ids) and C = 2, A = 300 (more than one 256-atom chunk per molecule: the per-molecule sums take a second launch)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _md_ref as ref
from _util import load_golden, seeded_state

pytestmark = pytest.mark.gpu

MASS_BY_INDEX = np.array([1.008, 12.011, 14.007, 15.999, 32.06, 18.998, 35.45])   # ANI-2x element order H C N O S F Cl
SEED = (0x9E3779B9 << 32) | 12345      # both key words in use
STEP0 = (3 << 32) | 17                 # both step words in use


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from torchani_amd import _lib

    _lib.lib()
    return torch.device("cuda:0")


def _stream():
    from torchani_amd.engine import _stream as s

    return s()


def _noise(dev, seed, step, Cn, A, rid=None):
    from torchani_amd import _lib

    out = torch.empty((Cn, A, 3), dtype=torch.float32, device=dev)
    r = None if rid is None else torch.as_tensor(rid, dtype=torch.int64).to(dev)
    _lib.check(_lib.lib().anihip_md_noise(_stream(), seed, step, Cn, A, None if r is None else r.data_ptr(), out.data_ptr()))
    return out.cpu().numpy()


class Kernels:
    """The C ABI on a state made from numpy arrays: x, v [C, A, 3], active [C, A], mass [C, A]."""

    def __init__(self, dev, x, v, active, mass, dt, langevin=False, kT=None, friction=None, rid=None, seed=SEED):
        from torchani_amd import _lib

        self.lib, self._lib = _lib.lib(), _lib
        Cn, A = active.shape
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)   # noqa: E731
        self.x, self.v, self.lo = f32(x), f32(v), torch.zeros((Cn, A, 3), dtype=torch.float32, device=dev)
        self.active = torch.from_numpy(active.astype(np.uint8)).to(dev)
        self.mass = f32(mass)
        self.inv_mass = (ref.ACC_UNIT / self.mass.double()).float()
        self.kT = None if kT is None else f32(kT)
        self.friction = None if friction is None else f32(friction)
        self.rid = None if rid is None else torch.as_tensor(rid, dtype=torch.int64).to(dev)
        self.P = _lib.MdParams(Cn, A, _lib.MD_LANGEVIN if langevin else 0, 0, dt, seed, 0)
        self.ws = torch.empty(self.lib.anihip_md_workspace_bytes(Cn, A), dtype=torch.uint8, device=dev)
        self.kinetic = torch.zeros(Cn, dtype=torch.float64, device=dev)
        self.f32 = f32

    @staticmethod
    def _ptr(t):
        return None if t is None else t.data_ptr()

    def drift(self, f, step):
        self.P.step = step
        self._f = self.f32(f)
        self._lib.check(self.lib.anihip_md_drift(
            _stream(), C.byref(self.P), self.active.data_ptr(), self.inv_mass.data_ptr(), self._ptr(self.kT),
            self._ptr(self.friction), self._ptr(self.rid), self.x.data_ptr(), self.lo.data_ptr(), self.v.data_ptr(),
            self._f.data_ptr()))

    def kick(self, f):
        self._f = self.f32(f)
        self._lib.check(self.lib.anihip_md_kick(
            _stream(), C.byref(self.P), self.active.data_ptr(), self.mass.data_ptr(), self.v.data_ptr(), self._f.data_ptr(),
            self.kinetic.data_ptr(), self.ws.data_ptr(), self.ws.numel()))

    def remove_drift(self):
        self._lib.check(self.lib.anihip_md_remove_drift(
            _stream(), C.byref(self.P), self.active.data_ptr(), self.mass.data_ptr(), self.v.data_ptr(), self.ws.data_ptr(),
            self.ws.numel()))


def _state(Cn, A, seed=11):
    """Random positions, velocities, two force sets, masses and an active mask with padding in the middle molecule and two
    fixed atoms; everything rounded to fp32 so that the reference starts from what the device holds."""
    rs = np.random.RandomState(seed)
    r32 = lambda a: a.astype(np.float32).astype(np.float64)   # noqa: E731
    x, v = r32(rs.uniform(-20.0, 20.0, (Cn, A, 3))), r32(rs.normal(0.0, 0.01, (Cn, A, 3)))
    f0, f1 = r32(rs.normal(0.0, 0.05, (Cn, A, 3))), r32(rs.normal(0.0, 0.05, (Cn, A, 3)))
    mass = r32(MASS_BY_INDEX[rs.randint(0, 7, (Cn, A))])
    active = np.ones((Cn, A), dtype=bool)
    active[Cn // 2, A - 9:] = False           # padding
    active[0, 5] = active[Cn - 1, A - 1] = False   # fixed
    v[~active] = 0.0
    return x, v, f0, f1, mass, active


def _assert_close(got_x, got_v, got_ke, want_x, want_v, want_ke):
    """The gates of every comparison with the reference: coordinates to 4 ulp of the largest one, velocities to 1e-5 of the
    largest, kinetic energies to relative 1e-6."""
    tol_x = 4.0 * np.spacing(np.float32(np.abs(want_x).max()))
    err_x, err_v = np.abs(got_x - want_x).max(), np.abs(got_v - want_v).max()
    err_ke = np.abs(got_ke / want_ke - 1.0).max()
    print(f"md device: |dx| {err_x:.2e} (gate {tol_x:.2e})  |dv| / max |v| {err_v / np.abs(want_v).max():.2e}  "
          f"|dKE| / KE {err_ke:.2e}")
    assert err_x <= tol_x
    assert err_v <= 1e-5 * np.abs(want_v).max()
    assert err_ke <= 1e-6


# ---- noise ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cn, A, rid, steps", [(3, 70, [5, 0, 3], [STEP0]), (2, 300, None, [STEP0, ref.MB_STEP | 2]),
                                               (64, 64, None, [0, 1, 2, 3])])
def test_noise_matches_reference(dev, Cn, A, rid, steps):
    worst, big = 0.0, 0.0
    for step in steps:
        got, want = _noise(dev, SEED, step, Cn, A, rid), ref.noise(SEED, step, Cn, A, rid)
        worst, big = max(worst, np.abs(got - want).max()), max(big, np.abs(want).max())
    print(f"md noise [{Cn}][{A}] x {len(steps)} steps: max |xi - xi_ref| = {worst:.2e}, max |xi| = {big:.2f}")
    assert worst <= 2e-5


def test_noise_rows_follow_replica_ids(dev):
    base = _noise(dev, SEED, STEP0, 6, 70)
    perm = [4, 1, 5, 0, 3, 2]
    assert np.array_equal(_noise(dev, SEED, STEP0, 6, 70, perm), base[perm])
    assert np.array_equal(_noise(dev, SEED, STEP0, 2, 70, [5, 3]), base[[5, 3]])     # nor on the batch size
    assert np.array_equal(_noise(dev, SEED, STEP0, 6, 33), base[:, :33])             # nor on the padded length
    assert np.array_equal(_noise(dev, SEED, STEP0, 6, 70), base)                      # bit-identical run to run
    assert not np.array_equal(_noise(dev, SEED, STEP0 + 1, 6, 70), base)
    assert not np.array_equal(_noise(dev, SEED ^ (1 << 40), STEP0, 6, 70), base)


# ---- kernels alone -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("langevin", [False, True], ids=["nve", "langevin"])
@pytest.mark.parametrize("Cn, A", [(3, 70), (2, 300)])
def test_drift_and_kick_match_reference(dev, Cn, A, langevin):
    x, v, f0, f1, mass, active = _state(Cn, A)
    dt = 0.5
    rid = [5, 0, 3][:Cn]
    kT = ref.KB_HARTREE * np.array([250.0, 300.0, 350.0])[:Cn]
    friction = np.array([0.002, 0.5, 0.01])[:Cn]
    k = Kernels(dev, x, v, active, mass, dt, langevin, kT if langevin else None, friction if langevin else None, rid)
    k.drift(f0, STEP0)
    k.kick(f1)
    xi = ref.noise(SEED, STEP0, Cn, A, rid)
    x1, vm = ref.drift(x, v, f0, active, mass, dt, langevin, kT, friction, xi)
    v1, ke = ref.kick(vm, f1, active, mass, dt)
    gx, gv, glo = k.x.cpu().numpy(), k.v.cpu().numpy(), k.lo.cpu().numpy()
    _assert_close(gx.astype(np.float64), gv.astype(np.float64), k.kinetic.cpu().numpy(), x1, v1, ke)
    # inactive atoms: coordinates bit-identical, velocity zero, no residual
    assert np.array_equal(gx[~active], x[~active].astype(np.float32))
    assert np.all(gv[~active] == 0.0) and np.all(glo[~active] == 0.0)
    # coords is the fp32 nearest to the pair, and the pair is closer to the reference than fp32 can hold
    pair = gx.astype(np.float64) + glo.astype(np.float64)
    assert np.array_equal(pair.astype(np.float32), gx)
    assert np.abs(pair - x1)[active].max() <= 0.25 * np.spacing(np.float32(np.abs(x1).max()))


def test_kick_zeroes_inactive_velocities_and_is_bit_identical(dev):
    x, v, f0, f1, mass, active = _state(2, 300)
    v[~active] = 0.123   # (set_temperature never writes these; a caller of the C ABI might)
    runs = []
    for _ in range(2):
        k = Kernels(dev, x, v, active, mass, 0.5)
        k.kick(f1)
        runs.append((k.v.clone(), k.kinetic.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert bool((runs[0][0].cpu().numpy()[~active] == 0.0).all())


# ---- two-float coordinates -----------------------------------------------------------------------------------------------

def test_two_float_coordinates_keep_steps_below_one_ulp(dev):
    """dt v = 1e-6 A at x = 200 A, where one fp32 ulp is 1.5e-5 A: 1000 drifts move the pair by 1e-3 A."""
    dt, v = 0.5, 2e-6
    x0 = np.array([[[200.0, -200.0, 0.0]]])
    k = Kernels(dev, x0, np.full((1, 1, 3), v), np.ones((1, 1), dtype=bool), np.array([[15.999]]), dt)
    zero = np.zeros((1, 1, 3))
    for s in range(1000):
        k.drift(zero, s)
    hi, lo = k.x.cpu().numpy().astype(np.float64), k.lo.cpu().numpy().astype(np.float64)
    pair = (hi + lo)[0, 0]
    print(f"md two-float: x = {pair[0]:.9f} (coords {hi[0, 0, 0]:.9f} + residual {lo[0, 0, 0]:.3e})")
    assert np.abs(pair - (x0[0, 0] + 1e-3)).max() <= 1e-7
    assert np.array_equal((hi + lo).astype(np.float32).astype(np.float64), hi)
    # what the residual is for: plain fp32 accumulation never leaves 200
    plain = np.float32(200.0)
    for _ in range(1000):
        plain = plain + np.float32(dt) * np.float32(v)
    assert plain == np.float32(200.0)


# ---- thermostat ----------------------------------------------------------------------------------------------------------

def test_thermostat_reaches_each_molecules_temperature(dev):
    """Zero forces: the O step is the exact Ornstein-Uhlenbeck update, so after 40 steps of friction 0.5 / fs (c1^40 = 2e-9)
    every velocity component is a fresh draw at T_c.  T_measured / T_c of one molecule (192 components) has variance 2 / 192."""
    Cn = A = 64
    rs = np.random.RandomState(2)
    mass = MASS_BY_INDEX[rs.randint(0, 7, (Cn, A))]
    T = 100.0 + 10.0 * np.arange(Cn)
    active = np.ones((Cn, A), dtype=bool)
    zero = np.zeros((Cn, A, 3))
    k = Kernels(dev, zero, zero, active, mass, 1.0, True, ref.KB_HARTREE * T, np.full(Cn, 0.5))
    for s in range(40):
        k.drift(zero, s)
        k.kick(zero)
    ratio = 2.0 * k.kinetic.cpu().numpy() / (3 * A * ref.KB_HARTREE) / T
    lo, hi, both = ratio[:Cn // 2].mean(), ratio[Cn // 2:].mean(), ratio.mean()
    print(f"md thermostat: mean T / T_c = {lo:.4f} (100-410 K), {hi:.4f} (420-730 K), {both:.4f} (all)")
    sigma_half = np.sqrt(2.0 / (3 * A * Cn // 2))
    assert abs(lo - 1.0) <= 5.0 * sigma_half and abs(hi - 1.0) <= 5.0 * sigma_half
    assert abs(both - 1.0) <= 5.0 * sigma_half / np.sqrt(2.0)
    # the positions moved by what the velocities say: x is the sum of the half drifts, all finite
    assert np.isfinite(k.x.cpu().numpy()).all()
    k.remove_drift()
    v = k.v.cpu().numpy().astype(np.float64)
    p = (mass[..., None] * v).sum(axis=1)
    scale = (mass[..., None] * np.abs(v)).sum(axis=1)
    print(f"md remove_drift: max |sum m v| / sum m |v| = {(np.abs(p) / scale).max():.2e}")
    assert (np.abs(p) <= 1e-5 * scale).all()


@pytest.mark.parametrize("Cn, A", [(3, 70), (2, 300)])
def test_remove_drift_matches_reference(dev, Cn, A):
    x, v, f0, f1, mass, active = _state(Cn, A)
    v = v + 0.02   # a drift worth removing
    v[~active] = 0.0
    k = Kernels(dev, x, v, active, mass, 0.5)
    k.remove_drift()
    m = np.where(active, mass, 0.0)[..., None]
    want = np.where(active[..., None], v - (m * v).sum(axis=1, keepdims=True) / m.sum(axis=1, keepdims=True), 0.0)
    got = k.v.cpu().numpy()
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
    assert np.all(got[~active] == 0.0)


# ---- whole steps on a model ----------------------------------------------------------------------------------------------

def _ani_case(base, dev, **kw):
    from torchani_amd.models import ANI2x

    g = load_golden(base)
    sp = torch.from_numpy(g["species"].astype(np.int64)).to(dev)
    x = torch.from_numpy(g["coords"]).to(dev)
    cell = None if g["cell"] is None else torch.from_numpy(g["cell"]).to(dev)
    pbc = None if g["pbc"] is None else tuple(bool(b) for b in g["pbc"])
    model = ANI2x(state_dict=seeded_state("ani2x", 8, 7), device=dev, periodic_table_index=False,
                  cutoff_fn=g["cutoff_fn"], row_capacity=256, **kw)
    return model, sp, x, cell, pbc


@pytest.mark.parametrize("base", ["rand_batch_ani2x", "triclinic_pbc_ani2x"])
def test_langevin_steps_on_ani2x_match_reference(dev, base):
    from torchani_amd.md import BatchedDynamics

    model, sp, x, cell, pbc = _ani_case(base, dev)
    Cn, A = sp.shape
    spn = sp.cpu().numpy()
    mass = np.where(spn >= 0, MASS_BY_INDEX[np.clip(spn, 0, 6)], 1.0).astype(np.float32).astype(np.float64)
    fixed = np.zeros((Cn, A), dtype=bool)
    fixed[0, 1] = fixed[Cn - 1, 0] = True
    active = (spn >= 0) & ~fixed
    T = 250.0 + 40.0 * np.arange(Cn)
    friction = np.linspace(0.002, 0.2, Cn)
    rid = list(np.random.RandomState(1).permutation(Cn) + 3)
    dt = 0.5
    bd = BatchedDynamics(model, sp, x, cell, pbc, dt=dt, masses=torch.from_numpy(mass).to(dev),
                         temperature=torch.from_numpy(T), friction=torch.from_numpy(friction),
                         fixed=torch.from_numpy(fixed).to(dev), replica_ids=torch.tensor(rid), seed=SEED)
    # Maxwell-Boltzmann velocities from the same stream, drift removed
    bd.set_temperature(torch.from_numpy(T))
    m = np.where(active, mass, 0.0)[..., None]
    v_mb = np.sqrt(ref.KB_HARTREE * T[:, None, None] * ref.ACC_UNIT / mass[..., None]) * ref.noise(SEED, ref.MB_STEP, Cn, A, rid)
    v_mb = np.where(active[..., None], v_mb, 0.0)
    v_mb = np.where(active[..., None], v_mb - (m * v_mb).sum(axis=1, keepdims=True) / m.sum(axis=1, keepdims=True), 0.0)
    got = bd.velocities.cpu().numpy()
    assert np.abs(got - v_mb).max() <= 1e-5 * np.abs(v_mb).max()
    ke_mb = 0.5 * (m * v_mb ** 2).sum(axis=(1, 2)) / ref.ACC_UNIT
    assert np.abs(bd.kinetic_energies().cpu().numpy() / ke_mb - 1.0).max() <= 1e-5
    kT = ref.KB_HARTREE * T.astype(np.float32).astype(np.float64)
    fr = friction.astype(np.float32).astype(np.float64)
    for s in range(3):
        x0 = bd.coordinates.double().cpu().numpy() + bd.coordinates_lo.double().cpu().numpy()
        v0, f0 = bd.velocities.double().cpu().numpy(), bd.forces.double().cpu().numpy()
        assert bd.steps_done == s
        bd.step()
        x1, vm = ref.drift(x0, v0, f0, active, mass, dt, True, kT, fr, ref.noise(SEED, s, Cn, A, rid))
        v1, ke = ref.kick(vm, bd.forces.double().cpu().numpy(), active, mass, dt)
        _assert_close(bd.coordinates.double().cpu().numpy(), bd.velocities.double().cpu().numpy(),
                      bd.kinetic_energies().cpu().numpy(), x1, v1, ke)
        assert np.array_equal(bd.coordinates.cpu().numpy()[~active], x.cpu().numpy()[~active])
    # the forces held are the model's at the coordinates held (an eager evaluation next to the replayed graph: the fp32
    # atomics of the force accumulation add in another order)
    out = model.energies_and_forces(sp, bd.coordinates, cell, pbc)
    assert (out.forces - bd.forces).abs().max().item() <= 1e-5
    assert (out.energies - bd.potential_energies).abs().max().item() <= 1e-6
    temps = bd.temperatures().cpu().numpy()
    assert np.allclose(temps, 2.0 * ke / (3 * active.sum(axis=1) * ref.KB_HARTREE), rtol=1e-6)   # Langevin: no dof removed
    assert torch.equal(bd.total_energies(), bd.potential_energies + bd.kinetic_energies())


def test_step_does_not_synchronize_and_annealing_is_read(dev):
    from torchani_amd.md import BatchedDynamics

    model, sp, x, cell, pbc = _ani_case("rand_batch_ani2x", dev)
    Cn, A = sp.shape
    mass = torch.from_numpy(MASS_BY_INDEX.astype(np.float32)).to(dev)[sp.clamp(min=0)]
    bd = BatchedDynamics(model, sp, x, cell, pbc, masses=mass, temperature=300.0, friction=0.5, seed=1)
    for _ in range(3):   # (the third evaluation captures the automatic HIP graph)
        bd.step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(4):
            bd.step()
        bd.kinetic_energies(), bd.temperatures(), bd.total_energies()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bd.steps_done == 7
    bd.run(5, check_every=2)
    assert bd.steps_done == 12
    # the user's write to ``temperature`` is read by the next step: at 0 K the thermostat only damps, whatever the noise
    bd.temperature.fill_(0.0)
    active = (sp >= 0).cpu().numpy()
    x0 = bd.coordinates.double().cpu().numpy() + bd.coordinates_lo.double().cpu().numpy()
    v0, f0 = bd.velocities.double().cpu().numpy(), bd.forces.double().cpu().numpy()
    bd.step()
    m = np.where(active, mass.double().cpu().numpy(), 1.0)
    x1, vm = ref.drift(x0, v0, f0, active, m, 0.5, True, np.zeros(Cn), np.full(Cn, np.float64(np.float32(0.5))),
                       np.zeros((Cn, A, 3)))
    v1, ke = ref.kick(vm, bd.forces.double().cpu().numpy(), active, m, 0.5)
    _assert_close(bd.coordinates.double().cpu().numpy(), bd.velocities.double().cpu().numpy(),
                  bd.kinetic_energies().cpu().numpy(), x1, v1, ke)


# ---- against the host driver ---------------------------------------------------------------------------------------------

def test_nve_agrees_with_host_driver_on_water_box(dev):
    """60 x 0.25 fs of NVE on the 3000-atom water box from the same velocities: the coordinates agree with MolecularDynamics
    to the 1e-3 A that test_gpu_md.py asks between its two runs, and the total energy drifts within that file's bound."""
    from test_gpu_md import make_model, water
    from torchani_amd.md import BatchedDynamics, MolecularDynamics

    sp, x, cell, pbc = water(10)
    spd = torch.from_numpy(sp.astype(np.int64)).to(dev)
    xd, cd = torch.from_numpy(x).to(dev), torch.from_numpy(cell).to(dev)
    masses = torch.tensor([1.008, 12.011, 14.007, 15.999, 32.06, 18.998, 35.45], device=dev)[spd]
    host = MolecularDynamics(make_model(dev, "cell_list"), spd, xd, cd, pbc, dt=0.25, masses=masses, seed=1)
    host.set_temperature(150.0)
    device = BatchedDynamics(make_model(dev, "cell_list"), spd, xd, cd, pbc, dt=0.25, masses=masses)
    device.set_velocities(host.velocities)
    e0, ke0 = device.total_energies().clone(), device.kinetic_energies().clone()
    assert abs((ke0 - host.kinetic_energies()).item()) <= 1e-6 * ke0.item()
    host.run(60)
    device.run(60)
    torch.cuda.synchronize()
    dx = (device.coordinates - host.coords).abs().max().item()
    drift = (device.total_energies() - e0).abs().item()
    dke = (device.kinetic_energies() - ke0).abs().item()
    print(f"md device vs host, water 3000 atoms, 60 x 0.25 fs NVE: max |x_device - x_host| = {dx:.2e} A, |dE_total| = "
          f"{drift:.2e} Ha (|dKE| = {dke:.2e})")
    assert dx < 1e-3
    assert drift < 0.02 * max(dke, 1e-3) + 1e-4
    # the velocities copied in carry the host driver's centre-of-mass velocity: every degree of freedom counts, and three
    # less (NVE, nothing fixed) once that velocity is removed
    ke = device.kinetic_energies()
    assert torch.allclose(device.temperatures(), 2.0 * ke / (3 * sp.size * ref.KB_HARTREE), rtol=1e-12)
    device.remove_center_of_mass_velocity()
    ke_rest = device.kinetic_energies()
    assert 0.0 < (ke - ke_rest).item() < 0.01 * ke.item()
    assert torch.allclose(device.temperatures(), 2.0 * ke_rest / ((3 * sp.size - 3) * ref.KB_HARTREE), rtol=1e-12)
    device.set_velocities(host.velocities)
    assert torch.allclose(device.temperatures(), 2.0 * device.kinetic_energies() / (3 * sp.size * ref.KB_HARTREE), rtol=1e-12)
