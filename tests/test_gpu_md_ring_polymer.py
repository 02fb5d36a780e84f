"""The ring-polymer integrator (anihip_md_rp_drift, anihip_md_rp_estimators, torchani_amd.md.RingPolymerDynamics) on the MI355X
against the fp64 reference of tests/_md_ring_polymer_ref.py, with the gates of tests/test_gpu_md_device.py.

Shapes (R polymers, P beads, A atoms): (2, 5, 70) odd P (no k = P / 2 mode), padding, one fixed atom, permuted replica ids, a
temperature and a friction per polymer; (1, 2, 300) the smallest P and more than one 64-atom and one 256-atom chunk;
(1, 64, 3) the largest P; (3, 8, 33) even P with the k = P / 2 mode, A no multiple of the wave; (1, 20, 9) and (1, 12, 40) the
kernel instances for up to 32 and 16 beads."""
import ctypes as C

import numpy as np
import pytest
import torch

import _md_ref as ref
import _md_ring_polymer_ref as rp
from _util import load_golden
from test_gpu_md_device import MASS_BY_INDEX, SEED, STEP0, Kernels, _ani_case, _assert_close, _stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from torchani_amd import _lib

    _lib.lib()
    return torch.device("cuda:0")


class RpKernels(Kernels):
    """The C ABI on a batch of R P entries: kT and friction [R] are repeated per bead, polymer r draws the streams rid[r] P + k."""

    def __init__(self, dev, P, x, v, active, mass, dt, kT, langevin=False, friction=None, rid=None, lam=1.0, seed=SEED):
        R = active.shape[0] // P
        self.beads, self.lam = P, lam
        self.bead_rid = None if rid is None else (np.asarray(rid)[:, None] * P + np.arange(P)).reshape(-1)
        super().__init__(dev, x, v, active, mass, dt, langevin, np.repeat(kT, P),
                         None if friction is None else np.repeat(friction, P), self.bead_rid, seed)
        self.est = torch.zeros((R, 2), dtype=torch.float64, device=dev)
        self.cen = torch.zeros((R, active.shape[1], 3), dtype=torch.float64, device=dev)

    def rp_drift(self, f, step):
        self.P.step = step
        self._f = self.f32(f)
        self._lib.check(self.lib.anihip_md_rp_drift(
            _stream(), C.byref(self.P), self.beads, self.lam, self.active.data_ptr(), self.inv_mass.data_ptr(),
            self.kT.data_ptr(), self._ptr(self.friction), self._ptr(self.rid), self.x.data_ptr(), self.lo.data_ptr(),
            self.v.data_ptr(), self._f.data_ptr()))

    def estimators(self, f):
        self._f = self.f32(f)
        self._lib.check(self.lib.anihip_md_rp_estimators(
            _stream(), C.byref(self.P), self.beads, self.active.data_ptr(), self.mass.data_ptr(), self.kT.data_ptr(),
            self.x.data_ptr(), self.lo.data_ptr(), self._f.data_ptr(), self.est.data_ptr(), self.cen.data_ptr(),
            self.ws.data_ptr(), self.ws.numel()))
        return self.est.cpu().numpy(), self.cen.cpu().numpy()

    def pair(self):
        return self.x.cpu().numpy().astype(np.float64) + self.lo.cpu().numpy().astype(np.float64)


def _rp_state(R, P, A, seed=11):
    """Ring polymers as a run holds them: centroids anywhere within 20 A of the origin, beads within a few tenths of an A
    of them, bead velocities of the size of P T, two force sets; masses and the active mask per polymer (padding at the end of the
    middle polymer, one fixed atom in the first), everything rounded to fp32 so that the reference starts from what the device
    holds.  Inactive atoms have beads apart too: they must come back bit for bit."""
    rs = np.random.RandomState(seed)
    r32 = lambda a: a.astype(np.float32).astype(np.float64)   # noqa: E731
    Cn = R * P
    x = r32(np.repeat(rs.uniform(-20.0, 20.0, (R, 1, A, 3)), P, axis=1).reshape(Cn, A, 3) + rs.normal(0.0, 0.15, (Cn, A, 3)))
    v = r32(rs.normal(0.0, 0.01 * np.sqrt(P), (Cn, A, 3)))
    f0, f1 = r32(rs.normal(0.0, 0.05, (Cn, A, 3))), r32(rs.normal(0.0, 0.05, (Cn, A, 3)))
    mass_r = r32(MASS_BY_INDEX[rs.randint(0, 7, (R, A))])
    active_r = np.ones((R, A), dtype=bool)
    if A > 9:
        active_r[R // 2, A - 9:] = False   # padding
        active_r[0, 5] = False             # fixed
    mass, active = np.repeat(mass_r, P, axis=0), np.repeat(active_r, P, axis=0)
    v[~active] = 0.0
    return x, v, f0, f1, mass, active


SHAPES = [(2, 5, 70), (1, 2, 300), (1, 64, 3), (3, 8, 33), (1, 20, 9), (1, 12, 40)]
CASES = [(*s, 1.0, langevin) for s in SHAPES for langevin in (False, True)] + [(2, 5, 70, 0.5, True)]   # (lambda: the thermostat's)


@pytest.mark.parametrize("R, P, A, lam, langevin", CASES)
def test_rp_drift_and_kick_match_reference(dev, R, P, A, lam, langevin):
    x, v, f0, f1, mass, active = _rp_state(R, P, A)
    dt = 0.5
    rid = [5, 0, 3][:R]
    r32 = lambda a: a.astype(np.float32).astype(np.float64)   # noqa: E731
    kT = r32(ref.KB_HARTREE * np.array([250.0, 330.0, 300.0])[:R])
    friction = r32(np.array([0.002, 0.5, 0.01])[:R])
    k = RpKernels(dev, P, x, v, active, mass, dt, kT, langevin, friction if langevin else None, rid, lam)
    k.rp_drift(f0, STEP0)
    k.kick(f1)
    xi = ref.noise(SEED, STEP0, R * P, A, k.bead_rid)
    x1, vm = rp.drift(x, v, f0, active, mass, dt, P, kT, langevin, friction, lam, xi)
    v1, ke = ref.kick(vm, f1, active, mass, dt)
    gx, gv, glo = k.x.cpu().numpy(), k.v.cpu().numpy(), k.lo.cpu().numpy()
    _assert_close(gx.astype(np.float64), gv.astype(np.float64), k.kinetic.cpu().numpy(), x1, v1, ke)
    # inactive atoms: coordinates bit-identical, velocity zero, no residual
    assert np.array_equal(gx[~active], x[~active].astype(np.float32))
    assert np.all(gv[~active] == 0.0) and np.all(glo[~active] == 0.0)
    # coords is the fp32 nearest to the pair, and the pair is closer to the reference than fp32 can hold
    pair = gx.astype(np.float64) + glo.astype(np.float64)
    assert np.array_equal(pair.astype(np.float32), gx)
    err = np.abs(pair - x1)[active].max()
    print(f"md ring polymer ({R}, {P}, {A}): |pair - x_ref| = {err:.2e} (gate {0.25 * np.spacing(np.float32(np.abs(x1).max())):.2e})")
    assert err <= 0.25 * np.spacing(np.float32(np.abs(x1).max()))
    assert np.abs(x1 - x)[active].max() > 1e-3   # (the step moved them by far more than the gate)


def test_equal_beads_stay_equal_and_follow_the_classical_drift(dev):
    """All beads on one point, at rest, with the same force on every bead: the springs never act, the beads stay equal bit for
    bit, and each follows the classical NVE drift of tests/_md_ref.py."""
    R, P, A = 2, 6, 70
    x, v, f0, f1, mass, active = _rp_state(R, P, A)
    fold = lambda a: np.repeat(a.reshape(R, P, A, -1)[:, :1], P, axis=1).reshape(R * P, A, -1)   # noqa: E731
    x, f0, f1 = fold(x), fold(f0), fold(f1)
    v = np.zeros_like(x)
    kT = ref.KB_HARTREE * np.array([250.0, 330.0])
    k = RpKernels(dev, P, x, v, active, mass, 0.5, kT)
    xr, vr = x, v
    for s, (fa, fb) in enumerate([(f0, f1), (f1, f0), (f0, f0)]):
        k.rp_drift(fa, s)
        k.kick(fb)
        xr, vm = ref.drift(xr, vr, fa, active, mass, 0.5)
        vr, ke = ref.kick(vm, fb, active, mass, 0.5)
        for t in (k.x, k.lo, k.v):
            b = t.view(R, P, A, 3)
            assert torch.equal(b, b[:, :1].expand(R, P, A, 3))
        _assert_close(k.x.double().cpu().numpy(), k.v.double().cpu().numpy(), k.kinetic.cpu().numpy(), xr, vr, ke)
        assert np.abs(k.pair() - xr)[active].max() <= 0.25 * np.spacing(np.float32(np.abs(xr).max()))


def test_centroid_keeps_steps_below_one_ulp(dev):
    """The analogue of test_two_float_coordinates_keep_steps_below_one_ulp: P = 4 beads at x = 200 A, where one fp32 ulp is
    1.5e-5 A, with dt v = 1e-6 A and zero forces: 1000 RPMD drifts move the centroid by 1e-3 A."""
    P, dt, v = 4, 0.5, 2e-6
    x0 = np.tile(np.array([[[200.0, -200.0, 0.0]]]), (P, 1, 1))
    k = RpKernels(dev, P, x0, np.full((P, 1, 3), v), np.ones((P, 1), dtype=bool), np.full((P, 1), 15.999), dt,
                  np.array([ref.KB_HARTREE * 300.0]))
    zero = np.zeros((P, 1, 3))
    for s in range(1000):
        k.rp_drift(zero, s)
    pair = k.pair()
    _, cen = k.estimators(zero)
    print(f"md ring polymer two-float: centroid x = {cen[0, 0, 0]:.9f} (coords {k.x[0, 0, 0].item():.9f} + residual "
          f"{k.lo[0, 0, 0].item():.3e})")
    assert np.abs(pair.mean(axis=0)[0] - (x0[0, 0] + 1e-3)).max() <= 1e-7
    assert np.abs(cen[0, 0] - (x0[0, 0] + 1e-3)).max() <= 1e-7
    assert np.array_equal(pair.astype(np.float32), k.x.cpu().numpy())
    assert np.array_equal(pair, np.tile(pair[:1], (P, 1, 1)))   # the beads stayed on one point


def test_free_ring_polymer_reaches_its_stationary_law(dev):
    """Zero forces under PILE, 200 steps of 1 fs from collapsed beads at rest (_md_ring_polymer_ref.FREE_CASE): the spread of
    the beads about their centroid and the bead kinetic temperature against the exact stationary law, which A and O each
    preserve at any dt.  The fp64 reference with the same noise passes the same gates (tests/test_md_ring_polymer_host.py)."""
    R, P, A, T, dt, friction, steps, seed = rp.FREE_CASE
    rs = np.random.RandomState(2)
    mass = np.repeat(MASS_BY_INDEX[rs.randint(0, 7, (R, A))], P, axis=0)
    zero = np.zeros((R * P, A, 3))
    k = RpKernels(dev, P, zero, zero, np.ones((R * P, A), dtype=bool), mass, dt, np.full(R, ref.KB_HARTREE * T), True,
                  np.full(R, friction), seed=seed)
    for s in range(steps):
        k.rp_drift(zero, s)
        k.kick(zero)
    spread, se, t_ratio, t_gate = rp.free_polymer_figures(k.pair(), k.kinetic.cpu().numpy(), mass, P, T)
    print(f"md ring polymer, free polymer on the device: spread / exact = {spread:.4f} (5 se = {5 * se:.4f}), "
          f"T_bead / (P T) = {t_ratio:.4f} (gate {t_gate:.4f})")
    assert abs(spread - 1.0) <= 5.0 * se
    assert abs(t_ratio - 1.0) <= t_gate


@pytest.mark.parametrize("R, P, A", [(2, 5, 70), (1, 2, 300)])
def test_estimators_match_reference_and_are_bit_identical(dev, R, P, A):
    x, v, f0, f1, mass, active = _rp_state(R, P, A)
    kT = (ref.KB_HARTREE * np.array([250.0, 330.0])[:R]).astype(np.float32).astype(np.float64)
    k = RpKernels(dev, P, x, v, active, mass, 0.5, kT)
    k.lo.copy_(torch.from_numpy((1e-7 * np.random.RandomState(3).uniform(-1, 1, x.shape)).astype(np.float32)))   # a residual to read
    est, cen = k.estimators(f0)
    S, W, S_abs, W_abs, cen_ref = rp.estimators(k.pair(), f0, active, mass, P, kT)
    # fp64 sums of P terms of the size of the largest coordinate: (P + 1) ulp of it bound the device's and the reference's orders
    tol_c = (P + 1) * np.spacing(np.abs(cen_ref).max())
    print(f"md ring polymer estimators ({R}, {P}, {A}): |dS| / sum |terms| = {np.abs(est[:, 0] - S).max() / S_abs.max():.2e}, "
          f"|dW| / sum |terms| = {np.abs(est[:, 1] - W).max() / W_abs.max():.2e}, |d centroid| = {np.abs(cen - cen_ref).max():.2e} "
          f"(gate {tol_c:.2e})")
    assert (np.abs(est[:, 0] - S) <= 1e-6 * S_abs).all() and (np.abs(est[:, 1] - W) <= 1e-6 * W_abs).all()
    assert np.abs(cen - cen_ref).max() <= tol_c
    assert (S > 0).all() and (W_abs > 0).all()
    est2, cen2 = k.estimators(f0)
    assert np.array_equal(est, est2) and np.array_equal(cen, cen2)


# ---- RingPolymerDynamics on ANI-2x ------------------------------------------------------------------------------------------

def _rp_case(base, dev, P, spread=0.02, **kw):
    from torchani_amd.md import RingPolymerDynamics

    model, sp, x, cell, pbc = _ani_case(base, dev)
    R, A = sp.shape
    spn = sp.cpu().numpy()
    mass = np.where(spn >= 0, MASS_BY_INDEX[np.clip(spn, 0, 6)], 1.0).astype(np.float32).astype(np.float64)
    beads = x.unsqueeze(1).repeat(1, P, 1, 1)
    if spread:
        g = torch.Generator().manual_seed(4)
        beads = beads + (spread * torch.randn(beads.shape, generator=g)).to(dev) * (sp >= 0).view(R, 1, A, 1)
    dyn = RingPolymerDynamics(model, sp, beads if spread else x, cell, pbc, beads=P, masses=torch.from_numpy(mass).to(dev), **kw)
    return dyn, sp, x, mass


@pytest.mark.parametrize("base", ["rand_batch_ani2x", "triclinic_pbc_ani2x"])
def test_pile_steps_on_ani2x_match_reference(dev, base):
    P, dt = 4, 0.5
    R, A = load_golden(base)["species"].shape
    fixed = np.zeros((R, A), dtype=bool)
    fixed[0, 1] = fixed[R - 1, 0] = True
    T = 250.0 + 40.0 * np.arange(R)
    friction = np.linspace(0.002, 0.2, R)
    rid = np.random.RandomState(1).permutation(R) + 3
    dyn, sp, x, mass_r = _rp_case(base, dev, P, dt=dt, temperature=torch.from_numpy(T), friction=torch.from_numpy(friction),
                                  fixed=torch.from_numpy(fixed).to(dev), replica_ids=torch.from_numpy(rid), seed=SEED)
    Cn = R * P
    assert tuple(dyn.coordinates.shape) == (Cn, A, 3) and dyn.beads == P and dyn.n_polymers == R
    active = np.repeat((sp.cpu().numpy() >= 0) & ~fixed, P, axis=0)
    mass = np.repeat(mass_r, P, axis=0)
    bead_rid = (rid[:, None] * P + np.arange(P)).reshape(-1)
    # Maxwell-Boltzmann velocities of the beads at P T, from the stream of the dynamics
    dyn.set_temperature(torch.from_numpy(T))
    v_mb = np.sqrt(ref.KB_HARTREE * P * np.repeat(T, P)[:, None, None] * ref.ACC_UNIT / mass[..., None]) \
        * ref.noise(SEED, ref.MB_STEP, Cn, A, bead_rid)
    v_mb = np.where(active[..., None], v_mb, 0.0)
    assert np.abs(dyn.velocities.cpu().numpy() - v_mb).max() <= 1e-5 * np.abs(v_mb).max()
    fr = friction.astype(np.float32).astype(np.float64)
    x_start = dyn.coordinates.cpu().numpy().copy()
    for s in range(3):
        if s == 2:   # the user's write between steps is read by the next one
            dyn.temperature.mul_(1.25)
        kT = ref.KB_HARTREE * dyn.temperature.view(R, P)[:, 0].double().cpu().numpy()
        x0 = dyn.coordinates.double().cpu().numpy() + dyn.coordinates_lo.double().cpu().numpy()
        v0, f0 = dyn.velocities.double().cpu().numpy(), dyn.forces.double().cpu().numpy()
        assert dyn.steps_done == s
        dyn.step()
        x1, vm = rp.drift(x0, v0, f0, active, mass, dt, P, kT, True, fr, 1.0, ref.noise(SEED, s, Cn, A, bead_rid))
        v1, ke = ref.kick(vm, dyn.forces.double().cpu().numpy(), active, mass, dt)
        _assert_close(dyn.coordinates.double().cpu().numpy(), dyn.velocities.double().cpu().numpy(),
                      dyn.kinetic_energies().cpu().numpy(), x1, v1, ke)
        assert np.array_equal(dyn.coordinates.cpu().numpy()[~active], x_start[~active])
    assert dyn.steps_done == 3
    # the observables against the reference estimators on the state held
    pair = dyn.coordinates.double().cpu().numpy() + dyn.coordinates_lo.double().cpu().numpy()
    S, W, S_abs, W_abs, cen = rp.estimators(pair, dyn.forces.double().cpu().numpy(), active, mass, P, kT)
    n_act = active.reshape(R, P, A)[:, 0].sum(axis=1)
    assert np.abs(dyn.spring_energies().cpu().numpy() - S).max() <= 1e-6 * S_abs.max()
    assert np.abs(dyn.centroids().cpu().numpy() - cen).max() <= (P + 1) * np.spacing(np.abs(cen).max())
    cv = dyn.quantum_kinetic_energies().cpu().numpy()
    prim = dyn.quantum_kinetic_energies("primitive").cpu().numpy()
    assert np.abs(cv - (1.5 * n_act * kT - W / (2 * P))).max() <= 1e-6 * (W_abs.max() + cv.max())
    assert np.abs(prim - (1.5 * n_act * P * kT - S / P)).max() <= 1e-6 * (S_abs.max() + np.abs(prim).max())
    e_rp = (dyn.kinetic_energies() + dyn.potential_energies).view(R, P).sum(dim=1).cpu().numpy() + S
    assert np.abs(dyn.ring_polymer_energies().cpu().numpy() - e_rp).max() <= 1e-6 * S_abs.max() + 1e-9 * np.abs(e_rp).max()
    assert np.allclose(dyn.temperatures().cpu().numpy(), 2.0 * ke / (3 * active.sum(axis=1) * ref.KB_HARTREE), rtol=1e-6)


def test_step_and_observables_do_not_synchronize(dev):
    dyn, sp, x, mass = _rp_case("rand_batch_ani2x", dev, 4, spread=0.0, temperature=300.0, friction=0.5, seed=1)
    for _ in range(3):   # (the third evaluation captures the automatic HIP graph)
        dyn.step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(4):
            dyn.step()
        dyn.kinetic_energies(), dyn.temperatures(), dyn.centroids(), dyn.spring_energies(), dyn.ring_polymer_energies()
        dyn.quantum_kinetic_energies(), dyn.quantum_kinetic_energies("primitive")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert dyn.steps_done == 7
    dyn.run(5, check_every=2)
    assert dyn.steps_done == 12
    # collapsed beads at the start have spread, and a [R, A, 3] start put every bead on the one point
    assert float(dyn.spring_energies().min()) > 0.0


def test_rpmd_conserves_the_ring_polymer_energy(dev):
    """thermostat=None over 100 x 0.25 fs from bead velocities at P x 300 K: the drift of ring_polymer_energies() within the NVE
    gate of tests/test_gpu_md_device.py."""
    dyn, sp, x, mass = _rp_case("rand_batch_ani2x", dev, 4, spread=0.0, dt=0.25, temperature=300.0, thermostat=None, seed=3)
    dyn.set_temperature(300.0)
    e0 = dyn.ring_polymer_energies().clone()
    ke0 = dyn.kinetic_energies().view(-1, 4).sum(dim=1).clone()
    dyn.run(100)
    torch.cuda.synchronize()
    drift = (dyn.ring_polymer_energies() - e0).abs()
    dke = (dyn.kinetic_energies().view(-1, 4).sum(dim=1) - ke0).abs()
    print(f"md ring polymer RPMD, 6 molecules x 4 beads, 100 x 0.25 fs: max |dE_rp| = {drift.max().item():.2e} Ha "
          f"(max |dKE| = {dke.max().item():.2e}, spring energy {dyn.spring_energies().max().item():.2e})")
    assert bool((drift <= 0.02 * dke.clamp(min=1e-3) + 1e-4).all())
    assert float(dyn.spring_energies().min()) > 1e-5   # (the beads did spread: the springs took part)


def test_error_paths(dev):
    from torchani_amd.md import BondConstraints, RingPolymerDynamics

    model, sp, x, cell, pbc = _ani_case("rand_batch_ani2x", dev)
    R, A = sp.shape
    mass = torch.from_numpy(MASS_BY_INDEX.astype(np.float32)).to(dev)[sp.clamp(min=0)]
    make = lambda coords=x, **kw: RingPolymerDynamics(model, sp, coords, cell, pbc, masses=mass,   # noqa: E731
                                                      **{"beads": 4, "temperature": 300.0, **kw})
    pairs = torch.full((R, 1, 2), -1, dtype=torch.int64)
    with pytest.raises(ValueError, match="constraints"):
        make(constraints=BondConstraints(pairs))
    with pytest.raises(ValueError, match="pressure"):
        make(pressure=1.0)
    for beads in (1, 65, 0, 2.5):
        with pytest.raises(ValueError, match="beads"):
            make(beads=beads)
    with pytest.raises(ValueError, match="restart"):
        make(coords=x.unsqueeze(1).repeat(1, 3, 1, 1))        # [R, 3, A, 3] with beads = 4
    with pytest.raises(ValueError, match="temperature"):
        make(temperature=None)
    with pytest.raises(ValueError, match="replica_ids"):
        make(replica_ids=torch.full((R,), 1 << 30, dtype=torch.int64))   # 2^30 x 4 + k overflows one Philox word
    with pytest.raises(ValueError, match="thermostat"):
        make(thermostat="langevin")
    make(replica_ids=torch.full((R,), (1 << 30) - 1, dtype=torch.int64))   # the largest that fits
    # the C ABI refuses what it can see
    from torchani_amd import _lib

    k = RpKernels(dev, 4, np.zeros((8, 3, 3)), np.zeros((8, 3, 3)), np.ones((8, 3), dtype=bool), np.ones((8, 3)), 0.5,
                  np.full(2, 1e-3))
    for beads in (1, 65, 3):   # out of range, and 8 entries are no multiple of 3
        k.beads = beads
        with pytest.raises(RuntimeError, match="beads"):
            k.rp_drift(np.zeros((8, 3, 3)), 0)
    assert _lib.MD_RP_MAX_BEADS == 64
