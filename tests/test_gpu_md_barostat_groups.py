"""Molecular cell rescaling, the barostat with bond constraints (anihip_md_group_terms and anihip_md_barostat_groups in
csrc/md.hip, ``barostat_scaling="molecular"`` of torchani_amd.md.BatchedDynamics) on the MI355X against the fp64 restatement of
tests/_md_barostat_groups_ref.py: the group terms and one move with everything given, the case without clusters against
anihip_md_barostat bit for bit, the NPT ideal gas of rigid bodies, whole NPT steps of rigid waters on ANI-2x in lock-step with
the reference, ``pressures()`` against a finite difference of the energy in the volume under rigid-group scaling, and the
behaviour of the Python layer.

Shapes: C = 3, A = 70 of test_gpu_md_constraints.py (padding, dimers, triangles, XH4 stars, 3-bond chains, a cluster on atoms 63
and 64, two anchored clusters, permuted replica ids) and C = 2, A = 300 (100 dimers and 100 free atoms per molecule, one dimer
on atoms 255 and 256: two chunks per molecule, three launches for the sums)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _md_barostat_groups_ref as gref
import _md_barostat_ref as bref
import _md_constraints_ref as cref
import _md_ref as ref
from test_gpu_md_barostat import BAR, Kernels, _fd_pressure, _stream
from test_gpu_md_barostat import _state as _free_state
from test_gpu_md_constraints import _case as _cluster_case
from test_gpu_md_constraints import _state as _cluster_state
from test_gpu_md_device import MASS_BY_INDEX, SEED, STEP0, _ani_case, _assert_close, _noise
from test_md_barostat_groups_host import RIGID_GAS_SEED, RIGID_GAS_STEPS

pytestmark = pytest.mark.gpu

TOL = 5e-11   # constraint_tolerance of the lock-step runs: the residual gate after three steps is 1e-10
# The largest |cell64 - cell_ref| / max |cell_ref| of the three lock-step NPT steps, as measured
# (profiles/md_barostat_groups_tests.txt): the device draws xi_b in fp32 and the reference in fp64.  The gate is ten times that.
CELL_DIFF_MEASURED = 2.45e-10


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from torchani_amd import _lib

    _lib.lib()
    return torch.device("cuda:0")


class GroupKernels(Kernels):
    """The C ABI of an NPT step with constraints on the state of test_gpu_md_barostat.Kernels (x in fp64, split into the
    two-float pair) and cluster tables from md.build_constraint_clusters; ``forces`` [C, A, 3] or zero."""

    def __init__(self, dev, x, v, species, fixed, mass, pairs, lengths, cell, dt, kT, friction, beta_T, tau_p, p0, rid=None,
                 seed=SEED, forces=None, tol=1e-10):
        from torchani_amd import md

        Cn, A = species.shape
        super().__init__(dev, x, v, ((species >= 0) & ~fixed).astype(np.uint8), mass, cell, dt, kT, friction, beta_T, tau_p, p0,
                         rid, seed)
        if (pairs >= 0).any():
            cl = md.build_constraint_clusters(torch.from_numpy(species), torch.from_numpy(pairs), torch.from_numpy(lengths),
                                              torch.from_numpy(fixed), self.inv_mass.cpu())
            self.active[cl.owned.to(dev)] = self._lib.MD_ATOM_CLUSTER
            self.tables = [t.to(dev).contiguous() for t in (cl.atoms, cl.count, cl.bonds, cl.d2, cl.w)]
            self.iterations = torch.zeros((cl.atoms.shape[0], 2), dtype=torch.int32, device=dev)
            self.Q = self._lib.MdClusters(cl.atoms.shape[0], *(t.data_ptr() for t in self.tables), self.iterations.data_ptr(),
                                          tol, 64, int(cl.count[:, 0].max()), int(cl.count[:, 1].max()), 0)
        else:
            self.Q = self._lib.MdClusters(0, None, None, None, None, None, None, 1.0, 1, 0, 0, 0)
        self.f = self.zero if forces is None else torch.from_numpy(np.ascontiguousarray(forces, dtype=np.float32)).to(dev)
        self.kinetic_mol = torch.zeros(Cn, dtype=torch.float64, device=dev)
        self.virial_mol = torch.zeros(Cn, dtype=torch.float64, device=dev)
        # (filled with NaN: a term that no cluster wrote and a sum read would show)
        self.scratch = torch.full((self._lib.md_group_scratch_bytes(Cn, A) // 8,), float("nan"), dtype=torch.float64, device=dev)

    def group_terms(self):
        self._lib.check(self.lib.anihip_md_group_terms(
            _stream(), C.byref(self.P), C.byref(self.Q), self.active.data_ptr(), self.mass.data_ptr(), self.x.data_ptr(),
            self.lo.data_ptr(), self.v.data_ptr(), self.f.data_ptr(), self.scratch.data_ptr(), self.kinetic_mol.data_ptr(),
            self.virial_mol.data_ptr()))

    def barostat_groups(self, step):
        self.P.step = step
        self._lib.check(self.lib.anihip_md_barostat_groups(
            _stream(), C.byref(self.P), self.beta_T, self.tau_p, self.active.data_ptr(), self.kT.data_ptr(), self.p0.data_ptr(),
            self._rid(), self.virial.data_ptr(), self.kinetic.data_ptr(), self.cell64.data_ptr(), self.cell32.data_ptr(),
            self.x.data_ptr(), self.lo.data_ptr(), self.v.data_ptr(), self.scale.data_ptr(), C.byref(self.Q), self.mass.data_ptr(),
            self.kinetic_mol.data_ptr(), self.virial_mol.data_ptr()))

    def drift(self, step):
        super().drift(step)
        self._lib.check(self.lib.anihip_md_constrain_drift(
            _stream(), C.byref(self.P), C.byref(self.Q), self.kT.data_ptr(), self.friction.data_ptr(), self._rid(),
            self.x.data_ptr(), self.lo.data_ptr(), self.v.data_ptr(), self.zero.data_ptr()))

    def kick(self):
        self._lib.check(self.lib.anihip_md_constrain_kick(
            _stream(), C.byref(self.P), C.byref(self.Q), self.x.data_ptr(), self.lo.data_ptr(), self.v.data_ptr(),
            self.zero.data_ptr()))
        super().kick()


def _as_pair(x, rs):
    """x plus a residual below half an fp32 ulp: exactly a pair of floats whose first is the fp32 nearest to the sum."""
    x = x + rs.uniform(-2.0 ** -26, 2.0 ** -26, x.shape) * np.abs(x)
    hi = x.astype(np.float32)
    return hi.astype(np.float64) + (x - hi).astype(np.float32).astype(np.float64)


def _move_case(which):
    """x (pairs of floats, |x| <= 20 A), v, forces, mass, species, fixed, pairs, lengths and triclinic cells."""
    if which == 1:
        x, v, forces, mass, species, fixed, pairs, lengths = _cluster_case(1)
    else:
        mol = [[(3 * i, 3 * i + 1)] for i in range(100)]   # atoms 3 i + 2 are free; (255, 256) lies across the chunks
        x, v, forces, mass, species, fixed, pairs, lengths = _cluster_state(2, 300, [mol, mol], [], [])
    rs = np.random.RandomState(21)
    x = _as_pair(0.92 * x, rs)   # (the clusters reach 1.5 A beyond the 20 A of the first atoms)
    assert np.abs(x).max() <= 20.0
    Cn = species.shape[0]
    at = np.arange(Cn)[:, None]
    lengths = np.linalg.norm(x[at, np.maximum(pairs[..., 0], 0)] - x[at, np.maximum(pairs[..., 1], 0)], axis=-1)
    cell = np.tile(np.diag([41.0, 39.0, 43.0]), (Cn, 1, 1)) + rs.uniform(-4.0, 4.0, (Cn, 3, 3))
    return x, v, forces[0], mass, species, fixed, pairs, lengths, cell


# ---- the group terms and the move with K, W, kT, P0, forces and velocities given ----------------------------------------------

@pytest.mark.parametrize("which", [1, 2], ids=["C3_A70", "C2_A300"])
def test_group_terms_and_move_match_reference(dev, which):
    """Gates of test_barostat_move_matches_reference: the pair coords + coords_lo within 1e-10 A, velocities within one fp32
    ulp of the largest |v|, cell64, scale, kinetic and kinetic_mol to 1e-13 relative, cell32 = (float)cell64, inactive atoms
    and anchored clusters untouched bit for bit; the reference is fed the device's own xi_b.  Bond vectors of the pair before and
    after the move within 1e-12 A (the pair resolves 20 * 2^-48 = 7e-14 A).  virial_mol: X_q is a sum of at most 8 products and
    a quotient in fp64, off by at most 10 * 2^-53 |x| <= 2.2e-14 A at |x| <= 20 A, which enters G times the forces of the
    cluster: |dG| <= 4e-14 A * sum |f| over the molecule's components (the sum's own rounding is far below that)."""
    x, v, f, mass, species, fixed, pairs, lengths, cell = _move_case(which)
    Cn, A = species.shape
    active = (species >= 0) & ~fixed
    v = np.where(active[..., None], v, 0.123)   # (what an inactive atom holds is none of the barostat's business)
    rs = np.random.RandomState(8)
    rid = [5, 0, 3][:Cn]
    kT = (ref.KB_HARTREE * np.array([250.0, 300.0, 350.0])[:Cn]).astype(np.float32).astype(np.float64)
    p0 = np.array([1.0, 1000.0, -500.0])[:Cn] / BAR
    beta_T, tau_p, dt = 4.57e-5 * BAR, 20.0, 0.5
    K = 0.5 * (np.where(active, mass, 0.0)[..., None] * v ** 2).sum(axis=(1, 2)) / ref.ACC_UNIT
    W = rs.normal(0.0, 0.3, (Cn, 3, 3))
    k = GroupKernels(dev, x, v, species, fixed, mass, pairs, lengths, cell, dt, kT, np.full(Cn, 0.01), beta_T, tau_p, p0, rid,
                     forces=f)
    cons = cref.Constraints(pairs, lengths, active, mass)
    assert k.Q.n_clusters == len(cons.clusters) == (15 if which == 1 else 200)
    k.kinetic.copy_(torch.from_numpy(K))
    k.virial.copy_(torch.from_numpy(W.reshape(Cn, 9)))
    assert np.array_equal(k.pair(), x)
    k.group_terms()
    Km, G = gref.group_terms(x, v, f, active, mass, cons)
    got_Km, got_G = k.kinetic_mol.cpu().numpy(), k.virial_mol.cpu().numpy()
    err_Km, err_G = np.abs(got_Km / Km - 1.0).max(), np.abs(got_G - G)
    gate_G = 4e-14 * np.abs(np.where(active[..., None], f, 0.0)).sum(axis=(1, 2))
    print(f"md barostat groups terms case {which}: K_mol / K = {', '.join(f'{a:.3f}' for a in Km / K)}  G = "
          f"{', '.join(f'{g:.3e}' for g in G)} Ha  d K_mol {err_Km:.1e}  |dG| {err_G.max():.1e} Ha (gate {gate_G.min():.1e})")
    assert np.all(Km < K) and err_Km <= 1e-13 and np.all(err_G <= gate_G) and np.all(np.abs(G) > 100.0 * gate_G)
    x_before, lo_before, v_before = k.x.clone(), k.lo.clone(), k.v.clone()
    k.barostat_groups(STEP0)
    xi = _noise(dev, SEED, bref.noise_word(STEP0), Cn, 1, rid)[:, 0, 0].astype(np.float64)
    x1, v1, cell1, K1, Km1, mu = gref.barostat_groups(x, v, cell, K, Km, W, G, active, mass, cons, kT, p0, beta_T, tau_p, dt, xi)
    got_cell, got_cell32 = k.cell64.cpu().numpy().reshape(Cn, 3, 3), k.cell32.cpu().numpy().reshape(Cn, 3, 3)
    pair, got_v = k.pair(), k.v.cpu().numpy()
    err_x = np.abs(pair - x1).max()
    ulp_v = np.spacing(np.float32(np.abs(v1[active]).max()))
    err_v = np.abs(got_v.astype(np.float64) - v1).max()
    err_mu, err_K = np.abs(k.scale.cpu().numpy() / mu - 1.0).max(), np.abs(k.kinetic.cpu().numpy() / K1 - 1.0).max()
    err_Km1 = np.abs(k.kinetic_mol.cpu().numpy() / Km1 - 1.0).max()
    err_cell = (np.abs(got_cell - cell1).max(axis=(1, 2)) / np.abs(cell1).max(axis=(1, 2))).max()
    at = np.arange(Cn)[:, None]
    i, j = np.maximum(pairs[..., 0], 0), np.maximum(pairs[..., 1], 0)
    err_bond = np.abs((pair[at, i] - pair[at, j]) - (x[at, i] - x[at, j])).max()
    print(f"md barostat groups move case {which}: mu - 1 = {', '.join(f'{m:.3e}' for m in mu - 1.0)}  |d pair| {err_x:.2e} A  |dv| "
          f"{err_v / ulp_v:.2f} ulp of max |v|  d mu {err_mu:.1e}  d K {err_K:.1e}  d K_mol {err_Km1:.1e}  d cell {err_cell:.1e}  "
          f"|d bond vector| {err_bond:.1e} A")
    assert np.abs(mu - 1.0).min() > 1e-6   # (a move worth comparing)
    assert err_x <= 1e-10
    assert err_v <= ulp_v
    assert err_mu <= 1e-13 and err_K <= 1e-13 and err_Km1 <= 1e-13 and err_cell <= 1e-13
    assert np.array_equal(got_cell32, got_cell.astype(np.float32))
    assert err_bond <= 1e-12
    # inactive atoms and the atoms of anchored clusters come back bit for bit; every other atom has moved
    _, free = gref.scaling_groups(active, mass, cons)
    moved = free.copy()
    for mol, atoms, _ in gref.scaling_groups(active, mass, cons)[0]:
        moved[mol[:, None], atoms] = True
    assert (~moved & active).sum() == (3 if which == 1 else 0) and (~moved).sum() == (14 if which == 1 else 0)
    off = torch.from_numpy(~moved).to(dev)
    assert torch.equal(k.x[off], x_before[off]) and torch.equal(k.lo[off], lo_before[off]) and torch.equal(k.v[off], v_before[off])
    on = torch.from_numpy(moved).to(dev)
    assert bool(((k.x[on] != x_before[on]) | (k.lo[on] != lo_before[on])).any(dim=-1).all())
    # coords is the fp32 nearest to the pair
    assert np.array_equal(pair.astype(np.float32), k.x.cpu().numpy())
    # the kinetic energy returned is that of the moved velocities (fp32 velocities: 1e-6)
    ke = 0.5 * (np.where(active, mass, 0.0)[..., None] * got_v.astype(np.float64) ** 2).sum(axis=(1, 2)) / ref.ACC_UNIT
    assert np.abs(k.kinetic.cpu().numpy() / ke - 1.0).max() <= 1e-6


@pytest.mark.parametrize("Cn, A", [(3, 70), (2, 300)])
def test_no_clusters_is_the_atomic_barostat_bit_for_bit(dev, Cn, A):
    """n_clusters = 0, kinetic_mol = kinetic and virial_mol = 0: anihip_md_barostat on the same inputs, every output equal to
    the bit; and anihip_md_group_terms without clusters returns the kinetic energy of anihip_md_kick to the bit and G = 0."""
    x, v, mass, active, cell = _free_state(Cn, A)
    active[active == 2] = 1
    v[active == 0] = 0.0   # (anihip_md_kick, which sums the kinetic energy to compare with, sets them to zero)
    species, fixed = np.where(active != 0, 0, -1), np.zeros((Cn, A), dtype=bool)
    rs = np.random.RandomState(8)
    rid = [5, 0, 3][:Cn]
    kT = ref.KB_HARTREE * np.array([250.0, 300.0, 350.0])[:Cn]
    p0 = np.array([1.0, 1000.0, -500.0])[:Cn] / BAR
    args = (cell, 0.5, kT, np.full(Cn, 0.01), 4.57e-5 * BAR, 20.0, p0, rid)
    W = torch.from_numpy(rs.normal(0.0, 0.3, (Cn, 9))).to(dev)
    a = Kernels(dev, x, v, active, mass, *args)
    g = GroupKernels(dev, x, v, species, fixed, mass, np.full((Cn, 1, 2), -1, dtype=np.int64), np.zeros((Cn, 1)), *args)
    assert g.Q.n_clusters == 0 and torch.equal(a.active, g.active)
    a.kick()   # (zero forces: the velocities stay, the kinetic energy is summed)
    g.group_terms()
    assert torch.equal(g.kinetic_mol, a.kinetic) and bool((a.kinetic > 0).all()) and torch.equal(g.virial_mol, torch.zeros_like(g.virial_mol))
    g.kinetic.copy_(a.kinetic)
    a.virial.copy_(W), g.virial.copy_(W)
    a.barostat(STEP0), g.barostat_groups(STEP0)
    assert bool(((a.scale - 1.0).abs() > 1e-6).all())
    for name in ("x", "lo", "v", "cell64", "cell32", "kinetic", "scale"):
        assert torch.equal(getattr(a, name), getattr(g, name)), name
    assert torch.equal(g.kinetic_mol, g.kinetic)


# ---- the NPT ideal gas of rigid bodies ------------------------------------------------------------------------------------------

def _rigid_gas(dev, seed, n_steps, rid=None):
    """Constrained drift / barostat_groups / constrained kick / group_terms with zero forces and a zero virial on the setup of
    the reference; returns the cells of every step [n_steps, C, 9] (one device copy per step, read at the end) and the kernels."""
    s = gref.rigid_gas_setup()
    Cn, A = s["n_mol"], s["n_atoms"]
    x, pairs, lengths = gref.rigid_gas_state(s)
    k = GroupKernels(dev, x, np.zeros((Cn, A, 3)), np.zeros((Cn, A), dtype=np.int64), np.zeros((Cn, A), dtype=bool),
                     np.full((Cn, A), s["mass"]), pairs, lengths, np.tile(np.eye(3) * s["side"], (Cn, 1, 1)), s["dt"],
                     np.full(Cn, s["kT"]), np.full(Cn, s["friction"]), s["beta_T"], s["tau_p"], np.full(Cn, s["p0"]), rid, seed)
    k.group_terms()
    cells = torch.empty((n_steps, Cn, 9), dtype=torch.float64, device=dev)
    for step in range(n_steps):
        k.drift(step)
        k.barostat_groups(step)
        k.kick()
        k.group_terms()
        cells[step].copy_(k.cell64)
    return cells, k, s


def test_device_samples_the_npt_ideal_gas_of_rigid_bodies(dev):
    """The setup, the seed, the step count and the gates of test_reference_samples_the_npt_ideal_gas_of_rigid_bodies (3 % on the
    mean volume, 15 % on its variance; the reference sits within a third of each).  Three rigid dimers and two free atoms are
    five groups: counting the eight atoms would move the mean by +50 %, the full kinetic energy in place of the centre-of-mass
    one by +33 %."""
    cells, k, s = _rigid_gas(dev, RIGID_GAS_SEED, RIGID_GAS_STEPS)
    vol = bref.volume(cells.cpu().numpy().reshape(-1, 3, 3)).reshape(RIGID_GAS_STEPS, s["n_mol"])
    mean, var = gref.rigid_gas_ratios(vol, s, drop=400)
    pair = k.pair()
    res = np.abs(np.linalg.norm(pair[:, 0:6:2] - pair[:, 1:6:2], axis=-1) / gref.RIGID_GAS_BOND - 1.0).max()
    it = k.iterations.cpu().numpy()
    print(f"md barostat groups device, rigid-body ideal gas seed {RIGID_GAS_SEED}, {RIGID_GAS_STEPS} steps: "
          f"<V> / ((N_g+1) kT/P0) = {mean:.4f}, Var V / ((N_g+1) (kT/P0)^2) = {var:.4f}, bond residual {res:.1e}")
    assert np.isfinite(pair).all() and it.max() < 64
    assert res <= 2e-10   # (the gate of test_gpu_md_constraints.py at the kernels' tolerance of 1e-10: the moves keep the bonds)
    assert abs(mean - 1.0) <= 0.03
    assert abs(var - 1.0) <= 0.15


def test_volume_path_is_bit_identical_and_follows_the_replica_id(dev):
    runs = [_rigid_gas(dev, 3, 50) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1].x, runs[1][1].x) and torch.equal(runs[0][1].lo, runs[1][1].lo)
    assert torch.equal(runs[0][1].v, runs[1][1].v) and torch.equal(runs[0][1].kinetic_mol, runs[1][1].kinetic_mol)
    rid = list(range(64))
    rid[1], rid[7], rid[63] = 7, 1, 1000
    other, _, _ = _rigid_gas(dev, 3, 50, rid)
    same = [c for c in range(64) if c not in (1, 7, 63)]
    assert torch.equal(other[:, same], runs[0][0][:, same])
    assert torch.equal(other[:, 1], runs[0][0][:, 7]) and torch.equal(other[:, 7], runs[0][0][:, 1])   # a replica, wherever it sits
    assert not torch.equal(other[:, 63], runs[0][0][:, 63])                                            # another id, another path


# ---- whole NPT steps of rigid waters on ANI-2x ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def water(dev):
    """ANI-2x x 8 on the water box, its masses, the rigid-water constraints and the reference's view of them."""
    from torchani_amd.md import hydrogen_constraints

    model, sp, x, cell, _ = _ani_case("water_pbc_ani2x", dev)
    pbc = (True, True, True)
    mass = MASS_BY_INDEX[sp.cpu().numpy()].astype(np.float32).astype(np.float64)
    bc = hydrogen_constraints(sp, x, cell, pbc, rigid_water=True, hydrogen=0, oxygen=3)
    assert int(bc.counts().sum()) == 30
    cons = cref.Constraints(bc.pairs.numpy(), bc.lengths.numpy(), np.ones(sp.shape, dtype=bool), mass)
    return model, sp, x, cell, pbc, mass, bc, cons


PAR = dict(dt=0.5, temperature=300.0, friction=0.05, replica_ids=torch.tensor([11]), seed=SEED, pressure=2000.0,
           compressibility=4.57e-5, barostat_time=200.0)


def _dynamics(water, dev):
    from torchani_amd.md import BatchedDynamics

    model, sp, x, cell, pbc, mass, bc, _ = water
    return BatchedDynamics(model, sp, x, cell, pbc, masses=torch.from_numpy(mass).to(dev), constraints=bc,
                           constraint_tolerance=TOL, barostat_scaling="molecular", **PAR)


def _reference_step(bd, mass, cons, step):
    """One step of ``bd`` in lock-step with the reference, which is fed the device's forces and virial and forms the group
    terms itself from the state before the step: returns (x, v, kinetic, cell, mu, K_mol, G) after it."""
    active = np.ones(mass.shape, dtype=bool)
    Cn, A = active.shape
    rid = bd._replica_ids.cpu().numpy()
    x0 = bd.coordinates.double().cpu().numpy() + bd.coordinates_lo.double().cpu().numpy()
    v0, f0 = bd.velocities.double().cpu().numpy(), bd.forces.double().cpu().numpy()
    K0, W0 = bd.kinetic_energies().cpu().numpy(), bd._model_eval.virial.cpu().numpy().reshape(1, 3, 3)
    Km0, G0 = gref.group_terms(x0, v0, f0, active, mass, cons)
    cell0 = bd.cell64.cpu().numpy().reshape(1, 3, 3)
    kT = (bd.temperature.cpu().numpy() * np.float32(ref.KB_HARTREE)).astype(np.float64)   # (the device forms k_B T in fp32)
    fr = bd.friction.double().cpu().numpy()
    p0 = bd.pressure.cpu().numpy() / BAR
    bd.step()
    x1, vm = cref.drift(x0, v0, f0, active, mass, PAR["dt"], cons, True, kT, fr, ref.noise(SEED, step, Cn, A, rid))
    x2, v2, cell1, _, _, mu = gref.barostat_groups(x1, vm, cell0, K0, Km0, W0, G0, active, mass, cons, kT, p0,
                                                   PAR["compressibility"] * BAR, PAR["barostat_time"], PAR["dt"],
                                                   bref.barostat_noise(SEED, step, Cn, rid))
    f1 = bd.forces.double().cpu().numpy()
    v3, ke = cref.kick(x2, v2, f1, active, mass, PAR["dt"], cons)
    Km3, G3 = gref.group_terms(x2, v3, f1, active, mass, cons)
    return x2, v3, ke, cell1, mu, Km3, G3


def _assert_step(bd, want):
    x2, v3, ke, cell1, mu, Km3, G3 = want
    _assert_close(bd.coordinates.double().cpu().numpy(), bd.velocities.double().cpu().numpy(), bd.kinetic_energies().cpu().numpy(),
                  x2, v3, ke)
    assert abs(bd._kinetic_mol.item() / Km3[0] - 1.0) <= 1e-6   # (the kinetic energies' gate)
    assert abs(bd.barostat_scale.item() / mu[0] - 1.0) <= 1e-6
    assert torch.equal(bd.cell, bd.cell64.float())
    got = bd.cell64.cpu().numpy().reshape(1, 3, 3)
    return np.abs(got - cell1).max() / np.abs(cell1).max()


def test_npt_steps_of_rigid_waters_on_ani2x_match_reference(dev, water):
    """Three steps of constrained drift, barostat_groups, evaluation, constrained kick, group_terms on ANI-2x x 8 with the gates
    of test_langevin_steps_on_ani2x_match_reference (coordinates to 4 fp32 ulp, velocities to 1e-5 of the largest, kinetic
    energies to 1e-6); the cell within ten times the difference measured (CELL_DIFF_MEASURED); the constraint residuals of the
    pair within 1e-10 after the third step.  The first move runs on a stale kinetic energy (``set_temperature``), which the
    step refreshes together with the group terms."""
    model, sp, x, cell, pbc, mass, bc, cons = water
    bd = _dynamics(water, dev)
    bd.set_temperature(300.0)
    worst, moves = 0.0, []
    for s in range(3):
        assert bd.steps_done == s
        want = _reference_step(bd, mass, cons, s)
        worst = max(worst, _assert_step(bd, want))
        moves.append(float(want[4][0]) - 1.0)
    pair = bd.coordinates.double().cpu().numpy() + bd.coordinates_lo.double().cpu().numpy()
    res = cref.residuals(pair, cons)
    print(f"md barostat groups NPT steps on water_pbc_ani2x: mu - 1 = {', '.join(f'{m:.3e}' for m in moves)}, largest |cell64 - "
          f"cell_ref| / max |cell_ref| = {worst:.2e}, constraint residual {res:.2e}, P_mol = {bd.pressures().item():.4e} bar, "
          f"K_mol / K = {bd._kinetic_mol.item() / bd.kinetic_energies().item():.3f}, V = {bd.volumes().item():.3f} A^3")
    assert min(abs(m) for m in moves) > 1e-5   # (moves that a wrong ordering would show in)
    assert worst <= 10.0 * CELL_DIFF_MEASURED
    assert res <= 1e-10
    bd.raise_on_unconverged_constraints()
    dof = 3 * 30 - 30
    assert np.allclose(bd.temperatures().item(), 2.0 * bd.kinetic_energies().item() / (dof * ref.KB_HARTREE), rtol=1e-12)
    # the forces and the virial held are the model's at the coordinates and the cell held
    out = model.energies_and_forces(sp, bd.coordinates, bd.cell, bd.pbc, stress=True)
    assert (out.forces - bd.forces).abs().max().item() <= 1e-5 * max(1.0, out.forces.abs().max().item())
    assert (out.virial - bd._model_eval.virial).abs().max().item() <= 1e-5 * max(1.0, out.virial.abs().max().item())


def test_stale_kinetic_energy_and_group_terms_are_refreshed_before_the_move(dev, water):
    """Velocities set between two steps: the next move uses the kinetic energies and the internal virial of the state it
    starts from, as the reference that recomputes them does."""
    model, sp, x, cell, pbc, mass, bc, cons = water
    bd = _dynamics(water, dev)
    bd.set_temperature(300.0)
    bd.step()
    before = bd._kinetic_mol.item()
    bd.set_velocities(1.5 * bd.velocities)
    want = _reference_step(bd, mass, cons, 1)
    diff = _assert_step(bd, want)
    assert diff <= 10.0 * CELL_DIFF_MEASURED
    # 2.25 times the centre-of-mass kinetic energy moves mu by (beta_T / tau_p) dt 2 (1.25 K_mol) / (9 V), far above the gate
    V = bd.volumes().item()
    shift = PAR["compressibility"] * BAR / PAR["barostat_time"] * PAR["dt"] * 2.0 * 1.25 * before / (9.0 * V)
    assert shift > 1e3 * 10.0 * CELL_DIFF_MEASURED


# ---- pressures() ----------------------------------------------------------------------------------------------------------------

def _scale_groups(x, s, mass, cons):
    """Group centres scaled by s, the groups translated rigidly; free atoms scaled."""
    active = np.ones(mass.shape, dtype=bool)
    clusters, free = gref.scaling_groups(active, mass, cons)
    out = np.where(free[..., None], s * x, x)
    for mol, atoms, m in clusters:
        out[mol[:, None], atoms] = x[mol[:, None], atoms] + ((s - 1.0) * gref.centres(x, m, atoms, mol))[:, None]
    return out


def test_molecular_pressure_matches_finite_differences_under_rigid_group_scaling(dev, water):
    """pressures() at rest (K_mol = 0: the configurational part, -(tr W + G) / (3 V)) against central differences of the energy
    in the volume with the cell and the waters' centres of mass scaled and the waters translated rigidly.  h and the gate are
    derived as in test_pressures_match_finite_differences_on_water (energy noise dE of the fp32 atomic energies, coordinates
    and cell; h = (dE / (2 |tr W + G|))^(1/3) capped at 0.02; gate = |FD(2h) - FD(h)| / 3 + 1.5 dE / (h V)).  The atomic-scaling
    pressure -tr W / (3 V) of the same state must be more than ten gates away: a missing G cannot pass."""
    from torchani_amd.geomopt import ModelEvaluator

    model, sp, x, cell, pbc, mass, bc, cons = water
    bd = _dynamics(water, dev)
    out = model.energies_and_forces(sp, x, cell, pbc)
    N = 30
    W, G, V = bd._model_eval.virial.cpu().numpy(), bd._virial_mol.item(), bd.volumes().item()
    dE = (8.0 * 2.0 ** -24 * np.sqrt(N) * float(out.atomic_energies.abs().max())
          + 2.0 ** -24 * float(x.abs().max()) * float(bd.forces.double().norm()) + 2.0 ** -24 * float(np.linalg.norm(W)))
    h = min(0.02, (dE / (2.0 * abs(np.trace(W) + G))) ** (1.0 / 3.0))
    xn = x.double().cpu().numpy()

    def fd(step):
        e = []
        for s in ((1.0 + step) ** (1.0 / 3.0), (1.0 - step) ** (1.0 / 3.0)):
            xs = torch.from_numpy(_scale_groups(xn, s, mass, cons)).float().to(dev).contiguous()
            e.append(ModelEvaluator(model, sp, (cell.double() * s).float(), pbc)(xs)[0].item())
        return -(e[0] - e[1]) / (2.0 * step * V)

    fd1, fd2 = fd(h), fd(2.0 * h)
    gate = abs(fd2 - fd1) / 3.0 + 1.5 * dE / (h * V)
    p = bd.pressures().item()
    p_atomic = -np.trace(W) / (3.0 * V) * BAR
    fd_atomic = _fd_pressure(lambda xs, cs: ModelEvaluator(model, sp, cs, pbc)(xs.contiguous())[0].item(), x, cell, h) * BAR
    print(f"md barostat groups pressures(): P_mol = {p:.6e} bar, finite difference under rigid-group scaling {fd1 * BAR:.6e} bar at "
          f"h = {h:.2e} ({fd2 * BAR:.6e} at 2h), |dP| = {abs(p - fd1 * BAR):.2e} bar, gate {gate * BAR:.2e} bar (energy noise "
          f"{dE:.1e} Ha); atomic scaling: P = {p_atomic:.6e} bar (finite difference {fd_atomic:.6e}), G = {G:.4e} Ha")
    assert bd.kinetic_energies().item() == 0.0 and bd._kinetic_mol.item() == 0.0
    assert abs(p - (-(np.trace(W) + G) / (3.0 * V)) * BAR) <= 1e-12 * abs(p)
    Gref = gref.group_terms(xn, np.zeros_like(xn), bd.forces.double().cpu().numpy(), np.ones((1, N), dtype=bool), mass, cons)[1]
    assert abs(G - Gref[0]) <= 4e-14 * float(bd.forces.double().abs().sum())   # (the bound of the move test)
    assert abs(p / BAR - fd1) <= gate
    assert gate <= 0.05 * abs(p / BAR)   # (a comparison that says something)
    assert abs(p_atomic - p) > 10.0 * gate * BAR
    # with kinetic energy: the centre-of-mass term on top
    bd.set_temperature(300.0)
    Km = gref.group_terms(xn, bd.velocities.double().cpu().numpy(), np.zeros_like(xn), np.ones((1, N), dtype=bool), mass, cons)[0][0]
    assert abs(bd.pressures().item() - (p + 2.0 * Km / (3.0 * V) * BAR)) <= 1e-6 * abs(p)


# ---- behaviour of the Python layer ------------------------------------------------------------------------------------------

def test_molecular_npt_step_does_not_synchronize(dev, water):
    bd = _dynamics(water, dev)
    bd.set_temperature(300.0)
    for _ in range(3):
        bd.step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            bd.step()
        bd.set_velocities(0.5 * bd.velocities)   # (stale kinetic energies and group terms are refreshed without a host read)
        bd.pressures()
        bd.step()
        bd.volumes(), bd.pressures(), bd.kinetic_energies(), bd.temperatures()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bd.steps_done == 7
    bd.run(3, check_every=2)   # (reads the constraints' iteration counts)
    assert bd.steps_done == 10 and int(bd.constraint_iterations.max()) < 64


def test_barostat_scaling_argument_errors(dev, water):
    from torchani_amd.md import BatchedDynamics

    model, sp, x, cell, pbc, mass, bc, _ = water
    m = torch.from_numpy(mass).to(dev)
    ok = dict(masses=m, temperature=300.0, pressure=1.0)
    with pytest.raises(ValueError, match="barostat_scaling"):
        BatchedDynamics(model, sp, x, cell, pbc, barostat_scaling="rigid", **ok)
    with pytest.raises(ValueError, match="pressure="):
        BatchedDynamics(model, sp, x, cell, pbc, masses=m, temperature=300.0, constraints=bc, barostat_scaling="molecular")
    fixed = torch.zeros(sp.shape, dtype=torch.bool, device=dev)
    fixed[0, 2] = True
    with pytest.raises(ValueError, match="fixed atoms"):
        BatchedDynamics(model, sp, x, cell, pbc, fixed=fixed, constraints=bc, barostat_scaling="molecular", **ok)
    with pytest.raises(ValueError, match='constraints.*barostat_scaling="molecular"'):
        BatchedDynamics(model, sp, x, cell, pbc, constraints=bc, **ok)
    # every other restriction of the barostat stays
    with pytest.raises(ValueError, match="Langevin"):
        BatchedDynamics(model, sp, x, cell, pbc, masses=m, pressure=1.0, constraints=bc, barostat_scaling="molecular")
    with pytest.raises(ValueError, match="periodic in all three"):
        BatchedDynamics(model, sp, x, cell, (True, True, False), constraints=bc, barostat_scaling="molecular", **ok)
    # molecular scaling without constraints: every atom is a group of its own, the pressure is the atomic one
    free = BatchedDynamics(model, sp, x, cell, pbc, barostat_scaling="molecular", **ok)
    atomic = BatchedDynamics(model, sp, x, cell, pbc, **ok)
    assert free._virial_mol.item() == 0.0 and free.pressures().item() == atomic.pressures().item()
