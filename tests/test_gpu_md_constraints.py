"""Bond-length constraints of the on-device MD integrator (SHAKE / RATTLE, csrc/md.hip: k_md_constrain) on the MI355X against
the fp64 reference of tests/_md_constraints_ref.py: the kernels with the forces given, the two-float residual far from the origin,
bit-identity without constraints, replicas, whole steps on ANI-2x and on a Lennard-Jones potential, the report of a cluster that
did not converge, and ``hydrogen_constraints``.

Lock-step comparisons run at constraint_tolerance = 1e-10 and use the gates of test_gpu_md_device.py (coordinates to 4 fp32 ulp of
the largest, velocities to 1e-5 of the largest, kinetic energies to 1e-6 relative)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _md_constraints_ref as cref
import _md_ref as ref
from test_gpu_md_device import MASS_BY_INDEX, SEED, STEP0, Kernels, _ani_case, _assert_close, _stream

pytestmark = pytest.mark.gpu

TOL = 1e-10


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from torchani_amd import _lib

    _lib.lib()
    return torch.device("cuda:0")


# ---- states ----------------------------------------------------------------------------------------------------------------

# case 1, per molecule: (atoms, constraints as pairs of atoms)
TRIANGLE = lambda a, b, c: [(a, b), (b, c), (c, a)]   # noqa: E731
CASE1 = [
    [(0, 1)], TRIANGLE(2, 3, 4), [(5, 6)],                       # molecule 0: atom 5 is fixed, an anchor
    [(10, 11), (10, 12), (10, 13), (10, 14)],                    # a 5-atom star
    [(20, 21), (21, 22), (22, 23)], [(63, 64)],                  # a 4-atom chain; a cluster across the wave boundary
], [
    [(0, 1)], [(31, 30)], [(40, 41), (41, 42), (42, 43)], TRIANGLE(50, 52, 51), [(59, 60)],   # molecule 1: padding from 61 on
], [
    [(63, 64)], [(3, 1), (3, 2), (3, 4), (3, 5)], [(68, 69), (67, 68)], [(10, 40)],   # molecule 2: atom 69 is fixed
]


def _pad_pairs(per_molecule):
    K = max(1, max(len(p) for p in per_molecule))
    out = np.full((len(per_molecule), K, 2), -1, dtype=np.int64)
    for c, p in enumerate(per_molecule):
        if p:
            out[c, :len(p)] = p
    return out


def _state(Cn, A, clusters, padding, fixed, seed=11):
    """Random fp32 positions, velocities, three force sets and masses; the atoms of every cluster sit about 1 A from the
    cluster's first atom.  Returns x, v, forces, mass, species (-1: padding), fixed, pairs, lengths (of the fp32 positions)."""
    rs = np.random.RandomState(seed)
    r32 = lambda a: a.astype(np.float32).astype(np.float64)   # noqa: E731
    x, v = rs.uniform(-20.0, 20.0, (Cn, A, 3)), r32(rs.normal(0.0, 0.01, (Cn, A, 3)))
    forces = [r32(rs.normal(0.0, 0.05, (Cn, A, 3))) for _ in range(3)]
    mass = r32(MASS_BY_INDEX[rs.randint(0, 7, (Cn, A))])
    species = np.zeros((Cn, A), dtype=np.int64)
    fx = np.zeros((Cn, A), dtype=bool)
    for c, i in padding:
        species[c, i] = -1
    for c, i in fixed:
        fx[c, i] = True
    for c, mol in enumerate(clusters):
        for bonds in mol:
            atoms = sorted({i for b in bonds for i in b})
            for i in atoms[1:]:
                d = rs.normal(size=3)
                x[c, i] = x[c, atoms[0]] + d / np.linalg.norm(d) * rs.uniform(0.9, 1.5)
    x = r32(x)
    v[(species < 0) | fx] = 0.0
    pairs = _pad_pairs([[b for bonds in mol for b in bonds] for mol in clusters])
    at = np.arange(Cn)[:, None]
    lengths = np.linalg.norm(x[at, np.maximum(pairs[..., 0], 0)] - x[at, np.maximum(pairs[..., 1], 0)], axis=-1)
    return x, v, forces, mass, species, fx, pairs, lengths


def _case(which):
    if which == 1:
        return _state(3, 70, CASE1, [(1, i) for i in range(61, 70)], [(0, 5), (2, 69)])
    # case 2: 150 dimers per molecule, (1, 2) ... (255, 256) ... (297, 298) and (299, 0); atom 5 of molecule 0 is fixed
    dimers = [[(i, (i + 1) % 300)] for i in range(1, 300, 2)]
    return _state(2, 300, [dimers, dimers], [], [(0, 5)])


class ConstrainedKernels(Kernels):
    """The C ABI of a step with constraints: anihip_md_drift + anihip_md_constrain_drift, anihip_md_constrain_kick +
    anihip_md_kick, on cluster tables from md.build_constraint_clusters."""

    def __init__(self, dev, x, v, species, fixed, mass, pairs, lengths, dt, tol=TOL, max_it=64, **kw):
        from torchani_amd import md

        active = (species >= 0) & ~fixed
        super().__init__(dev, x, v, active, mass, dt, **kw)
        cl = md.build_constraint_clusters(torch.from_numpy(species), torch.from_numpy(pairs), torch.from_numpy(lengths),
                                          torch.from_numpy(fixed), self.inv_mass.cpu())
        self.active[cl.owned.to(dev)] = self._lib.MD_ATOM_CLUSTER
        self.tables = [t.to(dev).contiguous() for t in (cl.atoms, cl.count, cl.bonds, cl.d2, cl.w)]
        self.iterations = torch.zeros((cl.atoms.shape[0], 2), dtype=torch.int32, device=dev)
        self.Q = self._lib.MdClusters(cl.atoms.shape[0], *(t.data_ptr() for t in self.tables), self.iterations.data_ptr(),
                                      tol, max_it, int(cl.count[:, 0].max()), int(cl.count[:, 1].max()), 0)

    def drift(self, f, step):
        super().drift(f, step)
        self._lib.check(self.lib.anihip_md_constrain_drift(
            _stream(), C.byref(self.P), C.byref(self.Q), self._ptr(self.kT), self._ptr(self.friction), self._ptr(self.rid),
            self.x.data_ptr(), self.lo.data_ptr(), self.v.data_ptr(), self._f.data_ptr()))

    def kick(self, f):
        self._f = self.f32(f)
        self._lib.check(self.lib.anihip_md_constrain_kick(
            _stream(), C.byref(self.P), C.byref(self.Q), self.x.data_ptr(), self.lo.data_ptr(), self.v.data_ptr(),
            self._f.data_ptr()))
        super().kick(f)

    def pair(self):
        return self.x.double().cpu().numpy() + self.lo.double().cpu().numpy()


def _check_residuals(x_pair, v, cons, tol, label):
    """Positions from the two-float pair: | |r| / d - 1 | <= 2 tol.  Velocities: |r_hat . dv| within 4 fp32 ulp of the cluster's
    largest |v| component (two roundings of at most half an ulp per component, projected on a unit vector, give 1.8 ulp)."""
    res_x = cref.residuals(x_pair, cons)
    worst_v = 0.0
    for rv, vmax in cref.velocity_residuals(x_pair, v, cons):
        ulp = np.spacing(vmax.astype(np.float32)).astype(np.float64)
        worst_v = max(worst_v, (rv / ulp[:, None]).max())
        assert (rv <= 4.0 * ulp[:, None]).all()
    print(f"md constraints {label}: position residual {res_x:.2e} (gate {2 * tol:.0e}), velocity residual {worst_v:.2f} fp32 ulp "
          f"of the cluster's largest |v| (gate 4)")
    assert res_x <= 2.0 * tol


# ---- the kernels with the forces given -------------------------------------------------------------------------------------

@pytest.mark.parametrize("langevin", [False, True], ids=["nve", "langevin"])
@pytest.mark.parametrize("which", [1, 2], ids=["C3_A70", "C2_A300"])
def test_constrained_drift_and_kick_match_reference(dev, which, langevin):
    x, v, forces, mass, species, fixed, pairs, lengths = _case(which)
    Cn, A = species.shape
    active = (species >= 0) & ~fixed
    dt = 0.5
    rid = [5, 0, 3][:Cn]
    kT = ref.KB_HARTREE * np.array([250.0, 300.0, 350.0])[:Cn]
    friction = np.array([0.002, 0.5, 0.01])[:Cn]
    k = ConstrainedKernels(dev, x, v, species, fixed, mass, pairs, lengths, dt, langevin=langevin,
                           kT=kT if langevin else None, friction=friction if langevin else None, rid=rid)
    cons = cref.Constraints(pairs, lengths, active, mass)
    assert len(cons.clusters) == k.Q.n_clusters == (15 if which == 1 else 300)
    for s in range(2):
        x0, v0 = k.pair(), k.v.double().cpu().numpy()
        k.drift(forces[s], STEP0 + s)
        k.kick(forces[s + 1])
        xi = ref.noise(SEED, STEP0 + s, Cn, A, rid)
        x1, vm = cref.drift(x0, v0, forces[s], active, mass, dt, cons, langevin, kT, friction, xi)
        v1, ke = cref.kick(x1, vm, forces[s + 1], active, mass, dt, cons)
        gx, gv = k.x.cpu().numpy(), k.v.cpu().numpy()
        _assert_close(gx.astype(np.float64), gv.astype(np.float64), k.kinetic.cpu().numpy(), x1, v1, ke)
        pair = k.pair()
        _check_residuals(pair, gv.astype(np.float64), cons, TOL, f"case {which} {'langevin' if langevin else 'nve'} step {s}")
        # the pair is normalized and closer to the reference than fp32 can hold; inactive atoms never move
        assert np.array_equal(pair.astype(np.float32), gx)
        assert np.abs(pair - x1)[active].max() <= 0.25 * np.spacing(np.float32(np.abs(x1).max()))
        assert np.array_equal(gx[~active], x[~active].astype(np.float32)) and np.all(gv[~active] == 0.0)
        it = k.iterations.cpu().numpy()
        print(f"md constraints case {which}: iterations, positions up to {it[:, 0].max()}, velocities up to {it[:, 1].max()}")
        assert it.max() < 64 and it[:, 0].min() >= 1


def test_projection_alone_matches_reference(dev):
    x, v, forces, mass, species, fixed, pairs, lengths = _case(1)
    active = (species >= 0) & ~fixed
    k = ConstrainedKernels(dev, x, v, species, fixed, mass, pairs, lengths, 0.5)
    k._lib.check(k.lib.anihip_md_project_velocities(_stream(), C.byref(k.P), C.byref(k.Q), k.x.data_ptr(), k.lo.data_ptr(),
                                                    k.v.data_ptr()))
    cons = cref.Constraints(pairs, lengths, active, mass)
    want, got = cref.project_v(x, v, cons), k.v.cpu().numpy()
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
    assert np.array_equal(got[~cons.owned], v[~cons.owned].astype(np.float32))   # atoms outside clusters are not touched
    assert np.array_equal(k.x.cpu().numpy(), x.astype(np.float32))
    _check_residuals(x, got.astype(np.float64), cons, TOL, "projection alone")


def test_two_float_pair_holds_the_bond_far_from_the_origin(dev):
    """The dimers of case 2 shifted to |x| = 200 A, where one fp32 ulp is 1.5e-5 A, 100 NVE steps with forces given: the bond
    lengths of coordinates + coordinates_lo stay within 2e-10 relative; those of ``coordinates`` alone cannot."""
    x, v, forces, mass, species, fixed, pairs, lengths = _case(2)
    x = (x + np.array([200.0, -200.0, 200.0])).astype(np.float32).astype(np.float64)
    at = np.arange(2)[:, None]
    lengths = np.linalg.norm(x[at, pairs[..., 0]] - x[at, pairs[..., 1]], axis=-1)
    k = ConstrainedKernels(dev, x, v, species, fixed, mass, pairs, lengths, 0.5)
    cons = cref.Constraints(pairs, lengths, (species >= 0) & ~fixed, mass)
    for s in range(100):
        k.drift(0.2 * forces[s % 3], s)
        k.kick(0.2 * forces[(s + 1) % 3])
    res_pair, res_hi = cref.residuals(k.pair(), cons), cref.residuals(k.x.double().cpu().numpy(), cons)
    print(f"md constraints at |x| = 200 A after 100 steps: bond residual of the two-float pair {res_pair:.2e}, of coordinates "
          f"alone {res_hi:.2e}; iterations up to {k.iterations.max().item()}")
    assert res_pair <= 2e-10
    assert res_hi > 1e-7   # (what the residual array is for)
    assert np.abs(k.pair() - x).max() > 0.05   # the atoms did move


# ---- BatchedDynamics with the forces given by a test model -----------------------------------------------------------------

class Springs:
    """A stand-in model: every atom on a spring to where it started (elementwise torch, deterministic), through the interface
    ModelEvaluator asks of an ANI model."""

    class Out:
        pass

    def __init__(self, x0, k=0.05):
        self.x0, self.k = x0.clone(), k

    def energies_and_forces(self, species, coordinates, cell=None, pbc=None, check_overflow=False):
        d = coordinates - self.x0
        out = self.Out()
        out.energies = 0.5 * self.k * d.double().pow(2).sum(dim=(1, 2))
        out.forces = -self.k * d
        return out

    def _overflow_impossible(self, *a):
        return True

    def _raise_on_pair_overflow(self):
        pass


def _dynamics(dev, state, rows=None, pad=0, **kw):
    """BatchedDynamics on the Springs model for the molecules ``rows`` of a state, padded by ``pad`` atoms."""
    from torchani_amd.md import BatchedDynamics

    x, v, forces, mass, species, fixed, pairs, lengths = state
    rows = list(range(species.shape[0])) if rows is None else rows
    padded = lambda a, fill: np.concatenate([a[rows], np.full((len(rows), pad) + a.shape[2:], fill, dtype=a.dtype)], axis=1)  # noqa: E731
    xd = torch.from_numpy(padded(x, 0.0).astype(np.float32)).to(dev)
    bd = BatchedDynamics(Springs(xd), torch.from_numpy(padded(species, -1)).to(dev), xd, dt=0.5,
                         masses=torch.from_numpy(padded(mass, 1.0).astype(np.float32)).to(dev),
                         fixed=torch.from_numpy(padded(fixed, False)).to(dev), seed=SEED, **kw)
    bd.set_velocities(torch.from_numpy(padded(v, 0.0).astype(np.float32)).to(dev))
    return bd


def test_no_constraints_is_bit_identical(dev):
    from torchani_amd.md import BondConstraints

    state = _case(1)
    kw = dict(temperature=300.0, friction=0.01, replica_ids=torch.tensor([5, 0, 3]))
    runs = []
    for extra in ({}, dict(constraints=None, constraint_tolerance=1e-10, constraint_max_iterations=8),
                  dict(constraints=BondConstraints(torch.full((3, 4, 2), -1, dtype=torch.int64)))):
        bd = _dynamics(dev, state, **kw, **extra)
        bd.run(5)
        assert bd._clusters is None and int(bd._active.max()) == 1
        runs.append((bd.coordinates.clone(), bd.coordinates_lo.clone(), bd.velocities.clone(), bd.kinetic_energies()))
    for other in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], other))
    # and the same state with constraints is another trajectory (the feature is on when asked for)
    bd = _dynamics(dev, state, constraints=BondConstraints(torch.from_numpy(state[6])), **kw)
    bd.run(5)
    assert not torch.equal(bd.coordinates, runs[0][0])


def test_constrained_replicas_follow_their_ids(dev):
    from torchani_amd.md import BondConstraints

    state = _case(1)
    pairs, lengths = state[6], state[7]

    def run(rows, pad, rid):
        bc = BondConstraints(torch.from_numpy(pairs[rows]), torch.from_numpy(lengths[rows]))
        bd = _dynamics(dev, state, rows, pad, temperature=300.0, friction=0.01, replica_ids=torch.tensor(rid), constraints=bc,
                       constraint_tolerance=TOL)
        bd.run(4)
        return bd

    base, perm = run([0, 1, 2], 0, [5, 0, 3]), [2, 0]
    other = run(perm, 7, [3, 5])
    for name in ("coordinates", "coordinates_lo", "velocities"):
        assert torch.equal(getattr(other, name)[:, :70], getattr(base, name)[perm]), name
    assert torch.equal(other.kinetic_energies(), base.kinetic_energies()[perm])
    assert torch.equal(base.n_constraints.cpu(), torch.tensor([13, 9, 8]))


def test_given_lengths_are_imposed_at_construction_and_checked(dev):
    from torchani_amd.md import BondConstraints

    state = _case(1)
    x, pairs, lengths = state[0], state[6], state[7]
    active = (state[4] >= 0) & ~state[5]
    want = lengths * np.where(np.arange(lengths.shape[1]) % 2 == 0, 1.03, 0.96)   # 3-4 % off the geometry
    bd = _dynamics(dev, state, constraints=BondConstraints(torch.from_numpy(pairs), torch.from_numpy(want)),
                   constraint_tolerance=TOL)
    cons = cref.Constraints(pairs, want, active, state[3])
    pair = bd.coordinates.double().cpu().numpy() + bd.coordinates_lo.double().cpu().numpy()
    x_ref, _ = cref.move(x, np.zeros_like(x), 1.0, cons)
    print(f"md constraints, lengths imposed at construction: residual {cref.residuals(pair, cons):.2e}, largest move "
          f"{np.abs(pair - x).max():.3f} A, |x - x_ref| {np.abs(pair - x_ref).max():.2e}")
    assert cref.residuals(pair, cons) <= 2 * TOL
    assert np.abs(pair - x_ref).max() <= 1e-8
    assert np.array_equal(pair[~cons.owned], x[~cons.owned])
    want[2, 0] *= 1.2
    with pytest.raises(ValueError, match="more than 10 % off"):
        _dynamics(dev, state, constraints=BondConstraints(torch.from_numpy(pairs), torch.from_numpy(want)))


def test_unconverged_cluster_is_reported(dev):
    """One sweep is not enough for the coupled constraints of the 4-atom chain: the iteration count the kernel stores reaches
    max_iterations, and run() raises at its status read and names the cluster.  (A count, not a fault: the kernel ran as ever.)"""
    from torchani_amd.md import BondConstraints

    state = _case(1)
    chain = np.full((3, 3, 2), -1, dtype=np.int64)
    chain[0] = [(20, 21), (21, 22), (22, 23)]
    bd = _dynamics(dev, state, constraints=BondConstraints(torch.from_numpy(chain)), constraint_max_iterations=1)
    with pytest.raises(RuntimeError, match=r"constraint cluster 0 \(molecule 0, atoms \[20, 21, 22, 23\]\) did not converge"):
        bd.run(3, check_every=3)
    assert bd.steps_done == 3
    ok = _dynamics(dev, state, constraints=BondConstraints(torch.from_numpy(chain)))
    ok.run(3, check_every=3)
    assert 1 < int(ok.constraint_iterations.max()) < 64


def test_constrained_step_does_not_synchronize(dev):
    from torchani_amd.md import BondConstraints

    state = _case(1)
    bd = _dynamics(dev, state, temperature=300.0, constraints=BondConstraints(torch.from_numpy(state[6])))
    bd.step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            bd.step()
        bd.kinetic_energies(), bd.temperatures()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bd.steps_done == 4


# ---- whole steps on models --------------------------------------------------------------------------------------------------

def _lock_step(bd, cons, active, mass, dt, n_steps, langevin, kT=None, fr=None, rid=None, seed=SEED):
    """n_steps of bd against the reference fed the device's state and forces at every step; returns the last kinetic energies."""
    Cn, A = active.shape
    for s in range(n_steps):
        x0 = bd.coordinates.double().cpu().numpy() + bd.coordinates_lo.double().cpu().numpy()
        v0, f0 = bd.velocities.double().cpu().numpy(), bd.forces.double().cpu().numpy()
        bd.step()
        xi = ref.noise(seed, s, Cn, A, rid) if langevin else None
        x1, vm = cref.drift(x0, v0, f0, active, mass, dt, cons, langevin, kT, fr, xi)
        v1, ke = cref.kick(x1, vm, bd.forces.double().cpu().numpy(), active, mass, dt, cons)
        _assert_close(bd.coordinates.double().cpu().numpy(), bd.velocities.double().cpu().numpy(),
                      bd.kinetic_energies().cpu().numpy(), x1, v1, ke)
    pair = bd.coordinates.double().cpu().numpy() + bd.coordinates_lo.double().cpu().numpy()
    _check_residuals(pair, bd.velocities.double().cpu().numpy(), cons, TOL, f"{type(bd.model).__name__} after {n_steps} steps")
    bd.raise_on_unconverged_constraints()
    return ke


@pytest.mark.parametrize("base", ["water_pbc_ani2x", "rand_batch_ani2x"])
def test_constrained_langevin_steps_on_ani2x_match_reference(dev, base):
    from torchani_amd.md import BatchedDynamics, hydrogen_constraints

    model, sp, x, cell, pbc = _ani_case(base, dev)
    Cn, A = sp.shape
    spn = sp.cpu().numpy()
    mass = np.where(spn >= 0, MASS_BY_INDEX[np.clip(spn, 0, 6)], 1.0).astype(np.float32).astype(np.float64)
    bc = hydrogen_constraints(sp, x, cell, pbc, rigid_water=(base == "water_pbc_ani2x"), hydrogen=0, oxygen=3)
    assert int(bc.counts().sum()) == (30 if base == "water_pbc_ani2x" else 6)
    fixed = np.zeros((Cn, A), dtype=bool)
    fixed[Cn - 1, 0] = True
    active = (spn >= 0) & ~fixed
    T = 250.0 + 40.0 * np.arange(Cn)
    friction = np.linspace(0.002, 0.2, Cn)
    rid = list(np.random.RandomState(1).permutation(Cn) + 3)
    dt = 0.5
    bd = BatchedDynamics(model, sp, x, cell, pbc, dt=dt, masses=torch.from_numpy(mass).to(dev), temperature=torch.from_numpy(T),
                         friction=torch.from_numpy(friction), fixed=torch.from_numpy(fixed).to(dev), replica_ids=torch.tensor(rid),
                         seed=SEED, constraints=bc, constraint_tolerance=TOL)
    xn = x.double().cpu().numpy()
    at = np.arange(Cn)[:, None]
    pairs = bc.pairs.numpy()
    lengths = np.linalg.norm(xn[at, np.maximum(pairs[..., 0], 0)] - xn[at, np.maximum(pairs[..., 1], 0)], axis=-1)
    assert np.allclose(lengths[pairs[..., 0] >= 0], bc.lengths.numpy()[pairs[..., 0] >= 0], rtol=1e-12)
    cons = cref.Constraints(pairs, bc.lengths.numpy(), active, mass)
    # Maxwell-Boltzmann velocities, drift removed, projected: tangent to the constraints from the start
    bd.set_temperature(torch.from_numpy(T))
    for rv, vmax in cref.velocity_residuals(xn, bd.velocities.double().cpu().numpy(), cons):
        assert (rv <= 4.0 * np.spacing(vmax.astype(np.float32))[:, None]).all()
    kT = ref.KB_HARTREE * T.astype(np.float32).astype(np.float64)
    ke = _lock_step(bd, cons, active, mass, dt, 3, True, kT, friction.astype(np.float32).astype(np.float64), rid)
    dof = 3 * active.sum(axis=1) - cons.per_molecule
    assert np.allclose(bd.temperatures().cpu().numpy(), 2.0 * ke / (dof * ref.KB_HARTREE), rtol=1e-6)
    assert np.array_equal(bd.coordinates.cpu().numpy()[~active], x.cpu().numpy()[~active])


def test_rigid_dimers_in_a_lennard_jones_potential_match_reference(dev):
    """16 rigid dimers (bond 1.1 A) on a 2.2 A grid in a standalone Lennard-Jones potential, 20 NVE steps of 1 fs."""
    from torchani_amd.md import BatchedDynamics, BondConstraints
    from torchani_amd.potentials import LennardJones

    rs = np.random.RandomState(3)
    grid = np.stack(np.meshgrid(np.arange(4), np.arange(2), np.arange(2), indexing="ij"), -1).reshape(-1, 3) * np.array([2.2, 2.2, 3.3])
    d = rs.normal(size=(16, 3)) * np.array([0.15, 0.15, 1.0])
    x = np.stack([grid, grid + 1.1 * d / np.linalg.norm(d, axis=-1, keepdims=True)], axis=1).reshape(1, 32, 3)
    x = x.astype(np.float32).astype(np.float64)
    pairs = np.arange(32, dtype=np.int64).reshape(1, 16, 2)
    lj = LennardJones(("H",), eps=(0.002,), sigma=(1.0,)).to(dev)
    mass = np.full((1, 32), np.float64(np.float32(12.011)))
    active = np.ones((1, 32), dtype=bool)
    dt = 1.0
    bd = BatchedDynamics(lj, torch.ones((1, 32), dtype=torch.int64, device=dev), torch.from_numpy(x).to(dev), dt=dt,
                         masses=torch.from_numpy(mass).to(dev), constraints=BondConstraints(torch.from_numpy(pairs)),
                         constraint_tolerance=TOL)
    bd.set_velocities(torch.from_numpy(rs.normal(0.0, 0.004, (1, 32, 3))).to(dev))
    lengths = np.linalg.norm(x[0, pairs[0, :, 0]] - x[0, pairs[0, :, 1]], axis=-1)[None]
    cons = cref.Constraints(pairs, lengths, active, mass)
    e0 = bd.total_energies().item()
    _lock_step(bd, cons, active, mass, dt, 20, False)
    print(f"md constraints, LJ dimers: |dE_total| over 20 fs = {abs(bd.total_energies().item() - e0):.2e} Ha, KE = "
          f"{bd.kinetic_energies().item():.2e} Ha")
    assert np.allclose(bd.temperatures().item(), 2.0 * bd.kinetic_energies().item() / ((96 - 16) * ref.KB_HARTREE), rtol=1e-12)


# ---- hydrogen_constraints ----------------------------------------------------------------------------------------------------

def test_hydrogen_constraints_on_the_water_box(dev):
    from torchani_amd.md import hydrogen_constraints

    model, sp, x, cell, pbc = _ani_case("water_pbc_ani2x", dev)
    plain = hydrogen_constraints(sp, x, cell, pbc, hydrogen=0, oxygen=3)
    rigid = hydrogen_constraints(sp, x, cell, pbc, rigid_water=True, hydrogen=0, oxygen=3)
    n_water = int((sp == 3).sum())
    assert plain.counts().tolist() == [2 * n_water] and rigid.counts().tolist() == [3 * n_water]
    spn, p = sp.cpu().numpy()[0], rigid.pairs[0].numpy()
    assert (spn[p[:2 * n_water, 0]] == 3).all() and (spn[p[:2 * n_water, 1]] == 0).all() and (spn[p[2 * n_water:]] == 0).all()
    assert np.array_equal(np.sort(p[:2 * n_water, 1]), np.nonzero(spn == 0)[0])          # every hydrogen once
    assert torch.equal(rigid.pairs[:, :2 * n_water], plain.pairs)
    assert 0.9 < rigid.lengths[0, :2 * n_water].min() and rigid.lengths[0, :2 * n_water].max() < 1.0
    assert 1.4 < rigid.lengths[0, 2 * n_water:].min() and rigid.lengths[0, 2 * n_water:].max() < 1.7
    # a hydrogen moved by a cell vector is the same periodic system, but its bond's plain difference is no longer the
    # minimum-image one: the integrator would see an 8 A bond
    h = int(p[0, 1])
    wrapped = x.clone()
    wrapped[0, h] += cell[0]
    with pytest.raises(ValueError, match="unwrap the molecule"):
        hydrogen_constraints(sp, wrapped, cell, pbc, hydrogen=0, oxygen=3)


def test_hydrogen_constraints_on_small_molecules(dev):
    from torchani_amd.md import hydrogen_constraints

    t = 1.09 / np.sqrt(3.0)
    ch4 = [(6, 0, 0, 0), (1, t, t, t), (1, t, -t, -t), (1, -t, t, -t), (1, -t, -t, t)]
    nh3 = [(1, 0.94, 0.0, -0.38), (1, -0.47, 0.81, -0.38), (7, 0, 0, 0), (1, -0.47, -0.81, -0.38)]
    h2o = [(1, 0.757, 0.586, 0.0), (8, 0, 0, 0), (1, -0.757, 0.586, 0.0)]
    sp = torch.full((3, 5), -1, dtype=torch.int64)
    x = torch.zeros((3, 5, 3))
    for c, mol in enumerate((ch4, nh3, h2o)):
        sp[c, :len(mol)] = torch.tensor([a[0] for a in mol])
        x[c, :len(mol)] = torch.tensor([a[1:] for a in mol])
    sp, x = sp.to(dev), x.to(dev)
    plain, rigid = hydrogen_constraints(sp, x), hydrogen_constraints(sp, x, rigid_water=True)
    assert plain.counts().tolist() == [4, 3, 2] and rigid.counts().tolist() == [4, 3, 3]
    assert plain.pairs[0].tolist() == [[0, 1], [0, 2], [0, 3], [0, 4]]
    assert plain.pairs[1].tolist() == [[2, 0], [2, 1], [2, 3], [-1, -1]]
    assert rigid.pairs[2].tolist() == [[1, 0], [1, 2], [0, 2], [-1, -1]]
    assert rigid.lengths[2, 2].item() == pytest.approx(2 * 0.757, rel=1e-6)
    assert hydrogen_constraints(sp, x, max_bond=0.8).counts().tolist() == [0, 0, 0]
