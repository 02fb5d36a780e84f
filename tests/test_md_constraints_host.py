"""Bond-length constraints without a GPU: the host cluster builder (torchani_amd.md.build_constraint_clusters), the fp64 reference
of tests/_md_constraints_ref.py (residuals, projector, momentum), the order of the constrained scheme and equipartition under the
reference Langevin dynamics."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _md_constraints_ref as cref
import _md_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pairs(per_molecule, K=None):
    K = K or max(1, max(len(p) for p in per_molecule))
    out = torch.full((len(per_molecule), K, 2), -1, dtype=torch.int64)
    for c, p in enumerate(per_molecule):
        if p:
            out[c, :len(p)] = torch.tensor(p)
    return out


# ---- the cluster builder -------------------------------------------------------------------------------------------------

def test_clusters_components_and_slot_order():
    from torchani_amd.md import build_constraint_clusters

    A = 12
    species = torch.zeros((2, A), dtype=torch.int64)
    species[1, 10:] = -1
    # molecule 0: a chain 7-3-9-1 given out of order, and a dimer 0-5 that sorts first; molecule 1: a triangle and a star
    per = [[(9, 3), (0, 5), (7, 3), (1, 9)], [(4, 2), (2, 6), (6, 4), (8, 0), (8, 1), (8, 3)]]
    pairs = _pairs(per)
    lengths = torch.arange(1, 13, dtype=torch.float64).view(2, 6) / 10
    fixed = torch.zeros((2, A), dtype=torch.bool)
    fixed[1, 8] = True   # the centre of the star: a fixed anchor
    inv_mass = torch.rand((2, A), dtype=torch.float64) + 0.5
    cl = build_constraint_clusters(species, pairs, lengths, fixed, inv_mass)
    assert cl.atoms.dtype == torch.int32 and cl.count.dtype == torch.int32 and cl.bonds.dtype == torch.uint8
    assert cl.d2.dtype == torch.float64 and cl.w.dtype == torch.float64
    assert cl.atoms.tolist() == [[0, 5] + [-1] * 6, [1, 3, 7, 9] + [-1] * 4, [A + 0, A + 1, A + 3, A + 8] + [-1] * 4,
                                 [A + 2, A + 4, A + 6] + [-1] * 5]
    assert cl.count.tolist() == [[2, 1], [4, 3], [4, 3], [3, 3]]
    assert cl.molecule.tolist() == [0, 0, 1, 1] and cl.per_molecule.tolist() == [4, 6]
    # constraints keep the order of ``pairs``, their atoms the orientation given, in slots of the ascending atom list
    assert cl.bonds[0, :1].tolist() == [[0, 1]]
    assert cl.bonds[1, :3].tolist() == [[3, 1], [2, 1], [0, 3]]
    assert cl.bonds[2, :3].tolist() == [[3, 0], [3, 1], [3, 2]]
    assert cl.bonds[3, :3].tolist() == [[1, 0], [0, 2], [2, 1]]
    assert torch.equal(cl.d2[1, :3], torch.tensor([0.1, 0.3, 0.4], dtype=torch.float64) ** 2)
    assert torch.equal(cl.d2[3, :3], torch.tensor([0.7, 0.8, 0.9], dtype=torch.float64) ** 2)
    assert bool((cl.d2[0, 1:] == 0).all())
    # w: the integrator's inverse masses, 0 for the fixed anchor, which the cluster does not own
    assert torch.equal(cl.w[1, :4], inv_mass[0, [1, 3, 7, 9]])
    assert cl.w[2, :4].tolist() == inv_mass[1, [0, 1, 3]].tolist() + [0.0]
    owned = torch.zeros((2, A), dtype=torch.bool)
    owned[0, [0, 5, 1, 3, 7, 9]] = True
    owned[1, [0, 1, 3, 2, 4, 6]] = True
    assert torch.equal(cl.owned, owned)
    # the same tables from the reference's cluster finder
    want = cref.find_clusters(pairs.numpy())
    assert [(c, atoms) for c, atoms, _ in want] == [(int(cl.molecule[q]), (cl.atoms[q, :cl.count[q, 0]] % A).tolist())
                                                    for q in range(4)]
    assert [[(a, b) for a, b, _ in bonds] for _, _, bonds in want] == [[tuple(ab) for ab in cl.bonds[q, :cl.count[q, 1]].tolist()]
                                                                      for q in range(4)]


def test_clusters_without_constraints_are_empty():
    from torchani_amd.md import build_constraint_clusters

    cl = build_constraint_clusters(torch.zeros((2, 5), dtype=torch.int64), torch.full((2, 3, 2), -1), torch.zeros(2, 3))
    assert cl.atoms.shape == (0, 8) and cl.bonds.shape == (0, 12, 2) and cl.per_molecule.tolist() == [0, 0]
    assert not bool(cl.owned.any())


def test_cluster_limits_and_over_determination():
    from torchani_amd.md import build_constraint_clusters

    species = torch.zeros((1, 12), dtype=torch.int64)
    build = lambda p: build_constraint_clusters(species, _pairs([p]), torch.ones(1, max(1, len(p)), dtype=torch.float64))  # noqa: E731
    chain = lambda n: [(i, i + 1) for i in range(n - 1)]   # noqa: E731
    assert build(chain(8)).count.tolist() == [[8, 7]]            # 8 atoms: the limit
    with pytest.raises(ValueError, match="more than 8 atoms"):
        build(chain(9))
    with pytest.raises(ValueError, match="more than 8 atoms"):   # a long chain, found before the labels settle
        build(chain(12))
    with pytest.raises(ValueError, match="more than 8 atoms"):   # a star of 9
        build([(0, i) for i in range(1, 9)])
    twelve = chain(8) + [(0, 2), (1, 3), (2, 4), (3, 5), (4, 6)]
    assert build(twelve).count.tolist() == [[8, 12]]             # 12 constraints: the limit
    with pytest.raises(ValueError, match="more than 12 constraints"):
        build(twelve + [(5, 7)])
    # 3n - 6: a tetrahedron of 4 atoms takes 6, a triangle 3, a dimer 1
    tetra = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    assert build(tetra).count.tolist() == [[4, 6]]
    assert build([(0, 1), (1, 2), (2, 0)]).count.tolist() == [[3, 3]]
    five = tetra + [(4, 0), (4, 1), (4, 2)]
    assert build(five).count.tolist() == [[5, 9]]
    with pytest.raises(ValueError, match="3n - 6"):
        build(five + [(4, 3)])
    with pytest.raises(ValueError, match="given twice"):         # the only way to over-determine a dimer
        build([(0, 1), (1, 0)])


def test_cluster_errors_for_padding_and_fixed_atoms():
    from torchani_amd.md import build_constraint_clusters

    species = torch.tensor([[0, 0, 3, -1]])
    one = torch.ones(1, 1, dtype=torch.float64)
    with pytest.raises(ValueError, match="padding atom"):
        build_constraint_clusters(species, _pairs([[(2, 3)]]), one)
    fixed = torch.tensor([[True, True, False, False]])
    with pytest.raises(ValueError, match="two fixed atoms"):
        build_constraint_clusters(species, _pairs([[(0, 1)]]), one, fixed)
    cl = build_constraint_clusters(species, _pairs([[(1, 2)]]), one, fixed)     # a fixed anchor gets w = 0
    assert cl.w[0, :2].tolist() == [0.0, 1.0] and cl.owned.tolist() == [[False, False, True, False]]
    with pytest.raises(ValueError, match="two different atoms"):
        build_constraint_clusters(species, _pairs([[(1, 1)]]), one)
    with pytest.raises(ValueError, match="two different atoms"):
        build_constraint_clusters(species, _pairs([[(1, 4)]]), one)
    with pytest.raises(ValueError, match="one negative index"):
        build_constraint_clusters(species, _pairs([[(1, -1)]]), one)
    with pytest.raises(ValueError, match="lengths must be > 0"):
        build_constraint_clusters(species, _pairs([[(1, 2)]]), 0 * one)


def test_bond_constraints_object_and_the_c_abi_mirror():
    from torchani_amd import _lib, md

    bc = md.BondConstraints(_pairs([[(0, 1)], []]))
    assert bc.lengths is None and bc.counts().tolist() == [1, 0]
    with pytest.raises(ValueError, match="pairs"):
        md.BondConstraints(torch.zeros((2, 3), dtype=torch.int64))
    with pytest.raises(ValueError, match="lengths"):
        md.BondConstraints(_pairs([[(0, 1)]]), torch.ones(2, 1))
    hdr = open(os.path.join(ROOT, "include", "anihip.h")).read()
    declared = set(re.findall(r"\b(anihip_[a-z_0-9]+)\s*\(", hdr))
    _lib.build()
    L = _lib.lib()
    for name in ("anihip_md_constrain_drift", "anihip_md_constrain_kick", "anihip_md_project_velocities"):
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and getattr(L, name) is not None
    for name, value in (("ATOM_CLUSTER", _lib.MD_ATOM_CLUSTER), ("CLUSTER_ATOMS", _lib.MD_CLUSTER_ATOMS),
                        ("CLUSTER_BONDS", _lib.MD_CLUSTER_BONDS)):
        assert int(re.search(rf"#define ANIHIP_MD_{name} (\d+)", hdr).group(1)) == value
    assert ctypes.sizeof(_lib.MdClusters) == 8 + 6 * 8 + 8 + 4 * 4 and _lib.MdClusters.tolerance.offset == 56


# ---- the reference -------------------------------------------------------------------------------------------------------

DIMER, TRIANGLE, CHAIN, STAR = [(0, 1)], [(0, 1), (1, 2), (2, 0)], [(0, 1), (1, 2), (2, 3)], [(0, 1), (0, 2), (0, 3), (0, 4)]
STAR_XYZ = 1.09 / np.sqrt(3.0) * np.array([[0, 0, 0], [1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float64)
TRIANGLE_XYZ = np.array([[0.0, 0.0, 0.0], [0.9572, 0.0, 0.0], [-0.24, 0.9266, 0.0]])
CHAIN_XYZ = np.array([[0.0, 0.0, 0.0], [1.2, 0.3, 0.0], [2.0, 1.3, 0.4], [3.3, 1.2, 1.1]])
DIMER_XYZ = np.array([[0.0, 0.0, 0.0], [0.7, 0.5, -0.4]])


def _molecules(xyz, bonds, mass, n_mol, seed):
    """n_mol copies of one shape, each rotated at random; lengths from the geometry."""
    rs = np.random.RandomState(seed)
    rot = np.linalg.qr(rs.normal(size=(n_mol, 3, 3)))[0]
    x = np.einsum("cij,aj->cai", rot, xyz) + rs.uniform(-5.0, 5.0, (n_mol, 1, 3))
    pairs = np.tile(np.array(bonds)[None], (n_mol, 1, 1))
    lengths = np.linalg.norm(xyz[pairs[0, :, 0]] - xyz[pairs[0, :, 1]], axis=-1)[None].repeat(n_mol, axis=0)
    m = np.tile(np.asarray(mass, dtype=np.float64)[None], (n_mol, 1))
    return x, pairs, lengths, m, np.ones(m.shape, dtype=bool)


@pytest.mark.parametrize("xyz, bonds, mass", [(DIMER_XYZ, DIMER, [15.999, 1.008]), (TRIANGLE_XYZ, TRIANGLE, [15.999, 1.008, 1.008]),
                                              (CHAIN_XYZ, CHAIN, [12.011, 14.007, 12.011, 15.999]),
                                              (STAR_XYZ, STAR, [12.011, 1.008, 1.008, 1.008, 1.008])],
                         ids=["dimer", "triangle", "chain", "star"])
def test_reference_move_and_projection(xyz, bonds, mass):
    x, pairs, lengths, m, active = _molecules(xyz, bonds, mass, 6, 3)
    cons = cref.Constraints(pairs, lengths, active, m)
    rs = np.random.RandomState(4)
    v = rs.normal(0.0, 0.02, x.shape)
    x1, v1 = cref.move(x, v, 2.0, cons)
    assert cref.residuals(x1, cons) <= 1e-12
    assert np.allclose(v1, (x1 - x) / 2.0, rtol=0, atol=1e-15)
    # the corrections lie along the bonds of the START of the move, weighted by w: the momentum is kept
    p0, p1 = (m[..., None] * v).sum(axis=1), (m[..., None] * v1).sum(axis=1)
    assert np.abs(p1 - p0).max() <= 1e-12 * np.abs(m[..., None] * v).sum(axis=1).max()
    # project_v: tangent, a projector, momentum conserving, and what a move does not see
    pv = cref.project_v(x, v, cons)
    for rv, vmax in cref.velocity_residuals(x, pv, cons):
        assert (rv <= 1e-14 * vmax[:, None]).all()
    assert np.abs(cref.project_v(x, pv, cons) - pv).max() <= 1e-15 * np.abs(v).max()
    assert np.abs((m[..., None] * (pv - v)).sum(axis=1)).max() <= 1e-14 * np.abs(m[..., None] * v).sum(axis=1).max()
    x2, _ = cref.move(x, pv, 2.0, cons)
    assert np.abs(x2 - x1).max() <= 1e-12
    # a fixed atom in the cluster: it stays, and the momentum is no longer the cluster's own
    active[:, 0] = False
    cons = cref.Constraints(pairs, lengths, active, m)
    v[:, 0] = 0.0
    x3, v3 = cref.move(x, v, 2.0, cons)
    assert np.array_equal(x3[:, 0], x[:, 0]) and np.all(v3[:, 0] == 0.0) and cref.residuals(x3, cons) <= 1e-12
    assert np.all(cref.project_v(x, v, cons)[:, 0] == 0.0)


def _well_energy_error(xyz, bonds, mass, dt, t_total, centres, k_spring=0.3):
    """Largest |E(t) - E(0)| of NVE in the well 1/2 k sum |x_i - centre_i|^2 (Hartree), constrained drift and kick."""
    x, pairs, lengths, m, active = _molecules(xyz, bonds, mass, 1, 5)
    cons = cref.Constraints(pairs, lengths, active, m)
    c = x + centres[None]
    force = lambda y: -k_spring * (y - c)   # noqa: E731
    v = cref.project_v(x, np.random.RandomState(6).normal(0.0, 0.01, x.shape), cons)
    energy = lambda y, u: (0.5 * k_spring * ((y - c) ** 2).sum() + 0.5 * (m[..., None] * u ** 2).sum() / ref.ACC_UNIT)   # noqa: E731
    e0, worst, f = energy(x, v), 0.0, force(x)
    for _ in range(int(round(t_total / dt))):
        x, v = cref.drift(x, v, f, active, m, dt, cons)
        f = force(x)
        v, _ = cref.kick(x, v, f, active, m, dt, cons)
        worst = max(worst, abs(energy(x, v) - e0))
    assert cref.residuals(x, cons) <= 1e-12
    return worst


@pytest.mark.parametrize("xyz, bonds, mass", [(DIMER_XYZ, DIMER, [15.999, 12.011]), (CHAIN_XYZ, CHAIN, [12.011, 14.007, 12.011, 15.999])],
                         ids=["dimer", "chain"])
def test_reference_scheme_is_second_order(xyz, bonds, mass):
    """A rigid dimer and a 3-bond chain, every atom on a spring to a point of its own (the springs pull the bonds apart): the
    energy error of the constrained velocity Verlet falls by 4 when dt is halved; between 3 and 5 is asked."""
    centres = np.random.RandomState(7).normal(0.0, 0.5, xyz.shape)
    errs = [_well_energy_error(xyz, bonds, mass, dt, 200.0, centres) for dt in (1.0, 0.5)]
    print(f"md constraints, order: max |dE| = {errs[0]:.3e} Ha at dt = 1 fs, {errs[1]:.3e} at 0.5 fs, ratio {errs[0] / errs[1]:.2f}")
    assert 3.0 <= errs[0] / errs[1] <= 5.0


@pytest.mark.parametrize("xyz, bonds, mass, n_mol, n_steps",
                         [(DIMER_XYZ, DIMER, [15.999, 1.008], 500, 40), (TRIANGLE_XYZ, TRIANGLE, [15.999, 1.008, 1.008], 500, 30),
                          (STAR_XYZ, STAR, [12.011, 1.008, 1.008, 1.008, 1.008], 300, 25)], ids=["dimer", "triangle", "star"])
def test_reference_equipartition(xyz, bonds, mass, n_mol, n_steps):
    """Free rigid bodies under the reference Langevin dynamics with zero forces: a molecule of n atoms and K constraints holds
    (3n - K) / 2 kT on average.  With friction 10 / fs and dt = 0.5 fs, c1 = 0.0067: the velocities of successive steps are
    independent draws, so 2 KE / kT of one molecule after one step is chi-squared with 3n - K degrees of freedom, and the mean
    over N samples has the relative standard error sqrt(2 / ((3n - K) N)).  Without the projection that follows O the mean is
    3n / 2 kT."""
    x, pairs, lengths, m, active = _molecules(xyz, bonds, mass, n_mol, 8)
    cons = cref.Constraints(pairs, lengths, active, m)
    dof = 3 * len(mass) - len(bonds)
    dt, T = 0.5, 300.0
    kT, friction = np.full(n_mol, ref.KB_HARTREE * T), np.full(n_mol, 10.0)
    zero, v, total = np.zeros(x.shape), np.zeros(x.shape), []
    for s in range(n_steps + 2):
        x, v = cref.drift(x, v, zero, active, m, dt, cons, True, kT, friction, ref.noise(21, s, n_mol, len(mass)))
        v, ke = cref.kick(x, v, zero, active, m, dt, cons)
        if s >= 2:
            total.append(ke)
    n = n_mol * n_steps
    got, want = np.mean(total), 0.5 * dof * kT[0]
    se = np.sqrt(2.0 / (dof * n))
    print(f"md constraints, equipartition: <KE> / ((3n - K) / 2 kT) = {got / want:.4f}, 3n - K = {dof}, {n} samples, "
          f"gate 4 standard errors = {4 * se:.4f}")
    assert 4.0 * se <= 0.02
    assert abs(got / want - 1.0) <= 4.0 * se
    assert cref.residuals(x, cons) <= 1e-12


# ---- hydrogen_constraints on host tensors (the in-molecule distance matrix; the cell-list path needs the GPU) ----------------

def test_hydrogen_constraints_without_a_cell():
    from torchani_amd.md import build_constraint_clusters, hydrogen_constraints

    # ethanol-like: C0 (H 3, 4, 5) - C1 (H 6, 7) - O2 (H 8), then a water O9 (H 10, 11), element indices H = 0, C = 1, O = 3
    sp = torch.tensor([[1, 1, 3, 0, 0, 0, 0, 0, 0, 3, 0, 0, -1]])
    x = torch.tensor([[[0.0, 0.0, 0.0], [1.52, 0.0, 0.0], [2.0, 1.35, 0.0], [-0.4, 1.0, 0.0], [-0.4, -0.5, 0.9], [-0.4, -0.5, -0.9],
                       [1.9, -0.5, 0.9], [1.9, -0.5, -0.9], [2.95, 1.3, 0.0], [6.0, 0.0, 0.0], [6.757, 0.586, 0.0],
                       [5.243, 0.586, 0.0], [0.0, 0.0, 0.0]]])
    bc = hydrogen_constraints(sp, x, rigid_water=True, hydrogen=0, oxygen=3)
    assert bc.pairs[0].tolist() == [[0, 3], [0, 4], [0, 5], [1, 6], [1, 7], [2, 8], [9, 10], [9, 11], [10, 11]]
    want = (x[0, bc.pairs[0, :, 0]] - x[0, bc.pairs[0, :, 1]]).double().norm(dim=-1)
    assert torch.allclose(bc.lengths[0], want, rtol=1e-12, atol=0)
    # the hydroxyl oxygen holds one hydrogen and has a carbon next to it: only the water gets its H-H pair
    cl = build_constraint_clusters(sp, bc.pairs, bc.lengths)
    assert cl.count.tolist() == [[4, 3], [3, 2], [2, 1], [3, 3]]
    assert hydrogen_constraints(sp, x, hydrogen=0, oxygen=3).counts().tolist() == [8]
    # with atomic numbers (the defaults) index 1 would be hydrogen: the species convention is the caller's to state
    z = torch.tensor([[6, 6, 8, 1, 1, 1, 1, 1, 1, 8, 1, 1, -1]])
    assert torch.equal(hydrogen_constraints(z, x, rigid_water=True).pairs, bc.pairs)
