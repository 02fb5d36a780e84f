"""CPU checks of the internal-coordinate constraints of torchani_amd.geomopt: the reference of tests/_geom_constraints_ref.py
(the fp64 restatement of include/anihip.h that the GPU tests compare the kernels with) against its defining properties and
against scipy's SLSQP on a Lennard-Jones cluster, the table builder with every error it raises, what the constructor refuses
in front of the device check, fragment_mask, rotate_dihedral, and the declarations of the C ABI."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import _geom_constraints_ref as gr
import _md_bias_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Gates of the oracle test: twice what this very comparison measured (the reference optimizer at fmax = 1e-5 Ha / A on fp32
# coordinates against SLSQP in fp64).  Measured: |E - E_SLSQP| <= 3.4e-9 Ha over the three constraint sets, |-lambda - central
# difference| <= 9.1e-6 Ha per A or rad at delta = 0.003 (not curvature-limited: the same at 0.01 for the dihedral; it is the
# force residual that fmax leaves).  The GPU test of the class uses the same gates.
ORACLE_E_GATE = 7e-9
ORACLE_SLOPE_GATE = 2e-5
ORACLE_DELTA = 0.003
ORACLE_SETS = {
    "distance": [(br.DISTANCE, (5, 6), 0.06)],
    "dihedral": [(br.DIHEDRAL, (0, 5, 6, 2), 0.05)],
    "three": [(br.DIHEDRAL, (0, 5, 6, 2), 0.05), (br.ANGLE, (0, 5, 1), 0.04), (br.DISTANCE, (5, 6), 0.06)],
}


def _make(md, kind, atoms):
    return {br.DISTANCE: md.distance, br.ANGLE: md.angle, br.DIHEDRAL: md.dihedral}[kind](*atoms)


def _tables(species, fixed, cvs, targets):
    from torchani_amd import geomopt

    t = geomopt.build_constraint_tables(species, fixed, geomopt.CVConstraints(cvs, targets))
    return gr.Tables(t.offset, t.kind, t.atoms, t.target)


def _random_case(seed=2):
    """One entry of 12 atoms about 1.5 A apart with five constraints that share atoms, atom 3 fixed."""
    from torchani_amd import md

    rs = np.random.RandomState(seed)
    x = (rs.uniform(-3.0, 3.0, (1, 12, 3))).astype(np.float32)
    cvs = [md.distance(0, 1), md.angle(1, 2, 3), md.dihedral(0, 2, 4, 5), md.distance(3, 6), md.angle(7, 0, 8)]
    active = np.ones((1, 12), dtype=bool)
    active[0, 3] = False
    fixed = torch.from_numpy(~active)
    t = _tables(torch.zeros((1, 12), dtype=torch.int64), fixed, cvs, [0.0] * 5)
    s, _ = gr.jacobian(t, 0, x.astype(np.float64).reshape(-1, 3), active.reshape(-1))
    return x, active, t, s, rs


# ---- the reference ------------------------------------------------------------------------------------------------------------

def test_reference_projection_removes_the_constrained_components():
    x, active, t, s, rs = _random_case()
    f = rs.normal(0.0, 0.05, x.shape).astype(np.float32)
    out = gr.project(t, x, f, active)
    assert out["status"][0] == 0 and np.abs(out["values"] - s).max() == 0.0
    _, J = gr.jacobian(t, 0, x.astype(np.float64).reshape(-1, 3), active.reshape(-1))
    fp = f.astype(np.float64).reshape(-1) - out["jtl"].reshape(-1)   # (before the fp32 rounding)
    worst = np.abs(J @ fp).max() / (np.linalg.norm(J) * np.linalg.norm(f))
    print(f"geom constraints reference: |J f'| / (|J| |f|) = {worst:.1e}, cond(G) = {out['cond'][0]:.1e}")
    assert worst <= 1e-12
    assert np.abs(out["jtl"][0, 3]).max() == 0.0 and np.array_equal(out["forces"][0, 3], f[0, 3])   # the fixed atom: an anchor
    untouched = [a for a in range(12) if a not in set(t.atoms[t.atoms >= 0].tolist())]
    assert untouched and np.array_equal(out["forces"][0, untouched], f[0, untouched])


def test_reference_restore_reaches_the_tolerance_by_the_minimum_norm_correction():
    x, active, t, s, rs = _random_case()
    t.target = s + rs.uniform(-0.08, 0.08, 5)
    first = {}
    out = gr.restore(t, x, active, 1e-10, 32, first_correction=first)
    assert out["status"][0] == 0 and 1 <= out["iterations"][0] <= 6
    # the fp64 iterate met the tolerance; the fp32 coordinates returned are within their own spacing of it
    r32 = np.abs(gr.residual(t, 0, out["values"].copy())).max()
    print(f"geom constraints reference: restore in {out['iterations'][0]} iterations, residual of the fp32 coordinates {r32:.1e}")
    assert (np.abs(gr.residual(t, 0, out["values"].copy())) <= gr.residual_bound(t, 0, out["coords"], 1e-10)).all()
    dx, J = first[0]
    # orthogonal to the null space of J: dx lies in the row space, so projecting it there changes nothing
    back = J.T @ np.linalg.lstsq(J.T, dx, rcond=None)[0]
    assert np.abs(back - dx).max() <= 1e-12 * np.abs(dx).max()
    null = np.linalg.svd(J)[2][5:]
    assert np.abs(null @ dx).max() <= 1e-12 * np.linalg.norm(dx)
    assert np.array_equal(out["coords"][0, 3], x[0, 3])   # the fixed atom does not move


@pytest.mark.parametrize("start, target", [(math.pi - 0.03, -math.pi + 0.03), (-math.pi + 0.03, math.pi - 0.03),
                                           (math.pi - 0.03, math.pi), (-math.pi + 0.02, math.pi - 0.01)])
def test_reference_dihedral_targets_are_reached_across_the_seam(start, target):
    from torchani_amd import md

    p = np.array([[-0.5, 1.0, 0.0], [0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [2.0, math.cos(start), math.sin(start)]])
    s0 = br.cv(br.DIHEDRAL, p)[0]
    p = p if abs(s0 - start) < 1e-9 else p * np.array([1.0, 1.0, -1.0])   # (the sign is the convention's)
    x = p[None].astype(np.float32)
    t = _tables(torch.zeros((1, 4), dtype=torch.int64), None, [md.dihedral(0, 1, 2, 3)], [target])
    out = gr.restore(t, x, np.ones((1, 4), dtype=bool), 1e-10, 32)
    assert out["status"][0] == 0 and out["iterations"][0] >= 1
    assert abs(br.wrap(out["values"][0] - target)) <= 1e-6
    assert np.abs(out["coords"].astype(np.float64) - x).max() <= 0.1   # the short way round


def test_reference_singularity_rule():
    from torchani_amd import md

    x, active, t, s, rs = _random_case()
    sp = torch.zeros((1, 12), dtype=torch.int64)
    f = np.zeros_like(x)
    ok = lambda cvs, fixed=None: gr.project(_tables(sp, fixed, cvs, None), x, f, np.ones((1, 12)) if fixed is None  # noqa: E731
                                            else ~fixed.numpy())["status"][0]
    assert ok([md.distance(0, 1), md.distance(1, 2)]) == 0
    assert ok([md.distance(0, 1), md.distance(1, 0)]) == gr.SINGULAR   # a redundant pair
    line = np.zeros((1, 12, 3), dtype=np.float32)
    line[0, :, 0] = np.arange(12)
    t3 = _tables(sp, None, [md.angle(0, 1, 2)], None)
    assert gr.project(t3, line, f, np.ones((1, 12)))["status"][0] == gr.SINGULAR   # collinear
    assert gr.singular(np.zeros((1, 1))) and not gr.singular(np.eye(3))


@pytest.mark.parametrize("name", list(ORACLE_SETS))
def test_constrained_minimum_matches_slsqp(name):
    """The reference optimizer (LbfgsReference on projected forces, restore after every step, fp32 coordinates) against SLSQP
    in fp64 under the same equality constraints, from the minimized bipyramid; -lambda against the central difference of
    SLSQP's relaxed energies at target +- ORACLE_DELTA."""
    from torchani_amd import md

    xm = gr.lj_minimum()
    E0, f0 = gr.lj(xm)
    assert abs(E0 / gr.LJ_EPS + 16.505384) <= 1e-5 and np.abs(f0).max() <= 1e-9
    cons = [(k, a, gr.cv_value(k, a, xm) + d) for k, a, d in ORACLE_SETS[name]]
    t = _tables(torch.zeros((1, 7), dtype=torch.int64), None, [_make(md, k, a) for k, a, _ in cons], [c[2] for c in cons])
    ref = gr.ConstrainedReference(gr.lj_batch, xm[None], np.ones((1, 7), dtype=bool), t, fmax=1e-5).run(300)
    assert ref.lb.converged.all() and ref.lb.n_steps[0] < 110
    resid = np.abs(gr.residual(t, 0, ref.values.copy()))
    assert (resid <= gr.residual_bound(t, 0, ref.x, 1e-8)).all(), (resid, gr.residual_bound(t, 0, ref.x, 1e-8))
    resid = resid.max()
    Es, xs = gr.slsqp(xm, cons)
    dE = abs(ref.energies[0] - Es)
    print(f"geom constraints oracle, {name}: {ref.lb.n_steps[0]} steps, residual {resid:.1e}, |E - E_SLSQP| = {dE:.1e} Ha "
          f"(gate {ORACLE_E_GATE:.0e})")
    assert dE <= ORACLE_E_GATE
    for i, (k, a, tt) in enumerate(cons):
        e = [gr.slsqp(xs, [c if j != i else (k, a, tt + sgn * ORACLE_DELTA) for j, c in enumerate(cons)])[0] for sgn in (1, -1)]
        slope = (e[0] - e[1]) / (2 * ORACLE_DELTA)
        print(f"    constraint {i}: -lambda = {-ref.multipliers[i]:.6e}, dE*/dt = {slope:.6e}, difference "
              f"{abs(-ref.multipliers[i] - slope):.1e} (gate {ORACLE_SLOPE_GATE:.0e})")
        assert abs(-ref.multipliers[i] - slope) <= ORACLE_SLOPE_GATE


# ---- the table builder --------------------------------------------------------------------------------------------------------

def _species(Cn=3, A=6):
    sp = torch.zeros((Cn, A), dtype=torch.int64)
    sp[1, A - 1] = -1   # padding
    return sp


def test_tables_layout():
    from torchani_amd import _lib, geomopt, md

    sp = _species()
    cvs = [md.distance(0, 1), md.angle(0, 1, torch.tensor([2, -1, 3])), md.dihedral(0, 1, 2, 3)]
    scan = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    t = geomopt.build_constraint_tables(sp, None, geomopt.CVConstraints(cvs, [1.5, 2.0, scan]))
    assert t.offset.tolist() == [0, 3, 5, 8] and t.offset.dtype == torch.int32
    assert t.kind.tolist() == [0, 1, 2, 0, 2, 0, 1, 2] and t.kind.dtype == torch.int32
    assert t.atoms.tolist() == [[0, 1, -1, -1], [0, 1, 2, -1], [0, 1, 2, 3], [6, 7, -1, -1], [6, 7, 8, 9], [12, 13, -1, -1],
                                [12, 13, 15, -1], [12, 13, 14, 15]] and t.atoms.dtype == torch.int32
    assert t.target.tolist() == [1.5, 2.0, 1.0, 1.5, 2.0, 1.5, 2.0, 3.0] and t.target.dtype == torch.float64
    assert t.index.tolist() == [[0, 1, 2], [3, -1, 4], [5, 6, 7]]
    # no targets: NaN, which the optimizer replaces by the values of the initial coordinates; a single CV and a single target
    t = geomopt.build_constraint_tables(sp, None, geomopt.CVConstraints(md.distance(0, 1)))
    assert torch.isnan(t.target).all() and t.offset.tolist() == [0, 1, 2, 3]
    t = geomopt.build_constraint_tables(sp, None, geomopt.CVConstraints(md.distance(0, 1), scan))
    assert t.target.tolist() == [1.0, 2.0, 3.0]
    # CVs that are -1 everywhere: empty tables
    t = geomopt.build_constraint_tables(sp, None, geomopt.CVConstraints(md.distance(torch.full((3,), -1), 1)))
    assert t.kind.numel() == 0 and t.offset.tolist() == [0, 0, 0, 0] and tuple(t.atoms.shape) == (0, 4)
    # a fixed atom inside a constraint is an anchor
    fixed = torch.zeros((3, 6), dtype=torch.bool)
    fixed[:, 0] = True
    assert geomopt.build_constraint_tables(sp, fixed, geomopt.CVConstraints(md.distance(0, 1))).kind.numel() == 3
    assert geomopt.MAX_CONSTRAINTS == _lib.GEOM_MAX_CONSTRAINTS == gr.MAX_CONSTRAINTS == 8


_D01 = None
BAD = [
    ("0 .. 5", lambda md: ([md.distance(0, 6)], None, None)),
    ("entry 2, distance of atoms \\(0, 7\\)", lambda md: ([md.distance(0, torch.tensor([1, 1, 7]))], None, None)),
    ("padding atom: entry 1, distance of atoms \\(0, 5\\)", lambda md: ([md.distance(0, 5)], None, None)),
    ("4 different atoms: entry 1, dihedral of atoms \\(0, 1, 2, 1\\)",
     lambda md: ([md.dihedral(0, 1, 2, torch.tensor([3, 1, 3]))], None, None)),
    ("entry 0 has 9 constraints, more than 8", lambda md: ([md.distance(i % 2, 2 + i % 3) for i in range(9)], None, None)),
    ("free atom, all of these are fixed: entry 0, angle of atoms \\(0, 1, 2\\)", lambda md: ([md.angle(0, 1, 2)], None, "012")),
    ("same CV was given twice: constraint 2, distance", lambda md: ((lambda d: [d, md.distance(2, 3), d])(md.distance(0, 1)),
                                                                    None, None)),
    ("one value per CV \\(2\\), got 1", lambda md: ([md.distance(0, 1), md.distance(1, 2)], [1.0], None)),
    ("a target must be a number or a tensor of shape \\(3,\\)", lambda md: ([md.distance(0, 1)], [torch.zeros(2)], None)),
    ("a target must be finite: entry 1", lambda md: ([md.distance(0, 1)], [torch.tensor([1.0, float("inf"), 1.0])], None)),
    ("index tensor must have shape \\(3,\\)", lambda md: ([md.distance(0, torch.tensor([1, 2]))], None, None)),
    ("needs CVs", lambda md: ([(0, 1)], None, None)),
]


@pytest.mark.parametrize("case", range(len(BAD)))
def test_builder_errors_name_the_entry_and_the_atoms(case):
    from torchani_amd import geomopt, md

    message, make = BAD[case]
    with pytest.raises(ValueError, match=message):
        cvs, targets, fix = make(md)
        fixed = None
        if fix:
            fixed = torch.zeros((3, 6), dtype=torch.bool)
            fixed[0, [int(ch) for ch in fix]] = True
        geomopt.build_constraint_tables(_species(), fixed, geomopt.CVConstraints(cvs, targets))


def test_constructor_refuses_before_it_needs_a_device():
    """Every check of the constraints is host work in front of the "needs a ROCm device" check: CPU tensors reach all of it."""
    from torchani_amd import geomopt, md

    sp = _species()
    x = torch.zeros((3, 6, 3))
    x[:, :, 0] = torch.arange(6.0) * 1.1
    x[:, 1::2, 1] = 0.8
    x[:, 3, 2] = 0.5
    make = lambda cons, **kw: geomopt.GeometryOptimizer(None, sp, x, constraints=cons, **kw)   # noqa: E731
    d01 = float((x[0, 0] - x[0, 1]).norm())
    with pytest.raises(ValueError, match="padding atom: entry 1"):
        make(geomopt.CVConstraints(md.distance(0, 5)))
    with pytest.raises(ValueError, match="must be a CVConstraints"):
        make([md.distance(0, 1)])
    with pytest.raises(ValueError, match="constraint_tolerance must be > 0"):
        make(geomopt.CVConstraints(md.distance(0, 1)), constraint_tolerance=0.0)
    with pytest.raises(ValueError, match="constraint_max_iterations must be an integer >= 1"):
        make(geomopt.CVConstraints(md.distance(0, 1)), constraint_max_iterations=0)
    with pytest.raises(ValueError, match="entry 2 \\(distance of atoms \\(0, 1\\)\\).*0\\.15.*rotate_dihedral"):
        make(geomopt.CVConstraints(md.distance(0, 1), torch.tensor([d01, d01 + 0.05, d01 + 0.15], dtype=torch.float64)))
    with pytest.raises(ValueError, match="entry 0 .*dihedral of atoms \\(0, 1, 2, 3\\).*rotate_dihedral"):
        make(geomopt.CVConstraints([md.distance(0, 1), md.dihedral(0, 1, 2, 3)], [d01, 3.0]))
    # valid constraints pass every host check and stop at the device check: held values, near targets, a seam
    s = float(geomopt._cv_values(2, x[0, :4].double()))
    for cons in (geomopt.CVConstraints(md.distance(0, 1)), geomopt.CVConstraints(md.distance(0, 1), d01 + 0.09),
                 geomopt.CVConstraints(md.dihedral(0, 1, 2, 3), s + 0.05 - 2 * math.pi), None):
        with pytest.raises(ValueError, match="ROCm device"):
            make(cons)
    with pytest.raises(ValueError, match="ROCm device"):
        geomopt.optimize_geometry(None, sp, x, constraints=geomopt.CVConstraints(md.distance(0, 1)), steps=3)


# ---- fragments and rotations --------------------------------------------------------------------------------------------------

def _butane():
    """n-butane, hand-built: the carbons zigzag in the xy plane (0 .. 3), hydrogens 4 .. 13 on C0 (3), C1 (2), C2 (2), C3 (3)."""
    c = np.array([[0.0, 0.0, 0.0], [1.26, 0.87, 0.0], [2.52, 0.0, 0.0], [3.78, 0.87, 0.0]])
    h = [c[0] + (-0.9, 0.62, 0.0), c[0] + (0.0, -0.63, 0.89), c[0] + (0.0, -0.63, -0.89),
         c[1] + (0.0, 0.63, 0.89), c[1] + (0.0, 0.63, -0.89), c[2] + (0.0, -0.63, 0.89), c[2] + (0.0, -0.63, -0.89),
         c[3] + (0.9, -0.62, 0.0), c[3] + (0.0, 0.63, 0.89), c[3] + (0.0, 0.63, -0.89)]
    z = torch.tensor([6] * 4 + [1] * 10)
    return z, torch.from_numpy(np.vstack([c, np.array(h)]))


def test_fragment_mask_on_butane_and_on_a_ring():
    from torchani_amd import geomopt

    z, x = _butane()
    m = geomopt.fragment_mask(z, x, 1, 2)
    assert m.dtype == torch.bool and m.nonzero().view(-1).tolist() == [2, 3, 9, 10, 11, 12, 13]
    assert geomopt.fragment_mask(z, x, 2, 1).nonzero().view(-1).tolist() == [0, 1, 4, 5, 6, 7, 8]
    assert geomopt.fragment_mask(z, x, 0, 4).nonzero().view(-1).tolist() == [4]   # a terminal hydrogen
    # padding atoms are in no fragment, wherever they sit
    zp, xp = torch.cat([z, torch.tensor([-1])]), torch.cat([x, x[2:3] + 0.1])
    assert geomopt.fragment_mask(zp, xp, 1, 2).nonzero().view(-1).tolist() == [2, 3, 9, 10, 11, 12, 13]
    # a loose scale bonds nothing: k alone
    assert geomopt.fragment_mask(z, x, 1, 2, scale=0.5).nonzero().view(-1).tolist() == [2]
    t = 2 * math.pi * torch.arange(6) / 6
    ring = torch.stack([1.39 * torch.cos(t), 1.39 * torch.sin(t), torch.zeros(6)], dim=1).double()
    with pytest.raises(ValueError, match="bond 0-1 is in a ring"):
        geomopt.fragment_mask(torch.full((6,), 6), ring, 0, 1)
    with pytest.raises(ValueError, match="no covalent radius for atomic number 35"):
        geomopt.fragment_mask(torch.tensor([6, 35]), ring[:2], 0, 1)
    with pytest.raises(ValueError, match="two different atoms"):
        geomopt.fragment_mask(z, x, 1, 1)


def test_rotate_dihedral_hits_the_angle_and_moves_the_fragment_rigidly():
    from torchani_amd import geomopt

    z, x = _butane()
    quad = (0, 1, 2, 3)
    moving = geomopt.fragment_mask(z, x, 1, 2)
    d0 = torch.cdist(x, x)
    assert abs(abs(float(geomopt._cv_values(2, x[list(quad)]))) - math.pi) <= 1e-12   # built trans
    for angle in (0.0, 1.0, -2.5, math.pi, -math.pi + 0.01, 3.1):
        y = geomopt.rotate_dihedral(x.float(), quad, angle, moving)
        assert y.dtype == torch.float64
        y = geomopt.rotate_dihedral(x, quad, angle, moving)
        got = br.cv(br.DIHEDRAL, y[list(quad)].numpy())[0]
        assert abs(br.wrap(got - angle)) <= 1e-12, (angle, got)
        d = torch.cdist(y, y)
        for side in (moving, ~moving):
            assert (d[side][:, side] - d0[side][:, side]).abs().max() <= 1e-12
        assert torch.equal(y[~moving], x[~moving]) and torch.equal(y[2], x[2])
    with pytest.raises(ValueError, match="moving must hold atom l = 3"):
        geomopt.rotate_dihedral(x, quad, 1.0, ~moving)


def test_torsion_scan_host_side():
    """The tuple, and the host work in front of the device check: with ``moving=None`` the fragment comes from the atomic
    numbers, which an ANI model without ``periodic_table_index`` gives through its ``symbols``."""
    from torchani_amd import geomopt, tuples

    assert tuples.TorsionScan._fields == ("angles", "energies", "coordinates", "converged", "torques")
    z, x = _butane()

    class Numbers:
        periodic_table_index, symbols = True, ("H", "C")

    class Indices:
        periodic_table_index, symbols = False, ("H", "C")

    for model, sp in ((Numbers(), z), (Indices(), torch.where(z == 6, 1, 0))):
        with pytest.raises(ValueError, match="ROCm device"):
            geomopt.torsion_scan(model, sp, x, (0, 1, 2, 3), [0.0, 1.0])
    with pytest.raises(ValueError, match="four dihedral atoms"):
        geomopt.torsion_scan(Numbers(), z, x, (0, 1, 2), [0.0])
    with pytest.raises(ValueError, match="moving must be a bool mask"):
        geomopt.torsion_scan(Numbers(), z, x, (0, 1, 2, 3), [0.0], moving=torch.zeros(3, dtype=torch.bool))
    with pytest.raises(ValueError, match="moving must hold atom l = 3"):
        geomopt.torsion_scan(Numbers(), z, x, (0, 1, 2, 3), [0.0], moving=torch.zeros(14, dtype=torch.bool))
    ring = torch.full((6,), 6)
    t = 2 * math.pi * torch.arange(6) / 6
    with pytest.raises(ValueError, match="in a ring"):
        geomopt.torsion_scan(Numbers(), ring, torch.stack([1.39 * torch.cos(t), 1.39 * torch.sin(t), torch.zeros(6)], dim=1),
                             (0, 1, 2, 3), [0.0])


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------

def test_abi_is_declared_and_bound():
    from torchani_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "anihip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(anihip_[a-z_0-9]+)\s*\(", code))
    L = _lib.lib()
    for name in ("anihip_geom_constraints_project", "anihip_geom_constraints_restore"):
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and getattr(L, name) is not None
        assert getattr(L, name).restype is C.c_int
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    assert "geom_constraints.hip" in _lib.SOURCES and "md_cv.h" in _lib.HEADERS
    assert re.search(r"#define\s+ANIHIP_ABI_VERSION\s+13\b", hdr) and _lib.ABI_VERSION == 13 and L.anihip_abi_version() == 13
    for name, value in (("GEOM_MAX_CONSTRAINTS", 8), ("GEOM_BAD_TABLE", 1), ("GEOM_SINGULAR", 2), ("GEOM_NOT_CONVERGED", 4)):
        assert re.search(rf"#define\s+ANIHIP_{name}\s+{value}\b", hdr), name
        assert getattr(_lib, name) == value
    assert (gr.BAD_TABLE, gr.SINGULAR, gr.NOT_CONVERGED) == (_lib.GEOM_BAD_TABLE, _lib.GEOM_SINGULAR, _lib.GEOM_NOT_CONVERGED)
    # the struct of the header, field for field: two int32, a double, then eight pointers
    body = re.search(r"typedef struct \{([^}]*)\} anihip_geom_constraints;", code).group(1)
    names = re.findall(r"\*?\b([a-z_A-Z0-9]+)\s*[,;]", body)
    assert names == [n for n, _ in _lib.GeomConstraints._fields_]
    assert C.sizeof(_lib.GeomConstraints) == 2 * 4 + 8 + 8 * C.sizeof(C.c_void_p)
    assert _lib.GeomConstraints.tolerance.offset == 8 and _lib.GeomConstraints.offset.offset == 16
    assert _lib.GeomConstraints.status.offset == 16 + 7 * 8
    assert C.sizeof(_lib.LbfgsParams) == 4 * 4 + 4 * 8 and C.sizeof(_lib.MdBias) == 6 * 4 + 17 * C.sizeof(C.c_void_p)   # unchanged
    # the CV formulas live in one header that both sources include
    csrc = os.path.join(ROOT, "torchani_amd", "csrc")
    assert "void cv_eval(" in open(os.path.join(csrc, "md_cv.h")).read()
    for src in ("md_bias.hip", "geom_constraints.hip"):
        text = open(os.path.join(csrc, src)).read()
        assert '#include "md_cv.h"' in text and "atan2(" not in text
