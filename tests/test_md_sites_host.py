"""CPU checks of the group CVs of biased MD (md.center, md.coordination): the reference of tests/_md_sites_ref.py (the fp64
restatement of include/anihip.h that the GPU tests compare the kernels with) against autograd, the value-site identity, the
table builder with every error it raises, what the constructors refuse, and the declarations of the C ABI."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import _md_bias_ref as br
import _md_sites_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORTHO = np.diag([9.0, 10.0, 11.0])
TRICLINIC = np.array([[9.0, 0.0, 0.0], [2.5, 9.5, 0.0], [-1.5, 2.0, 10.0]])


# ---- the reference ------------------------------------------------------------------------------------------------------------

def _torch_coordination(x, ga, gb, p, cell, pbc):
    """The definition of include/anihip.h written for autograd."""
    r0, d0, r_max, n = p
    b = 0.0 if math.isinf(r_max) else sr.base(r_max, r0, d0, n)
    s = x.new_zeros(())
    for i in ga:
        for j in gb:
            if i == j:
                continue
            d = x[i] - x[j]
            if cell is not None:
                h = torch.tensor(cell)
                shift = torch.round(d.detach() @ torch.linalg.inv(h)) * torch.tensor(pbc, dtype=torch.float64)
                d = d - shift @ h
            r = d.norm()
            if float(r.detach()) < r_max:
                s = s + (1.0 / (1.0 + (torch.clamp(r - d0, min=0.0) / r0) ** n) - b) / (1.0 - b)
    return s


COORD_CASES = [   # (name, cell, pbc, group A, group B, (r0, d0, r_max, n))
    ("open n=6", None, (0, 0, 0), [0, 1, 2], [3, 4, 5, 6, 7], (2.0, 0.0, math.inf, 6)),
    ("open n=2 cut", None, (0, 0, 0), [0, 1, 2], [3, 4, 5, 6, 7], (1.5, 0.0, 4.5, 2)),
    ("open n=12 d0", None, (0, 0, 0), [0, 1, 2, 3], [4, 5, 6, 7, 8, 9], (1.2, 1.5, 5.0, 12)),
    ("overlap", None, (0, 0, 0), [0, 1, 2, 3, 4], [3, 4, 5, 6], (2.0, 0.5, math.inf, 6)),
    ("same group", None, (0, 0, 0), list(range(8)), list(range(8)), (2.0, 0.0, 6.0, 6)),
    ("orthorhombic", ORTHO, (1, 1, 1), [0, 1, 2, 3], [4, 5, 6, 7, 8, 9], (2.0, 0.3, 4.4, 6)),
    ("triclinic", TRICLINIC, (1, 1, 1), [0, 1, 2, 3], [2, 3, 4, 5, 6, 7, 8, 9], (2.0, 0.0, 4.2, 6)),
    ("triclinic mixed pbc n=12", TRICLINIC, (1, 0, 1), [0, 1, 2, 3], [4, 5, 6, 7, 8, 9], (2.5, 0.4, 4.0, 12)),
]


@pytest.mark.parametrize("case", range(len(COORD_CASES)))
def test_reference_coordination_matches_autograd(case):
    name, cell, pbc, ga, gb, p = COORD_CASES[case]
    rs = np.random.RandomState(11 + case)
    x = rs.uniform(0.0, 6.0, (10, 3))
    if cell is not None:   # atoms displaced by whole lattice vectors: the minimum image has work to do
        x = x + (rs.randint(-2, 3, (10, 3)) * np.asarray(pbc)) @ cell
    s, sa, grad = sr.coordination(x, ga, gb, p, cell, pbc)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    st = _torch_coordination(xt, ga, gb, p, cell, pbc)
    st.backward()
    assert s > 0.1 and abs(s - float(st.detach())) <= 1e-12 * sa
    err = np.abs(grad - xt.grad.numpy()).max() / max(1.0, np.abs(grad).max())
    print(f"md sites reference: coordination ({name}) gradient against autograd, relative difference {err:.1e}")
    assert err <= 1e-12
    assert np.abs(grad.sum(axis=0)).max() <= 1e-12 * max(1.0, np.abs(grad).max())   # translation invariance


def test_reference_centre_gradients_match_autograd():
    """A CV on centres: the gradient on atom i of group v is w_i times the CV's gradient on the site, what the spread adds."""
    rs = np.random.RandomState(5)
    x = rs.normal(0.0, 2.0, (12, 3))
    groups = [np.array([0, 1, 2, 3]), np.array([3, 4, 5]), np.array([6, 7, 8, 9, 10]), np.array([11])]
    weights = [rs.uniform(0.5, 16.0, g.size) for g in groups]
    weights = [w / w.sum() for w in weights]
    worst = 0.0
    for kind, n in ((br.DISTANCE, 2), (br.ANGLE, 3), (br.DIHEDRAL, 4)):
        sites = np.stack([sr.center(x, groups[k], weights[k])[0] for k in range(n)])
        s, g = br.cv(kind, sites)
        grad = np.zeros_like(x)
        for k in range(n):
            for i, w in zip(groups[k], weights[k]):
                grad[i] += w * g[k]
        xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        st = [sum(float(w) * xt[int(i)] for i, w in zip(groups[k], weights[k])) for k in range(n)]
        if kind == br.DISTANCE:
            val = (st[0] - st[1]).norm()
        elif kind == br.ANGLE:
            a, b = st[0] - st[1], st[2] - st[1]
            val = torch.atan2(torch.linalg.cross(a, b).norm(), a @ b)
        else:
            b1, b2, b3 = st[1] - st[0], st[2] - st[1], st[3] - st[2]
            n1, n2 = torch.linalg.cross(b1, b2), torch.linalg.cross(b2, b3)
            val = torch.atan2(b2.norm() * (b1 @ n2), n1 @ n2)
        val.backward()
        assert abs(s - float(val.detach())) <= 1e-13
        worst = max(worst, np.abs(grad - xt.grad.numpy()).max() / max(1.0, np.abs(grad).max()))
    print(f"md sites reference: centre CV gradients against autograd, worst relative difference {worst:.1e}")
    assert worst <= 1e-12


def test_switch_is_continuous_at_r_max_and_one_below_d0():
    for n in (2, 6, 12):
        for d0 in (0.0, 0.8):
            p = (1.7, d0, 4.0, n)
            for r in (0.0, 0.5 * d0, d0):
                assert sr.switch(r, *p) == (1.0, 0.0)
            sw, dsw = sr.switch(np.nextafter(4.0, 0.0), *p)
            assert 0.0 <= sw <= 1e-15 and dsw < 0.0
            assert sr.switch(4.0, *p) == (0.0, 0.0) and sr.switch(7.0, *p) == (0.0, 0.0)
            # C1 at d0 (n >= 2), monotone, and dsw the derivative of sw
            assert abs(sr.switch(d0 + 1e-9, *p)[1]) <= 1e-7
            for r in np.linspace(d0 + 0.1, 3.9, 9):
                h = 1e-6
                num = (sr.switch(r + h, *p)[0] - sr.switch(r - h, *p)[0]) / (2 * h)
                assert abs(num - sr.switch(r, *p)[1]) <= 1e-8 and sr.switch(r, *p)[1] < 0
            q = (1.7, d0, math.inf, n)   # no cut: the plain rational function
            assert abs(sr.switch(d0 + 1.7, *q)[0] - 0.5) <= 1e-16 and sr.switch(1e9, *q)[0] > 0.0


def test_value_site_carries_the_number_exactly_through_the_distance_cv():
    """distance(value site, anchor) = s' bit for bit with the gradient exactly (+1, 0, 0) on the value site, and the two-float
    pair holds s to 2^-48 relative, down to the floor."""
    rs = np.random.RandomState(9)
    values = np.concatenate([[0.0, sr.FLOOR, 1e-30, 1.0, 1999.999, 2.0e6], 10.0 ** rs.uniform(-12, 7, 4000)])
    for s in values:
        sp = max(s, sr.FLOOR)
        hi, lo = sr.split(sp)
        x = float(hi) + float(lo)
        assert abs(x - sp) <= 2.0 ** -48 * sp and (lo == 0 or abs(float(lo)) >= 2.0 ** -126)
        d, g = br.cv(br.DISTANCE, np.array([[x, 0.0, 0.0], [0.0, 0.0, 0.0]]))
        assert d == x and g.tolist() == [[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]]
    assert sr.FLOOR == 2.0 ** -64


# ---- the table builder --------------------------------------------------------------------------------------------------------

def _species(Cn=2, A=6):
    sp = torch.zeros((Cn, A), dtype=torch.int64)
    sp[1, A - 1] = -1   # padding
    return sp


def test_tables_layout():
    from torchani_amd import _lib, md

    sp = _species()
    masses = torch.tensor([[1.0, 3.0, 1, 1, 1, 1], [2.0, 2.0, 1, 1, 1, 0]])
    mask = torch.zeros((2, 6), dtype=torch.bool)
    mask[0, :3] = True   # entry 1 has no such centre
    c1, c2 = md.center([1, 0]), md.center(mask, None)
    co = md.coordination([0, 1], [1, 2, 3], 1.5, r_max=4.0)
    d12 = md.distance(c1, c2)
    bias = [md.Restraint(d12, 1.0, 0.1), md.Restraint(co, 2.0, 0.1), md.Restraint(md.angle(4, c1, 3), 1.0, 1.0),
            md.Metadynamics([co, md.distance(0, c1)], (0.2, 0.1), 1e-3, 2)]
    st, bt = md.build_site_tables(sp, None, bias, masses=masses)
    assert st.max_sites == 4
    # entry 0: c1, c2, anchor, value; entry 1 (no c2): c1, anchor, value, none
    assert st.site_kind.tolist() == [[1, 1, 2, 3], [1, 2, 3, 0]] and st.site_ref.tolist() == [[0, 2, 0, 0], [1, 1, 1, 0]]
    assert st.group_offset.tolist() == [0, 2, 4, 7, 9, 12, 14, 17]
    assert st.group_atoms.tolist() == [0, 1, 6, 7, 0, 1, 2, 0, 1, 1, 2, 3, 6, 7, 7, 8, 9]
    assert st.group_weights[:7].tolist() == [0.25, 0.75, 0.5, 0.5, 1 / 3, 1 / 3, 1 / 3] and st.group_weights[7:].abs().max() == 0
    assert st.coord.tolist() == [[0, 3, 4, 3, 6], [1, 5, 6, 2, 6]]
    assert st.coord_params[0].tolist() == [1.5, 0.0, 4.0, sr.base(4.0, 1.5, 0.0, 6)]
    # atom 1 of entry 0: in c1 (slot 0), c2 (slot 1) and on both sides of the coordination number (slot 3, A before B)
    assert st.member_offset.tolist() == [0, 3, 7, 9, 10, 10, 10, 12, 15, 16, 17, 17, 17]
    assert st.member_site[3:7].tolist() == [[0, 0], [1, 0], [3, 1], [3, 2]]
    assert st.member_weight[3:7].tolist() == [0.75, 1 / 3, 0.0, 0.0]
    assert st.species_ext.tolist() == [[0] * 10, [0, 0, 0, 0, 0, -1, 0, 0, 0, -1]] and st.pbc == (0, 0, 0)
    # the CVs on extended indices A + v of entries of 10 atoms; entry 1 lacks the distance between the centres
    assert bt.cv_offset.tolist() == [0, 4, 7]
    assert bt.atoms.tolist() == [[6, 7, -1, -1], [9, 8, -1, -1], [4, 6, 3, -1], [0, 6, -1, -1],
                                 [18, 17, -1, -1], [14, 16, 13, -1], [10, 16, -1, -1]]
    assert bt.kind.tolist() == [0, 0, 1, 0, 0, 1, 0]
    assert bt.meta_cv.tolist() == [[1, 3], [0, 2]]   # the coordination number shares the row of its restraint
    # a bias without sites: what build_bias_tables gives, and no site tables
    plain = [md.Restraint(md.distance(0, 1), 1.0, 0.1)]
    st0, bt0 = md.build_site_tables(sp, None, plain)
    assert st0 is None and bt0.atoms.tolist() == md.build_bias_tables(sp, None, plain).atoms.tolist()
    # a periodic cell: passed by value with its inverse
    st, _ = md.build_site_tables(sp, None, [md.Restraint(co, 2.0, 0.1)], cell=torch.tensor(TRICLINIC), pbc=(True, False, True))
    assert st.pbc == (1, 0, 1) and np.allclose(np.array(st.cell).reshape(3, 3) @ np.array(st.inv_cell).reshape(3, 3), np.eye(3))
    assert _lib.MD_SITES_MAX == sr.MAX_SITES == 64


def _many(md, n):
    return [md.Restraint(md.distance(0, md.center([1, 2])), 1.0, 1.0, 0.0) for _ in range(n)]


BAD = [
    ("padding atom: entry 1, atom 5", {}, lambda md: [md.Restraint(md.distance(0, md.center([4, 5])), 1.0, 1.0)]),
    ("padding atom: entry 1, atom 5", {}, lambda md: [md.Restraint(md.coordination([0], torch.ones(6, dtype=torch.bool), 1.0), 1.0, 1.0)]),
    ("entry 0, atom index 6 of a group is outside 0 .. 5", {}, lambda md: [md.Restraint(md.distance(0, md.center([1, 6])), 1.0, 1.0)]),
    ("atom index 6 is outside 0 .. 5", {}, lambda md: [md.Restraint(md.distance(6, md.center([1, 2])), 1.0, 1.0)]),
    ("entry 1, distance with atom 7", {}, lambda md: [md.Restraint(md.distance(torch.tensor([1, 7]), md.center([1, 2])), 1.0, 1.0)]),
    ("entry 0 has more than 64 sites", {}, lambda md: [md.Restraint(md.dihedral(*(md.center([k % 5]) for k in range(4 * j, 4 * j + 4))), 1.0, 1.0)
                                                       for j in range(16)] + [md.Restraint(md.distance(0, md.center([1, 2])), 1.0, 1.0)]),
    ("entry 0 has 17 CVs, more than 16", {}, lambda md: _many(md, 17)),
    ("entry 0: r0 must be > 0", {}, lambda md: [md.Restraint(md.coordination([0], [1], 0.0), 1.0, 1.0)]),
    ("entry 0: d0 must be >= 0", {}, lambda md: [md.Restraint(md.coordination([0], [1], 1.0, d0=-0.1), 1.0, 1.0)]),
    ("entry 0: n must be an integer in 2 .. 32, got 1", {}, lambda md: [md.Restraint(md.coordination([0], [1], 1.0, n=1), 1.0, 1.0)]),
    ("n must be an integer in 2 .. 32, got 33", {}, lambda md: [md.Restraint(md.coordination([0], [1], 1.0, n=33), 1.0, 1.0)]),
    ("entry 0: r_max must be > d0", {}, lambda md: [md.Restraint(md.coordination([0], [1], 1.0, d0=2.0, r_max=2.0), 1.0, 1.0)]),
    ("entry 0: a periodic cell needs r_max", {"cell": torch.tensor(ORTHO), "pbc": (True, True, True)},
     lambda md: [md.Restraint(md.coordination([0], [1], 1.0), 1.0, 1.0)]),
    ("entry 0: r_max = 4.6 exceeds half the smallest perpendicular width", {"cell": torch.tensor(ORTHO), "pbc": (True, True, True)},
     lambda md: [md.Restraint(md.coordination([0], [1], 1.0, r_max=4.6), 1.0, 1.0)]),
    ("exceeds half the smallest perpendicular width", {"cell": torch.tensor(TRICLINIC), "pbc": (False, True, False)},
     lambda md: [md.Restraint(md.coordination([0], [1], 1.0, r_max=4.7), 1.0, 1.0)]),
    ("entry 1: the group has zero total mass", {"masses": torch.tensor([[1.0] * 6, [0.0, 0.0, 1, 1, 1, 0]])},
     lambda md: [md.Restraint(md.distance(3, md.center([0, 1])), 1.0, 1.0)]),
    ('weights="mass" needs the masses', {}, lambda md: [md.Restraint(md.distance(3, md.center([0, 1])), 1.0, 1.0)]),
    ("group mask must have shape \\(6,\\) or \\(2, 6\\), got \\(5,\\)", {},
     lambda md: [md.Restraint(md.distance(3, md.center(torch.ones(5, dtype=torch.bool), None)), 1.0, 1.0)]),
    ("group mask must have shape", {}, lambda md: [md.Restraint(md.coordination([0], torch.ones((3, 6), dtype=torch.bool), 1.0), 1.0, 1.0)]),
    ("2 different atoms", {}, lambda md: (lambda c: [md.Restraint(md.distance(c, c), 1.0, 1.0)])(md.center([0, 1], None))),
    ("k must be >= 0: entry 0", {}, lambda md: [md.Restraint(md.coordination([0], [1], 1.0), 1.0, -1.0)]),
]


@pytest.mark.parametrize("case", range(len(BAD)))
def test_builder_errors_name_the_entry(case):
    from torchani_amd import md

    message, kw, make = BAD[case]
    kw = dict(kw)
    if "masses" not in kw and "needs the masses" not in message:
        kw["masses"] = torch.ones((2, 6))
    with pytest.raises(ValueError, match=message):
        md.build_site_tables(_species(), None, make(md), **kw)


def test_the_triclinic_half_width_is_the_perpendicular_one():
    """Along b alone the width of TRICLINIC is 9.5 cos(atan(2 / 10)) = 9.316: 4.65 passes, 4.66 does not (the row's length 9.82 / 2 would)."""
    from torchani_amd import md

    kw = {"cell": torch.tensor(TRICLINIC), "pbc": (False, True, False)}
    md.build_site_tables(_species(), None, [md.Restraint(md.coordination([0], [1], 1.0, r_max=4.65), 1.0, 1.0)], **kw)
    with pytest.raises(ValueError, match="perpendicular width"):
        md.build_site_tables(_species(), None, [md.Restraint(md.coordination([0], [1], 1.0, r_max=4.66), 1.0, 1.0)], **kw)


def test_groups_and_parameters_are_checked_where_the_site_is_made():
    from torchani_amd import md

    for bad in ([0, 1.0], [True, 1], torch.tensor([0, 1]), torch.ones((2, 2, 2), dtype=torch.bool), [0, 0]):
        with pytest.raises(ValueError, match="group"):
            md.center(bad)
    with pytest.raises(ValueError, match='weights must be "mass" or None'):
        md.center([0, 1], "geometric")
    with pytest.raises(ValueError, match="r0 must be a number"):
        md.coordination([0], [1], "1")
    with pytest.raises(ValueError, match="n must be an integer"):
        md.coordination([0], [1], 1.0, n=6.0)
    site, cv = md.center([2, 0, 1]), md.coordination([0], [1, 2], 1.0)
    assert isinstance(site, md.Site) and site.atoms == (0, 1, 2) and isinstance(cv, md.CV) and cv.kind == 0
    assert isinstance(md.distance(0, site), md.CV) and isinstance(md.dihedral(site, 1, md.center([3]), 4), md.CV)


def test_constructors_refuse_before_they_need_a_device():
    from torchani_amd import geomopt, md

    sp = _species()
    x = torch.zeros((2, 6, 3))
    m = torch.ones((2, 6))
    com = [md.Restraint(md.distance(md.center([0, 1]), md.center([2, 3])), 1.0, 0.1)]
    coord = [md.Restraint(md.coordination([0, 1], [2, 3], 1.5, r_max=4.0), 1.0, 0.1)]
    with pytest.raises(ValueError, match="RingPolymerDynamics does not support bias"):
        md.RingPolymerDynamics(None, sp, x, beads=4, temperature=300.0, masses=m, bias=com)
    with pytest.raises(ValueError, match="no virial"):
        md.BatchedDynamics(None, sp[:1], x[:1], torch.eye(3) * 20.0, (True, True, True), temperature=300.0, pressure=1.0,
                           masses=m[:1], bias=coord)
    for cv in (com[0].cv, coord[0].cv):
        with pytest.raises(ValueError, match="does not support sites"):
            geomopt.CVConstraints([cv])
    with pytest.raises(ValueError, match="padding atom: entry 1, atom 5"):
        md.BatchedDynamics(None, sp, x, masses=m, bias=[md.Restraint(md.distance(0, md.center([4, 5])), 1.0, 0.1)])
    with pytest.raises(ValueError, match="a periodic cell needs r_max"):
        md.BatchedDynamics(None, sp[:1], x[:1], torch.eye(3) * 20.0, (True, True, True), masses=m[:1],
                           bias=[md.Restraint(md.coordination([0], [1], 1.0), 1.0, 0.1)])
    with pytest.raises(ValueError, match="pass masses"):   # mass weights without masses or a model that knows the elements
        md.BatchedDynamics(None, sp, x, bias=com)
    T = torch.tensor([250.0, 300.0])
    for make in (lambda: md.BatchedDynamics(None, sp, x, masses=m, bias=com + coord),
                 lambda: md.ReplicaExchangeDynamics(None, sp[:1].repeat(2, 1), x, temperature=T, masses=m, bias=com)):
        with pytest.raises(ValueError, match="ROCm device"):
            make()


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------

CTYPES = {"int32_t": C.c_int32, "double": C.c_double}


def test_abi_is_declared_and_bound():
    from torchani_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "anihip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(anihip_[a-z_0-9]+)\s*\(", code))
    L = _lib.lib()
    for name in ("anihip_md_sites_workspace_bytes", "anihip_md_sites_gather", "anihip_md_sites_spread"):
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and getattr(L, name) is not None
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    assert "md_sites.hip" in _lib.SOURCES and "md_sums.h" in _lib.HEADERS
    assert re.search(r"#define\s+ANIHIP_ABI_VERSION\s+13\b", hdr) and _lib.ABI_VERSION == 13 and L.anihip_abi_version() == 13
    for name, value in (("MD_SITES_MAX", 64), ("MD_SITE_NONE", 0), ("MD_SITE_CENTER", 1), ("MD_SITE_ANCHOR", 2),
                        ("MD_SITE_VALUE", 3), ("MD_SITE_ROLE_CENTER", 0), ("MD_SITE_ROLE_A", 1), ("MD_SITE_ROLE_B", 2),
                        ("MD_SITES_BAD_SITE", 1), ("MD_SITES_BAD_GROUP", 2), ("MD_SITES_BAD_MEMBER", 4)):
        assert re.search(rf"#define\s+ANIHIP_{name}\s+{value}\b", hdr), name
        assert getattr(_lib, name) == value
    assert (_lib.MD_SITE_NONE, _lib.MD_SITE_CENTER, _lib.MD_SITE_ANCHOR, _lib.MD_SITE_VALUE) == (sr.NONE, sr.CENTER, sr.ANCHOR, sr.VALUE)
    assert (_lib.MD_SITE_ROLE_CENTER, _lib.MD_SITE_ROLE_A, _lib.MD_SITE_ROLE_B) == (sr.ROLE_CENTER, sr.ROLE_A, sr.ROLE_B)
    # the struct of the header, field for field with its types
    body = re.search(r"typedef struct \{([^}]*)\} anihip_md_sites;", code).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(int32_t|double)\s+(.*)$", decl, flags=re.S)
        assert m, decl
        for item in m.group(2).split(","):
            item = item.strip()
            arr = re.match(r"([a-z_]+)\[(\d+)\]$", item)
            if item.startswith("*"):
                fields.append((item[1:], C.c_void_p))
            elif arr:
                fields.append((arr.group(1), CTYPES[m.group(1)] * int(arr.group(2))))
            else:
                fields.append((item, CTYPES[m.group(1)]))
    assert [n for n, _ in fields] == [n for n, _ in _lib.MdSites._fields_]
    for (n, want), (_, have) in zip(fields, _lib.MdSites._fields_):
        assert C.sizeof(want) == C.sizeof(have) and (want is have or want._type_ is have._type_), n
    assert C.sizeof(_lib.MdSites) == 10 * 4 + 18 * 8 + 11 * C.sizeof(C.c_void_p)
    assert _lib.MdSites.cell.offset == 40 and _lib.MdSites.site_kind.offset == 184 and _lib.MdSites.status.offset == 264
    # the prototypes: the number of arguments bound is the number declared
    for name in ("anihip_md_sites_workspace_bytes", "anihip_md_sites_gather", "anihip_md_sites_spread"):
        args = re.search(rf"\b{name}\s*\(([^)]*)\)", code).group(1)
        assert len(args.split(",")) == len(getattr(L, name).argtypes), name
    assert L.anihip_md_sites_workspace_bytes.restype is C.c_size_t
    # unchanged: the structs of the calls in between
    assert C.sizeof(_lib.MdBias) == 6 * 4 + 17 * C.sizeof(C.c_void_p) and C.sizeof(_lib.MdParams) == 4 * 4 + 8 + 8 + 8
    # the block sum is included, not copied; the bias kernels and their CV header do not know about sites
    csrc = os.path.join(ROOT, "torchani_amd", "csrc")
    text = open(os.path.join(csrc, "md_sites.hip")).read()
    assert '#include "md_sums.h"' in text and "void md_block_sum" not in text and "atomicAdd" not in text
    for src in ("md_bias.hip", "md_cv.h"):
        assert "sites" not in open(os.path.join(csrc, src)).read().lower()


def test_host_visible_errors_return_before_any_launch():
    """Null pointers, V beyond 64 and a short workspace are refused on the host: no device is touched."""
    from torchani_amd import _lib

    L = _lib.lib()
    params = _lib.MdParams(2, 6, 0, 0, 1.0, 0, 0)
    one = C.c_void_p(8)   # (never followed: the calls return first)
    s = _lib.MdSites(2, 4, 1, 2, 1, 2, (C.c_int32 * 3)(0, 0, 0), 0, (C.c_double * 9)(), (C.c_double * 9)(),
                     *([8] * 11))
    assert L.anihip_md_sites_workspace_bytes(C.byref(params), C.byref(s)) == 8
    assert L.anihip_md_sites_gather(None, C.byref(params), C.byref(s), one, one, one, one, one, one, one, 4) != 0
    assert b"workspace holds 4 bytes, 8 needed" in L.anihip_last_error()
    assert L.anihip_md_sites_gather(None, C.byref(params), C.byref(s), one, None, one, one, one, one, one, 8) != 0
    assert L.anihip_md_sites_spread(None, C.byref(params), C.byref(s), one, one, None, one) != 0
    assert b"null pointer" in L.anihip_last_error()
    s.max_sites = 65
    assert L.anihip_md_sites_spread(None, C.byref(params), C.byref(s), one, one, one, one) != 0
    assert b"max_sites must be in 1 .. 64" in L.anihip_last_error()
    s.max_sites, s.status = 4, None
    assert L.anihip_md_sites_gather(None, C.byref(params), C.byref(s), one, one, one, one, one, one, one, 8) != 0
    s.status, s.n_entries = 8, 3
    assert L.anihip_md_sites_gather(None, C.byref(params), C.byref(s), one, one, one, one, one, one, one, 8) != 0
    assert b"site tables of 3 entries for a batch of 2" in L.anihip_last_error()
