"""CPU checks of biased MD: the reference of tests/_md_bias_ref.py (the fp64 restatement of include/anihip.h that the GPU tests
compare the kernels with) against autograd and finite differences, the table builder with every error it raises, what the
constructors refuse, and the declarations of the C ABI."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import _md_bias_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ------------------------------------------------------------------------------------------------------------

def _torch_cv(kind, x):
    """The definitions of include/anihip.h written for autograd."""
    if kind == br.DISTANCE:
        return (x[0] - x[1]).norm()
    if kind == br.ANGLE:
        a, b = x[0] - x[1], x[2] - x[1]
        return torch.atan2(torch.linalg.cross(a, b).norm(), a @ b)
    b1, b2, b3 = x[1] - x[0], x[2] - x[1], x[3] - x[2]
    n1, n2 = torch.linalg.cross(b1, b2), torch.linalg.cross(b2, b3)
    return torch.atan2(b2.norm() * (b1 @ n2), n1 @ n2)


def _bent(theta):
    """Three atoms with the angle theta at the middle one."""
    return np.array([[1.2, 0.0, 0.0], [0.0, 0.0, 0.0], [1.1 * math.cos(theta), 1.1 * math.sin(theta), 0.0]]) + 0.3


def _twisted(phi):
    """Four atoms with a dihedral of +-phi (the sign is the convention's: the test reads it back)."""
    return np.array([[-0.5, 1.0, 0.0], [0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [2.0, math.cos(phi), math.sin(phi)]]) - 0.2


def test_reference_gradients_match_autograd():
    rs = np.random.RandomState(3)
    cases = [(kind, rs.normal(0.0, 1.5, (br.N_ATOMS[kind], 3))) for kind in (0, 1, 2) for _ in range(6)]
    cases += [(br.ANGLE, _bent(math.radians(t))) for t in (20.0, 90.0, 160.0, 175.0)]
    cases += [(br.DIHEDRAL, _twisted(p)) for p in (math.pi - 0.03, -math.pi + 0.03, 0.02, -1.0)]
    worst = 0.0
    for kind, x in cases:
        s, g = br.cv(kind, x)
        xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        st = _torch_cv(kind, xt)
        st.backward()
        assert abs(s - float(st.detach())) <= 1e-14
        err = np.abs(g - xt.grad.numpy()).max() / max(1.0, np.abs(g).max())
        worst = max(worst, err)
        assert np.isfinite(g).all() and err <= 1e-12, (kind, err)
        assert np.abs(g.sum(axis=0)).max() <= 1e-12 * max(1.0, np.abs(g).max())   # translation invariance
    # the conventions: a straight-ish angle is near pi, the planar zigzag is trans = pi
    assert abs(br.cv(br.ANGLE, _bent(math.radians(175.0)))[0] - math.radians(175.0)) <= 1e-12
    assert br.cv(br.DIHEDRAL, np.array([[1.0, 1, 0], [1, 0, 0], [2, 0, 0], [2, -1, 0.0]]))[0] == math.pi
    both = sorted(br.cv(br.DIHEDRAL, _twisted(p))[0] for p in (math.pi - 0.03, -math.pi + 0.03))
    assert -math.pi < both[0] < -math.pi + 0.05 and math.pi - 0.05 < both[1] <= math.pi
    print(f"md bias reference: CV gradients against autograd, worst relative difference {worst:.1e}")


def test_reference_restraint_and_wrap():
    assert br.wrap(math.pi) == -math.pi and br.wrap(-math.pi) == -math.pi and br.wrap(0.25) == 0.25
    assert abs(br.wrap(2.0 * math.pi - 0.05) + 0.05) <= 1e-15
    # flat bottom: inside, on the edge, outside on both sides
    assert br.restraint(br.DISTANCE, 5.2, 5.0, 0.3, 0.5) == (0.0, 0.0)
    assert br.restraint(br.DISTANCE, 5.5, 5.0, 0.3, 0.5) == (0.0, 0.0)
    E, dE = br.restraint(br.DISTANCE, 6.0, 5.0, 0.3, 0.5)
    assert abs(E - 0.5 * 0.3 * 0.25) <= 1e-16 and abs(dE - 0.15) <= 1e-16
    E, dE = br.restraint(br.DISTANCE, 4.0, 5.0, 0.3, 0.5)
    assert abs(E - 0.5 * 0.3 * 0.25) <= 1e-16 and abs(dE + 0.15) <= 1e-16
    # a dihedral across the seam: pi - 0.03 seen from a centre at -pi + 0.02 is 0.05 below it
    E, dE = br.restraint(br.DIHEDRAL, math.pi - 0.03, -math.pi + 0.02, 2.0, 0.0)
    assert abs(E - 0.0025) <= 1e-15 and abs(dE + 0.1) <= 1e-14
    for s in np.linspace(-3.0, 3.0, 13):   # dE/ds is the derivative of E
        for kind in (br.ANGLE, br.DIHEDRAL):
            h = 1e-6
            num = (br.restraint(kind, s + h, 0.4, 0.7, 0.3)[0] - br.restraint(kind, s - h, 0.4, 0.7, 0.3)[0]) / (2 * h)
            assert abs(num - br.restraint(kind, s, 0.4, 0.7, 0.3)[1]) <= 1e-8


def test_reference_hills_derivative_matches_central_difference():
    rs = np.random.RandomState(5)
    n = 300
    centers = np.stack([rs.uniform(-math.pi, math.pi, n), rs.uniform(2.0, 4.0, n)])
    heights = rs.uniform(0.5e-3, 2e-3, n)
    is2 = np.array([1.0 / 0.35 ** 2, 1.0 / 0.2 ** 2])
    for nd, periodic in ((1, [True]), (2, [True, False]), (2, [False, False])):
        for s in ([math.pi - 0.01, 3.0], [-math.pi + 0.02, 2.5], [0.3, 3.7]):
            s = np.array(s[:nd])
            V, dV, scale = br.hills_sum(s, centers, heights, is2, periodic)
            assert V > 0 and scale[0] == V
            for d in range(nd):
                h = np.zeros(nd)
                h[d] = 1e-5
                num = (br.hills_sum(s + h, centers, heights, is2, periodic)[0]
                       - br.hills_sum(s - h, centers, heights, is2, periodic)[0]) / 2e-5
                assert abs(num - dV[d]) <= 1e-7 * scale[d + 1] + 1e-12, (nd, d, num, dV[d])
            if nd == 1:
                assert dV[1] == 0.0
    # across the seam the bias is continuous: a hill at pi - 0.01 acts on -pi + 0.01
    V, _, _ = br.hills_sum([-math.pi + 0.01], np.array([[math.pi - 0.01], [0.0]]), np.array([1.0]), is2, [True])
    assert abs(V - math.exp(-0.5 * 0.02 ** 2 * is2[0])) <= 1e-14


# ---- the table builder --------------------------------------------------------------------------------------------------------

def _species(Cn=3, A=6):
    sp = torch.zeros((Cn, A), dtype=torch.int64)
    sp[1, A - 1] = -1   # padding
    return sp


def test_tables_layout():
    from torchani_amd import _lib, md

    sp = _species()
    d01 = md.distance(0, 1)
    ang = md.angle(0, 1, torch.tensor([2, -1, 3]))
    dih = md.dihedral(0, 1, 2, 3)
    bias = [md.Restraint(d01, torch.tensor([1.5, 1.6, 1.7], dtype=torch.float64), 0.1), md.Restraint(ang, 1.0, 0.2, 0.1),
            md.Metadynamics([dih, d01], (0.1, 0.2), 0.001, 2, bias_factor=6.0, walkers=torch.tensor([5, -1, 5]), max_hills=64)]
    t = md.build_bias_tables(sp, None, bias, temperature=torch.full((3,), 300.0))
    assert t.cv_offset.tolist() == [0, 3, 5, 8] and t.cv_offset.dtype == torch.int32
    assert t.kind.tolist() == [0, 1, 2, 0, 2, 0, 1, 2]
    assert t.atoms.tolist() == [[0, 1, -1, -1], [0, 1, 2, -1], [0, 1, 2, 3], [6, 7, -1, -1], [6, 7, 8, 9], [12, 13, -1, -1],
                                [12, 13, 15, -1], [12, 13, 14, 15]]
    assert t.restraint[:, 0].tolist() == [1.5, 1.0, 0.0, 1.6, 0.0, 1.7, 1.0, 0.0]
    assert t.restraint[:, 1].tolist() == [0.1, 0.2, 0.0, 0.1, 0.0, 0.1, 0.2, 0.0]
    # the metadynamics CV that is the restraint's object shares its row; the dihedral got a row of its own, after the restraints
    assert t.meta_cv.tolist() == [[2, 0], [-1, -1], [2, 0]]
    assert t.list.tolist() == [0, -1, 0] and t.rank_in_list.tolist() == [0, 0, 1]
    assert t.members.tolist() == [2] and t.list_entry.tolist() == [0] and t.bias_factor.tolist() == [6.0]
    assert torch.allclose(t.inv_sigma2[0], torch.tensor([100.0, 25.0], dtype=torch.float64)) and t.inv_sigma2[1].tolist() == [0, 0]
    assert t.height.tolist() == [0.001, 0.0, 0.001] and t.capacity == 64 and t.pace == 2 and t.used.tolist() == [0]
    assert t.cv_index.tolist() == [[0, 1, 2], [3, -1, 4], [5, 6, 7]]
    # private lists in batch order; plain metadynamics; preloaded hills
    c0 = torch.arange(12, dtype=torch.float64).view(3, 1, 4)
    t = md.build_bias_tables(sp, None, [md.Metadynamics(dih, 0.3, 0.002, 0, hills=(c0, c0[:, 0] + 1, torch.tensor([4, 0, 2])))])
    assert t.list.tolist() == [0, 1, 2] and t.members.tolist() == [1, 1, 1] and t.bias_factor.tolist() == [0.0, 0.0, 0.0]
    assert t.used.tolist() == [4, 0, 2] and tuple(t.centers.shape) == (3, 2, 4) and t.centers[1, 0].tolist() == [4, 5, 6, 7]
    assert t.centers[:, 1].abs().max() == 0 and t.heights[2].tolist() == [9, 10, 11, 12] and t.pace == 0
    # a bias without a CV anywhere: empty tables
    t = md.build_bias_tables(sp, None, [md.Restraint(md.distance(torch.full((3,), -1), 1), 1.0, 1.0)])
    assert t.kind.numel() == 0 and t.cv_offset.tolist() == [0, 0, 0, 0] and t.members.numel() == 0
    assert _lib.MD_BIAS_MAX_CVS == br.MAX_CVS == 16


BAD = [
    ("0 .. 5", lambda md: [md.Restraint(md.distance(0, 6), 1.0, 1.0)]),
    ("entry 2, distance of atoms \\(0, 7\\)", lambda md: [md.Restraint(md.distance(0, torch.tensor([1, 1, 7])), 1.0, 1.0)]),
    ("entry 0, angle of atoms \\(0, -2, 1\\)", lambda md: [md.Restraint(md.angle(0, torch.tensor([-2, 1, 1]), 1), 1.0, 1.0)]),
    ("padding atom: entry 1, distance of atoms \\(0, 5\\)", lambda md: [md.Restraint(md.distance(0, 5), 1.0, 1.0)]),
    ("4 different atoms: entry 1, dihedral of atoms \\(0, 1, 2, 1\\)",
     lambda md: [md.Restraint(md.dihedral(0, 1, 2, torch.tensor([3, 1, 3])), 1.0, 1.0)]),
    ("entry 0 has 17 CVs, more than 16", lambda md: [md.Restraint(md.distance(0, 1), 1.0, 1.0) for _ in range(17)]),
    ("one or two CVs", lambda md: [md.Metadynamics([md.distance(0, 1), md.distance(0, 2), md.distance(0, 3)], 0.1, 1e-3, 1)]),
    ("at most one Metadynamics", lambda md: [md.Metadynamics(md.distance(0, 1), 0.1, 1e-3, 1),
                                             md.Metadynamics(md.distance(0, 2), 0.1, 1e-3, 1)]),
    ("sigma must be > 0: entry 0", lambda md: [md.Metadynamics(md.distance(0, 1), 0.0, 1e-3, 1)]),
    ("sigma must be > 0: entry 2", lambda md: [md.Metadynamics(md.distance(0, 1), torch.tensor([0.1, 0.1, -0.1]), 1e-3, 1)]),
    ("height must be >= 0", lambda md: [md.Metadynamics(md.distance(0, 1), 0.1, -1e-3, 1)]),
    ("k must be >= 0: entry 1", lambda md: [md.Restraint(md.distance(0, 1), 1.0, torch.tensor([0.0, -0.5, 1.0]))]),
    ("half_width must be >= 0", lambda md: [md.Restraint(md.distance(0, 1), 1.0, 1.0, -0.1)]),
    ("pace must be an integer >= 0", lambda md: [md.Metadynamics(md.distance(0, 1), 0.1, 1e-3, -1)]),
    ("bias_factor must be > 1", lambda md: [md.Metadynamics(md.distance(0, 1), 0.1, 1e-3, 1, bias_factor=1.0)]),
    ("needs a temperature", lambda md: [md.Metadynamics(md.distance(0, 1), 0.1, 1e-3, 1, bias_factor=6.0)]),
    ("agree in sigma", lambda md: [md.Metadynamics(md.distance(0, 1), torch.tensor([0.1, 0.1, 0.2]), 1e-3, 1,
                                                   walkers=torch.tensor([0, 1, 0]))]),
    ("walker of list 4 but does not have", lambda md: [md.Metadynamics(md.distance(0, torch.tensor([1, -1, 1])), 0.1, 1e-3, 1,
                                                                      walkers=torch.tensor([4, 4, -1]))]),
    ("walkers must be an int64 tensor of shape \\(3,\\)", lambda md: [md.Metadynamics(md.distance(0, 1), 0.1, 1e-3, 1,
                                                                                    walkers=torch.tensor([0, 1]))]),
    ("hills must be centers \\[3, 1, H\\]", lambda md: [md.Metadynamics(md.distance(0, 1), 0.1, 1e-3, 1,
                                                                        hills=(torch.zeros(2, 1, 4), torch.zeros(2, 4)))]),
    ("more than max_hills = 8", lambda md: [md.Metadynamics(md.distance(0, 1), 0.1, 1e-3, 1, max_hills=8,
                                                            hills=(torch.zeros(3, 1, 9), torch.zeros(3, 9)))]),
    ("used counts", lambda md: [md.Metadynamics(md.distance(0, 1), 0.1, 1e-3, 1,
                                                hills=(torch.zeros(3, 1, 4), torch.zeros(3, 4), torch.tensor([1, 5, 0])))]),
    ("center must be", lambda md: [md.Restraint(md.distance(0, 1), torch.zeros(2), 1.0)]),
    ("same CV twice", lambda md: [md.Metadynamics([md.distance(0, 1)] * 2, 0.1, 1e-3, 1)]),
]


@pytest.mark.parametrize("case", range(len(BAD)))
def test_builder_errors_name_the_entry_and_the_atoms(case):
    """(Walkers of one list agree in the kinds of their CVs by construction: a CV object has one kind for every entry.)"""
    from torchani_amd import md

    message, make = BAD[case]
    with pytest.raises(ValueError, match=message):
        md.build_bias_tables(_species(), None, make(md))


def test_index_types_are_checked_where_the_cv_is_made():
    from torchani_amd import md

    for bad in (1.0, True, torch.tensor([0, 1], dtype=torch.int32), torch.zeros((2, 2), dtype=torch.int64)):
        with pytest.raises(ValueError, match="int or an int64 tensor"):
            md.distance(0, bad)
    with pytest.raises(ValueError, match="shape \\(3,\\)"):
        md.build_bias_tables(_species(), None, [md.Restraint(md.distance(0, torch.tensor([1, 2])), 1.0, 1.0)])
    with pytest.raises(ValueError, match="needs a CV"):
        md.Restraint((0, 1), 1.0, 1.0)
    cv = md.dihedral(0, 1, 2, torch.tensor([3, 4, 5]))
    assert isinstance(cv, md.CV) and cv.kind == 2 and len(cv.atoms) == 4 and md.angle(0, 1, 2).kind == 1


def test_constructors_refuse_before_they_need_a_device():
    """Every check of the bias is host work in front of the "needs a ROCm device" check: CPU tensors reach all of it."""
    from torchani_amd import md

    sp = _species()
    x = torch.zeros((3, 6, 3))
    rest = [md.Restraint(md.distance(0, 1), 1.0, 0.1)]
    meta = [md.Metadynamics(md.distance(0, 1), 0.1, 1e-3, 2)]
    T = torch.tensor([250.0, 300.0, 360.0])
    with pytest.raises(ValueError, match="RingPolymerDynamics does not support bias"):
        md.RingPolymerDynamics(None, sp, x, beads=4, temperature=300.0, bias=rest)
    with pytest.raises(ValueError, match="no virial"):
        md.BatchedDynamics(None, sp[:1], x[:1], torch.eye(3) * 20.0, (True, True, True), temperature=300.0, pressure=1.0,
                           bias=rest)
    with pytest.raises(ValueError, match="does not support Metadynamics"):
        md.ReplicaExchangeDynamics(None, sp[::2], x[::2], temperature=T[:2], bias=meta)
    with pytest.raises(ValueError, match="padding atom: entry 1"):
        md.BatchedDynamics(None, sp, x, bias=[md.Restraint(md.distance(0, 5), 1.0, 0.1)])
    with pytest.raises(ValueError, match="needs a temperature"):
        md.BatchedDynamics(None, sp, x, bias=[md.Metadynamics(md.distance(0, 1), 0.1, 1e-3, 2, bias_factor=6.0)])
    # a valid bias passes every host check and stops at the device check, restraints in a ladder included
    for make in (lambda: md.BatchedDynamics(None, sp, x, bias=rest + meta),
                 lambda: md.ReplicaExchangeDynamics(None, sp[::2], x[::2], temperature=T[:2], bias=rest)):
        with pytest.raises(ValueError, match="ROCm device"):
            make()


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------

def test_abi_is_declared_and_bound():
    from torchani_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "anihip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(anihip_[a-z_0-9]+)\s*\(", code))
    L = _lib.lib()
    for name in ("anihip_md_bias_workspace_bytes", "anihip_md_bias_apply", "anihip_md_bias_deposit", "anihip_md_bias_hills"):
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and getattr(L, name) is not None
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    assert "md_bias.hip" in _lib.SOURCES and "md.hip" in _lib.SOURCES and "md_sums.h" in _lib.HEADERS
    assert re.search(r"#define\s+ANIHIP_ABI_VERSION\s+13\b", hdr) and _lib.ABI_VERSION == 13
    for name, value in (("MD_BIAS_MAX_CVS", 16), ("MD_BIAS_CHUNK", _lib.MD_BIAS_CHUNK), ("MD_CV_DISTANCE", 0), ("MD_CV_ANGLE", 1),
                        ("MD_CV_DIHEDRAL", 2), ("MD_BIAS_BAD_OFFSET", 1), ("MD_BIAS_BAD_CV", 2), ("MD_BIAS_BAD_LIST", 4)):
        assert re.search(rf"#define\s+ANIHIP_{name}\s+{value}\b", hdr), name
        assert getattr(_lib, name) == value
    assert (_lib.MD_CV_DISTANCE, _lib.MD_CV_ANGLE, _lib.MD_CV_DIHEDRAL) == (br.DISTANCE, br.ANGLE, br.DIHEDRAL)
    assert _lib.MD_BIAS_CHUNK % 256 == 0   # whole passes of the 256 threads of a workgroup
    # the struct of the header, field for field: six int32, then seventeen pointers
    body = re.search(r"typedef struct \{([^}]*)\} anihip_md_bias;", code).group(1)
    names = re.findall(r"\*?\b([a-z_A-Z0-9]+)\s*[,;]", body)
    assert names == [n for n, _ in _lib.MdBias._fields_]
    ints = re.findall(r"^\s*int32_t\s+([^*;]+);", body, flags=re.M)
    assert sum(len(line.split(",")) for line in ints) == 6
    assert C.sizeof(_lib.MdBias) == 6 * 4 + 17 * C.sizeof(C.c_void_p)
    assert _lib.MdBias.cv_offset.offset == 24 and _lib.MdBias.n_entries.offset == 20 and _lib.MdBias.status.offset == 24 + 16 * 8
    assert C.sizeof(_lib.MdParams) == 4 * 4 + 8 + 8 + 8   # unchanged
    # the block sum lives in one header that both sources include
    csrc = os.path.join(ROOT, "torchani_amd", "csrc")
    assert "md_block_sum(double" in open(os.path.join(csrc, "md_sums.h")).read()
    for src in ("md.hip", "md_bias.hip"):
        text = open(os.path.join(csrc, src)).read()
        assert '#include "md_sums.h"' in text and "void md_block_sum" not in text
