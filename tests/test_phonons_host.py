"""CPU checks of the phonon code: the identities of the fp64 reference of tests/_phonon_ref.py (what the GPU tests compare the
kernels with) on a random translation-invariant model, the device-independent parts of torchani_amd.phonons (supercell order,
minimum-image lattice vectors, compact pattern, band paths, Monkhorst-Pack meshes, thermodynamic limits), every argument
error, and the declarations of the C ABI."""
import math
import os
import re

import numpy as np
import pytest
import torch

import _phonon_ref as ref
from torchani_amd import phonons
from torchani_amd.tuples import BlockHessian, ForceConstants, PhononMesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("anihip_phonon_fold", "anihip_phonon_dynmat", "anihip_phonon_dos")


def _model(seed, n, repeats):
    tau, a, masses = ref.random_crystal(seed, n)
    index, blocks = ref.spring_blocks(n, repeats, ref.random_springs(seed + 1, n))
    return tau, a, masses, index, blocks


# ---- the reference's own identities ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("repeats", [(3, 2, 4), (1, 1, 1)])
def test_union_of_commensurate_spectra_is_the_supercell_spectrum(repeats):
    n = 3
    tau, a, masses, index, blocks = _model(5, n, repeats)
    N = n * int(np.prod(repeats))
    H = ref.dense(index, blocks, N)
    assert np.abs(H - H.T).max() == 0.0 and np.abs(H.reshape(3 * N, N, 3).sum(axis=1)).max() < 1e-13   # symmetric, sum rule
    w = 1.0 / np.sqrt(np.tile(np.repeat(masses, 3), N // n))
    want = np.linalg.eigvalsh(H * w[:, None] * w[None, :])
    c = ref.compact_from_blocks(index, blocks.astype(np.float64), tau, a, repeats)
    assert c["missing"].sum() == 0 and c["defect"].max() < 1e-14 * np.abs(c["phi"]).max()   # (fp64 rounding of the spring sums)
    D = ref.dynmat(c["phi"], c["nvec"], c["ent_b"], c["ent_bp"], masses, ref.commensurate_q(repeats))
    got = np.sort(np.linalg.eigvalsh(D).reshape(-1))
    assert np.abs(got - want).max() < 1e-12 * np.abs(want).max()


def test_dynmat_symmetries():
    repeats = (3, 3, 3)
    tau, a, masses, index, blocks = _model(8, 2, repeats)
    c = ref.compact_from_blocks(index, blocks, tau, a, repeats)
    q = np.random.RandomState(0).uniform(-0.5, 0.5, (6, 3))
    q[0] = 0.0
    D, dD = ref.dynmat(c["phi"], c["nvec"], c["ent_b"], c["ent_bp"], masses, q, c["rvec"])
    scale = ref.gershgorin(D)
    assert np.abs(D - D.conj().transpose(0, 2, 1)).max() < 1e-14 * scale                                # Hermitian
    assert np.abs(dD - dD.conj().transpose(0, 1, 3, 2)).max() < 1e-13 * scale * np.abs(a).max()
    Dm = ref.dynmat(c["phi"], c["nvec"], c["ent_b"], c["ent_bp"], masses, -q)
    assert np.abs(Dm - D.conj()).max() < 1e-14 * scale                                                  # D(-q) = conj D(q)
    G = np.array([1.0, -2.0, 3.0])
    DG = ref.dynmat(c["phi"], c["nvec"], c["ent_b"], c["ent_bp"], masses, q + G)
    assert np.abs(DG - D).max() < 1e-13 * scale                                                         # D(q + G) = D(q)
    assert np.abs(D[0].imag).max() == 0.0 and np.abs(np.linalg.eigvalsh(D[0])[:3]).max() < 1e-13 * scale   # Gamma: acoustic
    # the derivative against a central difference along k = 2 pi q inv(a)^T
    h = 1e-6
    for al in range(3):
        dk = np.zeros(3)
        dk[al] = h
        dq = dk @ a.T / (2 * np.pi)
        Dp = ref.dynmat(c["phi"], c["nvec"], c["ent_b"], c["ent_bp"], masses, q + dq)
        Dn = ref.dynmat(c["phi"], c["nvec"], c["ent_b"], c["ent_bp"], masses, q - dq)
        assert np.abs((Dp - Dn) / (2 * h) - dD[:, al]).max() < 1e-8 * scale * np.abs(a).max()


def test_closed_forms_of_the_reference():
    tau, a, masses, springs, k = ref.cubic_lattice()
    index, blocks = ref.spring_blocks(1, (3, 3, 3), springs)
    c = ref.compact_from_blocks(index, blocks, tau, a, (3, 3, 3))
    q = np.random.RandomState(1).uniform(-0.5, 0.5, (5, 3))
    D = ref.dynmat(c["phi"], c["nvec"], c["ent_b"], c["ent_bp"], masses, q)
    lam, _ = ref.cubic_closed_form(q, a[0, 0], masses[0], k)
    assert np.abs(np.linalg.eigvalsh(D) - np.sort(lam, axis=1)).max() < 1e-13
    tau, a, masses, springs = ref.diatomic_chain()
    index, blocks = ref.spring_blocks(2, (4, 1, 1), springs)
    c = ref.compact_from_blocks(index, blocks, tau, a, (4, 1, 1))
    q = np.array([[0.0, 0, 0], [0.17, 0.3, -0.2], [0.5, 0, 0]])
    ev = np.linalg.eigvalsh(ref.dynmat(c["phi"], c["nvec"], c["ent_b"], c["ent_bp"], masses, q))
    lo, hi = ref.chain_closed_form(q[:, 0], masses[0], masses[1], 0.7)
    assert np.abs(ev[:, :4]).max() < 1e-14 and np.abs(ev[:, 4] - lo).max() < 1e-14 and np.abs(ev[:, 5] - hi).max() < 1e-14


# ---- the device-independent parts of phonons ---------------------------------------------------------------------------------
def test_supercell_order_and_fp64_construction():
    rs = np.random.RandomState(3)
    n, repeats = 3, (2, 3, 2)
    # coordinates at which tau + l . a in float32 differs from the float64 sum rounded once
    tau = rs.uniform(0, 3, (1, n, 3)).astype(np.float32)
    a = (3.1 * np.eye(3) + 0.2 * rs.uniform(-1, 1, (3, 3))).astype(np.float32)
    sp = torch.tensor([[0, 3, 1]])
    sc = phonons._supercell(sp, torch.from_numpy(tau), torch.from_numpy(a), repeats)
    cl = ref.cells(repeats)
    assert sc.repeats == repeats and sc.species.shape == (1, 36) and sc.coordinates.dtype == torch.float32
    assert sc.species[0].tolist() == [0, 3, 1] * 12
    assert sc.basis.dtype == torch.int32 and sc.basis.tolist() == [0, 1, 2] * 12
    assert sc.lattice.dtype == torch.int32 and np.array_equal(sc.lattice.numpy(), np.repeat(cl, n, axis=0))
    for l in ((0, 0, 0), (1, 2, 1), (0, 1, 1)):   # noqa: E741
        for b in range(n):
            k = ((l[0] * 3 + l[1]) * 2 + l[2]) * n + b
            assert sc.lattice[k].tolist() == list(l) and int(sc.basis[k]) == b
    want = ref.supercell_positions(tau[0].astype(np.float64), a.astype(np.float64), repeats)
    assert np.array_equal(sc.coordinates[0].numpy(), want.astype(np.float32))
    assert np.array_equal(sc.cell.numpy(), (a.astype(np.float64) * np.array(repeats)[:, None]).astype(np.float32))
    assert sc.primitive_cell.dtype == torch.float64 and sc.primitive_coordinates.dtype == torch.float64
    with pytest.raises(ValueError, match="needs tensors on a ROCm device"):
        phonons.supercell(sp, torch.from_numpy(tau), torch.from_numpy(a), repeats)


def test_minimum_image_lattice_vectors_on_a_skewed_cell():
    rs = np.random.RandomState(6)
    n, repeats = 4, (2, 3, 1)
    a = np.array([[3.0, 0.0, 0.0], [2.1, 2.4, 0.0], [-1.3, 1.7, 2.8]])   # strongly skewed: rounding alone is not enough
    tau = rs.uniform(0, 1, (n, 3)) @ a
    N = n * 6
    b, j = np.repeat(np.arange(n), N), np.tile(np.arange(N), n)
    nv = ref.lattice_vectors(tau, a, repeats, b, j)
    cl = ref.cells(repeats)
    assert np.all((nv - cl[j // n]) % np.array(repeats) == 0)                                # an image of j
    d = tau[j % n] + nv.astype(np.float64) @ a - tau[b]
    d2 = (d * d).sum(-1)
    assert np.abs(d2 - ref.brute_force_lattice_vectors(tau, a, repeats, b, j)).max() < 1e-12   # the nearest one
    frac = np.linalg.solve(a.T, (tau[j % n] + cl[j // n] @ a - tau[b]).T).T / np.array(repeats)
    rounded = cl[j // n] - np.array(repeats) * np.rint(frac).astype(np.int64)
    assert (rounded != nv).any()                                                             # the search did change some
    got = phonons._lattice_vectors(torch.from_numpy(tau), torch.from_numpy(a), repeats, torch.from_numpy(b), torch.from_numpy(j))
    assert np.array_equal(got.numpy(), nv)
    # wide supercell: rounding the fractional supercell components is the minimum image already
    wide = (4, 4, 4)
    Nw = n * 64
    bw, jw = np.repeat(np.arange(n), Nw), np.tile(np.arange(Nw), n)
    nvw = ref.lattice_vectors(tau, a, wide, bw, jw)
    dw = tau[jw % n] + nvw.astype(np.float64) @ a - tau[bw]
    assert np.abs((dw * dw).sum(-1) - ref.brute_force_lattice_vectors(tau, a, wide, bw, jw, span=2)).max() < 1e-12


def test_equidistant_images_take_opposite_vectors_in_the_two_directions():
    """Atoms exactly half a supercell apart: the pair (b -> b', n) and its reverse (b' -> b, -n) stay a Hermitian pair."""
    n, repeats = 2, (2, 2, 1)
    a = np.diag([3.0, 3.0, 4.0])
    tau = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 2.0]])            # b' above b: the images in the next cell along x or y are tied
    N = n * 4
    b, j = np.repeat(np.arange(n), N), np.tile(np.arange(N), n)
    nv = ref.lattice_vectors(tau, a, repeats, b, j)
    cl = ref.cells(repeats)
    got = phonons._lattice_vectors(torch.from_numpy(tau), torch.from_numpy(a), repeats, torch.from_numpy(b), torch.from_numpy(j))
    assert np.array_equal(got.numpy(), nv)
    seen = {(int(bb), int(jj % n), tuple(v)) for bb, jj, v in zip(b, j, nv)}
    ties = 0
    for bb, jj, v in zip(b, j, nv):
        bp, lc = int(jj % n), int(jj // n)
        if bb == bp and lc == ref.cell_index(-cl[lc], repeats):
            continue                                              # its own mirror image: one entry, no partner
        assert (bp, int(bb), tuple(-v)) in seen
        d = tau[bp] + v @ a - tau[bb]
        ties += int(np.isclose((d * d).sum(), ((d - 2 * np.array([3.0, 0, 0]) * np.sign(d[0])) ** 2).sum()))
    assert ties > 0


def test_compact_pattern_matches_the_reference():
    repeats = (2, 1, 3)
    tau, a, masses, index, blocks = _model(11, 5, repeats)
    N = 5 * 6
    want = ref.compact_pattern(index, 5, N)
    got = phonons._compact_pattern(torch.from_numpy(index), 5, N)
    for g, w in zip(got, want):
        assert np.array_equal(g.numpy().astype(np.int64), w)
    b, j, boff, poff, diag = want
    assert np.all(np.diff((b * 5 + j % 5) * N + j) > 0) and boff[-1] == poff[-1] == len(b)
    assert np.all(j[diag] == np.arange(5))


def test_band_path():
    cell = torch.tensor([[3.0, 0, 0], [0.5, 4.0, 0], [0, 0, 5.0]], dtype=torch.float64)
    pts = [[0, 0, 0], [0.5, 0, 0], [0.5, 0.5, 0], [0, 0, 0]]
    q, length = phonons.band_path(pts, 4, cell=cell)
    assert q.shape == (13, 3) and q.dtype == torch.float64 and length.shape == (13,)
    assert q[0].tolist() == [0, 0, 0] and q[4].tolist() == [0.5, 0, 0] and q[8].tolist() == [0.5, 0.5, 0] and q[12].tolist() == [0, 0, 0]
    assert torch.allclose(q[1], torch.tensor([0.125, 0, 0], dtype=torch.float64), atol=0, rtol=0)
    recip = 2 * math.pi * np.linalg.inv(cell.numpy()).T
    seg = [np.linalg.norm((np.array(pts[s + 1]) - np.array(pts[s])) @ recip) for s in range(3)]
    assert abs(length[4].item() - seg[0]) < 1e-14 and abs(length[12].item() - sum(seg)) < 1e-13 and length[0].item() == 0.0
    assert torch.all(length[1:] > length[:-1])
    q2, l2 = phonons.band_path(pts[:2], 2)
    assert l2.tolist() == [0.0, 0.25, 0.5]
    for bad in ([[0, 0, 0]], [[0, 0], [1, 1]]):
        with pytest.raises(ValueError, match="points must be"):
            phonons.band_path(bad, 3)
    with pytest.raises(ValueError, match="n_per_segment"):
        phonons.band_path(pts, 0)


@pytest.mark.parametrize("mesh,shift", [((4, 4, 3), (0, 0, 0)), ((4, 3, 2), (1, 0, 1)), ((1, 1, 1), (0, 0, 0)), ((5, 1, 2), (1, 1, 1))])
def test_monkhorst_pack_weights_and_time_reversal(mesh, shift):
    q, w = phonons.monkhorst_pack(mesh, shift)
    assert abs(w.sum().item() - 1.0) < 1e-14 and q.dtype == w.dtype == torch.float64
    assert torch.all(q >= -0.5) and torch.all(q < 0.5)
    full = (ref.cells(mesh) + 0.5 * np.array(shift)) / np.array(mesh)
    key = lambda x: tuple(np.round(np.mod(np.asarray(x), 1.0) * 2 * np.array(mesh)).astype(int) % (2 * np.array(mesh)))   # noqa: E731
    kept = {key(x): float(wt) for x, wt in zip(q.numpy(), w.numpy())}
    assert len(kept) == len(q)
    total = np.prod(mesh)
    for x in full:
        k, km = key(x), key(-x)
        assert (k in kept) != (km in kept) or k == km           # exactly one of q and -q is kept
        wt = kept[k] if k in kept else kept[km]
        assert abs(wt * total - (1.0 if k == km else 2.0)) < 1e-12
    with pytest.raises(ValueError):
        phonons.monkhorst_pack((4, 0, 4))
    with pytest.raises(ValueError):
        phonons.monkhorst_pack((4, 4, 4), (2, 0, 0))


def _einstein_mesh(n=2, Q=3):
    lam = torch.tensor(np.random.RandomState(2).uniform(0.01, 0.4, (Q, 3 * n)))
    w = torch.tensor([0.5, 0.25, 0.25], dtype=torch.float64)[:Q]
    return PhononMesh(torch.zeros(Q, 3), w, lam.sqrt(), lam, "cm^-1")


def test_thermodynamics_limits_and_reference():
    pm = _einstein_mesh()
    n = 2
    th = pm.thermodynamics([0.0, 1e-3, 300.0, 1e7])
    e = ref.HBAR * ref.SQRT_MHESSIAN_TO_RAD_PER_FS * np.sqrt(pm.eigenvalues.numpy())
    zpe = 0.5 * (pm.weights.numpy()[:, None] * e).sum()
    assert abs(th.zero_point_energy.item() - zpe) < 1e-15 * zpe and th.n_imaginary == 0
    assert th.free_energy[0].item() == th.zero_point_energy.item() and th.entropy[0].item() == 0.0 and th.heat_capacity[0].item() == 0.0
    assert abs(th.free_energy[1].item() - zpe) < 1e-12 * zpe and th.entropy[1].item() < 1e-30       # F -> zero-point energy
    assert abs(th.heat_capacity[3].item() / (3 * n * ref.KB) - 1.0) < 1e-6                            # C_v -> 3 n k_B
    z, F, S, Cv, nim = ref.thermodynamics(pm.eigenvalues.numpy(), pm.weights.numpy(), [1e-3, 300.0, 1e7])
    assert np.allclose(th.free_energy[1:].numpy(), F, rtol=1e-12, atol=0) and np.allclose(th.entropy[1:].numpy(), S, rtol=1e-11, atol=1e-40)
    assert np.allclose(th.heat_capacity[1:].numpy(), Cv, rtol=1e-11, atol=1e-40)
    # S = -dF/dT and C_v = T dS/dT
    h = 1e-3
    t2 = pm.thermodynamics([300.0 - h, 300.0 + h])
    assert abs(-(t2.free_energy[1] - t2.free_energy[0]).item() / (2 * h) - th.entropy[2].item()) < 1e-7 * th.entropy[2].item()
    assert abs(300.0 * (t2.entropy[1] - t2.entropy[0]).item() / (2 * h) - th.heat_capacity[2].item()) < 1e-6 * th.heat_capacity[2].item()
    # imaginary and zero modes are left out and counted
    lam = pm.eigenvalues.clone()
    lam[0, 0], lam[1, 2] = -0.1, 0.0
    cut = PhononMesh(pm.q, pm.weights, lam.abs().sqrt() * torch.sign(lam), lam, "cm^-1").thermodynamics([300.0])
    assert cut.n_imaginary == 2 and cut.zero_point_energy.item() < th.zero_point_energy.item()
    with pytest.raises(ValueError, match="temperatures"):
        pm.thermodynamics([-1.0])


def test_unit_constants():
    from torchani_amd import md, units

    assert phonons.KB == md.KB_HARTREE == ref.KB and phonons.HBAR == ref.HBAR
    assert abs(phonons.SQRT_MHESSIAN_TO_RAD_PER_FS / ref.SQRT_MHESSIAN_TO_RAD_PER_FS - 1.0) < 1e-15
    # omega / (2 pi c) is the wavenumber units.sqrt_mhessian2invcm gives
    assert abs(phonons.SQRT_MHESSIAN_TO_RAD_PER_FS * 1e15 / units.SPEED_OF_LIGHT / 100.0 / units.SQRT_MHESSIAN_TO_INVCM - 1.0) < 1e-15


# ---- argument errors -----------------------------------------------------------------------------------------------------------
def _cpu_force_constants(exact):
    tau, a, masses, springs, _ = ref.cubic_lattice()
    index, blocks = ref.spring_blocks(1, (2, 2, 2), springs)
    c = ref.compact_from_blocks(index, blocks, tau, a, (2, 2, 2))
    t = torch.from_numpy
    return ForceConstants(t(a), t(tau), t(masses), (2, 2, 2), t(c["boff"]).int(), t(c["poff"]).int(), t(c["ent_b"]).int(),
                          t(c["ent_bp"]).int(), t(c["nvec"]).int(), t(c["rvec"]), t(c["phi"]), exact, 0.0, 0)


def test_value_errors():
    sp, x, cell = torch.tensor([[0, 1]]), torch.zeros(1, 2, 3), torch.eye(3) * 4
    for bad in ((0, 1, 1), (2, 2), (1, 1, -3), (1.5, 1, 1), None):
        with pytest.raises(ValueError, match="repeats must be three integers >= 1"):
            phonons.supercell(sp, x, cell, bad)
        with pytest.raises(ValueError, match="repeats must be three integers >= 1"):
            phonons.force_constants(None, sp, x, cell, bad)
    for pbc in ((True, True, False), torch.tensor([False, True, True])):
        with pytest.raises(ValueError, match="periodic along all three axes"):
            phonons.supercell(sp, x, cell, (1, 1, 1), pbc=pbc)
        with pytest.raises(ValueError, match="periodic along all three axes"):
            phonons.force_constants(None, sp, x, cell, (1, 1, 1), pbc=pbc)
    with pytest.raises(ValueError, match=r"masses must be \[n\] = \[2\]"):
        phonons.force_constants(None, sp, x, cell, (1, 1, 1), masses=torch.ones(3))
    sc = phonons._supercell(sp, x, cell, (2, 1, 1))
    H = BlockHessian(torch.zeros((2, 0), dtype=torch.int64), torch.zeros((0, 3, 3)), 1, 4)
    with pytest.raises(ValueError, match=r"masses must be \[n\] = \[2\]"):
        phonons.force_constants_from_hessian(H, sc, torch.ones(4))
    with pytest.raises(ValueError, match="1 molecule of 4 atoms"):
        phonons.force_constants_from_hessian(BlockHessian(H.index, H.blocks, 1, 6), sc, torch.ones(2))
    with pytest.raises(ValueError, match="needs tensors on a ROCm device"):   # all arguments on the device: no CPU fallback
        phonons.force_constants_from_hessian(H, sc, torch.ones(2))
    fc = _cpu_force_constants(exact=False)
    for bad in (torch.zeros(3), torch.zeros(2, 2), torch.zeros(0, 3), [[0.0, 0.0]], torch.zeros(1, 2, 3)):
        with pytest.raises(ValueError, match="q must be"):
            phonons.dynamical_matrices(fc, bad)
        with pytest.raises(ValueError, match="q must be"):
            phonons.modes(fc, bad)
    with pytest.raises(ValueError, match="exact only at q commensurate"):
        phonons.dynamical_matrices(fc, [[0.3, 0.0, 0.0]])
    with pytest.raises(ValueError, match="exact only at q commensurate"):
        phonons.modes(fc, [[0.5, 0.0, 0.0], [0.25, 0.5, 0.0]])
    # commensurate q, an aliasing waiver or an exact supercell get as far as the device check
    for f, q, kw in ((fc, [[0.5, 0.0, -0.5]], {}), (fc, [[0.3, 0.0, 0.0]], dict(allow_aliasing=True)),
                     (_cpu_force_constants(exact=True), [[0.3, 0.0, 0.0]], {})):
        with pytest.raises(ValueError, match="needs tensors on a ROCm device"):
            phonons.dynamical_matrices(f, q, **kw)
    with pytest.raises(ValueError, match="eigensolver"):
        phonons.modes(fc, [[0.0, 0.0, 0.0]], eigensolver="magma")
    with pytest.raises(ValueError, match="Only meV and cm"):
        phonons.modes(fc, [[0.0, 0.0, 0.0]], unit="THz")
    assert phonons.is_commensurate(torch.tensor([[0.5, 1 / 3, 0.25], [0.5, 0.3, 0.25]], dtype=torch.float64), (2, 3, 4)).tolist() == [True, False]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_abi_declarations():
    from torchani_amd import _lib

    with open(os.path.join(ROOT, "include", "anihip.h")) as f:
        hdr = f.read()
    declared = set(re.findall(r"\b(anihip_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    L = _lib.lib()
    for name in NEW:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and getattr(L, name) is not None
        assert getattr(L, name).restype is __import__("ctypes").c_int
        args = re.search(rf"\bint {name}\s*\(([^)]*)\)", hdr).group(1)
        assert len(args.split(",")) == len(getattr(L, name).argtypes), name
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    assert "phonons.hip" in _lib.SOURCES
    assert re.search(r"#define\s+ANIHIP_ABI_VERSION\s+13\b", hdr) and _lib.ABI_VERSION == 13 and L.anihip_abi_version() == 13
    # bad arguments come back nonzero before any launch (no device is touched: this runs without one)
    assert L.anihip_phonon_fold(None, 0, 1, 1, 1, None, None, None, 0, None, None, None, None, None, None, None) != 0
    assert L.anihip_phonon_fold(None, 1, 1, 0, 1, None, None, None, 0, None, None, None, None, None, None, None) != 0
    assert L.anihip_phonon_fold(None, 2, 1, 1, 1, None, None, None, 4, None, None, None, None, None, None, None) != 0
    assert L.anihip_phonon_fold(None, 2, 1, 1, 1, None, None, None, 0, None, None, None, None, None, None, None) == 0   # no entries
    assert L.anihip_phonon_dynmat(None, 1, 1, None, None, None, None, None, None, None, None) != 0
    assert L.anihip_phonon_dos(None, 0, None, None, 0.0, 1.0, 0.0, 4, None) != 0
    assert b"sigma" in L.anihip_last_error()
