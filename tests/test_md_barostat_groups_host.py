"""Molecular cell rescaling (the barostat with bond constraints), the parts that need no GPU: the two entry points in the
header, the export list and the ctypes prototypes; the identities of the reference (tests/_md_barostat_groups_ref.py); and the
NPT ideal gas of rigid bodies under the reference, whose volume follows the Gamma(N_g + 1) law of its N_g scaling groups."""
import os
import re

import numpy as np

import _md_barostat_groups_ref as gref
import _md_barostat_ref as bref
import _md_constraints_ref as cref
import _md_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RIGID_GAS_SEED = 7      # (test_gpu_md_barostat_groups.py runs the device with the same seed and step count)
RIGID_GAS_STEPS = 3000  # the smallest multiple of 1 000 at which the reference sits within a third of both gates


def test_symbols_are_declared_exported_and_have_prototypes():
    import ctypes as C

    from torchani_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "anihip.h")).read()
    src = open(os.path.join(ROOT, "torchani_amd", "csrc", "md.hip")).read()
    text = open(os.path.join(ROOT, "torchani_amd", "_lib.py")).read()
    assert re.search(r"#define\s+ANIHIP_ABI_VERSION\s+13\b", hdr) and _lib.ABI_VERSION == 13
    # stream, params, clusters, nine pointers; stream, params, two doubles, twelve pointers, clusters, three pointers
    want = {"anihip_md_group_terms": ["vp", "C.POINTER(MdParams)", "C.POINTER(MdClusters)"] + ["vp"] * 9,
            "anihip_md_barostat_groups": ["vp", "C.POINTER(MdParams)", "C.c_double", "C.c_double"] + ["vp"] * 12
            + ["C.POINTER(MdClusters)"] + ["vp"] * 3}
    for name, args in want.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr)
        assert name in _lib.EXPORTED_SYMBOLS
        assert re.search(r'extern "C" int ' + name + r"\(", src)
        if os.path.exists(_lib.LIB_PATH):   # the built library exports it (no GPU needed to look)
            assert getattr(C.CDLL(_lib.LIB_PATH), name) is not None
        m = re.search(r"L\." + name + r"\.argtypes = \[(.*?)\]", text, re.S)
        assert m is not None
        assert [a.strip() for a in m.group(1).replace("\n", " ").split(",")] == args
        decl = re.search(r"int " + name + r"\((.*?)\);", hdr, re.S).group(1)
        assert len(decl.split(",")) == len(args)
        assert re.search(r'for name in \([^)]*"' + name + r'"[^)]*\):\s*getattr\(L, name\)\.restype = C\.c_int', text)
    # the scratch size of the header and of the Python layer: [C][A][2] and [C][ceil(A / 256)][2] doubles
    assert "ANIHIP_MD_GROUP_SCRATCH_BYTES" in hdr
    assert _lib.md_group_scratch_bytes(3, 70) == 3 * (70 + 1) * 16 and _lib.md_group_scratch_bytes(2, 300) == 2 * (300 + 2) * 16
    assert _lib.md_group_scratch_bytes(1, 256) == 257 * 16 and _lib.md_group_scratch_bytes(1, 257) == 259 * 16


def test_batched_dynamics_takes_barostat_scaling():
    import inspect

    from torchani_amd.md import BatchedDynamics

    assert inspect.signature(BatchedDynamics.__init__).parameters["barostat_scaling"].default == "atomic"


def _case(seed=0):
    """3 molecules x 12 atoms: a dimer, a triangle, a 3-bond chain, free atoms, padding in molecule 1 and, in molecule 2, a
    dimer anchored on a fixed atom."""
    rs = np.random.RandomState(seed)
    Cn, A = 3, 12
    mols = [[(0, 1), (2, 3), (3, 4), (4, 2), (5, 6), (6, 7), (7, 8)]] * 2 + [[(0, 1), (2, 3), (3, 4), (4, 2), (10, 11)]]
    K = max(len(p) for p in mols)
    pairs = np.full((Cn, K, 2), -1, dtype=np.int64)
    for c, p in enumerate(mols):
        pairs[c, :len(p)] = p
    x = rs.uniform(-10.0, 10.0, (Cn, A, 3))
    for c in range(Cn):
        for i, j in mols[c]:
            if j > i:
                d = rs.normal(size=3)
                x[c, j] = x[c, i] + d / np.linalg.norm(d)
    active = np.ones((Cn, A), dtype=bool)
    active[1, 9:] = False    # padding
    active[2, 11] = False    # fixed: the anchor of (10, 11)
    mass = rs.choice([1.008, 12.011, 15.999], (Cn, A))
    at = np.arange(Cn)[:, None]
    lengths = np.linalg.norm(x[at, np.maximum(pairs[..., 0], 0)] - x[at, np.maximum(pairs[..., 1], 0)], axis=-1)
    cons = cref.Constraints(pairs, lengths, active, mass)
    v = cref.project_v(x, np.where(active[..., None], rs.normal(0.0, 0.01, (Cn, A, 3)), 0.0), cons)
    f = rs.normal(0.0, 0.05, (Cn, A, 3))
    cell = np.tile(np.eye(3) * 25.0, (Cn, 1, 1)) + rs.normal(scale=1.0, size=(Cn, 3, 3))
    return x, v, f, cell, active, mass, pairs, cons, rs


def _kinetic(v, active, mass):
    return 0.5 * (np.where(active, mass, 0.0)[..., None] * v ** 2).sum(axis=(1, 2)) / ref.ACC_UNIT


def test_no_clusters_is_the_atomic_barostat_to_the_bit():
    x, v, f, cell, active, mass, _, _, rs = _case()
    Cn = x.shape[0]
    K, W = _kinetic(v, active, mass), rs.normal(scale=0.01, size=(Cn, 3, 3))
    kT, p0, xi = np.full(Cn, 1e-3), np.full(Cn, 2e-5), rs.normal(size=Cn)
    Km, G = gref.group_terms(x, v, f, active, mass, None)
    assert np.array_equal(G, np.zeros(Cn)) and np.allclose(Km, K, rtol=1e-14)
    want = bref.barostat(x, v, cell, K, W, active, kT, p0, 2000.0, 100.0, 0.5, xi)
    got = gref.barostat_groups(x, v, cell, K, K, W, G, active, mass, None, kT, p0, 2000.0, 100.0, 0.5, xi)
    for a, b in zip(want, (got[0], got[1], got[2], got[3], got[5])):
        assert np.array_equal(a, b)
    assert np.array_equal(got[4], got[3])


def test_move_keeps_bonds_and_relative_velocities_and_its_kinetic_energy_is_that_of_the_moved_velocities():
    x, v, f, cell, active, mass, pairs, cons, rs = _case()
    Cn = x.shape[0]
    K, W = _kinetic(v, active, mass), rs.normal(scale=0.01, size=(Cn, 3, 3))
    Km, G = gref.group_terms(x, v, f, active, mass, cons)
    assert np.all(Km < K) and np.all(Km > 0.0) and np.all(G != 0.0)
    kT, p0 = np.full(Cn, 1e-3), np.full(Cn, 2e-5)
    x1, v1, cell1, K1, Km1, mu = gref.barostat_groups(x, v, cell, K, Km, W, G, active, mass, cons, kT, p0, 2000.0, 100.0, 0.5,
                                                      3.0 * rs.normal(size=Cn))
    assert np.abs(mu - 1.0).min() > 1e-4   # (a move worth checking)
    at = np.arange(Cn)[:, None]
    i, j = np.maximum(pairs[..., 0], 0), np.maximum(pairs[..., 1], 0)
    assert np.abs((x1[at, i] - x1[at, j]) - (x[at, i] - x[at, j])).max() <= 1e-13
    assert np.abs((v1[at, i] - v1[at, j]) - (v[at, i] - v[at, j])).max() <= 1e-13
    assert np.abs(K1 / _kinetic(v1, active, mass) - 1.0).max() <= 1e-12
    assert np.abs(Km1 / gref.group_terms(x1, v1, f, active, mass, cons)[0] - 1.0).max() <= 1e-12
    assert np.allclose(bref.volume(cell1), mu ** 3 * bref.volume(cell), rtol=1e-13)
    # free atoms are rescaled, group centres are rescaled, the anchored dimer and the inactive atoms stay
    assert np.allclose(x1[0, 9:], mu[0] * x[0, 9:], rtol=1e-15) and np.allclose(v1[0, 9:] * mu[0], v[0, 9:], rtol=1e-15)
    m = mass[0, 2:5]
    assert np.allclose((m[:, None] * x1[0, 2:5]).sum(0) / m.sum(), mu[0] * (m[:, None] * x[0, 2:5]).sum(0) / m.sum(), rtol=1e-13)
    assert np.array_equal(x1[2, 10:], x[2, 10:]) and np.array_equal(v1[2, 10:], v[2, 10:])
    assert np.array_equal(x1[1, 9:], x[1, 9:]) and np.array_equal(v1[1, 9:], v[1, 9:])


def test_molecular_virial_is_the_strain_derivative_with_rigid_groups():
    """For a pair energy E = sum phi(|x_i - x_j|) in free space, tr W = sum r phi' is the derivative under x -> (1 + e) x, and
    tr W + G that under X_q -> (1 + e) X_q with the groups translated rigidly: central differences of E itself, to 1e-7
    relative (truncation e^2 = 1e-10; rounding 1e-16 / e = 1e-11)."""
    x, v, _, cell, active, mass, pairs, cons, rs = _case(1)
    x = x[:1] * 0.3
    active, mass = active[:1], mass[:1]
    cons = cref.Constraints(pairs[:1], np.ones(pairs[:1].shape[:2]), active, mass)

    def energy(y):
        d = np.linalg.norm(y[0, :, None] - y[0, None, :] + np.eye(12)[..., None], axis=-1)
        return 0.5 * (np.exp(-0.3 * d) * (1.0 - np.eye(12))).sum()

    e = 1e-5
    grad = np.zeros_like(x)
    for i in range(12):
        for k in range(3):
            dx = np.zeros_like(x)
            dx[0, i, k] = e
            grad[0, i, k] = (energy(x + dx) - energy(x - dx)) / (2.0 * e)
    trW = (grad * x).sum()
    Km, G = gref.group_terms(x, np.zeros_like(x), -grad, active, mass, cons)

    def scaled(mu):
        # V = 1, K_mol = 0, tr W + G = -3 and P0 = 0 make P_int = 1 and d eps = beta_T: mu is what was asked for
        return gref.barostat_groups(x, np.zeros_like(x), np.eye(3)[None], np.zeros(1), np.zeros(1), np.zeros((1, 3, 3)),
                                    np.full(1, -3.0), active, mass, cons, np.zeros(1), np.zeros(1), 3.0 * np.log(mu), 1.0, 1.0,
                                    np.zeros(1))

    up, down = scaled(1.0 + e), scaled(1.0 - e)
    assert abs(up[5][0] - (1.0 + e)) < 1e-15
    fd = (energy(up[0]) - energy(down[0])) / (2.0 * e)
    assert abs(fd - (trW + G[0])) <= 1e-7 * abs(trW) and abs(G[0]) > 1e-2 * abs(trW)


def test_reference_samples_the_npt_ideal_gas_of_rigid_bodies():
    """64 replicas x 8 atoms: three rigid dimers and two free atoms, N_g = 5 scaling groups, kT / P0 = 1000 / (N_g + 1) A^3, the
    other parameters of test_reference_samples_the_npt_ideal_gas; zero forces and a zero virial; the first 400 steps dropped.
    The volume follows Gamma(N_g + 1) with scale kT / P0: <V> = (N_g + 1) kT / P0 (gate 3 %), Var V = (N_g + 1) (kT / P0)^2 (gate
    15 %).  Counting atoms instead of groups (atomic scaling, were it possible) gives (8 + 1) / (5 + 1): the mean moves by
    +50 %.  The full kinetic energy in place of the centre-of-mass one adds the dimers' six rotational degrees of freedom,
    2 kT / V in the pressure, and moves the mean by more than 10 % (measured: profiles/md_barostat_groups_tests.txt).  The step
    count is the smallest multiple of 1 000 at which seed 7 gives both ratios within a third of their gates, which the device
    test relies on."""
    setup = gref.rigid_gas_setup()
    assert setup["n_mol"] == 64 and setup["n_atoms"] == 8 and setup["n_groups"] == 5
    assert abs(setup["v_unit"] - 1000.0 / 6.0) < 1e-12 and setup["beta_T"] == 1.0 / setup["p0"]
    vol = gref.rigid_gas_volumes(RIGID_GAS_SEED, RIGID_GAS_STEPS, setup)
    mean, var = gref.rigid_gas_ratios(vol, setup, drop=400)
    print(f"md barostat groups reference, rigid-body ideal gas seed {RIGID_GAS_SEED}, {RIGID_GAS_STEPS} steps: "
          f"<V> / ((N_g+1) kT/P0) = {mean:.4f}, Var V / ((N_g+1) (kT/P0)^2) = {var:.4f}")
    assert abs(mean - 1.0) <= 0.03
    assert abs(var - 1.0) <= 0.15
    assert abs(mean - 1.0) <= 0.01 and abs(var - 1.0) <= 0.05   # what the choice of the step count rests on
