"""The stochastic-cell-rescaling barostat of the device integrator, the parts that need no GPU: the entry point in the header,
the export list and the ctypes prototypes; the noise word of the reference (tests/_md_barostat_ref.py); the pressure unit; and
the NPT ideal gas under the reference, whose volume follows the Gamma(N + 1) law."""
import os
import re

import numpy as np

import _md_barostat_ref as bref
import _md_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDEAL_GAS_SEED = 7   # (test_gpu_md_barostat.py runs the device with the same seed)


def test_symbol_is_declared_exported_and_has_a_prototype():
    import ctypes as C

    from torchani_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "anihip.h")).read()
    assert re.search(r"\bint\s+anihip_md_barostat\s*\(", hdr)
    assert re.search(r"#define\s+ANIHIP_MD_BAROSTAT_STEP\s+\(1ull << 62\)", hdr)
    assert "anihip_md_barostat" in _lib.EXPORTED_SYMBOLS
    assert _lib.MD_BAROSTAT_STEP == bref.BAROSTAT_STEP == 1 << 62
    assert re.search(r"#define\s+ANIHIP_ABI_VERSION\s+13\b", hdr) and _lib.ABI_VERSION == 13
    src = open(os.path.join(ROOT, "torchani_amd", "csrc", "md.hip")).read()
    assert re.search(r'extern "C" int anihip_md_barostat\(', src)
    if os.path.exists(_lib.LIB_PATH):   # the built library exports it (no GPU needed to look)
        fn = C.CDLL(_lib.LIB_PATH).anihip_md_barostat
        assert fn is not None
    # the prototype: stream, params, two doubles, twelve pointers; an int status
    text = open(os.path.join(ROOT, "torchani_amd", "_lib.py")).read()
    m = re.search(r"L\.anihip_md_barostat\.argtypes = \[(.*?)\]", text, re.S)
    assert m is not None
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert args[:4] == ["vp", "C.POINTER(MdParams)", "C.c_double", "C.c_double"] and args[4:] == ["vp"] * 12
    decl = re.search(r"int anihip_md_barostat\((.*?)\);", hdr, re.S).group(1)
    assert len(decl.split(",")) == len(args)
    assert re.search(r'for name in \([^)]*"anihip_md_barostat"[^)]*\):\s*getattr\(L, name\)\.restype = C\.c_int', text)


def test_batched_dynamics_takes_the_barostat_arguments():
    import inspect

    from torchani_amd.geomopt import ModelEvaluator
    from torchani_amd.md import BatchedDynamics

    p = inspect.signature(BatchedDynamics.__init__).parameters
    assert p["pressure"].default is None
    assert p["compressibility"].default == 4.57e-5 and p["barostat_time"].default == 1000.0
    assert inspect.signature(ModelEvaluator.__init__).parameters["stress"].default is False
    assert hasattr(BatchedDynamics, "volumes") and hasattr(BatchedDynamics, "pressures")


def test_noise_word_is_disjoint_from_drift_and_maxwell_boltzmann_words():
    for step in (0, 1, 12345, (1 << 62) - 1):
        w = bref.noise_word(step)
        assert w >> 62 == 1                      # bit 62 set, bit 63 clear
        assert w & ((1 << 62) - 1) == step
        assert not step >> 62                    # a drift's word has neither
        assert (ref.MB_STEP | step) >> 63 == 1   # a Maxwell-Boltzmann draw's has bit 63
    # and the draws differ: the barostat's variate is not the drift's xi_x of atom 0
    seed = 99
    drift = ref.noise(seed, 5, 4, 1)[:, 0, 0]
    baro = bref.barostat_noise(seed, 5, 4)
    mb = ref.noise(seed, ref.MB_STEP | 5, 4, 1)[:, 0, 0]
    assert not np.any(drift == baro) and not np.any(mb == baro)
    # the variate follows the replica id, not the place in the batch
    assert np.array_equal(bref.barostat_noise(seed, 5, 4, [3, 1, 0, 2]), baro[[3, 1, 0, 2]])


def test_bar_conversion_constant():
    from torchani_amd.md import BAR_PER_HARTREE_ANGSTROM3

    hartree_J, angstrom_m, bar_Pa = 4.3597447222071e-18, 1e-10, 1e5   # CODATA 2018
    want = hartree_J / angstrom_m ** 3 / bar_Pa
    assert abs(BAR_PER_HARTREE_ANGSTROM3 / want - 1.0) < 1e-14
    assert BAR_PER_HARTREE_ANGSTROM3 == bref.BAR_PER_HARTREE_ANGSTROM3 == 4.3597447222071e7
    # water's compressibility, 4.57e-5 / bar, is about 2.0e3 Angstrom^3 / Hartree
    assert abs(4.57e-5 * BAR_PER_HARTREE_ANGSTROM3 - 1992.4) < 0.1


def test_move_scales_everything_consistently():
    rs = np.random.RandomState(0)
    Cn, A = 3, 5
    x, v = rs.normal(size=(Cn, A, 3)), rs.normal(size=(Cn, A, 3))
    cell = np.tile(np.eye(3) * 10.0, (Cn, 1, 1)) + rs.normal(scale=0.5, size=(Cn, 3, 3))
    active = np.ones((Cn, A), dtype=bool)
    active[1, 3:] = False
    K, W = rs.uniform(0.01, 0.02, Cn), rs.normal(scale=0.01, size=(Cn, 3, 3))
    kT, p0 = np.full(Cn, 1e-3), np.full(Cn, 2e-5)
    x1, v1, cell1, K1, mu = bref.barostat(x, v, cell, K, W, active, kT, p0, 2000.0, 100.0, 0.5, rs.normal(size=Cn))
    assert np.allclose(bref.volume(cell1), mu ** 3 * bref.volume(cell), rtol=1e-13)
    assert np.allclose(K1 * mu ** 2, K, rtol=1e-14)
    assert np.array_equal(x1[~active], x[~active]) and np.array_equal(v1[~active], v[~active])
    assert np.allclose(x1[active], (mu[:, None, None] * x)[active]) and np.allclose((v1 * mu[:, None, None])[active], v[active])
    # without noise, at P_int = P0, nothing moves; above P0 the box grows
    V = bref.volume(cell)
    p_int = (2.0 * K - np.trace(W, axis1=1, axis2=2)) / (3.0 * V)
    assert np.allclose(bref.barostat(x, v, cell, K, W, active, kT, p_int, 2000.0, 100.0, 0.5, np.zeros(Cn))[4], 1.0, rtol=1e-15)
    assert np.all(bref.barostat(x, v, cell, K, W, active, kT, p_int - 1e-5, 2000.0, 100.0, 0.5, np.zeros(Cn))[4] > 1.0)


def test_reference_samples_the_npt_ideal_gas():
    """64 replicas x 8 atoms, beta_T = 1 / P0, dt / tau_p = 0.02, gamma dt = 0.1, 4 000 steps with the first 400 dropped: the
    volume follows Gamma(N + 1) with scale kT / P0, so <V> = (N + 1) kT / P0 (gate 3 %) and Var V = (N + 1) (kT / P0)^2 (gate
    15 %).  A wrong count of degrees of freedom or a kT / V term in the equation of ln V moves the mean by 11 % or more at
    N = 8.  Seed 7 gives 1.0011 and 0.981, inside half of each gate, which the device test relies on."""
    setup = bref.ideal_gas_setup()
    assert abs(setup["dt"] / setup["tau_p"] - 0.02) < 1e-15 and abs(setup["friction"] * setup["dt"] - 0.1) < 1e-15
    assert setup["beta_T"] == 1.0 / setup["p0"] and setup["n_mol"] == 64 and setup["n_atoms"] == 8
    vol = bref.ideal_gas_volumes(IDEAL_GAS_SEED, 4000, setup)
    mean, var = bref.ideal_gas_ratios(vol, setup, drop=400)
    print(f"md barostat reference, ideal gas seed {IDEAL_GAS_SEED}: <V> / ((N+1) kT/P0) = {mean:.4f}, "
          f"Var V / ((N+1) (kT/P0)^2) = {var:.4f}")
    assert abs(mean - 1.0) <= 0.03
    assert abs(var - 1.0) <= 0.15
    assert abs(mean - 1.0) <= 0.015 and abs(var - 1.0) <= 0.075   # what the device test's choice of seed rests on
