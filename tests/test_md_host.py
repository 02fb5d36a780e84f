"""Host-side parts of the on-device MD integrator (no GPU): the fp64 reference of the GPU tests (tests/_md_ref.py) against
known answers and the properties it must have, argument validation of BatchedDynamics before any device work, and the
library's exports."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _md_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 2024   # of the moment test: any seed passes a 5 sigma gate with probability 1 - 1e-6; this one was checked


@pytest.mark.parametrize("counter, key, out", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, out):
    got = ref.philox4x32_10(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))
    assert tuple(int(w) for w in got) == out


def test_uniform_is_exact_in_fp32_and_open():
    u = np.array([0, 511, 512, 0xFFFFFFFF], dtype=np.uint32)
    p = ref.uniform(u)
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    assert p[0] == p[1] == 2.0 ** -24 and p[2] == 1.5 * 2.0 ** -23 and p[3] == 1.0 - 2.0 ** -24


def test_reference_noise_moments():
    xi = np.concatenate([ref.noise(SEED, s, 64, 64).ravel() for s in range(16)])
    n = xi.size
    assert n == 196608
    assert abs(xi.mean()) <= 5.0 / np.sqrt(n)
    assert abs(xi.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n)
    # the three components of an atom are uncorrelated (x and y share a radius, z is drawn apart)
    c = np.corrcoef(ref.noise(SEED, 3, 64, 64).reshape(-1, 3).T)
    assert np.abs(c - np.eye(3)).max() <= 5.0 / np.sqrt(64 * 64)


def test_reference_noise_follows_the_replica_not_the_batch_position():
    big = ref.noise(7, 5, 6, 10, replica_ids=[4, 9, 0, 2, 11, 3])
    small = ref.noise(7, 5, 2, 10, replica_ids=[11, 9])
    assert np.array_equal(small[0], big[4]) and np.array_equal(small[1], big[1])
    assert np.array_equal(ref.noise(7, 5, 3, 10)[2], ref.noise(7, 5, 1, 10, replica_ids=[2])[0])
    # a molecule of fewer atoms draws the same noise for the atoms it has; another step or seed draws other noise
    assert np.array_equal(ref.noise(7, 5, 3, 4), ref.noise(7, 5, 3, 10)[:, :4])
    assert not np.array_equal(ref.noise(7, 6, 3, 4), ref.noise(7, 5, 3, 4))
    assert not np.array_equal(ref.noise(7 + (1 << 32), 5, 3, 4), ref.noise(7, 5, 3, 4))
    assert not np.array_equal(ref.noise(7, 5 + (1 << 32), 3, 4), ref.noise(7, 5, 3, 4))


def test_reference_baoab_conserves_the_shadow_energy_of_an_oscillator():
    """With friction 0 the BAOAB step is velocity Verlet, which on f = -k x conserves exactly
    1/2 m v^2 + 1/2 k x^2 (1 - (omega dt)^2 / 4), omega^2 = k / m, while the energy itself oscillates at order (omega dt)^2."""
    m, k, dt = 1.008, 0.35, 0.5   # amu, Hartree / Angstrom^2, fs
    w2 = k * ref.ACC_UNIT / m
    x = np.array([[[0.1, 0.0, 0.0]]])
    v = np.array([[[0.0, 0.0, 0.0]]])
    mass, act = np.array([[m]]), np.array([[True]])
    xi = np.ones((1, 1, 3))   # multiplied by sigma = 0

    def energies(x, v):
        ke = 0.5 * m * v[0, 0, 0] ** 2 / ref.ACC_UNIT
        return ke + 0.5 * k * x[0, 0, 0] ** 2, ke + 0.5 * k * x[0, 0, 0] ** 2 * (1.0 - w2 * dt * dt / 4.0)

    e0, s0 = energies(x, v)
    de = ds = 0.0
    for _ in range(400):
        x, v = ref.drift(x, v, -k * x, act, mass, dt, langevin=True, kT=np.array([1e-3]), friction=np.array([0.0]), xi=xi)
        v, ke = ref.kick(v, -k * x, act, mass, dt)
        e, s = energies(x, v)
        assert ke[0] == pytest.approx(0.5 * m * v[0, 0, 0] ** 2 / ref.ACC_UNIT, rel=1e-14)
        de, ds = max(de, abs(e - e0)), max(ds, abs(s - s0))
    assert ds <= 1e-12 * e0
    assert de >= 1e-3 * e0   # (omega dt)^2 / 4 = 5.7e-3: the plain energy is not what the scheme conserves


def test_reference_thermostat_step_is_exact_ornstein_uhlenbeck():
    """Zero force: the velocity after one step is c1 v + sigma xi with sigma^2 = kT (1 - c1^2) / m, whatever dt."""
    kT, g, dt = np.array([ref.KB_HARTREE * 300.0]), np.array([0.5]), 1.0
    mass, act = np.array([[12.011, 1.008]]), np.array([[True, False]])
    v0 = np.array([[[0.01, -0.02, 0.03], [9.0, 9.0, 9.0]]])
    xi = ref.noise(1, 0, 1, 2)
    x1, v1 = ref.drift(np.zeros((1, 2, 3)), v0, np.zeros((1, 2, 3)), act, mass, dt, True, kT, g, xi)
    c1 = np.exp(-0.5)
    want = c1 * v0[0, 0] + np.sqrt(kT[0] * (1 - c1 * c1) * ref.ACC_UNIT / 12.011) * xi[0, 0]
    assert np.allclose(v1[0, 0], want, rtol=1e-14)
    assert np.allclose(x1[0, 0], 0.5 * dt * (v0[0, 0] + want), rtol=1e-14)
    assert np.all(v1[0, 1] == 0.0) and np.all(x1[0, 1] == 0.0)   # the inactive atom


def _cpu_inputs():
    return torch.zeros((2, 3), dtype=torch.long), torch.zeros((2, 3, 3))


@pytest.mark.parametrize("kw, match", [
    ({"dt": 0.0}, "dt"), ({"dt": -0.5}, "dt"), ({"friction": -0.1}, "friction"),
    ({"friction": torch.tensor([0.1, -0.1])}, "friction"), ({"friction": torch.ones(3)}, "friction"),
    ({"temperature": -1.0}, "temperature"), ({"temperature": torch.ones(5)}, "temperature"),
    ({"fixed": torch.zeros(3, dtype=torch.bool)}, "fixed"), ({"masses": torch.ones(2)}, "masses"),
    ({"replica_ids": torch.zeros(3, dtype=torch.long)}, "replica_ids"), ({"replica_ids": torch.tensor([0, -1])}, "replica_ids"),
    ({"replica_ids": torch.tensor([1, 1 << 32])}, "replica_ids"), ({"seed": -1}, "seed"), ({"seed": 1 << 64}, "seed"),
])
def test_bad_arguments_raise_before_device_work(kw, match):
    from torchani_amd.md import BatchedDynamics

    sp, x = _cpu_inputs()
    with pytest.raises(ValueError, match=match):
        BatchedDynamics(None, sp, x, **kw)


def test_cpu_tensors_and_bad_shapes_raise():
    from torchani_amd.md import BatchedDynamics

    sp, x = _cpu_inputs()
    with pytest.raises(ValueError, match="ROCm"):
        BatchedDynamics(None, sp, x)
    with pytest.raises(ValueError, match=r"\[C, A, 3\]"):
        BatchedDynamics(None, sp, x[:, :2])


def test_both_drivers_read_one_mass_table():
    from torchani_amd import md

    class Model:
        periodic_table_index = True

    z = torch.tensor([[1, 6, 7, 8, -1, 9, 16, 17]])
    m = md.default_masses(Model(), z)
    assert m.dtype == torch.float32 and m[0].tolist() == pytest.approx([1.008, 12.011, 14.007, 15.999, 0.0, 18.998, 32.06, 35.45])
    Model.periodic_table_index = False
    with pytest.raises(ValueError, match="masses"):
        md.default_masses(Model(), z)
    with pytest.raises(ValueError, match="masses"):   # a standalone pair potential has no periodic_table_index at all
        md.default_masses(object(), z)


def test_library_exports_the_md_entry_points():
    from torchani_amd import _lib, md

    _lib.build()
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "anihip.h")).read()
    declared = set(re.findall(r"\b(anihip_[a-z_0-9]+)\s*\(", hdr))
    for name in ("anihip_md_workspace_bytes", "anihip_md_drift", "anihip_md_kick", "anihip_md_remove_drift", "anihip_md_noise"):
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and getattr(L, name) is not None
    assert "md.hip" in _lib.SOURCES and _lib.ABI_VERSION == 13
    # the ctypes mirror and the constants of the header
    assert ctypes.sizeof(_lib.MdParams) == 4 * 4 + 8 + 8 + 8 and _lib.MdParams.dt.offset == 16
    assert float(re.search(r"#define ANIHIP_MD_ACC_UNIT (\S+)", hdr).group(1)) == md.ACC_UNIT == ref.ACC_UNIT
    assert int(re.search(r"#define ANIHIP_MD_LANGEVIN (\d+)", hdr).group(1)) == _lib.MD_LANGEVIN
    assert md.KB_HARTREE == ref.KB_HARTREE and md._MB_STEP == ref.MB_STEP
    # scratch: four doubles per 256-atom chunk and per molecule
    assert L.anihip_md_workspace_bytes(3, 70) == (3 + 3) * 32 and L.anihip_md_workspace_bytes(1, 257) == (2 + 1) * 32
    assert L.anihip_md_workspace_bytes(0, 5) == 0 and b"n_mol" in L.anihip_last_error()
