"""fp64 numpy restatement of what csrc/md.hip computes (include/anihip.h has the definition): Philox4x32-10, the Box-Muller
mapping of its four words to three normal variates, and the two halves of a velocity-Verlet / BAOAB step."""
import numpy as np

ACC_UNIT = 4.3597447222071e-18 / 1e-10 / 1.66053906660e-27 * 1e10 * 1e-30   # (Hartree / Angstrom) / amu in Angstrom / fs^2
KB_HARTREE = 3.166811563e-6
MB_STEP = 1 << 63   # step words of BatchedDynamics.set_temperature's draws

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter [..., 4] and key [2] (or [..., 2]) of 32-bit words -> [..., 4] uint32 (Salmon et al. 2011)."""
    c = [np.asarray(counter)[..., k].astype(np.uint64) & MASK for k in range(4)]
    key = np.asarray(key)
    k0, k1 = key[..., 0].astype(np.uint64) & MASK, key[..., 1].astype(np.uint64) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack(c, axis=-1).astype(np.uint32)


def uniform(u):
    """p(u) = ((u >> 9) + 0.5) 2^-23 in (0, 1)."""
    return ((np.asarray(u, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def noise(seed, step, n_mol, atoms_per_mol, replica_ids=None):
    """[C, A, 3] fp64: key (seed low, seed high), counter (atom, replica id or molecule index, step low, step high)."""
    rid = np.arange(n_mol) if replica_ids is None else np.asarray(replica_ids)
    ctr = np.empty((n_mol, atoms_per_mol, 4), dtype=np.uint64)
    ctr[..., 0] = np.arange(atoms_per_mol)[None, :]
    ctr[..., 1] = (rid.astype(np.uint64) & MASK)[:, None]
    ctr[..., 2] = step & 0xFFFFFFFF
    ctr[..., 3] = (step >> 32) & 0xFFFFFFFF
    u = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64))
    p = uniform(u)
    r0, r1 = np.sqrt(-2.0 * np.log(p[..., 0])), np.sqrt(-2.0 * np.log(p[..., 2]))
    return np.stack([r0 * np.cos(2 * np.pi * p[..., 1]), r0 * np.sin(2 * np.pi * p[..., 1]),
                     r1 * np.cos(2 * np.pi * p[..., 3])], axis=-1)


def drift(x, v, f, active, mass, dt, langevin=False, kT=None, friction=None, xi=None):
    """First half kick and the position update: x, v, f [C, A, 3], active [C, A] bool, mass [C, A] (amu), kT (Hartree) and
    friction (1 / fs) [C], xi [C, A, 3].  Returns the new (x, v); inactive atoms keep x and get v = 0."""
    act = np.asarray(active, dtype=bool)[..., None]
    im = (ACC_UNIT / np.asarray(mass, dtype=np.float64))[..., None]
    x, v = np.asarray(x, dtype=np.float64), np.asarray(v, dtype=np.float64)
    v1 = v + 0.5 * dt * np.asarray(f, dtype=np.float64) * im
    if langevin:
        c1 = np.exp(-np.asarray(friction, dtype=np.float64) * dt)[:, None, None]
        sigma = np.sqrt(np.asarray(kT, dtype=np.float64)[:, None, None] * (1.0 - c1 * c1) * im)
        x1 = x + 0.5 * dt * v1
        v1 = c1 * v1 + sigma * xi
        x1 = x1 + 0.5 * dt * v1
    else:
        x1 = x + dt * v1
    return np.where(act, x1, x), np.where(act, v1, 0.0)


def kick(v, f, active, mass, dt):
    """Second half kick; returns the new v and the kinetic energies [C] (Hartree) = 1/2 sum m v^2 / ACC_UNIT."""
    act = np.asarray(active, dtype=bool)[..., None]
    m = np.asarray(mass, dtype=np.float64)[..., None]
    v1 = np.where(act, np.asarray(v, dtype=np.float64) + 0.5 * dt * np.asarray(f, dtype=np.float64) * ACC_UNIT / m, 0.0)
    return v1, 0.5 * (np.where(act, m, 0.0) * v1 ** 2).sum(axis=(1, 2)) / ACC_UNIT
