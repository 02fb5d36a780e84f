"""fp64 numpy restatement of torchani_amd.phonons, what the phonon tests compare the kernels with: the supercell, the
minimum-image lattice vectors, the compact pattern, the fold over translations, D(q) and its derivatives, the smeared density of
states and the harmonic thermodynamics; and the synthetic crystals the tests run on (a random translation-invariant model of
symmetric pair springs, a simple-cubic monatomic lattice and a diatomic chain with closed-form dispersions)."""
import math

import numpy as np

HARTREE_TO_JOULE = 27.211386024367243 * 1.6021766208e-19
AMU_TO_KG = 1.660539040e-27
SQRT_MHESSIAN_TO_RAD_PER_FS = math.sqrt(HARTREE_TO_JOULE / AMU_TO_KG) / 1e-10 * 1e-15
HBAR = 0.024188843265857      # Hartree fs
KB = 3.166811563e-6           # Hartree / K
TIE_TOL = 1e-9


def cells(repeats):
    """int64 [N_c, 3] in cell-major order (l_3 fastest)."""
    return np.stack(np.meshgrid(*[np.arange(r) for r in repeats], indexing="ij"), -1).reshape(-1, 3).astype(np.int64)


def cell_index(l, repeats):   # noqa: E741
    l = np.mod(l, np.asarray(repeats))   # noqa: E741
    return (l[..., 0] * repeats[1] + l[..., 1]) * repeats[2] + l[..., 2]


def supercell_positions(tau, a, repeats):
    """float64 [N, 3]: tau_b + l . a, atom index = cell index * n + b."""
    l = cells(repeats).astype(np.float64)   # noqa: E741
    return (tau[None] + (l[:, 0:1] * a[0] + l[:, 1:2] * a[1] + l[:, 2:3] * a[2])[:, None]).reshape(-1, 3)


SHIFTS = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), -1).reshape(-1, 3)


def lattice_vectors(tau, a, repeats, b, j):
    """int64 [m, 3]: the minimum image by atom distance of supercell atom j as seen from basis atom b in the home cell; among
    images equidistant to TIE_TOL the lexicographically first lattice vector for b < b' (b = b': when the cell of j is not after
    its mirror cell), the last otherwise: the two directions of a pair take opposite vectors."""
    n, r = tau.shape[0], np.asarray(repeats, dtype=np.int64)
    bp, lp = j % n, cells(repeats)[j // n]
    d = tau[bp] + lp.astype(np.float64) @ a - tau[b]
    frac = np.linalg.solve(a.T, d.T).T / r
    base = lp - r * np.rint(frac).astype(np.int64)
    cand = base[:, None] + SHIFTS[None] * r
    dc = tau[bp][:, None] + cand.astype(np.float64) @ a - tau[b][:, None]
    d2 = (dc * dc).sum(-1)
    near = d2 <= d2.min(axis=1, keepdims=True) * (1.0 + TIE_TOL) + 1e-300
    span = 1 << 16
    rank = ((cand[..., 0] + span) * (2 * span) + cand[..., 1] + span) * (2 * span) + cand[..., 2] + span
    first = (b < bp) | ((b == bp) & (j // n <= cell_index(-lp, repeats)))
    pick = np.where(first, np.where(near, rank, 8 * span ** 3).argmin(axis=1), np.where(near, rank, -1).argmax(axis=1))
    return cand[np.arange(len(j)), pick]


def brute_force_lattice_vectors(tau, a, repeats, b, j, span=3):
    """The same by a search over every image within +-span supercells (no rounding step): the squared distances found."""
    n, r = tau.shape[0], np.asarray(repeats, dtype=np.int64)
    bp, lp = j % n, cells(repeats)[j // n]
    sh = np.stack(np.meshgrid(*[np.arange(-span, span + 1)] * 3, indexing="ij"), -1).reshape(-1, 3)
    cand = lp[:, None] + sh[None] * r
    dc = tau[bp][:, None] + cand.astype(np.float64) @ a - tau[b][:, None]
    return (dc * dc).sum(-1).min(axis=1)


def compact_pattern(index, n, n_atoms):
    """The home cell's columns sorted by (b, b', j): ent_b, ent_j [m], boff [n + 1], poff [n^2 + 1], diag_entry [n]."""
    home = np.nonzero(index[1] < n)[0]
    b, j = index[1][home], index[0][home]
    order = np.argsort((b * n + j % n) * n_atoms + j, kind="stable")
    b, j = b[order], j[order]
    boff = np.concatenate([[0], np.cumsum(np.bincount(b, minlength=n))])
    poff = np.concatenate([[0], np.cumsum(np.bincount(b * n + j % n, minlength=n * n))])
    diag = np.full(n, -1, dtype=np.int64)
    own = np.nonzero(b == j)[0]
    diag[b[own]] = own
    return b, j, boff, poff, diag


def symmetrized(index, blocks, n_atoms):
    """(sorted keys row * N + column, blocks (B_ij + B_ji^T) / 2 in that order), rounded to the dtype of ``blocks``: float32
    blocks give what anihip_block_hessian_prepare stores, float64 blocks the exact model."""
    key = index[0] * n_atoms + index[1]
    order = np.argsort(key)
    skey = key[order]
    tkey = index[1] * n_atoms + index[0]
    pos = np.searchsorted(skey, tkey)
    assert np.all(pos < len(skey)) and np.all(skey[np.minimum(pos, len(skey) - 1)] == tkey), "pattern is not symmetric"
    partner = order[pos]
    sym = ((blocks.astype(np.float64) + blocks[partner].astype(np.float64).transpose(0, 2, 1)) * 0.5).astype(blocks.dtype)
    return skey, sym[order]


def fold(index, blocks, n, repeats, ent_b, ent_j, boff=None, diag=None):
    """(phi float64 [m, 3, 3], missing [m], defect [m]): the mean over the translations in cell-major order (sequential sums),
    a block that is not stored counted as zero; with boff and diag the acoustic sum rule on the diagonal entries."""
    N = n * int(np.prod(repeats))
    skey, sym = symmetrized(index, blocks, N)
    cl = cells(repeats)
    lj, bp = cl[ent_j // n], ent_j % n
    m = len(ent_b)
    s = np.zeros((m, 3, 3))
    missing = np.zeros(m, dtype=np.int64)
    got = []
    for t in range(len(cl)):
        col = t * n + ent_b
        row = cell_index(lj + cl[t], repeats) * n + bp
        key = col * N + row                       # the block H_(col x),(row y): Phi_xy
        pos = np.minimum(np.searchsorted(skey, key), len(skey) - 1)
        found = skey[pos] == key
        blk = np.where(found[:, None, None], sym[pos].astype(np.float64), 0.0)
        s = s + blk
        missing += ~found
        got.append(blk)
    phi = s / float(len(cl))
    defect = np.zeros(m)
    for blk in got:
        defect = np.maximum(defect, np.abs(blk - phi).max(axis=(1, 2)))
    if boff is not None:
        for b in range(n):
            if diag[b] < 0:
                continue
            S = np.zeros((3, 3))
            for e in range(boff[b], boff[b + 1]):
                if e != diag[b]:
                    S = S + phi[e]
            phi[diag[b]] = -0.5 * (S + S.T)
    return phi, missing, defect


def dynmat(phi, nvec, ent_b, ent_bp, masses, q, rvec=None):
    """D complex128 [Q, 3n, 3n] (and dD / dk [Q, 3, 3n, 3n] with rvec) by direct summation."""
    n, Q = len(masses), len(q)
    D = np.zeros((Q, n, 3, n, 3), dtype=np.complex128)
    dD = None if rvec is None else np.zeros((Q, 3, n, 3, n, 3), dtype=np.complex128)
    t = q[:, None, 0] * nvec[None, :, 0] + q[:, None, 1] * nvec[None, :, 1] + q[:, None, 2] * nvec[None, :, 2]   # [Q, m]
    f = t - np.rint(t)
    ph = np.cos(2 * np.pi * f) + 1j * np.sin(2 * np.pi * f)
    w = 1.0 / np.sqrt(masses[ent_b] * masses[ent_bp])
    for e in range(len(ent_b)):
        c = ph[:, e, None, None] * (phi[e] * w[e])[None]
        D[:, ent_b[e], :, ent_bp[e], :] += c
        if dD is not None:
            for a in range(3):
                dD[:, a, ent_b[e], :, ent_bp[e], :] += 1j * rvec[e, a] * c
    D = D.reshape(Q, 3 * n, 3 * n)
    return D if rvec is None else (D, dD.reshape(Q, 3, 3 * n, 3 * n))


def gershgorin(D):
    return np.abs(D).sum(axis=-1).max()


def dos(freqs, weights, first, df, sigma, bins):
    fk = first + df * np.arange(bins)
    x = (fk[:, None] - freqs.reshape(-1)[None]) / sigma
    w = np.broadcast_to(weights[:, None], freqs.shape).reshape(-1)
    return fk, (w[None] * np.exp(-0.5 * x * x)).sum(axis=1) / (sigma * math.sqrt(2 * math.pi))


def thermodynamics(eigenvalues, weights, temperatures):
    """(zero-point energy, F [T], S [T], C_v [T], n_imaginary) per primitive cell, Hartree and Hartree / K; T > 0."""
    lam = eigenvalues.reshape(-1)
    w = np.broadcast_to(weights[:, None], eigenvalues.shape).reshape(-1)
    real = lam > 0
    e, w = HBAR * SQRT_MHESSIAN_TO_RAD_PER_FS * np.sqrt(lam[real]), w[real]
    zpe = 0.5 * (w * e).sum()
    F, S, Cv = [], [], []
    for T in temperatures:
        x = np.minimum(e / (KB * T), 700.0)   # (exp(700) is finite; every term is 0 to fp64 far below that)
        F.append(zpe + KB * T * (w * np.log1p(-np.exp(-x))).sum())
        S.append(KB * (w * (x / np.expm1(x) - np.log1p(-np.exp(-x)))).sum())
        Cv.append(KB * (w * x * x * np.exp(-x) / (1.0 - np.exp(-x)) ** 2).sum())
    return zpe, np.array(F), np.array(S), np.array(Cv), int((~real).sum())


# ---- synthetic crystals ----------------------------------------------------------------------------------------------------
def random_crystal(seed, n, skew=0.15):
    """(tau [n, 3], a [3, 3], masses [n]): a skewed cell of about 3 Angstrom with n atoms inside."""
    rs = np.random.RandomState(seed)
    a = 3.0 * np.eye(3) + skew * rs.uniform(-1, 1, (3, 3))
    return rs.uniform(0, 1, (n, 3)) @ a, a, rs.uniform(1.0, 16.0, n)


def random_springs(seed, n, per_atom=3, hub=None):
    """[(b, b', nvec, K)]: per basis atom per_atom springs to random atoms of the 27 nearest cells with random symmetric K;
    hub = (b, count) adds springs from b to `count` distinct (b', nvec) with nvec in {-1, 0, 1}^3."""
    rs = np.random.RandomState(seed)
    out = []

    def sym():
        k = rs.uniform(-1, 1, (3, 3))
        return 0.5 * (k + k.T) + np.eye(3)

    for b in range(n):
        for _ in range(per_atom):
            out.append((b, int(rs.randint(n)), rs.randint(-1, 2, 3), sym()))
    if hub is not None:
        b, count = hub
        pick = rs.permutation(27 * n)[:count]
        for p in pick:
            out.append((b, int(p % n), SHIFTS[p // n], sym()))
    return out


def spring_blocks(n, repeats, springs):
    """Column-sorted (index int64 [2, nnz], blocks float64 [nnz, 3, 3]) of the supercell Hessian of the energy
    sum over cells and springs of 1/2 (u_i - u_j)^T K (u_i - u_j), i = (b, l), j = (b', l + nvec mod repeats): symmetric, and
    every row sums to zero.  A spring whose ends fold onto one atom adds nothing."""
    cl = cells(repeats)
    N = n * len(cl)
    rows, cols, vals = [], [], []
    for b, bp, nv, K in springs:
        i = np.arange(len(cl)) * n + b
        j = cell_index(cl + np.asarray(nv), repeats) * n + bp
        keep = i != j
        i, j = i[keep], j[keep]
        for r, c, s in ((i, i, 1.0), (j, j, 1.0), (i, j, -1.0), (j, i, -1.0)):
            rows.append(r)
            cols.append(c)
            vals.append(np.broadcast_to(s * K, (len(r), 3, 3)))
    diag = np.arange(N)                               # every atom keeps a (possibly zero) diagonal block
    rows, cols, vals = np.concatenate(rows + [diag]), np.concatenate(cols + [diag]), np.concatenate(vals + [np.zeros((N, 3, 3))])
    key = cols * N + rows
    ukey, inv = np.unique(key, return_inverse=True)
    blocks = np.zeros((len(ukey), 3, 3))
    np.add.at(blocks, inv, vals)
    return np.stack([ukey % N, ukey // N]), blocks


def dense(index, blocks, n_atoms):
    H = np.zeros((n_atoms, 3, n_atoms, 3))
    H[index[0], :, index[1], :] = blocks
    return H.reshape(3 * n_atoms, 3 * n_atoms)


def commensurate_q(repeats):
    return cells(repeats).astype(np.float64) / np.asarray(repeats, dtype=np.float64)


def compact_from_blocks(index, blocks32, tau, a, repeats, asr=False):
    """Everything D(q) needs from a column-sorted supercell Hessian: dict of ent_b, ent_bp, ent_j, nvec, rvec, boff, poff, diag,
    phi, missing, defect."""
    n = len(tau)
    N = n * int(np.prod(repeats))
    ent_b, ent_j, boff, poff, diag = compact_pattern(index, n, N)
    nvec = lattice_vectors(tau, a, repeats, ent_b, ent_j)
    phi, missing, defect = fold(index, blocks32, n, repeats, ent_b, ent_j, *((boff, diag) if asr else (None, None)))
    return dict(ent_b=ent_b, ent_bp=ent_j % n, ent_j=ent_j, nvec=nvec, rvec=nvec.astype(np.float64) @ a, boff=boff, poff=poff,
                diag=diag, phi=phi, missing=missing, defect=defect)


def cubic_lattice(a=2.5, mass=12.0, k=((1.0, 0.3, 0.2), (0.25, 0.9, 0.15), (0.1, 0.35, 0.8))):
    """Simple-cubic monatomic lattice, nearest-neighbour springs diag(k[alpha]) along +-e_alpha:
    omega^2_x(q) = (2 / m) sum_alpha k[alpha][x] (1 - cos 2 pi q_alpha)."""
    k = np.asarray(k, dtype=np.float64)
    springs = [(0, 0, np.eye(3, dtype=np.int64)[al], np.diag(k[al])) for al in range(3)]
    return np.zeros((1, 3)), a * np.eye(3), np.array([mass]), springs, k


def cubic_closed_form(q, a, mass, k):
    """(eigenvalues [Q, 3], d eigenvalue / d k_beta [Q, 3, 3]) for polarizations x, y, z (not sorted)."""
    lam = (2.0 / mass) * ((1.0 - np.cos(2 * np.pi * q))[:, :, None] * k[None]).sum(axis=1)            # [Q, x]
    dlam = (2.0 / mass) * a * np.sin(2 * np.pi * q)[:, :, None] * k[None]                             # [Q, beta, x]
    return lam, dlam.transpose(0, 2, 1)


def diatomic_chain(a=3.0, m1=1.0, m2=3.0, k=0.7):
    """Two atoms per cell at 0 and a / 2 along x, springs diag(k, 0, 0) between neighbours:
    omega^2 = k (1/m1 + 1/m2) -+ k sqrt((1/m1 + 1/m2)^2 - 4 sin^2(pi q_x) / (m1 m2)); the y and z rows are zero."""
    K = np.diag([k, 0.0, 0.0])
    springs = [(0, 1, np.zeros(3, dtype=np.int64), K), (1, 0, np.array([1, 0, 0]), K)]
    tau = np.array([[0.0, 0.0, 0.0], [0.5 * a, 0.0, 0.0]])
    return tau, np.diag([a, 2.0 * a, 2.0 * a]), np.array([m1, m2]), springs


def chain_closed_form(qx, m1, m2, k):
    s = 1.0 / m1 + 1.0 / m2
    root = np.sqrt(s * s - 4.0 * np.sin(np.pi * qx) ** 2 / (m1 * m2))
    return k * (s - root), k * (s + root)
