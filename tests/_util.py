"""Shared helpers for the tests: golden fixtures, seeded weights, oracle packing."""
from __future__ import annotations

import functools
import glob
import os

import numpy as np

from oracle import oracle as orc
from torchani_amd.weights import random_state_dict

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_NAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz"))
                      if not os.path.basename(p).startswith(("nbrs_", "wgrads_", "stress_", "fgrads_", "cfg3_", "pairs_", "pairs2_", "d3_", "x2r_", "x2rtrain_", "mbis_", "simple_", "hess_", "grid_", "nbrsweep_")))   # reference neighbor lists /
#                                                                                      weight-gradient digests
WGRAD_NAMES = sorted(os.path.basename(p)[7:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "wgrads_*.npz")))
STRESS_NAMES = sorted(os.path.basename(p)[7:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "stress_*.npz")))
FGRAD_NAMES = sorted(os.path.basename(p)[7:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "fgrads_*.npz")))
WGRAD_BLOCK = 4096


def wgrad_upstream(C, A):
    """Per-atom loss weights of tests/golden/gen_golden_wgrads.py."""
    k = np.arange(C * A, dtype=np.float64)
    return (0.5 + np.modf(0.37 * k)[0]).reshape(C, A)


def wgrad_digest(flat):
    """Block sums / pattern dot products / sampled heads of a packed gradient vector (gen_golden_wgrads.py)."""
    n = flat.shape[0]
    nb = (n + WGRAD_BLOCK - 1) // WGRAD_BLOCK
    pad = np.zeros(nb * WGRAD_BLOCK, dtype=np.float64)
    pad[:n] = flat
    pat = np.cos(0.37 * np.arange(nb * WGRAD_BLOCK, dtype=np.float64))
    blocks = pad.reshape(nb, WGRAD_BLOCK)
    return blocks.sum(axis=1), (pad * pat).reshape(nb, WGRAD_BLOCK).sum(axis=1), blocks[::97, :64].copy()


def load_wgrads(base):
    with np.load(os.path.join(GOLDEN_DIR, "wgrads_" + base + ".npz")) as z:
        return {k: z[k] for k in z.files}


def load_golden(name):
    with np.load(os.path.join(GOLDEN_DIR, name + ".npz")) as z:
        g = {k: z[k] for k in z.files}
    g["kind"] = str(g["kind"])
    g["seed"] = int(g["seed"])
    g["n_members"] = int(g["n_members"])
    g["symbols"] = [str(s) for s in g["symbols"]]
    g.setdefault("cell", None)
    g.setdefault("pbc", None)
    g["cutoff_fn"] = str(g["cutoff_fn"]) if "cutoff_fn" in g else "cosine"
    return g


@functools.lru_cache(maxsize=4)
def seeded_state(kind, n_members, seed):
    return random_state_dict(kind, n_members, seed)


@functools.lru_cache(maxsize=4)
def oracle_networks(kind, n_members, seed):
    from torchani_amd.weights import arch_spec

    symbols, _, _ = arch_spec(kind)
    sd = seeded_state(kind, n_members, seed)
    dims, flat = orc.pack_networks(sd, symbols, n_members)
    sae = sd["energy_shifter.self_energies"].astype(np.float64)
    return dims, flat, sae


def oracle_params(kind, cutoff_fn="cosine"):
    return orc.params_2x(cutoff_fn) if kind == "ani2x" else orc.params_1x(cutoff_fn)


def load_sampled(name):
    """Large-system fixtures of tests/golden/gen_golden_configs.py (inputs whole, outputs on a sample of atoms)."""
    with np.load(os.path.join(GOLDEN_DIR, name + ".npz")) as z:
        g = {k: z[k] for k in z.files}
    g["seed"] = int(g["seed"])
    g["species"] = g["species"].astype(np.int64)
    g.setdefault("cell", None)
    g.setdefault("pbc", None)
    return g


def load_stress(base):
    with np.load(os.path.join(GOLDEN_DIR, "stress_" + base + ".npz")) as z:
        return {k: z[k] for k in z.files}


def load_fgrads(base):
    with np.load(os.path.join(GOLDEN_DIR, "fgrads_" + base + ".npz")) as z:
        return {k: z[k] for k in z.files}


def fgrad_direction(species):
    """Coordinate-space direction of tests/golden/gen_golden_fgrads.py (zero on padding atoms)."""
    C, A = species.shape
    q = 3.0 * np.arange(C * A, dtype=np.float64)
    t = np.stack([np.modf(0.37 * q)[0], np.modf(0.61 * q)[0] - 0.5, 0.25 - np.modf(0.13 * q)[0]], axis=-1)
    return t.reshape(C, A, 3) * (species >= 0)[..., None]


def _stress_state(case, seed=11):
    """ANI-2x x 8 parameter sets that stress the split-fp16 network arithmetic (its power-of-two scales come from
    weight-norm BOUNDS, include/anihip.h: anihip_mlp_desc.fused_bounds) away from the uniform +-1/sqrt(fan_in) init."""
    from torchani_amd.weights import NN_PREFIX, random_state_dict

    sd = {k: v.copy() for k, v in random_state_dict("ani2x", 8, seed).items()}
    rs = np.random.RandomState(seed + 1)
    layer_of = lambda k: 3 if ".final_layer." in k else int(k.split(".layers.")[1].split(".")[0])   # noqa: E731
    if case.startswith("scale"):
        sc = {"scale_small": (0.125, 0.125, 0.125, 0.125), "scale_large": (8.0, 8.0, 8.0, 8.0),
              "scale_mixed": (8.0, 0.125, 8.0, 0.125)}[case]
        for k in sd:
            if k.startswith(NN_PREFIX):
                sd[k] = (sd[k] * np.float32(sc[layer_of(k)])).astype(np.float32)
    elif case == "student_t":
        for k in sd:
            if k.startswith(NN_PREFIX) and k.endswith("weight"):
                bound = 1.0 / np.sqrt(sd[k].shape[1])
                sd[k] = (rs.standard_t(3, size=sd[k].shape) * bound / np.sqrt(3.0)).astype(np.float32)
    elif case == "outlier_row":
        for sym, layer, r in (("H", 1, 7), ("O", 0, 100), ("C", 2, 3)):
            k = f"{NN_PREFIX}members.3.atomics.{sym}.layers.{layer}.weight"
            sd[k][r] *= np.float32(100.0)
    else:
        raise ValueError(case)
    return sd


def conformers(n_mol, n_at, seed=5, species=(0, 1, 2, 3), p=(0.5, 0.3, 0.1, 0.1), min_atoms=2):
    """Seeded batch of small molecules, padded with -1 to n_at atoms (tools/train_bench.py's generator: with the defaults
    the same batch): a jittered 1.1 A lattice, min_atoms..n_at atoms per molecule, species drawn from ``species`` with
    probabilities ``p``."""
    rs = np.random.RandomState(seed)
    sp = np.full((n_mol, n_at), -1, dtype=np.int64)
    x = np.zeros((n_mol, n_at, 3), dtype=np.float32)
    side = int(np.ceil(n_at ** (1 / 3)))
    grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    for m in range(n_mol):
        k = rs.randint(min_atoms, n_at + 1)
        pick = rs.permutation(len(grid))[:k]
        x[m, :k] = 1.1 * grid[pick] + rs.uniform(-0.15, 0.15, (k, 3)).astype(np.float32)
        sp[m, :k] = rs.choice(list(species), size=k, p=p)
    return sp, x


def grad_blocks(dims, n_members):
    """The oracle's packed gradient layout (oracle.pack_networks; tests/test_gpu_training.py:flat_from_lists) cut into
    blocks: [((member, species, layer, "w" | "b"), slice)] in storage order."""
    dims = np.asarray(dims)
    out, off = [], 0
    for m in range(n_members):
        for s in range(dims.shape[0]):
            for l in range(dims.shape[1] - 1):
                nw, nb = int(dims[s, l] * dims[s, l + 1]), int(dims[s, l + 1])
                out.append(((m, s, l, "w"), slice(off, off + nw)))
                out.append(((m, s, l, "b"), slice(off + nw, off + nw + nb)))
                off += nw + nb
    return out


def mlp_magnitude_pass(species, aev, g_atom, dims, flat, n_members, celu_alpha=0.1):
    """fp64 numpy pass over ANI CELU networks in the oracle's packed layout (dims, flat).  With D_a = d e_a / d z per member
    and layer (z: the layer's pre-activation, e: the ensemble mean) and X_a the layer's input, returns two flat vectors in
    the layout of ``flat``:
      signed = sum_a g_a D_a^T X_a  (biases: sum_a g_a D_a) -- the weight gradients, to check this pass against the oracle;
      bound  = sum_a |g_a| |D_a|^T |X_a|  (biases: sum_a |g_a| |D_a|) -- the scale every summation error of a gradient
               entry is relative to."""
    species = np.asarray(species).reshape(-1)
    n = species.shape[0]
    dims = np.asarray(dims)
    S, nl = dims.shape[0], dims.shape[1] - 1
    aev = np.asarray(aev, dtype=np.float64).reshape(n, dims[0, 0])
    g = np.asarray(g_atom, dtype=np.float64).reshape(n)
    flat = np.asarray(flat, dtype=np.float64)
    signed, bound = np.zeros_like(flat), np.zeros_like(flat)
    blocks = iter(grad_blocks(dims, n_members))
    for m in range(n_members):
        for s in range(S):
            sl = [(next(blocks)[1], next(blocks)[1]) for _ in range(nl)]
            W = [flat[w].reshape(dims[s, l + 1], dims[s, l]) for l, (w, _) in enumerate(sl)]
            b = [flat[bb] for _, bb in sl]
            rows = np.nonzero(species == s)[0]
            if rows.size == 0:
                continue
            X, dz = [aev[rows]], []
            for l in range(nl - 1):
                z = X[l] @ W[l].T + b[l]
                zn = np.minimum(z, 0.0) / celu_alpha
                X.append(np.where(z > 0, z, celu_alpha * np.expm1(zn)))
                dz.append(np.where(z > 0, 1.0, np.exp(zn)))
            ga = g[rows]
            D = np.full((rows.size, dims[s, nl]), 1.0 / n_members)
            for l in range(nl - 1, -1, -1):
                w, bb = sl[l]
                signed[w] = ((ga[:, None] * D).T @ X[l]).reshape(-1)
                signed[bb] = ga @ D
                aD = np.abs(ga)[:, None] * np.abs(D)
                bound[w] = (aD.T @ np.abs(X[l])).reshape(-1)
                bound[bb] = aD.sum(axis=0)
                if l > 0:
                    D = (D @ W[l]) * dz[l - 1]
    return signed, bound



def mlp_tangent_magnitude_pass(species, aev, tangent, dims, flat, n_members, celu_alpha=0.1):
    """The same for the second-order pass of force training (oracle.mlp_tangent_weight_grads): S = sum_a v_a . d e_a / d aev_a,
    forward over reverse -- activations a_l and tangents adot_l (adot_0 = v), adjoints mu_l = dS / d adot_l, nu_l = dS / d a_l,
    p = mu c'(z), q = mu c''(z) zdot + nu c'(z).  Returns (signed, bound): signed = dS / d params (dW_l = p adot^T + q a^T,
    db_l = q), bound = sum_a |p| |adot|^T + |q| |a|^T (biases: sum_a |q|)."""
    species = np.asarray(species).reshape(-1)
    n = species.shape[0]
    dims = np.asarray(dims)
    S, nl = dims.shape[0], dims.shape[1] - 1
    aev = np.asarray(aev, dtype=np.float64).reshape(n, dims[0, 0])
    tangent = np.asarray(tangent, dtype=np.float64).reshape(n, dims[0, 0])
    flat = np.asarray(flat, dtype=np.float64)
    signed, bound = np.zeros_like(flat), np.zeros_like(flat)
    blocks = iter(grad_blocks(dims, n_members))
    for m in range(n_members):
        for s in range(S):
            sl = [(next(blocks)[1], next(blocks)[1]) for _ in range(nl)]
            W = [flat[w].reshape(dims[s, l + 1], dims[s, l]) for l, (w, _) in enumerate(sl)]
            b = [flat[bb] for _, bb in sl]
            rows = np.nonzero(species == s)[0]
            if rows.size == 0:
                continue
            A, Ad, c1, c2, zd = [aev[rows]], [tangent[rows]], [], [], []
            for l in range(nl):
                z = A[l] @ W[l].T + b[l]
                zd.append(Ad[l] @ W[l].T)
                if l < nl - 1:
                    e = np.exp(np.minimum(z, 0.0) / celu_alpha)
                    c1.append(np.where(z > 0, 1.0, e))
                    c2.append(np.where(z > 0, 0.0, e / celu_alpha))
                    A.append(np.where(z > 0, z, celu_alpha * (e - 1.0)))
                    Ad.append(c1[l] * zd[l])
                else:
                    c1.append(np.ones_like(z))
                    c2.append(np.zeros_like(z))
            mu = np.full((rows.size, dims[s, nl]), 1.0 / n_members)
            nu = np.zeros_like(mu)
            for l in range(nl - 1, -1, -1):
                w, bb = sl[l]
                p = mu * c1[l]
                q = mu * c2[l] * zd[l] + nu * c1[l]
                signed[w] = (p.T @ Ad[l] + q.T @ A[l]).reshape(-1)
                signed[bb] = q.sum(axis=0)
                bound[w] = (np.abs(p).T @ np.abs(Ad[l]) + np.abs(q).T @ np.abs(A[l])).reshape(-1)
                bound[bb] = np.abs(q).sum(axis=0)
                mu, nu = p @ W[l], q @ W[l]
    return signed, bound



def celu_kink_atoms(species, aev, dims, flat, n_members, rel=1e-6):
    """Atoms with a hidden pre-activation z within rel x (sum |W| |x| + |b|) of 0 in some member (fp64).  CELU's second
    derivative jumps from 1 / alpha to 0 at z = 0: for such an atom the fp32 rounding of z decides which side the second-order
    pass of force training takes, in any fp32 implementation."""
    species = np.asarray(species).reshape(-1)
    n = species.shape[0]
    dims = np.asarray(dims)
    S, nl = dims.shape[0], dims.shape[1] - 1
    aev = np.asarray(aev, dtype=np.float64).reshape(n, dims[0, 0])
    out = np.zeros(n, dtype=bool)
    blocks = iter(grad_blocks(dims, n_members))
    for m in range(n_members):
        for s in range(S):
            sl = [(next(blocks)[1], next(blocks)[1]) for _ in range(nl)]
            rows = np.nonzero(species == s)[0]
            if rows.size == 0:
                continue
            X = aev[rows]
            for l in range(nl - 1):
                W, b = flat[sl[l][0]].reshape(dims[s, l + 1], dims[s, l]), flat[sl[l][1]]
                z = X @ W.T + b
                out[rows] |= (np.abs(z) <= rel * (np.abs(X) @ np.abs(W).T + np.abs(b))).any(axis=1)
                X = np.where(z > 0, z, 0.1 * np.expm1(np.minimum(z, 0.0) / 0.1))
    return out


def block_error_ratios(got, ref, bound, blocks):
    """Per block: max |got - ref| / max(bound over the block) ({key: ratio}); a block whose bound is 0 (a species absent
    from the batch, a zero upstream) must be exactly 0 -- its ratio is inf otherwise."""
    out = {}
    for key, sl in blocks:
        err = float(np.abs(got[sl] - ref[sl]).max())
        bmax = float(bound[sl].max())
        out[key] = err / bmax if bmax > 0 else (0.0 if err == 0.0 else np.inf)
    return out
