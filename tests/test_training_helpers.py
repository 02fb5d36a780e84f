"""CPU checks of the helpers behind tests/test_gpu_training_scale.py: the fp64 numpy magnitude pass computes the same weight
gradients as the oracle (so its bound B is built from the right d e / d z and layer inputs), and the block splitter covers
the oracle's packed gradient layout exactly."""
import numpy as np
import pytest

from _util import (conformers, fgrad_direction, grad_blocks, load_golden, mlp_magnitude_pass, mlp_tangent_magnitude_pass,
                   oracle_networks, oracle_params, seeded_state)


@pytest.mark.parametrize("base", ["rand_batch_ani2x", "dense90_ani2x"])
def test_magnitude_pass_matches_oracle_weight_grads(oracle64, base):
    g = load_golden(base)
    dims, flat, _ = oracle_networks(g["kind"], g["n_members"], g["seed"])
    p = oracle_params(g["kind"], g["cutoff_fn"])
    aev = oracle64.aev(p, g["species"], g["coords"].astype(np.float64), g["cell"], g["pbc"])
    C, A = g["species"].shape
    # a signed upstream over four decades (what a per-molecule loss gradient looks like), non-zero on padding atoms too
    rs = np.random.RandomState(3)
    up = rs.choice([-1.0, 1.0], C * A) * 10.0 ** rs.uniform(-2, 2, C * A)
    ref = oracle64.mlp_weight_grads(g["species"], aev, up, dims, flat, n_members=g["n_members"])
    signed, bound = mlp_magnitude_pass(g["species"], aev, up, dims, flat, g["n_members"])
    assert signed.shape == bound.shape == ref.shape
    assert np.all(bound >= np.abs(signed) * (1 - 1e-12))
    for key, sl in grad_blocks(dims, g["n_members"]):
        scale = np.abs(ref[sl]).max()
        assert np.abs(signed[sl] - ref[sl]).max() <= 1e-12 * scale, key
        # a species that is absent from the batch has no gradient and no bound
        present = bool((g["species"] == key[1]).any())
        assert (bound[sl].max() > 0) == present, key
    # linear in the upstream gradient, and the bound only sees its magnitude
    s2, b2 = mlp_magnitude_pass(g["species"], aev, -4.0 * up, dims, flat, g["n_members"])
    assert np.abs(s2 + 4.0 * signed).max() <= 1e-14 * np.abs(signed).max() * 4
    assert np.abs(b2 - 4.0 * bound).max() <= 1e-14 * bound.max() * 4


@pytest.mark.parametrize("base", ["rand_batch_ani2x", "water_pbc_ani2x"])
def test_tangent_magnitude_pass_matches_oracle(oracle64, base):
    """The force-training (tangent) variant against oracle.mlp_tangent_weight_grads, with v = -J t as in training."""
    g = load_golden(base)
    dims, flat, _ = oracle_networks(g["kind"], g["n_members"], g["seed"])
    p = oracle_params(g["kind"], g["cutoff_fn"])
    aev, jt = oracle64.aev_jvp(p, g["species"], g["coords"].astype(np.float64), fgrad_direction(g["species"]), g["cell"],
                               g["pbc"])
    _, ref = oracle64.mlp_tangent_weight_grads(g["species"], aev, -jt, dims, flat, n_members=g["n_members"])
    signed, bound = mlp_tangent_magnitude_pass(g["species"], aev, -jt, dims, flat, g["n_members"])
    assert np.all(bound >= np.abs(signed) * (1 - 1e-12))
    for key, sl in grad_blocks(dims, g["n_members"]):
        assert np.abs(signed[sl] - ref[sl]).max() <= 1e-12 * max(bound[sl].max(), 1e-300), key


@pytest.mark.parametrize("kind", ["ani1x", "ani2x"])
def test_grad_blocks_round_trip_the_oracle_layout(kind):
    from oracle import oracle as orc
    from torchani_amd.weights import NN_PREFIX, arch_spec

    symbols, _, _ = arch_spec(kind)
    M = 8
    sd = seeded_state(kind, M, 4)
    dims, flat = orc.pack_networks(sd, symbols, M)
    blocks = grad_blocks(dims, M)
    nl = dims.shape[1] - 1
    assert len(blocks) == M * len(symbols) * nl * 2
    # contiguous, in order, covering the whole vector
    assert blocks[0][1].start == 0 and blocks[-1][1].stop == flat.size
    assert all(a[1].stop == b[1].start for a, b in zip(blocks, blocks[1:]))
    # every block holds the state-dict tensor it is named after
    for (m, s, l, wb), sl in blocks:
        name = f"layers.{l}" if l < nl - 1 else "final_layer"
        t = np.asarray(sd[f"{NN_PREFIX}members.{m}.atomics.{symbols[s]}.{name}.{'weight' if wb == 'w' else 'bias'}"])
        assert np.array_equal(flat[sl], t.astype(np.float64).reshape(-1)), (m, s, l, wb)
    # and cutting then concatenating gives the vector back
    assert np.array_equal(np.concatenate([flat[sl] for _, sl in blocks]), flat)


def test_conformers_generator():
    sp, x = conformers(64, 24, seed=5)
    assert sp.shape == (64, 24) and x.shape == (64, 24, 3)
    n_real = (sp >= 0).sum(axis=1)
    assert n_real.min() >= 2 and n_real.max() <= 24
    # real atoms first, then padding; padding atoms sit at the origin
    assert all(np.all(sp[m, :k] >= 0) and np.all(sp[m, k:] == -1) for m, k in enumerate(n_real))
    assert np.all(x[sp < 0] == 0)
    assert set(np.unique(sp[sp >= 0])) <= {0, 1, 2, 3}
    # seeded: the same batch twice; other species sets on request
    sp2, x2 = conformers(64, 24, seed=5)
    assert np.array_equal(sp, sp2) and np.array_equal(x, x2)
    sp7, _ = conformers(200, 24, seed=1, species=range(7), p=None)
    assert set(np.unique(sp7[sp7 >= 0])) == set(range(7))
    # no two atoms of a molecule closer than the jittered lattice allows
    for m in range(8):
        k = n_real[m]
        d = np.linalg.norm(x[m, :k, None] - x[m, None, :k], axis=-1) + 10 * np.eye(k)
        assert d.min() > 1.1 - 2 * 0.15 * np.sqrt(3)
