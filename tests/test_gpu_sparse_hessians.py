"""Block-sparse Hessians (grad.energies_forces_and_sparse_hessians) on the MI355X: agreement with the dense batched path
and with the reference's fp64 fixtures (tests/golden/hess_*.npz, hess_x2r_ani2xr_*.npz), completeness and symmetry of the
pattern, the 973-atom protein and the 46 357-atom solvated box (sum rule, symmetry, columns against central differences),
the errors, and that first-order calls launch none of the new kernels."""
import math
import os
import time

import numpy as np
import pytest
import torch

from _util import load_golden, seeded_state

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the measured spreads and timings go to stdout and, when TORCHANI_AMD_HESSIAN_REPORT names a file, are appended to it
REPORT = os.environ.get("TORCHANI_AMD_HESSIAN_REPORT")
DENSE_GATE = 1e-6   # max |H_sparse - H_dense| <= DENSE_GATE * max |H_dense|: the same fp32 arithmetic in another order
REF_GATE = 2e-5     # against the reference's fp64 Hessians, as test_gpu_hessians.py
ANI_BASES = ("ch4_ani1x", "rand_batch_ani2x", "dense90_ani2x", "small_ani2x", "water_pbc_ani2x", "water_pbc_smooth_ani2x",
             "triclinic_pbc_ani2x")
X2R_BASES = ("rand_batch_ani2x", "water_pbc_ani2x")


def report(line):
    print(line)
    if not REPORT:
        return
    try:
        os.makedirs(os.path.dirname(REPORT) or ".", exist_ok=True)
        with open(REPORT, "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from torchani_amd import _lib

    _lib.lib()
    return torch.device("cuda:0")


def _npz(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def _case(base, dev):
    from torchani_amd.models import ANI1x, ANI2x

    g = load_golden(base)
    ctor = ANI2x if g["kind"] == "ani2x" else ANI1x
    model = ctor(state_dict=seeded_state(g["kind"], 8, g["seed"]), device=dev, periodic_table_index=False,
                 cutoff_fn=g["cutoff_fn"], row_capacity=256)
    sp = torch.from_numpy(g["species"].astype(np.int64)).to(dev)
    x = torch.from_numpy(g["coords"]).to(dev)
    cell = None if g["cell"] is None else torch.from_numpy(g["cell"]).to(dev)
    pbc = None if g["pbc"] is None else torch.from_numpy(np.asarray(g["pbc"])).to(dev)
    return model, sp, x, cell, pbc


def _x2r_model(kind, seed, dev, batch=True):
    from torchani_amd.models import ANI2dr, ANI2xr, ANIr2s
    from torchani_amd.weights import random_state_dict

    factory = {"ani2xr": ANI2xr, "anir2s": ANIr2s, "ani2dr": ANI2dr}[kind]
    return factory(state_dict=random_state_dict(kind, 8, seed), device=dev, periodic_table_index=False,
                   neighborlist="batch" if batch else "auto", row_capacity=256)


def _x2r_case(base, dev):
    h = _npz(f"hess_x2r_ani2xr_{base}")
    sp = torch.from_numpy(h["species"]).to(dev)
    x = torch.from_numpy(h["coords"]).to(dev)
    cell = torch.from_numpy(h["cell"]).to(dev) if "cell" in h else None
    pbc = torch.from_numpy(h["pbc"]).to(dev) if "pbc" in h else None
    model = _x2r_model("ani2xr", int(h["seed"]), dev, batch=cell is None or sp.shape[0] > 1)
    return h, model, sp, x, cell, pbc


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def _check_against_dense(label, model, sp, x, cell, pbc):
    from torchani_amd import grad

    sparse, ts = _timed(lambda: grad.energies_forces_and_sparse_hessians(model, sp, x, cell=cell, pbc=pbc))
    dense, td = _timed(lambda: grad.energies_forces_and_hessians(model, sp, x, cell=cell, pbc=pbc))
    ef = grad.energies_and_forces(model, sp, x, cell, pbc, keep_vars=False)
    assert torch.allclose(sparse.energies, ef.energies, rtol=1e-12, atol=1e-9)
    assert torch.allclose(sparse.forces, ef.forces, rtol=0, atol=1e-6)
    H = sparse.hessians
    assert H.blocks.dtype == torch.float32 and H.index.dtype == torch.int64
    assert (H.n_molecules, H.n_atoms) == tuple(sp.shape)
    Hs = H.to_dense()
    Hd = dense.hessians.to(torch.float32)
    scale = Hd.abs().max().item()
    spread = (Hs - Hd).abs().max().item() / scale
    report(f"sparse vs dense {label}: max|dH| / max|H| = {spread:.2e}; nnz {H.nnz}; sparse {1e3 * ts:.1f} ms, "
           f"dense {1e3 * td:.1f} ms (first calls)")
    assert spread <= DENSE_GATE
    return H, Hs, Hd


@pytest.mark.parametrize("base", ANI_BASES)
def test_sparse_matches_dense_and_reference(dev, base):
    model, sp, x, cell, pbc = _case(base, dev)
    H, Hs, _ = _check_against_dense(base, model, sp, x, cell, pbc)
    h = _npz("hess_" + base)
    ref = h["hess"]
    err = np.abs(Hs[:, h["hess_rows"]].double().cpu().numpy() - ref).max() / np.abs(ref).max()
    report(f"sparse vs reference {base}: max|H - H_ref| / max|H_ref| = {err:.2e}")
    assert err <= REF_GATE
    # padding atoms hold no blocks
    pad = torch.nonzero((sp < 0).reshape(-1)).reshape(-1)
    assert not torch.isin(H.index, pad).any()


@pytest.mark.parametrize("base", X2R_BASES)
def test_sparse_ani2xr_matches_dense_and_reference(dev, base):
    h, model, sp, x, cell, pbc = _x2r_case(base, dev)
    H, Hs, _ = _check_against_dense("ani2xr " + base, model, sp, x, cell, pbc)
    ref = h["hess"].astype(np.float64)
    err = np.abs(Hs[:, h["hess_rows"]].double().cpu().numpy() - ref).max() / np.abs(ref).max()
    report(f"sparse vs reference ani2xr {base}: max|H - H_ref| / max|H_ref| = {err:.2e}")
    assert err <= REF_GATE


def _check_pattern(label, H, Hd):
    C, A = H.n_molecules, H.n_atoms
    scale = Hd.abs().max().item()
    inside = torch.zeros((C * A, C * A), dtype=torch.bool, device=Hd.device)
    inside[H.index[0], H.index[1]] = True
    mol = torch.arange(C * A, device=Hd.device) // A
    assert torch.all(mol[H.index[0]] == mol[H.index[1]])
    dense_blocks = Hd.reshape(C, A, 3, A, 3).abs().amax(dim=(2, 4))   # [C, A, A]
    outside = torch.stack([dense_blocks[c][~inside[c * A:(c + 1) * A, c * A:(c + 1) * A]].max()
                           if (~inside[c * A:(c + 1) * A, c * A:(c + 1) * A]).any() else dense_blocks.new_zeros(())
                           for c in range(C)]).max().item()
    # every stored (i, j) has (j, i) stored, with the transposed block
    key = H.index[0] * (C * A) + H.index[1]
    tkey = H.index[1] * (C * A) + H.index[0]
    order = torch.argsort(key)
    pos = torch.searchsorted(key[order], tkey)
    assert torch.all(key[order][pos.clamp(max=key.numel() - 1)] == tkey)
    asym = (H.blocks - H.blocks[order[pos]].transpose(1, 2)).abs().max().item() / scale
    report(f"pattern {label}: nnz {H.nnz} ({H.nnz / (C * A):.0f} per atom), dense outside the pattern "
           f"{outside / scale:.1e} of max|H|, block asymmetry {asym:.1e}")
    assert outside <= 1e-9 * scale
    assert asym <= 1e-5


def test_pattern_complete_small(dev):
    model, sp, x, cell, pbc = _case("small_ani2x", dev)
    H, Hs, Hd = _check_against_dense("small_ani2x", model, sp, x, cell, pbc)
    _check_pattern("small_ani2x", H, Hd)


def test_1hz5(dev):
    from torchani_amd import grad

    g = load_golden("1hz5_ani2x")
    from torchani_amd.models import ANI2x

    model = ANI2x(state_dict=seeded_state("ani2x", 8, g["seed"]), device=dev, periodic_table_index=False,
                  cutoff_fn=g["cutoff_fn"], row_capacity=256)
    sp = torch.from_numpy(g["species"].astype(np.int64)).to(dev)
    x = torch.from_numpy(g["coords"]).to(dev)
    H, Hs, Hd = _check_against_dense("1hz5_ani2x", model, sp, x, None, None)
    _check_pattern("1hz5_ani2x", H, Hd)
    # warm timings, median of 3
    ts = sorted(_timed(lambda: grad.energies_forces_and_sparse_hessians(model, sp, x))[1] for _ in range(3))[1]
    td = sorted(_timed(lambda: grad.energies_forces_and_hessians(model, sp, x))[1] for _ in range(3))[1]
    report(f"1hz5_ani2x (973 atoms): sparse {1e3 * ts:.1f} ms, dense {1e3 * td:.1f} ms (median of 3)")


def test_solvated_box_46k(dev):
    from torchani_amd import grad
    from torchani_amd.models import ANI2x

    g = load_golden("cfg3_1hz5_water_ani2x")
    model = ANI2x(state_dict=seeded_state("ani2x", 8, g["seed"]), device=dev, periodic_table_index=False,
                  cutoff_fn=g["cutoff_fn"], row_capacity=256)
    sp = torch.from_numpy(g["species"].astype(np.int64)).to(dev)
    x = torch.from_numpy(g["coords"]).to(dev)
    cell = torch.from_numpy(g["cell"]).to(dev)
    pbc = torch.from_numpy(np.asarray(g["pbc"])).to(dev)
    torch.cuda.reset_peak_memory_stats()
    out, t = _timed(lambda: grad.energies_forces_and_sparse_hessians(model, sp, x, cell=cell, pbc=pbc))
    peak = torch.cuda.max_memory_allocated()
    H = out.hessians
    N = sp.numel()
    scale = H.blocks.abs().max().item()
    report(f"cfg3_1hz5_water_ani2x ({N} atoms): sparse {t:.2f} s, nnz {H.nnz} ({H.nnz / N:.0f} per atom), "
           f"peak device memory {peak / 2**30:.2f} GiB")
    # translational sum rule: sum_j H[i, j] = 0
    rowsum = torch.zeros((N, 3, 3), dtype=torch.float64, device=dev).index_add_(0, H.index[0], H.blocks.double())
    sum_rule = rowsum.abs().max().item() / scale
    # block symmetry
    key = H.index[0] * N + H.index[1]
    order = torch.argsort(key)
    pos = torch.searchsorted(key[order], H.index[1] * N + H.index[0])
    asym = (H.blocks - H.blocks[order[pos]].transpose(1, 2)).abs().max().item() / scale
    # six columns against central differences of the forces, and against the analytic Hessian-vector product of the
    # autograd path (one direction through the dense kernels; H is symmetric, so its row (a, c) is column (a, c))
    h = 1e-3
    worst_fd = worst_hvp = 0.0
    rng = np.random.default_rng(7)
    xs = x.detach().clone().requires_grad_(True)
    f = grad.forces(model((sp, xs), cell, pbc).energies, xs, retain_graph=True, create_graph=True)
    for a in rng.choice(N, 6, replace=False):
        a = int(a)
        c = int(rng.integers(3))
        col = torch.zeros((N, 3), dtype=torch.float64, device=dev)
        sel = H.index[1] == a
        col[H.index[0][sel]] = H.blocks[sel][:, :, c].double()
        cmax = col.abs().max().item()
        (gr,) = torch.autograd.grad(f[0, a, c], xs, retain_graph=True)
        worst_hvp = max(worst_hvp, (col + gr[0].double()).abs().max().item() / cmax)
        xp, xm = x.clone(), x.clone()
        xp[0, a, c] += h
        xm[0, a, c] -= h
        fp = grad.energies_and_forces(model, sp, xp, cell, pbc, keep_vars=False).forces[0].double()
        fm = grad.energies_and_forces(model, sp, xm, cell, pbc, keep_vars=False).forces[0].double()
        step = (xp[0, a, c] - xm[0, a, c]).item()                   # (the step the coordinates' precision holds)
        fd = -(fp - fm) / step                                       # [N, 3] = H[(j, y), (a, c)]
        worst_fd = max(worst_fd, (col - fd).abs().max().item() / cmax)
    report(f"cfg3_1hz5_water_ani2x: sum rule {sum_rule:.1e}, block asymmetry {asym:.1e}; six columns against the autograd "
           f"HVP {worst_hvp:.1e} and against central differences (h = {h} A) {worst_fd:.1e} of the column max")
    assert sum_rule <= 1e-4
    assert asym <= 1e-5
    assert worst_hvp <= 1e-5
    # (measured 9.2e-3, on the diagonal block: fp32 forces at coordinates up to 77 A and the O(h^2) truncation of the
    # Gaussians' steep higher derivatives; the error grows for h = 3e-3 and 1e-2, the sum rule and the symmetry above and
    # the agreement with the dense path on 1hz5 are what pin the values)
    assert worst_fd <= 2e-2


def test_matvec_matches_dense(dev):
    from torchani_amd import grad

    model, sp, x, cell, pbc = _case("rand_batch_ani2x", dev)
    H = grad.energies_forces_and_sparse_hessians(model, sp, x, cell=cell, pbc=pbc).hessians
    Hd = grad.energies_forces_and_hessians(model, sp, x, cell=cell, pbc=pbc).hessians.double()
    v = torch.randn(x.shape, dtype=torch.float32, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    v = v * (sp >= 0).unsqueeze(-1)
    ref = torch.einsum("cij,cj->ci", Hd, v.double().reshape(sp.shape[0], -1)).reshape(v.shape)
    out = H.matvec(v).double()
    assert (out - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    S = H.to_sparse_coo()
    assert torch.allclose(torch.sparse.mm(S, v.reshape(-1, 1)).reshape(v.shape).double(), out, rtol=1e-5, atol=1e-6)


def test_errors(dev):
    from torchani_amd import grad

    g = load_golden("rand_batch_ani2x")
    sp = torch.from_numpy(g["species"].astype(np.int64)).to(dev)
    x = torch.from_numpy(g["coords"]).to(dev)
    with pytest.raises(ValueError, match="cutoff"):
        grad.energies_forces_and_sparse_hessians(_x2r_model("anir2s", 5, dev), sp, x)
    with pytest.raises(NotImplementedError, match="TwoBodyDispersionD3"):
        grad.energies_forces_and_sparse_hessians(_x2r_model("ani2dr", 5, dev), sp, x)


def test_first_order_calls_launch_no_sparse_kernels(dev, monkeypatch):
    from torchani_amd import engine, grad
    from torchani_amd.potentials import _AnalyticPair

    calls = {}

    def counting(owner, name):
        orig = getattr(owner, name)

        def f(*a, **k):
            calls[name] = calls.get(name, 0) + 1
            return orig(*a, **k)

        monkeypatch.setattr(owner, name, f)

    for name in ("hessian_pattern", "hessian_items", "hessian_extract"):
        counting(engine, name)
    counting(engine.AevEngine, "jvp_items")
    counting(engine.AevEngine, "backward_second_items")
    counting(engine.PackedNetworks, "rows_hvp_prepare")
    counting(engine.PackedNetworks, "rows_hvp")
    counting(_AnalyticPair, "hvp_items")
    h, model, sp, x, cell, pbc = _x2r_case("rand_batch_ani2x", dev)
    grad.energies_and_forces(model, sp, x, cell, pbc)
    xs = x.detach().clone().requires_grad_(True)
    model((sp, xs), cell, pbc).energies.sum().backward()
    grad.energies_forces_and_hessians(model, sp, x, cell=cell, pbc=pbc)
    assert sum(calls.values()) == 0
    grad.energies_forces_and_sparse_hessians(model, sp, x, cell=cell, pbc=pbc)
    assert calls["hessian_pattern"] == 1 and calls["rows_hvp_prepare"] == 1
    n = calls["hessian_items"]
    assert n >= 1 and all(calls[k] == n for k in ("hessian_extract", "jvp_items", "backward_second_items", "rows_hvp",
                                                  "hvp_items"))
