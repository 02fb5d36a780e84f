"""Lowest normal modes of block-sparse Hessians (grad.sparse_vibrational_analysis) on the MI355X: the operator of
anihip_block_hessian_prepare / anihip_block_hessian_spmm against fp64 products of the dense mass-weighted Hessian, the
eigenpairs against fp64 eigh and grad.vibrational_analysis, the rigid-body projection, the 46 357-atom solvated box, the
convergence errors, and that the first-order and Hessian calls launch none of the new kernels."""
import math
import os
import time

import numpy as np
import pytest
import torch

from _util import load_golden, seeded_state
from test_sparse_modes_host import dense_operator, reference_operator_blocks

pytestmark = pytest.mark.gpu

REPORT = os.environ.get("TORCHANI_AMD_HESSIAN_REPORT")
TOL = 1e-6


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


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def _masses(g, sp):
    from torchani_amd.extras.io import PERIODIC_TABLE
    from torchani_amd.utils import atomic_numbers_to_masses

    z = torch.tensor([PERIODIC_TABLE.index(s) for s in g["symbols"]], device=sp.device)
    an = torch.where(sp >= 0, z[sp.clamp(min=0)], torch.full_like(sp, -1))
    return atomic_numbers_to_masses(an, dtype=torch.float64)


_CACHE = {}


def _case(base, dev, kind="ani2x", cache=True):
    """(BlockHessian, masses [C, A] fp64, species, coordinates, pbc) of a fixture, cached per module."""
    key = (base, kind)
    if key in _CACHE:
        return _CACHE[key]
    from torchani_amd import grad
    from torchani_amd.models import ANI1x, ANI2x, ANI2xr
    from torchani_amd.weights import random_state_dict

    g = load_golden(base)
    sp = torch.from_numpy(g["species"].astype(np.int64)).to(dev)
    x = torch.from_numpy(g["coords"]).to(dev)
    cell = None if g["cell"] is None else torch.from_numpy(g["cell"]).to(dev)
    pbc = None if g["pbc"] is None else torch.from_numpy(np.asarray(g["pbc"])).to(dev)
    if kind == "ani2xr":
        model = ANI2xr(state_dict=random_state_dict("ani2xr", 8, 5), device=dev, periodic_table_index=False,
                       neighborlist="batch", row_capacity=256)
    else:
        ctor = ANI2x if g["kind"] == "ani2x" else ANI1x
        model = ctor(state_dict=seeded_state(g["kind"], 8, g["seed"]), device=dev, periodic_table_index=False,
                     cutoff_fn=g["cutoff_fn"], row_capacity=256)
    H = grad.energies_forces_and_sparse_hessians(model, sp, x, cell=cell, pbc=pbc).hessians
    out = (H, _masses(g, sp), sp, x, pbc)
    if cache:
        _CACHE[key] = out
    return out


@pytest.mark.parametrize("base", ["small_ani2x", "rand_batch_ani2x", "water_pbc_ani2x", "1hz5_ani2x"])
def test_operator_matches_dense(dev, base):
    from torchani_amd.engine import block_hessian_prepare, block_hessian_spmm

    H, masses, sp, _, _ = _case(base, dev)
    C, A = H.n_molecules, H.n_atoms
    op = block_hessian_prepare(H.index, H.blocks, masses.reshape(-1))
    assert torch.equal(op.diag >= 0, (sp >= 0).reshape(-1))
    ab = reference_operator_blocks(H.index, H.blocks, masses)
    assert (op.ablocks.double() - ab).abs().max().item() <= 1e-6 * ab.abs().max().item()
    assert torch.equal(op.rows.long(), H.index[0])
    Aref = dense_operator(H, masses)
    bound = op.gersh.view(C, A).amax(dim=1)
    assert torch.allclose(bound, Aref.abs().sum(dim=2).amax(dim=1), rtol=1e-6, atol=0)
    g = torch.Generator(device=dev).manual_seed(3)
    dof = (sp >= 0).repeat_interleave(3, dim=1)
    worst = 0.0
    for m in (1, 7, 32, 64):
        X = torch.randn((C, 3 * A, m), device=dev, generator=g) * dof.unsqueeze(2)
        Y = block_hessian_spmm(op, X)
        ref = Aref @ X.double()
        xn = X.double().norm(dim=1).amax(dim=1)                                      # [C]
        err = ((Y.double() - ref).abs().amax(dim=(1, 2)) / (bound * xn)).max().item()
        worst = max(worst, err)
        assert err <= 1e-6
        assert torch.equal(Y, block_hessian_spmm(op, X))                             # no atomics: bit-identical
        assert torch.all(Y[~dof] == 0)
    report(f"spmm {base}: max |Y - A X| / (||A||_G ||X||) = {worst:.1e} over m = 1, 7, 32, 64")


def _dense_reference(H, masses, c, project=None):
    """fp64 (eigenvalues, vectors [3A, d], operator) of molecule c's A over its real atoms (vectors embedded back into 3A),
    restricted to the range of the projector `project` when one is given."""
    Aref = dense_operator(H, masses)[c]
    real = (masses[c] > 0).repeat_interleave(3)
    B = torch.eye(Aref.shape[0], dtype=torch.float64, device=Aref.device)[:, real]
    if project is not None:
        U, s, _ = torch.linalg.svd(project @ B, full_matrices=False)
        B = U[:, s > 1e-8 * s[0]]
        Aref = project @ Aref @ project   # the operator the projected problem solves
    lam, V = torch.linalg.eigh(B.T @ Aref @ B)
    return lam, B @ V, Aref


def _check_against_dense(label, H, masses, va, n, project=None, rigid=None):
    from torchani_amd import grad, units

    C, A = H.n_molecules, H.n_atoms
    Ad = dense_operator(H, masses)
    bound = Ad.abs().sum(dim=2).amax(dim=1)
    worst_lam = worst_res = 0.0
    for c in range(C):
        lam, V, Ac = _dense_reference(H, masses, c, None if project is None else project[c])
        th = va.eigenvalues[c]
        mw = va.modes[c].reshape(n, 3 * A).T                                    # (mode_kind "mwn")
        worst_lam = max(worst_lam, ((th - lam[:n]).abs().max() / bound[c]).item())
        res = (Ac @ mw - mw * th).norm(dim=0)
        worst_res = max(worst_res, (res.max() / bound[c]).item())
        assert (th - lam[:n]).abs().max().item() <= TOL * bound[c].item()
        assert res.max().item() <= TOL * bound[c].item()
        if rigid is not None:
            assert (rigid[c].T @ mw).abs().max().item() <= 1e-8
        lam_ext = torch.cat([lam, lam.new_full((1,), math.inf)])
        gapped = []
        for i in range(n):
            gap = min((lam[i] - lam[i - 1]).abs().item() if i else math.inf, (lam_ext[i + 1] - lam[i]).abs().item())
            if gap > 1e-3 * bound[c].item():
                assert abs(torch.dot(V[:, i], mw[:, i]).item()) >= 0.999
                gapped.append(i)
        if project is None and gapped:
            real = masses[c] > 0
            Hd = H.to_dense()[c].double().reshape(A, 3, A, 3)[real][:, :, real].reshape(1, -1, 3 * int(real.sum()))
            ref = grad.vibrational_analysis(masses[c:c + 1, real], Hd)
            dsq = units.sqrt_mhessian2invcm(math.sqrt(2 * TOL * bound[c].item()) / (2 * math.pi))
            assert torch.allclose(va.freqs[c], ref.freqs[:n], rtol=1e-6, atol=dsq)
            gi = torch.tensor(gapped, device=va.freqs.device)
            assert torch.allclose(va.rmasses[c, gi], ref.rmasses[gi], rtol=1e-2)
            assert torch.allclose(va.fconstants[c, gi], ref.fconstants[gi], rtol=1e-2, atol=1e-6)
    report(f"modes {label}: {n} modes, n_iter {va.n_iter}, max |theta - lambda| {worst_lam:.1e} and residual "
           f"{worst_res:.1e} of ||A||_G")


@pytest.mark.parametrize("base,kind", [("small_ani2x", "ani2x"), ("1hz5_ani2x", "ani2x"), ("small_ani2x", "ani2xr"),
                                       ("rand_batch_ani2x", "ani2x"), ("water_pbc_ani2x", "ani2x")])
def test_eigenpairs_against_dense(dev, base, kind):
    from torchani_amd import grad

    H, masses, sp, _, _ = _case(base, dev, kind)
    n = min(20, 3 * int((sp >= 0).sum(dim=1).min()))
    va, t = _timed(lambda: grad.sparse_vibrational_analysis(masses, H, n, mode_kind="mwn"))
    assert va.freqs.shape == (H.n_molecules, n) and va.modes.shape == (H.n_molecules, n, H.n_atoms, 3)
    assert torch.all(va.modes.transpose(1, 2)[sp < 0] == 0)
    _check_against_dense(f"{kind} {base}", H, masses, va, n)
    again = grad.sparse_vibrational_analysis(masses, H, n, mode_kind="mwn")
    assert torch.equal(again.eigenvalues, va.eigenvalues) and torch.equal(again.modes, va.modes)
    report(f"modes {kind} {base}: {1e3 * t:.1f} ms (first call)")


def test_ch4_dense_route(dev):
    from torchani_amd import grad

    H, masses, sp, _, _ = _case("ch4_ani1x", dev)
    n = 3 * int((sp >= 0).sum(dim=1).min())
    va = grad.sparse_vibrational_analysis(masses, H, n, mode_kind="mwn")
    assert va.n_iter == 0
    _check_against_dense("ch4_ani1x", H, masses, va, n)
    with pytest.raises(ValueError, match="n_modes"):
        grad.sparse_vibrational_analysis(masses, H, n + 1)


def _rigid(masses, x, rotations):
    """[C, 3A, r] orthonormal mass-weighted rigid-body vectors (numpy), zero on padding."""
    out = []
    for c in range(masses.shape[0]):
        m = masses[c].cpu().numpy()
        real = m > 0
        r = x[c].double().cpu().numpy()
        sm = np.sqrt(np.where(real, m, 0.0))
        com = (m[real, None] * r[real]).sum(0) / m[real].sum()
        vs = []
        for e in np.eye(3):
            vs.append((sm[:, None] * e).reshape(-1))
            if rotations:
                vs.append((sm[:, None] * np.cross(e, (r - com) * real[:, None])).reshape(-1))
        u, s, _ = np.linalg.svd(np.stack(vs, 1), full_matrices=False)
        out.append(torch.from_numpy(u[:, s > 1e-8 * s[0]]).to(masses.device))
    return out


@pytest.mark.parametrize("base", ["small_ani2x", "water_pbc_ani2x"])
def test_project_rigid(dev, base):
    from torchani_amd import grad

    H, masses, sp, x, pbc = _case(base, dev)
    periodic = pbc is not None and bool(pbc.any())
    R = _rigid(masses, x, not periodic)
    assert R[0].shape[1] == (3 if periodic else 6)
    va = grad.sparse_vibrational_analysis(masses, H, 12, mode_kind="mwn", project_rigid=True, coordinates=x, pbc=pbc)
    proj = [torch.eye(3 * H.n_atoms, dtype=torch.float64, device=dev) - r @ r.T for r in R]
    _check_against_dense(f"{base} project_rigid", H, masses, va, 12, project=proj, rigid=R)


def test_not_converged(dev):
    from torchani_amd import grad

    H, masses, _, _, _ = _case("small_ani2x", dev)
    with pytest.raises(RuntimeError, match="did not converge"):
        grad.sparse_vibrational_analysis(masses, H, 20, max_iter=1)
    va = grad.sparse_vibrational_analysis(masses, H, 20, max_iter=1, check=False)
    bound = dense_operator(H, masses).abs().sum(dim=2).amax()
    assert va.n_iter == 1 and (va.residuals > TOL * bound).any()


def test_hand_built_unsorted_and_errors(dev):
    from torchani_amd import grad
    from torchani_amd.tuples import BlockHessian

    H, masses, _, _, _ = _case("small_ani2x", dev)
    perm = torch.randperm(H.nnz, generator=torch.Generator().manual_seed(0)).to(dev)
    Hp = BlockHessian(H.index[:, perm], H.blocks[perm], H.n_molecules, H.n_atoms)
    a = grad.sparse_vibrational_analysis(masses, H, 6)
    b = grad.sparse_vibrational_analysis(masses, Hp, 6)
    assert torch.equal(a.eigenvalues, b.eigenvalues)
    bad = masses.clone()
    bad[0, 3] = 0.0
    with pytest.raises(ValueError, match="masses"):
        grad.sparse_vibrational_analysis(bad, H, 6)
    off = (H.index[0] != H.index[1]).nonzero()[0, 0]
    keep = torch.ones(H.nnz, dtype=torch.bool, device=dev)
    keep[off] = False
    with pytest.raises(ValueError, match="symmetric"):
        grad.sparse_vibrational_analysis(masses, BlockHessian(H.index[:, keep], H.blocks[keep], 1, H.n_atoms), 6)


def test_solvated_box_46k(dev):
    from torchani_amd import grad

    H, masses, sp, x, pbc = _case("cfg3_1hz5_water_ani2x", dev, cache=False)   # (3.8 GiB: not kept)
    N = sp.numel()
    torch.cuda.reset_peak_memory_stats()
    base_mem = torch.cuda.memory_allocated()
    va, t = _timed(lambda: grad.sparse_vibrational_analysis(masses, H, 10, mode_kind="mwn"))
    peak = torch.cuda.max_memory_allocated() - base_mem
    from torchani_amd.engine import block_hessian_prepare

    bound = block_hessian_prepare(H.index, H.blocks, masses.reshape(-1)).gersh.max().item()
    q = va.modes[0].reshape(10, -1).T                                           # [3N, 10] mass-weighted, unit
    gram = q.T @ q
    orth = (gram - torch.eye(10, dtype=torch.float64, device=dev)).abs().max().item()
    w = masses.reshape(-1).rsqrt().repeat_interleave(3)
    rq = torch.stack([(q[:, i] * w).dot(H.matvec((q[:, i] * w).float()).double()) for i in range(10)])
    dq = (rq - va.eigenvalues[0]).abs().max().item() / bound
    report(f"cfg3_1hz5_water_ani2x ({N} atoms): 10 modes in {t:.2f} s, n_iter {va.n_iter}, peak device memory above the "
           f"Hessian {peak / 2**30:.2f} GiB; residual {va.residuals.max().item() / bound:.1e}, orthonormality {orth:.1e}, "
           f"|theta - matvec Rayleigh quotient| {dq:.1e} of ||A||_G; lowest {va.eigenvalues[0, :3].tolist()}")
    assert va.residuals.max().item() <= TOL * bound
    assert orth <= 1e-10
    assert dq <= 1e-5


def test_hessian_calls_launch_no_mode_kernels(dev, monkeypatch):
    from torchani_amd import engine, grad

    calls = {}

    def counting(name):
        orig = getattr(engine, name)

        def f(*a, **k):
            calls[name] = calls.get(name, 0) + 1
            return orig(*a, **k)

        monkeypatch.setattr(engine, name, f)

    counting("block_hessian_prepare")
    counting("block_hessian_spmm")
    from torchani_amd.models import ANI2x

    g = load_golden("rand_batch_ani2x")
    model = ANI2x(state_dict=seeded_state("ani2x", 8, g["seed"]), device=dev, periodic_table_index=False, row_capacity=256)
    sp = torch.from_numpy(g["species"].astype(np.int64)).to(dev)
    x = torch.from_numpy(g["coords"]).to(dev)
    grad.energies_and_forces(model, sp, x)
    H = grad.energies_forces_and_sparse_hessians(model, sp, x).hessians
    grad.energies_forces_and_hessians(model, sp, x)
    assert sum(calls.values()) == 0
    grad.sparse_vibrational_analysis(_masses(g, sp), H, 6)
    assert calls["block_hessian_prepare"] == 1 and calls["block_hessian_spmm"] >= 1
