"""Strain second derivatives (grad.energies_forces_and_strain_hessians) on the MI355X: parity with the reference's fp64
double autograd (tests/golden/hess_strain_*.npz), the exact relations to the coordinate Hessian of molecules without a
cell, the 46 357-atom solvated box (symmetry, sum rule, central differences of the engine's own virial, time and peak
memory), and the errors."""
import os
import time

import numpy as np
import pytest
import torch

from _util import load_golden, seeded_state

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REPORT = os.environ.get("TORCHANI_AMD_HESSIAN_REPORT")
REF_GATE = 2e-5   # of max |ref|, as the Hessian tests
ANI_BASES = ("water_pbc_ani2x", "water_pbc_smooth_ani2x", "triclinic_pbc_ani2x", "benzene_pbc_ani2x", "rand_batch_ani2x")
X2R = (("ani2xr", "water_pbc_ani2x"), ("anir2s", "rand_batch_ani2x"))


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
    x = torch.from_numpy(g["coords"]).to(dev).double()
    cell = None if g["cell"] is None else torch.from_numpy(g["cell"]).to(dev).double()
    pbc = None if g["pbc"] is None else torch.from_numpy(np.asarray(g["pbc"])).to(dev)
    return model, sp, x, cell, pbc


def _x2r_model(kind, seed, dev, batch=True):
    from torchani_amd.models import ANI2dr, ANI2xr, ANIr2s
    from torchani_amd.weights import random_state_dict

    factory = {"ani2xr": ANI2xr, "anir2s": ANIr2s, "ani2dr": ANI2dr}[kind]
    return factory(state_dict=random_state_dict(kind, 8, seed), device=dev, periodic_table_index=False,
                   neighborlist="batch" if batch else "auto", row_capacity=256)


def _compare(label, res, ref):
    out = {}
    for key in ("strain_hessians", "internal_strain", "virial"):
        mine = getattr(res, key).detach().cpu().numpy()
        want = ref[key]
        assert mine.shape == want.shape, (key, mine.shape, want.shape)
        scale = np.abs(want).max()
        out[key] = np.abs(mine - want).max() / scale
    report(f"strain {label}: max|d| / max|ref|: strain_hessians {out['strain_hessians']:.2e}, internal_strain "
           f"{out['internal_strain']:.2e}, virial {out['virial']:.2e}")
    for key, v in out.items():
        assert v <= REF_GATE, (key, v)


@pytest.mark.parametrize("base", ANI_BASES)
def test_strain_matches_reference(dev, base):
    from torchani_amd import grad

    model, sp, x, cell, pbc = _case(base, dev)
    res = grad.energies_forces_and_strain_hessians(model, sp, x, cell=cell, pbc=pbc)
    ef = grad.energies_and_forces(model, sp, x, cell, pbc, keep_vars=False)
    assert torch.allclose(res.energies, ef.energies, rtol=1e-12, atol=1e-9)
    assert torch.allclose(res.forces, ef.forces, rtol=0, atol=1e-6)
    assert res.strain_hessians.dtype == x.dtype and res.strain_hessians.shape == (sp.shape[0], 3, 3, 3, 3)
    assert res.internal_strain.shape == (sp.shape[0], sp.shape[1], 3, 3, 3)
    _compare(base, res, _npz("hess_strain_" + base))


@pytest.mark.parametrize("kind,base", X2R)
def test_strain_pair_models_match_reference(dev, kind, base):
    from torchani_amd import grad

    h = _npz(f"hess_strain_x2r_{kind}_{base}")
    sp = torch.from_numpy(h["species"]).to(dev)
    x = torch.from_numpy(h["coords"]).to(dev).double()
    cell = torch.from_numpy(h["cell"]).to(dev).double() if "cell" in h else None
    pbc = torch.from_numpy(h["pbc"]).to(dev) if "pbc" in h else None
    model = _x2r_model(kind, int(h["seed"]), dev, batch=cell is None or sp.shape[0] > 1)
    res = grad.energies_forces_and_strain_hessians(model, sp, x, cell=cell, pbc=pbc)
    _compare(f"{kind} {base}", res, h)


@pytest.mark.parametrize("base", ("small_ani2x", "dense90_ani2x"))
def test_molecule_strain_equals_hessian_contractions(dev, base):
    """Without a cell E(x S) depends on S only through the displacement x E_ab: the mixed block is H vec(x E_ab) plus the
    force term and the strain-strain block is vec(x E_ab)^T H vec(x E_pq), with H the batched coordinate Hessian."""
    from torchani_amd import grad

    model, sp, x, cell, pbc = _case(base, dev)
    res = grad.energies_forces_and_strain_hessians(model, sp, x)
    hess = grad.energies_forces_and_hessians(model, sp, x)
    H = hess.hessians.double()
    C, A = sp.shape
    real = (sp >= 0).double().unsqueeze(-1)
    xr = x.double() * real
    T = torch.zeros((C, A, 3, 3, 3), dtype=torch.float64, device=dev)   # [c, i, y, a, b] = x_ia delta_by
    for a in range(3):
        for b in range(3):
            T[:, :, b, a, b] = xr[:, :, a]
    Tf = T.reshape(C, 3 * A, 9)
    HT = (H @ Tf).reshape(C, A, 3, 3, 3)
    eye = torch.eye(3, dtype=torch.float64, device=dev)
    mixed = HT - eye.view(1, 1, 3, 3, 1) * hess.forces.double().view(C, A, 1, 1, 3)
    W = Tf.transpose(1, 2) @ H @ Tf
    d_mixed = (res.internal_strain.double() - mixed).abs().max().item() / mixed.abs().max().item()
    d_w = (res.strain_hessians.double().reshape(C, 9, 9) - W).abs().max().item() / W.abs().max().item()
    report(f"strain {base} vs Hessian contractions: mixed {d_mixed:.2e}, strain-strain {d_w:.2e}")
    assert d_mixed <= REF_GATE and d_w <= REF_GATE


def test_big_box(dev):
    """The 46 357-atom solvated box: symmetry, translational sum rule, and central differences of the engine's own
    first-order virial (ANI.energies_and_forces(stress=True)) along three strain directions.  That virial V(y) is the
    derivative with respect to a strain T applied on top of the strained geometry y = x S, so d E(x S) / d S = S^-T V(x S)
    is what is differenced."""
    from torchani_amd import grad

    model, sp, x, cell, pbc = _case("cfg3_1hz5_water_ani2x", dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base_mem = torch.cuda.memory_allocated(dev)
    grad.energies_forces_and_strain_hessians(model, sp, x, cell=cell, pbc=pbc)   # (warm-up: kernels and pack)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = grad.energies_forces_and_strain_hessians(model, sp, x, cell=cell, pbc=pbc)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    peak = (torch.cuda.max_memory_allocated(dev) - base_mem) / 2 ** 30
    W = res.strain_hessians.double().reshape(9, 9)
    scale = W.abs().max().item()
    asym = (W - W.T).abs().max().item() / scale
    ist = res.internal_strain.double()
    sum_rule = ist.sum(dim=1).abs().max().item() / ist.abs().max().item()
    h = 1e-3
    fd_err = []
    c32 = x.to(torch.float32)
    cell32 = cell.to(torch.float32)
    for (a, b) in ((0, 0), (1, 2), (2, 1)):
        E = torch.zeros((3, 3), dtype=torch.float32, device=dev)
        E[a, b] = h
        vs = []
        for sgn in (1.0, -1.0):
            S = torch.eye(3, dtype=torch.float32, device=dev) + sgn * E
            out = model.energies_and_forces(sp, c32 @ S, cell32 @ S, pbc, stress=True)
            vs.append(torch.linalg.inv(S.double()).T @ out.virial.double())
        fd = (vs[0] - vs[1]) / (2 * h)
        col = W[:, 3 * a + b].view(3, 3)
        fd_err.append((fd - col).abs().max().item() / col.abs().max().item())
    report(f"strain 46k box: {1e3 * dt:.0f} ms, peak {peak:.2f} GiB above the inputs; asymmetry {asym:.2e}, sum rule "
           f"{sum_rule:.2e}, central differences of the virial (h = {h}) {max(fd_err):.2e} of the column max")
    assert asym <= 1e-4 and sum_rule <= 1e-4
    assert max(fd_err) <= 2e-2


def test_errors(dev):
    from torchani_amd import grad

    h = _npz("hess_strain_x2r_ani2xr_water_pbc_ani2x")
    sp = torch.from_numpy(h["species"]).to(dev)
    x = torch.from_numpy(h["coords"]).to(dev)
    cell = torch.from_numpy(h["cell"]).to(dev)
    pbc = torch.from_numpy(h["pbc"]).to(dev)
    d3 = _x2r_model("ani2dr", 21, dev, batch=False)
    with pytest.raises(NotImplementedError, match="TwoBodyDispersionD3"):
        grad.energies_forces_and_strain_hessians(d3, sp, x, cell=cell, pbc=pbc)
    model, sp2, x2, cell2, pbc2 = _case("triclinic_pbc_ani2x", dev)
    res = grad.energies_forces_and_strain_hessians(model, sp2, x2, cell=cell2, pbc=pbc2)
    with pytest.raises(ValueError):
        grad.elastic_constants(res, cell2, pbc=pbc2)
    with pytest.raises(ValueError):
        grad.elastic_constants(res, None)
    C = grad.elastic_constants(res, cell2)   # (a cell without pbc: taken as periodic)
    assert C.shape == (1, 6, 6) and torch.allclose(C, C.transpose(1, 2), rtol=1e-4, atol=1e-6 * C.abs().max().item())
