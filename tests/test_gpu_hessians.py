"""Hessians with respect to the coordinates on the MI355X: the batched path (grad.energies_forces_and_hessians) and the
autograd path (grad.forces_and_hessians / Hessian-vector products) against the reference's own fp64 second derivatives
(tests/golden/hess_*.npz, gen_golden_hessians.py), their structure, the number of kernel calls, and the errors."""
import math
import os

import numpy as np
import pytest
import torch

from _util import load_golden, seeded_state

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the measured worst cases go to stdout and, when TORCHANI_AMD_HESSIAN_REPORT names a file, are appended to it
REPORT = os.environ.get("TORCHANI_AMD_HESSIAN_REPORT")
BASES = ("ch4_ani1x", "rand_batch_ani2x", "water_pbc_ani2x", "water_pbc_smooth_ani2x", "triclinic_pbc_ani2x",
         "dense90_ani2x", "small_ani2x")
GATE = 2e-5   # max |H - H_ref| <= GATE * max |H_ref| (measured worst case: 4.8e-6, water_pbc_ani2x)


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


def _hess(base):
    with np.load(os.path.join(GOLDEN, "hess_" + base + ".npz")) as z:
        return {k: z[k] for k in z.files}


def _case(base, dev, trainable=False):
    from torchani_amd.models import ANI1x, ANI2x

    g = load_golden(base)
    ctor = ANI2x if g["kind"] == "ani2x" else ANI1x
    model = ctor(state_dict=seeded_state(g["kind"], 8, g["seed"]), device=dev, periodic_table_index=False,
                 cutoff_fn=g["cutoff_fn"], row_capacity=256)
    if trainable:
        model.neural_networks.requires_grad_(True)
    sp = torch.from_numpy(g["species"].astype(np.int64)).to(dev)
    x = torch.from_numpy(g["coords"]).to(dev)
    cell = None if g["cell"] is None else torch.from_numpy(g["cell"]).to(dev)
    pbc = None if g["pbc"] is None else torch.from_numpy(np.asarray(g["pbc"])).to(dev)
    return g, model, sp, x, cell, pbc


def _autograd_rows(model, sp, x, cell, pbc, rows):
    from torchani_amd import grad

    xs = x.detach().clone().requires_grad_(True)
    e = model((sp, xs), cell, pbc).energies
    if len(rows) == 3 * x.shape[1]:
        return grad.forces_and_hessians(e, xs).hessians
    f = grad.forces(e, xs, retain_graph=True, create_graph=True).reshape(x.shape[0], -1)
    out = []
    for j in rows:
        (gj,) = torch.autograd.grad(f[:, j].sum(), xs, retain_graph=True)
        out.append(-gj.reshape(x.shape[0], 1, -1))
    return torch.cat(out, dim=1)


def _check_structure(H, sp, bound, full):
    C, n, _ = H.shape
    A = n // 3
    if full:
        assert (H - H.transpose(1, 2)).abs().max().item() <= bound
    # translational sum rule: sum over the atoms l of H[(k, a), (l, b)] = 0 (periodic boxes too)
    assert H.reshape(C, n, A, 3).sum(dim=2).abs().max().item() <= bound * math.sqrt(A)
    pad = (sp < 0).repeat_interleave(3, dim=1)
    if pad.any():
        assert torch.all(H.transpose(1, 2)[pad] == 0) and (not full or torch.all(H[pad] == 0))


@pytest.mark.parametrize("base", BASES)
def test_hessians_match_reference(dev, base):
    from torchani_amd import grad

    g, model, sp, x, cell, pbc = _case(base, dev)
    h = _hess(base)
    rows = h["hess_rows"]
    ref = h["hess"]
    scale = np.abs(ref).max()
    bound = GATE * scale
    efh = grad.energies_forces_and_hessians(model, sp, x, cell=cell, pbc=pbc)
    ef = grad.energies_and_forces(model, sp, x, cell, pbc, keep_vars=False)
    # (the same call; the forces' float atomics make two calls differ in the last bits)
    assert torch.allclose(efh.energies, ef.energies, rtol=1e-12, atol=1e-9)
    assert torch.allclose(efh.forces, ef.forces, rtol=0, atol=1e-6)
    Hb = efh.hessians
    assert Hb.shape == (x.shape[0], 3 * x.shape[1], 3 * x.shape[1]) and Hb.dtype == x.dtype
    err_b = np.abs(Hb[:, rows].double().cpu().numpy() - ref).max()
    Ha = _autograd_rows(model, sp, x, cell, pbc, rows)
    err_a = np.abs(Ha.double().cpu().numpy() - ref).max()
    report(f"hessian {base}: max|H_batched - H_ref| = {err_b:.2e}, max|H_autograd - H_ref| = {err_a:.2e}, "
           f"max|H_ref| = {scale:.2e} (gate {bound:.2e})")
    assert err_b <= bound and err_a <= bound
    _check_structure(Hb.double(), sp, bound, full=True)
    if len(rows) == 3 * x.shape[1]:
        _check_structure(Ha.double(), sp, bound, full=True)


@pytest.mark.parametrize("base", ["ch4_ani1x", "water_pbc_ani2x", "rand_batch_ani2x"])
def test_hvp_through_autograd(dev, base):
    from torchani_amd import grad

    g, model, sp, x, cell, pbc = _case(base, dev)
    ref = torch.from_numpy(_hess(base)["hess"])
    w = torch.from_numpy(np.random.RandomState(3).standard_normal(x.shape)).to(dev).to(x.dtype)
    xs = x.detach().clone().requires_grad_(True)
    e = model((sp, xs), cell, pbc).energies
    f = grad.forces(e, xs, retain_graph=True, create_graph=True)
    (hv,) = torch.autograd.grad((f * w).sum(), xs)
    want = -(ref @ w.double().cpu().reshape(x.shape[0], -1, 1)).reshape(x.shape)
    err = (hv.double().cpu() - want).abs().max().item()
    report(f"hvp {base}: max|autograd((F w).sum(), x) + H_ref w| = {err:.2e} (max {want.abs().max().item():.2e})")
    assert err <= GATE * ref.abs().max().item() * math.sqrt(w.numel())


def test_batched_call_counts(dev, monkeypatch):
    from torchani_amd import grad
    from torchani_amd.engine import AevEngine, PackedNetworks

    calls = {"jvp_batched": 0, "backward_second": 0, "input_hvp": 0}

    def counting(cls, name):
        orig = getattr(cls, name)

        def f(*a, **k):
            calls[name] += 1
            return orig(*a, **k)

        monkeypatch.setattr(cls, name, f)

    counting(AevEngine, "jvp_batched")
    counting(AevEngine, "backward_second")
    counting(PackedNetworks, "input_hvp")
    g, model, sp, x, cell, pbc = _case("dense90_ani2x", dev)
    grad.energies_forces_and_hessians(model, sp, x, cell=cell, pbc=pbc)
    packed = model.neural_networks._pack(dev)
    N = sp.numel()
    K = grad.hessian_chunk_size(sp.shape[0], sp.shape[1], model.aev_computer.out_dim,
                                -(-grad._hvp_row_bytes(packed, N) // N))
    want = -(-3 * sp.shape[1] // K)
    assert want < 3 * sp.shape[1]
    assert calls == {"jvp_batched": want, "backward_second": want, "input_hvp": want}
    # first-order paths launch none of the new kernels: frozen, and trainable with create_graph (force training)
    for k in calls:
        calls[k] = 0
    grad.energies_and_forces(model, sp, x, cell, pbc)
    g2, m2, sp2, x2, cell2, pbc2 = _case("dense90_ani2x", dev, trainable=True)
    out = grad.energies_and_forces(m2, sp2, x2, cell2, pbc2, create_graph=True)
    (out.forces ** 2).sum().backward()
    assert calls == {"jvp_batched": 0, "backward_second": 0, "input_hvp": 0}


def test_errors(dev):
    from torchani_amd import grad
    from torchani_amd.models import ANI2dr

    g, model, sp, x, cell, pbc = _case("ch4_ani1x", dev, trainable=True)
    xs = x.detach().clone().requires_grad_(True)
    e = model((sp, xs)).energies
    with pytest.raises(RuntimeError, match="frozen parameters"):
        grad.forces_and_hessians(e, xs)
    g = load_golden("rand_batch_ani2x")
    m = ANI2dr(seed=5, n_members=2, device=dev, periodic_table_index=False)
    sp = torch.from_numpy(g["species"].astype(np.int64)).to(dev)
    x = torch.from_numpy(g["coords"]).to(dev)
    with pytest.raises(NotImplementedError, match="D3"):
        grad.energies_forces_and_hessians(m, sp, x)
    xs = x.detach().clone().requires_grad_(True)
    e = m((sp, xs)).energies
    with pytest.raises(NotImplementedError, match="RepulsionXTB|D3"):
        grad.forces_and_hessians(e, xs)


def test_vibrational_analysis_end_to_end(dev):
    from torchani_amd import grad, units

    g, model, sp, x, cell, pbc = _case("ch4_ani1x", dev)
    h = _hess("ch4_ani1x")
    H = grad.energies_forces_and_hessians(model, sp, x).hessians.double().cpu()
    masses = torch.from_numpy(h["masses"])
    va = grad.vibrational_analysis(masses, H)
    # eigenvalues of the mass-weighted Hessian move by at most ||M^-1/2 dH M^-1/2||_2 <= 3A GATE max|H_ref| / m_min
    lam = lambda f: np.sign(f) * (np.asarray(f) / units.SQRT_MHESSIAN_TO_INVCM * 2 * math.pi) ** 2   # noqa: E731
    bound = H.shape[1] * GATE * np.abs(h["hess"]).max() / h["masses"].min()
    err = np.abs(lam(va.freqs.numpy()) - lam(h["freqs_mdu_invcm"])).max()
    report(f"vibrational analysis ch4_ani1x: max|d eigenvalue| = {err:.2e} (bound {bound:.2e})")
    assert err <= bound


def test_general_grid_self_consistent(dev):
    """A from_constants grid (general kernels): batched = autograd, symmetric, sum rule, and the central differences of the
    engine's own forces (no reference fixture: the grid fixture carries no networks)."""
    from torchani_amd import grad
    from torchani_amd.aev import AEVComputer
    from torchani_amd.models import ANI
    from torchani_amd.nn import ANINetworks, Ensemble

    with np.load(os.path.join(GOLDEN, "grid_r8_a4z4_batch.npz")) as z:
        g = {k: z[k] for k in z.files}
    aevc = AEVComputer.from_constants(float(g["Rcr"]), float(g["Rca"]), float(g["EtaR"]), g["ShfR"].tolist(),
                                      float(g["EtaA"]), float(g["Zeta"]), g["ShfA"].tolist(), g["ShfZ"].tolist(), 4,
                                      row_capacity=256)
    torch.manual_seed(11)
    hidden = {"H": (64, 48, 32), "C": (64, 32, 32), "N": (32, 32, 32), "O": (48, 32, 32)}
    nets = Ensemble([ANINetworks.build(("H", "C", "N", "O"), aevc.out_dim, hidden) for _ in range(2)])
    model = ANI(("H", "C", "N", "O"), aevc, nets, [0.0] * 4, periodic_table_index=False).to(dev)
    model.requires_grad_(False)
    sp = torch.from_numpy(g["species"].astype(np.int64)).to(dev)
    x = torch.from_numpy(g["coords"]).to(dev).double()
    Hb = grad.energies_forces_and_hessians(model, sp, x).hessians
    xs = x.clone().requires_grad_(True)
    Ha = grad.forces_and_hessians(model((sp, xs)).energies, xs).hessians
    scale = Hb.abs().max().item()
    d_ab = (Ha - Hb).abs().max().item()
    # central differences of the fp32 forces, h = 3e-4 A, on a few columns: small, because the cosine envelope's second
    # derivative jumps at the cutoff and this batch has a pair within 1e-2 A of it (column 17: the difference falls with h,
    # 2.7e-3 at 1e-2, 6.4e-4 at 1e-3, 8e-5 at 3e-4); the fp32 noise ~1e-6 / h sets the floor
    C, A = sp.shape
    cols = [0, 7, 17, 3 * A - 1]
    fd = []
    for j in cols:
        h = 3e-4
        dx = torch.zeros_like(x).reshape(C, -1)
        dx[:, j] = h
        fp = grad.energies_and_forces(model, sp, x + dx.view_as(x)).forces.double()
        fm = grad.energies_and_forces(model, sp, x - dx.view_as(x)).forces.double()
        fd.append(-(fp - fm).reshape(C, -1) / (2 * h))
    fd = torch.stack(fd, dim=2)
    d_fd = (Hb[:, :, cols].double() - fd).abs().max().item()
    report(f"hessian general grid: max|H_batched - H_autograd| = {d_ab:.2e}, max|H - central differences| = {d_fd:.2e}, "
           f"max|H| = {scale:.2e}")
    assert d_ab <= GATE * scale and d_fd <= 1e-3 * scale
    _check_structure(Hb.double(), sp, GATE * scale, full=True)
