"""Hessians with respect to the coordinates of models with closed-form pair potentials (ANI-2xr, ANI-r2s) and of the
standalone pair potentials, on the MI355X: both paths (grad.energies_forces_and_hessians and grad.forces_and_hessians)
against the reference's own fp64 second derivatives (tests/golden/hess_x2r_*.npz, hess_pairs_*.npz,
gen_golden_hessians_pairs.py), their structure, Hessian-vector products, a cell in which an atom sees its own image,
vibrational analysis, the number of pair HVP launches of first-order calls, and the errors that remain."""
import math
import os

import numpy as np
import pytest
import torch

from _util import load_golden

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REPORT = os.environ.get("TORCHANI_AMD_HESSIAN_REPORT")
GATE = 2e-5   # max |H - H_ref| <= GATE * max |H_ref|, as test_gpu_hessians.py
MODEL_CASES = [("ani2xr", "rand_batch_ani2x"), ("ani2xr", "water_pbc_ani2x"), ("ani2xr", "small_ani2x"),
               ("anir2s", "rand_batch_ani2x"), ("anir2s", "dense90_ani2x")]
STANDALONE_BASES = ("rand_batch_ani2x", "water_pbc_ani2x", "triclinic_pbc_ani2x")
# cases of tests/_aev_cases.py with rows of up to 256 entries at the pair cutoffs (the fourth 64-entry round of k_pair_hvp)
LONG_ROW_CASES = ("chunk256_open/seven", "chunk129_pbc/built")


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


def _model(kind, seed, dev, batch=True, trainable=False):
    from torchani_amd.models import ANI2dr, ANI2xr, ANIr2s
    from torchani_amd.weights import random_state_dict

    factory = {"ani2xr": ANI2xr, "anir2s": ANIr2s, "ani2dr": ANI2dr}[kind]
    model = factory(state_dict=random_state_dict(kind, 8, seed), device=dev, periodic_table_index=False,
                    neighborlist="batch" if batch else "auto", row_capacity=256)
    if trainable:
        model.neural_networks.requires_grad_(True)
    return model


def _x2r_case(kind, base, dev, trainable=False):
    h = _npz(f"hess_x2r_{kind}_{base}")
    sp = torch.from_numpy(h["species"]).to(dev)
    x = torch.from_numpy(h["coords"]).to(dev)
    cell = torch.from_numpy(h["cell"]).to(dev) if "cell" in h else None
    pbc = torch.from_numpy(h["pbc"]).to(dev) if "pbc" in h else None
    model = _model(kind, int(h["seed"]), dev, batch=cell is None or sp.shape[0] > 1, trainable=trainable)
    assert [str(s) for s in h["symbols"]] == list(model.symbols)
    return h, model, sp, x, cell, pbc


def _atomic_numbers(pot, sp):
    z = pot.atomic_numbers.to(sp.device)[sp.clamp(min=0)]
    return torch.where(sp >= 0, z, torch.full_like(z, -1))


def _autograd_rows(energy_fn, x, rows):
    """Rows of H through grad.forces_and_hessians (every row) or one autograd product per row."""
    from torchani_amd import grad

    xs = x.detach().clone().requires_grad_(True)
    e = energy_fn(xs)
    if len(rows) == 3 * x.shape[1]:
        return grad.forces_and_hessians(e, xs).hessians
    f = grad.forces(e, xs, retain_graph=True, create_graph=True).reshape(x.shape[0], -1)
    out = []
    for j in rows:
        (gj,) = torch.autograd.grad(f[:, j].sum(), xs, retain_graph=True)
        out.append(-gj.reshape(x.shape[0], 1, -1))
    return torch.cat(out, dim=1)


def _check_structure(H, sp, bound):
    C, n, _ = H.shape
    A = n // 3
    assert (H - H.transpose(1, 2)).abs().max().item() <= bound
    # translational sum rule: sum over the atoms l of H[(k, a), (l, b)] = 0
    assert H.reshape(C, n, A, 3).sum(dim=2).abs().max().item() <= bound * math.sqrt(A)
    pad = (sp < 0).repeat_interleave(3, dim=1)
    if pad.any():
        assert torch.all(H.transpose(1, 2)[pad] == 0) and torch.all(H[pad] == 0)


@pytest.mark.parametrize("kind,base", MODEL_CASES)
def test_model_hessians_match_reference(dev, kind, base):
    from torchani_amd import grad

    h, model, sp, x, cell, pbc = _x2r_case(kind, base, dev)
    rows, ref, ref_pair = h["hess_rows"], h["hess"].astype(np.float64), h["hess_pair"].astype(np.float64)
    bound = GATE * np.abs(ref).max()
    efh = grad.energies_forces_and_hessians(model, sp, x, cell=cell, pbc=pbc)
    ef = grad.energies_and_forces(model, sp, x, cell, pbc, keep_vars=False)
    assert torch.allclose(efh.energies, ef.energies, rtol=1e-12, atol=1e-9)
    assert torch.allclose(efh.forces, ef.forces, rtol=0, atol=1e-6)
    Hb = efh.hessians
    assert Hb.shape == (x.shape[0], 3 * x.shape[1], 3 * x.shape[1]) and Hb.dtype == x.dtype
    err_b = np.abs(Hb[:, rows].double().cpu().numpy() - ref).max()
    Ha = _autograd_rows(lambda xs: model((sp, xs), cell, pbc).energies, x, rows)
    err_a = np.abs(Ha.double().cpu().numpy() - ref).max()
    # the pair term alone, through the model's own potential used standalone (attributes a failure)
    pot = model.potentials["repulsion_xtb"]
    Hp = grad.energies_forces_and_hessians(pot, _atomic_numbers(pot, sp), x, cell=cell, pbc=pbc).hessians
    err_p = np.abs(Hp[:, rows].double().cpu().numpy() - ref_pair).max()
    report(f"pair hessian {kind} {base}: max|H_batched - H_ref| = {err_b:.2e}, max|H_autograd - H_ref| = {err_a:.2e}, "
           f"max|H_pair - H_pair_ref| = {err_p:.2e}, max|H_ref| = {np.abs(ref).max():.2e} (gate {bound:.2e})")
    assert err_p <= GATE * np.abs(ref_pair).max()
    assert err_b <= bound and err_a <= bound
    _check_structure(Hb.double(), sp, bound)


def _pairs2_consts():
    """The element constants of gen_golden_pairs2.py (its imports need the reference), as test_gpu_parity reads them."""
    src = open(os.path.join(GOLDEN, "gen_golden_pairs2.py")).read().split("def cases(symbols):")[0].split("CHARGES = ")[1]
    ns: dict = {}
    exec("CHARGES = " + src, ns)
    return ns


def _standalone_pots(symbols, periodic):
    from torchani_amd import potentials as P

    ns = _pairs2_consts()
    q = tuple(ns["CHARGES"][s] for s in symbols)
    pots = {"xtb_cos": P.RepulsionXTB(symbols, cutoff=5.2, cutoff_fn="cosine"),
            "xtb_smooth": P.RepulsionXTB(symbols, cutoff=5.2, cutoff_fn="smooth")}
    if not periodic:
        pots["xtb_inf"] = P.RepulsionXTB(symbols, cutoff=math.inf, cutoff_fn="smooth")
        pots["xtb_inf_cos"] = P.RepulsionXTB(symbols, cutoff=math.inf, cutoff_fn="cosine")
    pots.update({
        "zbl": P.RepulsionZBL(symbols, cutoff=5.2, cutoff_fn="smooth"),
        "zbl_cos": P.RepulsionZBL(symbols, k=0.4685, cutoff=4.0, cutoff_fn="cosine"),
        "lj": P.LennardJones(symbols, eps=tuple(ns["EPS"][s] for s in symbols), sigma=tuple(ns["SIGMA"][s] for s in symbols),
                             cutoff=7.5, cutoff_fn="smooth"),
        "lj_rep": P.RepulsionLJ(symbols, cutoff=5.2, cutoff_fn="smooth"),
        "lj_disp": P.DispersionLJ(symbols, cutoff=7.5, cutoff_fn="smooth"),
        "coulomb": P.FixedCoulomb(symbols, charges=q, dielectric=1.3, cutoff=7.5, cutoff_fn="smooth"),
        "mnok": P.FixedMNOK(symbols, charges=q, eta=tuple(ns["ETA"][s] for s in symbols), cutoff=7.5, cutoff_fn="smooth"),
    })
    return pots


@pytest.mark.parametrize("base", STANDALONE_BASES)
def test_standalone_hessians_match_reference(dev, base):
    from torchani_amd import grad

    g = load_golden(base)
    h = _npz("hess_pairs_" + base)
    rows = h["hess_rows"]
    sp = torch.from_numpy(g["species"].astype(np.int64)).to(dev)
    x = torch.from_numpy(g["coords"]).to(dev).double()
    cell = None if g["cell"] is None else torch.from_numpy(g["cell"]).to(dev)
    pbc = None if g["pbc"] is None else torch.from_numpy(np.asarray(g["pbc"])).to(dev)
    pots = _standalone_pots(g["symbols"], cell is not None)
    assert sorted(pots) == sorted(k[:-len("_hess")] for k in h if k.endswith("_hess"))
    for key, pot in pots.items():
        pot = pot.to(dev)
        z = _atomic_numbers(pot, sp)
        ref = h[key + "_hess"].astype(np.float64)
        bound = GATE * np.abs(ref).max()
        Hb = grad.energies_forces_and_hessians(pot, z, x, cell=cell, pbc=pbc).hessians
        err_b = np.abs(Hb[:, rows].double().cpu().numpy() - ref).max()
        Ha = _autograd_rows(lambda xs: pot(z, xs, cell, pbc), x, rows)
        err_a = np.abs(Ha.double().cpu().numpy() - ref).max()
        report(f"pair hessian standalone {base} {key}: max|H_batched - H_ref| = {err_b:.2e}, "
               f"max|H_autograd - H_ref| = {err_a:.2e}, max|H_ref| = {np.abs(ref).max():.2e}")
        assert err_b <= bound and err_a <= bound, key
        _check_structure(Hb.double(), sp, bound)


@pytest.mark.parametrize("case", LONG_ROW_CASES)
def test_standalone_hessians_on_long_rows(dev, case):
    """Every standalone potential on rows of up to 256 entries against the reference's fp64 Hessian rows
    (tests/golden/hess_pairs_<case>.npz) within 2e-5 max |H_ref|.  Row 3 i + c of H is the walk of central atom i, so the
    stored rows start with the three of the centre, the only atom of the shell cases whose row passes 192 entries at 5.2 A
    (at 7.5 A and without a cutoff every atom of chunk256_open/seven has one): k_pair_hvp's fourth 64-entry round in dense
    form, for every potential.  The item form runs through the block-sparse Hessian of a model carrying the potential, on
    the AEV's rows; only zbl_cos (4.0 A) fits inside the AEV cutoff, so there the fourth round walks entries past the
    potential's own cutoff.  First-order values: tests/test_gpu_parity.py."""
    import _aev_cases as ac
    from torchani_amd import grad
    from torchani_amd.models import ANI2x
    from torchani_amd.weights import arch_spec

    c = ac.case_by_name(case)
    h = _npz("hess_pairs_" + case.replace("/", "_"))
    assert np.array_equal(h["coords"], c.coords) and np.array_equal(h["species"], c.species)
    rows = h["hess_rows"]
    assert c.centre == 0 and rows[:3].tolist() == [0, 1, 2]
    symbols = list(arch_spec("ani2x")[0])
    sp = torch.from_numpy(c.species.astype(np.int64)).to(dev)
    x = torch.from_numpy(c.coords).to(dev).double()
    cell = None if c.cell is None else torch.from_numpy(c.cell).to(dev)
    pbc = None if c.pbc is None else torch.from_numpy(np.asarray(c.pbc)).to(dev)
    pots = _standalone_pots(symbols, cell is not None)
    assert sorted(pots) == sorted(k[:-len("_hess")] for k in h if k.endswith("_hess"))
    model = ANI2x(seed=3, device=dev, periodic_table_index=False, neighborlist="cell" if c.periodic else "batch",
                  row_capacity=256)
    model.set_enabled("nnp", False)
    sparse_keys = []
    for key, pot in pots.items():
        pot = pot.to(dev)
        z = _atomic_numbers(pot, sp)
        ref = h[key + "_hess"].astype(np.float64)
        bound = GATE * np.abs(ref).max()
        Hb = grad.energies_forces_and_hessians(pot, z, x, cell=cell, pbc=pbc).hessians
        d = np.abs(Hb[:, rows].double().cpu().numpy() - ref)
        err_b, err_c = d.max(), d[:, :3].max()
        line = (f"pair long rows {case} {key}: max|H_batched - H_ref| = {err_b:.2e} (the centre's rows {err_c:.2e}; max|H_ref| "
                f"= {np.abs(ref).max():.2e}, on the centre's rows {np.abs(ref[:, :3]).max():.2e})")
        err_s = None
        if pot.cutoff <= model.aev_computer.radial.cutoff + 1e-6:
            model.add_pair_potential("long_rows_" + key, pot)
            Hs = grad.energies_forces_and_sparse_hessians(model, sp, x, cell=cell, pbc=pbc).hessians.to_dense()
            model.set_enabled("long_rows_" + key, False)
            err_s = np.abs(Hs[:, rows].double().cpu().numpy() - ref).max()
            line += f", max|H_sparse - H_ref| = {err_s:.2e}"
            _check_structure(Hs.double(), sp, bound)
            sparse_keys.append(key)
        report(line)
        assert err_b <= bound and (err_s is None or err_s <= bound), key
        # the centre's rows at their own scale (they are small beside the shell atoms'): the same relative gate
        assert err_c <= GATE * np.abs(ref[:, :3]).max(), key
        _check_structure(Hb.double(), sp, bound)
    assert sparse_keys == ["zbl_cos"]


def _fd_columns(force_fn, x, cols, h=3e-4):
    """-(F(x + h e_j) - F(x - h e_j)) / 2h for the flat coordinate columns j: columns of H by central differences."""
    C = x.shape[0]
    out = []
    for j in cols:
        dx = torch.zeros_like(x).reshape(C, -1)
        dx[:, j] = h
        fp, fm = force_fn(x + dx.view_as(x)).double(), force_fn(x - dx.view_as(x)).double()
        out.append(-(fp - fm).reshape(C, -1) / (2 * h))
    return torch.stack(out, dim=2)


def test_atom_sees_its_own_image(dev):
    """A 3 A cubic cell with a 5.2 A cutoff: every atom has periodic images of itself in its row.  Such a pair does not
    depend on the coordinates: the Hessian of one atom alone is zero (its energy is not), and with two atoms the batched H
    equals autograd and central differences of the pair forces.  (Fixed charges: the xTB repulsion of an image 3 A away
    is ~1e-12 Ha, too small to show that the image is in the row.)"""
    from torchani_amd import grad
    from torchani_amd import potentials as P

    pot = P.FixedCoulomb(["H", "O"], charges=(0.4, -0.4), cutoff=5.2, cutoff_fn="smooth").to(dev)
    cell = torch.eye(3, dtype=torch.float64, device=dev) * 3.0
    pbc = torch.tensor([True, True, True], device=dev)
    z1 = torch.tensor([[8]], device=dev)
    x1 = torch.tensor([[[0.3, 0.2, 0.1]]], dtype=torch.float64, device=dev)
    e1 = grad.energies_forces_and_hessians(pot, z1, x1, cell=cell, pbc=pbc)
    assert e1.energies.abs().item() > 1e-6               # (the self-image pairs are in the rows)
    assert e1.hessians.abs().max().item() == 0.0
    z = torch.tensor([[8, 1]], device=dev)
    x = torch.tensor([[[0.3, 0.2, 0.1], [1.1, 0.6, 0.4]]], dtype=torch.float64, device=dev)
    Hb = grad.energies_forces_and_hessians(pot, z, x, cell=cell, pbc=pbc).hessians.double()
    Ha = _autograd_rows(lambda xs: pot(z, xs, cell, pbc), x, np.arange(6)).double()
    fd = _fd_columns(lambda xx: grad.energies_and_forces(pot, z, xx, cell, pbc).forces, x, range(6))
    scale = Hb.abs().max().item()
    d_ab, d_fd = (Ha - Hb).abs().max().item(), (fd - Hb).abs().max().item()
    report(f"pair hessian self-image cell: max|H_batched - H_autograd| = {d_ab:.2e}, "
           f"max|H - central differences| = {d_fd:.2e}, max|H| = {scale:.2e}")
    assert d_ab <= GATE * scale and d_fd <= 1e-3 * scale
    _check_structure(Hb, z, GATE * scale)


@pytest.mark.parametrize("base", ["rand_batch_ani2x", "water_pbc_ani2x"])
def test_hvp_through_autograd(dev, base):
    """autograd((F w).sum(), x) of ANI-2xr = -H w of the batched path; and, reference-free, the pair term's HVP through
    autograd = central differences of the pair forces along w."""
    from torchani_amd import grad

    h, model, sp, x, cell, pbc = _x2r_case("ani2xr", base, dev)
    w = torch.from_numpy(np.random.RandomState(3).standard_normal(x.shape)).to(dev).to(x.dtype)
    w = w * (sp >= 0).unsqueeze(-1).to(w.dtype)
    Hb = grad.energies_forces_and_hessians(model, sp, x, cell=cell, pbc=pbc).hessians.double()
    xs = x.detach().clone().requires_grad_(True)
    f = grad.forces(model((sp, xs), cell, pbc).energies, xs, retain_graph=True, create_graph=True)
    (hv,) = torch.autograd.grad((f * w).sum(), xs)
    want = -(Hb @ w.double().reshape(x.shape[0], -1, 1)).reshape(x.shape)
    err = (hv.double() - want).abs().max().item()
    bound = GATE * Hb.abs().max().item() * math.sqrt(w.numel())
    # the pair term alone: HVP through autograd against central differences of its forces, h = 3e-4 A
    pot = model.potentials["repulsion_xtb"]
    z = _atomic_numbers(pot, sp)
    xs = x.detach().clone().requires_grad_(True)
    fp = grad.forces(pot(z, xs, cell, pbc), xs, retain_graph=True, create_graph=True)
    (hv_p,) = torch.autograd.grad((fp * w).sum(), xs)
    step = 3e-4
    f_plus = grad.energies_and_forces(pot, z, x + step * w, cell, pbc).forces.double()
    f_minus = grad.energies_and_forces(pot, z, x - step * w, cell, pbc).forces.double()
    fd = (f_plus - f_minus) / (2 * step)   # = -H w
    err_fd = (hv_p.double() - fd).abs().max().item()
    scale_fd = fd.abs().max().item()
    report(f"pair hvp ani2xr {base}: max|autograd((F w).sum(), x) + H_batched w| = {err:.2e} (bound {bound:.2e}); "
           f"pair term: max|HVP - central differences| = {err_fd:.2e} (max {scale_fd:.2e})")
    assert err <= bound
    assert err_fd <= 1e-3 * scale_fd


def test_vibrational_analysis_ani2xr(dev):
    from torchani_amd import grad, units

    h = _npz("hess_x2r_vib_ani2xr")
    model = _model("ani2xr", int(h["seed"]), dev)
    sp = torch.from_numpy(h["species"]).to(dev)
    x = torch.from_numpy(h["coords"]).to(dev)
    H = grad.energies_forces_and_hessians(model, sp, x).hessians.double().cpu()
    err_h = np.abs(H.numpy() - h["hess"]).max()
    masses = torch.from_numpy(h["masses"])
    # eigenvalues of the mass-weighted Hessian move by at most ||M^-1/2 dH M^-1/2||_2 <= 3A GATE max|H_ref| / m_min
    bound = H.shape[1] * GATE * np.abs(h["hess"]).max() / h["masses"].min()
    lam = lambda f: np.sign(f) * (np.asarray(f) / units.SQRT_MHESSIAN_TO_INVCM * 2 * math.pi) ** 2   # noqa: E731
    # the perturbation of the mass-weighted Hessian, in the units of the eigenvalues
    w = np.repeat(h["masses"][0] ** -0.5, 3)
    d_mw = np.linalg.norm((H[0].numpy() - h["hess"][0]) * w[:, None] * w[None, :], 2)
    for mk in ("mdu", "mdn", "mwn"):
        va = grad.vibrational_analysis(masses, H, mode_kind=mk)
        ev, ref_ev = lam(va.freqs.numpy()), lam(h["freqs_" + mk])
        err = np.abs(ev - ref_ev).max()
        # modes, force constants and reduced masses where the eigenvalue is at least 100 perturbations away from its
        # neighbors (an eigenvector moves by about the perturbation over the gap)
        gap = np.abs(np.diff(ref_ev))
        checked, worst = 0, 0.0
        for k in range(ref_ev.size):
            g_k = min(gap[k - 1] if k > 0 else np.inf, gap[k] if k < gap.size else np.inf)
            if g_k < 100 * d_mw:
                continue
            m, r = va.modes[k].numpy(), h["modes_" + mk][k]
            s = np.sign((m * r).sum())
            worst = max(worst, np.abs(s * m - r).max() / np.abs(r).max())
            assert abs(va.rmasses[k].item() - h["rmasses_" + mk][k]) <= 1e-2 * h["rmasses_" + mk][k]
            assert abs(va.fconstants[k].item() - h["fconstants_" + mk][k]) <= 1e-2 * np.abs(h["fconstants_" + mk]).max()
            checked += 1
        report(f"vibrational analysis ani2xr ({mk}): max|H - H_ref| = {err_h:.2e}, max|d eigenvalue| = {err:.2e} "
               f"(bound {bound:.2e}), worst relative mode error {worst:.2e} over {checked} modes")
        assert err <= bound and worst <= 1e-2 and checked >= ref_ev.size // 2


def test_first_order_calls_launch_no_pair_hvp(dev, monkeypatch):
    from torchani_amd import grad
    from torchani_amd.potentials import _AnalyticPair

    calls = [0]
    orig = _AnalyticPair.hvp

    def counting(self, *a, **k):
        calls[0] += 1
        return orig(self, *a, **k)

    monkeypatch.setattr(_AnalyticPair, "hvp", counting)
    h, model, sp, x, cell, pbc = _x2r_case("ani2xr", "small_ani2x", dev)
    grad.energies_and_forces(model, sp, x, cell, pbc)
    xs = x.detach().clone().requires_grad_(True)
    model((sp, xs), cell, pbc).energies.sum().backward()
    h2, m2, sp2, x2, cell2, pbc2 = _x2r_case("ani2xr", "small_ani2x", dev, trainable=True)
    out = grad.energies_and_forces(m2, sp2, x2, cell2, pbc2, create_graph=True)
    (out.forces ** 2).sum().backward()
    assert calls[0] == 0
    # the batched path: one launch per chunk of directions
    grad.energies_forces_and_hessians(model, sp, x, cell=cell, pbc=pbc)
    packed = model.neural_networks._pack(dev)
    N = sp.numel()
    K = grad.hessian_chunk_size(sp.shape[0], sp.shape[1], model.aev_computer.out_dim,
                                -(-grad._hvp_row_bytes(packed, N) // N))
    assert calls[0] == -(-3 * sp.shape[1] // K)


def test_errors_that_remain(dev):
    from torchani_amd import grad

    g = load_golden("rand_batch_ani2x")
    m = _model("ani2dr", 5, dev)
    sp = torch.from_numpy(g["species"].astype(np.int64)).to(dev)
    x = torch.from_numpy(g["coords"]).to(dev)
    with pytest.raises(NotImplementedError, match="TwoBodyDispersionD3"):
        grad.energies_forces_and_hessians(m, sp, x)
    xs = x.detach().clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="TwoBodyDispersionD3"):
        grad.forces_and_hessians(m((sp, xs)).energies, xs)
    # asymmetric rows (ANIHIP_PAIR_PUSH) are refused by the kernel's entry point
    model = _model("ani2xr", 21, dev)
    pot = model.potentials["repulsion_xtb"]
    sp32 = sp.to(torch.int32).contiguous()
    rows = model._pair_rows(pot, sp32, x, None, None)
    t = torch.zeros((1, sp32.numel(), 3), dtype=torch.float32, device=dev)
    out = torch.zeros_like(t)
    with pytest.raises(RuntimeError, match="PUSH"):
        pot.hvp(sp32, rows._replace(symmetric=False), t, out)
    pot.hvp(sp32, rows, t, out)
    torch.cuda.synchronize()
    assert out.abs().max().item() == 0.0
