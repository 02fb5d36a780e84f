"""The fast training pass (anihip_mlp_train_forward + anihip_mlp_weight_grads of an F16X3 pack: the fused TRAIN kernel, then
per layer one bf16 / fp16 x 3 weight-gradient launch) at the scale of BASELINE config 5 -- thousands of atoms per species,
so several workgroups per species meet in dW through float atomics -- against the fp64 oracle.

Gate (per block = member x species x layer x weight | bias, tests/_util.py:grad_blocks): max |got - ref| <= TAU * max B over
the block, with B = sum_a |g_a| |D_a|^T |X_a| (biases: sum_a |g_a| |D_a|) from the fp64 magnitude pass of tests/_util.py --
the size of the terms a gradient entry sums, whatever cancels in it.  A block whose gradients are 1e-3 of the case's largest
is held to its own scale, not to the largest one.  The global gate of tests/test_gpu_training.py (WG_REL_TOL of the largest
gradient entry) holds as well.  Gates, ~20 x the worst ratio measured on the MI355X (every ratio goes to parity_report.txt):
TAU 2e-5 (worst 1.35e-6: a uniform upstream, whose output-layer bias gradients are fp32 sums of thousands of equal terms;
every other case <= 7.4e-7), TAU_TANGENT 6e-6 (worst 3.2e-7), JT_TOL 1.5e-5 (worst 6.3e-7)."""
import functools

import numpy as np
import pytest
import torch

from _util import (_stress_state, block_error_ratios, celu_kink_atoms, conformers, grad_blocks, mlp_magnitude_pass,
                   mlp_tangent_magnitude_pass, oracle_networks, oracle_params)
from test_gpu_parity import report
from test_gpu_training import WG_REL_TOL, flat_from_lists, flat_from_params, fresh_model

pytestmark = pytest.mark.gpu

TAU = 2e-5          # energy-loss weight gradients, per block against B
TAU_TANGENT = 6e-6  # force-loss (tangent) weight gradients, per block against their bound (tests/_util.py)
JT_TOL = 1.5e-5     # J t, per species of the central atom, against max(1, max |J t|)
SEED = 7
M = 8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from torchani_amd import _lib

    _lib.lib()
    return torch.device("cuda:0")


def _edge_batch():
    """One species with exactly ONE atom (C), one with 1537 = 3 x 512 + 1 = 2 x 768 + 1 atoms (H): one past a multiple of
    the weight-gradient kernels' atoms per workgroup of every layer (8400 atom slots: 768 for layer 0, 512 for layers 1 and
    2 -- the rows_per_chunk rule of anihip_mlp_weight_grads), S with 513; the rest N and O."""
    sp, x = conformers(700, 12, seed=13)
    real = np.flatnonzero(sp.reshape(-1) >= 0)
    rs = np.random.RandomState(14)
    counts = {1: 1, 0: 1537, 4: 513}
    rest = real.size - sum(counts.values())
    lab = np.concatenate([np.full(c, s) for s, c in counts.items()] + [np.full(rest // 2, 2), np.full(rest - rest // 2, 3)])
    flat_sp = sp.reshape(-1)
    flat_sp[real] = rs.permutation(lab)
    return sp, x


BATCHES = {
    "hcno8k": lambda: conformers(640, 24, seed=11),                    # 8.8 k atoms, H C N O
    "config5": lambda: conformers(2560, 24, seed=5),                   # tools/train_bench.py's batch: 33.7 k atoms
    "all7": lambda: conformers(640, 24, seed=12, species=range(7), p=(0.4, 0.25, 0.1, 0.1, 0.05, 0.05, 0.05)),
    "edge": _edge_batch,
}


@functools.lru_cache(maxsize=None)
def batch(name, dev):
    sp, x = BATCHES[name]()
    model = fresh_model("ani2x", SEED, dev)
    spd, xd = torch.from_numpy(sp).to(dev), torch.from_numpy(x).to(dev)
    with torch.no_grad():
        aev = model.aev_computer(spd, xd).detach().contiguous()
    C, A = sp.shape
    at = aev.view(C * A, -1)
    return {"sp": sp, "x": x, "C": C, "A": A, "spd": spd, "sp32": spd.to(torch.int32).contiguous(), "aev": at,
            "aev64": at.cpu().numpy().astype(np.float64), "n_real": (sp >= 0).sum(axis=1)}


def networks():
    return oracle_networks("ani2x", M, SEED)[:2]


def reference(oracle64, b, up, dims=None, flat=None):
    """(oracle weight gradients, bound B) for the upstream ``up`` [C, A] (padding atoms: ignored by both)."""
    if dims is None:
        dims, flat = networks()
    up = np.asarray(up, dtype=np.float64).reshape(-1)
    ref = oracle64.mlp_weight_grads(b["sp"], b["aev64"], up, dims, flat, n_members=M)
    _, bound = mlp_magnitude_pass(b["sp"], b["aev64"], up, dims, flat, M)
    return ref, bound


def gate(tag, got, ref, bound, dims=None, tau=None):
    """The block gate and the global gate; returns the worst block ratio (reported)."""
    dims = networks()[0] if dims is None else dims
    tau = TAU if tau is None else tau
    assert np.isfinite(got).all(), f"{tag}: non-finite gradients"
    r = block_error_ratios(got, ref, bound, grad_blocks(dims, M))
    worst = max(r, key=r.get)
    per_layer = {l: max(v for k, v in r.items() if k[2] == l) for l in range(dims.shape[1] - 1)}
    err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    report(f"wgrad-scale {tag:34s} worst |err|/B = {r[worst]:.2e} at {worst}  by layer "
           + " ".join(f"{v:.1e}" for v in per_layer.values()) + f"  max|err| = {err:.2e} (max |ref| {scale:.2e})")
    assert r[worst] <= tau, f"{tag}: block {worst} error {r[worst]:.3e} x its bound (gate {tau:.1e})"
    assert err <= WG_REL_TOL * scale
    return r[worst]


def mol_upstream(b, seed, pad=None):
    """A per-molecule loss gradient: signed, constant over a molecule's atoms, ~ N(0, 1) / sqrt(n_atoms) / C (MSE / sqrt(n)
    of config 5); padding atoms get the molecule's value as autograd gives them (or ``pad``)."""
    rs = np.random.RandomState(seed)
    g = rs.normal(0.0, 1.0, b["C"]) / np.sqrt(b["n_real"]) / b["C"]
    up = np.repeat(g[:, None], b["A"], axis=1)
    if pad is not None:
        up[b["sp"] < 0] = pad
    return up


def fast_pack(nets, dev):
    nets.requires_grad_(True)
    assert nets._fast_trainable()
    packed = nets._train_pack(dev, fast=True)
    assert packed.precision == "f16x3" and packed.fast_training()
    return packed


def grads_two_halves(packed, b, up):
    upd = torch.from_numpy(np.ascontiguousarray(up, dtype=np.float32)).to(b["aev"].device)
    _, ws = packed.train_forward(b["sp32"], b["aev"])
    gw, gb, _, _ = packed.weight_grads(b["sp32"], b["aev"], upd, workspace=ws)
    torch.cuda.synchronize()
    return flat_from_lists(gw, gb, packed.M, packed.S, packed.nl)


# ---- a. scale and composition --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BATCHES))
def test_fast_training_pass_at_scale(dev, oracle64, name):
    """Every route of the fast pass on batches of 5 k .. 34 k atoms: the two halves (train_forward, weight_grads on its
    workspace), the one-call form (its own forward, whole system: compacted layer-0 slabs), the one-call form in chunks of
    3001 atoms (lo != 0: plain slabs, one bucketing per chunk, the chunks' gradients summed) and the flat-buffer target
    accumulated twice."""
    b = batch(name, dev)
    counts = [int((b["sp"] == s).sum()) for s in range(7)]
    report(f"wgrad-scale batch {name}: {int(b['n_real'].sum())} atoms in {b['C']} x {b['A']}, per species {counts}")
    if name == "edge":
        assert counts[1] == 1 and counts[0] == 1537 and counts[4] == 513 and b["C"] * b["A"] == 8400
    up = mol_upstream(b, 1)
    ref, bound = reference(oracle64, b, up)
    nets = fresh_model("ani2x", SEED, dev).neural_networks
    packed = fast_pack(nets, dev)
    gate(f"{name} halves", grads_two_halves(packed, b, up), ref, bound)
    upd = torch.from_numpy(up.astype(np.float32)).to(dev)
    gw, gb, _, _ = packed.weight_grads(b["sp32"], b["aev"], upd)
    gate(f"{name} one call", flat_from_lists(gw, gb, M, packed.S, packed.nl), ref, bound)
    gw, gb, _, _ = packed.weight_grads(b["sp32"], b["aev"], upd, chunk=3001)
    gate(f"{name} chunks of 3001", flat_from_lists(gw, gb, M, packed.S, packed.nl), ref, bound)
    # flat buffer in torch's parameter order, accumulated by two training passes
    params = list(nets.parameters())
    offs = np.concatenate([[0], np.cumsum([q.numel() for q in params])])
    flat_g = torch.zeros(int(offs[-1]), dtype=torch.float32, device=dev)
    S, nl = packed.S, packed.nl
    base_ptr = flat_g.data_ptr()
    w_ptr = [[base_ptr + 4 * int(offs[(s * nl + l) * 2]) for l in range(nl)] for s in range(S)]
    b_ptr = [[base_ptr + 4 * int(offs[(s * nl + l) * 2 + 1]) for l in range(nl)] for s in range(S)]
    tgt = packed.flat_grad_target(w_ptr, b_ptr, int(offs[2 * S * nl]))
    for _ in range(2):
        _, ws = packed.train_forward(b["sp32"], b["aev"])
        packed.weight_grads(b["sp32"], b["aev"], upd, workspace=ws, target=tgt)
    torch.cuda.synchronize()
    fg = flat_g.cpu().numpy().astype(np.float64)
    gate(f"{name} flat target x 2", fg, 2.0 * ref, 2.0 * bound)
    if name == "hcno8k":   # the exact-fp32 layer-by-layer passes as a control
        p32 = nets._train_pack(dev)
        assert p32.precision == "fp32"
        gw, gb, _, _ = p32.weight_grads(b["sp32"], b["aev"], upd)
        gate(f"{name} fp32 passes", flat_from_lists(gw, gb, M, packed.S, packed.nl), ref, bound)


# ---- b. upstream distributions -------------------------------------------------------------------------------------------
def test_upstream_of_the_config5_loss(dev, oracle64):
    """d Loss / d atomic_e of MSE(E) / sqrt(n_atoms) (tools/train_bench.py) for the oracle's energies and a random target."""
    b = batch("hcno8k", dev)
    dims, flat = networks()
    ae, _, _ = oracle64.mlp(b["sp"], b["aev64"], dims, flat, n_members=M, want_grad=False)
    E = ae.reshape(b["C"], b["A"]).sum(axis=1)
    t = np.random.RandomState(1).normal(0, 0.1, b["C"])
    g = 2.0 * (E - t) / np.sqrt(b["n_real"]) / b["C"]
    up = np.repeat(g[:, None], b["A"], axis=1)
    assert (g > 0).any() and (g < 0).any()
    ref, bound = reference(oracle64, b, up)
    gate("hcno8k mse/sqrt(n) loss", grads_two_halves(fast_pack(fresh_model("ani2x", SEED, dev).neural_networks, dev), b, up),
         ref, bound)


def test_wide_and_outlier_upstreams(dev, oracle64):
    """Per-atom magnitudes log-uniform over 1e-6 .. 1e2 with random signs; one atom 1e4 x the rest."""
    b = batch("hcno8k", dev)
    packed = fast_pack(fresh_model("ani2x", SEED, dev).neural_networks, dev)
    rs = np.random.RandomState(2)
    shape = (b["C"], b["A"])
    wide = rs.choice([-1.0, 1.0], shape) * 10.0 ** rs.uniform(-6, 2, shape)
    ref, bound = reference(oracle64, b, wide)
    gate("hcno8k log-uniform 1e-6..1e2", grads_two_halves(packed, b, wide), ref, bound)
    outl = rs.choice([-1.0, 1.0], shape) * rs.uniform(0.5, 1.5, shape)
    real = np.argwhere(b["sp"] >= 0)
    c, a = real[len(real) // 3]
    outl[c, a] *= 1e4
    ref, bound = reference(oracle64, b, outl)
    gate("hcno8k one atom 1e4 x", grads_two_halves(packed, b, outl), ref, bound)


def test_overall_scale_of_the_upstream(dev, oracle64):
    """Upstream x 1e-8 and x 1e6: the gradients scale with it and the error stays the same fraction of B (the fp16 operand
    scale follows max |g|)."""
    b = batch("hcno8k", dev)
    packed = fast_pack(fresh_model("ani2x", SEED, dev).neural_networks, dev)
    up = mol_upstream(b, 3)
    ref, bound = reference(oracle64, b, up)
    r1 = gate("hcno8k upstream x 1", grads_two_halves(packed, b, up), ref, bound)
    for s in (1e-8, 1e6):
        r = gate(f"hcno8k upstream x {s:g}", grads_two_halves(packed, b, s * up), s * ref, s * bound)
        assert r <= 4.0 * r1 + 1e-9, f"x {s:g}: error / B {r:.2e} against {r1:.2e} at scale 1"


def test_zero_upstreams(dev, oracle64):
    """A species whose upstream is zero on every atom gets EXACTLY zero gradients (the others stay right); an all-zero
    upstream gives all-zero gradients, no NaN (the fp16 scale of max |g| = 0)."""
    b = batch("hcno8k", dev)
    packed = fast_pack(fresh_model("ani2x", SEED, dev).neural_networks, dev)
    dims, _ = networks()
    up = mol_upstream(b, 4)
    up[b["sp"] == 1] = 0.0
    ref, bound = reference(oracle64, b, up)
    got = grads_two_halves(packed, b, up)
    for (m, s, l, wb), sl in grad_blocks(dims, M):
        if s == 1:
            assert np.all(got[sl] == 0.0), (m, s, l, wb)
    gate("hcno8k species C upstream 0", got, ref, bound)
    got0 = grads_two_halves(packed, b, np.zeros((b["C"], b["A"])))
    assert np.all(got0 == 0.0), "all-zero upstream: gradients must be exactly 0"


def test_upstream_on_padding_atoms_is_ignored(dev, oracle64):
    """Large upstream values on padding atoms (species -1) change nothing beyond the gate: padding atoms have no network."""
    b = batch("hcno8k", dev)
    packed = fast_pack(fresh_model("ani2x", SEED, dev).neural_networks, dev)
    up = mol_upstream(b, 5, pad=0.0)
    ref, bound = reference(oracle64, b, up)
    r0 = gate("hcno8k padding upstream 0", grads_two_halves(packed, b, up), ref, bound)
    big = up.copy()
    pad = b["sp"] < 0
    big[pad] = 1e4 * np.abs(up).max() * np.where(np.arange(pad.sum()) % 2 == 0, 1.0, -1.0)
    r = gate("hcno8k padding upstream 1e4 x", grads_two_halves(packed, b, big), ref, bound)
    assert r <= 4.0 * r0 + 1e-9


# ---- c. repeated backward on one forward ---------------------------------------------------------------------------------
def test_repeated_backward_on_one_forward(dev, oracle64):
    """Two weight_grads calls on ONE train_forward workspace (loss.backward(retain_graph=True) twice): the second, with an
    upstream 1e6 x smaller, is as accurate as if it were the first -- its fp16 operand scale comes from its own max |g|, not
    from the running maximum of the call before."""
    b = batch("hcno8k", dev)
    packed = fast_pack(fresh_model("ani2x", SEED, dev).neural_networks, dev)
    up = mol_upstream(b, 6)
    ref, bound = reference(oracle64, b, up)
    _, ws = packed.train_forward(b["sp32"], b["aev"])
    out = []
    for s in (1e3, 1e-3):
        upd = torch.from_numpy((s * up).astype(np.float32)).to(dev)
        gw, gb, _, _ = packed.weight_grads(b["sp32"], b["aev"], upd, workspace=ws)
        torch.cuda.synchronize()
        out.append(flat_from_lists(gw, gb, M, packed.S, packed.nl))
    gate("hcno8k same forward, upstream x 1e3", out[0], 1e3 * ref, 1e3 * bound)
    gate("hcno8k same forward, then x 1e-3", out[1], 1e-3 * ref, 1e-3 * bound)


def test_repeated_autograd_backward(dev, oracle64):
    """The same through autograd: (1e3 e).sum().backward(retain_graph=True), zero the gradients, (1e-3 e).sum().backward()."""
    b = batch("hcno8k", dev)
    nets = fresh_model("ani2x", SEED, dev).neural_networks
    fast_pack(nets, dev)
    aev = b["aev"].view(b["C"], b["A"], -1)
    e = nets(b["spd"], aev)
    (1e3 * e).sum().backward(retain_graph=True)
    nets.zero_grad()
    (1e-3 * e).sum().backward()
    torch.cuda.synchronize()
    got = flat_from_params(nets, nets.symbols)
    ref, bound = reference(oracle64, b, np.ones((b["C"], b["A"])))
    gate("hcno8k autograd x 1e3 then x 1e-3", got, 1e-3 * ref, 1e-3 * bound)


# ---- d. weight-distribution stress ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["scale_small", "scale_large", "scale_mixed", "student_t", "outlier_row"])
def test_fast_training_pass_under_weight_distribution_stress(dev, oracle64, case):
    """tests/test_gpu_parity.py's parameter sets that stress the split-fp16 scales (bounds from weight norms), on the fast
    training pass, against the oracle on the same state dict."""
    from oracle import oracle as orc
    from torchani_amd.models import ANI2x
    from torchani_amd.weights import arch_spec

    b = batch("hcno8k", dev)
    sd = _stress_state(case)
    dims, flat = orc.pack_networks(sd, arch_spec("ani2x")[0], M)
    nets = ANI2x(state_dict=sd, device=dev, periodic_table_index=False).neural_networks
    packed = fast_pack(nets, dev)
    up = mol_upstream(b, 8)
    ref, bound = reference(oracle64, b, up, dims, flat)
    gate(f"hcno8k stress {case}", grads_two_halves(packed, b, up), ref, bound, dims)
    upd = torch.from_numpy(up.astype(np.float32)).to(dev)
    gw, gb, _, _ = packed.weight_grads(b["sp32"], b["aev"], upd)
    gate(f"hcno8k stress {case} one call", flat_from_lists(gw, gb, M, packed.S, packed.nl), ref, bound, dims)


# ---- e. force training at scale ------------------------------------------------------------------------------------------
def test_force_training_passes_at_scale(dev, oracle64):
    """anihip_aev_jvp (J t) and anihip_mlp_tangent_weight_grads (d/d params of sum_i v_i . d e_i / d aev_i, v = -J t) on
    4.4 k atoms, per block: J t by the species of the central atom, the parameter gradients by (member, species, layer)."""
    from _util import fgrad_direction

    sp, x = conformers(320, 24, seed=17)
    C, A = sp.shape
    dims, flat = networks()
    p = oracle_params("ani2x")
    t = fgrad_direction(sp)
    aev_ref, jt_ref = oracle64.aev_jvp(p, sp, x.astype(np.float64), t)
    val_ref, _ = oracle64.mlp_tangent_weight_grads(sp, aev_ref, -jt_ref, dims, flat, n_members=M)
    model = fresh_model("ani2x", SEED, dev)
    model.aev_computer.row_capacity = 256
    sp32 = torch.from_numpy(sp.astype(np.int32)).to(dev)
    aevc = model.aev_computer
    rows = aevc.neighbor_rows(sp32, torch.from_numpy(x).to(dev).contiguous())
    eng = aevc.engine()
    aev = eng.forward(sp32, rows)
    jt = eng.jvp(sp32, rows, torch.from_numpy(t.astype(np.float32)).to(dev))
    torch.cuda.synchronize()
    got_jt = jt.cpu().numpy().astype(np.float64)
    jr = jt_ref.reshape(C * A, -1)
    spf = sp.reshape(-1)
    worst = 0.0
    for s in range(4):
        rws = spf == s
        r = np.abs(got_jt[rws] - jr[rws]).max() / max(1.0, np.abs(jr[rws]).max())
        worst = max(worst, r)
        assert r < JT_TOL, (s, r)
    assert np.all(got_jt[spf < 0] == 0)
    packed = model.neural_networks._train_pack(dev)
    gw, gb, de = packed.tangent_weight_grads(sp32, aev, -jt)
    torch.cuda.synchronize()
    got = flat_from_lists(gw, gb, packed.M, packed.S, packed.nl)
    s_err = abs(de.double().sum().item() - val_ref)
    report(f"wgrad-scale force 4.4k: J t worst |err| / max(1, max|J t|) by species {worst:.2e}; |t.F err| = {s_err:.2e} "
           f"(t.F = {val_ref:+.4f})")
    # the network pass per block, the oracle and the bound on the SAME fp32 AEV and J t the kernel read.  An atom with a hidden
    # pre-activation within fp32 rounding of 0 (celu_kink_atoms: ~100 of these 4.2 k) puts the second-order terms on the
    # wrong side of CELU's jump in c'' = 1 / alpha -> 0 in any fp32 evaluation: with them, a plain numpy fp32 pass is off by
    # 5e-4 of the bound in layers 0-2, and so is the kernel (reported); without them (their tangent rows zeroed: they add
    # nothing to S) by 2e-7 -- that is where the gate holds the kernel.
    a64 = aev.cpu().numpy().astype(np.float64)
    kink = celu_kink_atoms(sp, a64, dims, flat, M)
    assert 0 < kink.sum() < 0.05 * (sp >= 0).sum()
    _, ref_all = oracle64.mlp_tangent_weight_grads(sp, a64, -got_jt, dims, flat, n_members=M)
    _, bound_all = mlp_tangent_magnitude_pass(sp, a64, -got_jt, dims, flat, M)
    r_all = block_error_ratios(got, ref_all, bound_all, grad_blocks(dims, M))
    report(f"wgrad-scale force 4.4k tangent, every atom (not gated): worst |err|/B = {max(r_all.values()):.2e}; "
           f"{int(kink.sum())} atoms near a CELU kink")
    v = (-jt) * torch.from_numpy(~kink).to(dev)[:, None]
    gw, gb, _ = packed.tangent_weight_grads(sp32, aev, v)
    torch.cuda.synchronize()
    got = flat_from_lists(gw, gb, packed.M, packed.S, packed.nl)
    v64 = v.cpu().numpy().astype(np.float64)
    _, ref32 = oracle64.mlp_tangent_weight_grads(sp, a64, v64, dims, flat, n_members=M)
    _, bound = mlp_tangent_magnitude_pass(sp, a64, v64, dims, flat, M)
    gate("force 4.4k tangent weight grads", got, ref32, bound, tau=TAU_TANGENT)
    assert s_err < 1e-5 * max(1.0, abs(val_ref))


# ---- f. graph-captured step ----------------------------------------------------------------------------------------------
def test_graph_captured_energy_training_step(dev, oracle64):
    """Forward + MSE(E) / sqrt(n) loss + backward of config 5's step, captured with torch.cuda.graph (tools/train_bench.py
    --graph, without the optimizer's step: the gradients land in torchani_amd.optim.Adam's flat buffer, zeroed inside the
    graph), replayed twice with the target rewritten in place in between: each replay's gradients follow ITS upstream (the
    replayed max |g| and fp16 scales track the new data)."""
    from torchani_amd.optim import Adam

    b = batch("hcno8k", dev)
    model = fresh_model("ani2x", SEED, dev)
    nets = model.neural_networks
    nets.requires_grad_(True)
    opt = Adam(nets.parameters(), lr=1e-4)
    fbuf = opt._flat[0]
    xd = torch.from_numpy(b["x"]).to(dev)
    spd = b["spd"]
    n_at = (spd >= 0).sum(dim=1).float()
    target = torch.zeros(b["C"], dtype=torch.float32, device=dev)
    rs = np.random.RandomState(9)
    targets = [rs.normal(0, 0.1, b["C"]), rs.normal(0, 0.1, b["C"]) - 5.0]

    def whole():
        fbuf.grad.zero_()
        aev = model.aev_computer(spd, xd)
        e = nets(spd, aev)
        loss = (torch.nn.functional.mse_loss(e, target, reduction="none") / n_at.sqrt()).mean()
        loss.backward()
        return aev, e

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            whole()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert nets._train_pack(dev, fast=True).flat_target is not None, "the gradients did not take the flat-buffer route"
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s_aev, s_e = whole()
    dims, flat = networks()
    for i, tg in enumerate(targets):
        target.copy_(torch.from_numpy(tg.astype(np.float32)))
        graph.replay()
        torch.cuda.synchronize()
        got = flat_from_params(nets, nets.symbols)
        E = s_e.detach().double().cpu().numpy()
        t32 = tg.astype(np.float32).astype(np.float64)
        g = 2.0 * (E - t32) / np.sqrt(b["n_real"]) / b["C"]
        a64 = s_aev.detach().cpu().numpy().astype(np.float64).reshape(b["C"] * b["A"], -1)
        ref = oracle64.mlp_weight_grads(b["sp"], a64, np.repeat(g[:, None], b["A"], axis=1), dims, flat, n_members=M)
        _, bound = mlp_magnitude_pass(b["sp"], a64, np.repeat(g[:, None], b["A"], axis=1), dims, flat, M)
        gate(f"hcno8k graph replay {i} (max |g| {np.abs(g).max():.1e})", got, ref, bound)
