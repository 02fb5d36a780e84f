"""Where the fused network kernel's operand scales and never-read registers can go wrong (csrc/mlp_fused.hip: the power-of-two
split scales s1 .. s4 folded into constants of the epilogues -- put_acc's pre-scaled form, celu_d2's scaled constants, the
backward seed, `osc * s` as one scalar --, their reciprocals by exponent arithmetic, and the registers that are defined without
an instruction on the paths that never read them: the derivative arrays of a row block a wave has no unit in, the AEV
registers of an item that fetches none, phase 5's `prev[]` on the register-sum path).

``PackedNetworks.forward_backward`` on seeded random ANI-2x weights and synthetic AEV rows with slab masks, against the package's
exact layer-by-layer path (an fp32 pack of the same weights), like test_gpu_fused_addressing.py and at its tolerances, which
are test_gpu_parity.test_mlp_ensemble's: per-atom energies 3e-7 Ha, d E / d AEV 1e-6 + 1e-5 of its largest entry.  Every case
is evaluated twice and must give the same bits.

Shapes.  1, 33, 64 and 65 atoms of a species -- a tile whose second row block has no valid row, a partial tile, a full one, two
tiles -- through each of the four compile-time-width networks (256/192/160, 224/192/160, 192/160/128, 160/128/96: between them
every wave is dealt a whole unit, one row block and no unit in some phase) and through the run-time-width kernel on all seven
species.

Scales.  The split scales follow the tile maximum of act0 (s0, s1) and the weight-norm bounds of the pack (s1 .. s4).  AEV rows
scaled by 2^-20, 1 and 2^13 with layer 0 scaled by 1, 1 and 2^7 move the tile maximum from its floor (alpha = 0.1: CELU is
bounded below) over 0.33 to about 3e5, more than twenty binades (test_act0_maximum_crosses_twenty_binades recomputes them); an
all-zero tile sits on the floor exactly.  The packs scale whole layers by
powers of two, so that the reference sees the same numbers; what a case scales up in one layer it scales down in the output
layer, because the energy gate is ABSOLUTE (3e-7 Ha) and means what it means in the parity test only for per-atom energies of
the order of one (the prints show them).  `large` / `small`: every hidden layer behind layer 0 and the output layer scaled by
2^2 / 2^-4 -- bounds[0 .. 4] grow by 2^2 .. 2^6 / shrink by 2^-4 .. 2^-12 -- with layer 0 scaled by 2^-6 in `large`, which
keeps its energies in range.

Register definitions: an atom without neighbors in a tile, a tile of such atoms only, 1 / 4 / 5 / 17 flagged slabs (kept operand,
its limit, staged operand, multi-pass phase 5 with prev[] live), want_grad off, one member and eight.

Other instantiations: the two-product backward at test_gpu_fused_addressing's bounds for it; GELU (the instantiation without
phase 5) and the training instantiation against the exact fp32 TRAINING passes of the same weights, the only exact path GELU
networks have: GELU at the tolerances above; the training forward through what reads its stored activations and per-layer
gradients -- the weight gradients (activations x gradients) and the bias gradients (column sums of the gradients) of every
layer -- at test_gpu_training's gate, 2e-5 of the largest gradient, and the energies at its 3e-7.
"""
import numpy as np
import pytest
import torch

from _util import seeded_state
from test_gpu_fused_addressing import BWD2_REL, BWD2_TOL, E_TOL, G_ABS, G_REL, make_case, run_fused
from torchani_amd import _lib

pytestmark = pytest.mark.gpu

WG_REL_TOL = 2e-5                # test_gpu_training: weight / bias gradients, relative to the largest entry
SEED = 31
H, C, N, O, S, F, CL = range(7)
# powers of two that multiply (layer 0, hidden layers 1 and 2, output layer) of every member and species, biases included
PACKS = {"plain": (0, 0, 0), "large": (-6, 2, 2), "small": (0, -4, -4), "act0-large": (7, 0, -20)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def packs(dev):
    """packs(name, M = 8, activation = 'celu') -> (split-fp16 pack: the fused kernel, fp32 pack: the exact layer-by-layer
    kernels) of the seeded weights with whole layers scaled as PACKS[name] says; built once each"""
    from torchani_amd.constants import CELU_ALPHA
    from torchani_amd.engine import PackedNetworks
    from torchani_amd.models import ANI2x

    model = ANI2x(state_dict=seeded_state("ani2x", 8, SEED), device=dev, periodic_table_index=False)
    plan = model.neural_networks._plan()
    made = {}

    def get(name, M=8, activation="celu"):
        key = (name, M, activation)
        if key not in made:
            k0, kh, k3 = PACKS[name]
            exps = (k0, kh, kh, k3)
            with torch.no_grad():
                W = [[[(w.detach() * 2.0 ** exps[l]).contiguous() for l, w in enumerate(ws)] for ws in wm] for wm in plan["weights"][:M]]
                B = [[[(b.detach() * 2.0 ** exps[l]).contiguous() for l, b in enumerate(bs)] for bs in bm] for bm in plan["biases"][:M]]
            fused = PackedNetworks(W, B, 1008, CELU_ALPHA, dev, "f16x3", activation=activation)
            exact = PackedNetworks(W, B, 1008, CELU_ALPHA, dev, "fp32", activation=activation)
            assert fused.M == M and fused.aev_len == 1008 and fused.radial_len == 112
            made[key] = (fused, exact)
        return made[key]

    return get


def reference(exact, sp, aev):
    e, g, _ = exact.forward_backward(sp, aev)
    torch.cuda.synchronize()
    return e, g


def check(tag, e, g, e_ref, g_ref, cols, g_abs=G_ABS, g_rel=G_REL):
    e_err = float((e - e_ref).abs().max())
    line = f"fused scales {tag}: max|e_atom| = {float(e_ref.abs().max()):.2e}  max|e_atom err| = {e_err:.2e}"
    if g is not None:
        gmax = float(g_ref[:, cols].abs().max())
        g_err = float((g[:, cols] - g_ref[:, cols]).abs().max())
        line += f"  max|d e/d aev err| = {g_err:.2e} (max {gmax:.2e}, gate {g_abs + g_rel * gmax:.2e})"
    print(line)
    assert bool(torch.isfinite(e).all())
    assert e_err < E_TOL
    if g is not None:
        assert bool(torch.isfinite(g).all())
        assert g_err < g_abs + g_rel * gmax
        other = torch.ones(g.shape[1], dtype=torch.bool, device=g.device)
        other[cols] = False
        assert not bool(g[:, other].any())   # nothing is written outside the flagged slabs


def fused_case(tag, pair, sp, aev, mask, cols, hint=0, **kw):
    fused, exact = pair
    e, g = run_fused(fused, sp, aev, mask, _lib.MLP_FLAG_FUSED_L0B, hint=hint)
    e_ref, g_ref = reference(exact, sp, aev)
    check(tag, e, g, e_ref, g_ref, cols, **kw)
    return e, g


# ---- every unit shape ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("species", [H, C, O, F], ids=["256-192-160", "224-192-160", "192-160-128", "160-128-96"])
def test_unit_shapes_compile_time_widths(dev, packs, species):
    for n in (1, 33, 64, 65):
        sp, aev, mask, cols = make_case(dev, [species] * n, 4, 200 + n)
        fused_case(f"species {species} n {n}", packs("plain"), sp, aev, mask, cols, hint=_lib.MLP_FLAG_SHAPED)


def test_unit_shapes_run_time_widths(dev, packs):
    """all seven species in one launch of the run-time-width kernel, 1, 33, 64 and 65 atoms of a species"""
    counts = {H: 65, C: 64, N: 33, O: 1, S: 33, F: 65, CL: 1}
    species = np.random.RandomState(2).permutation(np.repeat(list(counts), list(counts.values())))
    sp, aev, mask, cols = make_case(dev, species, 4, 210)
    fused_case("seven species, one launch", packs("plain"), sp, aev, mask, cols)


# ---- scales at their extremes ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shaped", [False, True], ids=["run-time", "compile-time"])
@pytest.mark.parametrize("pack,aev_exp", [("plain", -20), ("plain", 0), ("act0-large", 13), ("large", 0), ("large", -20),
                                          ("small", 0), ("small", 13)],
                         ids=["tiny-aev", "unit-aev", "act0-2^18", "large-bounds", "large-bounds-tiny-aev", "small-bounds",
                              "small-bounds-large-aev"])
def test_scales(dev, packs, pack, aev_exp, shaped):
    """130 hydrogen + 70 oxygen atoms, four flagged slabs; the AEV rows scaled by 2^aev_exp (the fp16 split of the layer-0
    operand takes 4 x AEV: 0.8 x 2^13 x 4 is inside fp16)"""
    sp, aev, mask, cols = make_case(dev, [H] * 130 + [O] * 70, 4, 220)
    aev = aev * 2.0 ** aev_exp
    fused_case(f"{pack} aev 2^{aev_exp} shaped={shaped}", packs(pack), sp, aev, mask, cols,
               hint=_lib.MLP_FLAG_SHAPED if shaped else 0)


def test_act0_maximum_crosses_twenty_binades(dev):
    """what test_scales' first three cases are for: the largest act0 of their hydrogen tiles, recomputed in fp64"""
    _, aev, _, _ = make_case(dev, [H] * 130 + [O] * 70, 4, 220)
    # act0 = celu(W0 aev + b0) with W0, b0 scaled by 2^k0 and aev by 2^aev_exp: from the seeded parameters in fp64
    from torchani_amd.models import ANI2x

    model = ANI2x(state_dict=seeded_state("ani2x", 8, SEED), device=dev, periodic_table_index=False)
    plan = model.neural_networks._plan()
    a64 = aev[:130].double()
    seen = []
    for pack, aev_exp in (("plain", -20), ("plain", 0), ("act0-large", 13)):
        k0 = PACKS[pack][0]
        top = 0.1   # (the kernel's floor: CELU >= -alpha)
        for m in range(8):
            W, b = plan["weights"][m][H][0].double(), plan["biases"][m][H][0].double()
            z = (a64 * 2.0 ** aev_exp) @ (W * 2.0 ** k0).T + b * 2.0 ** k0
            top = max(top, float(torch.nn.functional.celu(z, alpha=0.1).max()))
        seen.append(top)
    print("fused scales: largest act0 of the hydrogen tiles per case:", " ".join(f"{t:.3g}" for t in seen))
    assert seen[0] < 1.0 < seen[1] * 16 and seen[1] < 64.0
    assert np.log2(seen[2] / seen[0]) >= 20.0


@pytest.mark.parametrize("shaped", [False, True], ids=["run-time", "compile-time"])
def test_all_zero_tile(dev, packs, shaped):
    """65 hydrogen atoms with flagged slabs and all-zero rows: act0 = celu(b0), its tile maximum on the floor or a bias; the
    gradient is compared like everywhere (d E / d AEV of a zero row is not zero)"""
    sp, aev, mask, cols = make_case(dev, [H] * 65, 4, 230)
    aev = torch.zeros_like(aev)
    for pack in ("plain", "small"):
        fused_case(f"all-zero tile {pack} shaped={shaped}", packs(pack), sp, aev, mask, cols,
                   hint=_lib.MLP_FLAG_SHAPED if shaped else 0)


# ---- register definitions ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_slabs", [1, 4, 5, 17])
@pytest.mark.parametrize("shaped", [False, True], ids=["run-time", "compile-time"])
@pytest.mark.parametrize("M", [1, 8])
def test_flagged_slabs_and_members(dev, packs, n_slabs, shaped, M):
    """130 hydrogen + 70 oxygen atoms, one of them without neighbors: 1 / 4 flagged slabs keep the layer-0 operand (the items of
    members 1 .. 7 fetch no AEV rows: their registers are defined without an instruction) and sum the members in registers
    (prev[] never read), 5 stage it, 17 run five passes of phase 5 with prev[] live; one member: the first item of a tile is its
    last"""
    sp, aev, mask, cols = make_case(dev, [H] * 130 + [O] * 70, n_slabs, 240 + n_slabs, lonely=77)
    fused_case(f"{n_slabs} slabs M={M} shaped={shaped}", packs("plain", M), sp, aev, mask, cols,
               hint=_lib.MLP_FLAG_SHAPED if shaped else 0)


@pytest.mark.parametrize("shaped", [False, True], ids=["run-time", "compile-time"])
def test_tile_of_atoms_without_neighbors(dev, packs, shaped):
    """70 oxygen atoms none of which flags a slab (a tile with an empty mask: layer 0 multiplies nothing, phase 5 has no slab)
    beside 65 hydrogen atoms that do: energies as the reference's, no d E / d AEV written in the oxygen rows"""
    sp, aev, mask, cols = make_case(dev, [H] * 65 + [O] * 70, 4, 250)
    aev[65:] = 0.0
    mask[65:] = 0
    e, g = fused_case(f"empty-mask tile shaped={shaped}", packs("plain"), sp, aev, mask, cols,
                      hint=_lib.MLP_FLAG_SHAPED if shaped else 0, g_abs=float("inf"))
    e_ref, g_ref = reference(packs("plain")[1], sp, aev)
    check("empty-mask tile, hydrogen rows", e[:65], g[:65], e_ref[:65], g_ref[:65], cols)
    assert not bool(g[65:].any())


@pytest.mark.parametrize("shaped", [False, True], ids=["run-time", "compile-time"])
def test_without_gradient(dev, packs, shaped):
    """want_grad off (no phases 3 to 5: the seed is formed and not stored): energies at the gate, equal bit for bit to the
    energies of the call with the gradient"""
    fused, exact = packs("plain")
    sp, aev, mask, cols = make_case(dev, [H] * 130 + [O] * 70, 4, 260, lonely=5)
    hint = _lib.MLP_FLAG_SHAPED if shaped else 0
    e_g, _ = run_fused(fused, sp, aev, mask, _lib.MLP_FLAG_FUSED_L0B, hint=hint)
    got = []
    fused.flags = _lib.MLP_FLAG_FUSED_L0B
    try:
        for _ in range(2):
            e, g, _ = fused.forward_backward(sp, aev, want_grad=False, slab_mask=mask, tile_hint=hint)
            assert g is None
            got.append(e.clone())
    finally:
        fused.flags = None
    torch.cuda.synchronize()
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], e_g)
    e_ref, _ = reference(exact, sp, aev)
    check(f"no gradient shaped={shaped}", got[0], None, e_ref, None, cols)


# ---- other instantiations ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pack", ["plain", "small"])
def test_two_product_backward(dev, packs, pack):
    """MLP_FLAG_BWD_TWO_PRODUCTS (an instantiation of its own with the same folded epilogues), all seven species: energies equal
    to the three-product call's bit for bit, d E / d AEV inside test_gpu_fused_addressing's two bounds for it"""
    fused, exact = packs(pack)
    sp, aev, mask, cols = make_case(dev, [H, C, N, O, S, F, CL] * 19, 4, 270)
    e3, _ = run_fused(fused, sp, aev, mask, _lib.MLP_FLAG_FUSED_L0B)
    e2, g2 = run_fused(fused, sp, aev, mask, _lib.MLP_FLAG_FUSED_L0B, hint=_lib.MLP_FLAG_BWD_TWO_PRODUCTS)
    e_ref, g_ref = reference(exact, sp, aev)
    assert torch.equal(e2, e3)
    check(f"two-product backward {pack}", e2, g2, e_ref, g_ref, cols, g_abs=BWD2_TOL, g_rel=0.0)
    check(f"two-product backward {pack}, rounding bound", e2, g2, e_ref, g_ref, cols, g_abs=G_ABS, g_rel=BWD2_REL)


def exact_training_pass(exact, sp, aev, upstream):
    gw, gb, e, ga = exact.weight_grads(sp, aev, upstream, want_grad_aev=True)
    torch.cuda.synchronize()
    return gw, gb, e, ga


@pytest.mark.parametrize("pack", ["plain", "small"])
def test_gelu(dev, packs, pack):
    """the GELU instantiation (no phase 5: d act0 leaves for the layer-0 backward GEMM; the seed and phase 3 fold their scales,
    act1 does not) on all seven species with 1, 33, 64 and 65 atoms, against the exact fp32 training passes with a unit
    upstream gradient"""
    fused, exact = packs(pack, 8, "gelu")
    counts = {H: 65, C: 64, N: 33, O: 1, S: 33, F: 65, CL: 1}
    species = np.random.RandomState(3).permutation(np.repeat(list(counts), list(counts.values())))
    sp, aev, mask, cols = make_case(dev, species, 4, 280)
    e, g = run_fused(fused, sp, aev, mask, 0)
    _, _, e_ref, g_ref = exact_training_pass(exact, sp, aev, torch.ones(len(species), device=dev))
    check(f"gelu {pack}", e, g, e_ref, g_ref, cols)


def test_training_forward(dev, packs):
    """the TRAIN instantiation keeps the unfolded epilogues (it stores the unscaled activations and gradients from the
    accumulators) but takes its scales back by exponent arithmetic like the others: the training forward of the split-fp16 pack,
    twice -- per-atom energies equal bit for bit --, and the weight-gradient pass over what it stored, against the exact fp32
    training pass of the same weights.  The bias gradient of layer l is the column sum of the stored gradient dlt[l] alone, so it
    pins dlt[l] and its scale; the weight gradient of layer l + 1 is dlt[l + 1]^T act[l], so with dlt pinned it pins the stored
    activation act[l]: a scale that is wrong on one array and compensated on the other shows in the bias gradients.  (The
    weight-gradient kernels add with float atomics: their results are not held to bit equality between two evaluations.)"""
    fused, exact = packs("plain")
    assert fused.fast_training() and not exact.fast_training()
    counts = {H: 65, C: 64, N: 33, O: 1, S: 33, F: 65, CL: 1}
    species = np.random.RandomState(4).permutation(np.repeat(list(counts), list(counts.values())))
    sp, aev, _, _ = make_case(dev, species, 17, 290)
    up = torch.from_numpy(np.random.RandomState(6).uniform(-1.0, 1.0, len(species)).astype(np.float32)).to(dev)
    e_fwd, ws = fused.train_forward(sp, aev)
    e_again, ws_again = fused.train_forward(sp, aev)
    gw_ref, gb_ref, e_ref, _ = exact_training_pass(exact, sp, aev, up)
    torch.cuda.synchronize()
    assert torch.equal(e_fwd, e_again), "per-atom energies differ between two training forwards"
    assert float((e_fwd - e_ref).abs().max()) < E_TOL
    for tag, w in (("first", ws), ("second", ws_again)):   # (what each of the two forwards stored)
        gw, gb, _, _ = fused.weight_grads(sp, aev, up, workspace=w)   # (the energies are the forward half's)
        torch.cuda.synchronize()
        for name, got, ref in (("weights", gw, gw_ref), ("biases", gb, gb_ref)):
            for l in range(fused.nl):
                scale = max(float(ref[m][s][l].abs().max()) for m in range(8) for s in range(7))
                err = max(float((got[m][s][l] - ref[m][s][l]).abs().max()) for m in range(8) for s in range(7))
                print(f"fused scales training, {tag} forward: layer {l} {name}: max err {err:.2e} (max {scale:.2e}, "
                      f"gate {WG_REL_TOL * scale:.2e})")
                assert scale > 0.0 and err < WG_REL_TOL * scale
