"""The network kernels on depths, widths and ensemble sizes off ANI's (tests/_mlp_shapes.py has the shape table and says what
each shape reaches; tests/test_network_shapes_host.py checks the references and the packer on the CPU): PackedNetworks called
directly, every entry point against an fp64 reference on the same fp32-rounded AEV rows -- the oracle for CELU networks, the
torch-fp64 autograd reference for GELU networks and Hessian-vector products.

Every case first asserts the route it means to exercise, from what the library itself says: the difference of
anihip_mlp_forward_backward_workspace_bytes between want_grad 0 and 1 (layer by layer: every hidden layer's activations in
both; fused: nothing, plus the d E / d act0 hand-over with a gradient; fused with the layer-0 backward inside: nothing in
both), fast_training() for the training passes, and the refusals of the forced flags.

Gates, all taken from the tests of the ANI shapes:
  per-atom energies 3e-7 Ha, member energies 1.5e-6 Ha, d E / d AEV 1e-6 + 1e-5 max |ref|    test_gpu_parity.test_mlp_ensemble
  weight gradients, exact passes: WG_REL_TOL = 2e-5 of the largest reference entry, here per (member, species, layer) block
      so that a small layer cannot hide behind layer 0                                         test_gpu_training
  weight gradients, fast pass: per block TAU = 2e-5 of the block's bound B = sum |g| |D|^T |X| test_gpu_training_scale.gate
  tangent gradients 5e-5 of the largest entry, S to 1e-5 max(1, |S|)        test_tangent_weight_grads_match_oracle
  Hessian-vector products: HVP_GATE = test_gpu_hessians.GATE = 2e-5 of the largest reference entry -- the gate that file
      holds a whole Hessian column to, of which the network part (J^T H_aev J) is one term
Padding atoms and atoms outside a central range must come out exactly zero; so must the padded rows and columns of the
gradient arrays (include/anihip.h), which _unpack_grads slices away before anyone could see them.
Atoms that tests/_util.py:celu_kink_atoms flags (a hidden pre-activation within 1e-6 of its scale of zero: CELU's second
derivative jumps there) get a zero tangent in the second-order comparisons, at most 5 % of a case's atoms (host test).
"""
import os

import numpy as np
import pytest
import torch

from _mlp_shapes import (CASE_IDS, ROTATIONS, SHAPES, VARIANTS, expected_route, fb_route, fused_shape, l0b_shape, make_case,
                         parameter_lists, stage_stress, torch_reference)
from _pack_reference import pack_reference
from _util import block_error_ratios, celu_kink_atoms, grad_blocks, mlp_magnitude_pass
from test_gpu_hessians import GATE as HVP_GATE
from test_gpu_parity import E_ATOM_TOL, F_TOL, report
from test_gpu_training import WG_REL_TOL, flat_from_lists
from test_gpu_training_scale import TAU
from torchani_amd import _lib
from torchani_amd.engine import PackedNetworks

pytestmark = pytest.mark.gpu

E_TOL, M_TOL = 3e-7, 1.5e-6      # test_mlp_ensemble
G_ABS, G_REL = 1e-6, 1e-5        # the same test
TANGENT_REL, TANGENT_S = 5e-5, 1e-5   # test_tangent_weight_grads_match_oracle


def cases_of(*names):
    return [f"{name}-r{r}" for name in names for r in ROTATIONS[name]]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def packs(dev):
    """pack(case_id, precision, activation="celu", bias=True): one PackedNetworks per combination, shared by the module's tests"""
    made = {}

    def pack(case_id, precision, activation="celu", bias=True):
        key = (case_id, precision, activation, bias)
        if key not in made:
            c = make_case(case_id)
            W, B = c.weights(dev, bias=bias)
            made[key] = PackedNetworks(W, B, c.K0, 0.1, dev, precision=precision, activation=activation)
        return made[key]

    yield pack
    made.clear()


@pytest.fixture(scope="module")
def inputs(dev):
    """(species int32 [n], aev float32 [n][K0]) of a case on the device"""
    made = {}

    def get(case_id):
        if case_id not in made:
            c = make_case(case_id)
            made[case_id] = (torch.from_numpy(c.species).to(dev), torch.from_numpy(c.aev).to(dev).contiguous())
        return made[case_id]

    yield get
    made.clear()


@pytest.fixture(scope="module")
def oracle_fb(oracle64):
    """(atomic energies, d E / d AEV, member energies) of a case from the oracle, computed once"""
    made = {}

    def get(case_id):
        if case_id not in made:
            c = make_case(case_id)
            made[case_id] = oracle64.mlp(c.species, c.aev.astype(np.float64), c.dims, c.flat, n_members=c.M, want_members=True)
        return made[case_id]

    return get


@pytest.fixture(scope="module")
def oracle_wg(oracle64):
    """(weight gradients, bound B of the magnitude pass) of a case for its upstream g_atom, computed once"""
    made = {}

    def get(case_id):
        if case_id not in made:
            c = make_case(case_id)
            a64, g64 = c.aev.astype(np.float64), c.g_atom.astype(np.float64)
            ref = oracle64.mlp_weight_grads(c.species, a64, g64, c.dims, c.flat, n_members=c.M)
            _, bound = mlp_magnitude_pass(c.species, a64, g64, c.dims, c.flat, c.M)
            made[case_id] = (ref, bound)
        return made[case_id]

    return get


def fb_params():
    out = []
    for cid in CASE_IDS:
        name = cid.rsplit("-r", 1)[0]
        for v in VARIANTS:
            if v == "f16x3-unfused" and not fused_shape(name):
                continue   # (the default route is the layer-by-layer one already)
            if v == "f16x3-l0b" and not l0b_shape(name):
                continue   # (refused: test_forced_layer0_backward_is_refused_where_it_cannot_run)
            out.append((cid, v))
    return out


def check_fb(tag, c, e, g, me, ref, lo=0, hi=None, rows0=0):
    """gates of test_mlp_ensemble on the atoms lo..hi; g holds the rows from rows0 on; exact zeros elsewhere"""
    ae, ga, mem = ref
    n = c.species.size
    hi = n if hi is None else hi
    inside = np.zeros(n, dtype=bool)
    inside[lo:hi] = True
    real = inside & (c.species >= 0)
    e = e.cpu().numpy()
    e_err = np.abs(e - ae)[real].max()
    line = f"netshape {tag:44s} |e_atom err| = {e_err:.2e} (gate {E_TOL:.0e})"
    assert not e[~real].any(), "padding atoms / atoms outside the range must have zero energy"
    if g is not None:
        g = g.cpu().numpy()
        rows = np.arange(rows0, rows0 + g.shape[0])
        keep = real[rows]
        gmax = np.abs(ga[real]).max()
        g_err = np.abs(g - ga[rows])[keep].max()
        line += f"  |d e/d aev err| = {g_err:.2e} (max {gmax:.2e}, gate {G_ABS + G_REL * gmax:.2e})"
        assert not g[~keep].any(), "rows of padding atoms / atoms outside the range must be zero"
        assert gmax > 1e-4
    if me is not None:
        me = me.cpu().numpy()
        m_err = np.abs(me - mem)[:, real].max()
        line += f"  members {m_err:.2e} (gate {M_TOL:.1e})"
        assert not me[:, ~real].any()
    report(line)
    assert e_err < E_TOL
    if g is not None:
        assert g_err < G_ABS + G_REL * gmax
    if me is not None:
        assert m_err < M_TOL


def central_range(c):
    """lo .. hi strictly inside the atoms, neither end a multiple of 64, and the many-atom species with a number of atoms in
    it that is no multiple of the 64-row tile"""
    n = c.species.size
    lo, hi = 37, n - 29
    while (c.species[lo:hi] == c.many).sum() % 64 == 0 or hi % 64 == 0:
        hi -= 1
    assert 0 < lo < hi < n and lo % 64 and hi % 64
    return lo, hi


@pytest.mark.parametrize("case_id,variant", fb_params())
def test_forward_backward(dev, packs, inputs, oracle_fb, case_id, variant):
    """Per-atom energies, member energies and d E / d AEV of every shape on every route it can take; the same without a
    gradient, on a central range inside the atoms, and with the buffers holding the rows of the range only."""
    c = make_case(case_id)
    precision, flags = VARIANTS[variant]
    packed = packs(case_id, precision)
    sp, aev = inputs(case_id)
    n = c.species.size
    assert fb_route(packed, n, flags) == expected_route(c.name, variant)
    ref = oracle_fb(case_id)
    packed.flags = flags
    try:
        e, g, me = packed.forward_backward(sp, aev, want_members=True)
        check_fb(f"fb {case_id} {variant}", c, e, g, me, ref)
        e0, g0, _ = packed.forward_backward(sp, aev, want_grad=False)
        assert g0 is None
        check_fb(f"fb {case_id} {variant} no-grad", c, e0, None, None, ref)
        lo, hi = central_range(c)
        e1, g1, me1 = packed.forward_backward(sp, aev, lo=lo, hi=hi, want_members=True)
        check_fb(f"fb {case_id} {variant} range {lo}..{hi}", c, e1, g1, me1, ref, lo, hi)
        e2, g2, _ = packed.forward_backward(sp, aev[lo:hi].contiguous(), lo=lo, hi=hi, shard_rows=True)
        assert g2.shape[0] == hi - lo
        check_fb(f"fb {case_id} {variant} shard rows", c, e2, g2, None, ref, lo, hi, rows0=lo)
        torch.cuda.synchronize()
    finally:
        packed.flags = None


@pytest.mark.parametrize("variant", ["f16x3", "f16x3-bigtile", "fp32"])
@pytest.mark.parametrize("case_id", ["one_hidden-r0", "two_hidden-r0", "wide-r0"])
def test_operand_scales_follow_their_stage(dev, inputs, oracle64, case_id, variant):
    """One, two and three hidden layers through the layer-by-layer kernels with stages of very different size
    (tests/_mlp_shapes.py: stage_stress): activations in the hundreds, back-propagated values of 1e-5 and less.  The amax slots
    are numbered from the number of hidden layers (forward l, output layer 3, backward 3 + (nh - 1 - l)); with every stage of
    about the same size, as in the other cases, a GEMM that reads a neighbouring or an empty slot still gets a usable scale."""
    c = make_case(case_id)
    precision, flags = VARIANTS[variant]
    flat = stage_stress(c.dims, c.flat, c.M)
    W, B = parameter_lists(c.dims, flat, c.M, dev)
    packed = PackedNetworks(W, B, c.K0, 0.1, dev, precision=precision)
    sp, aev = inputs(case_id)
    assert fb_route(packed, c.species.size, flags) == "layers"
    ref = oracle64.mlp(c.species, c.aev.astype(np.float64), c.dims, flat, n_members=c.M, want_members=True)
    assert 1e-4 < np.abs(ref[0]).max() < 1.0 and np.abs(ref[1]).max() > 3e-4   # (a wrong scale costs two digits: > 1e-6)
    packed.flags = flags
    try:
        e, g, me = packed.forward_backward(sp, aev, want_members=True)
    finally:
        packed.flags = None
    check_fb(f"stage stress {case_id} {variant}", c, e, g, me, ref)


@pytest.mark.parametrize("name", [name for name in SHAPES if len(SHAPES[name][1][0]) == 3 and not l0b_shape(name)])
def test_forced_layer0_backward_is_refused_where_it_cannot_run(dev, packs, inputs, name):
    """MLP_FLAG_FUSED_L0B on packs the phase cannot serve -- a first hidden layer of 32 columns (its k range has no first
    half), a pack that is not fused at all -- is refused with the library's message, not answered."""
    case_id = f"{name}-r0"
    packed = packs(case_id, "f16x3")
    sp, aev = inputs(case_id)
    assert fb_route(packed, sp.numel(), _lib.MLP_FLAG_FUSED_L0B) == ("fused" if fused_shape(name) else "layers")
    packed.flags = _lib.MLP_FLAG_FUSED_L0B
    try:
        with pytest.raises(RuntimeError, match="ANIHIP_MLP_FLAG_FUSED_L0B needs the fused kernel"):
            packed.forward_backward(sp, aev)
    finally:
        packed.flags = None


# ---- training pass -----------------------------------------------------------------------------------------------------------
def layer_blocks(dims, M):
    """[((member, species, layer), weight slice, bias slice)] of the oracle's packed layout"""
    b = grad_blocks(dims, M)
    return [(b[i][0][:3], b[i][1], b[i + 1][1]) for i in range(0, len(b), 2)]


def exact_gate(tag, got, ref, dims, M):
    """WG_REL_TOL of the largest reference entry of every (member, species, layer) block; a block without a gradient (a
    species without atoms) must be exactly zero.  Returns the worst ratio."""
    assert got.shape == ref.shape and np.isfinite(got).all(), tag
    worst, where = 0.0, None
    for key, w, b in layer_blocks(dims, M):
        scale = max(np.abs(ref[w]).max(), np.abs(ref[b]).max())
        err = max(np.abs(got[w] - ref[w]).max(), np.abs(got[b] - ref[b]).max())
        if scale == 0.0:
            assert err == 0.0, f"{tag}: block {key} must be zero"
            continue
        if err / scale > worst:
            worst, where = err / scale, key
    assert worst < WG_REL_TOL, f"{tag}: block {where} error {worst:.3e} of its largest entry (gate {WG_REL_TOL:.0e})"
    return worst, where


def fast_gate(tag, got, ref, bound, dims, M):
    """test_gpu_training_scale.gate for a pack of M members: per block TAU of the block's bound, and the global gate"""
    assert got.shape == ref.shape and np.isfinite(got).all(), tag
    r = block_error_ratios(got, ref, bound, grad_blocks(dims, M))
    worst = max(r, key=r.get)
    assert r[worst] <= TAU, f"{tag}: block {worst} error {r[worst]:.3e} x its bound (gate {TAU:.1e})"
    assert np.abs(got - ref).max() <= WG_REL_TOL * np.abs(ref).max()
    return r[worst], worst


class GradSpy:
    """Looks at the gradient arrays of a training call BEFORE _unpack_grads slices the padding away: the padded rows and
    columns must be zero (include/anihip.h: anihip_mlp_weight_grads)."""

    def __init__(self, packed):
        self.packed, self.orig, self.seen = packed, packed._unpack_grads, 0

    def __enter__(self):
        def spy(total, sizes, offs):
            p, q = self.packed, 0
            for s in range(p.S):
                dims = [p.desc.net[s].dims[l] for l in range(p.nl + 1)]
                for l in range(p.nl):
                    out, inn = p.shapes[s][l]
                    w = total[int(offs[q]): int(offs[q]) + sizes[q]].view(p.M, dims[l + 1], dims[l]).clone()
                    b = total[int(offs[q + 1]): int(offs[q + 1]) + sizes[q + 1]].view(p.M, dims[l + 1]).clone()
                    q += 2
                    assert bool(torch.isfinite(w).all()) and bool(torch.isfinite(b).all())
                    w[:, :out, :inn] = 0.0
                    b[:, :out] = 0.0
                    assert not bool(w.any()), f"species {s} layer {l}: a padded weight-gradient entry is not zero"
                    assert not bool(b.any()), f"species {s} layer {l}: a padded bias-gradient entry is not zero"
                    self.seen += 1
            return self.orig(total, sizes, offs)

        self.packed._unpack_grads = spy
        return self

    def __exit__(self, *exc):
        del self.packed._unpack_grads
        return False


@pytest.mark.parametrize("want_grad_aev", [False, True], ids=["weights", "weights+daev"])
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("case_id", CASE_IDS)
def test_weight_grads(dev, packs, inputs, oracle_fb, oracle_wg, case_id, precision, want_grad_aev):
    """anihip_mlp_weight_grads on every shape: the fast pass (fused TRAIN kernel + split weight-gradient kernels) where the
    pack has it and no d Loss / d AEV is wanted, the exact-fp32 pass everywhere else; energies and d Loss / d AEV at the gates
    of forward_backward; once in chunks of 77 atoms, once as train_forward + weight_grads(workspace=...)."""
    c = make_case(case_id)
    packed = packs(case_id, precision)
    sp, aev = inputs(case_id)
    n = c.species.size
    want_fast = precision == "f16x3" and fused_shape(c.name)
    assert packed.fast_training() == want_fast
    # (the library decides from the same plan as forward_backward: csrc/mlp.hip, train_fused)
    assert (fb_route(packed, 1 << 16) != "layers") == want_fast
    fast = want_fast and not want_grad_aev
    ref, bound = oracle_wg(case_id)
    ae, ga, _ = oracle_fb(case_id)
    up = torch.from_numpy(c.g_atom).to(dev)

    def check(tag, out):
        gw, gb, e, gaev = out
        got = flat_from_lists(gw, gb, packed.M, packed.S, packed.nl)
        worst, where = fast_gate(tag, got, ref, bound, c.dims, c.M) if fast else exact_gate(tag, got, ref, c.dims, c.M)
        line = (f"netshape {tag:44s} {'fast ' if fast else 'exact'} worst block {worst:.2e} at {where} "
                f"(gate {TAU if fast else WG_REL_TOL:.0e} of its {'bound' if fast else 'largest entry'})")
        real = c.species >= 0
        e = e.cpu().numpy()
        e_err = np.abs(e - ae)[real].max()
        assert not e[~real].any()
        line += f"  |e_atom err| = {e_err:.2e}"
        if gaev is not None:
            ga_ref = ga * c.g_atom.astype(np.float64)[:, None]
            gaev = gaev.cpu().numpy()
            ga_err, gmax = np.abs(gaev - ga_ref).max(), np.abs(ga_ref).max()
            line += f"  |dL/daev err| = {ga_err:.2e} (max {gmax:.2e})"
            assert not gaev[~real].any()
            assert ga_err < G_ABS + G_REL * gmax
        report(line)
        assert e_err < E_TOL

    with GradSpy(packed) as spy:
        check(f"wgrad {case_id} {precision} daev={int(want_grad_aev)}", packed.weight_grads(sp, aev, up, want_grad_aev=want_grad_aev))
        assert spy.seen == packed.S * packed.nl
        if not want_grad_aev:
            check(f"wgrad {case_id} {precision} chunk 77", packed.weight_grads(sp, aev, up, chunk=77))
            e_fwd, ws = packed.train_forward(sp, aev)
            out = packed.weight_grads(sp, aev, up, workspace=ws)
            check(f"wgrad {case_id} {precision} two halves", (out[0], out[1], e_fwd, None))
    torch.cuda.synchronize()


def kink_free_tangent(c, tangent):
    kinks = celu_kink_atoms(c.species, c.aev.astype(np.float64), c.dims, c.flat, c.M)
    t = np.array(tangent, dtype=np.float32, copy=True)
    t[..., kinks, :] = 0.0
    t[..., c.species < 0, :] = 0.0
    return t, int(kinks.sum())


def check_tangent(tag, packed, out, val_ref, ref, per_atom=None):
    gw, gb, de = out
    got = flat_from_lists(gw, gb, packed.M, packed.S, packed.nl)
    assert got.shape == ref.shape and np.isfinite(got).all()
    scale, err = np.abs(ref).max(), np.abs(got - ref).max()
    s_err = abs(de.double().sum().item() - val_ref)
    report(f"netshape {tag:44s} max|dS/dw err| = {err:.2e} (max {scale:.2e}, gate {TANGENT_REL * scale:.2e})  "
           f"|S err| = {s_err:.2e} (S = {val_ref:+.5f})")
    assert scale > 1e-4
    assert err < TANGENT_REL * scale
    assert s_err < TANGENT_S * max(1.0, abs(val_ref))
    if per_atom is not None:
        assert np.abs(de.cpu().numpy() - per_atom).max() < TANGENT_S * max(1.0, np.abs(per_atom).max())


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("case_id", cases_of("one_hidden", "two_hidden", "wide", "fused_edges"))
def test_tangent_weight_grads(dev, packs, inputs, oracle64, case_id, precision):
    """The second-order pass of force training (exact fp32 from the fp32 arrays of either pack) against the oracle."""
    c = make_case(case_id)
    packed = packs(case_id, precision)
    sp, aev = inputs(case_id)
    t, n_kinks = kink_free_tangent(c, c.tangent)
    assert n_kinks <= 0.05 * c.species.size
    val_ref, ref = oracle64.mlp_tangent_weight_grads(c.species, c.aev.astype(np.float64), t.astype(np.float64), c.dims, c.flat,
                                                    n_members=c.M)
    with GradSpy(packed) as spy:
        out = packed.tangent_weight_grads(sp, aev, torch.from_numpy(t).to(dev))
        assert spy.seen == packed.S * packed.nl
    torch.cuda.synchronize()
    check_tangent(f"tangent {case_id} {precision} ({n_kinks} kink atoms)", packed, out, val_ref, ref)


# ---- Hessian-vector products ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", cases_of("one_hidden", "two_hidden", "fused_edges", "many_members"))
def test_input_and_rows_hvp(dev, packs, inputs, case_id):
    """input_hvp with two tangents per atom and rows_hvp over a row set that repeats atoms and leaves a species out, against
    the double backward of the torch-fp64 reference.  Gate: HVP_GATE of the largest reference entry."""
    c = make_case(case_id)
    packed = packs(case_id, "f16x3")
    sp, aev = inputs(case_id)
    ref_net = torch_reference(case_id)
    n = c.species.size
    rs = np.random.RandomState(17)
    t, n_kinks = kink_free_tangent(c, np.stack([c.tangent, rs.uniform(-0.5, 0.5, c.tangent.shape)]))
    a64 = c.aev.astype(np.float64)
    ref = ref_net.input_hvp(c.species, a64, t)
    got = packed.input_hvp(sp, aev, torch.from_numpy(t).to(dev)).cpu().numpy()
    scale, err = np.abs(ref).max(), np.abs(got - ref).max()
    report(f"netshape {'input_hvp ' + case_id:44s} max|H t err| = {err:.2e} (max {scale:.2e}, gate {HVP_GATE * scale:.2e}; "
           f"{n_kinks} kink atoms)")
    assert scale > 1e-4 and np.isfinite(got).all()
    assert err <= HVP_GATE * scale
    assert not got[:, c.species < 0].any()
    # explicit rows: 150 draws with repeats from the many-atom species, the one-atom species three times where a third
    # species is there to be left out (it has no atoms); packs of two species leave the one-atom species out
    kinks = celu_kink_atoms(c.species, a64, c.dims, c.flat, c.M)
    pool = np.flatnonzero((c.species == c.many) & ~kinks)
    row_atom = rs.choice(pool, 150, replace=True)
    assert np.unique(row_atom).size < row_atom.size
    if c.S >= 3:
        assert not kinks[c.species == c.single].any()
        row_atom = np.concatenate([row_atom, np.repeat(np.flatnonzero(c.species == c.single), 3)])
    row_atom = row_atom[np.argsort(c.species[row_atom], kind="stable")].astype(np.int32)   # species ascending
    assert set(c.species[row_atom]) < set(range(c.S)) or c.S == 1
    tr = rs.uniform(-0.5, 0.5, (row_atom.size, c.K0)).astype(np.float32)
    ref_r = ref_net.input_hvp(c.species[row_atom], a64[row_atom], tr[None])[0]
    ws = packed.rows_hvp_prepare(sp, aev, row_atom.size + 11)
    got_r = packed.rows_hvp(sp, ws, torch.from_numpy(row_atom).to(dev), torch.from_numpy(tr).to(dev)).cpu().numpy()
    scale_r, err_r = np.abs(ref_r).max(), np.abs(got_r - ref_r).max()
    report(f"netshape {'rows_hvp ' + case_id:44s} max|H t err| = {err_r:.2e} (max {scale_r:.2e}, gate {HVP_GATE * scale_r:.2e}; "
           f"{row_atom.size} rows over {np.unique(row_atom).size} atoms)")
    assert scale_r > 1e-4 and np.isfinite(got_r).all()
    assert err_r <= HVP_GATE * scale_r


# ---- device refresh --------------------------------------------------------------------------------------------------------------
def flat_of(W, B):
    out = []
    for m in range(len(W)):
        for s in range(len(W[0])):
            for l in range(len(W[0][0])):
                out += [W[m][s][l].detach().cpu().numpy().astype(np.float64).reshape(-1),
                        B[m][s][l].detach().cpu().numpy().astype(np.float64).reshape(-1)]
    return np.concatenate(out)


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("case_id", ["one_hidden-r0", "fused_edges-r0", "wide-r0"])
def test_refresh(dev, oracle64, inputs, case_id, precision):
    """anihip_mlp_repack after every parameter changed: the fp32 arrays (w, wt, bias; all an fp32 pack has) equal the
    restatement of the layouts for the new values bit for bit, padding included -- so they equal a fresh pack and their
    padding is zero --; the split planes equal a fresh pack's wherever
    test_device_repack_of_a_split_fp16_pack_equals_the_host_packer demands it (layers that keep their scale), the operand
    bounds are upper bounds a hair above the host's; forward_backward then matches the oracle on the new weights."""
    c = make_case(case_id)
    W, B = c.weights(dev)
    packed = PackedNetworks(W, B, c.K0, 0.1, dev, precision=precision)
    gen = torch.Generator().manual_seed(23)
    with torch.no_grad():
        for m in range(c.M):
            for s in range(c.S):
                for l in range(c.nl):
                    for q in (W[m][s][l], B[m][s][l]):
                        q.mul_(1.0 + 0.02 * (torch.rand(q.shape, generator=gen) - 0.5).to(dev))
    packed.refresh(W, B)
    torch.cuda.synchronize()
    assert not packed.scale_overflowed()
    Wc = [[[w.cpu() for w in sl] for sl in ml] for ml in W]
    Bc = [[[b.cpu() for b in sl] for sl in ml] for ml in B]
    want, _, _ = pack_reference(Wc, Bc, c.K0, precision)
    fresh = PackedNetworks(W, B, c.K0, 0.1, dev, precision=precision)
    compared = kept = 0
    for (s, name, l), t in want.items():
        a, b = packed.desc.net[s], fresh.desc.net[s]
        if name in ("w", "wt", "bias"):
            got = packed.array(getattr(a, name)[l], t.shape).cpu()
            assert torch.equal(got, t), (s, name, l)
            assert torch.equal(got, fresh.array(getattr(b, name)[l], t.shape).cpu()), (s, name, l)
            compared += 1
        elif name == "bounds":
            bd_a, bd_b = packed.array(a.fused_bounds, t.shape), fresh.array(b.fused_bounds, t.shape)
            assert torch.all(bd_a >= bd_b) and torch.allclose(bd_a, bd_b, rtol=3e-4)
        elif a.wh_scale[l] == b.wh_scale[l]:
            pa, pb = getattr(a, name)[l], getattr(b, name)[l]
            assert pa and pb
            assert torch.equal(packed.array(pa, t.shape, torch.float16), fresh.array(pb, t.shape, torch.float16)), (s, name, l)
            kept += 1
    assert compared == c.S * (3 * c.nl - 1)
    if precision == "f16x3":
        assert kept >= c.S * (c.nl - 1)   # (half of the planes at least: a 1 % change moves few layers out of their binade)
    sp, aev = inputs(case_id)
    ref = oracle64.mlp(c.species, c.aev.astype(np.float64), c.dims, flat_of(W, B), n_members=c.M, want_members=True)
    e, g, me = packed.forward_backward(sp, aev, want_members=True)
    check_fb(f"refresh {case_id} {precision}", c, e, g, me, ref)


# ---- GELU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no-bias"])
@pytest.mark.parametrize("case_id", cases_of("fused_fit", "many_members"))
def test_gelu_forward_backward(dev, packs, inputs, case_id, bias):
    """GELU networks (exact, erf) through the fused kernel, with and without biases, against the torch-fp64 reference at the
    gates of the CELU networks."""
    c = make_case(case_id)
    packed = packs(case_id, "f16x3", "gelu", bias)
    sp, aev = inputs(case_id)
    assert fb_route(packed, c.species.size) == "fused"
    ae, me, ga = torch_reference(case_id, "gelu", bias).energies(c.species, c.aev.astype(np.float64))
    e, g, mem = packed.forward_backward(sp, aev, want_members=True)
    check_fb(f"gelu fb {case_id} {'bias' if bias else 'no-bias'}", c, e, g, mem, (ae, ga, me))


@pytest.mark.parametrize("case_id,precision", [("one_hidden-r0", "f16x3"), ("one_hidden-r0", "fp32"), ("fused_edges-r0", "f16x3"),
                                               ("fused_edges-r0", "fp32"), ("fused_fit-r0", "fp32")])
def test_gelu_forward_backward_is_refused_outside_the_fused_kernel(dev, packs, inputs, case_id, precision):
    """Energies of GELU networks come from the fused kernel only: a pack it does not cover -- one hidden layer, a
    (256, 256, 256) network (outside its LDS budget), fp32 -- is refused with the library's message, not answered."""
    packed = packs(case_id, precision, "gelu")
    sp, aev = inputs(case_id)
    assert fb_route(packed, sp.numel()) == "layers"
    with pytest.raises(RuntimeError, match="GELU networks run through the fused network kernel only"):
        packed.forward_backward(sp, aev)


@pytest.mark.parametrize("case_id", ["one_hidden-r0", "two_hidden-r0", "fused_edges-r0"])
def test_gelu_training_passes(dev, packs, inputs, case_id):
    """train_forward / weight_grads and tangent_weight_grads of an fp32 GELU pack (they keep the pre-activations) against the
    torch-fp64 reference, at the gates of the CELU networks.  GELU has no kink: no atom is left out."""
    c = make_case(case_id)
    packed = packs(case_id, "fp32", "gelu")
    sp, aev = inputs(case_id)
    ref_net = torch_reference(case_id, "gelu")
    a64 = c.aev.astype(np.float64)
    ae, _, ga = ref_net.energies(c.species, a64)
    ref = ref_net.weight_grads(c.species, a64, c.g_atom)
    up = torch.from_numpy(c.g_atom).to(dev)
    real = c.species >= 0
    with GradSpy(packed):
        e_fwd, ws = packed.train_forward(sp, aev)
        gw, gb, _, _ = packed.weight_grads(sp, aev, up, workspace=ws)
        gw2, gb2, e2, gaev = packed.weight_grads(sp, aev, up, want_grad_aev=True)
        t = np.where(real[:, None], c.tangent, 0.0).astype(np.float32)
        out = packed.tangent_weight_grads(sp, aev, torch.from_numpy(t).to(dev))
    torch.cuda.synchronize()
    for tag, a, b, e in (("two halves", gw, gb, e_fwd), ("one call + daev", gw2, gb2, e2)):
        worst, where = exact_gate(f"gelu wgrad {case_id} {tag}", flat_from_lists(a, b, c.M, c.S, c.nl), ref, c.dims, c.M)
        e_err = np.abs(e.cpu().numpy() - ae)[real].max()
        report(f"netshape {'gelu wgrad ' + case_id + ' ' + tag:44s} exact worst block {worst:.2e} at {where} (gate {WG_REL_TOL:.0e})"
               f"  |e_atom err| = {e_err:.2e}")
        assert e_err < E_TOL
    ga_ref = ga * c.g_atom.astype(np.float64)[:, None]
    assert np.abs(gaev.cpu().numpy() - ga_ref).max() < G_ABS + G_REL * np.abs(ga_ref).max()
    val_ref, tref, per_atom = ref_net.tangent_weight_grads(c.species, a64, t)
    check_tangent(f"gelu tangent {case_id}", packed, out, val_ref, tref, per_atom)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_model_with_two_hidden_layers_end_to_end(dev):
    """A potential whose networks have two hidden layers of 40 and 24 units (padded to 64 and 32), three members, built with
    ANINetworks.build on an 8 / 4x4 grid, through grad.energies_and_forces against the oracle -- the way and at the tolerances
    of test_gpu_parity.test_model_on_a_general_grid."""
    from oracle import oracle as orc
    from oracle.oracle import Oracle
    from torchani_amd.aev import AEVComputer
    from torchani_amd.grad import energies_and_forces
    from torchani_amd.models import ANI
    from torchani_amd.nn import ANINetworks, Ensemble

    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid_r8_a4z4_batch.npz")) as z:
        g = {k: z[k] for k in z.files}
    symbols = ("H", "C", "N", "O")
    aevc = AEVComputer.from_constants(float(g["Rcr"]), float(g["Rca"]), float(g["EtaR"]), g["ShfR"].tolist(), float(g["EtaA"]),
                                      float(g["Zeta"]), g["ShfA"].tolist(), g["ShfZ"].tolist(), 4, row_capacity=256)
    torch.manual_seed(19)
    nets = Ensemble([ANINetworks.build(symbols, aevc.out_dim, {sym: (40, 24) for sym in symbols}) for _ in range(3)])
    sae = [-0.5, -37.8, -54.6, -75.0]
    model = ANI(symbols, aevc, nets, sae, periodic_table_index=False).to(dev)
    sp = torch.from_numpy(g["species"].astype(np.int64)).to(dev)
    x = torch.from_numpy(g["coords"]).to(dev)
    e, f = energies_and_forces(model, sp, x)
    out = model.energies_and_forces(sp, x)
    torch.cuda.synchronize()
    packed = nets._pack(dev)
    assert packed.nl == 3 and [packed.desc.net[0].dims[l] for l in range(4)] == [aevc.out_dim, 64, 32, 1]
    assert fb_route(packed, sp.numel()) == "layers"
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    dims, flat = orc.pack_networks(sd, symbols, 3)
    assert dims[0].tolist() == [aevc.out_dim, 40, 24, 1]
    p = orc.make_params(4, float(g["Rcr"]), float(g["Rca"]), float(g["EtaR"]), float(g["EtaA"]), float(g["Zeta"]),
                        g["ShfR"].tolist(), g["ShfA"].tolist(), g["ShfZ"].tolist(), "cosine")
    ref = Oracle("f64").energy_forces(p, g["species"], g["coords"], dims, flat, 3, sae=np.asarray(sae))
    ea_err = np.abs(out.atomic_energies.cpu().numpy() - ref["atomic_energies"]).max()
    f_err = np.abs(f.cpu().numpy() - ref["forces"]).max()
    e_err = np.abs(e.detach().cpu().numpy() - ref["energies"]).max()
    report(f"netshape {'end to end (40, 24) x 3':44s} |e_atom err| = {ea_err:.2e} (gate {E_ATOM_TOL:.0e})  |dF| = {f_err:.2e} "
           f"(gate {F_TOL:.0e})  |dE| = {e_err:.2e} ({str(e.dtype)[6:]} totals of up to {np.abs(ref['energies']).max():.0f} Ha)")
    assert ea_err < E_ATOM_TOL
    assert np.abs(out.forces.cpu().numpy() - ref["forces"]).max() < F_TOL and f_err < F_TOL
    assert np.abs(out.energies.cpu().numpy() - ref["energies"]).max() < 1e-5
    # (the autograd path returns the totals, several hundred Ha of self energies, in the dtype of the coordinates: rounding
    # them to fp32 alone moves them by up to 2^-24 |E|, 3e-5 Ha at 512 Ha)
    assert e_err < 1e-5 + (2.0 ** -24 * np.abs(ref["energies"]).max() if e.dtype == torch.float32 else 0.0)
