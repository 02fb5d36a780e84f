"""CPU side of the network-shape tests (tests/_mlp_shapes.py; the GPU side is tests/test_gpu_network_shapes.py): the two fp64
references agree on every shape, every case has the composition its docstring promises and keeps the cap on excluded atoms,
the packer's layouts are right for every shape, and the host path refuses what it cannot serve.

Reference agreement.  The torch-fp64 MLP and the oracle (oracle/ani_oracle.c) are held to 1e-12 on energies and 1e-8 absolute
on every derivative -- two orders under the tightest GPU gate (1e-6 + 1e-5 max |ref| on d E / d AEV), so the choice of
reference cannot decide a GPU test.  Measured here: energies 1e-16, member energies 3e-16, d E / d AEV 3e-17, weight gradients
5e-15, tangent gradients 9e-16 (absolute, on entries of order 1): the two differ by the order of their fp64 sums.  With
torch.nn.functional.celu in the torch reference the derivatives differed by 3e-10 (d E / d AEV) to 1e-8 (tangent gradients):
its backward holds 1 / alpha in fp32 -- tests/_mlp_shapes.py writes CELU out for that reason.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from _mlp_shapes import (CASE_IDS, ROTATIONS, SHAPES, VARIANTS, expected_route, fb_route, fused_shape, l0b_shape, make_case, pad32,
                         torch_reference)
from _util import celu_kink_atoms, grad_blocks, mlp_magnitude_pass
from test_abi_and_host import _check_pack_against_reference

E_AGREE = 1e-12      # energies, absolute (Ha)
D_AGREE = 1e-8       # derivatives, absolute
KINK_CAP = 0.05      # share of a case's atoms that celu_kink_atoms may flag (they leave the second-order comparisons)


def report(line):
    print(line)


@pytest.mark.parametrize("case_id", CASE_IDS)
def test_the_two_references_agree(oracle64, case_id):
    c = make_case(case_id)
    ref = torch_reference(case_id)
    a64 = c.aev.astype(np.float64)
    ae, ga, me = oracle64.mlp(c.species, a64, c.dims, c.flat, n_members=c.M, want_members=True)
    ae_t, me_t, ga_t = ref.energies(c.species, a64)
    wg = oracle64.mlp_weight_grads(c.species, a64, c.g_atom.astype(np.float64), c.dims, c.flat, n_members=c.M)
    wg_t = ref.weight_grads(c.species, a64, c.g_atom)
    val, tg = oracle64.mlp_tangent_weight_grads(c.species, a64, c.tangent.astype(np.float64), c.dims, c.flat, n_members=c.M)
    val_t, tg_t, _ = ref.tangent_weight_grads(c.species, a64, c.tangent)
    signed, _ = mlp_magnitude_pass(c.species, a64, c.g_atom, c.dims, c.flat, c.M)
    errs = {"e": np.abs(ae - ae_t).max(), "members": np.abs(me - me_t).max(), "dE/dAEV": np.abs(ga - ga_t).max(),
            "wgrad": np.abs(wg - wg_t).max(), "tangent": np.abs(tg - tg_t).max(), "S": abs(val - val_t),
            "magnitude pass": np.abs(wg - signed).max()}
    report(f"references {case_id:18s} " + "  ".join(f"{k} {v:.1e}" for k, v in errs.items())
           + f"  (max |wgrad| {np.abs(wg).max():.1e}, |tangent| {np.abs(tg).max():.1e})")
    assert np.abs(ae).max() > 1e-3 and np.abs(ga).max() > 1e-4 and np.abs(wg).max() > 1e-3 and np.abs(tg).max() > 1e-4
    assert errs["e"] < E_AGREE and errs["members"] < E_AGREE
    for k in ("dE/dAEV", "wgrad", "tangent", "S", "magnitude pass"):
        assert errs[k] < D_AGREE, k
    # padding atoms: zero energy and zero rows in both
    pad = c.species < 0
    assert not ae[pad].any() and not ae_t[pad].any() and not ga[pad].any() and not ga_t[pad].any()


@pytest.mark.parametrize("case_id", CASE_IDS)
def test_case_composition(case_id):
    """200..300 atoms; padding atoms; one species with more than two 64-row tiles and a partly filled last one; one species with
    exactly one atom (packs of two species or more); one species without atoms (three or more); and the reference alone keeps
    the atoms next to a CELU kink under the cap."""
    c = make_case(case_id)
    n = c.species.size
    counts = np.bincount(c.species[c.species >= 0], minlength=c.S)
    assert 200 <= n <= 300 and c.aev.shape == (n, c.K0) and c.aev.dtype == np.float32 and c.aev.min() >= 0.0
    assert (c.species < 0).sum() == c.n_pad > 0
    assert counts[c.many] > 128 and counts[c.many] % 64 != 0
    if c.S >= 2:
        assert counts[c.single] == 1
    if c.S >= 3:
        assert counts[c.empty] == 0
    assert counts.sum() + c.n_pad == n
    kinks = celu_kink_atoms(c.species, c.aev.astype(np.float64), c.dims, c.flat, c.M)
    report(f"composition {case_id:18s} n {n}  padding {c.n_pad}  per species {counts.tolist()}  kink atoms {int(kinks.sum())}")
    assert kinks.sum() <= KINK_CAP * n
    assert not kinks[c.species < 0].any()
    # the same parameters on every call, in fp32
    assert make_case(case_id) is c and np.array_equal(c.flat, c.flat.astype(np.float32).astype(np.float64))
    assert len(grad_blocks(c.dims, c.M)) == 2 * c.M * c.S * c.nl


def test_the_shape_table_reaches_what_it_says():
    """The routes the table's comments name, from the shapes alone (the GPU tests ask the library)."""
    assert [name for name in SHAPES if fused_shape(name)] == ["fused_fit", "fused_l0b_fit", "many_members"]
    assert [name for name in SHAPES if l0b_shape(name)] == ["fused_l0b_fit"]
    assert set(ROTATIONS) == set(SHAPES) and all(max(r) < len(SHAPES[name][1]) for name, r in ROTATIONS.items())
    K0, hidden, _ = SHAPES["long_row"]
    assert pad32(K0) > 1024 and K0 % 16 == 0 and all(max(h) <= 256 for h in hidden)
    assert SHAPES["one_hidden"][0] % 32 != 0 and SHAPES["many_members"][2] == 64
    # (256, 256, 256): inside the width limit of the fused kernel, outside its LDS budget; (256, 192, 256): the largest inside
    assert 256 + 256 > 448 >= 192 + 256


@pytest.mark.parametrize("name", list(SHAPES))
def test_pack_layout_of_every_shape(name):
    """anihip_mlp_pack into a host buffer == the torch restatement of the layouts (tests/_pack_reference.py), bit for bit: fp32
    and split-fp16, and GELU where the shape runs fused (the operand bounds carry a factor for GELU's derivative)."""
    c = make_case(f"{name}-r0")
    W, B = c.weights()
    pk = _check_pack_against_reference(W, B, c.K0)
    d = pk.desc
    for s in range(c.S):
        assert [d.net[s].dims[l] for l in range(c.nl + 1)] == [c.K0] + [pad32(h) for h in c.hidden[s]] + [1]
        assert bool(d.net[s].fused_bounds) == (c.nl == 4)
    assert pk.radial_len == (48 if c.K0 == 240 else 0)   # (240 = 16 x 3 + 32 x 6: the ANI form for three species)
    assert pk.fast_training() == fused_shape(name)
    fp = _check_pack_against_reference(W, B, c.K0, precision="fp32")
    assert fp.radial_len == 0 and not fp.fast_training()
    if fused_shape(name):
        _check_pack_against_reference(W, B, c.K0, activation="gelu")


@functools.lru_cache(maxsize=None)
def host_pack(name, precision="f16x3", activation="celu"):
    """the shape's first case packed into host memory: the route questions below read the descriptor alone"""
    from torchani_amd.engine import PackedNetworks

    c = make_case(f"{name}-r0")
    W, B = c.weights()
    return PackedNetworks(W, B, c.K0, 0.1, torch.device("cpu"), precision=precision, activation=activation)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(SHAPES))
def test_route_of_every_shape_and_variant(name, variant):
    """The route the GPU tests assert before they run a case (tests/test_gpu_network_shapes.py), from the workspace query alone:
    it is host code (csrc/mlp.hip: fb_plan), so every shape x variant is checked here without a device."""
    precision, flags = VARIANTS[variant]
    n = make_case(f"{name}-r0").species.size
    assert fb_route(host_pack(name, precision), n, flags) == expected_route(name, variant)


L0B_MIN_ATOMS = 24000   # csrc/mlp_fused.h: FUSED_L0B_MIN_ATOMS


def test_layer0_backward_moves_inside_the_fused_kernel_at_its_threshold():
    """Default flags: below FUSED_L0B_MIN_ATOMS atoms d E / d act0 is handed to a layer-0 backward GEMM, from it on the backward
    runs inside the kernel -- unless a flag says no, or the networks are GELU (that instantiation has no phase 5)."""
    from torchani_amd import _lib

    names = [name for name in SHAPES if l0b_shape(name)]
    assert names
    for name in names:
        pk = host_pack(name)
        assert fb_route(pk, L0B_MIN_ATOMS - 1) == "fused"
        assert fb_route(pk, L0B_MIN_ATOMS) == "fused_l0b"
        assert fb_route(pk, L0B_MIN_ATOMS, _lib.MLP_FLAG_NO_FUSED_L0B) == "fused"
        assert fb_route(pk, L0B_MIN_ATOMS, _lib.MLP_FLAG_SMALL_TILES) == "fused"
        assert fb_route(host_pack(name, activation="gelu"), L0B_MIN_ATOMS) == "fused"


@pytest.mark.parametrize("name", list(SHAPES))
def test_fast_training_is_the_library_rule(name):
    """PackedNetworks.fast_training() is anihip_mlp_fast_training: true exactly where forward_backward of a split-fp16 CELU pack
    runs fused, false for fp32 and GELU packs; and the library looks at the planes, not only at the widths."""
    from torchani_amd import _lib

    pk = host_pack(name)
    assert pk.fast_training() == (fb_route(pk, 1 << 16) != "layers") == fused_shape(name)
    assert not host_pack(name, "fp32").fast_training()
    L = _lib.lib()
    assert L.anihip_mlp_fast_training(None) == 0
    if fused_shape(name):
        gelu = host_pack(name, activation="gelu")
        assert fb_route(gelu, 1 << 16) == "fused" and not gelu.fast_training()
        d = _lib.MlpDesc.from_buffer_copy(pk.desc)
        assert L.anihip_mlp_fast_training(ctypes.byref(d)) == 1
        d.net[pk.S - 1].whf[1] = None   # (a descriptor without one fragment-ordered plane: no fused kernel, whatever the widths)
        assert L.anihip_mlp_fast_training(ctypes.byref(d)) == 0


def test_refusals_on_the_host_path():
    """flat_grad_target needs unpadded widths; PackedNetworks takes 2..4 Linear layers."""
    from torchani_amd.engine import PackedNetworks

    cpu = torch.device("cpu")
    for name in ("one_hidden", "two_hidden", "fused_fit"):   # 33 -> 64, 100 -> 128, 40 -> 64
        c = make_case(f"{name}-r0")
        W, B = c.weights()
        pk = PackedNetworks(W, B, c.K0, 0.1, cpu)
        with pytest.raises(ValueError, match="multiples of 32"):
            pk.flat_grad_target([[0] * c.nl] * c.S, [[0] * c.nl] * c.S, 1)
    c = make_case("long_row-r0")   # unpadded: accepted
    W, B = c.weights()
    sg = PackedNetworks(W, B, c.K0, 0.1, cpu).flat_grad_target([[64] * c.nl] * c.S, [[128] * c.nl] * c.S, 4096)
    assert sg[1].gw[2] == 64 and sg[0].gbias[0] == 128 and sg[1].member_stride == 4096 and sg[0].accumulate == 1
    rs = np.random.RandomState(0)
    for widths in ((16, 1), (16, 8, 8, 8, 8, 1)):   # 1 and 5 Linear layers
        W1 = [[[torch.from_numpy(rs.randn(o, i).astype(np.float32)) for i, o in zip(widths[:-1], widths[1:])]]]
        B1 = [[[torch.zeros(w.shape[0]) for w in W1[0][0]]]]
        with pytest.raises(ValueError, match="2..4 Linear layers"):
            PackedNetworks(W1, B1, 16, 0.1, cpu)


def test_weight_scale_when_the_largest_weight_is_just_below_a_power_of_two():
    """The split-fp16 planes put a layer's largest weight into [2^13, 2^14).  The largest float below 2^-4 -- a value uniform
    +-1 / sqrt(256) weights reach -- has log2f == -4 in fp32: the packer took the exponent from it and scaled such a layer by
    half of what the layouts promise (found by the (256, 256, 256) network of this table).  Exact powers of two and the float
    above one are the neighbouring cases."""
    rs = np.random.RandomState(4)
    below = float(np.nextafter(np.float32(2.0 ** -4), np.float32(0)))
    for top, want in ((below, 2.0 ** 18), (2.0 ** -4, 2.0 ** 17), (float(np.nextafter(np.float32(2.0 ** -4), np.float32(1))), 2.0 ** 17)):
        W = [[[torch.from_numpy(rs.uniform(-0.05, 0.05, (o, i)).astype(np.float32)) for i, o in ((32, 32), (32, 32), (32, 1))]]]
        W[0][0][1][3, 5] = -top
        B = [[[torch.zeros(w.shape[0]) for w in W[0][0]]]]
        pk = _check_pack_against_reference(W, B, 32)
        assert pk.desc.net[0].wh_scale[1] == want
        assert 2.0 ** 13 <= top * pk.desc.net[0].wh_scale[1] < 2.0 ** 14
