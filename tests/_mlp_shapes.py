"""Network shapes off ANI's for the network kernels (csrc/mlp.hip, mlp_fused.hip, train.hip, pack.hip): the shape table, seeded
cases in the oracle's packed layout, and a second fp64 reference (torch autograd on the CPU) for what the oracle does not
have -- GELU networks and input-space Hessian-vector products.

What the library accepts (include/anihip.h, check_desc, anihip_mlp_pack): 2..4 Linear layers, any hidden width (padded to 32),
1..64 members, 1..7 species, any AEV length that is a multiple of 16.  The shapes below are the smallest that reach each
decision the host code takes from a shape:

  one_hidden     nl = 2 (amax slots with nh = 1); K0 = 48 is no multiple of 32; widths padded 33 -> 64 and 8 -> 32
  two_hidden     nl = 3 (nh = 2); a hidden width of 1
  long_row       widths the fused kernel covers, but K0p = 1056 > 1024: layer by layer, layer 0 with k_valid
  wide           one species above FR_MAXH = 256 sends every species to the layer-by-layer kernels
  wide_320       the same with a 320-wide first layer
  fused_edges    (256, 256, 256) passes the width test of the fused kernel but not its LDS budget (H2 + max(H1, H3) <= 448
                 padded columns, csrc/mlp.hip: fused_dims_supported): the whole pack runs layer by layer; odd M; padded H3
  fused_fit      the largest tile the LDS takes (256, 192, 256), the narrowest (32, 256, 32), padded H3 (40 -> 64), odd M
  fused_l0b_min  (64, 128, 32) is the smallest network the layer-0 backward inside the fused kernel allows -- next to
                 (256, 256, 256) the pack is not fused at all and the forced flag is refused
  fused_l0b_fit  the same next to (256, 192, 256): runs with MLP_FLAG_FUSED_L0B forced
  many_members   S = 1, M at its limit of 64, one 32-column slab

(fused_fit and fused_l0b_fit exist because the (256, 256, 256) networks of fused_edges and fused_l0b_min turned out not to fit
the fused kernel's LDS: 174.6 KB of 160.)

A case: 200 to 300 atoms, some of them padding (species -1), ONE species with many atoms (more than two 64-row tiles, the last
one partly filled), one species with exactly one atom and -- from three species on -- one species with no atom at all.  A shape
has one case per "rotation" of these roles over its species that reaches something new (ROTATIONS): with rotation r species
r is the one with many atoms, r + 1 the one with one atom.  A pack of one species has no room for a one-atom species.
Weights and biases: uniform +-1 / sqrt(fan_in) like weights.random_network_state_dict, seeded; AEV rows: rand^2 * 0.8 like
test_gpu_fused_addressing.make_case (non-negative, mostly small); where the row has the ANI layout (K0 = 240 for three
species) the columns that only neighbors of the species without atoms could fill are zero, as in any real row.
"""
from __future__ import annotations

import ctypes as C
import functools
import zlib

import numpy as np
import torch

from torchani_amd import _lib

SHAPES = {
    # name: (K0, hidden widths per species, members)
    "one_hidden": (48, ((33,), (8,)), 5),
    "two_hidden": (80, ((100, 40), (1, 17)), 3),
    "long_row": (1040, ((160, 128, 96), (160, 128, 96)), 2),
    "wide": (384, ((288, 96, 33), (64, 32, 32)), 2),
    "wide_320": (384, ((320, 96, 33), (64, 32, 32)), 2),
    "fused_edges": (240, ((256, 256, 256), (32, 256, 32), (96, 224, 40)), 13),
    "fused_fit": (240, ((256, 192, 256), (32, 256, 32), (96, 224, 40)), 13),
    "fused_l0b_min": (240, ((64, 128, 32), (256, 256, 256), (96, 224, 40)), 4),
    "fused_l0b_fit": (240, ((64, 128, 32), (256, 192, 256), (96, 224, 40)), 4),
    "many_members": (16, ((7, 5, 3),), 64),
}
# rotations of the roles (many atoms / one atom / no atom) that reach something new: every network of the shapes that run
# fused gets the many-atom role once; the layer-by-layer shapes give it to each of their distinct networks
ROTATIONS = {"one_hidden": (0, 1), "two_hidden": (0, 1), "long_row": (0,), "wide": (0, 1), "wide_320": (0,),
             "fused_edges": (0,), "fused_fit": (0, 1, 2), "fused_l0b_min": (0,), "fused_l0b_fit": (0, 1, 2),
             "many_members": (0,)}
CASE_IDS = [f"{name}-r{r}" for name in SHAPES for r in ROTATIONS[name]]
# seeds: salt 0 unless tests/_util.py:celu_kink_atoms then flags more than 5 % of the case's atoms in the fp64 reference, else
# the salt among the first eight with the fewest flagged atoms (13 members x 768 hidden units x 250 atoms are 2.5 M
# pre-activations, each within 1e-6 of its scale of zero with probability ~1e-6 per side: a dozen atoms; the cap is checked in
# tests/test_network_shapes_host.py)
SEED_SALT = {"fused_edges-r0": 4}
FUSED_LDS_COLUMNS = 448   # H2 + max(H1, H3), padded columns (csrc/mlp.hip: fused_dims_supported)


def pad32(x):
    return (x + 31) // 32 * 32


def fused_shape(name, precision="f16x3"):
    """Does forward_backward of this shape run through the fused network kernel (csrc/mlp.hip: fb_plan)?"""
    K0, hidden, _ = SHAPES[name]
    if precision != "f16x3" or len(hidden[0]) != 3 or pad32(K0) > 1024:
        return False
    return all(max(map(pad32, h)) <= 256 and pad32(h[1]) + max(pad32(h[0]), pad32(h[2])) <= FUSED_LDS_COLUMNS for h in hidden)


def l0b_shape(name):
    """... and may its layer-0 backward run inside the kernel (fb_plan: l0b_ok, four-layer CELU packs)?"""
    return fused_shape(name) and all(pad32(h[0]) >= 64 and pad32(h[1]) >= 128 for h in SHAPES[name][1])


# ---- what the library says about its route ---------------------------------------------------------------------------------
def fb_route(packed, n, flags=0):
    """"layers" | "fused" (d E / d act0 handed to a layer-0 backward GEMM) | "fused_l0b", from the workspace a
    forward_backward call of n atoms touches without and with a gradient (csrc/mlp.hip: fb_plan, mlp_carve)"""
    L = _lib.lib()
    d = packed.desc
    old = d.flags
    d.flags = flags
    try:
        need0 = L.anihip_mlp_forward_backward_workspace_bytes(C.byref(d), n, 0)
        need1 = L.anihip_mlp_forward_backward_workspace_bytes(C.byref(d), n, 1)
    finally:
        d.flags = old
    act0 = 4 * packed.M * max(d.net[s].dims[1] for s in range(packed.S)) * n   # the first hidden layer of every member
    assert 0 < need0 <= need1 <= L.anihip_mlp_workspace_bytes(C.byref(d), n)
    if need0 >= act0:
        assert need1 == need0
        return "layers"
    if need1 - need0 >= act0:
        return "fused"
    assert need1 == need0
    return "fused_l0b"


VARIANTS = {"f16x3": ("f16x3", 0), "f16x3-unfused": ("f16x3", _lib.MLP_FLAG_NO_FUSED), "f16x3-bigtile": ("f16x3", _lib.MLP_FLAG_BIG_TILES),
            "f16x3-l0b": ("f16x3", _lib.MLP_FLAG_FUSED_L0B), "fp32": ("fp32", 0)}


def expected_route(name, variant):
    """(a forced layer-0 backward the shape cannot serve leaves the query at "fused": the call itself is refused)"""
    if variant in ("fp32", "f16x3-unfused") or not fused_shape(name):
        return "layers"
    return "fused_l0b" if variant == "f16x3-l0b" and l0b_shape(name) else "fused"
class Case:
    """name, rot, K0, hidden, M, S, nl; dims [S][nl + 1], flat (fp64 copy of the fp32 parameters, oracle.pack_networks order);
    species int32 [n], aev float32 [n][K0], g_atom float32 [n] (upstream of the training pass), tangent float32 [n][K0];
    n_pad, many / single / empty: the species in these roles (None where the shape has none)."""

    def weights(self, device=None, bias=True):
        """(W[m][s][l], B[m][s][l]) fp32 torch tensors in torch.nn.Linear layout; bias=False: zero biases"""
        return parameter_lists(self.dims, self.flat, self.M, device, bias)

    def flat_without_biases(self):
        out, off = self.flat.copy(), 0
        for m in range(self.M):
            for s in range(self.S):
                for l in range(self.nl):
                    kin, kout = int(self.dims[s, l]), int(self.dims[s, l + 1])
                    out[off + kin * kout:off + kin * kout + kout] = 0.0
                    off += kin * kout + kout
        return out


def parameter_lists(dims, flat, M, device=None, bias=True):
    """the packed vector ``flat`` (oracle.pack_networks order) as (W[m][s][l] [out][in], B[m][s][l] [out]) fp32 torch tensors"""
    S, nl = dims.shape[0], dims.shape[1] - 1
    W = [[[None] * nl for _ in range(S)] for _ in range(M)]
    B = [[[None] * nl for _ in range(S)] for _ in range(M)]
    off = 0
    for m in range(M):
        for s in range(S):
            for l in range(nl):
                kin, kout = int(dims[s, l]), int(dims[s, l + 1])
                w = torch.from_numpy(flat[off:off + kin * kout].astype(np.float32).reshape(kout, kin).copy())
                off += kin * kout
                b = torch.from_numpy(flat[off:off + kout].astype(np.float32).copy())
                off += kout
                if not bias:
                    b = torch.zeros_like(b)
                W[m][s][l] = w if device is None else w.to(device)
                B[m][s][l] = b if device is None else b.to(device)
    return W, B


def stage_stress(dims, flat, M, first=2.0 ** 10, last=2.0 ** -14):
    """``flat`` with layer 0 (weights and biases) times ``first`` and the output layer times ``last``, powers of two: the
    activations grow a thousandfold, what the backward pass hands down shrinks to 1e-5 .. 1e-6, d E / d AEV keeps a size the
    gates can see.  The layer-by-layer split-fp16 kernels scale every operand by a power of two taken from a running maximum
    of ITS stage (csrc/mlp.hip: the amax slots); a GEMM that reads another stage's slot, or an unwritten one (scale 1), then
    splits 1e-5-sized values in fp16's subnormal range -- two digits left -- or overflows the large ones."""
    out, off = np.array(flat, dtype=np.float64, copy=True), 0
    nl = dims.shape[1] - 1
    for m in range(M):
        for s in range(dims.shape[0]):
            for l in range(nl):
                n = int(dims[s, l]) * int(dims[s, l + 1]) + int(dims[s, l + 1])
                if l == 0:
                    out[off:off + n] *= first
                if l == nl - 1:
                    out[off:off + n] *= last
                off += n
    return out


def draw_parameters(dims, M, rs):
    """flat fp64 vector (of fp32 values) in oracle.pack_networks order: uniform +-1 / sqrt(fan_in)"""
    flat = []
    for m in range(M):
        for s in range(dims.shape[0]):
            for l in range(dims.shape[1] - 1):
                kin, kout = int(dims[s, l]), int(dims[s, l + 1])
                bound = 1.0 / np.sqrt(kin)
                flat.append(rs.uniform(-bound, bound, kout * kin).astype(np.float32))
                flat.append(rs.uniform(-bound, bound, kout).astype(np.float32))
    return np.concatenate(flat).astype(np.float64)


def ani_columns_of(S, species):
    """columns of an ANI-layout row (16 S radial + 32 S (S + 1) / 2 angular) that neighbors of ``species`` fill"""
    cols = list(range(16 * species, 16 * species + 16))
    for a in range(S):
        for b in range(a, S):
            if species in (a, b):
                first = 16 * S + 32 * (a * S - a * (a - 1) // 2 + (b - a))
                cols += list(range(first, first + 32))
    return np.asarray(cols)


@functools.lru_cache(maxsize=None)
def make_case(case_id):
    name, rot = case_id.rsplit("-r", 1)
    rot = int(rot)
    K0, hidden, M = SHAPES[name]
    seed = zlib.crc32(f"{case_id}/{SEED_SALT.get(case_id, 0)}".encode()) % (2 ** 31)
    rs = np.random.RandomState(seed)
    c = Case()
    c.id, c.name, c.rot, c.K0, c.hidden, c.M, c.S, c.nl = case_id, name, rot, K0, hidden, M, len(hidden), len(hidden[0]) + 1
    c.dims = np.asarray([[K0] + list(h) + [1] for h in hidden], dtype=np.int32)
    c.flat = draw_parameters(c.dims, M, rs)
    n = int(rs.randint(200, 301))
    c.n_pad = int(rs.randint(9, 20))
    c.many = rot % c.S
    c.single = (rot + 1) % c.S if c.S >= 2 else None
    c.empty = (rot + 2) % c.S if c.S >= 3 else None
    species = np.full(n, c.many, dtype=np.int32)
    special = rs.choice(n, c.n_pad + (c.single is not None), replace=False)
    species[special[:c.n_pad]] = -1
    if c.single is not None:
        species[special[c.n_pad]] = c.single
    c.species = species
    gen = torch.Generator().manual_seed(seed)
    c.aev = (torch.rand((n, K0), generator=gen) ** 2 * 0.8).numpy().astype(np.float32)
    if c.empty is not None and K0 == 16 * c.S + 16 * c.S * (c.S + 1):
        # the ANI layout of the row (16 radial columns per species, 32 angular ones per species pair): the columns of a species
        # without atoms are zero for every atom -- the training passes of such a pack skip them (csrc/train.h: x_slab_rad)
        c.aev[:, ani_columns_of(c.S, c.empty)] = 0.0
    c.g_atom = rs.uniform(-1.0, 1.0, n).astype(np.float32)
    c.tangent = rs.uniform(-0.5, 0.5, (n, K0)).astype(np.float32)
    return c


# ---- the second reference: torch float64 on the CPU, derivatives by autograd ----------------------------------------------
def _activation(x, activation, alpha):
    if activation == "celu":
        # NOT torch.nn.functional.celu: its backward holds 1 / alpha in fp32 (torch 2.x, fp64 tensors on the CPU), which puts
        # 1e-8 on its first derivative at alpha = 0.1 and 3e-7 on its second -- that is the 3e-10 by which a plain torch MLP
        # and the oracle differed on d E / d AEV.  Written out, values and both derivatives agree with exp(x / alpha) to 1e-16.
        return torch.where(x > 0, x, alpha * torch.expm1(torch.clamp(x, max=0.0) / alpha))
    if activation == "gelu":
        return torch.nn.functional.gelu(x)   # exact (erf): torch.nn.GELU(), what the kernels implement
    raise ValueError(activation)


class TorchReference:
    """fp64 MLP ensemble over the packed (dims, flat) layout of oracle.pack_networks: per member and species a chain of
    Linear layers with CELU(alpha) or exact GELU between them, atomic energy = mean over the members; padding atoms
    (species < 0) have zero energy.  Every derivative comes from torch autograd."""

    def __init__(self, dims, flat, n_members, activation="celu", celu_alpha=0.1):
        self.dims = np.asarray(dims)
        self.M, self.S, self.nl = int(n_members), self.dims.shape[0], self.dims.shape[1] - 1
        self.activation, self.alpha = activation, celu_alpha
        self.flat = torch.tensor(np.asarray(flat, dtype=np.float64), dtype=torch.float64, requires_grad=True)
        self.views, off = [], 0
        for m in range(self.M):
            for s in range(self.S):
                layers = []
                for l in range(self.nl):
                    kin, kout = int(self.dims[s, l]), int(self.dims[s, l + 1])
                    layers.append((slice(off, off + kin * kout), slice(off + kin * kout, off + kin * kout + kout), kout, kin))
                    off += kin * kout + kout
                self.views.append(layers)
        assert off == self.flat.numel()

    def member_energies(self, species, aev):
        """[M][n] (a differentiable function of self.flat and aev)"""
        species = torch.as_tensor(np.asarray(species).reshape(-1).astype(np.int64))
        n = species.numel()
        out = []
        for m in range(self.M):
            e = torch.zeros(n, dtype=torch.float64)
            for s in range(self.S):
                rows = torch.nonzero(species == s).reshape(-1)
                if rows.numel() == 0:
                    continue
                x = aev[rows]
                for l, (w, b, kout, kin) in enumerate(self.views[m * self.S + s]):
                    x = x @ self.flat[w].view(kout, kin).t() + self.flat[b]
                    if l < self.nl - 1:
                        x = _activation(x, self.activation, self.alpha)
                e = e.index_add(0, rows, x[:, 0])
            out.append(e)
        return torch.stack(out)

    def _aev(self, aev):
        return torch.tensor(np.asarray(aev, dtype=np.float64), dtype=torch.float64, requires_grad=True)

    def energies(self, species, aev):
        """(atomic energies [n], member energies [M][n], d atomic_e / d aev [n][K0]) as numpy fp64"""
        a = self._aev(aev)
        me = self.member_energies(species, a)
        ae = me.mean(dim=0)
        (g,) = torch.autograd.grad(ae.sum(), a)
        return ae.detach().numpy(), me.detach().numpy(), g.numpy()

    def weight_grads(self, species, aev, g_atom):
        """d (sum_i g_atom[i] atomic_e[i]) / d params, in the layout of flat"""
        a = self._aev(aev)
        ae = self.member_energies(species, a).mean(dim=0)
        loss = (ae * torch.as_tensor(np.asarray(g_atom, dtype=np.float64).reshape(-1))).sum()
        (g,) = torch.autograd.grad(loss, self.flat)
        return g.numpy()

    def tangent_weight_grads(self, species, aev, tangent):
        """(S, d S / d params, per-atom terms of S) for S = sum_i tangent_i . d atomic_e[i] / d aev_i"""
        a = self._aev(aev)
        ae = self.member_energies(species, a).mean(dim=0)
        (ga,) = torch.autograd.grad(ae.sum(), a, create_graph=True)
        per_atom = (ga * torch.as_tensor(np.asarray(tangent, dtype=np.float64))).sum(dim=1)
        (g,) = torch.autograd.grad(per_atom.sum(), self.flat)
        return float(per_atom.sum().detach()), g.numpy(), per_atom.detach().numpy()

    def input_hvp(self, species, aev, tangents):
        """[K][n][K0]: (d^2 atomic_e[i] / d aev_i^2) tangents[k][i], by double backward"""
        out = []
        for t in np.asarray(tangents, dtype=np.float64):
            a = self._aev(aev)
            ae = self.member_energies(species, a).mean(dim=0)
            (ga,) = torch.autograd.grad(ae.sum(), a, create_graph=True)
            (h,) = torch.autograd.grad((ga * torch.as_tensor(t)).sum(), a)
            out.append(h.numpy())
        return np.stack(out)


@functools.lru_cache(maxsize=None)
def torch_reference(case_id, activation="celu", bias=True):
    c = make_case(case_id)
    return TorchReference(c.dims, c.flat if bias else c.flat_without_biases(), c.M, activation)
