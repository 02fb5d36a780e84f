"""Where the fused network kernel's addresses can go wrong (csrc/mlp_fused.hip: weight rings and per-column parameters on a
wave-uniform base + 32-bit lane offset, kernel arguments re-read at the head of every phase, the per-species launches'
FusedArgs::one): ``PackedNetworks.forward_backward`` on seeded random ANI-2x weights and synthetic AEV rows with slab masks,
against the package's exact layer-by-layer path (an fp32 pack of the same weights) -- the compile-time-width networks one
species at a time, the run-time-width kernel on all seven species, partial last tiles and more than one tile per workgroup,
1 / 4 / 5 / 17 flagged slabs per tile (kept operand, its limit, staged operand, multi-pass phase 5), an atom without
neighbors, a central range inside a tile, the tile queue on and off, the two-product backward; the second stream of the
queued per-species launches, which is the pack's own (anihip_mlp_desc.aux_stream): with and without it, created lazily, one
per pack under two host threads.

Tolerances are those of test_gpu_parity.test_mlp_ensemble for the same quantities (per-atom energies 3e-7 Ha, d E / d AEV
1e-6 + 1e-5 of its largest entry).  Every case is evaluated twice: the kernel sums in a fixed order, so per-atom energies
and d E / d AEV are equal bit for bit.

Synthetic rows: every atom of a case flags the same slabs (the tile's mask is then that mask, whatever the tile), its AEV
is zero outside them -- the reference multiplies every column -- and d E / d AEV is compared inside them (forward_backward
defines it nowhere else).  The queue needs four rounds of tiles over the CUs (per-species launches) or more tiles than CUs
(one launch for all species): those two cases are as small as that allows, everything else a few hundred atoms.
"""
import threading
import time

import numpy as np
import pytest
import torch

from _util import seeded_state
from torchani_amd import _lib

pytestmark = pytest.mark.gpu

E_TOL = 3e-7                     # test_gpu_parity.test_mlp_ensemble
G_ABS, G_REL = 1e-6, 1e-5        # the same test: |d e / d aev err| < 1e-6 + 1e-5 max |d e / d aev|
BWD2_TOL = 1e-4                  # test_two_product_backward_is_off_by_default_and_inside_the_parity_gate: the parity gate
# ... and a bound of this file's own for d E / d AEV, which that gate (made for forces) does not pin down: the two-product
# backward counts the weights of its three GEMMs as rounded to fp16, a relative 2^-12 each (include/anihip.h), so the result
# moves by at most 3 x 2^-12 of its largest entry on top of the three-product gate's absolute part
BWD2_REL = 3 * 2.0 ** -12
SEED = 31
H, C, N, O, S, F, CL = range(7)  # ANI-2x species; networks 256/192/160 (H), 224/192/160 (C), 192/160/128 (N, O), 160/128/96
N_SLABS = 32                     # 4 radial + 28 angular 32-column slabs of the 1008-column row
# flagged slabs of a case: radial ones first (the fourth radial slab has 16 valid columns), then angular ones
SLABS = {1: (5,), 4: (0, 3, 4, 31), 5: (0, 1, 3, 9, 30), 17: tuple(range(2, 32, 2)) + (3, 31)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def packs(dev):
    """(split-fp16 pack: the fused kernel, fp32 pack: the exact layer-by-layer kernels) of one set of weights"""
    from torchani_amd.models import ANI2x

    model = ANI2x(state_dict=seeded_state("ani2x", 8, SEED), device=dev, periodic_table_index=False)
    nets = model.neural_networks
    fused = nets._pack(dev)
    nets.mlp_precision = "fp32"
    try:
        exact = nets._pack(dev)
    finally:
        nets.mlp_precision = None
    assert fused.precision == "f16x3" and exact.precision == "fp32" and fused.M == 8 and fused.aev_len == 1008
    return fused, exact


def fresh_pack(dev):
    """a split-fp16 pack of `packs`' weights that no call has touched yet (from a model instance of its own)"""
    from torchani_amd.models import ANI2x

    model = ANI2x(state_dict=seeded_state("ani2x", 8, SEED), device=dev, periodic_table_index=False)
    return model.neural_networks._pack(dev)


@pytest.fixture(scope="module")
def queued(dev, packs):
    """The smallest system whose per-species launches draw their tiles from queues (test_tile_queue_of_the_per_species_launches
    derives the size), with its result through `packs`' fused pack and that pack's own second stream: (species, AEV rows, slab
    masks, per-atom energies, d E / d AEV).  Shared by the tests below, which leave it unchanged."""
    fused, _ = packs
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    n = 4 * n_cu * 64 + 3 * 64 + 17
    sp, aev, mask, _ = make_case(dev, np.where(np.arange(n) % 3 == 2, O, H), 4, 21)
    e, g = run_fused(fused, sp, aev, mask, _lib.MLP_FLAG_FUSED_L0B, hint=_lib.MLP_FLAG_SHAPED)
    return sp, aev, mask, e, g


def slab_columns(slabs, radial_len=112):
    """columns of the row that the flagged slabs cover, in the ANI slab order (include/anihip.h)"""
    rs = (radial_len + 31) // 32
    cols = []
    for j in slabs:
        c0 = 32 * j if j < rs else radial_len + 32 * (j - rs)
        nv = radial_len - 32 * (rs - 1) if j == rs - 1 else 32
        cols += list(range(c0, c0 + nv))
    return torch.tensor(sorted(cols), dtype=torch.int64)


def make_case(dev, species, n_slabs, seed, lonely=None):
    """species [n] (numpy), every atom flagging SLABS[n_slabs]; atom `lonely` has no neighbor: mask 0, a zero row"""
    n = len(species)
    gen = torch.Generator().manual_seed(seed)
    cols = slab_columns(SLABS[n_slabs])
    aev = torch.zeros((n, 1008), dtype=torch.float32)
    aev[:, cols] = torch.rand((n, cols.numel()), generator=gen) ** 2 * 0.8   # (AEV terms: non-negative, mostly small)
    bits = 0
    for j in SLABS[n_slabs]:
        bits |= 1 << j
    mask = torch.full((n,), bits - (1 << 32) if bits >= 1 << 31 else bits, dtype=torch.int32)
    if lonely is not None:
        aev[lonely] = 0.0
        mask[lonely] = 0
    sp = torch.from_numpy(np.asarray(species, dtype=np.int32))
    return sp.to(dev), aev.to(dev), mask.to(dev), cols.to(dev)


def run_fused(fused, sp, aev, mask, flags, hint=0, lo=0, hi=None, shard=False):
    """two evaluations: (energies, d E / d AEV) of the first, after asserting that the second equals it bit for bit"""
    got = []
    fused.flags = flags
    try:
        for _ in range(2):
            rows = aev.shape[0]
            ga = torch.zeros((rows, fused.aev_len), dtype=torch.float32, device=aev.device)
            e, _, _ = fused.forward_backward(sp, aev, lo=lo, hi=hi, grad_aev=ga, slab_mask=mask, shard_rows=shard, tile_hint=hint)
            got.append((e.clone(), ga))
    finally:
        fused.flags = None
    torch.cuda.synchronize()
    assert torch.equal(got[0][0], got[1][0]), "per-atom energies differ between two evaluations"
    assert torch.equal(got[0][1], got[1][1]), "d E / d AEV differs between two evaluations"
    return got[0]


def reference(exact, sp, aev_full):
    e, g, _ = exact.forward_backward(sp, aev_full)
    torch.cuda.synchronize()
    return e, g


def check(tag, e, g, e_ref, g_ref, cols, g_abs=G_ABS, g_rel=G_REL):
    e_err = float((e - e_ref).abs().max())
    gmax = float(g_ref[:, cols].abs().max())
    g_err = float((g[:, cols] - g_ref[:, cols]).abs().max())
    print(f"fused addressing {tag}: max|e_atom err| = {e_err:.2e}  max|d e/d aev err| = {g_err:.2e} (max {gmax:.2e})")
    assert gmax > 1e-4, "the case exercises nothing"
    assert e_err < E_TOL
    assert g_err < g_abs + g_rel * gmax
    # outside the flagged slabs nothing is written (the rows were zero before the call)
    other = torch.ones(g.shape[1], dtype=torch.bool, device=g.device)
    other[cols] = False
    assert not bool(g[:, other].any())


@pytest.mark.parametrize("species", [H, C, O, F], ids=["256-192-160", "224-192-160", "192-160-128", "160-128-96"])
def test_compile_time_widths_one_species(dev, packs, species):
    """Per-species launches (MLP_FLAG_SHAPED: FusedArgs::one, the compile-time-width instantiations) of 1, 63, 64, 65 and 130
    atoms -- a lone row, partial last tiles, one full tile, more than one tile -- with four flagged slabs (the kept operand)."""
    fused, exact = packs
    for n in (1, 63, 64, 65, 130):
        sp, aev, mask, cols = make_case(dev, [species] * n, 4, 100 + n)
        e, g = run_fused(fused, sp, aev, mask, _lib.MLP_FLAG_FUSED_L0B, hint=_lib.MLP_FLAG_SHAPED)
        e_ref, g_ref = reference(exact, sp, aev)
        check(f"species {species} n {n}", e, g, e_ref, g_ref, cols)


@pytest.mark.parametrize("shaped", [False, True], ids=["one-launch", "per-species"])
def test_all_seven_species_mixed(dev, packs, shaped):
    """All seven species in one call of 333 atoms: the run-time-width instantiation (one launch), or seven per-species launches
    of which four take a compile-time-width instantiation each."""
    fused, exact = packs
    rs = np.random.RandomState(5)
    species = rs.randint(0, 7, 333)
    sp, aev, mask, cols = make_case(dev, species, 4, 7)
    e, g = run_fused(fused, sp, aev, mask, _lib.MLP_FLAG_FUSED_L0B, hint=_lib.MLP_FLAG_SHAPED if shaped else 0)
    e_ref, g_ref = reference(exact, sp, aev)
    check(f"seven species shaped={shaped}", e, g, e_ref, g_ref, cols)


@pytest.mark.parametrize("n_slabs", [1, 4, 5, 17])
@pytest.mark.parametrize("shaped", [False, True], ids=["run-time", "compile-time"])
def test_flagged_slabs_per_tile(dev, packs, n_slabs, shaped):
    """1, 4, 5 and 17 flagged slabs per tile on 130 hydrogen + 70 oxygen atoms: the kept layer-0 operand (<= 4), the staged one,
    five passes of phase 5 with the read-add-write over the members; one atom has no neighbor at all (mask 0, a zero row:
    its tile still writes the tile's slabs of its row)."""
    fused, exact = packs
    species = [H] * 130 + [O] * 70
    sp, aev, mask, cols = make_case(dev, species, n_slabs, 40 + n_slabs, lonely=77)
    e, g = run_fused(fused, sp, aev, mask, _lib.MLP_FLAG_FUSED_L0B, hint=_lib.MLP_FLAG_SHAPED if shaped else 0)
    e_ref, g_ref = reference(exact, sp, aev)
    check(f"{n_slabs} slabs shaped={shaped}", e, g, e_ref, g_ref, cols)


@pytest.mark.parametrize("shaped", [False, True], ids=["run-time", "compile-time"])
def test_central_range_inside_a_tile(dev, packs, shaped):
    """lo / hi that start and end inside a tile, shard_rows=True: the AEV and d E / d AEV buffers hold the rows lo .. hi only,
    atoms outside the range keep zero energy."""
    fused, exact = packs
    rs = np.random.RandomState(11)
    species = rs.choice([H, H, O], 300)
    lo, hi = 37, 37 + 171
    sp, aev, mask, cols = make_case(dev, species, 4, 12)
    part = aev[lo:hi].contiguous()
    e, g = run_fused(fused, sp, part, mask, _lib.MLP_FLAG_FUSED_L0B, hint=_lib.MLP_FLAG_SHAPED if shaped else 0, lo=lo, hi=hi,
                     shard=True)
    e_ref, g_ref = reference(exact, sp, aev)
    assert not bool(e[:lo].any()) and not bool(e[hi:].any())
    check(f"range {lo}..{hi} shaped={shaped}", e[lo:hi], g, e_ref[lo:hi], g_ref[lo:hi], cols)


def test_tile_queue_of_the_per_species_launches(dev, packs):
    """The queue ON through the flag the host sets for large water-like systems (MLP_FLAG_SHAPED): from four rounds of tiles over
    the CUs on, the per-species launches draw their tiles from one counter per species on two streams -- the smallest such
    system (hydrogen : oxygen 2 : 1), a sample of its rows against the reference (the two evaluations, whose workgroups draw
    their tiles in whatever order they come free, agree bit for bit).  Below that size the same flag is the static order:
    the queue OFF, every other test of this file."""
    fused, exact = packs
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    # csrc/mlp.hip turns the per-species queues on when tiles >= 4 * grid, with tiles = ceil(n / 64) + 7 (one spare tile per
    # species of the pack) and grid = one workgroup per CU (119 KB of LDS each): 4 n_cu full tiles and a little more
    n = 4 * n_cu * 64 + 3 * 64 + 17
    species = np.where(np.arange(n) % 3 == 2, O, H)
    sp, aev, mask, cols = make_case(dev, species, 4, 21)
    e, g = run_fused(fused, sp, aev, mask, _lib.MLP_FLAG_FUSED_L0B, hint=_lib.MLP_FLAG_SHAPED)
    pick = torch.from_numpy(np.random.RandomState(3).choice(n, 4096, replace=False)).to(dev)
    e_ref, g_ref = reference(exact, sp[pick].contiguous(), aev[pick].contiguous())
    check("queued per-species launches", e[pick], g[pick], e_ref, g_ref, cols)


def test_tile_queue_of_the_one_launch_form(dev, packs):
    """The queue ON in the run-time-width instantiation: all seven species, more tiles than CUs and more atoms than the
    single-launch preparation of small inputs takes (16 384)."""
    fused, exact = packs
    # csrc/mlp.hip hands the tiles out by falling cost when tiles > grid (ceil(n / 64) + 7 tiles against one workgroup per
    # CU: 256 on this part, 272 tiles here), at most 8192 tiles, and the input is past the small-input preparation (> 16 384)
    n = 16384 + 64 * 9 + 5
    assert n // 64 + 7 > torch.cuda.get_device_properties(dev).multi_processor_count
    species = np.random.RandomState(9).randint(0, 7, n)
    sp, aev, mask, cols = make_case(dev, species, 5, 22)
    e, g = run_fused(fused, sp, aev, mask, _lib.MLP_FLAG_FUSED_L0B)
    e_ref, g_ref = reference(exact, sp, aev)
    check("queued single launch", e, g, e_ref, g_ref, cols)


@pytest.mark.parametrize("species", [[H] * 64, [H, C, N, O, S, F, CL] * 9 + [H]], ids=["hydrogen-tile", "mixed-tile"])
def test_two_product_backward(dev, packs, species):
    """MLP_FLAG_BWD_TWO_PRODUCTS through the tile hint (the backward GEMMs leave out (weight lo) x (gradient hi); the same
    epilogues and rings): energies bit-identical to the three-product call's, d E / d AEV inside the parity gate of its
    existing test against the layer-by-layer reference and inside three fp16 weight roundings of it (BWD2_REL) -- and
    different from the three-product result, or the flag did nothing."""
    fused, exact = packs
    sp, aev, mask, cols = make_case(dev, species, 4, 33)
    e3, g3 = run_fused(fused, sp, aev, mask, _lib.MLP_FLAG_FUSED_L0B)
    e2, g2 = run_fused(fused, sp, aev, mask, _lib.MLP_FLAG_FUSED_L0B, hint=_lib.MLP_FLAG_BWD_TWO_PRODUCTS)
    e_ref, g_ref = reference(exact, sp, aev)
    assert torch.equal(e2, e3)
    assert float((g2 - g3).abs().max()) > 0.0
    check("two-product backward", e2, g2, e_ref, g_ref, cols, g_abs=BWD2_TOL, g_rel=0.0)
    check("two-product backward, rounding bound", e2, g2, e_ref, g_ref, cols, g_abs=G_ABS, g_rel=BWD2_REL)


def test_queued_launches_with_and_without_the_second_stream(dev, packs, queued):
    """The queued per-species launches with the pack's stream and events in the descriptor (forward_backward put them there at
    the first call with MLP_FLAG_SHAPED) and with the three fields cleared -- the library then creates nothing and launches on
    the caller's stream in static tile order: per-atom energies and d E / d AEV equal bit for bit (a tile's result does not
    depend on who computes it)."""
    fused, _ = packs
    sp, aev, mask, e, g = queued
    d = fused.desc
    handles = (d.aux_stream, d.fork_event, d.join_event)
    assert all(handles) and fused._second is not None
    assert handles[0] != torch.cuda.current_stream(dev).cuda_stream and handles[1] != handles[2]
    try:
        d.aux_stream = d.fork_event = d.join_event = None
        e0, g0 = run_fused(fused, sp, aev, mask, _lib.MLP_FLAG_FUSED_L0B, hint=_lib.MLP_FLAG_SHAPED)
        assert d.aux_stream is None and d.fork_event is None and d.join_event is None   # (nobody put them back behind our back)
    finally:
        d.aux_stream, d.fork_event, d.join_event = handles
    assert torch.equal(e, e0), "per-atom energies differ with and without the second stream"
    assert torch.equal(g, g0), "d E / d AEV differs with and without the second stream"


def test_second_stream_is_created_lazily(dev, packs):
    """A pack that has only been called without MLP_FLAG_SHAPED (member packs, training packs, small systems) holds no stream
    and no events and hands none to the library; the first call with the flag creates them.  Same weights, same kernel: the
    results equal those of `packs`' fused pack bit for bit."""
    fused, _ = packs
    pack = fresh_pack(dev)
    sp, aev, mask, _ = make_case(dev, [H] * 130 + [O] * 70, 4, 44)
    d = pack.desc
    assert d.aux_stream is None and d.fork_event is None and d.join_event is None and pack._second is None
    e, g = run_fused(pack, sp, aev, mask, _lib.MLP_FLAG_FUSED_L0B)
    assert d.aux_stream is None and d.fork_event is None and d.join_event is None and pack._second is None
    e1, g1 = run_fused(pack, sp, aev, mask, _lib.MLP_FLAG_FUSED_L0B, hint=_lib.MLP_FLAG_SHAPED)
    assert d.aux_stream and d.fork_event and d.join_event
    assert pack._second[0].cuda_stream == d.aux_stream and d.aux_stream != fused.desc.aux_stream
    for hint, (ea, ga) in ((0, (e, g)), (_lib.MLP_FLAG_SHAPED, (e1, g1))):
        eb, gb = run_fused(fused, sp, aev, mask, _lib.MLP_FLAG_FUSED_L0B, hint=hint)
        assert torch.equal(ea, eb) and torch.equal(ga, gb)


def test_two_host_threads_with_a_second_stream_each(dev, queued):
    """Two packs of the same weights, each with a second stream and events of its own, called from two host threads at once
    (ctypes releases the GIL), each on a stream of its own as the caller's stream, three queued calls per thread: nothing is
    shared between them -- the library keeps no stream, event or lock -- and every result equals the single-threaded one bit for
    bit.  Four streams in all.  The threads are joined with a time limit (three calls per thread, so six single-threaded calls
    if the device ran them one after the other; ten times that plus 30 s for a busy host), so a stall fails the test instead of
    blocking it."""
    sp, aev, mask, e_ref, g_ref = queued
    twins = [fresh_pack(dev) for _ in range(2)]
    streams = [torch.cuda.Stream(device=dev) for _ in twins]
    for pack in twins:
        pack.flags = _lib.MLP_FLAG_FUSED_L0B
    torch.cuda.synchronize()

    def calls(k, count, out):
        try:
            with torch.cuda.stream(streams[k]):
                for _ in range(count):
                    ga = torch.zeros_like(aev)
                    e, _, _ = twins[k].forward_backward(sp, aev, grad_aev=ga, slab_mask=mask, tile_hint=_lib.MLP_FLAG_SHAPED)
                    out.append((e, ga))
                streams[k].synchronize()
        except BaseException as err:   # (handed to the main thread, which fails the test with it)
            out.append(err)

    single = []
    t0 = time.perf_counter()
    calls(0, 1, single)
    t_single = time.perf_counter() - t0
    limit = 30.0 + 10 * 6 * t_single
    results = [[], []]
    threads = [threading.Thread(target=calls, args=(k, 3, results[k]), daemon=True) for k in range(2)]
    t0 = time.perf_counter()
    for t in threads:
        t.start()
    for t in threads:
        t.join(max(0.0, limit - (time.perf_counter() - t0)))
    t_both = time.perf_counter() - t0
    print(f"two host threads: one call alone {t_single:.3f} s, 2 x 3 calls {t_both:.3f} s (limit {limit:.1f} s)")
    assert not any(t.is_alive() for t in threads), f"a thread has not come back after {limit:.1f} s"
    torch.cuda.synchronize()
    aux = [pack.desc.aux_stream for pack in twins]
    assert all(aux) and len({*aux, *(s.cuda_stream for s in streams)}) == 4
    for tag, out in (("alone", single), ("thread 0", results[0]), ("thread 1", results[1])):
        assert len(out) == (1 if tag == "alone" else 3), f"{tag}: {out[-1] if out else 'no result'}"
        for e, ga in out:
            assert torch.equal(e, e_ref), f"{tag}: per-atom energies differ from the single-threaded result"
            assert torch.equal(ga, g_ref), f"{tag}: d E / d AEV differs from the single-threaded result"
