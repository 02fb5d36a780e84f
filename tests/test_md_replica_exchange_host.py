"""CPU checks of temperature replica exchange: the declarations of the entry point, the ladder builder's errors, and the
definition itself (tests/_md_replica_exchange_ref.py, the fp64 restatement of include/anihip.h that the GPU tests compare the
kernels with): one attempt leaves the canonical law of every rung invariant, occupancy stays a permutation, and the round-trip
counter counts."""
import os
import re

import numpy as np
import pytest

import _md_replica_exchange_ref as rx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_and_bound():
    import ctypes as C

    from torchani_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "anihip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(anihip_[a-z_0-9]+)\s*\(", code))
    assert "anihip_md_exchange" in declared and "anihip_md_exchange" in _lib.EXPORTED_SYMBOLS
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    assert re.search(r"#define\s+ANIHIP_MD_EXCHANGE_STEP\s+\(1ull << 61\)", hdr)
    assert _lib.MD_EXCHANGE_STEP == rx.EXCHANGE_STEP == 1 << 61
    # disjoint from the barostat's bit and the Maxwell-Boltzmann bit
    assert _lib.MD_EXCHANGE_STEP & (_lib.MD_BAROSTAT_STEP | 1 << 63) == 0
    assert re.search(r"#define\s+ANIHIP_ABI_VERSION\s+13\b", hdr) and _lib.ABI_VERSION == 13
    assert re.search(r"#define\s+ANIHIP_MD_LADDERS_CHECK\s+1\b", hdr) and _lib.MD_LADDERS_CHECK == 1
    # the struct of the header, field for field: four int32 and ten pointers
    body = re.search(r"typedef struct \{([^}]*)\} anihip_md_ladders;", code).group(1)
    names = re.findall(r"\*?\b([a-z_A-Z]+)\s*[,;]", body)
    assert names == [n for n, _ in _lib.MdLadders._fields_]
    assert C.sizeof(_lib.MdLadders) == 4 * 4 + 10 * C.sizeof(C.c_void_p)
    from torchani_amd.md import BatchedDynamics, ReplicaExchangeDynamics, RingPolymerDynamics

    assert issubclass(ReplicaExchangeDynamics, BatchedDynamics) and not issubclass(ReplicaExchangeDynamics, RingPolymerDynamics)
    for name in ("_drift", "_kick", "_evaluate", "run", "kinetic_energies", "temperatures"):
        assert name not in ReplicaExchangeDynamics.__dict__


def test_temperature_ladder_is_geometric():
    from torchani_amd.md import temperature_ladder

    t = temperature_ladder(300.0, 600.0, 8).numpy()
    assert t.dtype == np.float64 and t[0] == 300.0 and abs(t[-1] - 600.0) <= 1e-10
    assert np.allclose(t[1:] / t[:-1], 2.0 ** (1.0 / 7.0), rtol=1e-14, atol=0)
    assert np.allclose(t, rx.geometric(300.0, 600.0, 8), rtol=1e-14, atol=0)
    for bad in ((300.0, 600.0, 1), (600.0, 300.0, 4), (0.0, 300.0, 4)):
        with pytest.raises(ValueError):
            temperature_ladder(*bad)


def test_ladder_builder_tables_and_errors():
    import torch

    from torchani_amd.md import build_ladders

    T = torch.tensor([300.0, 350.0, 400.0, 200.0, 250.0, 100.0, 500.0])
    # the default: one ladder of every entry in batch order needs rising temperatures
    with pytest.raises(ValueError, match="strictly increasing"):
        build_ladders(None, T)
    t = build_ladders(None, T[:3])
    assert t.slot.tolist() == [[0, 1, 2]] and t.count.tolist() == [3] and t.rung_of.tolist() == [0, 1, 2]
    assert t.direction.tolist() == [1, 0, -1] and t.rung_temperatures.tolist() == [[300.0, 350.0, 400.0]]
    # two ladders, column order is rung order, entry 5 in none
    lad = torch.tensor([[3, 4, 0, 6], [1, 2, -1, -1]])
    t = build_ladders(lad, T)
    assert t.slot.dtype == torch.int32 and t.slot.tolist() == lad.tolist() and t.count.tolist() == [4, 2]
    assert t.rung_of.tolist() == [2, 0, 1, 0, 1, -1, 3] and t.ladder_of.tolist() == [0, 1, 1, 0, 0, 0, 0]
    assert t.direction.tolist() == [0, 1, -1, 1, 0, 0, -1]
    assert t.rung_temperatures.tolist() == [[200.0, 250.0, 300.0, 500.0], [350.0, 400.0, 0.0, 0.0]]
    same = torch.zeros((7, 3), dtype=torch.int64)
    build_ladders(lad, T, same, same.bool())
    with pytest.raises(ValueError, match="two ladders"):
        build_ladders(torch.tensor([[3, 4], [4, 0]]), T)
    with pytest.raises(ValueError, match="strictly increasing"):
        build_ladders(torch.tensor([[0, 1, 3]]), T)
    with pytest.raises(ValueError, match="strictly increasing"):
        build_ladders(torch.tensor([[0, 0 + 1]]), torch.tensor([300.0, 300.0]))   # equal is not increasing
    with pytest.raises(ValueError, match="tail"):
        build_ladders(torch.tensor([[3, -1, 4]]), T)
    with pytest.raises(ValueError, match="fewer than 2"):
        build_ladders(torch.tensor([[3, 4], [0, -1]]), T)
    with pytest.raises(ValueError, match="at least 2 rungs"):
        build_ladders(torch.tensor([[3], [0]]), T)
    with pytest.raises(ValueError, match="batch indices"):
        build_ladders(torch.tensor([[3, 7]]), T)
    with pytest.raises(ValueError, match="> 0"):
        build_ladders(torch.tensor([[0, 1]]), torch.tensor([0.0, 300.0]))
    species = same.clone()
    species[4, 1] = 1
    with pytest.raises(ValueError, match="species differ"):
        build_ladders(lad, T, species)
    build_ladders(torch.tensor([[1, 2], [3, 0]]), T, species)   # entry 4 is in no ladder
    fixed = same.bool()
    fixed[2, 0] = True
    with pytest.raises(ValueError, match="fixed differ"):
        build_ladders(lad, T, same, fixed)


@pytest.mark.parametrize("rs_seed, n", rx.INVARIANCE_RUNS)
def test_one_attempt_leaves_every_rung_canonical(rs_seed, n):
    """L = 4096 ladders of K = 8 rungs, 300 -> 600 K geometric, E ~ Gamma(3) kT of the rung: after one attempt the per-rung
    mean of E / (3 kT) is within 5 standard errors 1 / sqrt(3 L) of 1.  The reference gives |z| of 1.31 and 1.64 for the two parities at
    an acceptance of 0.91; the rule with the sign of arg flipped gives |z| of 20."""
    lad, E = rx.invariance_case(rs_seed)
    z0 = rx.invariance_z(lad.slot, E, lad.rung_kT)
    acc = lad.attempt(n, rx.INVARIANCE_SEED, E)
    z = rx.invariance_z(lad.slot, E, lad.rung_kT)
    rate = acc / lad.attempts.sum()
    print(f"replica exchange reference, attempt {n}: acceptance {rate:.3f}, |z| before {np.abs(z0).max():.2f}, after "
          f"{np.abs(z).max():.2f}  ({np.array2string(z, precision=2)})")
    assert lad.attempts.sum() == rx.INVARIANCE_L * ((rx.INVARIANCE_K - (n & 1)) // 2)
    assert 0.85 < rate < 0.97
    assert np.abs(z0).max() <= 5.0 and np.abs(z).max() <= 5.0
    # the usual mistake is caught by the same gate
    bad, E = rx.invariance_case(rs_seed)
    acc_bad = bad.attempt(n, rx.INVARIANCE_SEED, E, wrong_sign=True)
    z_bad = rx.invariance_z(bad.slot, E, bad.rung_kT)
    print(f"    sign of arg flipped: acceptance {acc_bad / bad.attempts.sum():.3f}, max |z| {np.abs(z_bad).max():.1f}")
    assert np.abs(z_bad).max() > 10.0


def test_occupancy_stays_a_permutation_and_unpaired_rungs_keep_their_entry():
    rs = np.random.RandomState(3)
    slot = np.full((3, 8), -1)
    perm = rs.permutation(16)
    slot[0, :5], slot[1, :2], slot[2, :8] = perm[:5], perm[5:7], perm[7:15]
    kT = np.tile(rx.KB_HARTREE * rx.geometric(250.0, 700.0, 8), (3, 1))
    lad = rx.Ladders(slot, kT, 16, ladder_ids=[7, 2, 9])
    members = [set(slot[l][slot[l] >= 0]) for l in range(3)]
    accepted = 0
    for n in range(12):
        before = lad.slot.copy()
        E = rs.normal(0.0, 3e-3, 16)
        accepted += lad.attempt(n, 11, E)
        for l in range(3):
            row = lad.slot[l]
            assert set(row[row >= 0]) == members[l] and (row[lad.count[l]:] == -1).all()
        m = lad.rung_of >= 0
        assert m.sum() == 15 and not m[perm[15]]
        assert (lad.slot[lad.ladder_of[m], lad.rung_of[m]] == np.nonzero(m)[0]).all()
        # rung 0 at odd n, and the top rung where it has no partner, keep their entry
        if n & 1:
            assert (lad.slot[:, 0] == before[:, 0]).all()
        for l, cnt in enumerate(lad.count):
            if (cnt - (n & 1)) % 2 == 1:
                assert lad.slot[l, cnt - 1] == before[l, cnt - 1]
        # a ladder of two rungs is never paired at odd n
        assert lad.attempts[1, 0] == (n + 2) // 2
    assert 0 < accepted < lad.attempts.sum()
    assert (lad.attempts[0, 4:] == 0).all() and (lad.attempts[1, 1:] == 0).all()


def test_round_trip_counter_on_a_hand_made_sequence():
    """One ladder of three rungs; energies that force the outcome (arg = +-1e6).  Entry 0 climbs from rung 0 to the top and
    comes back: one round trip, counted when it reaches rung 0."""
    kT = [rx.KB_HARTREE * np.array([100.0, 200.0, 400.0])]
    lad = rx.Ladders([[0, 1, 2]], kT, 3)
    big = 1e6 * kT[0][0] * 2.0

    def go(n, accept):
        k = n & 1
        a, b = lad.slot[0, k], lad.slot[0, k + 1]
        E = np.zeros(3)
        E[a], E[b] = (big, 0.0) if accept else (0.0, big)   # the colder rung holds the higher energy: always accepted
        assert lad.attempt(n, 1, E) == int(accept)

    assert lad.direction.tolist() == [1, 0, -1]
    go(0, True)    # (0, 1): entry 0 to rung 1, entry 1 to rung 0
    assert lad.slot.tolist() == [[1, 0, 2]] and lad.direction.tolist() == [1, 1, -1] and lad.round_trips.tolist() == [0, 0, 0]
    go(1, True)    # (1, 2): entry 0 to the top, entry 2 down to rung 1 with direction -1
    assert lad.slot.tolist() == [[1, 2, 0]] and lad.direction.tolist() == [-1, 1, -1]
    go(2, False)   # rejected: nothing moves
    assert lad.slot.tolist() == [[1, 2, 0]] and lad.round_trips.tolist() == [0, 0, 0]
    go(2, True)    # (0, 1): entry 2, which started at the top with direction -1, reaches rung 0: that counts, by the definition
    assert lad.slot.tolist() == [[2, 1, 0]] and lad.round_trips.tolist() == [0, 0, 1] and lad.direction.tolist() == [-1, 1, 1]
    go(3, True)    # (1, 2): entry 0 down to rung 1, entry 1 to the top
    assert lad.slot.tolist() == [[2, 0, 1]] and lad.direction.tolist() == [-1, -1, 1]
    go(4, True)    # (0, 1): entry 0 is back at rung 0: its round trip
    assert lad.slot.tolist() == [[0, 2, 1]] and lad.round_trips.tolist() == [1, 0, 1] and lad.direction.tolist() == [1, -1, 1]
    assert lad.attempts.tolist() == [[4, 2]] and lad.accepts.tolist() == [[3, 2]]
    assert lad.rung_of.tolist() == [0, 2, 1]
