"""Temperature replica exchange (anihip_md_exchange in csrc/md.hip, torchani_amd.md.ReplicaExchangeDynamics) on the MI355X
against the fp64 reference of tests/_md_replica_exchange_ref.py: attempts through the C ABI with the energies given, decision for
decision; the invariance of the canonical law on 4096 ladders; the error returns; the class on ANI-2x and on a standalone
Lennard-Jones potential in lock-step with the reference; and a ladder of Lennard-Jones dimers whose per-rung averages must be
those of the same trajectories without exchange."""
import ctypes as C

import numpy as np
import pytest
import torch

import _md_constraints_ref as cref
import _md_ref as ref
import _md_replica_exchange_ref as rx
from _util import load_golden, seeded_state
from test_gpu_md_device import MASS_BY_INDEX, SEED, _state, _stream

pytestmark = pytest.mark.gpu

ATTEMPT0 = (3 << 32) | 16   # both step words in use; even, so six consecutive attempts cover both parities


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from torchani_amd import _lib

    _lib.lib()
    return torch.device("cuda:0")


class Exchange:
    """anihip_md_exchange on device copies of a reference ``rx.Ladders`` and of v [C, A, 3], active [C, A], kinetic [C]."""

    def __init__(self, dev, lad, v, active, kinetic, seed=SEED, langevin=True, flags=0):
        from torchani_amd import _lib

        self.lib, self._lib = _lib.lib(), _lib
        Cn, A = active.shape
        put = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)   # noqa: E731
        self.slot, self.count, self.rung_of = put(lad.slot, np.int32), put(lad.count, np.int32), put(lad.rung_of, np.int32)
        self.rung_kT = put(lad.rung_kT, np.float32)
        self.ids = put(lad.ladder_ids, np.int64)
        self.attempts, self.accepts = put(lad.attempts, np.int64), put(lad.accepts, np.int64)
        self.direction, self.round_trips = put(lad.direction, np.int8), put(lad.round_trips, np.int32)
        self.scale = torch.full((Cn,), np.nan, dtype=torch.float64, device=dev)   # (nothing may depend on what it held)
        self.v, self.active, self.kinetic = put(v, np.float32), put(active, np.uint8), put(kinetic, np.float64)
        L, K = lad.slot.shape
        self.ladders = _lib.MdLadders(L, K, flags, 0, self.slot.data_ptr(), self.count.data_ptr(), self.rung_of.data_ptr(),
                                      self.rung_kT.data_ptr(), self.ids.data_ptr(), self.attempts.data_ptr(),
                                      self.accepts.data_ptr(), self.direction.data_ptr(), self.round_trips.data_ptr(),
                                      self.scale.data_ptr())
        self.P = _lib.MdParams(Cn, A, _lib.MD_LANGEVIN if langevin else 0, 0, 0.5, seed, 0)

    def attempt(self, n, energies):
        self.P.step = n
        self._E = torch.from_numpy(np.ascontiguousarray(energies, dtype=np.float64)).to(self.v.device)
        self._lib.check(self.lib.anihip_md_exchange(_stream(), C.byref(self.P), C.byref(self.ladders), self._E.data_ptr(),
                                                    self.active.data_ptr(), self.v.data_ptr(), self.kinetic.data_ptr()))

    def tables(self):
        return tuple(t.cpu().numpy() for t in (self.slot, self.rung_of, self.attempts, self.accepts, self.direction,
                                               self.round_trips))


def _tables(lad):
    return lad.slot, lad.rung_of, lad.attempts, lad.accepts, lad.direction, lad.round_trips


def _abi_case(which):
    """(slot [L, K], rung kT [L, K], C, A, ladder ids): three ladders of 5, 2 and 8 rungs in a batch of 16 with one entry in
    no ladder and a shuffled occupancy; or one ladder of two rungs of 300 atoms (two 256-atom chunks per entry)."""
    if which == "three_ladders":
        perm = np.random.RandomState(3).permutation(16)
        slot = np.full((3, 8), -1)
        slot[0, :5], slot[1, :2], slot[2, :8] = perm[:5], perm[5:7], perm[7:15]
        kT = np.tile(ref.KB_HARTREE * rx.geometric(250.0, 700.0, 8), (3, 1))
        return slot, kT, 16, 70, [7, 2, 9]
    return np.array([[1, 0]]), ref.KB_HARTREE * np.array([[300.0, 400.0]]), 2, 300, [4]


@pytest.mark.parametrize("which", ["three_ladders", "two_chunks"])
def test_attempts_match_reference_decision_for_decision(dev, which):
    slot, kT, Cn, A, ids = _abi_case(which)
    _, v, _, _, _, active = _state(Cn, A)
    active = active.astype(np.uint8)
    active[Cn - 1, 2:6] = 2                                    # atoms of constraint clusters are scaled like free ones
    v[active == 0] = np.float32(0.0123)                        # a padding or fixed atom is not touched, whatever it holds
    rs = np.random.RandomState(8)
    kinetic = rs.uniform(0.01, 0.05, Cn)
    energies = rs.uniform(-0.012, 0.012, (6, Cn))              # arg spans about +-3 at the cold end of the ladder
    # the reference alone first: no decision is closer than 1e-6 to its threshold, and both outcomes occur
    dry = rx.Ladders(slot, kT, Cn, ids)
    taken = [dry.attempt(ATTEMPT0 + s, SEED, energies[s]) for s in range(6)]
    assert dry.margin >= 1e-6, dry.margin
    assert 0 < sum(taken) < dry.attempts.sum()
    lad = rx.Ladders(slot, kT, Cn, ids)
    k = Exchange(dev, lad, v, active, kinetic)
    v_ref, ke_ref = v.copy(), kinetic.copy()
    worst_v = worst_ke = 0.0
    for s in range(6):
        rung_before, v_before, ke_before = lad.rung_of.copy(), k.v.cpu().numpy(), k.kinetic.cpu().numpy()
        lad.attempt(ATTEMPT0 + s, SEED, energies[s], ke_ref, v_ref, active)
        k.attempt(ATTEMPT0 + s, energies[s])
        for got, want in zip(k.tables(), _tables(lad)):
            assert got.dtype == want.dtype and np.array_equal(got, want)
        got_v, got_ke = k.v.cpu().numpy(), k.kinetic.cpu().numpy()
        ulp = np.spacing(np.abs(v_ref).astype(np.float32)).astype(np.float64)
        worst_v = max(worst_v, (np.abs(got_v - v_ref) / ulp).max())
        worst_ke = max(worst_ke, np.abs(got_ke / ke_ref - 1.0).max())
        assert (np.abs(got_v - v_ref) <= 2.0 * ulp).all()
        assert np.abs(got_ke / ke_ref - 1.0).max() <= 1e-12
        # everything that was not accepted is bit-identical to before, and so are the atoms that never move
        kept = lad.rung_of == rung_before
        assert np.array_equal(got_v[kept], v_before[kept]) and np.array_equal(got_ke[kept], ke_before[kept])
        assert np.array_equal(got_v[active == 0], v_before[active == 0])
        moved = ~kept
        assert (got_v[moved][active[moved] != 0] != v_before[moved][active[moved] != 0]).any() or not moved.any()
        v_ref, ke_ref = got_v.astype(np.float64), got_ke.copy()   # (the next attempt starts from what the device holds)
    print(f"md replica exchange [{which}]: {sum(taken)} of {lad.attempts.sum()} pairs accepted in 6 attempts, smallest "
          f"|ln u - arg| {dry.margin:.2e}, velocities within {worst_v:.2f} fp32 ulp, kinetic within {worst_ke:.1e}")
    if which == "three_ladders":
        assert (lad.rung_of[np.setdiff1d(np.arange(16), slot[slot >= 0])] == -1).all()
        assert lad.attempts[0, 3] == 3 and lad.attempts[0, 4] == 0      # five rungs: the top one sits the even attempts out


@pytest.mark.parametrize("rs_seed, n", rx.INVARIANCE_RUNS)
def test_one_attempt_leaves_every_rung_canonical_on_the_device(dev, rs_seed, n):
    """The case of tests/test_md_replica_exchange_host.py (L = 4096, K = 8, A = 1): the device takes the reference's decisions
    exactly, and the per-rung mean of E / (3 kT) read back through its slot table stays within 5 standard errors of 1."""
    lad, E = rx.invariance_case(rs_seed)
    Cn = E.shape[0]
    k = Exchange(dev, lad, np.zeros((Cn, 1, 3)), np.ones((Cn, 1), dtype=np.uint8), np.ones(Cn), seed=rx.INVARIANCE_SEED)
    k.ids = None
    k.ladders.ladder_ids = None                                     # (NULL: the ladder's own index)
    accepted = lad.attempt(n, rx.INVARIANCE_SEED, E)
    assert lad.margin >= 1e-9, lad.margin
    k.attempt(n, E)
    slot = k.slot.cpu().numpy()
    z = rx.invariance_z(slot, E, lad.rung_kT)
    print(f"md replica exchange, 4096 ladders x 8 rungs, attempt {n}: {int(k.accepts.sum())} accepted (reference {accepted}), "
          f"max |z| {np.abs(z).max():.2f}")
    assert int(k.accepts.sum()) == accepted and int(k.attempts.sum()) == lad.attempts.sum()
    assert np.array_equal(slot, lad.slot) and np.array_equal(k.rung_of.cpu().numpy(), lad.rung_of)
    assert np.abs(z).max() <= 5.0
    assert np.array_equal(np.sort(slot, axis=None), np.arange(Cn))


def test_error_returns(dev):
    slot, kT, Cn, A, ids = _abi_case("three_ladders")
    v, active, ke, E = np.zeros((Cn, A, 3)), np.ones((Cn, A), dtype=np.uint8), np.ones(Cn), np.zeros(Cn)
    lad = rx.Ladders(slot, kT, Cn, ids)
    k = Exchange(dev, lad, v, active, ke)
    k.ladders.max_rungs = 1
    with pytest.raises(RuntimeError, match="2 rungs"):
        k.attempt(0, E)
    k = Exchange(dev, lad, v, active, ke, langevin=False)
    with pytest.raises(RuntimeError, match="Langevin"):
        k.attempt(0, E)
    k = Exchange(dev, lad, v, active, ke)
    with pytest.raises(RuntimeError, match="2\\^61"):
        k.attempt(1 << 61, E)
    k.attempt((1 << 61) - 1, E)
    # a slot outside -1 .. C - 1, in the lower or the upper rung of a pair of the even attempts: refused where the caller asks
    # for the check and nothing launched; without the check the call returns 0, the pair is not decided or counted, and its
    # member in range keeps rung, velocities and kinetic energy -- its scale is written, whatever scale held before
    v = np.random.RandomState(2).normal(0.0, 0.01, (Cn, A, 3))
    ke = np.random.RandomState(3).uniform(0.01, 0.05, Cn)
    for bad in (Cn, -2):
        for at, other in ((3, 2), (2, 3)):
            k = Exchange(dev, lad, v, active, ke, flags=k._lib.MD_LADDERS_CHECK)
            k.attempt(0, E)
            keeper = int(k.slot[2, other])
            k.slot[2, at] = bad
            before, v_before, ke_before = k.tables(), k.v.clone(), k.kinetic.clone()
            with pytest.raises(RuntimeError, match="slot"):
                k.attempt(2, E)
            assert all(np.array_equal(x, y) for x, y in zip(k.tables(), before))
            assert torch.equal(k.v, v_before) and torch.equal(k.kinetic, ke_before)
            k.ladders.flags = 0
            k.scale.fill_(2.0)
            k.attempt(2, np.where(np.arange(Cn) % 2 == 0, 1.0, -1.0))
            after = k.tables()
            assert np.array_equal(after[0][2, 2:4], before[0][2, 2:4]) and after[1][keeper] == before[1][keeper] == other
            assert after[2][2, 2] == before[2][2, 2] and after[3][2, 2] == before[3][2, 2]
            assert after[2][2, 0] == before[2][2, 0] + 1                    # (the other pairs of the ladder were decided)
            assert float(k.scale[keeper]) == 1.0
            assert torch.equal(k.v[keeper], v_before[keeper]) and torch.equal(k.kinetic[keeper], ke_before[keeper])


# ---- through the class -------------------------------------------------------------------------------------------------------

def _ani_replicas(dev, order=(1, 1, 1, 0, 0, 3)):
    """Molecules of the padded random batch, repeated: a ladder of three of molecule 1 (5 padding atoms), one of two of
    molecule 0, and molecule 3 in no ladder."""
    from torchani_amd.models import ANI2x

    g = load_golden("rand_batch_ani2x")
    order = list(order)
    sp = torch.from_numpy(g["species"].astype(np.int64)[order]).to(dev)
    x = torch.from_numpy(g["coords"][order]).to(dev)
    model = ANI2x(state_dict=seeded_state("ani2x", 8, 7), device=dev, periodic_table_index=False, cutoff_fn=g["cutoff_fn"],
                  row_capacity=256)
    spn = sp.cpu().numpy()
    mass = np.where(spn >= 0, MASS_BY_INDEX[np.clip(spn, 0, 6)], 1.0).astype(np.float32)
    assert (spn < 0).any()
    return model, sp, x, torch.from_numpy(mass).to(dev)


ANI_T = torch.tensor([250.0, 300.0, 360.0, 280.0, 330.0, 500.0], dtype=torch.float64)
ANI_LADDERS = torch.tensor([[0, 1, 2], [3, 4, -1]])


def _lj_replicas(dev, Cn=5):
    """Cn replicas of a cluster of 8 atoms on a cube of 1.15 A in a standalone Lennard-Jones potential."""
    from torchani_amd.potentials import LennardJones

    cube = np.stack(np.meshgrid(np.arange(2), np.arange(2), np.arange(2), indexing="ij"), -1).reshape(-1, 3) * 1.15
    x = torch.from_numpy(np.tile(cube.astype(np.float32), (Cn, 1, 1))).to(dev)
    lj = LennardJones(("H",), eps=(0.002,), sigma=(1.0,)).to(dev)
    return lj, torch.ones((Cn, 8), dtype=torch.int64, device=dev), x, torch.full((Cn, 8), 12.011, device=dev)


def _lock_step(dyn, lad, n_steps, every, overwrite_at=None):
    """``n_steps`` steps of ``dyn`` with the reference ladders ``lad`` taking every attempt on the device's potential
    energies; every table, and ``temperature`` through the rungs, must agree exactly.  Returns the accepted swaps."""
    accepted = 0
    for s in range(n_steps):
        if s == overwrite_at:   # the user's write is read by the next attempt
            dyn.rung_temperatures.mul_(1.125)
        t_before = dyn.temperature.cpu().numpy()
        dyn.step()
        if (s + 1) % every:
            assert np.array_equal(dyn.temperature.cpu().numpy(), t_before)
            continue
        n = (s + 1) // every - 1
        assert dyn.attempts_done == n + 1
        rung_t = dyn.rung_temperatures.cpu()
        lad.rung_kT = torch.mul(rung_t, ref.KB_HARTREE).double().numpy()   # (the fp32 product the attempt formed)
        accepted += lad.attempt(n, dyn.seed, dyn.potential_energies.cpu().numpy())
        assert lad.margin >= 1e-6, lad.margin
        got = (dyn.replicas_at_rungs(), dyn.rungs(), dyn.exchange_attempts, dyn.exchange_accepts, dyn._direction, dyn.round_trips())
        for g, want in zip(got, _tables(lad)):
            assert np.array_equal(g.cpu().numpy(), want)
        assert np.array_equal(dyn.temperature.cpu().numpy(), lad.temperatures(t_before, rung_t.numpy()))
        rates = dyn.acceptance_rates().cpu().numpy()
        assert np.array_equal(rates, lad.accepts / np.maximum(lad.attempts, 1))
        # the kinetic energies held are those of the rescaled velocities
        v2 = (dyn.velocities.double() ** 2).sum(dim=-1)
        ke = 0.5 * (dyn.masses.double() * (dyn._active != 0) * v2).sum(dim=1).cpu().numpy() / ref.ACC_UNIT
        assert np.abs(dyn.kinetic_energies().cpu().numpy() / ke - 1.0).max() <= 1e-6
        by = dyn.by_rung(dyn.potential_energies).cpu().numpy()
        assert np.array_equal(by[lad.slot >= 0], dyn.potential_energies.cpu().numpy()[lad.slot[lad.slot >= 0]])
        assert (by[lad.slot < 0] == 0.0).all()
    return accepted


def test_class_on_ani2x_in_lock_step_with_reference(dev):
    from torchani_amd.md import ReplicaExchangeDynamics

    model, sp, x, mass = _ani_replicas(dev)
    fixed = torch.zeros(sp.shape, dtype=torch.bool)
    fixed[:3, 1] = True                                           # the same atom in every replica of the first ladder
    dyn = ReplicaExchangeDynamics(model, sp, x, dt=0.5, masses=mass, temperature=ANI_T, friction=0.05, fixed=fixed.to(dev),
                                  ladders=ANI_LADDERS, exchange_every=2, ladder_ids=torch.tensor([9, 4]), seed=SEED,
                                  replica_ids=torch.tensor([3, 8, 5, 7, 4, 6]))
    assert dyn.n_ladders == 2 and dyn.max_rungs == 3 and dyn.rungs().tolist() == [0, 1, 2, 0, 1, -1]
    dyn.set_temperature(ANI_T)
    lad = rx.Ladders(ANI_LADDERS.numpy(), ref.KB_HARTREE * dyn.rung_temperatures.cpu().numpy(), 6, [9, 4])
    accepted = _lock_step(dyn, lad, 6, 2, overwrite_at=3)
    assert dyn.steps_done == 6 and dyn.attempts_done == 3
    assert float(dyn.temperature[5]) == 500.0                      # in no ladder: never rewritten
    assert dyn.exchange_attempts.tolist() == [[2, 1], [2, 0]]
    print(f"md replica exchange, ANI-2x x 8: {accepted} of 5 pairs accepted in 3 attempts")


def test_class_on_lennard_jones_in_lock_step_with_reference(dev):
    from torchani_amd.md import ReplicaExchangeDynamics, temperature_ladder

    lj, sp, x, mass = _lj_replicas(dev)
    T = temperature_ladder(60.0, 240.0, 5)
    dyn = ReplicaExchangeDynamics(lj, sp, x, dt=1.0, masses=mass, temperature=T, friction=0.02, exchange_every=2, seed=7)
    dyn.set_temperature(T)
    lad = rx.Ladders(np.arange(5)[None], ref.KB_HARTREE * dyn.rung_temperatures.cpu().numpy(), 5)
    accepted = _lock_step(dyn, lad, 6, 2, overwrite_at=3)
    assert dyn.exchange_attempts.tolist() == [[2, 1, 2, 1]]
    print(f"md replica exchange, Lennard-Jones cluster x 5: {accepted} of 6 pairs accepted in 3 attempts")


def test_step_and_observables_do_not_synchronize(dev):
    from torchani_amd.md import ReplicaExchangeDynamics

    model, sp, x, mass = _ani_replicas(dev)
    dyn = ReplicaExchangeDynamics(model, sp, x, masses=mass, temperature=ANI_T, ladders=ANI_LADDERS, exchange_every=1, seed=1)
    dyn.set_temperature(ANI_T)
    for _ in range(3):   # (the third evaluation captures the automatic HIP graph)
        dyn.step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(4):
            dyn.step()
        dyn.rungs(), dyn.replicas_at_rungs(), dyn.acceptance_rates(), dyn.round_trips(), dyn.by_rung(dyn.potential_energies)
        dyn.by_rung(dyn.velocities), dyn.exchange_attempts.sum(), dyn.exchange_accepts.sum(), dyn.kinetic_energies()
        dyn.temperatures()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert dyn.steps_done == 7 and dyn.attempts_done == 7
    assert dyn.exchange_attempts.tolist() == [[4, 3], [4, 0]]
    assert tuple(dyn.by_rung(dyn.velocities).shape) == (2, 3, 14, 3)


def test_exchange_every_zero_is_bit_identical_to_batched_dynamics(dev):
    """Ten steps with exchange_every=0 against BatchedDynamics: the same bits in coordinates (both floats), velocities and
    kinetic energies, on the standalone Lennard-Jones potential and on ANI-2x x 8.  ANI-2x runs with deterministic_forces
    (force sums in 64-bit fixed point): its default float atomics add in an order that varies from run to run, and two runs
    of anything would differ by that."""
    from torchani_amd.md import BatchedDynamics, ReplicaExchangeDynamics

    for case, ladders in ((_lj_replicas, None), (_ani_replicas, ANI_LADDERS)):
        model, sp, x, mass = case(dev)
        if ladders is not None:
            model.deterministic_forces = True   # (the Lennard-Jones forces are the same bits in every run as they are)
        T = ANI_T if ladders is not None else torch.linspace(60.0, 240.0, sp.shape[0], dtype=torch.float64)
        kw = dict(dt=0.5, masses=mass, temperature=T, friction=0.05, seed=SEED)
        a = ReplicaExchangeDynamics(model, sp, x, ladders=ladders, exchange_every=0, **kw)
        b = BatchedDynamics(model, sp, x, **kw)
        for d in (a, b):
            d.set_temperature(T)
            d.run(10)
        assert a.steps_done == 10 and a.attempts_done == 0 and int(a.exchange_attempts.sum()) == 0
        assert torch.equal(a.temperature, b.temperature) and a.rungs().tolist() == build_rungs(ladders, sp.shape[0])
        dx = (a.coordinates - b.coordinates).abs().max().item()
        dv = (a.velocities - b.velocities).abs().max().item()
        print(f"md replica exchange, exchange_every=0 on {type(model).__name__}: max |dx| {dx:.1e} A, max |dv| {dv:.1e} A/fs "
              "against BatchedDynamics after 10 steps")
        assert torch.equal(a.coordinates, b.coordinates) and torch.equal(a.coordinates_lo, b.coordinates_lo)
        assert torch.equal(a.velocities, b.velocities) and torch.equal(a.kinetic_energies(), b.kinetic_energies())
        assert torch.equal(a.potential_energies, b.potential_energies)


def build_rungs(ladders, n):
    """The rungs that the ladders start with: column order, -1 outside every ladder."""
    if ladders is None:
        return list(range(n))
    out = [-1] * n
    for row in ladders.tolist():
        for k, c in enumerate(row):
            if c >= 0:
                out[c] = k
    return out


def test_constrained_velocities_stay_tangent_after_a_swap(dev):
    """X-H bonds held by RATTLE: an accepted swap scales the velocities of an entry uniformly, so the residuals r_hat . dv stay
    under the gate of tests/test_gpu_md_constraints.py (4 fp32 ulp of the cluster's largest |v|) without a projection."""
    from torchani_amd.md import ReplicaExchangeDynamics, hydrogen_constraints

    model, sp, x, mass = _ani_replicas(dev)
    bc = hydrogen_constraints(sp, x, hydrogen=0, oxygen=3)
    assert int(bc.counts().sum()) > 0
    dyn = ReplicaExchangeDynamics(model, sp, x, dt=0.5, masses=mass, temperature=ANI_T, friction=0.05, ladders=ANI_LADDERS,
                                  exchange_every=1, seed=SEED, constraints=bc, constraint_tolerance=1e-8)
    dyn.set_temperature(ANI_T)
    active = sp.cpu().numpy() >= 0
    cons = cref.Constraints(bc.pairs.numpy(), bc.lengths.numpy(), active, mass.double().cpu().numpy())
    swaps, worst = 0, 0.0
    for _ in range(6):
        before = int(dyn.exchange_accepts.sum())
        dyn.step()
        if int(dyn.exchange_accepts.sum()) == before:
            continue
        swaps += 1
        pair = dyn.coordinates.double().cpu().numpy() + dyn.coordinates_lo.double().cpu().numpy()
        for rv, vmax in cref.velocity_residuals(pair, dyn.velocities.double().cpu().numpy(), cons):
            ulp = np.spacing(vmax.astype(np.float32)).astype(np.float64)
            worst = max(worst, (rv / ulp[:, None]).max())
            assert (rv <= 4.0 * ulp[:, None]).all()
    print(f"md replica exchange with X-H constraints: {swaps} of 6 attempts swapped, velocity residual {worst:.2f} fp32 ulp (gate 4)")
    assert swaps > 0
    dyn.raise_on_unconverged_constraints()


def test_a_ladder_follows_the_same_trajectory_elsewhere_in_the_batch(dev):
    """The two ladders with their places in the batch swapped, each keeping its ladder id and its replica ids: the same
    decisions, and the same bits in coordinates, velocities and kinetic energies.  The model runs with deterministic_forces:
    a force is then an integer sum of its pair terms, exact in any order, and a pair term is a function of the molecule's own
    atoms alone, so the exchange and the integrator are compared with nothing in between."""
    from torchani_amd.md import ReplicaExchangeDynamics

    T2 = torch.cat([ANI_T[3:5], ANI_T[:3], ANI_T[5:]])
    runs = []
    for order, T, ladders, lids, rids in (((1, 1, 1, 0, 0, 3), ANI_T, ANI_LADDERS, [9, 4], [3, 8, 5, 7, 4, 6]),
                                          ((0, 0, 1, 1, 1, 3), T2, torch.tensor([[0, 1, -1], [2, 3, 4]]), [4, 9], [7, 4, 3, 8, 5, 6])):
        model, sp, x, mass = _ani_replicas(dev, order)
        model.deterministic_forces = True
        dyn = ReplicaExchangeDynamics(model, sp, x, dt=0.5, masses=mass, temperature=T, friction=0.05, ladders=ladders,
                                      exchange_every=1, ladder_ids=torch.tensor(lids), seed=SEED, replica_ids=torch.tensor(rids))
        dyn.set_temperature(T)
        dyn.run(6)
        runs.append(dyn)
    a, b = runs
    here, there = [0, 1, 2, 3, 4, 5], [2, 3, 4, 0, 1, 5]
    assert a.rungs().tolist() == b.rungs()[there].tolist()
    assert a.exchange_accepts.tolist() == b.exchange_accepts.flip(0).tolist() and int(a.exchange_accepts.sum()) > 0
    assert a.round_trips().tolist() == b.round_trips()[there].tolist()
    assert torch.equal(a.temperature[here], b.temperature[there])
    dx = (a.coordinates - b.coordinates[there]).abs().max().item()
    dv = (a.velocities - b.velocities[there]).abs().max().item()
    print(f"md replica exchange, ladders at swapped places: max |dx| {dx:.1e} A, max |dv| {dv:.1e} A/fs after 6 steps")
    assert torch.equal(a.coordinates, b.coordinates[there]) and torch.equal(a.coordinates_lo, b.coordinates_lo[there])
    assert torch.equal(a.velocities, b.velocities[there]) and torch.equal(a.kinetic_energies(), b.kinetic_energies()[there])


# ---- sampling ----------------------------------------------------------------------------------------------------------------

# (Rungs 30 -> 120 K were tried first: at 120 K, a fifth of the well depth of 632 K, dimers came apart within the 8 ps, with and
# without exchange -- bonds of 7 A -- and an unbound pair in vacuum has no stationary law to compare.  The top rung is 60 K, and
# the bottom one 15 K, which keeps the ladder ratio of 4 and the spacing of 1.59 between neighbors that 30 -> 120 K had.)
DIMER = dict(ladders=64, rungs=4, t_min=15.0, t_max=60.0, dt=2.0, friction=0.05, steps=4000, every=20)


def _dimer_run(dev, every):
    """64 ladders x 4 rungs of a Lennard-Jones dimer (eps 0.002 Ha, sigma 1 A, bond at 2^(1/6) A); returns the per-ladder
    averages over the second half of the run of the potential energy and the kinetic temperature by rung [L, K], the
    acceptance rates, and the largest bond length met."""
    from torchani_amd.md import ReplicaExchangeDynamics, temperature_ladder
    from torchani_amd.potentials import LennardJones

    L, K = DIMER["ladders"], DIMER["rungs"]
    lj = LennardJones(("H",), eps=(0.002,), sigma=(1.0,)).to(dev)
    x = torch.zeros((L * K, 2, 3), device=dev)
    x[:, 1, 0] = 2.0 ** (1.0 / 6.0)
    T = temperature_ladder(DIMER["t_min"], DIMER["t_max"], K).repeat(L)
    dyn = ReplicaExchangeDynamics(lj, torch.ones((L * K, 2), dtype=torch.int64, device=dev), x, dt=DIMER["dt"],
                                  masses=torch.full((L * K, 2), 12.011, device=dev), temperature=T, friction=DIMER["friction"],
                                  ladders=torch.arange(L * K).view(L, K), exchange_every=every, seed=11, remove_drift=False)
    dyn.set_temperature(T)
    pe = torch.zeros((L, K), dtype=torch.float64, device=dev)
    tk = torch.zeros((L, K), dtype=torch.float64, device=dev)
    far = torch.zeros((), device=dev)
    half = DIMER["steps"] // 2
    for s in range(DIMER["steps"]):
        dyn.step()
        if s >= half:
            pe += dyn.by_rung(dyn.potential_energies)
            tk += dyn.by_rung(dyn.temperatures())
            far = torch.maximum(far, (dyn.coordinates[:, 1] - dyn.coordinates[:, 0]).norm(dim=-1).max())
    dyn.raise_on_overflow()
    return (pe / half).cpu().numpy(), (tk / half).cpu().numpy(), dyn.acceptance_rates().cpu().numpy(), float(far), dyn


def test_exchange_leaves_the_sampling_of_every_rung_unchanged(dev):
    """The yardstick is the code path without exchange: the same 256 trajectories at fixed temperatures.  Per rung, the mean
    potential energy agrees within 5 combined standard errors (from the 64 per-ladder averages of each run), the kinetic
    temperature agrees with the rung temperature within 5 standard errors, and the acceptance rate of every pair of rungs of
    every ladder (192 pairs of 100 attempts each) lies strictly between 0 and 1.

    Measured: <PE> by rung -1.976, -1.959, -1.930, -1.879 mHa with exchange against -1.975, -1.959, -1.934, -1.872 without (z =
    -2.17, 0.05, 2.32, -1.13); kinetic T 14.98, 23.85, 37.71, 60.09 K (z = -0.33, 0.43, -0.54, 0.33); acceptance by pair 0.850,
    0.840, 0.826, of a single pair of a single ladder 0.72 to 0.92; 3947 round trips; longest bond 1.65 A."""
    pe_x, tk_x, rates, far_x, dyn = _dimer_run(dev, DIMER["every"])
    pe_0, tk_0, _, far_0, _ = _dimer_run(dev, 0)
    L, K = pe_x.shape
    T = rx.geometric(DIMER["t_min"], DIMER["t_max"], K)
    se = lambda a: a.std(axis=0, ddof=1) / np.sqrt(L)   # noqa: E731
    z_pe = (pe_x.mean(axis=0) - pe_0.mean(axis=0)) / np.sqrt(se(pe_x) ** 2 + se(pe_0) ** 2)
    z_tx, z_t0 = (tk_x.mean(axis=0) - T) / se(tk_x), (tk_0.mean(axis=0) - T) / se(tk_0)
    trips = int(dyn.round_trips().sum())
    print(f"md replica exchange, LJ dimer, {L} ladders x {K} rungs {np.array2string(T, precision=1)} K, {DIMER['steps']} x "
          f"{DIMER['dt']} fs, exchange every {DIMER['every']}:")
    print(f"    <PE> by rung with exchange {np.array2string(pe_x.mean(axis=0), precision=6)} Ha")
    print(f"    <PE> by rung without       {np.array2string(pe_0.mean(axis=0), precision=6)} Ha, z = {np.array2string(z_pe, precision=2)}")
    print(f"    kinetic T by rung with exchange {np.array2string(tk_x.mean(axis=0), precision=2)} K, z = {np.array2string(z_tx, precision=2)}"
          f"; without, z = {np.array2string(z_t0, precision=2)}")
    print(f"    acceptance by pair {np.array2string(rates.mean(axis=0), precision=3)} (min {rates.min():.3f}, max {rates.max():.3f}), "
          f"{trips} round trips, longest bond {far_x:.2f} A (without exchange {far_0:.2f} A)")
    assert far_x < 2.5 and far_0 < 2.5, "a dimer came apart: the ensemble of the rung is no longer the bound one"
    assert np.abs(z_pe).max() <= 5.0
    assert np.abs(z_tx).max() <= 5.0 and np.abs(z_t0).max() <= 5.0
    assert rates.shape == (L, K - 1) and (rates > 0.0).all() and (rates < 1.0).all()
    assert int(dyn.exchange_attempts.sum()) == L * (DIMER["steps"] // DIMER["every"] // 2) * 3
