"""Biased MD (csrc/md_bias.hip, torchani_amd.md.BatchedDynamics(bias=...)) on the MI355X against the fp64 reference of
tests/_md_bias_ref.py: collective variables, restraints and the force sum through the C ABI, the hills kernels at counts around
the chunk size, the deposit with its capacity rule, the error returns, and the class in lock-step with the reference on ANI-2x
and Lennard-Jones, without host synchronization, bit-identical without a bias, under replica exchange, and sampling a restrained
dimer and a free energy by multiple-walker well-tempered metadynamics.

Gates, derived and not measured: CV values 1e-12 (fp64 arithmetic of a dozen operations on numbers of order 10); energies
1e-11 of the sum of the absolute terms (summation order and the rounding of exp at these counts); forces one fp32 ulp of the
reference value (the kernel and the reference round the same fp64 sum, which differs by fp64 rounding alone)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _md_bias_ref as br
import _md_ref as ref
import _md_replica_exchange_ref as rx
from test_gpu_md_device import SEED, _state, _stream
from test_gpu_md_replica_exchange import _ani_replicas, _lj_replicas

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
GUARD = 16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from torchani_amd import _lib

    _lib.lib()
    return torch.device("cuda:0")


class Abi:
    """The C ABI on the tables of ``build_bias_tables``: device copies, hill buffers of ``capacity`` filled with a sentinel and
    followed by guard elements, and the outputs."""

    def __init__(self, dev, tables, Cn, A, capacity=None, **broken):
        from torchani_amd import _lib

        self.lib, self._lib, self.dev, self.Cn, self.A = _lib.lib(), _lib, dev, Cn, A
        t = tables._asdict()
        t.update(broken)   # (a test of the error returns swaps a table for a broken one)
        self.names = ("cv_offset", "kind", "atoms", "restraint", "meta_cv", "inv_sigma2", "height", "list", "rank_in_list",
                      "members", "list_entry", "bias_factor")
        self.t = {k: torch.as_tensor(t[k]).to(dev).contiguous() for k in self.names}
        G = int(t["members"].numel())
        self.G, self.cap = G, int(tables.capacity if capacity is None else capacity) if G else 0
        cap = self.cap
        self.centers_buf = torch.full((G * 2 * cap + GUARD,), SENTINEL, dtype=torch.float64, device=dev)
        self.heights_buf = torch.full((G * cap + GUARD,), SENTINEL, dtype=torch.float64, device=dev)
        self.centers = self.centers_buf[:G * 2 * cap].view(G, 2, cap)
        self.heights = self.heights_buf[:G * cap].view(G, cap)
        n0 = tables.heights.shape[1]
        if G and n0:
            self.centers[:, :, :n0], self.heights[:, :n0] = tables.centers.to(dev), tables.heights.to(dev)
        self.used = torch.as_tensor(t["used"]).to(dev).to(torch.int32).contiguous()
        self.dropped = torch.zeros(G, dtype=torch.int32, device=dev)
        self.status = torch.full((Cn,), -1, dtype=torch.int32, device=dev)
        ncv = int(self.t["kind"].numel())
        self.cv_values = torch.full((max(1, ncv),), SENTINEL, dtype=torch.float64, device=dev)
        self.e_bias = torch.full((Cn,), SENTINEL, dtype=torch.float64, device=dev)
        self.e_meta = torch.full((Cn,), SENTINEL, dtype=torch.float64, device=dev)
        ptr = lambda x: x.data_ptr() if x.numel() else None   # noqa: E731
        self.b = _lib.MdBias(ncv, G, cap, 0, 0, Cn, *(ptr(self.t[k]) for k in self.names), ptr(self.used), ptr(self.dropped),
                             ptr(self.centers_buf), ptr(self.heights_buf), self.status.data_ptr())
        self.P = _lib.MdParams(Cn, A, 0, 0, 1.0, 0, 0)
        self.ws = torch.empty(max(8, self.lib.anihip_md_bias_workspace_bytes(C.byref(self.P), C.byref(self.b))), dtype=torch.uint8,
                              device=dev)

    def set_x(self, x64):
        """Two-float coordinates of the fp64 positions."""
        hi = x64.astype(np.float32)
        self.x = torch.from_numpy(hi).to(self.dev)
        self.lo = torch.from_numpy((x64 - hi.astype(np.float64)).astype(np.float32)).to(self.dev)
        return self.x.double().cpu().numpy() + self.lo.double().cpu().numpy()   # what the kernels read, exactly

    def apply(self, forces, bound=0):
        self.f = torch.from_numpy(np.ascontiguousarray(forces, dtype=np.float32)).to(self.dev)
        self.b.hills_bound = bound
        rc = self.lib.anihip_md_bias_apply(_stream(), C.byref(self.P), C.byref(self.b), self.x.data_ptr(), self.lo.data_ptr(),
                                           self.f.data_ptr(), self.e_bias.data_ptr(), self.e_meta.data_ptr(),
                                           self.cv_values.data_ptr(), self.ws.data_ptr(), self.ws.numel())
        self._lib.check(rc)
        return {"forces": self.f.cpu().numpy(), "cv_values": self.cv_values.cpu().numpy(), "bias_energies": self.e_bias.cpu().numpy(),
                "meta_energies": self.e_meta.cpu().numpy(), "status": self.status.cpu().numpy()}

    def deposit(self, kT):
        self.kT = None if kT is None else torch.from_numpy(np.asarray(kT, dtype=np.float32)).to(self.dev)
        self._lib.check(self.lib.anihip_md_bias_deposit(
            _stream(), C.byref(self.P), C.byref(self.b), None if kT is None else self.kT.data_ptr(), self.cv_values.data_ptr(),
            self.e_meta.data_ptr()))

    def hills(self, g, values):
        v = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)).to(self.dev)
        out_v = torch.full((v.shape[0],), SENTINEL, dtype=torch.float64, device=self.dev)
        out_d = torch.full((v.shape[0], 2), SENTINEL, dtype=torch.float64, device=self.dev)
        self._lib.check(self.lib.anihip_md_bias_hills(_stream(), C.byref(self.b), g, v.shape[0], v.data_ptr(), out_v.data_ptr(),
                                                      out_d.data_ptr()))
        return out_v.cpu().numpy(), out_d.cpu().numpy()

    def guards_untouched(self):
        return bool((self.centers_buf[self.G * 2 * self.cap:] == SENTINEL).all()) and bool(
            (self.heights_buf[self.G * self.cap:] == SENTINEL).all())


def _compare(got, want, what):
    """The gates of the module docstring; prints every figure before it asserts."""
    dcv = np.abs(got["cv_values"][:want["cv_values"].size] - want["cv_values"]).max() if want["cv_values"].size else 0.0
    scale = want["energy_scale"]
    de = np.abs(got["bias_energies"] - want["bias_energies"])
    dm = np.abs(got["meta_energies"] - want["meta_energies"])
    ulp = br.ulp32(want["forces"])
    df = np.abs(got["forces"].astype(np.float64) - want["forces"].astype(np.float64))
    worst = (df / ulp).max()
    moved = np.abs(want["bias_forces"]).sum(axis=-1) > 0
    print(f"md bias, {what}: max |d cv| {dcv:.1e}, max |dE| / sum|terms| {np.max(de / np.maximum(scale, 1e-300)):.1e}, forces "
          f"within {worst:.2f} fp32 ulp on {int(moved.sum())} biased atoms (largest bias force "
          f"{np.abs(want['bias_forces']).max():.2e} Ha/A)")
    assert dcv <= 1e-12
    assert (de <= 1e-11 * scale).all() and (dm <= 1e-11 * scale).all()
    assert (df <= ulp).all()
    return moved


# ---- CVs, restraints and forces through the C ABI -----------------------------------------------------------------------------

def _special_positions(origin):
    """Thirteen atoms with constructed geometry, fp32-exact where it matters: two dihedrals within 0.05 rad of +-pi on either
    side, angles of 25, 60, 110, 155 and 175 degrees at one vertex, and a distance of exactly 5 (3-4-5)."""
    p = np.zeros((13, 3))
    # dihedral A (atoms 0-3) and B (atoms 0, 1, 2, 4): the fourth atom at +-(pi - 0.03) about the axis 1-2
    p[0], p[1], p[2] = (-0.5, 1.0, 0.0), (0.0, 0.0, 0.0), (1.5, 0.0, 0.0)
    for a, phi in ((3, math.pi - 0.03), (4, -math.pi + 0.03)):
        p[a] = (2.0, math.cos(phi), math.sin(phi))
    # angles at atom 5 between atom 6 and atoms 7 .. 11
    p[5], p[6] = (4.0, 4.0, 1.0), (5.2, 4.0, 1.0)
    for a, deg in zip(range(7, 12), (25.0, 60.0, 110.0, 155.0, 175.0)):
        t = math.radians(deg)
        p[a] = p[5] + 1.1 * np.array([math.cos(t), math.sin(t), 0.0])
    p[12] = p[5] + np.array([3.0, 4.0, 0.0])   # |5 - 12| = 5 exactly
    return p + origin


def _cv_case(Cn, A, perm=None):
    """Species, fp64 positions and the bias of the CV / restraint / force tests on the ``_state`` batches; ``perm`` puts entry
    perm[c] of the unpermuted case at batch position c."""
    from torchani_amd import md

    x, _, f0, _, _, _ = _state(Cn, A)
    species = np.zeros((Cn, A), dtype=np.int64)
    species[Cn // 2, A - 9:] = -1   # the padding of _state
    rs = np.random.RandomState(21)
    lo = rs.uniform(-1e-7, 1e-7, x.shape)   # a second float on every coordinate
    base = A - 13 - 31 if A > 256 else 20   # A = 300: atoms 256 .. 268, and CVs below straddle atom 256
    special = _special_positions(np.array([8.0, -3.0, 2.0]))
    x[0, base:base + 13] = special.astype(np.float32)
    lo[0, base:base + 13] = 0.0
    x = x + lo
    perm = list(range(Cn)) if perm is None else list(perm)
    inv = {old: new for new, old in enumerate(perm)}

    def only(entries):
        """An index tensor that is ``entries[old]`` at the position of old entry ``old`` and -1 elsewhere."""
        t = torch.full((Cn,), -1, dtype=torch.int64)
        for old, i in entries.items():
            t[inv[old]] = i
        return t

    def values(by_old, default=0.0):
        t = torch.full((Cn,), default, dtype=torch.float64)
        for old, v in by_old.items():
            t[inv[old]] = v
        return t

    e0 = lambda i: only({0: base + i})   # noqa: E731  (an atom of the constructed group of entry 0)
    at0 = lambda i: only({0: i})   # noqa: E731
    two = lambda a, b: {0: a, 1: b} if Cn > 2 else {0: a}   # noqa: E731  (with C = 2 the other entry has no CV at all)
    dih_a = md.dihedral(e0(0), e0(1), e0(2), e0(3))
    dih_b = md.dihedral(e0(0), e0(1), e0(2), e0(4))
    s_a, s_b = br.cv(2, special[[0, 1, 2, 3]])[0], br.cv(2, special[[0, 1, 2, 4]])[0]
    assert min(s_a, s_b) < -math.pi + 0.05 and max(s_a, s_b) > math.pi - 0.05
    bias = [
        # the centre across the seam from the value: the restraint wraps
        md.Restraint(dih_a, values({0: -s_a + math.copysign(0.01, s_a)}), 0.3),
        md.Restraint(dih_b, values({0: s_b}), 0.2, 0.01),
    ]
    bias += [md.Restraint(md.angle(e0(6), e0(5), e0(a)), 1.7, 0.05) for a in range(7, 12)]
    # |5 - 12| = 5: inside the flat bottom, exactly on its edge, outside
    bias += [md.Restraint(md.distance(e0(5), e0(12)), c, 0.04, 0.5) for c in (5.2, 4.5, 4.0)]
    # six more on random atoms of entry 0 (16 in all), the first three also in entry 1 with centres of their own; atom 3 is
    # shared by four of them, and for A = 300 their atoms lie on both sides of atom 256
    far = 260 if A > 256 else 50
    bias += [
        md.Restraint(md.distance(only(two(3, 4)), only(two(far, 30))), values(two(25.0, 31.0)), 0.002),
        md.Restraint(md.angle(only(two(3, 2)), only(two(255 if A > 256 else 9, 17)), only(two(far + 1, 40))),
                     values(two(1.2, 2.0)), 0.05, values(two(0.1, 0.0))),
        md.Restraint(md.dihedral(only(two(3, 0)), only(two(11, 1)), only(two(far + 2, 2)), only(two(7, 3))),
                     values(two(0.5, -2.0)), 0.03),
        md.Restraint(md.distance(at0(3), e0(12)), 14.0, 0.001),
        md.Restraint(md.angle(at0(1), at0(far + 3), at0(2)), 0.4, 0.02),
        md.Restraint(md.dihedral(at0(14), at0(far + 4), at0(far + 5), at0(15)), 3.0, 0.01),
    ]
    # 40 hills on the two seam dihedrals of entry 0, their centres on the far side of the seam from the values
    n0 = 40
    centers = np.stack([br.wrap(rs.uniform(-0.3, 0.3, n0) - s_a), br.wrap(rs.uniform(-0.3, 0.3, n0) - s_b)])[None]
    heights = rs.uniform(0.5e-3, 2e-3, (1, n0))
    meta = md.Metadynamics([dih_a, dih_b], (0.2, 0.25), 1e-3, 1, walkers=only({0: 7}), max_hills=64,
                           hills=(torch.from_numpy(centers), torch.from_numpy(heights)))
    return species[perm], x[perm], f0[perm], bias + [meta]


@pytest.mark.parametrize("Cn,A", [(3, 70), (2, 300)])
def test_cvs_restraints_and_forces_match_reference(dev, Cn, A):
    from torchani_amd import md

    species, x, f0, bias = _cv_case(Cn, A)
    tables = md.build_bias_tables(torch.from_numpy(species), None, bias)
    counts = np.diff(tables.cv_offset.numpy())
    assert counts[0] == 16 and counts[-1] == 0 and (Cn == 2 or counts[1] == 3)
    if A > 256:   # CVs whose atoms lie on both sides of atom 256
        at = tables.atoms.numpy() % A
        assert ((np.where(at >= 0, at, A).min(axis=1) < 256) & (at.max(axis=1) >= 256)).sum() >= 4
    k = Abi(dev, tables, Cn, A)
    xk = k.set_x(x)
    assert np.abs(xk - x).max() <= 1e-12
    model = br.Bias(tables)
    want = model.apply(xk, f0.astype(np.float32))
    # what the case promises: angles in 20 .. 160 degrees and one at 175, both sides of the seam, the three flat-bottom regimes
    kinds, vals = tables.kind.numpy()[:16], want["cv_values"][:16]
    ang = np.degrees(vals[kinds == br.ANGLE])
    assert ((ang > 20.0) & (ang < 160.0)).sum() >= 4 and np.abs(ang - 175.0).min() < 1e-3
    dih = vals[kinds == br.DIHEDRAL]
    assert (dih > math.pi - 0.05).any() and (dih < -math.pi + 0.05).any()
    five = [r for r in range(16) if kinds[r] == br.DISTANCE and vals[r] == 5.0]
    assert len(five) == 3
    e = [br.restraint(br.DISTANCE, 5.0, *tables.restraint.numpy()[r]) for r in five]
    assert e[0] == (0.0, 0.0) and e[1] == (0.0, 0.0) and e[2][0] > 0.0
    assert np.isfinite(want["bias_forces"]).all() and want["meta_energies"][0] > 1e-4
    for f_in, what in ((f0, "random incoming forces"), (np.zeros_like(f0), "zero incoming forces")):
        want = model.apply(xk, f_in.astype(np.float32))
        got = k.apply(f_in)
        assert (got["status"] == 0).all()
        moved = _compare(got, want, f"C = {Cn}, A = {A}, {what}")
        # atoms of no CV keep their bits; entries without a CV report zero energies
        assert np.array_equal(got["forces"][~moved], f_in.astype(np.float32)[~moved])
        assert got["bias_energies"][-1] == 0.0 and got["meta_energies"][-1] == 0.0
        again = k.apply(f_in)
        for key in got:
            assert np.array_equal(got[key], again[key]), key
    assert k.guards_untouched()


def test_an_entry_gives_the_same_bits_elsewhere_in_the_batch(dev):
    from torchani_amd import md

    Cn, A = 3, 70
    out = {}
    for perm in ((0, 1, 2), (2, 0, 1)):
        species, x, f0, bias = _cv_case(Cn, A, perm)
        tables = md.build_bias_tables(torch.from_numpy(species), None, bias)
        k = Abi(dev, tables, Cn, A)
        k.set_x(x)
        got = k.apply(f0)
        off = tables.cv_offset.numpy()
        out[perm] = {old: (got["forces"][new], got["bias_energies"][new], got["meta_energies"][new],
                           got["cv_values"][off[new]:off[new + 1]]) for new, old in enumerate(perm)}
    for old in range(Cn):
        for a, b in zip(out[(0, 1, 2)][old], out[(2, 0, 1)][old]):
            assert np.array_equal(a, b)


# ---- hills ----------------------------------------------------------------------------------------------------------------------

def _hills_case(n_cv, capacity, counts):
    """Eight entries of six atoms: list 10 shared by the entries 0 and 2 (not adjacent), private lists 11 .. 15, entry 3 without
    metadynamics.  A dihedral (periodic) and, with two CVs, a distance; random hills within a few sigma of the walkers."""
    from torchani_amd import md

    Cn, A = 8, 6
    rs = np.random.RandomState(31 + n_cv)
    x = rs.uniform(-2.0, 2.0, (Cn, A, 3)).astype(np.float32).astype(np.float64)
    walkers = torch.tensor([10, 11, 10, -1, 12, 13, 14, 15])
    cvs = [md.dihedral(0, 1, 2, 3), md.distance(4, 5)][:n_cv]
    sig = (0.4, 0.3)[:n_cv]
    G, H = 6, max(counts)
    firsts = [0, 1, 4, 5, 6, 7]
    centers, heights = np.zeros((G, 2, H)), rs.uniform(0.5e-3, 2e-3, (G, H))
    for g, c in enumerate(firsts):
        centers[g, 0] = br.wrap(br.cv(2, x[c, :4])[0] + rs.normal(0.0, 0.8, H))
        centers[g, 1] = np.linalg.norm(x[c, 4] - x[c, 5]) + rs.normal(0.0, 0.6, H)
    meta = md.Metadynamics(cvs, sig, 1e-3, 1, walkers=walkers, max_hills=capacity,
                           hills=(torch.from_numpy(centers[:, :n_cv]), torch.from_numpy(heights), torch.tensor(counts)))
    rest = [md.Restraint(md.distance(0, 5), 2.0, 0.01)]
    species = np.zeros((Cn, A), dtype=np.int64)
    return species, x, md.build_bias_tables(torch.from_numpy(species), None, rest + [meta]), firsts


@pytest.mark.parametrize("n_cv", [1, 2])
def test_hills_at_counts_around_the_chunk(dev, n_cv):
    from torchani_amd import _lib

    chunk = _lib.MD_BIAS_CHUNK
    counts = [3 * chunk + 7, 0, 1, chunk - 1, chunk, chunk + 1]
    species, x, tables, firsts = _hills_case(n_cv, 4 * chunk, counts)
    assert tables.list.tolist() == [0, 1, 0, -1, 2, 3, 4, 5] and tables.rank_in_list.tolist() == [0, 0, 1, 0, 0, 0, 0, 0]
    Cn, A = species.shape
    k = Abi(dev, tables, Cn, A)
    xk = k.set_x(x)
    model = br.Bias(tables)
    f0 = np.random.RandomState(2).normal(0.0, 0.05, x.shape).astype(np.float32)
    want = model.apply(xk, f0)
    got = k.apply(f0)
    assert (got["status"] == 0).all() and got["meta_energies"][3] == 0.0 and got["meta_energies"][1] == 0.0
    assert (want["meta_energies"][[0, 2, 4, 5, 6, 7]] > 0).all()
    _compare(got, want, f"hills, {n_cv} CV, counts {counts}")
    # the grid sized by the caller's bound gives the same bits as the grid over the capacity
    bounded = k.apply(f0, bound=max(counts))
    for key in got:
        assert np.array_equal(got[key], bounded[key]), key
    # the readout of every list at 257 points, and at the walkers themselves
    rs = np.random.RandomState(9)
    off = tables.cv_offset.numpy()
    worst = 0.0
    for g, c in enumerate(firsts):
        idx = [int(i) for i in tables.meta_cv[c] if i >= 0]
        here = np.array([want["cv_values"][off[c] + i] for i in idx])
        pts = np.zeros((257, 2))
        pts[:, :n_cv] = here + rs.normal(0.0, 1.0, (257, n_cv))
        pts[0, :n_cv] = got["cv_values"][off[c] + np.array(idx)]   # the walker's own values, as the device holds them
        V, dV = k.hills(g, pts)
        n = counts[g]
        periodic = [True, False][:n_cv]
        for p in range(257):
            wV, wd, scale = br.hills_sum(pts[p, :n_cv], model.centers[g][:, :n], model.heights[g][:n], model.inv_sigma2[c], periodic)
            tol = 1e-11 * scale
            assert abs(V[p] - wV) <= tol[0] and (np.abs(dV[p] - wd) <= tol[1:]).all(), (g, p)
            if scale[0] > 0:
                worst = max(worst, abs(V[p] - wV) / scale[0])
        assert V[0] == got["meta_energies"][c]   # the same chunks in the same order: the same bits
        if n == 0:
            assert (V == 0.0).all() and (dV == 0.0).all()
    print(f"md bias, anihip_md_bias_hills, {n_cv} CV: 6 lists x 257 points, worst |dV| / sum|w g| {worst:.1e}")
    assert k.guards_untouched()


# ---- deposit --------------------------------------------------------------------------------------------------------------------

def _deposit_case(gamma, capacity):
    from torchani_amd import md

    Cn, A = 8, 6
    walkers = torch.tensor([2, 0, 1, 2, 2, 1, 2, 2])   # lists of 1, 2 and 5 members
    meta = md.Metadynamics([md.dihedral(0, 1, 2, 3), md.distance(4, 5)], (0.4, 0.3),
                           torch.linspace(0.8e-3, 1.5e-3, Cn, dtype=torch.float64), 1, bias_factor=gamma, walkers=walkers,
                           max_hills=capacity)
    species = np.zeros((Cn, A), dtype=np.int64)
    T = torch.linspace(250.0, 400.0, Cn)
    return species, md.build_bias_tables(torch.from_numpy(species), None, [meta], temperature=T), T


@pytest.mark.parametrize("gamma", [None, 6.0])
def test_deposit_three_rounds(dev, gamma):
    species, tables, T = _deposit_case(gamma, 32)
    assert tables.members.tolist() == [1, 2, 5] and tables.rank_in_list.tolist() == [0, 0, 0, 1, 2, 1, 3, 4]
    Cn, A = species.shape
    k = Abi(dev, tables, Cn, A)
    model = br.Bias(tables)
    kT = torch.mul(T, ref.KB_HARTREE).numpy()   # the fp32 product
    rs = np.random.RandomState(4)
    f0 = np.zeros((Cn, A, 3), dtype=np.float32)
    worst = 0.0
    for rnd in range(3):
        # (round 1: the walkers close to their hills of round 0, so that the well-tempered factor bites)
        xk = k.set_x(prev + rs.normal(0.0, 0.02, prev.shape) if rnd == 1 else rs.uniform(-2.0, 2.0, (Cn, A, 3)))
        prev = xk
        got = k.apply(f0)
        _compare(got, model.apply(xk, f0), f"deposit round {rnd}, gamma {gamma}")
        k.deposit(None if gamma is None else kT)
        model.deposit(kT, got["cv_values"], got["meta_energies"])   # on the device's own values: the centres are copies
        used = k.used.cpu().numpy()
        assert np.array_equal(used, model.used) and used.tolist() == [(rnd + 1) * m for m in (1, 2, 5)]
        centers, heights = k.centers.cpu().numpy(), k.heights.cpu().numpy()
        for g in range(3):
            n = used[g]
            assert np.array_equal(centers[g][:, :n], model.centers[g][:, :n])   # bit for bit the cv_values given
            assert (centers[g][:, n:] == SENTINEL).all() and (heights[g][n:] == SENTINEL).all()
            err = np.abs(heights[g][:n] - model.heights[g][:n]) / np.spacing(model.heights[g][:n])
            worst = max(worst, err.max())
            assert (err <= 4.0).all()
        if gamma is not None and rnd == 1:
            last = heights[2][5:10] / tables.height.numpy()[[0, 3, 4, 6, 7]]
            assert (last < 0.999).all() and (last > 0.0).all()
    assert int(k.dropped.sum()) == 0 and k.guards_untouched()
    print(f"md bias, deposit, gamma {gamma}: 3 rounds on lists of 1, 2, 5 walkers, heights within {worst:.1f} fp64 ulp")


def test_deposit_never_writes_past_capacity(dev):
    species, tables, T = _deposit_case(None, 5)
    Cn, A = species.shape
    k = Abi(dev, tables, Cn, A)
    rs = np.random.RandomState(6)
    for _ in range(3):
        k.set_x(rs.uniform(-2.0, 2.0, (Cn, A, 3)))
        k.apply(np.zeros((Cn, A, 3), dtype=np.float32))
        k.deposit(None)
    assert k.used.tolist() == [3, 4, 5] and k.dropped.tolist() == [0, 2, 10]
    heights = k.heights.cpu().numpy()
    for g, n in enumerate((3, 4, 5)):
        assert (heights[g][:n] != SENTINEL).all() and (heights[g][n:] == SENTINEL).all()
    assert k.guards_untouched()


# ---- errors ---------------------------------------------------------------------------------------------------------------------

def test_broken_tables_move_nothing_and_are_reported(dev):
    from torchani_amd import _lib

    species, x, tables, _ = _hills_case(2, 2048, [5, 0, 1, 2, 3, 4])
    Cn, A = species.shape
    f0 = np.random.RandomState(2).normal(0.0, 0.05, x.shape).astype(np.float32)
    good = Abi(dev, tables, Cn, A)
    good.set_x(x)
    want = good.apply(f0)
    off = tables.cv_offset.numpy()

    def broken(name, index, value):
        t = getattr(tables, name).clone()
        t[index] = value
        return {name: t}

    r5 = int(off[5])   # entry 5 is the one that every case breaks
    cases = [
        (broken("atoms", (r5, 1), Cn * A + 3), _lib.MD_BIAS_BAD_CV),           # outside the batch
        (broken("atoms", (r5, 1), 2), _lib.MD_BIAS_BAD_CV),                    # an atom of entry 0
        (broken("atoms", (r5, 1), int(tables.atoms[r5, 0])), _lib.MD_BIAS_BAD_CV),   # twice the same
        (broken("atoms", (r5 + 1, 3), -1), _lib.MD_BIAS_BAD_CV),               # a dihedral of three atoms
        (broken("kind", r5, 3), _lib.MD_BIAS_BAD_CV),
        (broken("list", 5, 6), _lib.MD_BIAS_BAD_LIST),
        (broken("rank_in_list", 5, 1), _lib.MD_BIAS_BAD_LIST),
        (broken("meta_cv", (5, 1), 3), _lib.MD_BIAS_BAD_LIST),
        (broken("meta_cv", (5, 0), -1), _lib.MD_BIAS_BAD_LIST),
    ]
    for tab, bit in cases:
        k = Abi(dev, tables, Cn, A, **tab)
        k.set_x(x)
        got = k.apply(f0)
        assert got["status"][5] == bit and (np.delete(got["status"], 5) == 0).all(), (tab, got["status"])
        assert np.array_equal(got["forces"][5], f0[5])                                        # nothing moved
        assert got["bias_energies"][5] == SENTINEL and (got["cv_values"][off[5]:off[6]] == SENTINEL).all()
        for c in (0, 1, 2, 3, 4, 6, 7):                                                       # the others as if nothing were wrong
            assert np.array_equal(got["forces"][c], want["forces"][c]) and got["bias_energies"][c] == want["bias_energies"][c]
        k.deposit(None)
        # the flagged entry appends no hill: the slot that the round reserved for it keeps what it held
        # (the buffers were preloaded past ``used``: what a slot held is the preloaded value; a deposited height is 1e-3)
        assert k.used.tolist() == [7, 1, 2, 3, 4, 5] and k.guards_untouched()
        assert float(k.heights[3, 2]) == float(tables.heights[3, 2]) != 1e-3
        assert float(k.heights[4, 3]) == 1e-3 and float(k.heights[2, 1]) == 1e-3
    # a CSR offset that falls, and an entry of 17 CVs: both entries around it are refused, nothing is read out of range
    for value in (int(off[5]) - 1, int(off[5]) + 17):
        bad = tables.cv_offset.clone()
        bad[6] = value
        k = Abi(dev, tables, Cn, A, cv_offset=bad)
        k.set_x(x)
        got = k.apply(f0)
        assert got["status"][5] & _lib.MD_BIAS_BAD_OFFSET or got["status"][6] & _lib.MD_BIAS_BAD_OFFSET
        flagged = got["status"] != 0
        assert np.array_equal(got["forces"][flagged], f0[flagged])
    # what the host can see returns nonzero before anything is launched
    L, k = _lib.lib(), good
    args = lambda: [_stream(), C.byref(k.P), C.byref(k.b), k.x.data_ptr(), k.lo.data_ptr(), k.f.data_ptr(),   # noqa: E731
                    k.e_bias.data_ptr(), k.e_meta.data_ptr(), k.cv_values.data_ptr(), k.ws.data_ptr(), k.ws.numel()]
    before = k.f.clone()
    a = args()
    a[10] = 8
    assert L.anihip_md_bias_apply(*a) != 0 and b"workspace" in L.anihip_last_error()
    for null in (3, 5, 6):
        a = args()
        a[null] = None
        assert L.anihip_md_bias_apply(*a) != 0
    k.b.n_entries = Cn + 1
    assert L.anihip_md_bias_apply(*args()) != 0 and b"entries" in L.anihip_last_error()
    k.b.n_entries = Cn
    k.b.hills_bound = k.cap + 1
    assert L.anihip_md_bias_apply(*args()) != 0
    k.b.hills_bound = 0
    v = torch.zeros((4, 2), dtype=torch.float64, device=dev)
    o = torch.zeros((4, 3), dtype=torch.float64, device=dev)
    for g in (-1, 6):
        assert L.anihip_md_bias_hills(_stream(), C.byref(k.b), g, 4, v.data_ptr(), o.data_ptr(), o[:, 1:].data_ptr()) != 0
    assert L.anihip_md_bias_hills(_stream(), C.byref(k.b), 0, 4, None, o.data_ptr(), o.data_ptr()) != 0
    assert L.anihip_md_bias_deposit(_stream(), C.byref(k.P), C.byref(k.b), None, None, k.e_meta.data_ptr()) != 0
    assert torch.equal(k.f, before) and k.used.tolist() == [5, 0, 1, 2, 3, 4]
    # a list whose list_entry is out of range reads out NaN
    k = Abi(dev, tables, Cn, A, list_entry=torch.tensor([0, 1, 4, 99, 6, 7], dtype=torch.int32))
    V, dV = k.hills(3, np.zeros((4, 2)))
    assert np.isnan(V).all() and np.isnan(dV).all()


# ---- through the class ----------------------------------------------------------------------------------------------------------

def _lock_step(dyn, model, n_steps, what):
    """``n_steps`` steps of ``dyn`` with the reference recomputing CVs, energies, bias forces and deposits from the device's
    coordinates after each: the gates of the ABI tests, hill tables exact in count and centres."""
    b = dyn._bias
    deposits = 0
    for s in range(n_steps):
        dyn.step()
        x = dyn.coordinates.double().cpu().numpy() + dyn.coordinates_lo.double().cpu().numpy()
        _, f_model = dyn._model_eval(dyn.coordinates)   # (bit-reproducible evaluators: the forces the bias was added to)
        want = model.apply(x, f_model.cpu().numpy())
        got = {"forces": dyn.forces.cpu().numpy(), "cv_values": b.cv_values.cpu().numpy(),
               "bias_energies": dyn.bias_energies.cpu().numpy(), "meta_energies": b.meta_energies.cpu().numpy()}
        # at a deposit step the hills were appended after the bias was applied: the reference follows the same order
        _compare(got, want, f"{what}, step {s + 1}")
        cvs = dyn.collective_variables().cpu().numpy()
        idx = b.tables.cv_index.numpy()
        assert np.array_equal(cvs[idx >= 0], got["cv_values"][idx[idx >= 0]]) and np.isnan(cvs[idx < 0]).all()
        total = dyn.total_energies().cpu().numpy()
        assert np.array_equal(total, (dyn.potential_energies + dyn.bias_energies + dyn.kinetic_energies()).cpu().numpy())
        if b.n_lists and b.pace and (s + 1) % b.pace == 0:
            kT = torch.mul(dyn.temperature, ref.KB_HARTREE).cpu().numpy()
            model.deposit(kT, got["cv_values"], got["meta_energies"])
            deposits += 1
        if b.n_lists:
            centers, heights, used = (t.cpu().numpy() for t in dyn.hills())
            assert np.array_equal(used, model.used) and list(used) == b.counts
            for g in range(b.n_lists):
                n = used[g]
                assert np.array_equal(centers[g][:, :n], model.centers[g][:, :n])
                assert (np.abs(heights[g][:n] - model.heights[g][:n]) <= 4.0 * np.spacing(model.heights[g][:n])).all()
                assert (heights[g][n:] == 0.0).all()
    return deposits


def test_class_on_ani2x_in_lock_step_with_reference(dev):
    from torchani_amd import md

    model, sp, x, mass = _ani_replicas(dev)
    model.deterministic_forces = True   # (force sums in fixed point: a second evaluation gives the same bits)
    T = torch.tensor([300.0, 320.0, 340.0, 300.0, 310.0, 330.0], dtype=torch.float64)
    dist, dih = md.distance(0, 2), md.dihedral(0, 1, 2, 3)
    bias = [md.Restraint(md.angle(1, 2, 3), 1.9, 0.05, torch.tensor([0.0, 0.1, 0.0, 0.05, 0.0, 0.2], dtype=torch.float64)),
            md.Restraint(dist, 2.0, 0.02),
            md.Metadynamics([dist, dih], (0.1, 0.3), 2e-4, 2, bias_factor=6.0, walkers=torch.tensor([4, 4, 4, 9, -1, -1]),
                            max_hills=16)]
    dyn = md.BatchedDynamics(model, sp, x, dt=0.5, masses=mass, temperature=T, friction=0.05, seed=SEED, bias=bias)
    dyn.set_temperature(T)
    b = dyn._bias
    assert b.n_lists == 2 and b.members == [3, 1] and b.counts == [0, 0] and int(b.used.sum()) == 0   # nothing at construction
    assert tuple(dyn.collective_variables().shape) == (6, 3) and dyn.bias_energies.dtype == torch.float64
    ref_bias = br.Bias(b.tables)
    deposits = _lock_step(dyn, ref_bias, 6, "ANI-2x x 6, Langevin, a restraint, walls and 2-CV well-tempered hills")
    assert deposits == 3 and b.counts == [9, 3] and dyn.steps_done == 6
    assert float(dyn._bias.meta_energies[:4].min()) > 0.0 and float(dyn._bias.meta_energies[4:].abs().max()) == 0.0
    # the observables of the hills: the bias at the walkers' own CVs is the energy held, the free energy its multiple
    cv = dyn.collective_variables()[:, [1, 2]]
    V = dyn.metadynamics_bias(cv[:3], list=0)
    # (the energies held are those of before the last deposit; the readout sees the hills of after it)
    assert V.shape == (3,) and bool((V > dyn._bias.meta_energies[:3]).all())
    assert torch.equal(dyn.free_energies(cv[:3], list=0), -6.0 / 5.0 * V)
    # more walkers than room: step() raises on the host before the deposit that would not fit
    dyn.run(4)
    assert b.counts == [15, 5]
    dyn.step()
    with pytest.raises(RuntimeError, match="list 0 holds 15 hills and its 3 walkers"):
        dyn.step()
    assert dyn.hills()[2].tolist() == [15, 5] and int(b.dropped.sum()) == 0


def test_class_on_lennard_jones_in_lock_step_with_reference(dev):
    from torchani_amd import md

    lj, sp, x, mass = _lj_replicas(dev)
    center = torch.linspace(1.0, 1.4, 5, dtype=torch.float64)   # umbrella windows across the batch
    dyn = md.BatchedDynamics(lj, sp, x, dt=1.0, masses=mass, seed=7, bias=[md.Restraint(md.distance(0, 7), center, 0.05)])
    dyn.set_temperature(100.0)
    e0, bias0 = dyn.total_energies().clone(), dyn.bias_energies.clone()
    _lock_step(dyn, br.Bias(dyn._bias.tables), 6, "Lennard-Jones cube x 5, NVE, umbrella windows on a distance")
    assert float(dyn.bias_energies.min()) > 0.0
    # NVE conserves potential + bias + kinetic
    drift = (dyn.total_energies() - e0).abs().max().item()
    moved = float((dyn.bias_energies - bias0).abs().max())
    print(f"md bias, LJ cube NVE: |d(total energy)| after 6 steps {drift:.1e} Ha; the bias energies (up to "
          f"{dyn.bias_energies.max().item():.1e} Ha) changed by up to {moved:.1e} Ha")
    # (without the bias in the total, the total would change by what the bias energies changed by)
    assert drift < 0.1 * moved
    with pytest.raises(ValueError, match="no Metadynamics"):
        dyn.hills()


def test_step_and_observables_do_not_synchronize(dev):
    from torchani_amd import md

    model, sp, x, mass = _ani_replicas(dev)
    T = torch.full((6,), 300.0, dtype=torch.float64)
    dist = md.distance(0, 2)
    bias = [md.Restraint(dist, 2.0, 0.02), md.Metadynamics(dist, 0.1, 2e-4, 2, bias_factor=6.0,
                                                           walkers=torch.tensor([0, 0, 0, 1, -1, -1]), max_hills=64)]
    dyn = md.BatchedDynamics(model, sp, x, masses=mass, temperature=T, seed=1, bias=bias)
    dyn.set_temperature(T)
    for _ in range(3):   # (the third evaluation captures the automatic HIP graph)
        dyn.step()
    values = torch.linspace(1.5, 3.0, 33, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(4):   # deposits after steps 4 and 6
            dyn.step()
        dyn.collective_variables(), dyn.hills(), dyn.metadynamics_bias(values, list=1), dyn.free_energies(values)
        dyn.total_energies(), dyn.bias_energies.sum()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert dyn.steps_done == 7 and dyn._bias.counts == [9, 3] and dyn.hills()[2].tolist() == [9, 3]


def test_no_bias_is_bit_identical(dev):
    """bias=None and a bias whose every index is -1 launch nothing more: the same bits over 8 steps as a dynamics built
    without the argument."""
    from torchani_amd import md

    lj, sp, x, mass = _lj_replicas(dev)
    none = torch.full((5,), -1, dtype=torch.int64)
    empty = [md.Restraint(md.distance(none, 1), 1.0, 1.0), md.Metadynamics(md.angle(0, none, 2), 0.1, 1e-3, 1)]
    kw = dict(dt=1.0, masses=mass, temperature=120.0, friction=0.05, seed=SEED)
    runs = [md.BatchedDynamics(lj, sp, x, **kw), md.BatchedDynamics(lj, sp, x, bias=None, **kw),
            md.BatchedDynamics(lj, sp, x, bias=empty, **kw)]
    for d in runs:
        assert d._bias is None
        d.set_temperature(120.0)
        d.run(8)
    for d in runs[1:]:
        for name in ("coordinates", "coordinates_lo", "velocities", "forces", "potential_energies"):
            assert torch.equal(getattr(d, name), getattr(runs[0], name)), name
        assert torch.equal(d.total_energies(), runs[0].total_energies()) and float(d.bias_energies.abs().max()) == 0.0


def test_replica_exchange_takes_potential_plus_bias(dev):
    """In lock-step with the reference ladders of the replica-exchange tests, fed potential + bias energies."""
    from torchani_amd import md

    lj, sp, x, mass = _lj_replicas(dev)
    T = md.temperature_ladder(60.0, 240.0, 5)
    center = torch.tensor([1.0, 1.3, 0.9, 1.5, 1.1], dtype=torch.float64)
    dyn = md.ReplicaExchangeDynamics(lj, sp, x, dt=1.0, masses=mass, temperature=T, friction=0.02, exchange_every=2, seed=7,
                                     bias=[md.Restraint(md.distance(0, 7), center, 0.3)])
    dyn.set_temperature(T)
    lad = rx.Ladders(np.arange(5)[None], ref.KB_HARTREE * dyn.rung_temperatures.cpu().numpy(), 5)
    accepted = differs = 0
    for s in range(8):
        dyn.step()
        if (s + 1) % 2:
            continue
        n = (s + 1) // 2 - 1
        both = (dyn.potential_energies + dyn.bias_energies).cpu().numpy()
        accepted += lad.attempt(n, dyn.seed, both)
        assert lad.margin >= 1e-6, lad.margin
        assert np.array_equal(dyn.replicas_at_rungs().cpu().numpy(), lad.slot)
        assert np.array_equal(dyn.exchange_accepts.cpu().numpy(), lad.accepts)
        gap = np.abs(np.diff(dyn.bias_energies.cpu().numpy())).max()
        differs = max(differs, gap)
    assert differs > 1e-4, "the restraint energies must matter to the decisions"
    print(f"md bias, replica exchange with restraints, LJ cube x 5: {accepted} swaps accepted in 4 attempts, bias energies "
          f"of neighbors up to {differs:.1e} Ha apart")


def _dimers(dev, n, eps, r0):
    from torchani_amd.potentials import LennardJones

    lj = LennardJones(("H",), eps=(eps,), sigma=(3.0,)).to(dev)
    x = torch.zeros((n, 2, 3), device=dev)
    x[:, 1, 0] = r0
    return lj, torch.ones((n, 2), dtype=torch.int64, device=dev), x, torch.full((n, 2), 12.011, device=dev)


def test_restraint_sampling_of_a_dimer(dev):
    """4096 Lennard-Jones dimers (eps 0.002 Ha, sigma 3 A, infinite cutoff) with a harmonic restraint on their distance
    (center 4 A, k 0.02 Ha / A^2) at 300 K, 400 steps of 2 fs with friction 0.05 / fs from r = 4: the mean and the variance of r
    at the last step against the quadrature of r^2 exp(-beta (U_LJ + U_restraint)), within 5 standard errors."""
    from torchani_amd import md

    n, kT = 4096, ref.KB_HARTREE * 300.0
    lj, sp, x, mass = _dimers(dev, n, 0.002, 4.0)
    dyn = md.BatchedDynamics(lj, sp, x, dt=2.0, masses=mass, temperature=300.0, friction=0.05, seed=5, remove_drift=False,
                             bias=[md.Restraint(md.distance(0, 1), 4.0, 0.02)])
    dyn.set_temperature(300.0)
    dyn.run(400, check_every=400)
    r = dyn.collective_variables()[:, 0].cpu().numpy()
    grid = np.linspace(2.0, 7.0, 20001)
    U = br.dimer_free_energy(grid, 0.002, 3.0, kT) + 0.5 * 0.02 * (grid - 4.0) ** 2
    w = np.exp(-(U - U.min()) / kT)
    w /= w.sum()
    mu = (w * grid).sum()
    var = (w * (grid - mu) ** 2).sum()
    m4 = (w * (grid - mu) ** 4).sum()
    z_mean = (r.mean() - mu) / math.sqrt(var / n)
    z_var = (((r - mu) ** 2).mean() - var) / math.sqrt((m4 - var * var) / n)
    print(f"md bias, restrained LJ dimer x {n}: <r> {r.mean():.4f} A against {mu:.4f} (z = {z_mean:.2f}), <(r - mu)^2> "
          f"{((r - mu) ** 2).mean():.5f} A^2 against {var:.5f} (z = {z_var:.2f})")
    assert abs(z_mean) <= 5.0 and abs(z_var) <= 5.0


# max |F - F_exact| / kT, means removed, of tests/_md_bias_ref.py::dimer_metadynamics (numpy, this protocol, the deposit timing of
# include/anihip.h) over the seeds 0 .. 4: 0.434, 0.350, 0.257, 0.322, 0.247.  The gate is twice the largest.
FE_REFERENCE_WORST = 0.434
FE_GATE = 2.0 * FE_REFERENCE_WORST


def test_multiple_walker_metadynamics_recovers_the_free_energy(dev):
    """128 Lennard-Jones dimers (eps 0.005 Ha, sigma 3 A) as the walkers of one shared well-tempered bias on their distance:
    sigma 0.1 A, height 0.02 kT, bias factor 6, a hill per walker every 10 steps, 1000 steps of 2 fs at 300 K (12 800 hills),
    flat-bottom walls at 4.25 +- 1.75 A.  ``free_energies`` on 49 points of 3.1 .. 5.5 A against U(r) - 2 kT ln r, means
    removed.  F spreads over 3.74 kT on this range, so the gate, below half of that, fails a run without bias by a wide
    margin (an unbiased F is flat: its error is the 3.74 kT spread's own deviation from its mean, 2.4 kT at the wall side)."""
    from torchani_amd import md

    n, kT = 128, ref.KB_HARTREE * 300.0
    assert FE_GATE < 1.87
    lj, sp, x, mass = _dimers(dev, n, 0.005, 2.0 ** (1.0 / 6.0) * 3.0)
    r = md.distance(0, 1)
    bias = [md.Restraint(r, 4.25, 0.05, 1.75),
            md.Metadynamics(r, 0.1, 0.02 * kT, 10, bias_factor=6.0, walkers=torch.zeros(n, dtype=torch.int64), max_hills=12800)]
    dyn = md.BatchedDynamics(lj, sp, x, dt=2.0, masses=mass, temperature=300.0, friction=0.05, seed=3, remove_drift=False,
                             bias=bias)
    dyn.set_temperature(300.0)
    dyn.run(1000, check_every=1000)
    assert dyn.hills()[2].tolist() == [12800]
    grid = np.linspace(3.1, 5.5, 49)
    F = dyn.free_energies(torch.from_numpy(grid).to(dev)).cpu().numpy()
    exact = br.dimer_free_energy(grid, 0.005, 3.0, kT)
    err = np.abs((F - F.mean()) - (exact - exact.mean())).max() / kT
    flat = np.abs(exact - exact.mean()).max() / kT
    print(f"md bias, multiple-walker well-tempered metadynamics, {n} LJ dimers, 12 800 hills: max |dF| {err:.3f} kT on 3.1 .. "
          f"5.5 A (numpy reference over 5 seeds: at most {FE_REFERENCE_WORST} kT; gate {FE_GATE:.3f} kT; a flat F would be "
          f"{flat:.2f} kT off)")
    assert flat > 2.0 * FE_GATE
    assert err <= FE_GATE
