"""Reaction paths (torchani_amd.geomopt.ReactionPathFollower, anihip_irc_*) on the MI355X: the three entry points alone against
the fp64 reference (tests/_irc_ref.py) on synthetic Hessians, gradients, coordinates and masses; lock-step parity of whole points
on a padded ANI-2x batch and a periodic box; the reaction path through the D2h saddle of the four-atom Lennard-Jones cluster
through the public interface, against the fp64 path of the host rehearsal; refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from _irc_ref import (ENERGY_ROSE, LOCKSTEP_STEP, MINIMUM, PATH_FULL, RUNNING, IrcReference, fixture_masses, lj4_saddle,
                      run_lj_path)
from _util import load_golden, seeded_state

pytestmark = pytest.mark.gpu

REPORT = os.environ.get("TORCHANI_AMD_IRC_REPORT")
# The gates of tests/test_gpu_saddle.py, with its arguments: whole points in lock-step are compared to 1e-4 of the largest
# component of the step (the gate of the L-BFGS lock-step); the kernels alone, both sides fp64 and rounding the displacement to
# fp32 at the end, to one fp32 rounding of an element plus fp64 noise (the LQA displacement is a smooth function of the
# projected Hessian: no eigenvalue gap enters, except the gap of >= 0.01 below the second mode on the first point).
PARITY = 1e-4
KERNEL_PARITY = 1e-6
HESSIAN_PARITY = 1e-9   # the Bofill update: fp64 noise of xi = y - H s over |xi| |s|, four orders of margin
ARC_PARITY = 1e-8       # the arc increment: the kernel finds t to 1e-12 of the step (1e-9 is its contract), the reference by bisection
# What moves in an entry without an internal coordinate (one free atom and nothing fixed) is the rounding noise of the
# projection, about 1e-17 A on both sides: such displacements are only required to stay below this.
NOISE = 1e-12
LJ_FMAX = 1e-5          # the fp32 floor of Lennard-Jones forces argued in test_gpu_geomopt.py
STEP, FMAX, FLOOR, MAX_POINTS = 0.05, 1e-3, 1e-7, 3


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


# ---- the entry points alone ------------------------------------------------------------------------------------------

class Raw:
    """Device state of anihip_irc for kind, masses [C, A], x, f [C, A, 3], e [C], H [C, n, n] (numpy)."""

    def __init__(self, dev, kind, masses, x, f, e, H, periodic, direction=None, n_points=None, arcs=None, reason=None,
                 step=STEP, fmax=FMAX, max_points=MAX_POINTS):
        from torchani_amd import _lib
        from torchani_amd.geomopt import irc_workspace_bytes

        self.lib, self._lib = _lib.lib(), _lib
        Cn, A = kind.shape
        n = 3 * A
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt).contiguous()   # noqa: E731
        self.kind, self.masses = t(kind, torch.uint8), t(masses, torch.float64)
        self.x, self.f = t(x, torch.float32), t(f, torch.float32)
        self.e, self.H = t(e, torch.float64), t(H, torch.float64)
        self.direction = None if direction is None else t(direction, torch.float64)
        self.last = torch.full((Cn, A, 3), 7.0, dtype=torch.float32, device=dev)
        self.arcs = torch.zeros(Cn, dtype=torch.float64, device=dev) if arcs is None else t(arcs, torch.float64)
        self.n_points = torch.zeros(Cn, dtype=torch.int32, device=dev) if n_points is None else t(n_points, torch.int32)
        self.reason = torch.zeros(Cn, dtype=torch.int32, device=dev) if reason is None else t(reason, torch.int32)
        self.status = torch.zeros(Cn, dtype=torch.int32, device=dev)
        self.path_x = torch.full((Cn, max_points, A, 3), np.nan, dtype=torch.float32, device=dev)
        self.path_e = torch.full((Cn, max_points), np.nan, dtype=torch.float64, device=dev)
        self.path_s = torch.full((Cn, max_points), np.nan, dtype=torch.float64, device=dev)
        self.ws = torch.zeros(irc_workspace_bytes(Cn, A), dtype=torch.uint8, device=dev)
        self.projected = torch.eye(n, dtype=torch.float64, device=dev).repeat(Cn, 1, 1)
        self.st = _lib.Irc(Cn, A, int(periodic), max_points, step, fmax, FLOOR, self.kind.data_ptr(), self.masses.data_ptr(),
                           self.x.data_ptr(), self.e.data_ptr(), self.f.data_ptr(), self.H.data_ptr(),
                           None if direction is None else self.direction.data_ptr(), self.last.data_ptr(),
                           self.arcs.data_ptr(), self.n_points.data_ptr(), self.reason.data_ptr(), self.status.data_ptr(),
                           self.path_x.data_ptr(), self.path_e.data_ptr(), self.path_s.data_ptr(), self.ws.data_ptr(),
                           self.ws.numel())

    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    def project(self):
        self._lib.check(self.lib.anihip_irc_project(self.stream(), C.byref(self.st), self.projected.data_ptr()))

    def step(self):
        lam, V = torch.linalg.eigh(self.projected)
        self.lam, self.V = lam.contiguous(), V.contiguous()
        self._lib.check(self.lib.anihip_irc_step(self.stream(), C.byref(self.st), self.lam.data_ptr(), self.V.data_ptr()))

    def commit(self, e_new, f_new, update):
        self.e_new = torch.from_numpy(np.ascontiguousarray(e_new)).to(self.x.device, torch.float64)
        self.f_new = torch.from_numpy(np.ascontiguousarray(f_new)).to(self.x.device, torch.float32).contiguous()
        self._lib.check(self.lib.anihip_irc_commit(self.stream(), C.byref(self.st), self.e_new.data_ptr(),
                                                   self.f_new.data_ptr(), int(update)))

    def tensors(self):
        return (self.x, self.f, self.e, self.H, self.arcs, self.n_points, self.reason, self.path_x, self.path_e, self.path_s)


def _same(a, b):
    """Bit for bit, the NaN of unused path slots alike."""
    if not a.is_floating_point():
        return torch.equal(a, b)
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(), b.nan_to_num())


def _synthetic(A, rs, lowest):
    """x, f, H of one molecule of A atoms: a spectrum of order one, separated by >= 1e-3, its lowest value ``lowest``."""
    n = 3 * A
    x = rs.uniform(-1.0, 1.0, (A, 3)) * max(1.0, A ** (1 / 3))
    if A == 2:
        x[1] = x[0] + [0.4, -0.7, 0.9]
    U, _ = np.linalg.qr(rs.randn(n, n))
    spec = np.sort(rs.uniform(0.5, 8.0, n)) + 1e-3 * np.arange(n)
    spec[0] = lowest
    if n > 4:
        spec[1] = lowest + 0.37
    H = (U * spec) @ U.T
    return x, rs.uniform(-0.3, 0.3, (A, 3)), 0.5 * (H + H.T)


# entry: (lowest eigenvalue of H, variant, scale of the forces, points already on the path)
ENTRIES = [(-0.7, "plain", 1.0, 0),       # the first point along +direction
           (-0.7, "plain", 1.0, 0),       # the same molecule along -direction
           (-0.7, "plain", 1.0, 2),       # LQA with a negative lowest eigenvalue; the append fills the path
           (0.3, "plain", 1.0, 1),        # positive definite, the minimum of the model is far: no landing
           (0.3, "plain", 1e-3, 1),       # positive definite, the minimum of the model is nearer than the step: it lands
           (-0.4, "padding", 1.0, 1),     # the last atoms padding
           (0.3, "fixed", 1.0, 1),        # the first atom fixed
           (0.3, "padding", 1e-3, 1)]     # padding, lands


def _batch(A, rs):
    kinds, ms, xs, fs, Hs = [], [], [], [], []
    for c, (lowest, variant, fscale, _) in enumerate(ENTRIES):
        if c == 1:
            x, f, H, m = xs[0], fs[0], Hs[0], ms[0]
        else:
            x, f, H = _synthetic(A, rs, lowest)
            m = rs.uniform(1.0, 40.0, A)
        kind = np.ones(A, dtype=np.uint8)
        if variant == "padding":
            kind[A - max(1, A // 3):] = 0
        if variant == "fixed":
            kind[0] = 2
        kinds.append(kind), ms.append(m), xs.append(x), fs.append(f * fscale if c != 1 else f), Hs.append(H)
    direction = rs.randn(len(ENTRIES), 3 * A)
    direction[1] = -direction[0]
    n_points = np.array([e[3] for e in ENTRIES])
    if A == 1:   # (one atom has no mode to start along: every entry takes the LQA step, which is zero)
        n_points[:2] = 1
    return np.stack(kinds), np.stack(ms), np.stack(xs), np.stack(fs), np.stack(Hs), direction, n_points


def _reference(kind, masses, periodic, direction, n_points, arcs, max_points=MAX_POINTS, step=STEP, fmax=FMAX):
    ref = IrcReference(kind, masses, periodic, step, fmax, FLOOR, max_points, direction=direction)
    ref.n_points = np.asarray(n_points, dtype=np.int64).copy()
    ref.arc = np.asarray(arcs, dtype=np.float64).copy()
    return ref


def _check_move(raw, dr, x0, gate=KERNEL_PARITY):
    """last_step against the reference's displacement, and the coordinates moved by exactly last_step."""
    got = raw.last.cpu().numpy().astype(np.float64)
    worst = 0.0
    for c in range(dr.shape[0]):
        scale = np.abs(dr[c]).max()
        err = np.abs(got[c] - dr[c]).max()
        if scale <= NOISE:
            assert np.abs(got[c]).max() <= NOISE, c
            continue
        worst = max(worst, err / scale)
        assert err <= gate * scale, (c, err / scale)
    x1 = (torch.from_numpy(x0).to(raw.x.device, torch.float32) + raw.last)
    assert torch.equal(raw.x, x1)
    return worst


@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("A", [1, 2, 3, 4, 21, 22, 86])
def test_entry_points_against_reference(dev, A, periodic):
    """One whole point of the eight molecules of ENTRIES through the raw entry points: the projection and the step against the
    reference, then commit with made-up new energies and forces that take every branch, and the Bofill update."""
    rs = np.random.RandomState(300 + A)
    kind, masses, x, f, H, direction, n_points = _batch(A, rs)
    Cn = len(ENTRIES)
    e = rs.uniform(-1.0, 1.0, Cn)
    arcs = rs.uniform(0.1, 0.5, Cn) * (n_points > 0)
    raw = Raw(dev, kind, masses, x, f, e, H, periodic, direction=direction, n_points=n_points, arcs=arcs)
    x32, f32 = raw.x.cpu().numpy(), raw.f.cpu().numpy()
    ref = _reference(kind, masses, periodic, direction, n_points, arcs)
    raw.project()
    raw.step()
    dr = ref.propose(x32, e, f32, H)
    assert raw.status.cpu().tolist() == [0] * Cn
    worst = _check_move(raw, dr, x32)
    dof = np.array([np.abs(dr[c]).max() > NOISE for c in range(Cn)])   # (False: no internal coordinate, see NOISE)
    if A >= 3:
        assert dof.all()
        assert np.abs(dr[0] + dr[1]).max() == 0.0                       # the two signs of the direction
        # a landing threshold exists where every moving mode has a positive eigenvalue (entry 5 keeps the negative one of
        # its Hessian or not, as the padding cuts it)
        assert np.isfinite(ref.margin[[3, 4, 6, 7]]).all() and (A < 21 or not np.isfinite(ref.margin[2]))
        assert ref.landed[[4, 7]].all() and not ref.landed[[2, 3, 5, 6]].any()
    # the landing threshold is nowhere near: both sides take the same branch
    assert ref.margin.min() >= 1e-2, ref.margin
    # commit: 0 append, 1 the energy rises, 2 append and the path is full, 3 a minimum by fmax, the others append; an entry
    # without an internal coordinate gets forces below fmax, so that it ends as a minimum whether its noise is zero or not
    e_new = e - rs.uniform(1e-3, 1e-2, Cn)
    e_new[1] = e[1] + 1e-5
    f_new = f32 + rs.uniform(-0.05, 0.05, f32.shape).astype(np.float32)
    f_new[3] = 1e-5 * f32[3]
    f_new[~dof] = 1e-5 * f32[~dof]
    x_moved = raw.x.clone()
    raw.commit(e_new, f_new, True)
    ref.judge(e_new, f_new, True)
    assert raw.status.cpu().tolist() == [0] * Cn
    assert raw.reason.cpu().tolist() == ref.reason.tolist() and raw.n_points.cpu().tolist() == ref.n_points.tolist()
    if A >= 3:
        assert ref.reason.tolist() == [RUNNING, ENERGY_ROSE, PATH_FULL, MINIMUM, RUNNING, RUNNING, RUNNING, RUNNING]
        assert ref.n_points.tolist() == [1, 0, 3, 2, 2, 2, 2, 2]
    Hd, got_arcs = raw.H.cpu().numpy(), raw.arcs.cpu().numpy()
    px, pe, ps = raw.path_x.cpu().numpy(), raw.path_e.cpu().numpy(), raw.path_s.cpu().numpy()
    worst_h = worst_s = 0.0
    for c in range(Cn):
        slot = np.zeros(MAX_POINTS, dtype=bool)
        if ref.reason[c] == ENERGY_ROSE:   # x, e, f, H, the arc bit for bit those of before, nothing appended
            assert raw.e[c].item() == e[c] and np.array_equal(raw.f[c].cpu().numpy(), f32[c])
            assert np.array_equal(raw.x[c].cpu().numpy(), x32[c]) and np.array_equal(Hd[c], H[c]) and got_arcs[c] == arcs[c]
        else:                              # committed and appended at the slot of the old count
            assert raw.e[c].item() == e_new[c] and torch.equal(raw.f[c].cpu(), torch.from_numpy(f_new[c]))
            assert torch.equal(raw.x[c], x_moved[c])
            k = n_points[c]
            slot[k] = True
            assert np.array_equal(px[c, k], x_moved[c].cpu().numpy()) and pe[c, k] == e_new[c] and ps[c, k] == got_arcs[c]
            ds, ds_ref = got_arcs[c] - arcs[c], ref.ds[c]
            if dof[c]:
                worst_s = max(worst_s, abs(ds - ds_ref) / ds_ref)
                # (the increment is read as a difference of cumulative arcs: their rounding is allowed for)
                assert abs(ds - ds_ref) <= ARC_PARITY * ds_ref + 4e-16 * arcs[c], (c, ds, ds_ref)
            else:
                assert 0.0 <= ds <= NOISE
        assert np.isnan(px[c][~slot]).all() and np.isnan(pe[c][~slot]).all() and np.isnan(ps[c][~slot]).all()
        err = np.abs(Hd[c] - ref.H[c]).max() / np.abs(ref.H[c]).max()
        if dof[c]:
            worst_h = max(worst_h, err)
            assert err <= HESSIAN_PARITY, (c, err)
        assert np.array_equal(Hd[c], Hd[c].T)
    report(f"irc entry points A = {A}, periodic {periodic}: worst |d last_step| / max |s_ref| = {worst:.1e}, worst |d arc "
           f"increment| / increment = {worst_s:.1e}, worst |d H| / max |H| after Bofill = {worst_h:.1e}, smallest landing margin "
           f"{ref.margin.min():.1e}")


def test_finished_batch_changes_nothing(dev):
    rs = np.random.RandomState(5)
    kind, masses, x, f, H, direction, n_points = _batch(4, rs)
    Cn = len(ENTRIES)
    e = rs.uniform(-1.0, 1.0, Cn)
    reason = np.array([MINIMUM, ENERGY_ROSE, PATH_FULL, MINIMUM, ENERGY_ROSE, PATH_FULL, MINIMUM, MINIMUM])
    raw = Raw(dev, kind, masses, x, f, e, H, False, direction=direction, n_points=n_points, arcs=0.1 * n_points, reason=reason)
    before = [t.clone() for t in raw.tensors() + (raw.projected,)]
    raw.project()
    raw.step()
    raw.commit(e - 1.0, raw.f.cpu().numpy() + 1.0, True)
    assert all(_same(a, b) for a, b in zip(before, raw.tensors() + (raw.projected,)))
    assert not raw.last.any() and not raw.status.any()


def test_status_bits_leave_the_other_entries_alone(dev):
    """A kind above 2, a mass that is zero, negative or not finite on a real atom (a fixed one included) and a force that is not
    finite set their bits and freeze their entries; the entries between them step as if alone."""
    from torchani_amd import _lib

    rs = np.random.RandomState(8)
    A = 5
    kind, masses, x, f, H, direction, n_points = _batch(A, rs)
    Cn = len(ENTRIES)
    bad_kind, bad_m, bad_f = kind.copy(), masses.copy(), f.copy()
    bad_kind[0, 1] = 3
    bad_m[2, 3] = 0.0
    bad_m[4, 0] = np.nan
    bad_m[6, 0] = -2.0          # the fixed atom of entry 6
    bad_f[3, 1, 1] = np.inf
    bad_m[5, A - 1] = np.nan    # a padding atom: its mass is never read
    e = np.zeros(Cn)
    raw = Raw(dev, bad_kind, bad_m, x, bad_f, e, H, False, direction=direction, n_points=n_points)
    raw.project()
    raw.step()
    want = [_lib.IRC_BAD_TABLE, 0, _lib.IRC_BAD_TABLE, _lib.IRC_NONFINITE, _lib.IRC_BAD_TABLE, 0, _lib.IRC_BAD_TABLE, 0]
    assert raw.status.cpu().tolist() == want
    good = [c for c in range(Cn) if want[c] == 0]
    ref = _reference(kind[good], masses[good], False, direction[good], n_points[good], np.zeros(len(good)))
    dr = ref.propose(x[good].astype(np.float32), e[good], f[good].astype(np.float32), H[good])
    got = raw.last.cpu().numpy().astype(np.float64)
    for k, c in enumerate(good):
        assert np.abs(got[c] - dr[k]).max() <= KERNEL_PARITY * np.abs(dr[k]).max()
    bad = [c for c in range(Cn) if want[c] != 0]
    assert not got[bad].any() and torch.equal(raw.x[bad].cpu(), torch.from_numpy(x[bad].astype(np.float32)))
    # a new energy that is not finite: its entry is restored and flagged, the others commit
    x_before = torch.from_numpy(x.astype(np.float32))
    e_new = e - 1e-3
    e_new[1] = np.nan
    raw.commit(e_new, np.full_like(f, 0.1, dtype=np.float32), True)
    want[1] = _lib.IRC_NONFINITE
    assert raw.status.cpu().tolist() == want
    assert torch.equal(raw.x[1].cpu(), x_before[1]) and raw.n_points.cpu().tolist() == [0, 0, 2, 1, 1, 2, 1, 2]
    assert raw.reason.cpu().tolist() == [0] * Cn


# ---- whole points in lock-step with the reference -------------------------------------------------------------------------

def _ani_case(base, dev):
    from torchani_amd.models import ANI1x, ANI2x

    g = load_golden(base)
    sp = torch.from_numpy(g["species"].astype(np.int64)).to(dev)
    x = torch.from_numpy(g["coords"]).to(dev)
    cell = None if g["cell"] is None else torch.from_numpy(g["cell"]).to(dev)
    pbc = None if g["pbc"] is None else torch.from_numpy(np.asarray(g["pbc"])).to(dev)
    ctor = ANI2x if g["kind"] == "ani2x" else ANI1x
    model = ctor(state_dict=seeded_state(g["kind"], 8, g["seed"]), device=dev, periodic_table_index=False,
                 cutoff_fn=g["cutoff_fn"], row_capacity=256)
    masses = torch.from_numpy(fixture_masses(g)).to(dev)
    return model, sp, x, cell, pbc, masses


def _lockstep(model, sp, x, cell, pbc, masses, hessian_every, n_calls):
    """Steps the follower phase by phase; before each point the reference receives the coordinates, energies, forces and, on
    exact calls, the Hessian read back from the device, and after the move the trial energies and forces."""
    from torchani_amd.geomopt import ReactionPathFollower

    opt = ReactionPathFollower(model, sp, x, cell, pbc, masses=masses, step=LOCKSTEP_STEP, max_points=n_calls,
                               hessian_every=hessian_every, fmax=1e-4)
    st = opt._state
    ref = IrcReference(opt._kind.cpu().numpy(), masses.cpu().numpy(), bool(st.periodic), LOCKSTEP_STEP, st.fmax, st.energy_floor,
                       n_calls)
    worst = worst_h = worst_s = 0.0
    compared = skipped = 0
    for k in range(n_calls):
        opt._refresh_hessians()
        xk, ek, fk = opt.coordinates.cpu().numpy(), opt.energies.cpu().numpy(), opt.forces.cpu().numpy()
        Hk = opt.hessians.cpu().numpy()
        exact = k % hessian_every == 0
        if not exact:   # the Bofill updates of both sides since the last exact Hessian
            for c in range(sp.shape[0]):
                err = np.abs(Hk[c] - ref.H[c]).max() / np.abs(ref.H[c]).max()
                worst_h = max(worst_h, err)
                assert err <= HESSIAN_PARITY, (k, c, err)
        arcs_before = opt.arc_lengths.cpu().numpy()
        opt._move()
        dr = ref.propose(xk, ek, fk, Hk if exact else None)
        got = opt.last_step.cpu().numpy().astype(np.float64)
        opt._judge()
        ref.judge(opt.trial_energies.cpu().numpy(), opt.trial_forces.cpu().numpy(), (k + 1) % hessian_every != 0)
        assert not bool(opt.status.any())
        arcs = opt.arc_lengths.cpu().numpy()
        for c in range(sp.shape[0]):
            if ref.pending[c] is None:
                assert not got[c].any(), (k, c)
                continue
            if ref.margin[c] < 1e-6:   # on the landing threshold: the two sides may take different branches
                skipped += 1
                continue
            compared += 1
            scale = np.abs(dr[c]).max()
            err = np.abs(got[c] - dr[c]).max()
            worst = max(worst, err / scale)
            assert err <= PARITY * scale, (k, c, err / scale)
            if ref.reason[c] != ENERGY_ROSE:
                ds = arcs[c] - arcs_before[c]
                worst_s = max(worst_s, abs(ds - ref.ds[c]) / ref.ds[c])
                assert abs(ds - ref.ds[c]) <= ARC_PARITY * ref.ds[c] + 4e-16 * arcs[c], (k, c)
        assert opt.reasons.cpu().tolist() == ref.reason.tolist(), k
        assert opt.n_points.cpu().tolist() == ref.n_points.tolist(), k
    assert skipped <= 0.1 * (compared + skipped)
    return worst, worst_h, worst_s, compared, skipped, opt, ref


@pytest.mark.parametrize("hessian_every", [1, 4])
@pytest.mark.parametrize("base", ["rand_batch_ani2x", "water_pbc_ani2x"])
def test_lockstep(dev, base, hessian_every):
    model, sp, x, cell, pbc, masses = _ani_case(base, dev)
    worst, worst_h, worst_s, compared, skipped, opt, ref = _lockstep(model, sp, x, cell, pbc, masses, hessian_every, 8)
    report(f"irc lock-step {base}, hessian_every {hessian_every}, step {LOCKSTEP_STEP}, 8 points: worst |d last_step| / max "
           f"|s_ref| = {worst:.1e} (gate {PARITY:.0e}), worst |d H| / max |H| between exact Hessians = {worst_h:.1e} (gate "
           f"{HESSIAN_PARITY:.0e}), worst |d arc increment| / increment = {worst_s:.1e}, {compared} pairs compared, {skipped} "
           f"skipped; points {ref.n_points.tolist()}, reasons {ref.reason.tolist()}, exact Hessians "
           f"{opt.n_hessians.cpu().tolist()}")
    assert compared > 0 and ref.n_points.sum() > 0
    # the paths on the device are the committed points
    n = opt.n_points.cpu().numpy()
    for c in range(sp.shape[0]):
        assert not torch.isnan(opt.path_energies[c, :n[c]]).any() and torch.isnan(opt.path_energies[c, n[c]:]).all()
        if n[c] and ref.reason[c] != ENERGY_ROSE:
            assert torch.equal(opt.path_coordinates[c, n[c] - 1], opt.coordinates[c])
            assert opt.path_arc_lengths[c, n[c] - 1].item() == opt.arc_lengths[c].item()


# ---- the four-atom Lennard-Jones cluster through the public interface ------------------------------------------------------

_LJ4 = {}
EQUAL, UNEQUAL = (1.0, 1.0, 1.0, 1.0), (1.0, 4.0, 9.0, 16.0)
LJ_KW = dict(step=0.05, max_points=128, fmax=LJ_FMAX, energy_floor=2e-6)   # (the floor: a few fp32 ulps of |E| = 6)


def _lj4(dev):
    """The saddles of four diamond starts (0.002 sigma of noise, seeds 0 to 3) as in tests/test_gpu_saddle.py, and their
    reaction paths: with equal masses twice, with masses (1, 4, 9, 16) once."""
    if "out" in _LJ4:
        return _LJ4["out"]
    from _saddle_ref import lj4_diamond
    from torchani_amd.geomopt import follow_reaction_path, optimize_saddle
    from torchani_amd.potentials import LennardJones

    lj = LennardJones(("H",), eps=(1.0,), sigma=(1.0,)).to(dev)
    x = torch.from_numpy(np.stack([lj4_diamond(0.002, s) for s in range(4)])).to(dev)
    sp = torch.ones((4, 4), dtype=torch.int64, device=dev)
    saddles = optimize_saddle(lj, sp, x, fmax=LJ_FMAX, steps=60, negative_tol=1e-2)
    mass = lambda m: torch.tensor(m, dtype=torch.float64, device=dev).repeat(4, 1)   # noqa: E731
    paths = [follow_reaction_path(lj, sp, saddles, masses=mass(EQUAL), **LJ_KW) for _ in range(2)]
    paths.append(follow_reaction_path(lj, sp, saddles, masses=mass(UNEQUAL), **LJ_KW))
    _LJ4["out"] = (lj, sp, saddles, paths)
    return _LJ4["out"]


def _branches(path, c):
    """The two branches of entry c from the saddle outwards: (coordinates, energies, arc lengths), the saddle first."""
    P = (path.energies.shape[1] - 1) // 2
    x, e, s = path.coordinates[c].cpu().numpy(), path.energies[c].cpu().numpy(), path.arc_lengths[c].cpu().numpy()
    nf, nb = int(path.n_forward[c]), int(path.n_backward[c])
    fwd = slice(P, P + nf + 1)
    bwd = slice(P, P - nb - 1 if P - nb - 1 >= 0 else None, -1)
    return (x[fwd], e[fwd], s[fwd]), (x[bwd], e[bwd], -s[bwd])


@pytest.mark.parametrize("which", ["equal", "unequal"])
def test_lj4_paths_reach_the_tetrahedron(dev, which):
    lj, sp, saddles, paths = _lj4(dev)
    path, masses = (paths[0], EQUAL) if which == "equal" else (paths[2], UNEQUAL)
    P = LJ_KW["max_points"]
    assert path.coordinates.shape == (4, 2 * P + 1, 4, 3) and path.energies.shape == path.arc_lengths.shape == (4, 2 * P + 1)
    assert path.coordinates.dtype == saddles.coordinates.dtype and path.reasons.shape == (4, 2)
    assert torch.equal(path.coordinates[:, P], saddles.coordinates.float().to(saddles.coordinates.dtype))
    assert not path.arc_lengths[:, P].any()
    ends, counts = [], []
    for c in range(4):
        nf, nb = int(path.n_forward[c]), int(path.n_backward[c])
        counts.append((nf, nb))
        # the NaN layout: exactly the slots P - nb .. P + nf are used
        used = torch.zeros(2 * P + 1, dtype=torch.bool)
        used[P - nb:P + nf + 1] = True
        assert torch.equal(~torch.isnan(path.energies[c]).cpu(), used) and torch.equal(~torch.isnan(path.arc_lengths[c]).cpu(), used)
        assert torch.equal(~torch.isnan(path.coordinates[c]).any(dim=-1).any(dim=-1).cpu(), used)
        for side, (x, e, s) in enumerate(_branches(path, c)):
            assert int(path.reasons[c, side]) in (MINIMUM, ENERGY_ROSE)
            assert abs(e[-1] + 6.0) <= 6e-5, (c, side, e[-1])        # the gate of the descent test of test_gpu_saddle.py
            ends.append(e[-1])
            de = np.diff(e)
            assert np.all((de < 0.0) | (np.abs(de) <= LJ_KW["energy_floor"])), (c, side, de.max())
            assert np.all(np.diff(s) > 0.0) and s[0] == 0.0
    report(f"irc LJ4 masses {masses}: points (forward, backward) {counts}, reasons {path.reasons.cpu().tolist()}, path lengths "
           f"{[round(float(np.nanmax(np.abs(path.arc_lengths[c].cpu().numpy()))), 4) for c in range(4)]}, worst E_end + 6 = "
           f"{max(abs(v + 6.0) for v in ends):.1e}")


@pytest.mark.parametrize("which", ["equal", "unequal"])
def test_lj4_chords_stay_below_the_arc_increments(dev, which):
    """The chord of every step, in mass-weighted length, is at most its arc increment (1 + 1e-6): the path is a curve.

    The stored points are fp32, whose spacing at |x| = 0.56 is 6e-8 A, and the follower keeps landing (forces still above
    fmax = 1e-5) until its steps are 1e-7 long: there the rounding of the coordinates is all of the chord.  The step kernel
    therefore hands commit an arc increment that is never below the chord between the two points it stores (include/anihip.h).
    Measured on the MI355X: worst chord / increment 1 + 0 over the 209 steps with equal masses, 1 + 2.0e-15 over the 449 with
    unequal ones; with the model's arc alone one step of the 209 (increment 1.37e-7, chord 1.39e-7) was over the gate."""
    lj, sp, saddles, paths = _lj4(dev)
    path, masses = (paths[0], EQUAL) if which == "equal" else (paths[2], UNEQUAL)
    sm = np.sqrt(np.array(masses))[None, :, None]
    worst_chord = worst_long = 0.0
    over, n_steps = [], 0
    for c in range(4):
        for side, (x, e, s) in enumerate(_branches(path, c)):
            ds = np.diff(s)
            chord = np.sqrt(((sm * np.diff(x.astype(np.float64), axis=0)) ** 2).sum(axis=(1, 2)))
            n_steps += len(ds)
            worst_chord = max(worst_chord, (chord / ds).max())
            worst_long = max(worst_long, (chord[ds >= 1e-3] / ds[ds >= 1e-3]).max())
            over += [(c, side, float(ds[k]), float(chord[k] / ds[k] - 1.0)) for k in range(len(ds))
                     if chord[k] > ds[k] * (1.0 + 1e-6)]
    report(f"irc LJ4 masses {masses}: worst chord / arc increment = 1 + {worst_chord - 1.0:.1e} over all {n_steps} steps, 1 + "
           f"{worst_long - 1.0:.1e} over the steps of at least 1e-3; steps over the gate (entry, side, increment, excess): {over}")
    assert not over


def test_lj4_paths_are_reproducible_and_depend_on_the_masses(dev):
    lj, sp, saddles, (first, again, unequal) = _lj4(dev)
    for a, b in zip(first, again):   # no atomics on this path: two runs agree bit for bit (NaN slots alike)
        assert _same(a, b)
    P = LJ_KW["max_points"]
    d = (first.coordinates[:, P + 3] - unequal.coordinates[:, P + 3]).abs().amax().item()
    assert d > 1e-3, d   # the third point already lies elsewhere ...
    for c in range(4):   # ... and the ends are the same minimum
        for (_, e0, _), (_, e1, _) in zip(_branches(first, c), _branches(unequal, c)):
            assert abs(e0[-1] - e1[-1]) <= 1.2e-4 and abs(e1[-1] + 6.0) <= 6e-5


def _interpolate(s, e, at):
    """Cubic interpolation of e(s) through the four nearest points of the path."""
    out = np.empty(len(at))
    for k, v in enumerate(at):
        i = int(np.clip(np.searchsorted(s, v) - 2, 0, len(s) - 4))
        out[k] = np.polyval(np.polyfit(s[i:i + 4] - v, e[i:i + 4], 3), 0.0)
    return out


@pytest.mark.parametrize("hessian_every", [5, 1])
def test_lj4_path_energies_against_the_fine_fp64_path(dev, hessian_every):
    """The energy along the path at equal arc length against the fp64 reference path of step 0.0125 (exact Hessians at every
    point).  The method's own error is the same deviation of the fp64 reference path of step 0.05 with the follower's Hessian
    schedule; the GPU path (fp32 energies and coordinates) may deviate by twice that plus 1e-5 eps.

    Measured: with exact Hessians at every point the fp64 path of step 0.05 deviates by 1.485e-2 eps (24 points, length
    1.0639), the GPU paths by 1.485e-2; with the default hessian_every = 5 (Bofill updates in between) the fp64 path deviates by
    3.619e-2 eps (26 points, length 1.0673) and the GPU paths by 3.619e-2.  So the GPU path is the reference's to 3e-6 eps on
    either schedule, and the default schedule itself costs 2.4 times the deviation of exact Hessians: held against the gate
    from exact Hessians (2.97e-2) the default run would miss it, by the method and not by the device."""
    from torchani_amd.geomopt import follow_reaction_path

    lj, sp, saddles, paths = _lj4(dev)
    if hessian_every == 5:
        path = paths[0]
    else:
        path = follow_reaction_path(lj, sp, saddles, masses=torch.ones((4, 4), dtype=torch.float64, device=dev),
                                    hessian_every=hessian_every, **LJ_KW)
    x0, e0, mode = lj4_saddle()
    fine = run_lj_path(x0, mode, EQUAL, 0.0125, fmax=1e-6)
    coarse = run_lj_path(x0, mode, EQUAL, 0.05, fmax=LJ_FMAX, energy_floor=LJ_KW["energy_floor"], hessian_every=hessian_every)
    fs, fe = np.array([0.0] + fine.path_s[0]), np.array([e0] + fine.path_e[0])

    def deviation(s, e):
        inside = s <= fs[-1]
        d = np.abs(_interpolate(fs, fe, s[inside]) - e[inside])
        return max(d.max(), np.abs(e[~inside] - fe[-1]).max() if (~inside).any() else 0.0)

    own = deviation(np.array([0.0] + coarse.path_s[0]), np.array([e0] + coarse.path_e[0]))
    gate = 2.0 * own + 1e-5
    worst = 0.0
    for c in range(4):
        for x, e, s in _branches(path, c):
            worst = max(worst, deviation(s, e))
    report(f"irc LJ4 energy along the path against the fp64 path of step 0.0125 at equal arc length, hessian_every "
           f"{hessian_every}: the fp64 path of step 0.05 deviates by {own:.3e} eps ({coarse.n_points[0]} points, length "
           f"{coarse.arc[0]:.4f}), the GPU paths by at most {worst:.3e} eps (gate {gate:.3e})")
    assert worst <= gate


# ---- fixed atoms, copies, refusals -----------------------------------------------------------------------------------------

def test_fixed_atoms_never_move_and_result_is_a_copy(dev):
    from torchani_amd.geomopt import ReactionPathFollower

    model, sp, x, cell, pbc, masses = _ani_case("rand_batch_ani2x", dev)
    fixed = torch.zeros_like(sp, dtype=torch.bool)
    fixed[:, :2] = True
    opt = ReactionPathFollower(model, sp, x, cell, pbc, masses=masses, fixed=fixed, hessian_every=2, step=LOCKSTEP_STEP,
                               max_points=8)
    x0 = opt.coordinates.clone()
    still = fixed | (sp < 0)
    for _ in range(4):
        opt.step()
        assert torch.all(opt.last_step[still] == 0)
    assert torch.equal(opt.coordinates[still], x0[still])
    assert int(opt.n_points.sum()) > 0 and not bool(opt.status.any())
    n = opt.n_points.cpu()
    for c in range(sp.shape[0]):
        assert torch.equal(opt.path_coordinates[c, :n[c]][:, still[c]], x0[c][still[c]].expand(int(n[c]), -1, -1))
    res = opt.result()
    kept = [t.clone() for t in res]
    opt.step()
    assert all(_same(a, b) for a, b in zip(res, kept))
    assert int(opt.n_points.sum()) > int(kept[3].sum())


def test_device_refusals(dev):
    from torchani_amd.geomopt import SADDLE_MAX_COORDS, CVConstraints, ReactionPathFollower, follow_reaction_path
    from torchani_amd.md_bias import distance
    from torchani_amd.models import ANI2dr

    model, sp, x, cell, pbc, masses = _ani_case("rand_batch_ani2x", dev)
    with pytest.raises(NotImplementedError, match="TwoBodyDispersionD3"):
        ReactionPathFollower(ANI2dr(seed=0, n_members=2, device=dev, periodic_table_index=False), sp, x, masses=masses)
    with pytest.raises(NotImplementedError, match="constraints"):
        ReactionPathFollower(model, sp, x, masses=masses, constraints=CVConstraints([distance(0, 1)]))
    big = SADDLE_MAX_COORDS // 3 + 1
    with pytest.raises(ValueError, match="SADDLE_MAX_COORDS"):
        ReactionPathFollower(model, torch.zeros((1, big), dtype=torch.int64, device=dev), torch.zeros((1, big, 3), device=dev))
    with pytest.raises(ValueError, match="pass masses"):
        ReactionPathFollower(model, sp, x)   # (species are element indices: no default masses)
    try:
        model.requires_grad_(True)
        with pytest.raises(RuntimeError, match="frozen parameters"):
            ReactionPathFollower(model, sp, x, masses=masses)
    finally:
        model.requires_grad_(False)
    with pytest.raises(ValueError, match="ROCm"):
        ReactionPathFollower(model, sp.cpu(), x.cpu(), masses=masses.cpu())
    lj, lsp, saddles, _ = _lj4(dev)
    wrong = saddles._replace(n_negative=torch.tensor([1, 1, 0, 1], device=dev))
    with pytest.raises(ValueError, match="entry 2 is not a first-order saddle"):
        follow_reaction_path(lj, lsp, wrong, masses=torch.ones((4, 4), device=dev))
