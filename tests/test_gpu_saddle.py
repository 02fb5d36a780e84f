"""Saddle-point search (torchani_amd.geomopt.SaddleOptimizer, anihip_saddle_*) on the MI355X: the three entry points alone
against the fp64 reference (tests/_saddle_ref.py) on synthetic Hessians, gradients and coordinates; lock-step parity of whole
steps on a padded ANI-2x batch and a periodic box; the D2h saddle of the four-atom Lennard-Jones cluster through the public
interface, checked by an independent fp64 Hessian, vibrational analysis and the descent to the two minima; refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from _saddle_ref import LJ4_SADDLE, SaddleReference, bofill, lj4_diamond, lj_hessian, rigid_basis
from _util import load_golden, seeded_state

pytestmark = pytest.mark.gpu

REPORT = os.environ.get("TORCHANI_AMD_SADDLE_REPORT")
PARITY = 1e-4   # max |last_step - s_ref| <= PARITY * max |s_ref|, per molecule and step: the gate of the L-BFGS lock-step
# The kernels alone, on synthetic inputs of order one with separated spectra: both sides are fp64 and round the displacement to
# fp32 at the end, so they differ by one fp32 rounding of an element (6e-8 of it) plus fp64 noise amplified by the eigenvalue
# gaps (>= 1e-3 here: 1e-13 / 1e-3).
KERNEL_PARITY = 1e-6
# fp64 noise of the Bofill update: xi = y - H s cancels to ~1e-16 |H| |s|, the coefficients divide by |xi| |s| and |s|^2, so the
# update is off by ~1e-14 of the largest element of the updated Hessian; four orders of margin, as PARITY has.
HESSIAN_PARITY = 1e-9
# A backward-stable symmetric eigensolver is off by ~n eps |H'| <= 1e-13 mu; three orders of margin.
EIGENVALUE_PARITY = 1e-10
LJ_FMAX = 1e-5   # the fp32 floor of Lennard-Jones forces argued in test_gpu_geomopt.py


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

TRUST, MAX_TRUST, MIN_TRUST, FLOOR = 0.05, 0.15, 1e-4, 1e-7


class Raw:
    """Device state of anihip_saddle for kind [C, A], x, f [C, A, 3], e [C], H [C, n, n], trust [C] (numpy)."""

    def __init__(self, dev, kind, x, f, e, H, trust, periodic, fmax=1e-6, mode=None, converged=None):
        from torchani_amd import _lib
        from torchani_amd.geomopt import saddle_workspace_bytes

        self.lib, self._lib = _lib.lib(), _lib
        Cn, A = kind.shape
        n = 3 * A
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt).contiguous()   # noqa: E731
        self.kind = t(kind, torch.uint8)
        self.x, self.f = t(x, torch.float32), t(f, torch.float32)
        self.e, self.H, self.trust = t(e, torch.float64), t(H, torch.float64), t(trust, torch.float64)
        self.eig = torch.zeros(Cn, dtype=torch.float64, device=dev)
        self.modes = torch.zeros((Cn, n), dtype=torch.float64, device=dev) if mode is None else t(mode, torch.float64)
        self.last = torch.full((Cn, A, 3), 7.0, dtype=torch.float32, device=dev)
        self.accepted = torch.zeros(Cn, dtype=torch.bool, device=dev)
        self.converged = torch.zeros(Cn, dtype=torch.bool, device=dev) if converged is None else t(converged, torch.bool)
        self.n_steps = torch.zeros(Cn, dtype=torch.int32, device=dev)
        self.n_rejected = torch.zeros(Cn, dtype=torch.int32, device=dev)
        self.status = torch.zeros(Cn, dtype=torch.int32, device=dev)
        self.ws = torch.zeros(saddle_workspace_bytes(Cn, A), dtype=torch.uint8, device=dev)
        self.projected = torch.eye(n, dtype=torch.float64, device=dev).repeat(Cn, 1, 1)
        self.st = _lib.Saddle(Cn, A, int(periodic), int(mode is not None), fmax, MAX_TRUST, MIN_TRUST, FLOOR, self.kind.data_ptr(),
                              self.x.data_ptr(), self.e.data_ptr(), self.f.data_ptr(), self.H.data_ptr(), self.trust.data_ptr(),
                              self.eig.data_ptr(), self.modes.data_ptr(), self.last.data_ptr(), self.accepted.data_ptr(),
                              self.converged.data_ptr(), self.n_steps.data_ptr(), self.n_rejected.data_ptr(),
                              self.status.data_ptr(), self.ws.data_ptr(), self.ws.numel())

    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    def project(self):
        self._lib.check(self.lib.anihip_saddle_project(self.stream(), C.byref(self.st), self.projected.data_ptr()))

    def step(self, lam=None, V=None):
        if lam is None:
            lam, V = torch.linalg.eigh(self.projected)
        self.lam, self.V = lam.contiguous(), V.contiguous()
        self._lib.check(self.lib.anihip_saddle_step(self.stream(), C.byref(self.st), self.lam.data_ptr(), self.V.data_ptr()))

    def accept(self, e_new, f_new, update):
        self.e_new = torch.from_numpy(np.ascontiguousarray(e_new)).to(self.x.device, torch.float64)
        self.f_new = torch.from_numpy(np.ascontiguousarray(f_new)).to(self.x.device, torch.float32).contiguous()
        self._lib.check(self.lib.anihip_saddle_accept(self.stream(), C.byref(self.st), self.e_new.data_ptr(),
                                                      self.f_new.data_ptr(), int(update)))


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


def _variants(A, rs):
    """Four molecules: plain with a negative lowest mode and a small radius (clipped), plain and positive definite with a
    large radius (not clipped), the last atoms padding, the first atom fixed."""
    kinds, xs, fs, Hs = [], [], [], []
    for v, lowest in enumerate((-0.7, 0.3, -0.4, -0.9)):
        x, f, H = _synthetic(A, rs, lowest)
        kind = np.ones(A, dtype=np.uint8)
        if v == 2:
            kind[A - max(1, A // 3):] = 0
        if v == 3:
            kind[0] = 2
        kinds.append(kind), xs.append(x), fs.append(f), Hs.append(H)
    trust = np.array([0.01, 50.0, TRUST, TRUST])
    return np.stack(kinds), np.stack(xs), np.stack(fs), np.stack(Hs), trust


def _reference(kind, periodic, trust, fmax=1e-6, follow="lowest", mode=None):
    ref = SaddleReference(kind, periodic, follow, TRUST, MAX_TRUST, MIN_TRUST, FLOOR, fmax, mode=mode)
    ref.trust = np.asarray(trust, dtype=np.float64).copy()
    return ref


def _check_move(raw, ref, dr, x0, gate=KERNEL_PARITY):
    """last_step against the reference's displacement, the coordinates moved by exactly last_step, eigenvalues."""
    got = raw.last.cpu().numpy().astype(np.float64)
    worst = 0.0
    for c in range(dr.shape[0]):
        scale = np.abs(dr[c]).max()
        err = np.abs(got[c] - dr[c]).max()
        if scale == 0.0:
            assert err == 0.0, c
            continue
        worst = max(worst, err / scale)
        assert err <= gate * scale, (c, err / scale)
        mu = 1.0 + np.abs(ref.H[c]).sum(axis=1).max()
        assert abs(raw.eig[c].item() - ref.eigenvalues[c]) <= EIGENVALUE_PARITY * mu, c
    x1 = (torch.from_numpy(x0).to(raw.x.device, torch.float32) + raw.last)
    assert torch.equal(raw.x, x1)
    return worst


@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("A", [1, 2, 3, 4, 21, 22, 86])
def test_entry_points_against_reference(dev, A, periodic):
    """One whole step of four molecules (see _variants) through the raw entry points: the projection and the step against the
    reference, then accept with made-up new energies that hit every branch of the ratio test, and the Bofill update."""
    rs = np.random.RandomState(100 + A)
    kind, x, f, H, trust = _variants(A, rs)
    e = rs.uniform(-1.0, 1.0, 4)
    raw = Raw(dev, kind, x, f, e, H, trust, periodic)
    x32 = raw.x.cpu().numpy()
    f32 = raw.f.cpu().numpy()
    ref = _reference(kind, periodic, trust)
    raw.project()
    raw.step()
    dr = ref.propose(x32, e, f32, H)
    assert raw.status.cpu().tolist() == [0, 0, 0, 0]
    assert np.array_equal(raw.converged.cpu().numpy(), ref.converged)
    worst = _check_move(raw, ref, dr, x32)
    moved = [c for c in range(4) if ref.pending[c] is not None]
    if A >= 3:   # (one or two atoms leave some variants without an internal coordinate: they are the zero-step cases)
        lams = [ref.eigenvalues[c] for c in moved]
        assert len(moved) == 4 and min(lams) < 0 < max(lams)          # both signs of the followed eigenvalue
        assert ref.pending[0][3] == trust[0]                          # the radius clips ...
        assert (A == 3 and not periodic) or ref.pending[1][3] < trust[1]   # ... and does not (A = 3, open: a 50 A step, clipped too)
    if A >= 21:   # (enough coordinates for the synthetic spectrum to survive the projection: the signs as constructed)
        assert ref.eigenvalues[0] < 0 < ref.eigenvalues[1]
    # new energies: rho = 1 (the radius may grow), 0.6 (kept), 0.1 (halved), 2.5 (rejected)
    rho = np.array([1.0, 0.6, 0.1, 2.5])
    e_new = e.copy()
    for c in moved:
        e_new[c] = e[c] + rho[c] * ref.pending[c][2]
        assert A <= 2 or abs(ref.pending[c][2]) > FLOOR
    f_new = f32 + rs.uniform(-0.05, 0.05, f32.shape).astype(np.float32)
    x_moved = raw.x.clone()
    raw.accept(e_new, f_new, True)
    ref.judge(e_new, f_new, True)
    assert np.array_equal(raw.accepted.cpu().numpy(), ref.accepted)
    assert np.array_equal(raw.n_steps.cpu().numpy(), ref.n_steps) and np.array_equal(raw.n_rejected.cpu().numpy(), ref.n_rejected)
    assert np.array_equal(raw.trust.cpu().numpy(), ref.trust)
    assert raw.status.cpu().tolist() == [0, 0, 0, 0]
    Hd = raw.H.cpu().numpy()
    worst_h = 0.0
    for c in range(4):
        if ref.accepted[c]:   # committed
            assert raw.e[c].item() == e_new[c] and torch.equal(raw.f[c].cpu(), torch.from_numpy(f_new[c]))
            assert torch.equal(raw.x[c], x_moved[c])
        else:                 # rejected or frozen: x, e, f bit for bit those of before
            assert raw.e[c].item() == e[c] and np.array_equal(raw.f[c].cpu().numpy(), f32[c])
            assert np.array_equal(raw.x[c].cpu().numpy(), x32[c])
            assert np.array_equal(Hd[c], H[c])
        err = np.abs(Hd[c] - ref.H[c]).max() / np.abs(ref.H[c]).max()
        worst_h = max(worst_h, err)
        assert err <= HESSIAN_PARITY, (c, err)
        assert np.array_equal(Hd[c], Hd[c].T)
    if A > 2:
        assert ref.accepted.tolist() == [True, True, True, False]
        assert ref.trust.tolist() == [0.02, 50.0, TRUST / 2, TRUST / 4]
    report(f"saddle entry points A = {A}, periodic {periodic}: worst |d last_step| / max |s_ref| = {worst:.1e}, "
           f"worst |d H| / max |H| after Bofill = {worst_h:.1e}")


def _diagonal_case(A=4):
    """Nothing to project (a fixed atom, periodic): H' is diagonal and the eigenvectors are unit vectors, exactly."""
    n = 3 * A
    kind = np.ones((1, A), dtype=np.uint8)
    kind[0, A - 1] = 2
    diag = np.concatenate([[-1.0, -0.5, 0.25, 0.5], np.arange(1.0, n - 3)])
    H = np.diag(diag)
    x = np.arange(n, dtype=np.float64).reshape(1, A, 3) * 0.25 + 1.0
    return kind, x, H[None], diag


def _unit_eigenpairs(raw, dev):
    d = torch.diagonal(raw.projected[0]).cpu().numpy()
    assert np.array_equal(raw.projected[0].cpu().numpy(), np.diag(d))
    perm = np.argsort(d, kind="stable")
    V = np.eye(d.size)[:, perm]
    return torch.from_numpy(d[perm][None]).to(dev), torch.from_numpy(V[None]).to(dev)


def test_zero_gradient_components(dev):
    """Exact zeros: g = 0 (no step, accepted below the energy floor, the Bofill update skipped for s = 0); g~_k = 0 (no step along
    the followed mode); a mode with g~_i = 0 below the others (it neither moves nor enters the bracket of the shift)."""
    kind, x, H, diag = _diagonal_case()
    A = kind.shape[1]
    n = 3 * A
    f = np.zeros((3, A, 3))
    f[1].reshape(-1)[[2, 3, 5]] = [0.2, -0.1, 0.3]            # g~_0 = 0: the followed mode has no gradient
    f[2].reshape(-1)[[0, 2, 4]] = [0.1, 0.2, -0.15]           # g~_1 = 0 at lam_1 = -0.5, below the other modes with a gradient
    kind3, x3, H3 = np.repeat(kind, 3, 0), np.repeat(x, 3, 0), np.repeat(H, 3, 0)
    e = np.zeros(3)
    raw = Raw(dev, kind3, x3, f, e, H3, np.full(3, 5.0), True, fmax=0.0)
    raw.project()
    lam, V = _unit_eigenpairs(raw, dev)
    raw.step(lam.repeat(3, 1), V.repeat(3, 1, 1))
    ref = _reference(kind3, True, np.full(3, 5.0), fmax=0.0)
    dr = ref.propose(x3, e, f, H3)
    _check_move(raw, ref, dr, x3.astype(np.float32).astype(np.float64))
    last = raw.last.cpu().numpy().reshape(3, n)
    assert not last[0].any()
    assert last[1][0] == 0.0 and last[1][[2, 3, 5]].all()
    assert last[2][1] == 0.0 and last[2][[0, 2, 4]].all()
    # lam_0 = -1 is climbed: s_0 = -g_0 / (lam_0 - gp) has the sign of g_0 = -f_0; the others descend
    assert last[2][0] < 0 and last[2][2] > 0 and last[2][4] < 0
    Hb = raw.H.clone()
    raw.accept(np.array([0.0, 1.0, -1.0]), f.astype(np.float32) * 0.5, True)
    assert raw.accepted.cpu().tolist()[0] and raw.n_steps.cpu().tolist()[0] == 1   # |predicted| = 0 < energy_floor
    assert torch.equal(raw.H[0], Hb[0]) and raw.trust[0].item() == 5.0
    assert raw.status.cpu().tolist() == [0, 0, 0]


def test_bofill_with_xi_orthogonal_to_s(dev):
    """xi . s = 0 exactly: phi = 0, the update is the symmetric Powell term alone."""
    kind, x, H, diag = _diagonal_case()
    A = kind.shape[1]
    n = 3 * A
    f = np.zeros((1, A, 3))
    f[0, 0, 0] = 0.25                                          # a gradient along coordinate 0 only: s = (s_0, 0, ...)
    raw = Raw(dev, kind, x, f, np.zeros(1), H, np.array([0.03125]), True, fmax=0.0)
    raw.project()
    raw.step(*_unit_eigenpairs(raw, dev))
    s = (raw.x.double() - torch.from_numpy(x).to(dev).float().double()).cpu().numpy().reshape(n)
    assert s[0] != 0.0 and not s[1:].any()
    # y_0 = H_00 s_0 = -s_0 exactly (f_0 - f'_0 with f'_0 = 0), so xi_0 = 0; xi_j = y_j elsewhere on the active coordinates
    f_old = np.zeros(n, dtype=np.float32)
    f_old[0] = np.float32(-s[0])
    assert float(f_old[0]) == -s[0]
    raw.f.copy_(torch.from_numpy(f_old.reshape(1, A, 3)))
    f_new = np.zeros(n, dtype=np.float32)
    f_new[1:n - 3] = -np.linspace(0.1, 0.4, n - 4).astype(np.float32)
    f_new[n - 3:] = 9.0                                        # the fixed atom: not an active coordinate, no part in xi
    pred = -0.25 * s[0] - 0.5 * s[0] ** 2                      # g_0 s_0 + lam_0 s_0^2 / 2: rho = 1
    raw.accept(np.array([pred]), f_new.reshape(1, A, 3), True)
    assert raw.accepted.cpu().tolist() == [True]
    y = (f_old.astype(np.float64) - f_new.astype(np.float64))
    y[n - 3:] = 0.0
    xi = y - H[0] @ s
    assert xi @ s == 0.0 and xi[1:n - 3].all()
    want = H[0] + (np.outer(xi, s) + np.outer(s, xi)) / (s @ s)
    act = np.arange(n) < n - 3
    assert np.allclose(bofill(H[0][np.ix_(act, act)], s[act], y[act]), want[np.ix_(act, act)], rtol=0, atol=1e-12)
    got = raw.H[0].cpu().numpy()
    assert np.abs(got - want).max() <= HESSIAN_PARITY * np.abs(want).max()
    assert np.array_equal(got, got.T)


def test_all_converged_batch_changes_nothing(dev):
    rs = np.random.RandomState(5)
    kind, x, f, H, trust = _variants(4, rs)
    f *= 1e-9
    e = rs.uniform(-1.0, 1.0, 4)
    raw = Raw(dev, kind, x, f, e, H, trust, False, fmax=1e-6)
    before = [t.clone() for t in (raw.x, raw.f, raw.e, raw.H, raw.trust, raw.modes, raw.projected, raw.n_steps, raw.n_rejected)]
    raw.project()
    assert raw.converged.cpu().tolist() == [True] * 4
    raw.step()
    raw.accept(e + 1.0, raw.f.cpu().numpy() + 1.0, True)
    after = (raw.x, raw.f, raw.e, raw.H, raw.trust, raw.modes, raw.projected, raw.n_steps, raw.n_rejected)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert not raw.last.any() and not raw.accepted.any() and not raw.status.any()


def test_follow_by_overlap_and_status_bits(dev):
    """follow = 1 picks the mode of largest overlap with ``modes`` (here the third eigenvector of the projected Hessian); a
    kind above 2 and a force that is not finite set their bits, freeze their entries and leave the others alone."""
    rs = np.random.RandomState(8)
    A = 5
    kind, x, f, H, trust = _variants(A, rs)
    ref0 = _reference(kind, False, trust)
    ref0.propose(x.astype(np.float32), np.zeros(4), f.astype(np.float32), H)
    # the reference's own third mode, perturbed
    mode = np.zeros((4, 3 * A))
    for c in range(4):
        act = ref0.active(c)
        no_fixed = not np.any(kind[c] == 2)
        Q = rigid_basis(x[c].astype(np.float32).astype(np.float64)[kind[c] == 1], None, no_fixed, no_fixed)
        P = np.eye(act.sum()) - Q @ Q.T
        mu = 1.0 + np.abs(H[c]).sum(axis=1).max()
        lam, V = np.linalg.eigh(P @ H[c][np.ix_(act, act)] @ P + mu * Q @ Q.T)
        mode[c][act] = V[:, 2] + 0.05 * rs.randn(act.sum())
    bad_kind = kind.copy()
    bad_kind[2, 1] = 3
    bad_f = f.copy()
    bad_f[3, 1, 1] = np.inf
    raw = Raw(dev, bad_kind, x, bad_f, np.zeros(4), H, trust, False, mode=mode)
    raw.project()
    raw.step()
    from torchani_amd import _lib

    assert raw.status.cpu().tolist() == [0, 0, _lib.SADDLE_BAD_TABLE, _lib.SADDLE_NONFINITE]
    ref = _reference(kind[:2], False, trust[:2], follow="overlap", mode=mode[:2])
    dr = ref.propose(x[:2].astype(np.float32), np.zeros(2), f[:2].astype(np.float32), H[:2])
    got = raw.last.cpu().numpy().astype(np.float64)
    for c in range(2):
        assert np.abs(got[c] - dr[c]).max() <= KERNEL_PARITY * np.abs(dr[c]).max()
        assert ref.eigenvalues[c] > ref0.eigenvalues[c] and abs(raw.eig[c].item() - ref.eigenvalues[c]) < 1e-9
    assert not got[2:].any() and torch.equal(raw.x[2:].cpu(), torch.from_numpy(x[2:].astype(np.float32)))


# ---- whole steps in lock-step with the reference --------------------------------------------------------------------------

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
    return model, sp, x, cell, pbc


def _lockstep(model, sp, x, cell, pbc, hessian_every, n_steps):
    """Steps the optimizer phase by phase; before each step the reference receives the coordinates, energies, forces and, on
    exact steps, the Hessian read back from the device, and after the move the trial energies and forces.  Returns the worst
    |last_step - s_ref| / max |s_ref| and the number of (molecule, step) pairs compared and skipped."""
    from torchani_amd.geomopt import SaddleOptimizer

    opt = SaddleOptimizer(model, sp, x, cell, pbc, hessian_every=hessian_every)
    opt.fmax = 1e-4
    st = opt._state
    ref = SaddleReference(opt._kind.cpu().numpy(), bool(st.periodic), "lowest", TRUST, st.max_trust, st.min_trust, st.energy_floor,
                          opt.fmax)
    worst = worst_h = 0.0
    compared = skipped = 0
    for k in range(n_steps):
        opt._refresh_hessians()
        xk, ek, fk = opt.coordinates.cpu().numpy(), opt.energies.cpu().numpy(), opt.forces.cpu().numpy()
        Hk = opt.hessians.cpu().numpy()
        exact = k % hessian_every == 0
        if not exact:   # the Bofill updates of both sides since the last exact Hessian
            for c in range(sp.shape[0]):
                err = np.abs(Hk[c] - ref.H[c]).max() / np.abs(ref.H[c]).max()
                worst_h = max(worst_h, err)
                assert err <= HESSIAN_PARITY, (k, c, err)
        opt._move()
        dr = ref.propose(xk, ek, fk, Hk if exact else None)
        got = opt.last_step.cpu().numpy().astype(np.float64)
        assert np.array_equal(opt.converged.cpu().numpy(), ref.converged), k
        opt._judge()
        ref.judge(opt.trial_energies.cpu().numpy(), opt.trial_forces.cpu().numpy(), (k + 1) % hessian_every != 0)
        assert not bool(opt.status.any())
        for c in range(sp.shape[0]):
            if ref.pending[c] is None:
                assert not got[c].any(), (k, c)
                continue
            if ref.gap[c] <= 1e-6:   # the followed mode is not defined
                skipped += 1
                continue
            compared += 1
            scale = np.abs(dr[c]).max()
            err = np.abs(got[c] - dr[c]).max()
            worst = max(worst, err / scale)
            assert err <= PARITY * scale, (k, c, err / scale)
            mu = 1.0 + np.abs(ref.H[c]).sum(axis=1).max()
            assert abs(opt.eigenvalues[c].item() - ref.eigenvalues[c]) <= EIGENVALUE_PARITY * mu, (k, c)
        assert np.array_equal(opt.accepted.cpu().numpy(), ref.accepted), k
        assert np.array_equal(opt.n_steps.cpu().numpy(), ref.n_steps), k
        assert np.array_equal(opt.n_rejected.cpu().numpy(), ref.n_rejected), k
        assert np.array_equal(opt.trust_radii.cpu().numpy(), ref.trust), k
    assert skipped <= 0.1 * (compared + skipped)
    return worst, worst_h, compared, skipped, opt, ref


@pytest.mark.parametrize("hessian_every", [1, 4])
@pytest.mark.parametrize("base", ["rand_batch_ani2x", "water_pbc_ani2x"])
def test_lockstep(dev, base, hessian_every):
    model, sp, x, cell, pbc = _ani_case(base, dev)
    worst, worst_h, compared, skipped, opt, ref = _lockstep(model, sp, x, cell, pbc, hessian_every, 8)
    report(f"saddle lock-step {base}, hessian_every {hessian_every}, 8 steps: worst |d last_step| / max |s_ref| = {worst:.1e} "
           f"(gate {PARITY:.0e}), worst |d H| / max |H| between exact Hessians = {worst_h:.1e} (gate {HESSIAN_PARITY:.0e}), "
           f"{compared} pairs compared, {skipped} skipped; accepted steps {ref.n_steps.tolist()}, rejected "
           f"{ref.n_rejected.tolist()}, exact Hessians {opt.n_hessians.cpu().tolist()}")
    assert compared > 0 and ref.n_steps.sum() > 0
    assert opt.n_hessians.cpu().tolist() == [-(-8 // hessian_every)] * sp.shape[0]


# ---- the four-atom Lennard-Jones cluster through the public interface ------------------------------------------------------

_LJ4 = {}


def _lj4(dev):
    """Four diamond starts (0.002 sigma of noise, seeds 0 to 3) and the tetrahedral minimum, searched twice."""
    if "out" in _LJ4:
        return _LJ4["out"]
    from torchani_amd.geomopt import optimize_saddle
    from torchani_amd.potentials import LennardJones

    lj = LennardJones(("H",), eps=(1.0,), sigma=(1.0,)).to(dev)
    r = 2.0 ** (1.0 / 6.0)
    tetra = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) * r / np.sqrt(8.0)
    x = torch.from_numpy(np.stack([lj4_diamond(0.002, s) for s in range(4)] + [tetra])).to(dev)
    sp = torch.ones((5, 4), dtype=torch.int64, device=dev)
    runs = [optimize_saddle(lj, sp, x, fmax=LJ_FMAX, steps=60, negative_tol=1e-2) for _ in range(2)]
    _LJ4["out"] = (lj, sp, x, runs)
    return _LJ4["out"]


def test_lj4_saddle(dev):
    lj, sp, x, (res, again) = _lj4(dev)
    e = res.energies.cpu().numpy()
    report(f"saddle LJ4 diamonds + tetrahedron, fmax {LJ_FMAX:.0e}: converged {res.converged.cpu().tolist()}, n_steps "
           f"{res.n_steps.cpu().tolist()}, n_negative {res.n_negative.cpu().tolist()}, E - E_saddle "
           f"{(e[:4] - LJ4_SADDLE).tolist()}, E_min {e[4]}")
    assert res.converged.cpu().tolist() == [True] * 5
    assert res.n_negative.cpu().tolist() == [1, 1, 1, 1, 0]
    assert np.all(np.abs(e[:4] - LJ4_SADDLE) <= 1e-5 * abs(LJ4_SADDLE)), e[:4] - LJ4_SADDLE   # the gate of the LJ minima
    xs = res.coordinates.cpu().numpy()
    for c in range(4):   # an independent fp64 Hessian at the returned coordinates
        lam = np.linalg.eigvalsh(lj_hessian(xs[c]))
        assert (lam < -0.1).sum() == 1 and (np.abs(lam) < 1e-3).sum() == 6 and (lam > 10.0).sum() == 5, lam
    # the minimum: converged at once, index 0, never moved
    assert abs(e[4] + 6.0) < 1e-5 and int(res.n_steps[4]) == 0
    assert torch.equal(res.coordinates[4], x[4].float().double())
    # no atomics on this path: two runs agree bit for bit
    for a, b in zip(res, again):
        assert torch.equal(a, b)
    assert res.coordinates.dtype == x.dtype and res.modes.shape == (5, 4, 3)
    assert torch.allclose(res.modes.reshape(5, -1).norm(dim=1), torch.ones(5, dtype=torch.float64, device=dev))


def test_lj4_saddle_has_one_imaginary_mode(dev):
    from torchani_amd import grad

    lj, sp, _, (res, _) = _lj4(dev)
    H = grad.energies_forces_and_hessians(lj, sp[:1], res.coordinates[:1].clone()).hessians
    masses = torch.full((1, 4), 39.948, dtype=torch.float64, device=dev)
    f = grad.vibrational_analysis(masses, H.double()).freqs.cpu().numpy()
    top = np.abs(f).max()
    report(f"saddle LJ4: frequencies / highest {np.round(np.sort(f) / top, 4).tolist()}")
    assert (f < -0.03 * top).sum() == 1 and (np.abs(f) <= 0.02 * top).sum() == 6 and (f > 0.3 * top).sum() == 5


def test_descend_from_lj4_saddle_reaches_the_tetrahedron(dev):
    from torchani_amd.geomopt import descend_from_saddle

    lj, sp, _, (res, _) = _lj4(dev)
    four = type(res)(*(t[:4] for t in res))
    fwd, bwd = descend_from_saddle(lj, sp[:4], four, delta=0.05, fmax=LJ_FMAX, steps=2000, alpha=70.0)
    for side in (fwd, bwd):
        assert bool(side.converged.all())
        assert np.all(np.abs(side.energies.cpu().numpy() + 6.0) <= 6e-5), side.energies
    report(f"saddle LJ4 descent: forward {fwd.energies.cpu().tolist()} in {fwd.n_steps.cpu().tolist()} steps, backward "
           f"{bwd.energies.cpu().tolist()} in {bwd.n_steps.cpu().tolist()}")


def test_fixed_atoms_never_move_and_result_is_a_copy(dev):
    from torchani_amd.geomopt import SaddleOptimizer

    model, sp, x, cell, pbc = _ani_case("rand_batch_ani2x", dev)
    fixed = torch.zeros_like(sp, dtype=torch.bool)
    fixed[:, :2] = True
    opt = SaddleOptimizer(model, sp, x, cell, pbc, fixed=fixed, hessian_every=2)
    x0 = opt.coordinates.clone()
    for _ in range(4):
        opt.step()
        assert torch.all(opt.last_step[fixed | (sp < 0)] == 0)
    assert torch.equal(opt.coordinates[fixed | (sp < 0)], x0[fixed | (sp < 0)])
    assert int(opt.n_steps.sum()) > 0 and not bool(opt.status.any())
    res = opt.result()
    kept = [t.clone() for t in res]
    opt.step()
    assert all(torch.equal(a, b) for a, b in zip(res, kept))


def test_device_refusals(dev):
    from torchani_amd.geomopt import SADDLE_MAX_COORDS, CVConstraints, SaddleOptimizer
    from torchani_amd.md_bias import distance
    from torchani_amd.models import ANI2dr

    model, sp, x, cell, pbc = _ani_case("rand_batch_ani2x", dev)
    with pytest.raises(NotImplementedError, match="TwoBodyDispersionD3"):
        SaddleOptimizer(ANI2dr(seed=0, n_members=2, device=dev, periodic_table_index=False), sp, x)
    with pytest.raises(NotImplementedError, match="constraints"):
        SaddleOptimizer(model, sp, x, constraints=CVConstraints([distance(0, 1)]))
    big = SADDLE_MAX_COORDS // 3 + 1
    with pytest.raises(ValueError, match="SADDLE_MAX_COORDS"):
        SaddleOptimizer(model, torch.zeros((1, big), dtype=torch.int64, device=dev), torch.zeros((1, big, 3), device=dev))
    try:
        model.requires_grad_(True)
        with pytest.raises(RuntimeError, match="frozen parameters"):
            SaddleOptimizer(model, sp, x)
    finally:
        model.requires_grad_(False)
    with pytest.raises(ValueError, match="ROCm"):
        SaddleOptimizer(model, sp.cpu(), x.cpu())
