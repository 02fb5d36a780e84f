"""Internal-coordinate constraints of the batched L-BFGS (csrc/geom_constraints.hip, torchani_amd.geomopt.GeometryOptimizer(
constraints=...)) on the MI355X against the fp64 reference of tests/_geom_constraints_ref.py: the projection and the restore
through the C ABI, broken and singular tables, and the class in lock-step with the reference on ANI-2x, converging a dihedral
and a distance scan of a Lennard-Jones cluster in one batch against the SLSQP oracle, torsion_scan, bit-identical without
constraints, without host synchronization, and the error of run().

Gates, derived and not measured: projected forces one fp32 ulp of max(|f_i|, |(J^T lambda)_i|) per component (the kernel and
the reference round the same fp64 difference; their lambda differ by cond(G) x 2^-53 <= 1e-12 relative at the cond(G) <= 1e4
asserted beside every case, far inside half an fp32 ulp = 6e-8 relative); values 1e-11 of their size and multipliers 1e-11 of
the largest of the entry; restored coordinates one fp32 ulp of the reference's; iteration counts equal.  The oracle gates are
those found on the CPU (tests/test_geom_constraints_host.py)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _geom_constraints_ref as gr
import _md_bias_ref as br
from _geomopt_ref import LbfgsReference
from test_geom_constraints_host import ORACLE_DELTA, ORACLE_E_GATE, ORACLE_SLOPE_GATE
from test_gpu_geomopt import PARITY, _ani_case
from test_gpu_md_device import _state, _stream

pytestmark = pytest.mark.gpu

COND_MAX = 1e4
TOL, MAX_IT = 1e-8, 32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from torchani_amd import _lib

    _lib.lib()
    return torch.device("cuda:0")


def _cvs(spec, Cn):
    """md CVs from [(kind, {entry: atoms}), ...]: an entry that is not named does not have the constraint."""
    from torchani_amd import md

    out = []
    for kind, per_entry in spec:
        idx = torch.full((Cn, kind + 2), -1, dtype=torch.int64)
        for c, atoms in per_entry.items():
            idx[c] = torch.tensor(atoms)
        out.append({0: md.distance, 1: md.angle, 2: md.dihedral}[kind](*(idx[:, j].clone() for j in range(kind + 2))))
    return out


def _build(spec, Cn, A, active):
    from torchani_amd import geomopt

    t = geomopt.build_constraint_tables(torch.zeros((Cn, A), dtype=torch.int64), torch.from_numpy(~active.astype(bool)),
                                        geomopt.CVConstraints(_cvs(spec, Cn)))
    return gr.Tables(t.offset, t.kind, t.atoms, np.zeros(t.kind.numel()))


class Abi:
    """The C ABI on device copies of the tables; the outputs prefilled with NaN / -1 so that what is not written shows."""

    def __init__(self, dev, t, Cn, A, active, tolerance=TOL, max_iterations=MAX_IT):
        from torchani_amd import _lib

        self.lib, self._lib, self.dev, self.Cn, self.A = _lib.lib(), _lib, dev, Cn, A
        N = t.kind.shape[0]
        self.d = {"offset": torch.from_numpy(t.offset.astype(np.int32)).to(dev), "kind": torch.from_numpy(t.kind.astype(np.int32)).to(dev),
                  "atoms": torch.from_numpy(t.atoms.astype(np.int32)).to(dev).contiguous(),
                  "target": torch.from_numpy(t.target.astype(np.float64)).to(dev)}
        self.values = torch.full((N,), float("nan"), dtype=torch.float64, device=dev)
        self.multipliers = torch.full((N,), float("nan"), dtype=torch.float64, device=dev)
        self.iterations = torch.full((Cn,), -1, dtype=torch.int32, device=dev)
        self.status = torch.zeros(Cn, dtype=torch.int32, device=dev)
        self.active = torch.from_numpy(np.ascontiguousarray(active, dtype=np.uint8)).to(dev)
        self.g = _lib.GeomConstraints(N, max_iterations, tolerance, *(self.d[k].data_ptr() for k in ("offset", "kind", "atoms", "target")),
                                      self.values.data_ptr(), self.multipliers.data_ptr(), self.iterations.data_ptr(),
                                      self.status.data_ptr())

    def project(self, x32, f32):
        x = torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32)).to(self.dev)
        f = torch.from_numpy(np.ascontiguousarray(f32, dtype=np.float32)).to(self.dev)
        self.status.zero_()
        self._lib.check(self.lib.anihip_geom_constraints_project(_stream(), self.Cn, self.A, C.byref(self.g), self.active.data_ptr(),
                                                                 x.data_ptr(), f.data_ptr()))
        return {"forces": f.cpu().numpy(), "multipliers": self.multipliers.cpu().numpy(), "values": self.values.cpu().numpy(),
                "status": self.status.cpu().numpy()}

    def restore(self, x32):
        x = torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32)).to(self.dev)
        self.status.zero_()
        self._lib.check(self.lib.anihip_geom_constraints_restore(_stream(), self.Cn, self.A, C.byref(self.g), self.active.data_ptr(),
                                                                 x.data_ptr()))
        return {"coords": x.cpu().numpy(), "values": self.values.cpu().numpy(), "iterations": self.iterations.cpu().numpy(),
                "status": self.status.cpu().numpy()}


def _compare_project(got, want, f_in, what):
    """The gates of the module docstring; prints every figure before it asserts."""
    assert np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    assert want["cond"].max() <= COND_MAX, want["cond"]
    scale = np.maximum(np.abs(f_in.astype(np.float64)), np.abs(want["jtl"]))
    ulp = br.ulp32(scale)
    df = np.abs(got["forces"].astype(np.float64) - want["forces"].astype(np.float64))
    held = ~np.isnan(want["values"])
    assert np.array_equal(np.isnan(got["values"]), ~held) and np.array_equal(np.isnan(got["multipliers"]), ~held)
    dv = np.abs(got["values"][held] - want["values"][held]) / np.abs(want["values"][held])
    lam_scale = max(np.abs(want["multipliers"][held]).max(), 1e-300)
    dl = np.abs(got["multipliers"][held] - want["multipliers"][held]) / lam_scale
    print(f"geom constraints project, {what}: cond(G) per entry {[f'{c:.1e}' for c in want['cond']]}, forces within "
          f"{(df / ulp).max():.2f} fp32 ulp on {int((np.abs(want['jtl']).sum(-1) > 0).sum())} atoms (largest |J^T lambda| "
          f"{np.abs(want['jtl']).max():.2e}), values {dv.max():.1e}, multipliers {dl.max():.1e} relative")
    assert (df <= ulp).all()
    assert dv.max() <= 1e-11 and dl.max() <= 1e-11


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------

def _abi_spec(Cn, A):
    """Entries of 8, 0 and 1 constraints (3, 70), or 8 and 1 (2, 300) with atoms on both sides of atom 256.  The constraints of
    the first entry share atoms, and its atom 5 is fixed (test_gpu_md_device._state); so is atom 69 of the last entry of (3, 70)."""
    if A == 70:
        a = [3, 5, 9, 17, 33, 41, 58, 69]
        last, one = 2, (69, 12, 40)
    else:
        a = [3, 5, 250, 255, 256, 257, 270, 299]
        last, one = 1, (299 - 9, 10, 280)   # (the nine last atoms of the middle entry, which is the last one here, are padding)
    spec = [(0, {0: (a[0], a[1])}), (0, {0: (a[1], a[2])}), (1, {0: (a[0], a[2], a[3])}), (1, {0: (a[3], a[4], a[5]), last: one}),
            (2, {0: (a[0], a[3], a[4], a[6])}), (2, {0: (a[4], a[5], a[6], a[7])}), (0, {0: (a[6], a[7])}),
            (1, {0: (a[1], a[7], a[2])})]
    return spec, last


def _gather(x, rs):
    """The atoms of _state are scattered over 40 A; put them into a box of 10 A so that the constraints have arms of a few
    Angstrom, as in a molecule."""
    return rs.uniform(-5.0, 5.0, x.shape).astype(np.float32)


@pytest.mark.parametrize("Cn, A", [(3, 70), (2, 300)])
@pytest.mark.parametrize("zero_forces", [False, True])
def test_projection_matches_reference(dev, Cn, A, zero_forces):
    x, _, f0, _, _, active = _state(Cn, A)
    x = _gather(x, np.random.RandomState(4))
    f = np.zeros_like(f0, dtype=np.float32) if zero_forces else f0.astype(np.float32)
    spec, last = _abi_spec(Cn, A)
    t = _build(spec, Cn, A, active)
    assert [len(t.rows(c)) for c in range(Cn)] == ([8, 0, 1] if Cn == 3 else [8, 1]) and not active[0, 5]
    abi = Abi(dev, t, Cn, A, active)
    got, want = abi.project(x, f), gr.project(t, x, f, active)
    _compare_project(got, want, f, f"(C, A) = ({Cn}, {A}), {'zero' if zero_forces else 'random'} forces")
    named = np.zeros(Cn * A, dtype=bool)
    named[t.atoms[t.atoms >= 0]] = True
    assert np.array_equal(got["forces"].reshape(-1, 3)[~named], f.reshape(-1, 3)[~named])   # bit-identical
    assert np.array_equal(got["forces"][0, 5], f[0, 5])   # the anchor keeps its force
    if zero_forces:
        assert np.abs(got["forces"]).max() == 0.0 and np.abs(got["multipliers"]).max() == 0.0
    again = abi.project(x, f)
    for k in ("forces", "multipliers", "values"):
        assert np.array_equal(got[k], again[k], equal_nan=True), k


@pytest.mark.parametrize("Cn, A", [(3, 70), (2, 300)])
def test_restore_matches_reference(dev, Cn, A):
    """From displacements of up to 0.2 A (the optimizer's maxstep) off the targets."""
    x, _, _, _, _, active = _state(Cn, A)
    rs = np.random.RandomState(6)
    x = _gather(x, rs)
    spec, last = _abi_spec(Cn, A)
    t = _build(spec, Cn, A, active)
    d = rs.normal(size=x.shape)
    d *= rs.uniform(0.0, 0.2, x.shape[:2])[..., None] / np.linalg.norm(d, axis=-1, keepdims=True)
    x_on = (x.astype(np.float64) + d).astype(np.float32)
    for c in range(Cn):
        t.target[list(t.rows(c))] = gr.jacobian(t, c, x_on.astype(np.float64).reshape(-1, 3), active.reshape(-1))[0]
    abi = Abi(dev, t, Cn, A, active)
    got, want = abi.restore(x), gr.restore(t, x, active, TOL, MAX_IT)
    assert np.array_equal(got["status"], want["status"]) and not want["status"].any()
    has = np.array([len(t.rows(c)) > 0 for c in range(Cn)])
    assert np.array_equal(got["iterations"][has], want["iterations"][has]) and (got["iterations"][~has] == -1).all()
    assert want["iterations"][has].min() >= 2
    dx = np.abs(got["coords"].astype(np.float64) - want["coords"].astype(np.float64))
    ulp = br.ulp32(want["coords"])
    at_own = np.concatenate([gr.jacobian(t, c, got["coords"].astype(np.float64).reshape(-1, 3), active.reshape(-1))[0]
                             for c in range(Cn)])
    dv = np.abs(got["values"] - at_own) / np.abs(at_own)
    resid = np.concatenate([np.abs(gr.residual(t, c, got["values"][list(t.rows(c))].copy())) for c in range(Cn)])
    bound = np.concatenate([gr.residual_bound(t, c, got["coords"], TOL) for c in range(Cn)])
    print(f"geom constraints restore, (C, A) = ({Cn}, {A}): iterations {got['iterations'].tolist()}, coordinates within "
          f"{(dx / ulp).max():.2f} fp32 ulp, moved up to {np.abs(got['coords'] - x).max():.3f} A, values {dv.max():.1e} relative, "
          f"worst residual {resid.max():.1e} (bound {bound[resid.argmax()]:.1e})")
    assert (dx <= ulp).all() and dv.max() <= 1e-11 and (resid <= bound).all()
    named = np.zeros(Cn * A, dtype=bool)
    named[t.atoms[t.atoms >= 0]] = True
    assert np.array_equal(got["coords"].reshape(-1, 3)[~named], x.reshape(-1, 3)[~named])
    assert np.array_equal(got["coords"][0, 5], x[0, 5])   # the fixed atom
    again = abi.restore(x)
    for k in ("coords", "values", "iterations"):
        assert np.array_equal(got[k], again[k], equal_nan=True), k
    # already on the targets (those that the fp32 coordinates have): nothing is written but the values and a count of zero
    t.target[:] = got["values"]
    on = Abi(dev, t, Cn, A, active).restore(got["coords"])
    assert np.array_equal(on["coords"], got["coords"]) and (on["iterations"][has] == 0).all()
    assert np.array_equal(on["values"], got["values"]) and not on["status"].any()


def test_dihedral_is_restored_across_the_seam(dev):
    Cn, A = 3, 70
    x, _, _, _, _, active = _state(Cn, A)
    x = x.astype(np.float32)
    for c, (start, target) in enumerate([(math.pi - 0.03, -math.pi + 0.03), (-math.pi + 0.03, math.pi - 0.03),
                                         (math.pi - 0.04, math.pi)]):
        p = np.array([[-0.5, 1.0, 0.0], [0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [2.0, math.cos(start), math.sin(start)]])
        if abs(br.cv(br.DIHEDRAL, p)[0] - start) > 1e-9:
            p = p * np.array([1.0, 1.0, -1.0])
        x[c, [10, 20, 30, 40]] = (p + 3.0).astype(np.float32)
    t = _build([(2, {c: (10, 20, 30, 40) for c in range(Cn)})], Cn, A, active)
    t.target[:] = [-math.pi + 0.03, math.pi - 0.03, math.pi]
    got, want = Abi(dev, t, Cn, A, active).restore(x), gr.restore(t, x, active, TOL, MAX_IT)
    assert not got["status"].any() and np.array_equal(got["iterations"], want["iterations"]) and want["iterations"].min() >= 2
    assert (np.abs(got["coords"].astype(np.float64) - want["coords"]) <= br.ulp32(want["coords"])).all()
    for c in range(Cn):
        assert abs(br.wrap(got["values"][c] - t.target[c])) <= gr.residual_bound(t, c, got["coords"], TOL)[0]
    assert np.abs(got["coords"] - x).max() <= 0.1   # the short way round


def test_an_entry_gives_the_same_bits_wherever_it_sits(dev):
    Cn, A = 3, 70
    x, _, f0, _, _, active = _state(Cn, A)
    rs = np.random.RandomState(8)
    x, f = _gather(x, rs), f0.astype(np.float32)
    spec, _ = _abi_spec(Cn, A)
    moved = [(k, {2: per[0]}) for k, per in spec if 0 in per]   # the constraints of entry 0 on entry 2
    x2, f2, act2 = x.copy(), f.copy(), active.copy()
    x2[2], f2[2], act2[2] = x[0], f[0], active[0]
    ta, tb = _build(spec, Cn, A, active), _build(moved, Cn, A, act2)
    ta.target[:8] = tb.target[:] = gr.jacobian(ta, 0, x.astype(np.float64).reshape(-1, 3), active.reshape(-1))[0] + 0.05
    ta.target[8] = gr.jacobian(ta, 2, x.astype(np.float64).reshape(-1, 3), active.reshape(-1))[0][0]
    a, b = Abi(dev, ta, Cn, A, active), Abi(dev, tb, Cn, A, act2)
    pa, pb = a.project(x, f), b.project(x2, f2)
    assert np.array_equal(pa["forces"][0], pb["forces"][2]) and np.array_equal(pa["multipliers"][:8], pb["multipliers"])
    ra, rb = a.restore(x), b.restore(x2)
    assert ra["iterations"][0] == rb["iterations"][2] >= 2
    assert np.array_equal(ra["coords"][0], rb["coords"][2]) and np.array_equal(ra["values"][:8], rb["values"])


def _good(Cn, A):
    spec = [(0, {c: (3, 9) for c in range(Cn)}), (1, {c: (9, 17, 33) for c in range(Cn)})]
    return spec


BROKEN = ["offset falls", "offset spans nine", "offset past the end", "kind", "atom of another entry", "atom repeated",
          "atom missing", "redundant pair", "collinear angle", "max_iterations = 1"]


@pytest.mark.parametrize("what", BROKEN)
def test_broken_and_singular_entries_are_flagged_and_left_alone(dev, what):
    """The last entry is broken; it is flagged with exactly its bit and nothing of it is written, the others behave as if
    nothing were wrong (the same bits as with good tables)."""
    Cn, A = 3, 70
    x, _, f0, _, _, active = _state(Cn, A)
    rs = np.random.RandomState(9)
    x, f = _gather(x, rs), f0.astype(np.float32)
    t = _build(_good(Cn, A), Cn, A, active)
    # (targets that one Newton iteration reaches where only one is allowed: its error is quadratic, 1e-4^2 << 1e-8)
    max_it, off = (1, 1e-4) if what == "max_iterations = 1" else (MAX_IT, 0.05)
    for c in range(Cn):
        t.target[list(t.rows(c))] = gr.jacobian(t, c, x.astype(np.float64).reshape(-1, 3), active.reshape(-1))[0] + off
    good = Abi(dev, t, Cn, A, active, max_iterations=max_it)
    p0, r0 = good.project(x, f), good.restore(x)
    assert not p0["status"].any() and not r0["status"].any() and r0["iterations"].min() >= 1
    b = gr.Tables(t.offset.copy(), t.kind.copy(), t.atoms.copy(), t.target.copy())
    xb = x.copy()
    bits = (gr.BAD_TABLE, gr.BAD_TABLE)
    if what == "offset falls":
        b.offset[3] = b.offset[2] - 1
    elif what == "offset spans nine":
        extra = 9 - 2
        b.offset[3] = b.offset[2] + 9
        b.kind = np.concatenate([b.kind, np.zeros(extra, dtype=np.int64)])
        b.atoms = np.concatenate([b.atoms, np.tile(np.array([[2 * A + 1, 2 * A + 2, -1, -1]]), (extra, 1))])
        b.target = np.concatenate([b.target, np.ones(extra)])
    elif what == "offset past the end":
        b.offset[3] = b.offset[2] + 3
    elif what == "kind":
        b.kind[5] = 3
    elif what == "atom of another entry":
        b.atoms[5, 1] = A + 17
    elif what == "atom repeated":
        b.atoms[5, 2] = b.atoms[5, 0]
    elif what == "atom missing":
        b.atoms[5, 2] = -1
    elif what == "redundant pair":
        b.kind[5], b.atoms[5], b.target[5] = 0, [2 * A + 9, 2 * A + 3, -1, -1], b.target[4] + 0.01
        bits = (gr.SINGULAR, gr.SINGULAR)
    elif what == "collinear angle":
        xb[2, 17], xb[2, 33] = xb[2, 9] + np.float32(1.0) * np.array([1, 0, 0], np.float32), xb[2, 9] - np.array([2, 0, 0], np.float32)
        with np.errstate(all="ignore"):
            assert br.cv(br.ANGLE, xb[2, [9, 17, 33]].astype(np.float64))[0] == 0.0   # (y and z agree exactly: a x b = 0)
        b.target[5] = 3.0
        bits = (gr.SINGULAR, gr.SINGULAR)
    else:
        b.target[4] += 0.5   # far: one Newton iteration does not get there
        bits = (0, gr.NOT_CONVERGED)
    abi = Abi(dev, b, Cn, A, active, max_iterations=max_it)
    if what == "collinear angle":
        good = Abi(dev, t, Cn, A, active)
        p0, r0 = good.project(xb, f), good.restore(xb)   # (the others see the same coordinates)
    p, r = abi.project(xb, f), abi.restore(xb)
    wp, wr = gr.project(b, xb, f, active), gr.restore(b, xb, active, TOL, max_it)
    assert p["status"].tolist() == [0, 0, bits[0]] == wp["status"].tolist()
    assert r["status"].tolist() == [0, 0, bits[1]] == wr["status"].tolist()
    # the others: the bits of the good tables
    assert np.array_equal(p["forces"][:2], p0["forces"][:2]) and np.array_equal(p["multipliers"][:4], p0["multipliers"][:4])
    assert np.array_equal(r["coords"][:2], r0["coords"][:2]) and np.array_equal(r["values"][:4], r0["values"][:4])
    assert np.array_equal(r["iterations"][:2], r0["iterations"][:2])
    # the flagged entry: nothing written
    if bits[0]:
        assert np.array_equal(p["forces"][2], f[2]) and np.isnan(p["multipliers"][4:]).all()
    else:   # (the projection does not read the targets)
        assert np.array_equal(p["forces"][2], p0["forces"][2]) and np.array_equal(p["multipliers"][4:], p0["multipliers"][4:])
    assert np.array_equal(r["coords"][2], xb[2]) and r["iterations"][2] == -1
    # (the restore's own values: those of the projection are still there where the projection ran)
    vals = Abi(dev, b, Cn, A, active, max_iterations=max_it).restore(xb)["values"]
    assert np.isnan(vals[4:]).all()


def test_host_visible_errors_return_nonzero(dev):
    from torchani_amd import _lib

    Cn, A = 3, 70
    x, _, f0, _, _, active = _state(Cn, A)
    t = _build(_good(Cn, A), Cn, A, active)
    L = _lib.lib()
    xd, fd = torch.from_numpy(x.astype(np.float32)).to(dev), torch.from_numpy(f0.astype(np.float32)).to(dev)
    keep = xd.clone(), fd.clone()
    for kw, message in (({"tolerance": 0.0}, "tolerance must be > 0"), ({"max_iterations": 0}, "max_iterations must be >= 1")):
        abi = Abi(dev, t, Cn, A, active, **kw)
        for rc in (L.anihip_geom_constraints_project(_stream(), Cn, A, C.byref(abi.g), abi.active.data_ptr(), xd.data_ptr(), fd.data_ptr()),
                   L.anihip_geom_constraints_restore(_stream(), Cn, A, C.byref(abi.g), abi.active.data_ptr(), xd.data_ptr())):
            assert rc != 0 and message in L.anihip_last_error().decode()
    abi = Abi(dev, t, Cn, A, active)
    assert L.anihip_geom_constraints_project(_stream(), Cn, A, C.byref(abi.g), abi.active.data_ptr(), xd.data_ptr(), None) != 0
    assert L.anihip_geom_constraints_project(_stream(), Cn, A, None, abi.active.data_ptr(), xd.data_ptr(), fd.data_ptr()) != 0
    assert L.anihip_geom_constraints_restore(_stream(), Cn, A, C.byref(abi.g), None, xd.data_ptr()) != 0
    abi.g.target = None
    assert L.anihip_geom_constraints_restore(_stream(), Cn, A, C.byref(abi.g), abi.active.data_ptr(), xd.data_ptr()) != 0
    assert "null pointer" in L.anihip_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(xd, keep[0]) and torch.equal(fd, keep[1])


# ---- the class ----------------------------------------------------------------------------------------------------------------

def _spy(opt):
    """Keeps the unprojected forces of every evaluation and the coordinates in front of every restore."""
    seen = {"raw": None, "pre": None}
    model_eval, restore = opt._model_eval, opt._restore

    def evaluate(x):
        e, f = model_eval(x)
        seen["raw"] = f.clone()
        return e, f

    def restore_spy():
        seen["pre"] = opt.coordinates.clone()
        restore()

    evaluate.raise_on_overflow = model_eval.raise_on_overflow
    opt._model_eval, opt._restore = evaluate, restore_spy
    opt._evaluate()
    return seen


@pytest.mark.parametrize("base", ["rand_batch_ani2x", "water_pbc_ani2x"])
def test_lockstep_with_reference(dev, base):
    """20 steps; the reference is fed the device's x_k and unprojected f_k and reproduces the projected forces, last_step (the
    PARITY gate of test_gpu_geomopt), the restored coordinates, converged and n_steps."""
    from torchani_amd import geomopt, md

    model, sp, x, cell, pbc = _ani_case(base, dev)
    Cn, A = sp.shape
    fixed = torch.zeros(sp.shape, dtype=torch.bool, device=dev)
    fixed[0, 1] = True
    if base == "rand_batch_ani2x":
        assert bool((sp < 0).any()) and bool((sp[:, :7] >= 0).all())
        cvs = [md.distance(0, 1), md.angle(1, 2, 3), md.dihedral(0, 2, 4, 5), md.distance(torch.tensor([6, -1, 6, -1, 6, 6]), 3)]
    else:
        cvs = [md.distance(0, 1), md.angle(1, 0, 2), md.dihedral(1, 0, 3, 4), md.distance(0, 3)]   # O-H, H-O-H, and across waters
    d0 = (x[:, 0] - x[:, 1]).double().norm(dim=-1).cpu()
    cons = geomopt.CVConstraints(cvs)
    tab = geomopt.build_constraint_tables(sp, fixed, cons)
    opt = geomopt.GeometryOptimizer(model, sp, x, cell, pbc, memory=5, fixed=fixed, constraints=cons)
    t = gr.Tables(tab.offset, tab.kind, tab.atoms, opt._tables.target)
    assert abs(float(opt._tables.target[0]) - float(d0[0])) <= 1e-6   # targets None: the initial values
    active = ((sp >= 0) & ~fixed).cpu().numpy()
    seen = _spy(opt)
    p = opt._params
    ref = LbfgsReference(Cn, 5, p.maxstep, 1.0 / p.inv_alpha, p.damping, opt.fmax)
    worst = {"f": 0.0, "dr": 0.0, "x": 0.0}
    for k in range(20):
        xk, raw, fk = opt.coordinates.cpu().numpy(), seen["raw"].cpu().numpy(), opt.forces.cpu().numpy()
        want = gr.project(t, xk, raw, active)
        assert not want["status"].any() and want["cond"].max() <= COND_MAX
        ulp = br.ulp32(np.maximum(np.abs(raw.astype(np.float64)), np.abs(want["jtl"])))
        df = np.abs(fk.astype(np.float64) - want["forces"])
        worst["f"] = max(worst["f"], (df / ulp).max())
        assert (df <= ulp).all(), k
        lam = opt.constraint_multipliers().cpu().numpy()
        idx = tab.index.numpy()
        assert np.array_equal(np.isnan(lam), idx < 0)
        assert np.abs(lam[idx >= 0] - want["multipliers"][idx[idx >= 0]]).max() <= 1e-11 * np.abs(want["multipliers"]).max()
        opt.step()
        dr = ref.step(xk, fk, active)
        got = opt.last_step.cpu().numpy()
        assert np.array_equal(opt.converged.cpu().numpy(), ref.converged) and np.array_equal(opt.n_steps.cpu().numpy(), ref.n_steps), k
        for c in range(Cn):
            scale, err = np.abs(dr[c]).max(), np.abs(got[c] - dr[c]).max()
            assert err <= PARITY * scale, (k, c, err, scale)
            worst["dr"] = max(worst["dr"], err / scale if scale else 0.0)
        pre = seen["pre"].cpu().numpy()
        back = gr.restore(t, pre, active, TOL, MAX_IT)
        assert not back["status"].any()
        assert np.array_equal(opt.constraint_iterations.cpu().numpy(), back["iterations"]), k
        dx = np.abs(opt.coordinates.cpu().numpy().astype(np.float64) - back["coords"])
        worst["x"] = max(worst["x"], (dx / br.ulp32(back["coords"])).max())
        assert (dx <= br.ulp32(back["coords"])).all(), k
    held, x32 = opt.constraint_values().cpu().numpy(), opt.coordinates.cpu().numpy()
    for c in range(Cn):
        resid = np.abs(gr.residual(t, c, held[c][idx[c] >= 0].copy()))
        assert (resid <= gr.residual_bound(t, c, x32, TOL)).all(), (c, resid)
    assert not opt._geom_status.any()
    print(f"geom constraints lock-step {base}, 20 steps: projected forces within {worst['f']:.2f} fp32 ulp, last_step "
          f"{worst['dr']:.1e} of max |dr_ref| (gate {PARITY:.0e}), restored coordinates within {worst['x']:.2f} fp32 ulp; "
          f"restore iterations of the last step {opt.constraint_iterations.tolist()}")


_SCAN = {}
DIH, DIST = (0, 5, 6, 2), (5, 6)
SCAN_K = (-2, -1, 0, 1, 2)


def _lj(dev):
    from torchani_amd.potentials import LennardJones

    return LennardJones(("H",), eps=(gr.LJ_EPS,), sigma=(gr.LJ_SIGMA,)).to(dev)


def _scan(dev):
    """The bipyramid x 9: entries 0 .. 4 a dihedral scan about s0 + 0.05 in steps of ORACLE_DELTA, entries 5 .. 8 a distance
    scan about d0 + 0.06; relaxed in one batch from the minimum.  The SLSQP oracle of every entry, computed once."""
    if "out" in _SCAN:
        return _SCAN["out"]
    from torchani_amd import geomopt

    xm = gr.lj_minimum()
    s0, d0 = gr.cv_value(br.DIHEDRAL, DIH, xm), gr.cv_value(br.DISTANCE, DIST, xm)
    t_dih = [s0 + 0.05 + k * ORACLE_DELTA for k in SCAN_K]
    t_dist = [d0 + 0.06 + k * ORACLE_DELTA for k in (-1, 0, 1, 2)]
    cvs = _cvs([(2, {c: DIH for c in range(5)}), (0, {c: DIST for c in range(5, 9)})], 9)
    targets = [torch.tensor(t_dih + [0.0] * 4, dtype=torch.float64), torch.tensor([0.0] * 5 + t_dist, dtype=torch.float64)]
    sp = torch.ones((9, 7), dtype=torch.int64, device=dev)
    x = torch.from_numpy(np.tile(xm, (9, 1, 1))).to(dev)
    opt = geomopt.GeometryOptimizer(_lj(dev), sp, x, constraints=geomopt.CVConstraints(cvs, targets))
    out = opt.run(fmax=1e-5, steps=300)
    oracle = [gr.slsqp(xm, [(br.DIHEDRAL, DIH, t)])[0] for t in t_dih] + [gr.slsqp(xm, [(br.DISTANCE, DIST, t)])[0] for t in t_dist]
    _SCAN["out"] = (opt, out, np.array(oracle), t_dih, t_dist, xm)
    return _SCAN["out"]


def test_scans_converge_to_the_oracle(dev):
    opt, out, oracle, t_dih, t_dist, xm = _scan(dev)
    assert bool(out.converged.all()) and int(out.n_steps.max()) < 110
    E = out.energies.cpu().numpy()
    print(f"geom constraints LJ7 x 9, a dihedral and a distance scan: n_steps {out.n_steps.tolist()}, max |E - E_SLSQP| = "
          f"{np.abs(E - oracle).max():.1e} Ha (gate {ORACLE_E_GATE:.0e})")
    assert np.abs(E - oracle).max() <= ORACLE_E_GATE
    # residuals: bounded from the fp32 spacing of the coordinates (gr.residual_bound: sum_i |grad_i s| sqrt(3) / 2 ulp(max |x|)
    # on top of the tolerance; 1.7 ulp for a distance, the same over the arms for a dihedral)
    vals = opt.constraint_values().cpu().numpy()
    tab = opt._tables
    t = gr.Tables(tab.offset, tab.kind, tab.atoms, tab.target)
    x32 = opt.coordinates.cpu().numpy()
    for c in range(9):
        got = vals[c][~np.isnan(vals[c])]
        assert got.size == 1
        resid, bound = np.abs(gr.residual(t, c, got.copy())), gr.residual_bound(t, c, x32, TOL)
        print(f"    entry {c}: residual {resid[0]:.1e} (bound {bound[0]:.1e})")
        assert (resid <= bound).all()
    # torques: -lambda against the central difference of the returned energies
    slope = -opt.constraint_multipliers().cpu().numpy()
    for lo, n, col in ((0, 5, 0), (5, 4, 1)):
        for c in range(lo + 1, lo + n - 1):
            cd = (E[c + 1] - E[c - 1]) / (2 * ORACLE_DELTA)
            print(f"    entry {c}: -lambda = {slope[c, col]:.6e}, central difference {cd:.6e}, difference {abs(slope[c, col] - cd):.1e} "
                  f"(gate {ORACLE_SLOPE_GATE:.0e})")
            assert abs(slope[c, col] - cd) <= ORACLE_SLOPE_GATE


def test_torsion_scan_gives_the_energies_of_the_hand_built_batch(dev):
    from torchani_amd import geomopt

    opt, out, oracle, t_dih, t_dist, xm = _scan(dev)
    moving = torch.zeros(7, dtype=torch.bool)
    moving[DIH[3]] = True
    sp = torch.ones(7, dtype=torch.int64, device=dev)
    scan = geomopt.torsion_scan(_lj(dev), sp, torch.from_numpy(xm).to(dev), DIH, t_dih, moving=moving, fmax=1e-5, steps=300)
    assert tuple(scan.energies.shape) == (5,) and tuple(scan.coordinates.shape) == (5, 7, 3) and bool(scan.converged.all())
    E = scan.energies.cpu().numpy()
    # both are within ORACLE_E_GATE of the same oracle
    print(f"geom constraints torsion_scan: max |E - E_batch| = {np.abs(E - out.energies.cpu().numpy()[:5]).max():.1e} Ha, "
          f"max |E - E_SLSQP| = {np.abs(E - oracle[:5]).max():.1e} Ha")
    assert np.abs(E - oracle[:5]).max() <= ORACLE_E_GATE
    assert np.abs(E - out.energies.cpu().numpy()[:5]).max() <= 2 * ORACLE_E_GATE
    assert np.abs(scan.angles.cpu().numpy() - np.array(t_dih)).max() == 0.0
    tq = scan.torques.cpu().numpy()
    assert np.abs(tq + opt.constraint_multipliers().cpu().numpy()[:5, 0]).max() <= 2 * ORACLE_SLOPE_GATE
    # two molecules at once: the M axis
    two = geomopt.torsion_scan(_lj(dev), sp.expand(2, 7), torch.from_numpy(np.stack([xm, xm + 1.0])).to(dev),
                               (DIH[0], DIH[1], torch.tensor([DIH[2]] * 2), DIH[3]), t_dih[1:3], moving=moving, fmax=1e-5, steps=300)
    assert tuple(two.energies.shape) == (2, 2) and tuple(two.coordinates.shape) == (2, 2, 7, 3)
    assert np.abs(two.energies.cpu().numpy() - oracle[1:3]).max() <= ORACLE_E_GATE


def test_without_constraints_nothing_changes(dev):
    """constraints=None, and CVs that are -1 in every entry, are bit-identical to an optimizer built without the argument."""
    from torchani_amd import geomopt, md

    xm = gr.lj_minimum()
    rs = np.random.RandomState(1)
    x = torch.from_numpy(np.tile(xm, (3, 1, 1)) + rs.uniform(-0.1, 0.1, (3, 7, 3))).to(dev)
    sp = torch.ones((3, 7), dtype=torch.int64, device=dev)
    none = torch.full((3,), -1, dtype=torch.int64)
    runs = []
    for kw in ({}, {"constraints": None}, {"constraints": geomopt.CVConstraints([md.distance(none, 1), md.dihedral(0, 1, none, 3)])}):
        opt = geomopt.GeometryOptimizer(_lj(dev), sp, x, **kw)
        assert opt._geom is None
        for _ in range(10):
            opt.step()
        runs.append((opt.coordinates.clone(), opt.forces.clone(), opt.last_step.clone(), opt.energies.clone()))
        with pytest.raises(ValueError, match="no constraints"):
            opt.constraint_values()
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)


def test_step_does_not_synchronize(dev):
    from torchani_amd import geomopt, md

    model, sp, x, cell, pbc = _ani_case("rand_batch_ani2x", dev)
    opt = geomopt.GeometryOptimizer(model, sp, x, cell, pbc, constraints=geomopt.CVConstraints([md.distance(0, 1), md.dihedral(0, 2, 4, 5)]))
    for _ in range(3):   # (the third evaluation captures the automatic HIP graph)
        opt.step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(5):
            opt.step()
        values, lam = opt.constraint_values(), opt.constraint_multipliers()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert int(opt.n_steps.max()) > 0 and tuple(values.shape) == (sp.shape[0], 2) and bool(torch.isfinite(lam).all())


def test_run_raises_for_a_singular_entry_and_names_it(dev):
    """Two CV objects for one distance in entry 1 only: on its targets the restore has nothing to solve, the projection of
    the first evaluation finds G singular, and run() reports it at its first read."""
    from torchani_amd import geomopt, md

    xm = gr.lj_minimum()
    x = torch.from_numpy(np.tile(xm, (3, 1, 1))).to(dev)
    sp = torch.ones((3, 7), dtype=torch.int64, device=dev)
    cvs = [md.distance(5, 6), md.distance(torch.tensor([-1, 6, -1]), 5), md.angle(0, 5, 1)]
    opt = geomopt.GeometryOptimizer(_lj(dev), sp, x, constraints=geomopt.CVConstraints(cvs))
    with pytest.raises(RuntimeError, match="entry 1 \\(distance of atoms \\(5, 6\\), distance of atoms \\(6, 5\\), angle of atoms "
                                           "\\(0, 5, 1\\)\\).*singular"):
        opt.run(fmax=1e-5, steps=20, check_every=5)
    assert opt._geom_status.tolist() == [0, gr.SINGULAR, 0]
    assert int(opt.n_steps.max()) <= 5
    # a far target is refused at construction, with the way out
    with pytest.raises(ValueError, match="rotate_dihedral"):
        geomopt.GeometryOptimizer(_lj(dev), sp, x, constraints=geomopt.CVConstraints(md.dihedral(*DIH), 3.0))
