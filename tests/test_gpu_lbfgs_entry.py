"""anihip_lbfgs_step through its raw entry point on the MI355X, entry by entry at the shape edges of csrc/lbfgs.hip: the synthetic
cases of tests/_lbfgs_cases.py (every instantiation of k_lb_dots, memory 1 and 256, ring wrap-around over one to 65 slot groups, pairs
rejected with the ring full and empty, an atom cut by a chunk boundary, 257 molecules in mixed states, garbage forces on inactive
atoms) in lock step with the fp64 two-loop reference that mirrors the fp32 pair storage; converged molecules frozen bit for bit,
history included; the same bits wherever a molecule sits in a batch and run to run; nothing written outside the buffers; argument
errors refused before any launch.  tests/test_lbfgs_cases_host.py proves without a device that the cases reach those paths."""
import ctypes as C

import numpy as np
import pytest
import torch

import _lbfgs_cases as L
from _lbfgs_cases import CASES, SOLO, report

pytestmark = pytest.mark.gpu

# last_step is the fp32 rounding of an fp64 product (2^-24 relative); upstream of it kernel and reference do fp64 arithmetic on
# identical fp32 inputs (the reference stores its pairs in fp32 too) and differ by the 1e-9 that the host test bounds: twice the
# output rounding, of the molecule's largest component
ULP = 2.0 ** -23
GUARD = 4096    # bytes of pattern before and after every guarded buffer
PATTERN = 0xA5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from torchani_amd import _lib

    _lib.lib()
    return torch.device("cuda:0")


class Stepper:
    """The tensors of one optimizer (a whole case, or its molecule `only` alone) and anihip_lbfgs_step on them.  With `guard`
    every tensor the kernels write lies inside a larger one, GUARD bytes of PATTERN on either side."""

    def __init__(self, dev, prob, only=None, guard=False):
        from torchani_amd import _lib

        case = prob.case
        self.prob, self.only = prob, only
        self.C = Cn = case.C if only is None else 1
        self.lay = L.layout(Cn, case.A, case.memory)
        self.params = _lib.LbfgsParams(Cn, case.A, case.memory, 0, 1.0 / case.alpha, case.maxstep, case.damping, case.fmax)
        self.workspace_bytes = int(_lib.lib().anihip_lbfgs_workspace_bytes(Cn, case.A, case.memory))
        assert self.workspace_bytes == self.lay.total
        self._outer = []
        pad = GUARD if guard else 0

        def buffer(nbytes, dtype, shape):
            outer = torch.full((nbytes + 2 * pad,), PATTERN, dtype=torch.uint8, device=dev)
            inner = outer[pad:pad + nbytes]
            inner.zero_()
            self._outer.append((outer, nbytes))
            return inner.view(dtype).view(shape)

        active = prob.active if only is None else prob.active[only:only + 1]
        x = prob.x_start if only is None else prob.x_start[only:only + 1]
        self.active = torch.from_numpy(np.ascontiguousarray(active).astype(np.uint8)).to(dev)
        self.workspace = buffer(self.workspace_bytes, torch.uint8, (self.workspace_bytes,))
        self.x = buffer(Cn * case.A * 12, torch.float32, (Cn, case.A, 3))
        self.last_step = buffer(Cn * case.A * 12, torch.float32, (Cn, case.A, 3))
        self.converged = buffer(Cn, torch.uint8, (Cn,))
        self.n_steps = buffer(Cn * 4, torch.int32, (Cn,))
        self.f = torch.zeros((Cn, case.A, 3), dtype=torch.float32, device=dev)
        self.x.copy_(torch.from_numpy(np.ascontiguousarray(x)))

    def call(self, params=None, workspace_bytes=None, null=None):
        """The raw call; `null` names a pointer argument to pass as NULL.  Returns the status."""
        from torchani_amd import _lib, geomopt

        ptr = dict(active=self.active, coords=self.x, forces=self.f, workspace=self.workspace, last_step=self.last_step,
                   converged=self.converged, n_steps=self.n_steps)
        p = {k: (None if k == null else t.data_ptr()) for k, t in ptr.items()}
        par = None if null == "params" else C.byref(self.params if params is None else params)
        return _lib.lib().anihip_lbfgs_step(
            geomopt._stream(), par, p["active"], p["coords"], p["forces"], p["workspace"],
            self.workspace_bytes if workspace_bytes is None else workspace_bytes, p["last_step"], p["converged"], p["n_steps"])

    def step(self, forces):
        from torchani_amd import _lib

        self.f.copy_(torch.from_numpy(forces))
        _lib.check(self.call())

    def host_forces(self, x):
        return self.prob.forces(x, only=self.only)

    def guards_intact(self):
        for outer, nbytes in self._outer:
            if not (bool((outer[:GUARD] == PATTERN).all()) and bool((outer[GUARD + nbytes:] == PATTERN).all())):
                return False
        return True

    def tensors(self):
        return [self.workspace, self.x, self.last_step, self.converged, self.n_steps, self.f, self.active]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("name", [k.name for k in CASES])
def test_lockstep_against_reference(dev, name):
    """Per step: x_k read back, f_k from the host potential, one kernel step and one reference step on the same x_k, f_k."""
    prob = L.problem(name)
    case = prob.case
    run = Stepper(dev, prob)
    ref = prob.reference()
    act = prob.active
    worst = 0.0
    failures = []
    for k in range(case.steps):
        x = run.x.cpu().numpy()
        f = prob.forces(x)
        run.step(f)
        dr = ref.step(x, f, act)
        got, x_new = run.last_step.cpu().numpy(), run.x.cpu().numpy()
        scale = np.abs(dr).reshape(case.C, -1).max(axis=1)
        err = np.abs(got - dr).reshape(case.C, -1).max(axis=1)
        ulps = np.divide(err, scale, out=np.zeros_like(err), where=scale > 0) / ULP
        worst = max(worst, ulps.max()) if np.isfinite(ulps).all() else np.inf
        exact = {"converged": np.array_equal(run.converged.cpu().numpy().astype(bool), ref.converged),
                 "n_steps": np.array_equal(run.n_steps.cpu().numpy(), ref.n_steps),
                 "x = fp32(x + last_step) on active atoms": np.array_equal(_bits(x_new[act]), _bits(x[act] + got[act])),
                 "inactive atoms unmoved": np.array_equal(_bits(x_new[~act]), _bits(x[~act])) and not np.any(got[~act]),
                 "no step where the reference has none": not np.any(err[scale == 0.0])}
        failures += [(k, what) for what, ok in exact.items() if not ok]
        if not ulps.max() <= 1.0:   # (a NaN fails too)
            failures.append((k, int(ulps.argmax()), float(ulps.max())))
        if len(failures) > 20 or not (exact["converged"] and exact["n_steps"]):   # the trajectories have parted: stop, report
            break
    conv = sorted(set(ref.converged_at[ref.converged_at >= 0].tolist()))
    report(f"lbfgs entry lock-step {name} (C {case.C}, A {case.A}, memory {case.memory}, {case.steps} steps): worst |last_step - "
           f"dr_ref| / max |dr_ref| = {worst:.3f} fp32 ulp (gate 1); pairs stored {int(ref.accepted.sum())}, rejected "
           f"{int(ref.rejected.sum())} (ring full {int(ref.rejected_full.sum())}, of them with s.y < 0 "
           f"{int(ref.rejected_full_curved.sum())}, after a wrap {int(ref.rejected_full_wrapped.sum())}; ring empty {int(ref.rejected_empty.sum())}; s = y = 0 {int(ref.rejected_still.sum())}); "
           f"converged {int(ref.converged.sum())} at steps {conv}; decisions off their thresholds by >= "
           f"{min(ref.margin.values()):.1e}")
    assert not failures, failures[:5]


def _molecule_regions(run, ws, c):
    """The bytes of molecule c in every region of the workspace (the offsets of _lbfgs_cases.layout)."""
    lay = run.lay
    return {name: ws[lay.offsets[name] + c * size:lay.offsets[name] + (c + 1) * size].copy() for name, size in lay.sizes.items()}


@pytest.mark.parametrize("name", ["v4_two_waves", "many_molecules"])
def test_converged_molecules_stay_frozen(dev, name):
    """From the step after its convergence on a molecule is handed forces of 1 Ha / A on every atom: nothing of it changes."""
    prob = L.problem(name)
    case = prob.case
    run = Stepper(dev, prob)
    frozen = {}
    checked = 0
    for k in range(case.steps):
        x = run.x.cpu().numpy()
        f = prob.forces(x)
        for c in frozen:
            f[c] = 1.0
        run.step(f)
        conv = run.converged.cpu().numpy().astype(bool)
        x_new, got, n_steps = run.x.cpu().numpy(), run.last_step.cpu().numpy(), run.n_steps.cpu().numpy()
        ws = run.workspace.cpu().numpy()
        for c in np.nonzero(conv)[0]:
            assert not np.any(got[c]), (k, c)
            if c not in frozen:
                frozen[c] = (k, x_new[c].copy(), n_steps[c], _molecule_regions(run, ws, c))
                continue
            _, x_then, n_then, regions = frozen[c]
            assert np.array_equal(_bits(x_new[c]), _bits(x_then)) and n_steps[c] == n_then, (k, c)
            for region, then in _molecule_regions(run, ws, c).items():
                assert np.array_equal(then, regions[region]), (k, c, region)
            checked += 1
        assert all(conv[c] for c in frozen), k
    steps = sorted({k for k, *_ in frozen.values()})
    report(f"lbfgs entry frozen {name}: {len(frozen)} of {case.C} molecules converged at steps {steps}; {checked} later molecule-steps "
           f"with forces of 1 Ha / A: coordinates, n_steps and all {len(run.lay.sizes)} workspace regions bit-identical")
    assert len(frozen) == case.C and len(steps) >= 2 and checked >= case.C


def _history(run, steps):
    """Coordinates, last_step and n_steps after every step (on the device)."""
    out = []
    for _ in range(steps):
        run.step(run.host_forces(run.x.cpu().numpy()))
        out.append((run.x.clone(), run.last_step.clone(), run.n_steps.clone()))
    return out


@pytest.mark.parametrize("name", ["many_molecules", "split_atom"])
def test_an_entry_gives_the_same_bits_wherever_it_sits(dev, name):
    """No atomics and every sum in a fixed order: a molecule stepped alone (C = 1) and at its place in the batch, and the whole
    batch twice."""
    prob = L.problem(name)
    case = prob.case
    first, second = (_history(Stepper(dev, prob), case.steps) for _ in range(2))
    for k in range(case.steps):
        assert all(torch.equal(a, b) for a, b in zip(first[k], second[k])), k
    moved = []
    for c in SOLO[name]:
        alone = _history(Stepper(dev, prob, only=c), case.steps)
        for k in range(case.steps):
            assert all(torch.equal(a[0], b[c]) for a, b in zip(alone[k], first[k])), (c, k)
        moved.append(int(alone[-1][2][0]))
    report(f"lbfgs entry placement {name}: two runs of {case.steps} steps bit-identical; molecules {list(SOLO[name])} alone (C = 1) "
           f"and in the batch of {case.C} bit-identical, n_steps {moved}")
    assert min(moved) > 0


@pytest.mark.parametrize("name", ["one_atom", "v4_three_groups", "full_memory", "split_atom"])
def test_nothing_is_written_outside_the_buffers(dev, name):
    """Workspace (of exactly anihip_lbfgs_workspace_bytes), coords, last_step, converged and n_steps each between two guard bands
    of a byte pattern, the whole case run: the bands are as they were."""
    prob = L.problem(name)
    run = Stepper(dev, prob, guard=True)
    assert run.guards_intact() and run.workspace.numel() == run.workspace_bytes
    for _ in range(prob.case.steps):
        run.step(run.host_forces(run.x.cpu().numpy()))
    torch.cuda.synchronize()
    ok = run.guards_intact()
    report(f"lbfgs entry guard bands {name}: workspace {run.workspace_bytes} bytes, {prob.case.steps} steps, n_steps "
           f"{run.n_steps.cpu().tolist()[:4]}: {GUARD} bytes before and after each of 5 buffers intact: {ok}")
    assert ok and int(run.n_steps.max()) > 0


def test_argument_errors(dev):
    """Host-side refusals: a non-zero status, a message, nothing launched and no tensor changed."""
    from torchani_amd import _lib

    prob = L.problem("one_atom")
    run = Stepper(dev, prob)
    run.step(prob.forces(prob.x_start))
    run.f.copy_(torch.from_numpy(prob.forces(run.x.cpu().numpy())))
    before = [t.clone() for t in run.tensors()]

    def params(**kw):
        p = _lib.LbfgsParams.from_buffer_copy(run.params)
        for key, value in kw.items():
            setattr(p, key, value)
        return p

    bad = [("workspace_bytes one short", dict(workspace_bytes=run.workspace_bytes - 1), b"workspace"),
           ("memory 0", dict(params=params(memory=0)), b"memory"),
           ("memory 257", dict(params=params(memory=257)), b"memory"),
           ("n_mol 0", dict(params=params(n_mol=0)), b"n_mol"),
           ("maxstep 0", dict(params=params(maxstep=0.0)), b"maxstep"),
           ("maxstep < 0", dict(params=params(maxstep=-0.1)), b"maxstep"),
           ("damping 0", dict(params=params(damping=0.0)), b"damping"),
           ("damping < 0", dict(params=params(damping=-1.0)), b"damping"),
           ("inv_alpha 0", dict(params=params(inv_alpha=0.0)), b"inv_alpha"),
           ("inv_alpha < 0", dict(params=params(inv_alpha=-1.0)), b"inv_alpha"),
           ("fmax < 0", dict(params=params(fmax=-1e-3)), b"fmax")]
    bad += [(f"null {name}", dict(null=name), b"null") for name in ("params", "active", "coords", "forces", "workspace", "last_step",
                                                                    "converged", "n_steps")]
    # (the four positive-or-zero parameters share one message; that each call differs from the accepted call at the end in one
    # argument only is what ties the refusal to that argument)
    for what, kw, word in bad:
        status = run.call(**kw)
        message = _lib.lib().anihip_last_error()
        torch.cuda.synchronize()
        assert status != 0 and word in message, (what, status, message)
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(run.tensors(), before)), what
    report(f"lbfgs entry argument errors: {len(bad)} bad calls refused, no tensor changed")
    _lib.check(run.call())   # and the good call still goes through
    assert run.n_steps.cpu().tolist() == [2, 2, 2]
