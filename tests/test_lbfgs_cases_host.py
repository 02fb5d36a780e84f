"""Host-side proof (no GPU) that the synthetic cases of tests/_lbfgs_cases.py are fit for tests/test_gpu_lbfgs_entry.py: every case
has the layout of csrc/lbfgs.hip it was chosen for, the reference trajectory of every case takes the branches the case is there
for, no decision of that trajectory sits on a rounding edge, and the two-loop reference agrees with a numpy restatement of the
kernels' compact algebra to 1e-9, so a difference on the GPU is not a difference of form."""
import numpy as np
import pytest

import _lbfgs_cases as L
from _lbfgs_cases import CASES, SPLIT_ATOM, report

NAMES = [k.name for k in CASES]
EDGE = 1e-9        # no decision of a reference trajectory closer to its threshold than this, relative
FORM = 1e-9        # max |p_compact - p_two_loop| <= FORM * max |p_two_loop|, per step
_RUNS = {}


class Run:
    """A case on the reference's own trajectory, with the compact restatement stepped next to it."""

    def __init__(self, name):
        self.prob = prob = L.problem(name)
        case = prob.case
        compact = [L.Compact(3 * case.A, case.memory, case.alpha) for _ in range(case.C)]
        self.form = 0.0        # worst max |p_compact - p_two_loop| / max |p_two_loop|
        self.atom_forces = []  # per step: |f_i| [C, A] of the active atoms, 0 on the others
        self.most_pairs = np.zeros(case.C, dtype=np.int64)

        def watch(k, x, f, dr, ref):
            fm = np.where(prob.active[..., None], f.astype(np.float64), 0.0)
            self.atom_forces.append(np.sqrt((fm ** 2).sum(axis=-1)))
            for c in np.nonzero(~ref.converged)[0]:
                p = compact[c].direction(x[c].astype(np.float64).ravel(), fm[c].ravel())
                p_ref = ref.direction[c]
                self.form = max(self.form, np.abs(p - p_ref).max() / np.abs(p_ref).max())
                assert compact[c].D.size == len(ref.pairs[c])
                self.most_pairs[c] = max(self.most_pairs[c], len(ref.pairs[c]))

        self.ref = L.run_reference(prob, watch)


def run(name):
    if name not in _RUNS:
        _RUNS[name] = Run(name)
    return _RUNS[name]


@pytest.mark.parametrize("name", NAMES)
def test_layout_is_what_the_case_is_for(name):
    case = L.BY_NAME[name]
    lay = L.layout(case.C, case.A, case.memory)
    got = dict(V=lay.V, G=lay.G, Gc=lay.Gc, R=lay.R, n_pad=lay.n_pad)
    report(f"lbfgs case {name}: C {case.C}, A {case.A}, memory {case.memory}: n {lay.n}, n_pad {lay.n_pad}, V {lay.V}, G {lay.G}, "
           f"Gc {lay.Gc}, M1 {lay.M1}, R {lay.R}")
    assert got == case.expect
    assert lay.M1 == case.memory + 1 and lay.n == 3 * case.A


def test_layout_edges_named_by_the_cases():
    lay = {k.name: L.layout(k.C, k.A, k.memory) for k in CASES}
    assert lay["one_atom"].n == 3 and lay["one_atom"].M1 == 2
    assert lay["v1_full_group"].n == 63 and lay["v1_full_group"].M1 == L.LB_SLOTS                # one slot group, full
    assert lay["v2_lone_slot"].n == 66 and lay["v2_lone_slot"].M1 - L.LB_SLOTS == 1              # second group: one slot
    assert lay["v4_three_groups"].n == 129 and lay["v4_three_groups"].M1 == 2 * L.LB_SLOTS + 1  # third group: one slot
    assert L.BY_NAME["v4_two_waves"].A == 64 + 1
    assert lay["v8"].n == 258
    assert lay["full_memory"].M1 == 257 and L.BY_NAME["full_memory"].memory == 256
    assert 3 * SPLIT_ATOM == 64 * lay["split_atom"].V - 1 and lay["split_atom"].n == 1029        # coordinate 1023 | 1024, 1025
    many = L.BY_NAME["many_molecules"]
    assert many.C * lay["many_molecules"].G * lay["many_molecules"].R >= 256
    # the sizes on either side of every change of V, next to the ones the cases use
    assert [L.layout(1, A, 1).V for A in (21, 22, 42, 43, 85, 86, 170, 171)] == [1, 2, 2, 4, 4, 8, 8, 16]
    assert [L.layout(1, A, 1).G for A in (341, 342)] == [1, 2]


def test_workspace_bytes_match_library_on_every_case():
    from torchani_amd import _lib
    from torchani_amd.geomopt import lbfgs_workspace_bytes

    _lib.build()
    lib = _lib.lib()
    for case in CASES:
        for C in (case.C, 1):   # (the GPU tests also step single molecules of a case)
            want = lib.anihip_lbfgs_workspace_bytes(C, case.A, case.memory)
            assert want == lbfgs_workspace_bytes(C, case.A, case.memory) == L.layout(C, case.A, case.memory).total, case.name


def _per_case_paths(name, r):
    """The events the case is in the table for."""
    ref, case, prob = r.ref, r.prob.case, r.prob
    with_pairs = ref.rejected - ref.rejected_empty
    if name == "one_atom":             # memory 1: every accepted pair after the first drops the one before it
        assert np.all(ref.accepted >= 10) and np.all(r.most_pairs == 1)
    if name in ("v1_full_group", "v2_lone_slot", "v4_three_groups"):
        # pairs rejected with the ring full: by every molecule once it no longer moves (s = y = 0), and by the last one, on its late
        # ridge, real pairs with s.y < 0 that the spare slot then holds
        assert np.all(ref.rejected_full >= 1) and np.all(r.most_pairs == case.memory)
        assert ref.rejected_full_curved[-1] >= 3 and ref.rejected_full_curved[-1] <= ref.rejected_full[-1] - ref.rejected_still[-1]
        assert ref.rejected_full_wrapped[-1] >= 3     # ... after the ring has wrapped: the spare slot has held a pair before
    if name in ("v2_lone_slot", "v4_three_groups", "v8"):   # the candidate slot has been round the ring at least twice
        assert ref.accepted.max() >= 2 * (case.memory + 1) and np.all(r.most_pairs == case.memory)
    if name == "v4_two_waves":
        assert np.all(ref.converged) and len(set(ref.converged_at.tolist())) >= 2 and np.all(ref.converged_at > 0)
        assert prob.active[0].all() and not prob.active[1, 50:].any() and prob.active[2, 64] and not prob.active[2, 31]
    if name == "full_memory":
        assert ref.accepted[0] >= 257 and r.most_pairs[0] == 256 and ref.n_steps[0] == case.steps
    if name == "split_atom":
        assert np.all(ref.converged) and len(set(ref.converged_at.tolist())) >= 2
        assert prob.active[0, SPLIT_ATOM] and not prob.active[1, SPLIT_ATOM] and prob.active[2, SPLIT_ATOM]
        last = ref.converged_at[0] - 1     # the last step molecule 0 took: only the split atom kept it from converging
        fa = r.atom_forces[last][0]
        others = np.delete(fa, SPLIT_ATOM).max()
        report(f"lbfgs case split_atom: molecule 0 at its last step ({last}): |f| of atom {SPLIT_ATOM} {fa[SPLIT_ATOM]:.2e}, largest "
               f"of the others {others:.2e}, fmax {case.fmax:.0e}")
        assert others < case.fmax <= fa[SPLIT_ATOM]
        assert np.argmax(r.atom_forces[ref.converged_at[0]][0]) == SPLIT_ATOM
    if name == "concave_start":
        assert ref.rejected_empty[0] >= 1 and with_pairs[1] >= 1 and ref.rejected_empty[1] == 0
    if name == "many_molecules":
        roles = np.array(prob.roles)
        assert [roles[c] for c in (0, 4, 7, 1)] == ["inactive", "minimum", "concave", "running"]
        assert {role: int((roles == role).sum()) for role in L.ROLES} == dict(inactive=52, minimum=52, concave=21, running=132)
        still = (roles == "inactive") | (roles == "minimum")
        assert not prob.active[roles == "inactive"].any() and prob.active[roles == "minimum"].all()
        assert np.all(ref.converged_at[still] == 0) and np.all(ref.n_steps[still] == 0)
        assert np.all(ref.rejected_empty[roles == "concave"] >= 1)
        assert np.all(ref.converged_at[~still] > 0) and np.all(ref.rejected[roles == "running"] == 0)   # all converge, later
        assert len(set(ref.converged_at[~still].tolist())) >= 2
        assert (~prob.active[roles == "running"]).any()
        run_c, rej_c, conv_c = L.SOLO["many_molecules"]
        assert roles[run_c] == "running" and roles[rej_c] == "concave" and ref.converged_at[conv_c] > 0


@pytest.mark.parametrize("name", NAMES)
def test_reference_trajectory_reaches_the_paths(name):
    r = run(name)
    ref, case = r.ref, r.prob.case
    conv = sorted(set(ref.converged_at[ref.converged_at >= 0].tolist()))
    report(f"lbfgs case {name}, reference trajectory of {case.steps} steps: pairs accepted {int(ref.accepted.sum())} (most per "
           f"molecule {int(ref.accepted.max())}), rejected {int(ref.rejected.sum())} (ring full {int(ref.rejected_full.sum())}, "
           f"of them with s.y < 0 {int(ref.rejected_full_curved.sum())}, after a wrap {int(ref.rejected_full_wrapped.sum())}; ring empty {int(ref.rejected_empty.sum())}; of molecules that "
           f"no longer moved, s = y = 0, {int(ref.rejected_still.sum())}), steps scaled to maxstep {int(ref.clipped.sum())}, not scaled "
           f"{int(ref.unclipped.sum())}, molecules converged {int(ref.converged.sum())} of {case.C} at steps {conv}")
    assert ref.clipped.sum() >= 1 and ref.unclipped.sum() >= 1     # both branches of longest >= maxstep
    assert np.array_equal(ref.accepted + ref.rejected, np.maximum(ref.n_steps - 1, 0))
    if case.fmax == 0.0:
        assert not ref.converged.any() and np.all(ref.n_steps == case.steps)
    _per_case_paths(name, r)


@pytest.mark.parametrize("name", NAMES)
def test_no_decision_on_a_rounding_edge(name):
    m = run(name).ref.margin
    report(f"lbfgs case {name}: smallest |s.y| / sum |s_i y_i| = {m['curvature']:.1e}, |max |f_i| - fmax| / fmax = {m['fmax']:.1e}, "
           f"|longest - maxstep| / maxstep = {m['maxstep']:.1e} (each to be >= {EDGE:.0e}; {int(run(name).ref.rejected_still.sum())} pairs with s = y = 0 have no margin and are zero "
           f"for the kernel too)")
    assert m["curvature"] >= EDGE and m["fmax"] >= EDGE and m["maxstep"] >= EDGE


@pytest.mark.parametrize("name", NAMES)
def test_two_loop_equals_the_compact_form_of_the_kernels(name):
    r = run(name)
    report(f"lbfgs case {name}: worst max |p_compact - p_two_loop| / max |p_two_loop| = {r.form:.1e} (gate {FORM:.0e})")
    assert r.form <= FORM


def test_pair_dtype_rounds_before_the_curvature_test():
    """s.y = 2^-30 > 0 in fp64, but y rounds to (1, -1, 0) in fp32 and s.y = 0: the default reference decides on the fp64 value
    and stores the pair, the mirror decides on the rounded one and does not; and a pair that is stored is stored rounded."""
    from _geomopt_ref import LbfgsReference

    act = np.ones((1, 1), dtype=bool)
    x0, x1 = np.zeros((1, 1, 3)), np.array([[[1.0, 1.0, 0.0]]])
    f0 = np.array([[[1.0, 0.0, 0.0]]])
    f1 = f0 - np.array([[[1.0, -(1.0 - 2.0 ** -30), 0.0]]])      # y = f0 - f1 = (1, -(1 - 2^-30), 0): s.y = 2^-30 > 0
    kept = []
    for dtype in (None, np.float32):
        ref = LbfgsReference(1, memory=2, maxstep=1.0, alpha=1.0, damping=1.0, fmax=0.0, pair_dtype=dtype)
        ref.step(x0, f0, act)
        ref.step(x1, f1, act)
        kept.append(len(ref.pairs[0]))
    assert kept == [1, 0]                                          # fp32: y = (1, -1, 0), s.y = 0: not stored
    ref = LbfgsReference(1, memory=2, maxstep=1.0, alpha=1.0, damping=1.0, fmax=0.0, pair_dtype=np.float32)
    ref.step(x0, f0, act)
    ref.step(x1 * (1.0 + 2.0 ** -30), f1 - 1.0, act)
    (s, y), = ref.pairs[0]
    assert s.dtype == np.float64 and np.array_equal(s, [1.0, 1.0, 0.0]) and np.array_equal(y, y.astype(np.float32))
