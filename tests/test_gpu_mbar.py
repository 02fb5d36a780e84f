"""MBAR (csrc/mbar.hip, torchani_amd.md.MBAR) on the MI355X against the fp64 reference of tests/_mbar_ref.py: one iteration
entry by entry over the shape edges of the kernels through the C ABI, structured and dense, stability under large shifts, the
log weights of sampled, external and all states in slabs, the histograms, determinism, broken tables; and through the class the
solvers, the uncertainties, the calls that must not synchronize, umbrella windows on Lennard-Jones dimers end to end, a
temperature ladder, and pooling.

The gate of an iteration is derived, not measured: every term of a log-sum-exp carries a few ulp, its exponent argument |u|
2^-52, a sum of M terms at most M 2^-53 relative, so with |u| <= 1e3 and K N <= 2e6 |df| <= 1e-9 absolute (measured: see
profiles/mbar_tests.txt)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
from scipy.special import logsumexp

import _mbar_ref as mr
import _md_bias_ref as br

pytestmark = pytest.mark.gpu

F_GATE = 1e-9
KS = (1, 2, 63, 64, 65, 257, 1025)
NS = (1, 255, 256, 257, 4099, 100003)
RS = (0, 1, 3, 16)
SHAPES = [(K, N) for K in KS for N in NS if K * N <= 2_000_000]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from torchani_amd import _lib

    _lib.lib()
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Abi:
    """A problem on the device and the calls of the C ABI on it."""

    def __init__(self, dev, n_k, beta=None, restraint=None, kinds=None, energy=None, cv=None, u=None):
        from torchani_amd import _lib

        self.lib, self.dev = _lib, dev
        put = lambda a, dt=torch.float64: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)  # noqa: E731
        self.K = len(n_k)
        self.R = 0 if restraint is None or u is not None else restraint.shape[1]
        self.N = u.shape[1] if u is not None else (cv.shape[0] if cv is not None and self.R else len(energy))
        self.held = dict(n_k=put(n_k), beta=put(beta), restraint=put(restraint), kinds=put(kinds, torch.int32), energy=put(energy),
                         cv=put(cv), u=put(u))
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
        h = self.held
        self.struct = _lib.Mbar(self.N, self.K, self.R, ptr(h["beta"]), ptr(h["n_k"]), ptr(h["restraint"]), ptr(h["kinds"]),
                                ptr(h["energy"]), ptr(h["cv"]), ptr(h["u"]), self.status.data_ptr())
        nbytes = _lib.lib().anihip_mbar_workspace_bytes(C.byref(self.struct))
        assert nbytes > 0
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def iterate(self, f, n_iter=1, sentinel=None):
        f_in = torch.as_tensor(f, dtype=torch.float64).to(self.dev)
        out = torch.full((self.K,), float("nan") if sentinel is None else sentinel, dtype=torch.float64, device=self.dev)
        delta = torch.full((1,), float("nan") if sentinel is None else sentinel, dtype=torch.float64, device=self.dev)
        self.lib.check(self.lib.lib().anihip_mbar_iterate(_stream(), C.byref(self.struct), f_in.data_ptr(), n_iter, out.data_ptr(),
                                                          delta.data_ptr(), self.ws.data_ptr(), self.ws.numel()))
        return out, delta

    def log_weights(self, f, target, first=0, count=None, beta=None, rows=None, u=None, sentinel=float("nan")):
        count = self.N - first if count is None else count
        f_in = torch.as_tensor(f, dtype=torch.float64).to(self.dev)
        shape = (count, self.K) if target == self.lib.MBAR_TARGET_ALL else (count,)
        out = torch.full(shape, sentinel, dtype=torch.float64, device=self.dev)
        put = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(self.dev)  # noqa: E731
        held = [put(beta), put(rows), put(u)]
        self.lib.check(self.lib.lib().anihip_mbar_log_weights(
            _stream(), C.byref(self.struct), f_in.data_ptr(), target, *(None if t is None else t.data_ptr() for t in held), first,
            count, out.data_ptr(), self.ws.data_ptr(), self.ws.numel()))
        return out


def _histogram(dev, log_w, cv, columns, lo, hi, bins):
    from torchani_amd import _lib

    L = _lib.lib()
    n, total = len(log_w), int(np.prod(bins))
    w, s = torch.as_tensor(log_w).to(dev), torch.as_tensor(np.ascontiguousarray(cv)).to(dev)
    ws = torch.empty(L.anihip_mbar_histogram_workspace_bytes(n, total), dtype=torch.uint8, device=dev)
    out = torch.full((total,), float("nan"), dtype=torch.float64, device=dev)
    counts = torch.full((total,), -1, dtype=torch.int64, device=dev)
    m = len(columns)
    pad = lambda v, fill: (list(v) + [fill])[:2]   # noqa: E731
    _lib.check(L.anihip_mbar_histogram(_stream(), n, w.data_ptr(), s.data_ptr(), cv.shape[1], m, (C.c_int32 * 2)(*pad(columns, 0)),
                                       (C.c_double * 2)(*pad(lo, 0.0)), (C.c_double * 2)(*pad(hi, 1.0)),
                                       (C.c_int32 * 2)(*pad(bins, 1)), out.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel()))
    return out.cpu().numpy(), counts.cpu().numpy()


def _case(K, R, N, seed):
    """A structured problem with mixed kinds, dihedral samples and centres within 1e-3 of +-pi, flat-bottom and k = 0 rows,
    several unsampled states (state K - 1 among them), energies and differing beta; |u| stays below 1e3."""
    rs = np.random.RandomState(seed)
    kinds = np.array([(r + 2) % 3 for r in range(R)], dtype=np.int32)   # the first column a dihedral
    cv = rs.uniform(0.5, 3.0, (N, R))
    restraint = np.zeros((K, R, 3))
    restraint[..., 0] = rs.uniform(0.5, 3.0, (K, R))
    restraint[..., 1] = rs.uniform(0.0, 4.0, (K, R)) * (rs.uniform(size=(K, R)) > 0.2)
    restraint[..., 2] = rs.uniform(0.0, 0.5, (K, R)) * (rs.uniform(size=(K, R)) > 0.5)
    for r in np.flatnonzero(kinds == br.DIHEDRAL):
        cv[:, r] = rs.uniform(-math.pi, math.pi, N)
        edge = rs.uniform(size=N) < 0.3
        cv[edge, r] = rs.choice([-1.0, 1.0], edge.sum()) * (math.pi - rs.uniform(0.0, 1e-3, edge.sum()))
        restraint[:, r, 0] = rs.uniform(-math.pi, math.pi, K)
        edge = rs.uniform(size=K) < 0.3
        restraint[edge, r, 0] = rs.choice([-1.0, 1.0], edge.sum()) * (math.pi - rs.uniform(0.0, 1e-3, edge.sum()))
    beta = rs.uniform(0.5, 2.0, K)
    energy = rs.uniform(-5.0, 5.0, N)
    n_k = rs.multinomial(N, rs.dirichlet(np.ones(K))).astype(np.float64)
    if K > 1:
        off = rs.uniform(size=K) < 0.25
        off[K - 1] = True
        off[int(np.argmax(n_k))] = False
        n_k[int(np.argmax(n_k))] += n_k[off].sum()
        n_k[off] = 0.0
    return dict(n_k=n_k, beta=beta, restraint=restraint, kinds=kinds, energy=energy, cv=cv), rs.normal(0.0, 1.0, K)


@pytest.mark.parametrize("K,N", SHAPES)
def test_one_iteration_matches_reference(dev, K, N):
    worst = 0.0
    for R in RS:
        case, f = _case(K, R, N, 1000 * R + K + N)
        u = mr.reduced_potentials(case["beta"], case["restraint"], case["kinds"], case["energy"], case["cv"])
        assert np.abs(u).max() <= 1e3
        want, want_delta = mr.iterate(u, case["n_k"], f)
        got, delta = Abi(dev, **case).iterate(f)
        err = np.abs(got.cpu().numpy() - want).max()
        worst = max(worst, err)
        assert err <= F_GATE, (R, err)
        assert abs(float(delta) - want_delta) <= F_GATE
        if R == 3:   # the dense mode on the same u
            dense, d2 = Abi(dev, case["n_k"], u=u).iterate(f)
            err = np.abs(dense.cpu().numpy() - want).max()
            worst = max(worst, err)
            assert err <= F_GATE and abs(float(d2) - want_delta) <= F_GATE, ("dense", err)
    print(f"mbar, one iteration K = {K}, N = {N}, R in {RS} and dense: max |f' - reference| {worst:.2e} (gate {F_GATE:.0e})")


def test_several_iterations_in_one_call_match_the_reference(dev):
    case, f = _case(65, 3, 4099, 5)
    u = mr.reduced_potentials(case["beta"], case["restraint"], case["kinds"], case["energy"], case["cv"])
    want = f
    for _ in range(5):
        want, want_delta = mr.iterate(u, case["n_k"], want)
    got, delta = Abi(dev, **case).iterate(f, 5)
    err = np.abs(got.cpu().numpy() - want).max()
    print(f"mbar, five iterations in one call: max |f - reference| {err:.2e}, delta {float(delta):.3e} against {want_delta:.3e}")
    assert err <= 5 * F_GATE and abs(float(delta) - want_delta) <= 5 * F_GATE


def test_large_shifts_stay_finite_and_match(dev):
    """u shifted by +-1e4 per state (dense), and energies of +-1e4 / beta (structured): the same gate scaled by |u| / 1e3."""
    rs = np.random.RandomState(11)
    case, f = _case(7, 1, 1000, 12)
    u = mr.reduced_potentials(case["beta"], case["restraint"], case["kinds"], case["energy"], case["cv"])
    shifted = u + rs.choice([-1e4, 1e4], 7)[:, None]
    f = f + rs.uniform(-1e4, 1e4, 7)
    want, _ = mr.iterate(shifted, case["n_k"], f)
    got, delta = Abi(dev, case["n_k"], u=shifted).iterate(f)
    err = np.abs(got.cpu().numpy() - want).max()
    assert np.isfinite(got.cpu().numpy()).all() and np.isfinite(float(delta)) and err <= 10 * F_GATE, err
    case["energy"] = rs.choice([-1e4, 1e4], 1000) * rs.uniform(0.5, 1.0, 1000)
    u2 = mr.reduced_potentials(case["beta"], case["restraint"], case["kinds"], case["energy"], case["cv"])
    want2, _ = mr.iterate(u2, case["n_k"], f)
    got2, _ = Abi(dev, **case).iterate(f)
    err2 = np.abs(got2.cpu().numpy() - want2).max()
    print(f"mbar, |u| up to {np.abs(shifted).max():.1e} (dense) and {np.abs(u2).max():.1e} (structured): max |f' - reference| "
          f"{err:.2e} and {err2:.2e} (gate {20 * F_GATE:.0e})")
    assert np.isfinite(got2.cpu().numpy()).all() and err2 <= 20 * F_GATE, err2


def test_log_weights_of_sampled_external_and_all_states(dev):
    from torchani_amd import _lib

    case, f = _case(5, 3, 4099, 21)
    u = mr.reduced_potentials(case["beta"], case["restraint"], case["kinds"], case["energy"], case["cv"])
    f, _ = mr.solve(u, case["n_k"])
    abi = Abi(dev, **case)
    sampled = int(np.argmax(case["n_k"]))
    got = abi.log_weights(f, sampled).cpu().numpy()
    want = mr.log_weights(u, case["n_k"], f, u[sampled])
    assert np.abs(got - want).max() <= 1e-10 and abs(logsumexp(got)) <= 1e-12
    # an external target: another temperature, other rows
    beta_t, rows_t = np.array([1.3]), case["restraint"][1] * 0.5
    u_t = mr.reduced_potentials(beta_t, rows_t[None], case["kinds"], case["energy"], case["cv"])[0]
    got_t = abi.log_weights(f, _lib.MBAR_TARGET_EXTERNAL, beta=beta_t, rows=rows_t).cpu().numpy()
    want_t = mr.log_weights(u, case["n_k"], f, u_t)
    assert np.abs(got_t - want_t).max() <= 1e-10 and abs(logsumexp(got_t)) <= 1e-12
    # a slab of one target: edges inside and across the reduction chunks of 1024
    part = abi.log_weights(f, sampled, first=1000, count=1100).cpu().numpy()
    assert np.array_equal(part, got[1000:2100])
    # all states in slabs
    want_all = mr.log_weights_all(u, case["n_k"], f)
    worst = 0.0
    for first, count in ((0, 100), (100, 924), (1024, 1024), (2000, 2099)):
        slab = abi.log_weights(f, _lib.MBAR_TARGET_ALL, first=first, count=count).cpu().numpy()
        worst = max(worst, np.abs(slab - want_all[first:first + count]).max())
    dense = Abi(dev, case["n_k"], u=u)
    d_all = dense.log_weights(f, _lib.MBAR_TARGET_ALL).cpu().numpy()
    d_ext = dense.log_weights(f, _lib.MBAR_TARGET_EXTERNAL, u=u_t).cpu().numpy()
    print(f"mbar, log weights: sampled {np.abs(got - want).max():.1e}, external {np.abs(got_t - want_t).max():.1e}, all states in "
          f"slabs {worst:.1e}, dense {np.abs(d_all - want_all).max():.1e}; |lse| {abs(logsumexp(got)):.1e}, {abs(logsumexp(got_t)):.1e}")
    assert worst <= 1e-10 and np.abs(d_all - want_all).max() <= 1e-10 and np.abs(d_ext - want_t).max() <= 1e-10
    sums = np.exp(want_all).sum(axis=0)
    assert np.abs(sums - 1.0).max() <= 1e-9   # (f is converged: every column of W is normalized)


@pytest.mark.parametrize("n", [1, 63, 4099, 300001])
def test_histograms_in_one_and_two_columns(dev, n):
    rs = np.random.RandomState(n)
    cv = rs.uniform(-0.2, 1.2, (n, 3))
    edges = np.linspace(0.0, 1.0, 11)
    cv[::7, 0] = rs.choice(edges, len(cv[::7]))        # exactly on edges, the last one included (out of range)
    cv[::11, 2] = rs.choice([-0.5, 1.5], len(cv[::11]))   # below the first edge and above the last
    cv[(cv[:, 0] >= 0.3) & (cv[:, 0] < 0.4), 0] = 0.45     # an empty bin
    log_w = rs.normal(0.0, 30.0, n)
    worst = 0.0
    for columns, lo, hi, bins in (([0], [0.0], [1.0], [10]), ([2, 0], [0.0, 0.0], [1.0, 1.0], [7, 10]), ([1], [0.1], [0.9], [4096])):
        want, want_counts = mr.histogram(log_w, cv, columns, lo, hi, bins)
        got, counts = _histogram(dev, log_w, cv, columns, lo, hi, bins)
        assert np.array_equal(counts, want_counts)
        in_range = np.ones(n, dtype=bool)
        for c, col in enumerate(columns):
            in_range &= (cv[:, col] >= lo[c]) & (cv[:, col] < hi[c])
        assert counts.sum() == in_range.sum()
        full = want_counts > 0
        assert np.array_equal(np.isneginf(got), ~full)
        if columns == [0] and n >= 63:
            assert counts[3] == 0 and counts[2] > 0 and counts[4] > 0   # the empty bin between populated ones
        if full.any():
            worst = max(worst, np.abs(got[full] - want[full]).max())
    print(f"mbar, histograms of {n} samples in 10, 7 x 10 and 4096 bins: max |lse - reference| {worst:.1e} (gate 1e-11)")
    assert worst <= 1e-11


def test_the_same_call_gives_the_same_bits(dev):
    from torchani_amd import _lib

    case, f = _case(65, 3, 100003, 31)
    abi = Abi(dev, **case)
    a, da = abi.iterate(f, 2)
    wa = abi.log_weights(f, 0)
    ha = _histogram(dev, wa.cpu().numpy(), case["cv"], [1], [0.5], [3.0], [48])
    b, db = abi.iterate(f, 2)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        x = torch.randn(512, 512, device=dev)
        (x @ x).sum()   # unrelated work first
        other = Abi(dev, **case)
        c, dc = other.iterate(f, 2)
        wc = other.log_weights(f, 0)
        all_c = other.log_weights(f, _lib.MBAR_TARGET_ALL, first=5, count=3000)
    side.synchronize()
    hc = _histogram(dev, wc.cpu().numpy(), case["cv"], [1], [0.5], [3.0], [48])
    all_a = abi.log_weights(f, _lib.MBAR_TARGET_ALL, first=5, count=3000)
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(da, db) and torch.equal(da, dc)
    assert torch.equal(wa, wc) and torch.equal(all_a, all_c)
    assert np.array_equal(ha[0], hc[0]) and np.array_equal(ha[1], hc[1])


def test_broken_tables_are_reported_and_nothing_is_written(dev):
    from torchani_amd import _lib

    base, f = _case(5, 3, 1000, 41)

    def broken(**change):
        case = {k: v.copy() for k, v in base.items()}
        for name, (index, value) in change.items():
            case[name][index] = value
        return Abi(dev, **case)

    flat = dict(restraint=((0, 2, 2), 0.3))   # (a flat bottom swallows a NaN in fmax: the check must see it)
    for what, abi, bit in (("NaN in cv", broken(cv=((17, 1), np.nan)), _lib.MBAR_BAD_SAMPLES),
                           ("NaN in cv under a flat bottom", broken(cv=((999, 2), np.nan), **flat), _lib.MBAR_BAD_SAMPLES),
                           ("inf in energy", broken(energy=(5, np.inf)), _lib.MBAR_BAD_SAMPLES),
                           ("negative n_k", broken(n_k=(0, -1.0)), _lib.MBAR_BAD_COUNTS),
                           ("all n_k zero", broken(n_k=(slice(None), 0.0)), _lib.MBAR_BAD_COUNTS),
                           ("negative k", broken(restraint=((1, 1, 1), -1.0)), _lib.MBAR_BAD_STATES),
                           ("unknown kind", broken(kinds=(0, 3)), _lib.MBAR_BAD_STATES)):
        out, delta = abi.iterate(f, 2, sentinel=-7.0)
        assert int(abi.status) & bit, what
        assert bool((out == -7.0).all()) and float(delta) == -7.0, what
        lw = abi.log_weights(f, 0, sentinel=-7.0)
        every = abi.log_weights(f, _lib.MBAR_TARGET_ALL, first=0, count=1000, sentinel=-7.0)
        assert int(abi.status) & bit and bool((lw == -7.0).all()) and bool((every == -7.0).all()), what
    good = broken()
    out, _ = good.iterate(f)
    assert int(good.status) == 0 and bool(torch.isfinite(out).all())
    # a NaN outside the slab of an all-states call is not this call's to report
    late = broken(cv=((900, 0), np.nan))
    slab = late.log_weights(f, _lib.MBAR_TARGET_ALL, first=0, count=800)
    assert int(late.status) == 0 and bool(torch.isfinite(slab).all())
    u = mr.reduced_potentials(base["beta"], base["restraint"], base["kinds"], base["energy"], base["cv"])
    u[3, 77] = np.nan
    dense = Abi(dev, base["n_k"], u=u)
    out, _ = dense.iterate(f, 1, sentinel=-7.0)
    assert int(dense.status) == _lib.MBAR_BAD_SAMPLES and bool((out == -7.0).all())


# ---- through the class ----------------------------------------------------------------------------------------------------------

def _harmonic(dev):
    from torchani_amd import md

    restraint, n_k, cv, exact = mr.harmonic_case(0)
    kT = 1.0 / br.KB_HARTREE   # a temperature at which beta = 1 / Hartree
    states = md.ThermodynamicStates(kT, restraint[:, 0, 0], restraint[:, 0, 1])
    u = mr.reduced_potentials(states.beta.numpy(), restraint, [0], None, cv)
    return states, n_k, cv, u


def test_solvers_reach_the_reference_and_adaptive_takes_fewer_iterations(dev):
    from torchani_amd import md

    states, n_k, cv, u = _harmonic(dev)
    want, _ = mr.solve(u, n_k, tolerance=1e-13)
    x = torch.from_numpy(cv).to(dev)
    runs = {}
    for solver in ("adaptive", "self-consistent"):
        m = md.MBAR(states, n_k, x)
        f = m.solve(solver=solver)
        err = np.abs(f.cpu().numpy() - want).max()
        runs[solver] = (m.iterations, m.weight_passes, err, m)
        assert m.converged and m.delta < 1e-10 and err <= 1e-8, (solver, err, m.delta)
    dense = md.MBAR.from_reduced_potentials(torch.from_numpy(u).to(dev), n_k)
    err_dense = np.abs(dense.solve().cpu().numpy() - want).max()
    m = runs["adaptive"][3]
    se = m.uncertainties().cpu().numpy()
    want_se = mr.uncertainties(np.exp(mr.log_weights_all(u, n_k, want)), n_k)
    off = ~np.eye(6, dtype=bool)
    rel = np.abs(se[off] / want_se[off] - 1.0).max()
    print(f"mbar, six harmonic states, 10 000 samples: adaptive {runs['adaptive'][0]} kernel iterations and {runs['adaptive'][1]} "
          f"weight passes (|f - reference| {runs['adaptive'][2]:.1e}), self-consistent {runs['self-consistent'][0]} iterations "
          f"({runs['self-consistent'][2]:.1e}), dense {err_dense:.1e}; uncertainties within {rel:.1e} relative")
    assert err_dense <= 1e-8
    assert runs["adaptive"][0] < runs["self-consistent"][0]
    assert rel <= 1e-6 and np.abs(np.diag(se)).max() <= 1e-6
    fh = m.free_energies("hartree").cpu().numpy()
    assert np.allclose(fh, want / states.beta.numpy(), rtol=0, atol=1e-8 / states.beta.numpy()[0])


def test_blocks_and_read_outs_do_not_synchronize(dev):
    from torchani_amd import md

    states, n_k, cv, u = _harmonic(dev)
    x = torch.from_numpy(cv).to(dev)
    m = md.MBAR(states, n_k, x)
    m.solve(max_iterations=32, check_every=32)   # (allocations and the first use of every torch routine)
    values = x[:, 0] ** 2
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m.iterate(32, "adaptive")
        m.iterate(32, "self-consistent")
        w0, w5, wu = m.log_weights(0), m.log_weights(5), m.log_weights()
        a = m.expectation(values, 2)
        p = m.pmf(0, (-1.0, 3.0, 40), 5)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    want, _ = mr.solve(u, n_k, tolerance=1e-13)
    lw = mr.log_weights(u, n_k, want, u[2])
    assert abs(float(a) - (np.exp(lw) * cv[:, 0] ** 2).sum()) <= 1e-8
    assert abs(float(torch.logsumexp(wu, 0))) <= 1e-12 and abs(float(torch.logsumexp(w0, 0))) <= 1e-12
    F, counts = mr.pmf(mr.log_weights(u, n_k, want, u[5]), cv, [0], [-1.0], [3.0], [40])
    got = p.free_energy.cpu().numpy()
    full = counts > 0
    assert np.array_equal(p.counts.cpu().numpy(), counts) and np.isposinf(got[~full]).all()
    assert np.abs(got[full] - F[full]).max() <= 1e-8 and p.edges[0].shape == (41,)


def test_pooling_identical_states(dev):
    """Four restrained Lennard-Jones dimers, entries 0 and 2 in one window and 1 and 3 in another: ``from_dynamics`` pools them
    into two states, and f equals that of the four entries kept apart as four states (two pairs of identical rows)."""
    from test_gpu_md_bias import _dimers
    from torchani_amd import md

    centers = torch.tensor([3.4, 3.7, 3.4, 3.7], dtype=torch.float64)
    lj, sp, x, mass = _dimers(dev, 4, 0.005, 3.5)
    x[:, 1, 0] = centers.to(dev)
    dyn = md.BatchedDynamics(lj, sp, x, dt=2.0, masses=mass, temperature=300.0, friction=0.05, seed=9, remove_drift=False,
                             bias=[md.Restraint(md.distance(0, 1), centers, 0.05)])
    dyn.set_temperature(300.0)
    series = dyn.attach(md.TimeSeries(("cv",), every=10, capacity=20))
    dyn.run(200, check_every=200)
    pooled = md.MBAR.from_dynamics(dyn, series)
    assert pooled.n_states == 2 and pooled.n_k.tolist() == [40.0, 40.0] and pooled.n_samples == 80
    assert pooled.states.restraint[:, 0, 0].tolist() == [3.4, 3.7]
    pooled.solve(tolerance=1e-13, max_iterations=320)
    apart = md.MBAR(md.ThermodynamicStates(300.0, centers, 0.05), [20, 20, 20, 20], series.values("cv").reshape(-1, 1))
    apart.solve(tolerance=1e-13, max_iterations=320)
    assert pooled.converged and apart.converged
    f1, f2 = pooled.f.cpu().numpy(), apart.f.cpu().numpy()
    err = max(abs(f2[2] - f2[0]), abs(f2[3] - f2[1]), abs(f2[1] - f1[1]))
    print(f"mbar, two pairs of identical entries pooled by from_dynamics against four states kept apart: f = {f1[1]:.6f} kT, "
          f"max |df| {err:.1e}")
    assert err <= 1e-12


# max |F_MBAR - F_exact| / kT over the 48 bins, means removed, of tests/_mbar_ref.py::dimer_umbrella with umbrella_error (numpy,
# this protocol) over the seeds 0 .. 4: 0.2205, 0.0814, 0.0989, 0.0626, 0.1127, no empty bin in any.  The gate is twice the largest.
# (The stand-in that the protocol was first tried with gave 0.051 to 0.113 kT over the same seed numbers.  It is another program
# than this driver, so a seed names another trajectory there; four of the five runs here lie in its range and seed 0 is the
# largest draw of a statistical error.  The device run measured 0.093 kT.)
UMBRELLA_REFERENCE_WORST = 0.2205
UMBRELLA_GATE = 2.0 * UMBRELLA_REFERENCE_WORST


def test_umbrella_windows_recover_the_free_energy_of_a_dimer(dev):
    """17 windows at 3.1, 3.25, ..., 5.5 A on the distance of Lennard-Jones dimers (eps 0.005 Ha, sigma 3 A, mass 12.011), k =
    0.05 Ha / A^2, 64 copies each: Langevin at 300 K, 2 fs, friction 0.05 / fs, 1000 steps from the window centres, the distance
    recorded every 10 steps, the first 20 samples discarded.  The PMF at the unbiased state on 48 bins of 3.1 .. 5.5 A against
    U(r) - 2 kT ln r at the bin centres, means removed."""
    from test_gpu_md_bias import _dimers
    from torchani_amd import md

    p = mr.UMBRELLA
    centers = np.repeat(p["centers"], p["copies"])
    n, kT = len(centers), br.KB_HARTREE * p["T"]
    lj, sp, x, mass = _dimers(dev, n, p["eps"], 4.0)
    x[:, 1, 0] = torch.from_numpy(centers).to(dev)
    dyn = md.BatchedDynamics(lj, sp, x, dt=p["dt"], masses=mass, temperature=p["T"], friction=p["friction"], seed=3,
                             remove_drift=False,
                             bias=[md.Restraint(md.distance(0, 1), torch.from_numpy(centers), p["k"])])
    dyn.set_temperature(p["T"])
    series = dyn.attach(md.TimeSeries(("cv",), every=p["every"], capacity=p["steps"] // p["every"]))
    dyn.run(p["steps"], check_every=p["steps"])
    m = md.MBAR.from_dynamics(dyn, series, discard=p["discard"])
    assert m.n_states == 17 and m.n_samples == n * 80 and m.n_k.tolist() == [64.0 * 80] * 17
    m.solve()
    assert m.converged
    pmf = m.pmf(0, (p["lo"], p["hi"], p["bins"]))
    F, counts = pmf.free_energy.cpu().numpy(), pmf.counts.cpu().numpy()
    mid = 0.5 * (pmf.edges[0][1:] + pmf.edges[0][:-1]).cpu().numpy()
    exact = br.dimer_free_energy(mid, p["eps"], p["sigma"], kT) / kT
    flat = np.abs(exact - exact.mean()).max()
    assert (counts > 0).all(), counts
    err = np.abs((F - F.mean()) - (exact - exact.mean())).max()
    print(f"mbar, 17 umbrella windows x 64 LJ dimers, {m.n_samples} samples: {m.iterations} kernel iterations, max |dF| {err:.3f} kT "
          f"on 48 bins (numpy reference over 5 seeds: at most {UMBRELLA_REFERENCE_WORST} kT; gate {UMBRELLA_GATE:.3f} kT; a flat "
          f"F would be {flat:.2f} kT off; F spans {exact.max() - exact.min():.2f} kT); smallest bin {counts.min()} samples")
    assert flat > 2.0 * UMBRELLA_GATE
    assert err <= UMBRELLA_GATE


def test_temperature_ladder_matches_the_reference_on_the_recorded_series(dev):
    """The restrained Lennard-Jones dimer ladder of the replica-exchange tests, 8 ladders x 4 rungs, 200 steps: f and
    <potential> at every rung and at a temperature between two rungs against the numpy reference fed the recorded series."""
    from test_gpu_md_replica_exchange import DIMER
    from torchani_amd import md
    from torchani_amd.potentials import LennardJones

    L, K = 8, DIMER["rungs"]
    r0 = 2.0 ** (1.0 / 6.0)
    lj = LennardJones(("H",), eps=(0.002,), sigma=(1.0,)).to(dev)
    x = torch.zeros((L * K, 2, 3), device=dev)
    x[:, 1, 0] = r0
    T = md.temperature_ladder(DIMER["t_min"], DIMER["t_max"], K).repeat(L)
    rows = (r0, 0.01, 0.02)
    dyn = md.ReplicaExchangeDynamics(lj, torch.ones((L * K, 2), dtype=torch.int64, device=dev), x, dt=DIMER["dt"],
                                     masses=torch.full((L * K, 2), 12.011, device=dev), temperature=T,
                                     friction=DIMER["friction"], ladders=torch.arange(L * K).view(L, K), exchange_every=20, seed=11,
                                     remove_drift=False, bias=[md.Restraint(md.distance(0, 1), *rows)])
    dyn.set_temperature(T)
    series = dyn.attach(md.TimeSeries(("potential", "cv", "rung"), every=10, capacity=20))
    dyn.run(200, check_every=200)
    assert int(dyn.exchange_accepts.sum()) > 0
    for ladder in (0, 5):
        m = md.MBAR.from_dynamics(dyn, series, ladder=ladder)
        m.solve(tolerance=1e-12)
        on = slice(ladder * K, (ladder + 1) * K)
        E = series.values("potential")[:, on].reshape(-1).cpu().numpy()
        cv = series.values("cv")[:, on].reshape(-1, 1).cpu().numpy()
        rung = series.values("rung")[:, on].reshape(-1).cpu().numpy().astype(np.int64)
        n_k = np.bincount(rung, minlength=K).astype(np.float64)
        assert m.n_k.tolist() == n_k.tolist() == [20.0] * K and m.n_samples == 20 * K
        Tr = dyn.rung_temperatures[ladder].cpu().double().numpy()
        beta = 1.0 / (br.KB_HARTREE * Tr)
        restraint = np.tile(np.array(rows), (K, 1, 1))
        u = mr.reduced_potentials(beta, restraint, [0], E, cv)
        want, _ = mr.solve(u, n_k, tolerance=1e-13)
        err = np.abs(m.f.cpu().numpy() - want).max()
        Ed = torch.from_numpy(E).to(dev)
        worst = 0.0
        for k in range(K):
            worst = max(worst, abs(float(m.expectation(Ed, k)) - (np.exp(mr.log_weights(u, n_k, want, u[k])) * E).sum()))
        T_mid = 0.5 * (Tr[1] + Tr[2])
        u_mid = mr.reduced_potentials([1.0 / (br.KB_HARTREE * T_mid)], restraint[:1], [0], E, cv)[0]
        mid = float(m.expectation(Ed, md.ThermodynamicStates(T_mid, [[rows[0]]], rows[1], rows[2])))
        worst = max(worst, abs(mid - (np.exp(mr.log_weights(u, n_k, want, u_mid)) * E).sum()))
        print(f"mbar, ladder {ladder} of {L} x {K} restrained LJ dimers at {np.array2string(Tr, precision=1)} K, {m.n_samples} "
              f"samples: max |f - reference| {err:.1e}, max |<E> - reference| {worst:.1e} Ha; f = {np.array2string(want, precision=3)}")
        assert err <= 1e-8 and worst <= 1e-8
