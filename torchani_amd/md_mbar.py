"""MBAR on the device: free energies, potentials of mean force and reweighted averages from biased and tempered MD.

``MBAR`` is the multistate Bennett acceptance ratio estimator (Shirts and Chodera 2008; binless WHAM is the same equations) on
the kernels of csrc/mbar.hip (include/anihip.h has the exact definition).  A thermodynamic state is an inverse temperature and
one flat-bottom harmonic restraint row per CV column (``ThermodynamicStates``), a sample its potential energy and its CV values,
so the reduced potential u_k(x_n) is evaluated where it is needed and the N x K matrix never exists; ``from_reduced_potentials``
takes a dense matrix instead.  ``from_dynamics`` builds the problem from a ``TimeSeries`` recorded by ``BatchedDynamics``
(umbrella windows across the batch) or ``ReplicaExchangeDynamics`` (temperature ladders).

Out of scope: decorrelation and statistical inefficiencies (subsample with ``stride``: the uncertainties assume independent
samples), bootstrap, WHAM grids of more than two columns, pressure or volume in the reduced potential, and more than one GPU.
"""
from __future__ import annotations

import ctypes as C
import typing as tp

import torch
from torch import Tensor

from . import _lib
from .tuples import PMF

_KINDS = {"distance": _lib.MD_CV_DISTANCE, "angle": _lib.MD_CV_ANGLE, "dihedral": _lib.MD_CV_DIHEDRAL}
_SOLVERS = ("adaptive", "self-consistent")
ADAPTIVE_MAX_STATES = 1024
_SLAB_BYTES = 1 << 27   # of a slab of ln W [n, K] while W^T W is accumulated


def _f64(value) -> Tensor:
    # (a Python float must not pass through fp32)
    return value.detach().cpu().to(torch.float64) if isinstance(value, Tensor) else torch.as_tensor(value, dtype=torch.float64)


class ThermodynamicStates:
    """K states over R CV columns: ``temperature`` in K (a number or [K]), ``centers`` [K, R] (or [K] for one column), ``k``
    (Hartree per squared unit of the CV) and ``half_widths`` numbers or tensors that broadcast to [K, R], ``kinds`` one of
    "distance", "angle", "dihedral" (or the ANIHIP_MD_CV_* integer) per column, default "distance".  Without ``centers`` the
    states differ in temperature alone.  The restraint of a state is that of ``md.Restraint``: with d = s - center (wrapped
    into [-pi, pi) for a dihedral) and e = max(0, |d| - half_width), E = k e^2 / 2.  Host tensors: ``beta`` fp64 [K] in 1 /
    Hartree, ``restraint`` fp64 [K, R, 3], ``kinds`` int32 [R]."""

    def __init__(self, temperature, centers=None, k=None, half_widths=None, kinds=None) -> None:
        from .md import KB_HARTREE

        T = _f64(temperature)
        if T.dim() > 1:
            raise ValueError(f"temperature must be a number or a tensor of shape [K], got {tuple(T.shape)}")
        if centers is None:
            if k is not None or half_widths is not None or kinds is not None:
                raise ValueError("k, half_widths and kinds describe restraints: pass centers too")
            c = torch.zeros((T.numel(), 0), dtype=torch.float64)
        else:
            c = _f64(centers)
            if c.dim() == 0:
                c = c.reshape(1, 1)
            elif c.dim() == 1:
                c = c.unsqueeze(1)
            if c.dim() != 2:
                raise ValueError(f"centers must have shape [K, R] or [K], got {tuple(c.shape)}")
            if k is None:
                raise ValueError("centers without k: a restraint needs its force constant")
        K, R = c.shape
        if T.dim() == 1 and T.numel() != K:
            if K == 1:
                c, K = c.expand(T.numel(), R), T.numel()
            elif T.numel() != 1:
                raise ValueError(f"temperature holds {T.numel()} states and centers {K}")
        T = T.reshape(-1).expand(K) if T.numel() == 1 else T
        if K < 1:
            raise ValueError("at least one state is needed")
        if R > _lib.MD_BIAS_MAX_CVS:
            raise ValueError(f"{R} CV columns, more than {_lib.MD_BIAS_MAX_CVS}")
        if not bool((torch.isfinite(T) & (T > 0)).all()):
            raise ValueError("temperature must be > 0")
        rows = torch.zeros((K, R, 3), dtype=torch.float64)
        rows[..., 0] = c
        for slot, value, name in ((1, k, "k"), (2, half_widths, "half_widths")):
            if value is None:
                continue
            v = _f64(value)
            if v.dim() == 1 and R == 1 and v.numel() == K:
                v = v.unsqueeze(1)
            try:
                rows[..., slot] = v.expand(K, R) if v.dim() else v
            except RuntimeError:
                raise ValueError(f"{name} must broadcast to {(K, R)}, got {tuple(v.shape)}") from None
        if not bool(torch.isfinite(rows).all()) or bool((rows[..., 1:] < 0).any()):
            raise ValueError("centers must be finite, k and half_widths finite and >= 0")
        if kinds is None:
            kinds = ["distance"] * R
        kinds = [kinds] if isinstance(kinds, (str, int)) else list(kinds)
        if len(kinds) != R:
            raise ValueError(f"kinds must name {R} columns, got {len(kinds)}")
        codes = []
        for kind in kinds:
            code = _KINDS.get(kind, kind) if isinstance(kind, str) else int(kind)
            if code not in _KINDS.values():
                raise ValueError(f"unknown CV kind {kind!r}: one of {tuple(_KINDS)}")
            codes.append(code)
        self.temperature = T.clone()
        self.beta = 1.0 / (KB_HARTREE * T)
        self.restraint = rows.contiguous()
        self.kinds = torch.tensor(codes, dtype=torch.int32)

    @property
    def n_states(self) -> int:
        return int(self.beta.numel())

    @property
    def n_columns(self) -> int:
        return int(self.restraint.shape[1])


def _check_counts(n_k, K: int) -> Tensor:
    n = _f64(n_k).reshape(-1)
    if n.numel() != K:
        raise ValueError(f"n_k must hold one count per state ({K}), got {n.numel()}")
    if not bool((torch.isfinite(n) & (n >= 0) & (n == n.round())).all()):
        raise ValueError("n_k must hold counts: integers >= 0")
    if not bool((n > 0).any()):
        raise ValueError("n_k is zero everywhere: no state was sampled")
    return n


class MBAR:
    """``MBAR(states, n_k, cv=None, energies=None)``: K ``states`` (a ``ThermodynamicStates``), ``n_k`` [K] how many of the
    N samples were drawn in each (0: a state that was not sampled, for which f is predicted), ``cv`` fp64 [N, R] the CV values of
    the samples in the columns of ``states`` (device), ``energies`` fp64 [N] their potential energies in Hartree (device; None
    counts as zeros, which is exact when every state has the same temperature).  The order of the samples does not matter.

    ``solve()`` finds the reduced free energies f [K] (f[0] = 0); the read-outs, all on the device: ``free_energies``,
    ``uncertainties``, ``log_weights``, ``expectation`` and ``pmf``.  ``iterate``, ``log_weights``, ``expectation`` and ``pmf``
    never read on the host; ``solve`` reads ``delta`` once per ``check_every`` iterations."""

    def __init__(self, states: ThermodynamicStates, n_k, cv: tp.Optional[Tensor] = None,
                 energies: tp.Optional[Tensor] = None) -> None:
        if not isinstance(states, ThermodynamicStates):
            raise ValueError("states must be a ThermodynamicStates (MBAR.from_reduced_potentials takes a matrix)")
        K, R = states.n_states, states.n_columns
        counts = _check_counts(n_k, K)
        if cv is None and energies is None:
            raise ValueError("MBAR needs samples: cv [N, R], energies [N], or both")
        if R and cv is None:
            raise ValueError(f"the states restrain {R} CV columns: cv [N, {R}] is needed")
        if cv is not None:
            if cv.dim() == 1 and R == 1:
                cv = cv.unsqueeze(1)
            if cv.dim() != 2 or cv.shape[1] != R:
                raise ValueError(f"cv must have shape [N, {R}], got {tuple(cv.shape)}")
        N = int(cv.shape[0] if cv is not None else energies.shape[0])
        if energies is not None and tuple(energies.shape) != (N,):
            raise ValueError(f"energies must have shape ({N},), got {tuple(energies.shape)}")
        if N < 1 or int(counts.sum()) != N:
            raise ValueError(f"n_k sums to {int(counts.sum())} and there are {N} samples")
        if energies is None and bool((states.beta != states.beta[0]).any()):
            raise ValueError("states of different temperatures need the potential energies of the samples")
        first = cv if cv is not None else energies
        if not first.is_cuda:
            raise ValueError("MBAR needs tensors on a ROCm device (no CPU fallback)")
        dev = first.device
        self.states, self.device, self.dense = states, dev, False
        self._cv = (cv if cv is not None else torch.zeros((N, 0), device=dev)).to(device=dev, dtype=torch.float64).contiguous()
        self._energy = None if energies is None else energies.to(device=dev, dtype=torch.float64).contiguous()
        self._beta, self._rows, self._kinds = (t.to(dev).contiguous() for t in (states.beta, states.restraint, states.kinds))
        self._u = None
        self._finish(counts, K, R, N)

    @classmethod
    def from_reduced_potentials(cls, u_kn: Tensor, n_k) -> "MBAR":
        """The dense form: ``u_kn`` fp64 [K, N] (device), the reduced potential of every sample in every state."""
        if not isinstance(u_kn, Tensor) or u_kn.dim() != 2:
            raise ValueError("u_kn must be a tensor of shape [K, N]")
        K, N = u_kn.shape
        counts = _check_counts(n_k, K)
        if N < 1 or int(counts.sum()) != N:
            raise ValueError(f"n_k sums to {int(counts.sum())} and there are {N} samples")
        if not u_kn.is_cuda:
            raise ValueError("MBAR needs tensors on a ROCm device (no CPU fallback)")
        self = cls.__new__(cls)
        self.states, self.device, self.dense = None, u_kn.device, True
        self._u = u_kn.to(torch.float64).contiguous()
        self._cv, self._energy, self._beta, self._rows, self._kinds = None, None, None, None, None
        self._finish(counts, K, 0, N)
        return self

    def _finish(self, counts: Tensor, K: int, R: int, N: int) -> None:
        dev = self.device
        self.n_states, self.n_columns, self.n_samples = K, R, N
        self.n_k = counts.to(dev)
        self._sampled = (counts > 0).nonzero().view(-1).to(dev)   # (host knowledge: no device read later)
        self._first_sampled = int((counts > 0).nonzero()[0])
        self._sampled_mask = (counts > 0).to(dev)
        self._status = torch.zeros(1, dtype=torch.int32, device=dev)
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()   # noqa: E731
        self._problem = _lib.Mbar(N, K, R, ptr(self._beta), ptr(self.n_k), ptr(self._rows), ptr(self._kinds), ptr(self._energy),
                                  ptr(self._cv), ptr(self._u), self._status.data_ptr())
        nbytes = _lib.lib().anihip_mbar_workspace_bytes(C.byref(self._problem))
        if nbytes == 0:
            _lib.check(1)
        self._workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self._delta = torch.zeros(1, dtype=torch.float64, device=dev)
        self.f = torch.zeros(K, dtype=torch.float64, device=dev)
        self.iterations, self.weight_passes, self.converged, self.delta = 0, 0, False, float("inf")
        self._wtw: tp.Optional[Tensor] = None

    # ---- from a recorded trajectory -------------------------------------------------------------------------------------------
    @classmethod
    def from_dynamics(cls, dyn, series, discard: int = 0, stride: int = 1, ladder: int = 0) -> "MBAR":
        """The problem of a ``TimeSeries`` attached to ``dyn``.  On a ``BatchedDynamics`` the states are the distinct
        (temperature, restraint rows) among the entries, in the order of their first entry, and entries with identical
        parameters pool their samples into one state.  On a ``ReplicaExchangeDynamics`` the states are the rungs of ladder
        ``ladder`` and a sample belongs to the rung that its entry held when it was taken ("rung" must be recorded).  The
        samples are those ``discard``, ``discard + stride``, ... of the series.  "cv" must be recorded when the dynamics has
        restraints and "potential" when the temperatures differ (at one temperature the energy cancels).

        Raises ValueError for a dynamics with ``Metadynamics`` (a time-dependent bias is not a state), a ring that has wrapped
        (its samples are no longer the trajectory from a known start), a NaN in a CV column (an entry without that CV), ring
        polymers, a barostat (no volume in the reduced potential) and a ladder whose entries hold different restraints."""
        states, n_k, cv, energy, entries = cls._tables_from_dynamics(dyn, series, discard, stride, ladder)
        self = cls(states, n_k, cv, energy)
        self.entries = entries
        return self

    @staticmethod
    def _tables_from_dynamics(dyn, series, discard: int, stride: int, ladder: int):
        """(states, n_k, cv [N, R] or None, energies [N] or None, the entries used): what ``from_dynamics`` hands to the
        constructor, on the device of the series."""
        from . import md

        if isinstance(dyn, md.RingPolymerDynamics):
            raise ValueError("MBAR.from_dynamics does not take ring polymers: a bead is not a sample of the physical system")
        if getattr(dyn, "barostat", False):
            raise ValueError("MBAR.from_dynamics does not take a barostat: the reduced potential has no pressure-volume term")
        bias = dyn._bias
        if bias is not None and bias.n_lists:
            raise ValueError("MBAR.from_dynamics does not take Metadynamics: a time-dependent bias is not a thermodynamic state")
        if series._dyn is not dyn:
            raise ValueError("the TimeSeries is not attached to this dynamics")
        if series.n_samples > series.capacity:
            raise ValueError(f"the TimeSeries has wrapped ({series.n_samples} samples in a ring of {series.capacity}): MBAR needs "
                             "every sample since the start it discards from")
        for name, value, low in (("discard", discard, 0), ("stride", stride, 1)):
            if isinstance(value, bool) or int(value) != value or value < low:
                raise ValueError(f"{name} must be an integer >= {low}, got {value}")
        n_kept = len(range(int(discard), series.n_samples, int(stride)))
        if n_kept < 1:
            raise ValueError(f"discard = {discard} leaves none of the {series.n_samples} samples")
        keep = slice(int(discard), None, int(stride))
        Cn = int(dyn.species.shape[0])
        # the restraint rows of every entry [C, R, 3] and the kinds [R] (host tables of the bias)
        if bias is None:
            rows, kinds, R = torch.zeros((Cn, 0, 3), dtype=torch.float64), torch.zeros(0, dtype=torch.int32), 0
        else:
            t = bias.tables
            idx = t.cv_index
            R = int(idx.shape[1])
            if bool((idx < 0).any()):
                c, r = (int(v) for v in (idx < 0).nonzero()[0])
                raise ValueError(f"entry {c} does not have CV column {r} (a NaN in the series): every entry needs every column")
            rows, kinds = t.restraint[idx], t.kind[idx[0]]
            if bool((t.kind[idx] != kinds.view(1, R)).any()):
                raise ValueError("the entries disagree in the kind of a CV column")
        if R and "cv" not in series.quantities:
            raise ValueError('the dynamics has restraints: the TimeSeries must record "cv"')
        laddered = isinstance(dyn, md.ReplicaExchangeDynamics)
        if laddered:
            if isinstance(ladder, bool) or int(ladder) != ladder or not 0 <= ladder < dyn.n_ladders:
                raise ValueError(f"ladder must be an integer in 0 .. {dyn.n_ladders - 1}, got {ladder}")
            if "rung" not in series.quantities:
                raise ValueError('a ladder needs the rung of every sample: the TimeSeries must record "rung"')
            slots = dyn._slot[int(ladder)].cpu().long()
            entries = slots[slots >= 0].sort().values
            if R and bool((rows[entries] != rows[entries[:1]]).any()):
                raise ValueError(f"the entries of ladder {ladder} hold different restraints: its rungs differ in temperature alone")
            T = dyn.rung_temperatures[int(ladder), :entries.numel()].cpu().double()
            states = ThermodynamicStates(T, rows[entries[0], :, 0].unsqueeze(0) if R else None, rows[entries[0], :, 1] if R else None,
                                         rows[entries[0], :, 2] if R else None, kinds.tolist() if R else None)
        else:
            entries = torch.arange(Cn)
            T = dyn.temperature.cpu().double()
            if not getattr(dyn, "langevin", True):
                raise ValueError("MBAR.from_dynamics needs a thermostat: NVE samples belong to no temperature")
            key = torch.cat([T.view(Cn, 1), rows.reshape(Cn, 3 * R)], dim=1)
            uniq, inverse = torch.unique(key, dim=0, return_inverse=True)
            first = torch.full((uniq.shape[0],), Cn, dtype=torch.int64).scatter_reduce(0, inverse, torch.arange(Cn), "amin")
            order = torch.argsort(first)
            rank = torch.empty_like(order)
            rank[order] = torch.arange(order.numel())
            state_of = rank[inverse]
            lead = first[order]
            states = ThermodynamicStates(T[lead], rows[lead, :, 0] if R else None, rows[lead, :, 1] if R else None,
                                         rows[lead, :, 2] if R else None, kinds.tolist() if R else None)
        K = states.n_states
        need_energy = bool((states.beta != states.beta[0]).any())
        if need_energy and "potential" not in series.quantities:
            raise ValueError('the temperatures differ: the TimeSeries must record "potential"')
        dev = dyn.coordinates.device
        on = entries.to(dev)
        cv = None
        if R:
            cv = series.values("cv")[keep][:, on]   # [n, E, R]
            if bool(torch.isnan(cv).any()):
                raise ValueError("NaN in a CV column of the series: every entry needs every column")
            cv = cv.reshape(-1, R)
        energy = series.values("potential")[keep][:, on].reshape(-1) if need_energy else None
        if laddered:
            rung = series.values("rung")[keep][:, on].reshape(-1).cpu().long()
            if bool(((rung < 0) | (rung >= K)).any()):
                raise ValueError(f"the series holds rungs outside 0 .. {K - 1}")
            n_k = torch.bincount(rung, minlength=K)
        else:
            n_k = torch.bincount(state_of, minlength=K) * n_kept
        return states, n_k, cv, energy, entries

    # ---- the solver -----------------------------------------------------------------------------------------------------------
    def _iterate(self, f_in: Tensor, n: int, f_out: Tensor) -> None:
        from .engine import _stream

        _lib.check(_lib.lib().anihip_mbar_iterate(_stream(), C.byref(self._problem), f_in.data_ptr(), int(n), f_out.data_ptr(),
                                                  self._delta.data_ptr(), self._workspace.data_ptr(), self._workspace.numel()))
        self.iterations += int(n)

    def _weights_product(self, f: Tensor) -> tp.Tuple[Tensor, Tensor]:
        """(W^T W [K, K], column sums of W [K]) over slabs of ln W [n, K]: N x K is never held."""
        from .engine import _stream

        K, N = self.n_states, self.n_samples
        slab = max(1, min(N, _SLAB_BYTES // (8 * K)))
        buf = torch.empty((slab, K), dtype=torch.float64, device=self.device)
        wtw = torch.zeros((K, K), dtype=torch.float64, device=self.device)
        sums = torch.zeros(K, dtype=torch.float64, device=self.device)
        for first in range(0, N, slab):
            n = min(slab, N - first)
            _lib.check(_lib.lib().anihip_mbar_log_weights(
                _stream(), C.byref(self._problem), f.data_ptr(), _lib.MBAR_TARGET_ALL, None, None, None, first, n, buf.data_ptr(),
                self._workspace.data_ptr(), self._workspace.numel()))
            W = buf[:n].exp()
            wtw += W.T @ W
            sums += W.sum(dim=0)
        self.weight_passes += 1
        return wtw, sums

    def _gradient(self, f: Tensor, f_next: Tensor) -> Tensor:
        """The gradient of the MBAR objective at f from one iteration f -> f_next: sum_n W_nk = exp(f_k - f'_k - c), and c from
        sum_k N_k sum_n W_nk = N."""
        s = (f - f_next).exp()
        s = s * (self.n_samples / (self.n_k * s).sum())
        return self.n_k * (s - 1.0)

    def _adaptive_step(self, f: Tensor, f_sci: Tensor) -> tp.Tuple[Tensor, Tensor]:
        """From f and its iterate f_sci to the next (f, iterate): the Newton candidate on the sampled states (the first one
        pinned) when the norm of its gradient is the smaller one, the self-consistent step otherwise (pymbar's adaptive rule).
        Two kernel iterations and one pass over the weights; the choice is made on the device."""
        wtw, sums = self._weights_product(f)
        on = self._sampled
        free = on[1:]
        n_on = self.n_k[free]
        g = n_on * (sums[free] - 1.0)
        H = torch.diag(n_on * sums[free]) - n_on.view(-1, 1) * wtw[free][:, free] * n_on.view(1, -1)
        L, _ = torch.linalg.cholesky_ex(H)
        step = torch.cholesky_solve(g.view(-1, 1), L).view(-1)
        f_nr = f.clone()
        f_nr.index_add_(0, free, -step)
        nr_next, sci_next = torch.empty_like(f), torch.empty_like(f)
        self._iterate(f_nr, 1, nr_next)
        self._iterate(f_sci, 1, sci_next)
        # (the unsampled states of the candidate follow from the sampled ones: they are those of its iterate, up to the shift)
        off_shift = nr_next + (f_nr[self._first_sampled] - nr_next[self._first_sampled])
        f_nr = torch.where(self._sampled_mask, f_nr, off_shift)
        f_nr = f_nr - f_nr[0]
        g_nr, g_sci = self._gradient(f_nr, nr_next), self._gradient(f_sci, sci_next)
        take = (g_nr * g_nr).sum() < (g_sci * g_sci).sum()   # (False for a NaN: a failed factorization falls back)
        return torch.where(take, f_nr, f_sci), torch.where(take, nr_next, sci_next)

    def iterate(self, n_iterations: int, solver: str = "self-consistent") -> None:
        """One block of the solver on ``f``, without a host read: ``n_iterations`` kernel iterations ("self-consistent"), or one
        kernel iteration and ``(n_iterations - 1) // 2`` adaptive steps of two each ("adaptive": never more than ``n_iterations``
        in all; fewer than three leave no room for a step and run self-consistently).  ``_delta`` (device) holds max |f' - f|
        of the last iteration."""
        if solver not in _SOLVERS:
            raise ValueError(f"solver must be one of {_SOLVERS}, got {solver!r}")
        if isinstance(n_iterations, bool) or int(n_iterations) != n_iterations or n_iterations < 1:
            raise ValueError(f"n_iterations must be an integer >= 1, got {n_iterations}")
        self._wtw = None
        if solver == "self-consistent" or self._sampled.numel() < 2 or int(n_iterations) < 3:
            self._iterate(self.f, int(n_iterations), self.f)
            return
        if self.n_states > ADAPTIVE_MAX_STATES:
            raise ValueError(f'solver="adaptive" handles up to {ADAPTIVE_MAX_STATES} states (it factorizes a K x K matrix): '
                             'use "self-consistent"')
        f, nxt = self.f, torch.empty_like(self.f)
        self._iterate(f, 1, nxt)
        for _ in range((int(n_iterations) - 1) // 2):
            f, nxt = self._adaptive_step(f, nxt)
        self._delta.copy_((nxt - f).abs().max().view(1))
        self.f = nxt

    def solve(self, tolerance: float = 1e-10, max_iterations: int = 10000, solver: str = "adaptive",
              check_every: int = 32) -> Tensor:
        """Iterate from the current ``f`` until an iteration moves no f_k by more than ``tolerance`` (in kT), in blocks of
        ``check_every`` kernel iterations with one host read of ``delta`` after each.  solver: "self-consistent" (the kernel
        alone), or "adaptive" (K <= 1024): within a block, steps that take the Newton candidate from the gradient and Hessian
        of the MBAR objective (from W^T W, accumulated by matmul over slabs of log weights, state 0 pinned) when its gradient
        norm is the smaller one and the self-consistent step otherwise.  Sets ``f``, ``iterations`` (kernel iterations, this call),
        ``weight_passes``, ``converged`` and ``delta``; returns ``f``.  Raises RuntimeError for tables that the kernels refuse."""
        if not tolerance > 0:
            raise ValueError(f"tolerance must be > 0, got {tolerance}")
        for name, value in (("max_iterations", max_iterations), ("check_every", check_every)):
            if isinstance(value, bool) or int(value) != value or value < 1:
                raise ValueError(f"{name} must be an integer >= 1, got {value}")
        if solver not in _SOLVERS:
            raise ValueError(f"solver must be one of {_SOLVERS}, got {solver!r}")
        self.iterations, self.weight_passes, self.converged = 0, 0, False
        while self.iterations < max_iterations and not self.converged:
            self.iterate(min(int(check_every), int(max_iterations) - self.iterations), solver)
            self.delta = float(self._delta)   # (the one host read of the block)
            self.raise_on_status()
            self.converged = self.delta < tolerance
        return self.f

    def raise_on_status(self) -> None:
        """Raise on what the kernels found wrong in the tables (one host synchronization)."""
        bits = int(self._status)
        if bits:
            what = [text for bit, text in ((_lib.MBAR_BAD_COUNTS, "a count that is negative or not finite, or no count above 0"),
                                           (_lib.MBAR_BAD_SAMPLES, "an energy, a CV value or a reduced potential that is not finite"),
                                           (_lib.MBAR_BAD_STATES, "a state whose temperature or restraint row is out of range"))
                    if bits & bit]
            raise RuntimeError("MBAR: " + "; ".join(what) + " (nothing was written)")

    # ---- read-outs, on the device ---------------------------------------------------------------------------------------------
    def free_energies(self, unit: str = "kT") -> Tensor:
        """fp64 [K]: f_k - f_0 in kT of each state ("kT"), or f_k / beta_k in Hartree ("hartree", structured problems)."""
        if unit == "kT":
            return self.f.clone()
        if unit != "hartree":
            raise ValueError(f'unit must be "kT" or "hartree", got {unit!r}')
        if self.dense:
            raise ValueError('a dense problem has no temperatures: unit="kT" only')
        return self.f / self._beta

    def uncertainties(self) -> Tensor:
        """fp64 [K, K]: the standard error of f_i - f_j in kT from the asymptotic covariance of Shirts and Chodera (2008) in
        its K x K form: with W^T W = V S^2 V^T, Theta = V S pinv(I - S V^T N V S) S V^T, eigenvalues of the inner matrix
        below 1e-10 of the largest counting as zero.  Independent samples are assumed."""
        wtw, _ = self._weights_product(self.f)
        s2, V = torch.linalg.eigh(wtw)
        S = s2.clamp(min=0.0).sqrt()
        inner = torch.eye(self.n_states, dtype=torch.float64, device=self.device) - S.view(-1, 1) * (V.T @ (self.n_k.view(-1, 1) * V)) * S
        w, Q = torch.linalg.eigh(0.5 * (inner + inner.T))
        keep = w.abs() > 1e-10 * w.abs().max()
        inv = torch.where(keep, 1.0 / torch.where(keep, w, torch.ones_like(w)), torch.zeros_like(w))
        VS = V * S
        theta = VS @ ((Q * inv) @ Q.T) @ VS.T
        dg = theta.diagonal()
        return (dg.view(-1, 1) + dg.view(1, -1) - 2.0 * theta).clamp(min=0.0).sqrt()

    def _target(self, state):
        """(index, beta, rows, u) of anihip_mbar_log_weights for ``state``."""
        if state is None:
            if self.dense:
                raise ValueError("a dense problem has no unbiased state: pass a state index or the reduced potentials [N]")
            return _lib.MBAR_TARGET_EXTERNAL, self._beta[:1], torch.zeros((max(1, self.n_columns), 3), dtype=torch.float64,
                                                                          device=self.device), None
        if isinstance(state, ThermodynamicStates):
            if self.dense:
                raise ValueError("a dense problem takes a state index or the reduced potentials [N] of the target")
            if state.n_states != 1 or state.n_columns != self.n_columns or not torch.equal(state.kinds, self.states.kinds):
                raise ValueError(f"a target is one state over the {self.n_columns} columns of the problem, of the same kinds")
            return _lib.MBAR_TARGET_EXTERNAL, state.beta.to(self.device), state.restraint[0].to(self.device).contiguous(), None
        if isinstance(state, Tensor):
            if not self.dense or tuple(state.shape) != (self.n_samples,):
                raise ValueError(f"reduced potentials of a target fit a dense problem and have shape ({self.n_samples},)")
            return _lib.MBAR_TARGET_EXTERNAL, None, None, state.to(device=self.device, dtype=torch.float64).contiguous()
        if isinstance(state, bool) or int(state) != state or not 0 <= state < self.n_states:
            raise ValueError(f"state must be an index in 0 .. {self.n_states - 1}, a one-state ThermodynamicStates or None")
        return int(state), None, None, None

    def log_weights(self, state=None) -> Tensor:
        """fp64 [N]: ln W_n of every sample in ``state``: an index, a one-state ``ThermodynamicStates`` that need not be among
        the sampled ones, or None for the unbiased state at the first temperature.  Their log-sum-exp is 0."""
        from .engine import _stream

        index, beta, rows, u = self._target(state)
        out = torch.empty(self.n_samples, dtype=torch.float64, device=self.device)
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        _lib.check(_lib.lib().anihip_mbar_log_weights(
            _stream(), C.byref(self._problem), self.f.data_ptr(), index, ptr(beta), ptr(rows), ptr(u), 0, self.n_samples,
            out.data_ptr(), self._workspace.data_ptr(), self._workspace.numel()))
        return out

    def expectation(self, values: Tensor, state=None) -> Tensor:
        """sum_n W_n A_n of ``values`` [N] or [N, ...] (device) in ``state`` (as for ``log_weights``), fp64."""
        if values.shape[:1] != (self.n_samples,):
            raise ValueError(f"values must have shape [{self.n_samples}, ...], got {tuple(values.shape)}")
        w = self.log_weights(state).exp()
        a = values.to(device=self.device, dtype=torch.float64)
        return (w.view(-1, *([1] * (a.dim() - 1))) * a).sum(dim=0)

    def pmf(self, columns, edges, state=None) -> PMF:
        """The potential of mean force along one or two CV columns in ``state``: ``columns`` an index or a pair of them,
        ``edges`` (lo, hi, bins) per column, uniform (for one column the triple itself).  A sample on an edge belongs to the
        bin on its right; samples below lo or at and above hi are left out.  Returns ``PMF(free_energy, edges, counts)``: in
        kT, the minimum at 0, inf in empty bins."""
        from .engine import _stream

        if self.dense:
            raise ValueError("a dense problem has no CV columns: histogram log_weights() yourself")
        columns = [columns] if isinstance(columns, int) else list(columns)
        if len(columns) == 1 and len(edges) == 3 and not isinstance(edges[0], (tuple, list)):
            edges = [edges]
        edges = [tuple(e) for e in edges]
        if len(columns) not in (1, 2) or len(edges) != len(columns) or any(len(e) != 3 for e in edges):
            raise ValueError("pmf takes one or two columns and (lo, hi, bins) for each")
        n = len(columns)
        bins = [int(e[2]) for e in edges]
        total = bins[0] * (bins[1] if n == 2 else 1)
        for c, (lo, hi, b) in zip(columns, edges):
            if isinstance(c, bool) or int(c) != c or not 0 <= c < self.n_columns:
                raise ValueError(f"column must be in 0 .. {self.n_columns - 1}, got {c}")
            if int(b) != b or b < 1 or not hi > lo:
                raise ValueError(f"edges need lo < hi and bins >= 1, got {(lo, hi, b)}")
        if total > _lib.MBAR_MAX_BINS:
            raise ValueError(f"{total} bins in all, more than {_lib.MBAR_MAX_BINS}")
        lw = self.log_weights(state)
        L = _lib.lib()
        ws = torch.empty(L.anihip_mbar_histogram_workspace_bytes(self.n_samples, total), dtype=torch.uint8, device=self.device)
        lse = torch.empty(total, dtype=torch.float64, device=self.device)
        counts = torch.empty(total, dtype=torch.int64, device=self.device)
        _lib.check(L.anihip_mbar_histogram(
            _stream(), self.n_samples, lw.data_ptr(), self._cv.data_ptr(), self.n_columns, n, (C.c_int32 * 2)(*columns),
            (C.c_double * 2)(*[float(e[0]) for e in edges]), (C.c_double * 2)(*[float(e[1]) for e in edges]),
            (C.c_int32 * 2)(*bins), lse.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel()))
        F = -lse
        F = torch.where(torch.isinf(F), F, F - F.min()).view(*bins)   # (every bin empty: inf everywhere, not inf - inf)
        grids = tuple(torch.linspace(float(lo), float(hi), int(b) + 1, dtype=torch.float64, device=self.device) for lo, hi, b in edges)
        return PMF(F, grids, counts.view(*bins))
