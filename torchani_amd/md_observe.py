"""Observers of ``md.BatchedDynamics``: what a trajectory is sampled for, accumulated on the device.

``dyn.attach(observer)`` makes ``step()`` sample the state it leaves behind whenever ``steps_done % observer.every == 0``: after the
kick, after a metadynamics deposit and after a replica-exchange attempt.  A sample queues work on the stream and never reads on
the host; ``run()`` reads the observers' status words with its other periodic checks.  ``TimeSeries`` and ``Trajectory`` are
plain copies into device rings; ``RadialDistribution``, ``MeanSquaredDisplacement`` and ``VelocityAutocorrelation`` run the
kernels of csrc/md_observe.hip (include/anihip.h has their exact definitions).  ``HeatFlux`` and ``HeatFluxAutocorrelation``
evaluate the model's flux stage at a sample (anihip_aev_backward_flux, anihip_md_heat_flux): one extra evaluation each.
"""
from __future__ import annotations

import ctypes as C
import math
import typing as tp

import torch
from torch import Tensor

from . import _lib

LIGHT_SPEED_CM_PER_FS = 2.99792458e-5   # c in cm / fs: wavenumber = omega / (2 pi c)
_SERIES = ("potential", "kinetic", "total", "temperature", "bias", "volume", "pressure", "cv", "rung")


def _positive_int(value, name: str, low: int = 1) -> int:
    if isinstance(value, bool) or int(value) != value or value < low:
        raise ValueError(f"{name} must be an integer >= {low}, got {value}")
    return int(value)


class Observer:
    """What ``BatchedDynamics.attach`` takes: ``every`` (steps between samples), ``n_samples`` (taken so far, a host count)."""

    every: int

    def __init__(self, every: int) -> None:
        self.every = _positive_int(every, "every")
        self.n_samples = 0
        self._dyn = None

    def _attach(self, dyn) -> None:
        """The refusals (host only, before anything is allocated), then the device buffers."""
        if self._dyn is not None:
            raise ValueError("this observer is attached already: an observer watches one dynamics")
        self._check(dyn)
        self._dyn = dyn
        self._allocate(dyn)

    def _check(self, dyn) -> None:
        pass

    def _allocate(self, dyn) -> None:
        pass

    def _sample(self, dyn) -> None:
        raise NotImplementedError

    def reset(self) -> None:
        """Forget every sample."""
        self.n_samples = 0

    def raise_on_status(self) -> None:
        """Raise on what a sample found wrong on the device (one host synchronization); ``run()`` calls it."""

    def _need_attached(self):
        if self._dyn is None:
            raise ValueError("attach the observer to a dynamics first: dyn.attach(observer)")
        return self._dyn


class _Ring(Observer):
    """A ring of ``capacity`` samples with their step numbers on the host.  ``on_full``: "raise" at the sample that does not
    fit, or "wrap" over the oldest."""

    def __init__(self, every: int, capacity: int, on_full: str) -> None:
        super().__init__(every)
        self.capacity = _positive_int(capacity, "capacity")
        if on_full not in ("raise", "wrap"):
            raise ValueError(f'on_full must be "raise" or "wrap", got {on_full!r}')
        self.on_full = on_full
        self._steps: tp.List[int] = []

    def _slot(self, dyn) -> int:
        """The slot of the sample being taken (counted from the host-side number of samples)."""
        if self.n_samples >= self.capacity and self.on_full == "raise":
            raise RuntimeError(f"{type(self).__name__} is full: {self.capacity} samples taken (step {dyn.steps_done}); a larger "
                               'capacity, a larger every, or on_full="wrap"')
        self._steps.append(int(dyn.steps_done))
        if len(self._steps) > self.capacity:
            del self._steps[0]
        k = self.n_samples % self.capacity
        self.n_samples += 1
        return k

    def _ordered(self, buf: Tensor) -> Tensor:
        """The samples held, oldest first (a copy)."""
        n = self.n_samples
        if n <= self.capacity:
            return buf[:n].clone()
        k = n % self.capacity
        return torch.cat([buf[k:], buf[:k]])

    def steps(self) -> Tensor:
        """int64 [n] (host): ``steps_done`` at the samples held, oldest first."""
        return torch.tensor(self._steps, dtype=torch.int64)

    def reset(self) -> None:
        super().reset()
        self._steps.clear()


class TimeSeries(_Ring):
    """Series of per-entry quantities: ``quantities`` out of "potential", "kinetic", "total", "temperature", "bias", "volume",
    "pressure" (the values ``potential_energies``, ``kinetic_energies()``, ``total_energies()``, ``temperatures()``,
    ``bias_energies``, ``volumes()`` and ``pressures()`` have at that step), "cv" (``collective_variables()``, every column) and
    "rung" (``rungs()`` of ``ReplicaExchangeDynamics``).  Each is kept in an fp64 device buffer [capacity, ...]; a quantity that
    the dynamics does not have raises at ``attach``."""

    def __init__(self, quantities: tp.Sequence[str], every: int, capacity: int, on_full: str = "raise") -> None:
        super().__init__(every, capacity, on_full)
        quantities = (quantities,) if isinstance(quantities, str) else tuple(quantities)
        for q in quantities:
            if q not in _SERIES:
                raise ValueError(f"unknown quantity {q!r}: TimeSeries has {_SERIES}")
        if not quantities or len(set(quantities)) != len(quantities):
            raise ValueError("quantities must name at least one quantity, each once")
        self.quantities = quantities
        self._buffers: tp.Dict[str, Tensor] = {}

    def _read(self, dyn, q: str) -> Tensor:
        if q == "potential":
            return dyn.potential_energies
        if q == "bias":
            return dyn.bias_energies
        accessor = {"kinetic": "kinetic_energies", "total": "total_energies", "temperature": "temperatures", "volume": "volumes",
                    "pressure": "pressures", "cv": "collective_variables", "rung": "rungs"}[q]
        return getattr(dyn, accessor)()

    def _check(self, dyn) -> None:
        for q in self.quantities:
            if q in ("bias", "cv") and dyn._bias is None:
                raise ValueError(f'TimeSeries: "{q}" needs a dynamics with bias=')
            if q == "volume" and dyn.cell is None:
                raise ValueError('TimeSeries: "volume" needs a cell')
            if q == "pressure" and not dyn.barostat:
                raise ValueError('TimeSeries: "pressure" needs the virial, which only a dynamics with pressure= evaluates')
            if q == "rung" and not hasattr(dyn, "rungs"):
                raise ValueError('TimeSeries: "rung" needs a ReplicaExchangeDynamics')

    def _allocate(self, dyn) -> None:
        for q in self.quantities:
            first = self._read(dyn, q)
            self._buffers[q] = torch.zeros((self.capacity,) + tuple(first.shape), dtype=torch.float64, device=first.device)

    def _sample(self, dyn) -> None:
        k = self._slot(dyn)
        for q in self.quantities:
            self._buffers[q][k].copy_(self._read(dyn, q))

    def values(self, name: str) -> Tensor:
        """fp64 [n, ...]: the series of ``name``, oldest first."""
        if name not in self._buffers:
            raise ValueError(f"{name!r} is not recorded: this TimeSeries holds {self.quantities}")
        return self._ordered(self._buffers[name])


class Trajectory(_Ring):
    """A device ring of frames: ``coordinates`` as held (fp32), or ``coordinates + coordinates_lo`` summed in fp64
    (``dtype=torch.float64``); with ``velocities=True`` the velocities too (fp32), and the fp64 cell where a barostat moves it."""

    def __init__(self, every: int, capacity: int, velocities: bool = False, dtype: torch.dtype = torch.float32,
                 on_full: str = "raise") -> None:
        super().__init__(every, capacity, on_full)
        if dtype not in (torch.float32, torch.float64):
            raise ValueError(f"dtype must be torch.float32 or torch.float64, got {dtype}")
        self.velocities, self.dtype = bool(velocities), dtype
        self._frames = self._vframes = self._cells = None

    def _allocate(self, dyn) -> None:
        shape, dev = (self.capacity,) + tuple(dyn.coordinates.shape), dyn.coordinates.device
        self._frames = torch.zeros(shape, dtype=self.dtype, device=dev)
        if self.velocities:
            self._vframes = torch.zeros(shape, dtype=torch.float32, device=dev)
        if dyn.barostat:
            self._cells = torch.zeros((self.capacity, 3, 3), dtype=torch.float64, device=dev)

    def _sample(self, dyn) -> None:
        k = self._slot(dyn)
        if self.dtype == torch.float64:
            torch.add(dyn.coordinates.double(), dyn.coordinates_lo.double(), out=self._frames[k])
        else:
            self._frames[k].copy_(dyn.coordinates)
        if self._vframes is not None:
            self._vframes[k].copy_(dyn.velocities)
        if self._cells is not None:
            self._cells[k].copy_(dyn.cell64.view(3, 3))

    def frames(self) -> Tensor:
        """[n, C, A, 3], oldest first."""
        self._need_attached()
        return self._ordered(self._frames)

    def velocity_frames(self) -> Tensor:
        """fp32 [n, C, A, 3], oldest first."""
        self._need_attached()
        if self._vframes is None:
            raise ValueError("this Trajectory keeps no velocities: pass velocities=True")
        return self._ordered(self._vframes)

    def cells(self) -> Tensor:
        """fp64 [n, 3, 3], oldest first: the cell at every frame (the constant one without a barostat)."""
        dyn = self._need_attached()
        if self._cells is not None:
            return self._ordered(self._cells)
        if dyn.cell is None:
            raise ValueError("cells() needs a cell")
        n = min(self.n_samples, self.capacity)
        return dyn.cell.to(device=dyn.coordinates.device, dtype=torch.float64).view(1, 3, 3).repeat(n, 1, 1)


def _element_indices(dyn) -> Tensor:
    """int32 [C, A]: the model's element indices of the batch (-1: padding), as the neighbor rows carry them."""
    ev = dyn._model_eval
    if ev.standalone:
        return ev._species32
    return dyn.model._elem_idxs(dyn.species).to(torch.int32).contiguous()


class RadialDistribution(Observer):
    """Pair-distance histograms up to ``r_max`` (Angstrom) in ``bins`` bins of width ``r_max / bins`` for at most 8 ``pairs``
    (a, b) of the model's symbols, ordered: central atoms of element a, neighbors of element b.  At a sample the neighbor
    rows of the current coordinates are built by an ``AevEngine`` whose radial cutoff is ``r_max`` (rows of at most 256
    entries, "batch" or "cell" mode by the rule of the standalone potentials) and anihip_md_rdf_accumulate adds them to
    ``counts()``: uint64 [P, bins] summed over the entries, or [C, P, bins] with ``per_entry=True``.  Periodic images count as
    the engine counts them, an atom's own image included, so ``r_max`` may exceed half the smallest width of the cell.  An
    atom with more than 256 neighbors within ``r_max`` raises at the next periodic check of ``run()``: lower ``r_max``.

    ``coordination_numbers()`` is the running integral per central atom and works with or without a cell.  ``g()`` is
    ``counts <V> / (n_samples N_a N_b shell volume)`` with exact shell volumes, N_a N_b summed over the entries (every entry
    lives in the one cell of the batch) and <V> the mean of the volumes at the samples, accumulated on the device; under a
    barostat that normalization neglects the covariance of the counts with the volume.  It needs a cell that is periodic in
    all three directions."""

    def __init__(self, pairs: tp.Sequence[tp.Tuple[str, str]], r_max: float, bins: int, every: int, per_entry: bool = False) -> None:
        super().__init__(every)
        pairs = [tuple(p) for p in pairs]
        if not 1 <= len(pairs) <= _lib.MD_RDF_MAX_PAIRS or any(len(p) != 2 for p in pairs):
            raise ValueError(f"pairs must hold 1 .. {_lib.MD_RDF_MAX_PAIRS} pairs (a, b) of element symbols")
        if len(set(pairs)) != len(pairs):
            raise ValueError("a pair is given twice (pairs are ordered: (a, b) and (b, a) are two)")
        self.bins = _positive_int(bins, "bins")
        if self.bins > _lib.MD_RDF_MAX_BINS:
            raise ValueError(f"bins must be at most {_lib.MD_RDF_MAX_BINS}, got {bins}")
        if len(pairs) * self.bins > 8192:
            raise ValueError(f"pairs x bins must be at most 8192 (the workgroup's histogram), got {len(pairs)} x {bins}")
        if not (r_max > 1e-2 and math.isfinite(r_max)):
            raise ValueError(f"r_max must be > 0.01 Angstrom, got {r_max}")
        self.pairs, self.r_max, self.per_entry = pairs, float(r_max), bool(per_entry)
        self._counts = None

    def _check(self, dyn) -> None:
        symbols = tuple(dyn.model.symbols)
        if len(symbols) > 7:
            raise ValueError("RadialDistribution: at most 7 elements (the species field of a neighbor row)")
        for p in self.pairs:
            for s in p:
                if s not in symbols:
                    raise ValueError(f"RadialDistribution: {s!r} is not an element of the model, which has {symbols}")

    def _allocate(self, dyn) -> None:
        from .constants import aev_constants_2x
        from .engine import AevEngine

        symbols = tuple(dyn.model.symbols)
        self._slot_table = (C.c_int8 * 64)(*([-1] * 64))
        for p, (a, b) in enumerate(self.pairs):
            self._slot_table[8 * symbols.index(a) + symbols.index(b)] = p
        self._species32 = _element_indices(dyn)
        Cn, A = self._species32.shape
        dev = dyn.coordinates.device
        self._mode = "cell" if (Cn == 1 and A > 512) else "batch"
        self._engine = AevEngine(aev_constants_2x(len(symbols))._replace(Rcr=self.r_max, Rca=1e-3))
        self._params = _lib.MdParams(Cn, A, 0, 0, dyn.dt, 0, 0)
        shape = (Cn, len(self.pairs), self.bins) if self.per_entry else (len(self.pairs), self.bins)
        self._counts = torch.zeros(shape, dtype=torch.int64, device=dev)   # (the bits of the kernel's uint64 counters)
        self._status = torch.zeros(_lib.STATUS_WORDS, dtype=torch.int32, device=dev)
        self._volume_sum = torch.zeros(1, dtype=torch.float64, device=dev)
        # atoms of each element per entry, and of each pair's two elements
        per = torch.stack([(self._species32 == k).sum(dim=1) for k in range(len(symbols))], dim=1).double()   # [C, n_sym]
        ia = torch.tensor([symbols.index(a) for a, _ in self.pairs], device=dev)
        ib = torch.tensor([symbols.index(b) for _, b in self.pairs], device=dev)
        self._n_a, self._n_b = per[:, ia], per[:, ib]   # [C, P]
        self._full_pbc = dyn.cell is not None and dyn.pbc is not None and all(dyn.pbc)
        self._has_cell = dyn.cell is not None

    def _sample(self, dyn) -> None:
        from .engine import _stream

        rows = self._engine.neighbors(self._species32, dyn.coordinates, dyn.cell, dyn.pbc, mode=self._mode,
                                      row_cap=_lib.MAX_RAD)
        _lib.check(_lib.lib().anihip_md_rdf_accumulate(
            _stream(), C.byref(self._params), len(self.pairs), self.bins, self.r_max, int(self.per_entry), self._slot_table,
            self._species32.data_ptr(), rows.meta.data_ptr(), rows.ent.data_ptr(), rows.ent.shape[0],
            self._counts.data_ptr()))
        torch.bitwise_or(self._status, rows.status, out=self._status)
        if self._has_cell:
            self._volume_sum.add_(dyn.volumes())
        self.n_samples += 1

    def reset(self) -> None:
        super().reset()
        if self._counts is not None:
            self._counts.zero_()
            self._status.zero_()
            self._volume_sum.zero_()

    def raise_on_status(self) -> None:
        if self._counts is not None and int(self._status[0].item()) & (_lib.ST_ROW_OVERFLOW | _lib.ST_ENTRY_OVERFLOW):
            raise RuntimeError(f"RadialDistribution: an atom has more than {_lib.MAX_RAD} neighbors within r_max = {self.r_max} A, "
                               "more than a neighbor row holds, and its row was dropped from the counts: lower r_max")

    # ---- results -------------------------------------------------------------------------------------------------------
    def counts(self) -> Tensor:
        """uint64 [P, bins] or [C, P, bins]: the raw counters (a copy)."""
        self._need_attached()
        return self._counts.clone().view(torch.uint64)

    def edges(self) -> Tensor:
        """fp64 [bins + 1] (host): the bin edges in Angstrom."""
        return torch.arange(self.bins + 1, dtype=torch.float64) * (self.r_max / self.bins)

    def _atoms(self, n: Tensor) -> Tensor:
        """[C, P] counts to the shape of ``counts()`` without its last axis."""
        return n if self.per_entry else n.sum(dim=0)

    def coordination_numbers(self) -> Tensor:
        """fp64, the shape of ``counts()``: the mean number of neighbors of element b within the upper edge of each bin of
        a central atom of element a (NaN where there is no such atom or no sample)."""
        self._need_attached()
        return self._counts.double().cumsum(dim=-1) / (self.n_samples * self._atoms(self._n_a)).unsqueeze(-1)

    def g(self) -> Tensor:
        """fp64, the shape of ``counts()``: the radial distribution function of each pair at the bins."""
        self._need_attached()
        if not self._full_pbc:
            raise ValueError("g() needs a cell that is periodic in all three directions (the ideal-gas density it divides by); "
                             "coordination_numbers() works without one")
        edges = self.edges().to(self._counts.device)
        shell = 4.0 * math.pi / 3.0 * (edges[1:] ** 3 - edges[:-1] ** 3)
        pairs = self._atoms(self._n_a * self._n_b).unsqueeze(-1)
        return self._counts.double() * (self._volume_sum / max(self.n_samples, 1)) / (self.n_samples * pairs * shell)


def origins(n_samples: int, lags: int) -> Tensor:
    """int64 [lags] (host): the time origins n_l that lag l has after ``n_samples`` samples of a multiple-origin correlation,
    every sample k being paired with the samples k - l, l = 0 .. min(k, lags - 1): n_l = max(n_samples - l, 0)."""
    return (int(n_samples) - torch.arange(int(lags), dtype=torch.int64)).clamp(min=0)


class _Correlation(Observer):
    """Multiple time origins over a device ring of the last ``lags`` samples (anihip_md_corr_accumulate): the sum S [C, S, M]
    per entry, species and lag in fp64, the origins per lag on the host.  Padding atoms are dropped; ``species_values`` are the
    values of ``species`` behind the S columns (ascending), ``atom_counts`` [C, S] their atoms."""

    kind = _lib.MD_CORR_MSD
    bytes_per_value = 8

    def __init__(self, lags: int, every: int, max_bytes: int = 1 << 30) -> None:
        super().__init__(every)
        self.lags = _positive_int(lags, "lags")
        if self.lags > 65536:
            raise ValueError(f"lags must be at most 65536, got {lags}")
        self.max_bytes = int(max_bytes)
        self._sums = None

    def _tables(self, species: Tensor) -> tp.Tuple[Tensor, Tensor, Tensor, Tensor]:
        """(species_values [S], gather [C, G], gather_species [C, G], atom_counts [C, S]) of ``species`` [C, A] on the host."""
        sp = species.detach().cpu()
        values = torch.unique(sp[sp >= 0])
        if not 1 <= values.numel() <= _lib.MAX_SPECIES:
            raise ValueError(f"{type(self).__name__}: the batch must hold 1 .. {_lib.MAX_SPECIES} species, got {values.numel()}")
        index = torch.searchsorted(values, sp.clamp(min=int(values[0])))
        index = torch.where(sp >= 0, index, torch.full_like(index, values.numel()))   # (padding sorts last)
        order = torch.argsort(index, dim=1, stable=True)
        sorted_index = torch.gather(index, 1, order)
        G = max(int((sp >= 0).sum(dim=1).max()), 1)
        real = sorted_index[:, :G] < values.numel()
        gather = torch.where(real, order[:, :G], torch.full_like(order[:, :G], -1)).to(torch.int32)
        gather_species = torch.where(real, sorted_index[:, :G], torch.full_like(sorted_index[:, :G], -1)).to(torch.int32)
        counts = torch.stack([(index == k).sum(dim=1) for k in range(values.numel())], dim=1)
        return values, gather.contiguous(), gather_species.contiguous(), counts

    def ring_bytes(self, n_entries: int, max_atoms: int) -> int:
        return self.lags * n_entries * 3 * max_atoms * self.bytes_per_value

    def _check(self, dyn) -> None:
        from . import md

        name = type(self).__name__
        if isinstance(dyn, md.RingPolymerDynamics):
            raise ValueError(f"{name} is not available on RingPolymerDynamics: the beads are not trajectories (TimeSeries, "
                             "Trajectory and RadialDistribution are)")
        self._host_tables = self._tables(dyn.species)
        need = self.ring_bytes(dyn.species.shape[0], self._host_tables[1].shape[1])
        if need > self.max_bytes:
            raise ValueError(f"{name}: the ring of {self.lags} samples takes {need} bytes, more than max_bytes = {self.max_bytes}: "
                             "fewer lags (with a larger every for the same time span), or a larger max_bytes")

    def _allocate(self, dyn) -> None:
        dev = dyn.coordinates.device
        values, gather, gather_species, counts = self._host_tables
        Cn, A = dyn.species.shape
        self.species_values, self.atom_counts = values, counts.to(dev)
        self._gather, self._gather_species = gather.to(dev), gather_species.to(dev)
        self._G, self._S = gather.shape[1], values.numel()
        self._params = _lib.MdParams(Cn, A, 0, 0, dyn.dt, 0, 0)
        self._ring = torch.zeros(self.ring_bytes(Cn, self._G), dtype=torch.uint8, device=dev)
        self._sums = torch.zeros((Cn, self._S, self.lags), dtype=torch.float64, device=dev)
        self._workspace = torch.empty(_lib.lib().anihip_md_corr_workspace_bytes(Cn, self._G, self.lags, self._S),
                                      dtype=torch.uint8, device=dev)
        self._dt = dyn.dt

    def _input(self, dyn) -> tp.Tuple[Tensor, tp.Optional[Tensor]]:
        raise NotImplementedError

    def _sample(self, dyn) -> None:
        from .engine import _stream

        x, x_lo = self._input(dyn)
        _lib.check(_lib.lib().anihip_md_corr_accumulate(
            _stream(), C.byref(self._params), self.kind, self.lags, self._S, self._G, self.n_samples, self._gather.data_ptr(),
            self._gather_species.data_ptr(), x.data_ptr(), None if x_lo is None else x_lo.data_ptr(), self._ring.data_ptr(),
            self._sums.data_ptr(), self._workspace.data_ptr(), self._workspace.numel()))
        self.n_samples += 1

    def reset(self) -> None:
        super().reset()
        if self._sums is not None:
            self._sums.zero_()

    # ---- results -------------------------------------------------------------------------------------------------------
    def sums(self) -> Tensor:
        """fp64 [C, S, M]: the raw sums (a copy)."""
        self._need_attached()
        return self._sums.clone()

    def origins(self) -> Tensor:
        """int64 [M] (host): time origins per lag."""
        return origins(self.n_samples, self.lags)

    def times(self) -> Tensor:
        """fp64 [M] (host): l every dt, in fs."""
        return torch.arange(self.lags, dtype=torch.float64) * (self.every * self._need_attached().dt)

    def _normalized(self) -> Tensor:
        n_l = self.origins().to(self._sums.device).double()
        return self._sums / (n_l.view(1, 1, -1) * self.atom_counts.double().unsqueeze(-1))

    def total(self) -> Tensor:
        """fp64 [C, M]: all species together, each weighted by its atoms."""
        self._need_attached()
        n_l = self.origins().to(self._sums.device).double()
        return self._sums.sum(dim=1) / (n_l.view(1, -1) * self.atom_counts.double().sum(dim=1, keepdim=True))


class MeanSquaredDisplacement(_Correlation):
    """MSD(l) = <|x(k) - x(k - l)|^2> over atoms and time origins, from the fp64 positions ``coordinates + coordinates_lo``
    (kept unwrapped by the dynamics) sampled every ``every`` steps: ``msd()`` fp64 [C, S, lags] per entry and species, NaN at a
    lag without an origin.  Refused on a dynamics with a barostat, which rescales the unwrapped coordinates."""

    kind = _lib.MD_CORR_MSD
    bytes_per_value = 8

    def _check(self, dyn) -> None:
        if dyn.barostat:
            raise ValueError("MeanSquaredDisplacement is not available with a barostat: the unwrapped coordinates are rescaled "
                             "with the cell, so their differences are not displacements")
        super()._check(dyn)

    def _input(self, dyn):
        return dyn.coordinates, dyn.coordinates_lo

    def msd(self) -> Tensor:
        """fp64 [C, S, M], Angstrom^2."""
        self._need_attached()
        return self._normalized()

    def diffusion_coefficients(self, fit: tp.Tuple[int, int]) -> Tensor:
        """fp64 [C, S], Angstrom^2 / fs: the least-squares slope of the MSD against time over the lags fit[0] <= l < fit[1],
        divided by 6."""
        l0, l1 = int(fit[0]), int(fit[1])
        if not (0 <= l0 and l0 + 2 <= l1 <= self.lags):
            raise ValueError(f"fit must be a range of at least two lags within 0 .. {self.lags}, got {fit}")
        y = self.msd()[..., l0:l1]
        t = self.times()[l0:l1].to(y.device)
        tc = t - t.mean()
        return (y * tc).sum(dim=-1) / (tc * tc).sum() / 6.0


def cosine_spectrum(vacf: Tensor, dt: float, window: tp.Optional[str] = "hann") -> tp.Tuple[Tensor, Tensor]:
    """The cosine transform of a correlation function sampled at l dt, l = 0 .. L - 1 (last axis, fs):
    density_j = dt (w_0 C_0 + 2 sum_{l >= 1} w_l C_l cos(omega_j l dt)) at omega_j = pi j / (L dt), j = 0 .. L - 1, with the
    falling half of a Hann window w_l = (1 + cos(pi l / L)) / 2 (``window="hann"``) or none (None).  Returns (wavenumbers
    in 1 / cm [L], density [..., L]); torch only, on the device of ``vacf``."""
    if window not in ("hann", None):
        raise ValueError(f'window must be "hann" or None, got {window!r}')
    L = vacf.shape[-1]
    l = torch.arange(L, dtype=torch.float64, device=vacf.device)   # noqa: E741
    w = 0.5 * (1.0 + torch.cos(math.pi * l / L)) if window == "hann" else torch.ones_like(l)
    w = torch.where(l == 0, 0.5 * w, w) * 2.0 * dt
    kernel = torch.cos(math.pi * torch.outer(l, l) / L)   # [lag, frequency]
    density = (vacf.double() * w) @ kernel
    omega = math.pi * l / (L * dt)
    return omega / (2.0 * math.pi * LIGHT_SPEED_CM_PER_FS), density


class VelocityAutocorrelation(_Correlation):
    """VACF(l) = <v(k) . v(k - l)> over atoms and time origins from the fp32 velocities sampled every ``every`` steps
    (products and sums in fp64): ``vacf()`` fp64 [C, S, lags], (Angstrom / fs)^2, NaN at a lag without an origin."""

    kind = _lib.MD_CORR_VACF
    bytes_per_value = 4

    def _input(self, dyn):
        return dyn.velocities, None

    def vacf(self) -> Tensor:
        """fp64 [C, S, M]."""
        self._need_attached()
        return self._normalized()

    def spectrum(self, window: tp.Optional[str] = "hann") -> tp.Tuple[Tensor, Tensor]:
        """(wavenumbers in 1 / cm [L], density [C, S, L]): ``cosine_spectrum`` of the VACF over the L lags that have an
        origin -- the vibrational density of states up to a factor."""
        L = int((self.origins() > 0).sum())
        if L < 2:
            raise ValueError("spectrum() needs at least two lags with an origin")
        return cosine_spectrum(self.vacf()[..., :L], self.every * self._need_attached().dt, window)


# ---- heat flux -------------------------------------------------------------------------------------------------------------
def _check_flux(dyn, name: str) -> None:
    """What the heat-flux observers refuse (host only): everything whose forces carry a flux the model's flux stage does not
    compute, and models without that stage."""
    from . import md

    if isinstance(dyn, md.RingPolymerDynamics):
        raise ValueError(f"{name} is not available on RingPolymerDynamics: the beads are not trajectories, and their springs carry "
                         "a flux of their own")
    if dyn._clusters is not None:
        raise ValueError(f"{name} is not available with constraints: the constraint forces carry a heat flux that is not computed")
    if dyn._bias is not None:
        raise ValueError(f"{name} is not available with a bias: the bias forces carry a heat flux that is not computed")
    if dyn._model_eval.standalone or not hasattr(dyn.model, "heat_flux_terms"):
        raise ValueError(f"{name}: {type(dyn.model).__name__} is a pair potential, and the pair halves have no flux kernel yet")
    try:
        dyn.model._refuse_heat_flux()
    except NotImplementedError as err:
        raise ValueError(f"{name}: {err}") from None


def _flux_of(dyn) -> Tensor:
    """J [C, 3, 3] fp64 of the state the dynamics holds (coordinates and velocities of the same instant: after the kick).  One
    evaluation of the model's flux stage on the stream, no host read."""
    return dyn.model.heat_flux_terms(dyn.species, dyn.coordinates, dyn.velocities, dyn.masses, dyn.cell, dyn.pbc)[0]


class HeatFlux(_Ring):
    """A device ring of the heat flux J [capacity, C, 3, 3] (fp64, Hartree Angstrom / fs): per entry the kinetic convective
    term sum_i 1/2 m_i |v_i|^2 v_i, the potential convective term sum_i e_i v_i (e_i: the ensemble-mean network output, no self
    energies) and the virial term -sum_i sum_j d_ij (dE_i/d d_ij . v_j) -- ``grad.heat_flux`` has the definitions.  A sample
    evaluates the model's flux stage at the coordinates and velocities held, both after the kick: ONE EXTRA EVALUATION of the
    model per sample (neighbor rows, AEVs, networks forward and backward, the flux backward in place of the force backward),
    about the cost of a step; the step itself is untouched.  Works on open molecules and in cells.

    Refused at ``attach``: RingPolymerDynamics, constraints and a bias (their forces carry a flux that is not computed), and
    models with pair potentials."""

    def __init__(self, every: int, capacity: int, on_full: str = "raise") -> None:
        super().__init__(every, capacity, on_full)
        self._buf = None

    def _check(self, dyn) -> None:
        _check_flux(dyn, "HeatFlux")

    def _allocate(self, dyn) -> None:
        self._buf = torch.zeros((self.capacity, dyn.species.shape[0], 3, 3), dtype=torch.float64, device=dyn.coordinates.device)

    def _sample(self, dyn) -> None:
        k = self._slot(dyn)
        self._buf[k].copy_(_flux_of(dyn))

    def values(self) -> Tensor:
        """fp64 [n, C, 3, 3], oldest first: (kinetic, convective, virial) x (x, y, z)."""
        self._need_attached()
        return self._ordered(self._buf)

    def total(self) -> Tensor:
        """fp64 [n, C, 3]: J, the sum of the three terms."""
        return self.values().sum(dim=2)


class HeatFluxAutocorrelation(Observer):
    """<J(0) . J(t)> over multiple time origins, and the Green-Kubo thermal conductivity from it.  Every ``every`` steps the
    total heat flux J [C, 3] (see ``HeatFlux``: one extra evaluation of the model per sample) goes into a device ring of the
    last ``lags`` samples and its dot products with the ring are added to the sums [C, lags] (fp64): plain torch on the stream,
    the ring slot and the lags that exist come from the host-side sample count, nothing is read on the host.

    ``hfacf()`` [C, lags] is the average over the origins (``origins()``, NaN at a lag without one) in (Hartree Angstrom / fs)^2,
    ``thermal_conductivity()`` its running integral 1 / (3 V k_B T^2) int_0^t <J(0) . J(s)> ds in W / (m K).

    Refused at ``attach``: what ``HeatFlux`` refuses, a barostat (V and J's normalization move with the cell) and a cell that
    is not periodic in all three directions (no volume)."""

    def __init__(self, lags: int, every: int) -> None:
        super().__init__(every)
        self.lags = _positive_int(lags, "lags")
        self._ring = self._sums = None
        self._dt = None

    def _check(self, dyn) -> None:
        name = "HeatFluxAutocorrelation"
        _check_flux(dyn, name)
        if dyn.barostat:
            raise ValueError(f"{name} is not available with a barostat: the volume that normalizes the conductivity moves")
        if dyn.cell is None or dyn.pbc is None or not all(dyn.pbc):
            raise ValueError(f"{name} needs a cell that is periodic in all three directions: an open system has no volume to "
                             "normalize the conductivity by (HeatFlux records J without one)")

    def _allocate(self, dyn) -> None:
        self._init_buffers(dyn.species.shape[0], dyn.coordinates.device, dyn.dt)
        self._temp_sum = torch.zeros(dyn.species.shape[0], dtype=torch.float64, device=dyn.coordinates.device)

    def _init_buffers(self, n_entries: int, device, dt: float) -> None:
        self._ring = torch.zeros((self.lags, n_entries, 3), dtype=torch.float64, device=device)
        self._sums = torch.zeros((n_entries, self.lags), dtype=torch.float64, device=device)
        self._lag_index = torch.arange(self.lags, device=device)
        self._dt = float(dt)

    def _push(self, j: Tensor) -> None:
        """One sample J [C, 3] (fp64, on the device of the ring): ring slot k mod M, then S[c, l] += J . ring[(k - l) mod M] for
        the lags l = 0 .. min(k, M - 1) that exist, k the host-side sample count."""
        k, M = self.n_samples, self.lags
        cur = k % M
        self._ring[cur].copy_(j)
        n = min(k, M - 1) + 1
        slots = torch.remainder(cur - self._lag_index[:n], M)
        self._sums[:, :n] += (self._ring.index_select(0, slots) * self._ring[cur]).sum(dim=-1).t()
        self.n_samples += 1

    def _sample(self, dyn) -> None:
        self._temp_sum.add_(dyn.temperatures())
        self._push(_flux_of(dyn).sum(dim=1))

    def reset(self) -> None:
        super().reset()
        if self._sums is not None:
            self._sums.zero_()
            self._ring.zero_()
            if self._dyn is not None:
                self._temp_sum.zero_()

    # ---- results -------------------------------------------------------------------------------------------------------
    def _need_buffers(self) -> None:
        if self._sums is None:
            raise ValueError("attach the observer to a dynamics first: dyn.attach(observer)")

    def origins(self) -> Tensor:
        """int64 [M] (host): time origins per lag."""
        return origins(self.n_samples, self.lags)

    def times(self) -> Tensor:
        """fp64 [M] (host): l every dt, in fs."""
        self._need_buffers()
        return torch.arange(self.lags, dtype=torch.float64) * (self.every * self._dt)

    def hfacf(self) -> Tensor:
        """fp64 [C, M], (Hartree Angstrom / fs)^2: <J(0) . J(l every dt)>, NaN at a lag without an origin."""
        self._need_buffers()
        n_l = self.origins().to(self._sums.device).double()
        return torch.where(n_l > 0, self._sums / n_l.clamp(min=1.0), torch.full_like(self._sums, float("nan")))

    def mean_temperatures(self) -> Tensor:
        """fp64 [C], K: the mean of ``temperatures()`` over the samples."""
        self._need_attached()
        return self._temp_sum / max(self.n_samples, 1)

    def thermal_conductivity(self, temperature=None, volume=None) -> Tensor:
        """fp64 [C, M], W / (m K): kappa(t_l) = 1 / (3 V k_B T^2) int_0^{t_l} <J(0) . J(s)> ds by the trapezoid rule over the
        lags.  T: ``temperature`` (a number or [C]), else the thermostat's target, else -- NVE -- the mean kinetic temperature
        of the samples.  V: ``volume`` (Angstrom^3), else the cell's.  A running integral: read it where it has reached its
        plateau and before the noise of the tail takes over; NaN from the first lag without an origin on."""
        from .md import KB_HARTREE
        from .units import HARTREE_PER_ANGSTROM_FS_KELVIN_TO_WATT_PER_METER_KELVIN as TO_SI

        h = self.hfacf()
        dev = h.device
        if temperature is None:
            dyn = self._need_attached()
            temperature = dyn.temperature.double() if dyn.langevin else self.mean_temperatures()
        if volume is None:
            volume = self._need_attached().volumes()
        T = torch.as_tensor(temperature, dtype=torch.float64, device=dev).reshape(-1, 1)
        V = torch.as_tensor(volume, dtype=torch.float64, device=dev).reshape(-1, 1)
        integral = (torch.cumsum(h, dim=1) - 0.5 * (h[:, :1] + h)) * (self.every * self._dt)
        return integral * (TO_SI / (3.0 * KB_HARTREE)) / (V * T * T)
