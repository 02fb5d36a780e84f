"""The host side of biased MD (``md.BatchedDynamics(bias=...)``): collective variables, restraints on them, metadynamics, the
tables of ``anihip_md_bias`` (include/anihip.h has the exact definition) and the device state that csrc/md_bias.hip works on.
``torchani_amd.md`` re-exports the public names."""
from __future__ import annotations

import ctypes as C
import typing as tp

import torch
from torch import Tensor

from . import _lib

_CV_NAMES = {_lib.MD_CV_DISTANCE: "distance", _lib.MD_CV_ANGLE: "angle", _lib.MD_CV_DIHEDRAL: "dihedral"}
Index = tp.Union[int, Tensor]
Number = tp.Union[float, Tensor]


class CV(tp.NamedTuple):
    """A collective variable on atoms of one batch entry: ``kind`` (``_lib.MD_CV_*``) and one index per atom, each an int (the
    same atom in every entry) or an int64 [C] tensor (-1: this entry does not have this CV)."""
    kind: int
    atoms: tp.Tuple[Index, ...]


def _cv(kind: int, *atoms: Index) -> CV:
    for i in atoms:
        if isinstance(i, Tensor):
            if i.dtype != torch.int64 or i.dim() != 1:
                raise ValueError(f"a {_CV_NAMES[kind]} index must be an int or an int64 tensor of shape [C], got {i.dtype} "
                                 f"{tuple(i.shape)}")
        elif isinstance(i, bool) or not isinstance(i, int):
            raise ValueError(f"a {_CV_NAMES[kind]} index must be an int or an int64 tensor of shape [C], got {i!r}")
    return CV(kind, tuple(atoms))


def distance(i: Index, j: Index) -> CV:
    """s = |x_i - x_j| in Angstrom, the plain difference of the unwrapped coordinates (no minimum image)."""
    return _cv(_lib.MD_CV_DISTANCE, i, j)


def angle(i: Index, j: Index, k: Index) -> CV:
    """The angle i-j-k at j in [0, pi]."""
    return _cv(_lib.MD_CV_ANGLE, i, j, k)


def dihedral(i: Index, j: Index, k: Index, l: Index) -> CV:   # noqa: E741
    """The dihedral i-j-k-l in (-pi, pi], trans = pi."""
    return _cv(_lib.MD_CV_DIHEDRAL, i, j, k, l)


class Restraint:
    """A flat-bottom harmonic restraint on ``cv``: with d = s - center (wrapped into [-pi, pi) for a dihedral) and
    e = max(0, |d| - half_width), E = k e^2 / 2.  ``center``, ``k`` (Hartree / Angstrom^2 or Hartree / rad^2, >= 0, 0 switches
    it off) and ``half_width`` are numbers or [C] tensors: per-entry centres are umbrella windows across the batch."""

    def __init__(self, cv: CV, center: Number, k: Number, half_width: Number = 0.0) -> None:
        if not isinstance(cv, CV):
            raise ValueError("Restraint needs a CV: md.distance, md.angle or md.dihedral")
        self.cv, self.center, self.k, self.half_width = cv, center, k, half_width


class Metadynamics:
    """Metadynamics on one or two CVs per entry.  ``sigma``: the Gaussian width of each CV, a number (every CV), or one number
    or [C] tensor per CV; ``height`` in Hartree, a number or [C]; ``pace`` in steps, 0 never deposits (a static bias from
    ``hills``); ``bias_factor`` gamma > 1 is well-tempered metadynamics (needs Langevin dynamics), None plain.  ``walkers``:
    None gives every entry a hill list of its own; int64 [C] makes the entries with the same id share one list (multiple
    walkers), -1 leaves an entry without metadynamics.  Lists are numbered in ascending order of the ids.  ``max_hills``: the
    capacity of every list; ``hills``: (centers [G, n_cv, H], heights [G, H]) or (centers, heights, used [G]) to start from,
    what ``BatchedDynamics.hills()`` returned."""

    def __init__(self, cvs, sigma, height: Number, pace: int, bias_factor: tp.Optional[float] = None,
                 walkers: tp.Optional[Tensor] = None, max_hills: int = 4096, hills=None) -> None:
        cvs = (cvs,) if isinstance(cvs, CV) else tuple(cvs)
        if not all(isinstance(cv, CV) for cv in cvs):
            raise ValueError("Metadynamics needs CVs: md.distance, md.angle or md.dihedral")
        if not 1 <= len(cvs) <= 2:
            raise ValueError(f"Metadynamics takes one or two CVs, got {len(cvs)}")
        if isinstance(sigma, (int, float)) or (isinstance(sigma, Tensor) and len(cvs) == 1):
            sigma = (sigma,) * len(cvs)
        sigma = tuple(sigma)
        if len(sigma) != len(cvs):
            raise ValueError(f"sigma must be a number or one value per CV ({len(cvs)}), got {len(sigma)}")
        if isinstance(pace, bool) or int(pace) != pace or pace < 0:
            raise ValueError(f"pace must be an integer >= 0, got {pace}")
        if bias_factor is not None and not bias_factor > 1:
            raise ValueError(f"bias_factor must be > 1 (None: plain metadynamics), got {bias_factor}")
        if isinstance(max_hills, bool) or int(max_hills) != max_hills or not 1 <= max_hills <= 1 << 30:
            raise ValueError(f"max_hills must be an integer in 1 .. 2^30, got {max_hills}")
        self.cvs, self.sigma, self.height, self.pace = cvs, sigma, height, int(pace)
        self.bias_factor, self.walkers, self.max_hills, self.hills = bias_factor, walkers, int(max_hills), hills


class BiasTables(tp.NamedTuple):
    """The tables of anihip_md_bias (include/anihip.h) on the host, and what the class derives from them."""
    cv_offset: Tensor      # int32 [C + 1]
    kind: Tensor           # int32 [Ncv]
    atoms: Tensor          # int32 [Ncv, 4]: global atom index c A + i, -1 in the unused slots
    restraint: Tensor      # fp64 [Ncv, 3]: center, k, half_width
    meta_cv: Tensor        # int32 [C, 2]: positions of the metadynamics CVs within the entry's CVs, -1
    inv_sigma2: Tensor     # fp64 [C, 2]
    height: Tensor         # fp64 [C]
    list: Tensor           # int32 [C]: -1 without metadynamics
    rank_in_list: Tensor   # int32 [C]
    members: Tensor        # int32 [G]
    list_entry: Tensor     # int32 [G]: the first member
    bias_factor: Tensor    # fp64 [G]: 0 for plain metadynamics
    used: Tensor           # int32 [G]: hills to start from
    centers: Tensor        # fp64 [G, 2, H]
    heights: Tensor        # fp64 [G, H]
    capacity: int
    pace: int
    cv_index: Tensor       # int64 [C, R]: the row of column r (a restraint, or a metadynamics CV without one) in the CSR arrays, -1


def _per_entry(value, name: str, n: int) -> Tensor:
    # (a Python float must not pass through fp32)
    t = value.detach().cpu().to(torch.float64) if isinstance(value, Tensor) else torch.as_tensor(value, dtype=torch.float64)
    if t.dim() == 0:
        t = t.expand(n)
    if tuple(t.shape) != (n,):
        raise ValueError(f"{name} must be a number or a tensor of shape ({n},), got {tuple(t.shape)}")
    return t


def build_bias_tables(species: Tensor, fixed: tp.Optional[Tensor], bias, temperature=None) -> BiasTables:
    """Validate ``bias`` (a sequence of ``Restraint`` and at most one ``Metadynamics``) for a batch of ``species`` [C, A] and
    lay out the tables of include/anihip.h.  Pure host torch; reads no device.  ``fixed`` is accepted for symmetry with the
    constraint builder: a CV may sit on a fixed atom (an anchor), whose force the integrator ignores.  ``temperature``: what
    the dynamics was given, None for NVE, which a ``bias_factor`` refuses.

    The CVs of an entry are ordered as the restraints were given, then the metadynamics CVs that no restraint holds (a
    ``Metadynamics`` CV that is the very object of a ``Restraint`` shares its row).  Raises ValueError for an index outside
    -1 .. A - 1, a CV on a padding atom, a repeated atom, more than 16 CVs in an entry, k or
    half_width < 0, sigma <= 0, height < 0, a walker without its CVs, sigmas that differ within a list, ``bias_factor`` without
    a temperature, and ``hills`` of the wrong shape or beyond ``max_hills``."""
    species = species.detach().cpu()
    if species.dim() != 2:
        raise ValueError("expected species [C, A]")
    Cn, A = species.shape
    if fixed is not None and tuple(fixed.shape) != (Cn, A):
        raise ValueError(f"fixed must be a bool mask of shape {(Cn, A)}, got {tuple(fixed.shape)}")
    if isinstance(bias, (Restraint, Metadynamics)):
        bias = (bias,)
    bias = tuple(bias)
    metas = [b for b in bias if isinstance(b, Metadynamics)]
    rows: tp.List[tp.Tuple[CV, Tensor, Tensor, Tensor]] = []
    zeros = torch.zeros(Cn, dtype=torch.float64)
    for b in bias:
        if isinstance(b, Restraint):
            rows.append((b.cv, _per_entry(b.center, "center", Cn), _per_entry(b.k, "k", Cn),
                         _per_entry(b.half_width, "half_width", Cn)))
        elif not isinstance(b, Metadynamics):
            raise ValueError(f"bias takes Restraint and Metadynamics objects, got {type(b).__name__}")
    if len(metas) > 1:
        raise ValueError(f"at most one Metadynamics per dynamics, got {len(metas)}")
    meta = metas[0] if metas else None
    meta_rows: tp.List[int] = []
    if meta is not None:
        for cv in meta.cvs:
            held = [r for r, row in enumerate(rows) if row[0] is cv]
            if held:
                meta_rows.append(held[0])
            else:
                meta_rows.append(len(rows))
                rows.append((cv, zeros, zeros, zeros))
        if len(set(meta_rows)) != len(meta_rows):
            raise ValueError("Metadynamics was given the same CV twice")
    R = len(rows)
    real = species >= 0
    entry = torch.arange(Cn)
    present = torch.zeros((Cn, R), dtype=torch.bool)
    idx_all = torch.full((Cn, R, 4), -1, dtype=torch.int64)
    for r, (cv, center, k, hw) in enumerate(rows):
        name, n = _CV_NAMES[cv.kind], len(cv.atoms)
        cols = []
        for i in cv.atoms:
            if isinstance(i, Tensor):
                if tuple(i.shape) != (Cn,):
                    raise ValueError(f"{name}: an index tensor must have shape ({Cn},), got {tuple(i.shape)}")
                cols.append(i.detach().cpu())
            else:
                if not 0 <= i < A:
                    raise ValueError(f"{name}: atom index {i} is outside 0 .. {A - 1}")
                cols.append(torch.full((Cn,), i, dtype=torch.int64))
        idx = torch.stack(cols, dim=1)

        def where(bad: Tensor) -> str:
            c = int(bad.nonzero()[0])
            return f"entry {c}, {name} of atoms {tuple(idx[c].tolist())}"

        bad = ((idx < -1) | (idx >= A)).any(dim=1)
        if bool(bad.any()):
            raise ValueError(f"a CV needs atom indices in 0 .. {A - 1}, or -1 in an index tensor for an entry without it: {where(bad)}")
        absent = (idx == -1).any(dim=1)   # (-1 in any index tensor: the entry does not have this CV)
        here = ~absent
        bad = here & ~real[entry.view(-1, 1), idx.clamp(min=0)].all(dim=1)
        if bool(bad.any()):
            raise ValueError(f"CV on a padding atom: {where(bad)}")
        rep = torch.zeros(Cn, dtype=torch.bool)
        for a in range(n):
            for b2 in range(a):
                rep |= idx[:, a] == idx[:, b2]
        bad = here & rep
        if bool(bad.any()):
            raise ValueError(f"a CV needs {n} different atoms: {where(bad)}")
        for t, what in ((k, "k"), (hw, "half_width")):
            bad = here & ~(torch.isfinite(t) & (t >= 0))
            if bool(bad.any()):
                raise ValueError(f"{what} must be >= 0: {where(bad)} has {float(t[int(bad.nonzero()[0])]):g}")
        bad = here & ~torch.isfinite(center)
        if bool(bad.any()):
            raise ValueError(f"center must be finite: {where(bad)}")
        present[:, r] = here
        idx_all[:, r, :n] = idx
    count = present.sum(dim=1)
    if bool((count > _lib.MD_BIAS_MAX_CVS).any()):
        c = int((count > _lib.MD_BIAS_MAX_CVS).nonzero()[0])
        raise ValueError(f"entry {c} has {int(count[c])} CVs, more than {_lib.MD_BIAS_MAX_CVS}")
    cv_offset = torch.zeros(Cn + 1, dtype=torch.int64)
    cv_offset[1:] = torch.cumsum(count, 0)
    ce, re = present.nonzero(as_tuple=True)   # (sorted by entry, then by row: the CSR order)
    ncv = ce.numel()
    cv_index = torch.full((Cn, R), -1, dtype=torch.int64)
    cv_index[ce, re] = torch.arange(ncv)
    kinds = torch.tensor([row[0].kind for row in rows], dtype=torch.int32)
    kind = kinds[re] if ncv else torch.zeros(0, dtype=torch.int32)
    atoms = idx_all[ce, re]
    atoms = torch.where(atoms >= 0, atoms + (ce * A).view(-1, 1), atoms).to(torch.int32)
    if R:
        per_row = torch.stack([torch.stack([row[1], row[2], row[3]], dim=1) for row in rows], dim=1)   # [C, R, 3]
        restraint = per_row[ce, re].contiguous()
    else:
        restraint = torch.zeros((0, 3), dtype=torch.float64)

    # ---- metadynamics ----
    meta_cv = torch.full((Cn, 2), -1, dtype=torch.int32)
    inv_sigma2 = torch.zeros((Cn, 2), dtype=torch.float64)
    height = torch.zeros(Cn, dtype=torch.float64)
    lst = torch.full((Cn,), -1, dtype=torch.int32)
    rank = torch.zeros(Cn, dtype=torch.int32)
    G, capacity, pace = 0, 0, 0
    gamma = 0.0
    has = torch.zeros(Cn, dtype=torch.bool)
    if meta is not None:
        nd = len(meta_rows)
        have = present[:, meta_rows]
        if meta.walkers is None:
            walkers = torch.arange(Cn)
            has = have.all(dim=1)
            bad = have.any(dim=1) & ~has
            if bool(bad.any()):
                raise ValueError(f"entry {int(bad.nonzero()[0])} has one of the two metadynamics CVs and not the other")
        else:
            walkers = torch.as_tensor(meta.walkers).detach().cpu()
            if walkers.dtype != torch.int64 or tuple(walkers.shape) != (Cn,):
                raise ValueError(f"walkers must be an int64 tensor of shape ({Cn},)")
            if bool((walkers < -1).any()):
                raise ValueError("walkers must hold list ids >= 0, or -1 for an entry without metadynamics")
            has = walkers >= 0
            bad = has & ~have.all(dim=1)
            if bool(bad.any()):
                c = int(bad.nonzero()[0])
                raise ValueError(f"entry {c} is a walker of list {int(walkers[c])} but does not have every metadynamics CV")
        if meta.bias_factor is not None:
            if temperature is None:
                raise ValueError("bias_factor (well-tempered metadynamics) needs a temperature: Langevin dynamics, not NVE")
            gamma = float(meta.bias_factor)
        sig = torch.stack([_per_entry(s, "sigma", Cn) for s in meta.sigma], dim=1)
        bad = has & ~(torch.isfinite(sig) & (sig > 0)).all(dim=1)
        if bool(bad.any()):
            raise ValueError(f"sigma must be > 0: entry {int(bad.nonzero()[0])}")
        h = _per_entry(meta.height, "height", Cn)
        bad = has & ~(torch.isfinite(h) & (h >= 0))
        if bool(bad.any()):
            raise ValueError(f"height must be >= 0: entry {int(bad.nonzero()[0])}")
        capacity, pace = meta.max_hills, meta.pace
        members_of = has.nonzero().view(-1)
        if members_of.numel():
            ids, g_of = torch.unique(walkers[members_of], return_inverse=True)
            G = ids.numel()
            size = torch.bincount(g_of, minlength=G)
            start = torch.cumsum(size, 0) - size
            order = torch.argsort(g_of, stable=True)   # (members_of ascends: batch order within a list)
            rk = torch.empty_like(g_of)
            rk[order] = torch.arange(g_of.numel()) - start[g_of[order]]
            lst[members_of], rank[members_of] = g_of.to(torch.int32), rk.to(torch.int32)
            first = members_of[order][start]
            for d in range(nd):
                meta_cv[members_of, d] = (cv_index[members_of, meta_rows[d]] - cv_offset[members_of]).to(torch.int32)
            inv_sigma2[members_of, :nd] = 1.0 / sig[members_of] ** 2
            height[members_of] = h[members_of]
            bad = (sig[members_of] != sig[first[g_of]]).any(dim=1)
            if bool(bad.any()):
                c = int(members_of[int(bad.nonzero()[0])])
                raise ValueError(f"the walkers of a list must agree in sigma (and in the kinds of their CVs): entry {c} differs "
                                 f"from entry {int(first[int(lst[c])])} of list {int(lst[c])}")
    members = torch.zeros(G, dtype=torch.int32)
    list_entry = torch.zeros(G, dtype=torch.int32)
    if G:
        members, list_entry = size.to(torch.int32), first.to(torch.int32)
    used = torch.zeros(G, dtype=torch.int32)
    centers, heights = torch.zeros((G, 2, 0), dtype=torch.float64), torch.zeros((G, 0), dtype=torch.float64)
    if meta is not None and meta.hills is not None:
        hl = tuple(meta.hills)
        if len(hl) not in (2, 3):
            raise ValueError("hills must be (centers, heights) or (centers, heights, used)")
        c0 = torch.as_tensor(hl[0]).detach().cpu().to(torch.float64)
        h0 = torch.as_tensor(hl[1]).detach().cpu().to(torch.float64)
        nd = len(meta_rows)
        if c0.dim() != 3 or c0.shape[0] != G or c0.shape[1] not in (nd, 2) or tuple(h0.shape) != (G, c0.shape[2]):
            raise ValueError(f"hills must be centers [{G}, {nd}, H] and heights [{G}, H], got {tuple(c0.shape)} and "
                             f"{tuple(h0.shape)}")
        H = c0.shape[2]
        if H > capacity:
            raise ValueError(f"hills holds {H} hills per list, more than max_hills = {capacity}")
        u0 = torch.full((G,), H, dtype=torch.int64) if len(hl) == 2 else torch.as_tensor(hl[2]).detach().cpu().to(torch.int64)
        if tuple(u0.shape) != (G,) or bool(((u0 < 0) | (u0 > H)).any()):
            raise ValueError(f"the used counts of hills must be {G} integers in 0 .. {H}")
        centers = torch.zeros((G, 2, H), dtype=torch.float64)
        centers[:, :c0.shape[1]] = c0
        heights, used = h0.contiguous(), u0.to(torch.int32)
    return BiasTables(cv_offset.to(torch.int32), kind, atoms.contiguous(), restraint, meta_cv, inv_sigma2, height, lst, rank,
                      members, list_entry, torch.full((G,), gamma, dtype=torch.float64), used, centers, heights, int(capacity),
                      int(pace), cv_index)


class DeviceBias:
    """The tables on the device, the hill lists and the outputs of anihip_md_bias_apply.  The host keeps every hill count
    (preloaded + deposits x members), so no call here reads the device."""

    def __init__(self, tables: BiasTables, n_mol: int, atoms_per_mol: int, device: torch.device) -> None:
        t = tables
        self.tables, self.n_lists, self.capacity, self.pace = t, int(t.members.numel()), t.capacity, t.pace
        dev = lambda x: x.to(device).contiguous()   # noqa: E731
        self._held = [dev(x) for x in (t.cv_offset, t.kind, t.atoms, t.restraint, t.meta_cv, t.inv_sigma2, t.height, t.list,
                                       t.rank_in_list, t.members, t.list_entry, t.bias_factor)]
        G, cap = self.n_lists, (t.capacity if self.n_lists else 0)
        self.used = dev(t.used)
        self.dropped = torch.zeros(G, dtype=torch.int32, device=device)
        self.centers = torch.zeros((G, 2, cap), dtype=torch.float64, device=device)
        self.heights = torch.zeros((G, cap), dtype=torch.float64, device=device)
        n0 = t.heights.shape[1]
        if G and n0:
            self.centers[:, :, :n0], self.heights[:, :n0] = dev(t.centers), dev(t.heights)
        self.status = torch.zeros(n_mol, dtype=torch.int32, device=device)
        self.cv_values = torch.zeros(max(1, t.kind.numel()), dtype=torch.float64, device=device)
        self.bias_energies = torch.zeros(n_mol, dtype=torch.float64, device=device)
        self.meta_energies = torch.zeros(n_mol, dtype=torch.float64, device=device)
        self.cv_index = dev(t.cv_index)
        self.counts = [int(u) for u in t.used.tolist()]
        self.members = [int(m) for m in t.members.tolist()]
        self.gamma = float(t.bias_factor[0]) if G else 0.0
        ptr = [x.data_ptr() if x.numel() else None for x in self._held]
        self.struct = _lib.MdBias(int(t.kind.numel()), G, cap, 0, 0, n_mol, *ptr,
                                  *(x.data_ptr() if x.numel() else None
                                    for x in (self.used, self.dropped, self.centers, self.heights)), self.status.data_ptr())
        self.params = _lib.MdParams(n_mol, atoms_per_mol, 0, 0, 1.0, 0, 0)
        nbytes = _lib.lib().anihip_md_bias_workspace_bytes(C.byref(self.params), C.byref(self.struct))
        self.workspace = torch.empty(max(1, nbytes), dtype=torch.uint8, device=device)

    def apply(self, coordinates: Tensor, coordinates_lo: Tensor, forces: Tensor) -> None:
        """anihip_md_bias_apply: the bias force added to ``forces`` in place; energies and CV values kept here."""
        from .engine import _stream

        self.struct.hills_bound = max([1] + self.counts) if self.n_lists else 0
        _lib.check(_lib.lib().anihip_md_bias_apply(
            _stream(), C.byref(self.params), C.byref(self.struct), coordinates.data_ptr(), coordinates_lo.data_ptr(),
            forces.data_ptr(), self.bias_energies.data_ptr(), self.meta_energies.data_ptr(), self.cv_values.data_ptr(),
            self.workspace.data_ptr(), self.workspace.numel()))

    def deposit(self, kT: tp.Optional[Tensor]) -> None:
        """anihip_md_bias_deposit on the CV values and energies of the last ``apply``; raises before a round that would not
        fit (the host knows the counts)."""
        from .engine import _stream

        for g, (n, m) in enumerate(zip(self.counts, self.members)):
            if n + m > self.capacity:
                raise RuntimeError(f"metadynamics list {g} holds {n} hills and its {m} walkers would deposit past max_hills = "
                                   f"{self.capacity}: construct Metadynamics with a larger max_hills (hills= restarts from hills())")
        _lib.check(_lib.lib().anihip_md_bias_deposit(
            _stream(), C.byref(self.params), C.byref(self.struct), None if kT is None else kT.data_ptr(),
            self.cv_values.data_ptr(), self.meta_energies.data_ptr()))
        self.counts = [n + m for n, m in zip(self.counts, self.members)]

    def hills_at(self, values: Tensor, list: int) -> tp.Tuple[Tensor, Tensor]:   # noqa: A002
        """anihip_md_bias_hills: V [n] and dV/ds [n, 2] of one list at ``values`` [n] or [n, n_cv]."""
        from .engine import _stream

        if isinstance(list, bool) or int(list) != list or not 0 <= list < self.n_lists:
            raise ValueError(f"list must be an integer in 0 .. {self.n_lists - 1}, got {list}")
        v = values.to(device=self.used.device, dtype=torch.float64)
        if v.dim() == 1:
            v = v.unsqueeze(1)
        if v.dim() != 2 or v.shape[1] not in (1, 2):
            raise ValueError(f"values must have shape [n] or [n, n_cv], got {tuple(values.shape)}")
        pts = torch.zeros((v.shape[0], 2), dtype=torch.float64, device=v.device)
        pts[:, :v.shape[1]] = v
        out_v = torch.empty(v.shape[0], dtype=torch.float64, device=v.device)
        out_d = torch.empty((v.shape[0], 2), dtype=torch.float64, device=v.device)
        _lib.check(_lib.lib().anihip_md_bias_hills(_stream(), C.byref(self.struct), int(list), v.shape[0], pts.data_ptr(),
                                                   out_v.data_ptr(), out_d.data_ptr()))
        return out_v, out_d
