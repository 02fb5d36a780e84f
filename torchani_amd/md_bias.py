"""The host side of biased MD (``md.BatchedDynamics(bias=...)``): collective variables, restraints on them, metadynamics, the
tables of ``anihip_md_bias`` (include/anihip.h has the exact definition) and the device state that csrc/md_bias.hip works on.
``torchani_amd.md`` re-exports the public names."""
from __future__ import annotations

import copy
import ctypes as C
import math
import typing as tp

import torch
from torch import Tensor

from . import _lib

_CV_NAMES = {_lib.MD_CV_DISTANCE: "distance", _lib.MD_CV_ANGLE: "angle", _lib.MD_CV_DIHEDRAL: "dihedral"}
Number = tp.Union[float, Tensor]
Group = tp.Union[tp.Sequence[int], Tensor]


class Coordination(tp.NamedTuple):
    """What ``coordination`` was given: the two groups and the switching function."""
    group_a: Group
    group_b: Group
    r0: float
    d0: float
    n: int
    r_max: tp.Optional[float]


class Site:
    """A pseudo-atom that stands for a group of atoms wherever ``distance``, ``angle`` and ``dihedral`` take an atom index:
    ``center`` makes one.  (The two sites that carry a coordination number, of kinds "value" and "anchor", are internal to
    ``coordination``.)  The same object named twice is the same site."""
    __slots__ = ("kind", "atoms", "weights", "coordination")

    def __init__(self, kind: str, atoms: tp.Optional[Group] = None, weights: tp.Optional[str] = None,
                 coordination: tp.Optional[Coordination] = None) -> None:
        self.kind, self.atoms, self.weights, self.coordination = kind, atoms, weights, coordination


Index = tp.Union[int, Tensor, Site]


class CV(tp.NamedTuple):
    """A collective variable on atoms of one batch entry: ``kind`` (``_lib.MD_CV_*``) and one index per atom, each an int (the
    same atom in every entry), an int64 [C] tensor (-1: this entry does not have this CV) or a ``Site``."""
    kind: int
    atoms: tp.Tuple[Index, ...]


def _cv(kind: int, *atoms: Index) -> CV:
    for i in atoms:
        if isinstance(i, Site):
            continue
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


def _group(atoms, what: str) -> Group:
    """A group as it is kept: a tuple of distinct ints in ascending order, or a bool mask of one or two dimensions."""
    if isinstance(atoms, Tensor):
        if atoms.dtype != torch.bool or atoms.dim() not in (1, 2):
            raise ValueError(f"{what}: a group is a sequence of atom indices or a bool mask [A] or [C, A], got {atoms.dtype} "
                             f"{tuple(atoms.shape)}")
        return atoms.detach().cpu()
    atoms = tuple(atoms)
    if any(isinstance(i, bool) or not isinstance(i, int) for i in atoms):
        raise ValueError(f"{what}: a group is a sequence of atom indices (ints) or a bool mask [A] or [C, A], got {atoms!r}")
    if len(set(atoms)) != len(atoms):
        raise ValueError(f"{what}: a group names every atom once, got {atoms!r}")
    return tuple(sorted(atoms))


def center(atoms: Group, weights: tp.Optional[str] = "mass") -> Site:
    """The centre of a group of atoms as a site: x = sum_i w_i x_i over the plain unwrapped coordinates (no minimum image),
    w_i = m_i / sum m for ``weights="mass"`` (the masses of the dynamics) or 1 / n for None.  ``atoms``: a sequence of ints (the
    same atoms in every entry) or a bool mask [A] or [C, A]; an entry whose row is empty has no such site, and no CV on it."""
    if weights not in ("mass", None):
        raise ValueError(f'weights must be "mass" or None, got {weights!r}')
    return Site("center", _group(atoms, "center"), weights)


def coordination(group_a: Group, group_b: Group, r0: float, d0: float = 0.0, n: int = 6, r_max: tp.Optional[float] = None) -> CV:
    """s = sum_{i in A} sum_{j in B, j != i} sw(r_ij) with x = max(r - d0, 0) / r0 and sw = 1 / (1 + x^n), shifted and scaled
    to reach 0 at ``r_max`` and cut there (None: no cut; a periodic cell needs one, at most half its smallest perpendicular
    width).  Distances take the minimum image when the dynamics has a periodic cell.  The groups are given as for ``center``
    and may overlap; an entry in which either is empty does not have the CV.  include/anihip.h has the exact definition."""
    for x, name in ((r0, "r0"), (d0, "d0"), (r_max, "r_max")):
        if not (x is None and name == "r_max") and (isinstance(x, bool) or not isinstance(x, (int, float))):
            raise ValueError(f"coordination: {name} must be a number, got {x!r}")
    if isinstance(n, bool) or not isinstance(n, int):
        raise ValueError(f"coordination: n must be an integer, got {n!r}")
    co = Coordination(_group(group_a, "coordination"), _group(group_b, "coordination"), float(r0), float(d0), n,
                      None if r_max is None or r_max == math.inf else float(r_max))
    # the distance between a site at (s, 0, 0) and one at the origin: the kernels of the atom CVs carry it unchanged
    return CV(_lib.MD_CV_DISTANCE, (Site("value", coordination=co), Site("anchor", coordination=co)))


def has_sites(cv: CV) -> bool:
    return any(isinstance(i, Site) for i in cv.atoms)


class Restraint:
    """A flat-bottom harmonic restraint on ``cv``: with d = s - center (wrapped into [-pi, pi) for a dihedral) and
    e = max(0, |d| - half_width), E = k e^2 / 2.  ``center``, ``k`` (Hartree / Angstrom^2 or Hartree / rad^2, >= 0, 0 switches
    it off) and ``half_width`` are numbers or [C] tensors: per-entry centres are umbrella windows across the batch."""

    def __init__(self, cv: CV, center: Number, k: Number, half_width: Number = 0.0) -> None:
        if not isinstance(cv, CV):
            raise ValueError("Restraint needs a CV: md.distance, md.angle, md.dihedral or md.coordination")
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
            raise ValueError("Metadynamics needs CVs: md.distance, md.angle, md.dihedral or md.coordination")
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


class SiteTables(tp.NamedTuple):
    """The tables of anihip_md_sites (include/anihip.h) on the host."""
    max_sites: int         # V: an extended entry has A + V atoms
    site_kind: Tensor      # int32 [C, V]: _lib.MD_SITE_*
    site_ref: Tensor       # int32 [C, V]: the group of a centre, the coordination row of an anchor or a value site
    group_offset: Tensor   # int32 [Ng + 1]
    group_atoms: Tensor    # int32 [Nga]: global atom index c A + i, ascending within a group
    group_weights: Tensor  # fp64 [Nga]
    coord: Tensor          # int32 [Nq, 5]: entry, group A, group B, slot of the value site, n
    coord_params: Tensor   # fp64 [Nq, 4]: r0, d0, r_max (inf: none), b = base(r_max)
    member_offset: Tensor  # int32 [C A + 1]
    member_site: Tensor    # int32 [Nm, 2]: slot, _lib.MD_SITE_ROLE_*
    member_weight: Tensor  # fp64 [Nm]
    pbc: tp.Tuple[int, int, int]
    cell: tp.Tuple[float, ...]       # 9, row-major (zeros without a periodic direction)
    inv_cell: tp.Tuple[float, ...]
    species_ext: Tensor    # int64 [C, A + V]: species, then 0 for a site the entry has and -1 for one it lacks


def switch_base(r: float, r0: float, d0: float, n: int) -> float:
    """1 / (1 + x^n), x = max(r - d0, 0) / r0, x^n by repeated multiplication as the kernels form it."""
    x = max(r - d0, 0.0) / r0
    p = x
    for _ in range(2, n):
        p *= x
    return 1.0 / (1.0 + p * x)


def _group_rows(group: Group, Cn: int, A: int, real: Tensor, what: str) -> tp.List[Tensor]:
    """The atoms of ``group`` in every entry, ascending."""
    if isinstance(group, Tensor):
        if tuple(group.shape) not in ((A,), (Cn, A)):
            raise ValueError(f"{what}: a group mask must have shape ({A},) or ({Cn}, {A}), got {tuple(group.shape)}")
        mask = group.expand(Cn, A)
        rows = [mask[c].nonzero().view(-1) for c in range(Cn)]
    else:
        for i in group:
            if not 0 <= i < A:
                raise ValueError(f"{what}: entry 0, atom index {i} of a group is outside 0 .. {A - 1}")
        rows = [torch.tensor(group, dtype=torch.int64)] * Cn
    for c, row in enumerate(rows):
        if row.numel() and not bool(real[c, row].all()):
            i = int(row[(~real[c, row]).nonzero()[0]])
            raise ValueError(f"{what}: group on a padding atom: entry {c}, atom {i}")
    return rows


def build_site_tables(species: Tensor, fixed: tp.Optional[Tensor], bias, temperature=None, masses=None, cell=None,
                      pbc=None) -> tp.Tuple[tp.Optional[SiteTables], BiasTables]:
    """``build_bias_tables`` for a bias whose CVs may hold sites (``center``) and coordination numbers (``coordination``).
    Every site an entry has becomes atom A + v of its extended entry of A + V atoms, v counting the entry's sites in the order
    in which the bias first names them (a coordination number takes two slots, anchor then value) and V the largest count
    of any entry; the CVs are then resolved to these indices and handed to the unchanged ``build_bias_tables`` with the species
    extended accordingly, whose messages and limits apply.  Returns (site tables, bias tables); the first is None for a bias
    without sites, the second then what ``build_bias_tables`` gives for ``species``.

    ``masses``: fp32 [C, A] or a function that returns them, needed (and called) only for mass-weighted centres.  ``cell`` and
    ``pbc``: the constant cell of the dynamics, for the minimum image of coordination numbers.  Raises ValueError, naming the
    entry, for a group on a padding atom, an index out of range, more than 64 sites in an entry, r0 <= 0, d0 < 0, n outside
    2 .. 32, r_max <= d0, a periodic cell without r_max, an r_max beyond half the smallest perpendicular width of the cell, a
    centre of zero total mass and a mask of the wrong shape."""
    species = species.detach().cpu()
    if species.dim() != 2:
        raise ValueError("expected species [C, A]")
    Cn, A = species.shape
    items = (bias,) if isinstance(bias, (Restraint, Metadynamics)) else tuple(bias)
    cvs: tp.List[CV] = []
    for b in items:
        cvs += [b.cv] if isinstance(b, Restraint) else list(b.cvs) if isinstance(b, Metadynamics) else []
    if not any(has_sites(cv) for cv in cvs):
        return None, build_bias_tables(species, fixed, items, temperature)
    real = species >= 0
    # units in the order in which the bias first names them: a centre (one slot) or a coordination number (anchor, value)
    units: tp.List[tp.Union[Site, Coordination]] = []
    for cv in cvs:
        name = _CV_NAMES[cv.kind]
        for i in cv.atoms:
            if isinstance(i, Site):
                unit = i if i.kind == "center" else i.coordination
                if not any(u is unit for u in units):
                    units.append(unit)
            elif isinstance(i, Tensor):   # (an index of A or more would name a site slot of the extended entry)
                if tuple(i.shape) == (Cn,) and bool(((i < -1) | (i >= A)).any()):
                    c = int(((i < -1) | (i >= A)).nonzero()[0])
                    raise ValueError(f"a CV needs atom indices in 0 .. {A - 1}, or -1 in an index tensor for an entry without "
                                     f"it: entry {c}, {name} with atom {int(i[c])}")
            elif not 0 <= i < A:
                raise ValueError(f"{name}: atom index {i} is outside 0 .. {A - 1}")
    periodic = (0, 0, 0) if cell is None or pbc is None else tuple(int(bool(p)) for p in pbc)
    h = inv = None
    half_width = math.inf
    if any(periodic):
        h = torch.as_tensor(cell).detach().cpu().to(torch.float64).reshape(3, 3)
        inv = torch.linalg.inv(h)
        half_width = 0.5 * min(1.0 / float(inv[:, k].norm()) for k in range(3) if periodic[k])
    m_host = None
    group_lists: tp.List[Tensor] = []
    weight_lists: tp.List[Tensor] = []
    site_kind = torch.zeros((Cn, _lib.MD_SITES_MAX + 2), dtype=torch.int32)
    site_ref = torch.zeros_like(site_kind)
    count = [0] * Cn
    slot_of: tp.List[Tensor] = []   # per unit: int64 [C], the slot of the centre or of the anchor, -1
    coord: tp.List[tp.List[int]] = []
    coord_params: tp.List[tp.List[float]] = []
    memb: tp.List[tp.Tuple[Tensor, int, int, Tensor]] = []   # (global atoms, slot, role, weights)

    def add_group(c: int, row: Tensor, w: tp.Optional[Tensor]) -> int:
        group_lists.append(row + c * A)
        weight_lists.append(torch.zeros(row.numel(), dtype=torch.float64) if w is None else w)
        return len(group_lists) - 1

    def take(c: int, n: int) -> int:
        v, count[c] = count[c], count[c] + n
        if count[c] > _lib.MD_SITES_MAX:
            raise ValueError(f"entry {c} has more than {_lib.MD_SITES_MAX} sites (a centre is one, a coordination number two)")
        return v

    for unit in units:
        slots = torch.full((Cn,), -1, dtype=torch.int64)
        if isinstance(unit, Site):
            rows = _group_rows(unit.atoms, Cn, A, real, "center")
            if unit.weights == "mass" and m_host is None:
                if masses is None:
                    raise ValueError('a centre with weights="mass" needs the masses [C, A]')
                m_host = (masses() if callable(masses) else masses).detach().cpu().to(torch.float32)
                if tuple(m_host.shape) != (Cn, A):
                    raise ValueError(f"masses must have shape {(Cn, A)}, got {tuple(m_host.shape)}")
            for c, row in enumerate(rows):
                if not row.numel():
                    continue
                if unit.weights == "mass":
                    m = m_host[c, row].to(torch.float64)
                    if not float(m.sum()) > 0 or bool((m < 0).any()):
                        raise ValueError(f"center: entry {c}: the group has zero total mass (or a negative mass)")
                    w = m / m.sum()
                else:
                    w = torch.full((row.numel(),), 1.0 / row.numel(), dtype=torch.float64)
                v = take(c, 1)
                slots[c] = v
                site_kind[c, v], site_ref[c, v] = _lib.MD_SITE_CENTER, add_group(c, row, w)
                memb.append((row + c * A, v, _lib.MD_SITE_ROLE_CENTER, w))
        else:
            co = unit
            rows_a = _group_rows(co.group_a, Cn, A, real, "coordination")
            rows_b = _group_rows(co.group_b, Cn, A, real, "coordination")
            here = [c for c in range(Cn) if rows_a[c].numel() and rows_b[c].numel()]
            where = f"coordination: entry {here[0] if here else 0}: "
            if not (math.isfinite(co.r0) and co.r0 > 0):
                raise ValueError(where + f"r0 must be > 0, got {co.r0:g}")
            if not (math.isfinite(co.d0) and co.d0 >= 0):
                raise ValueError(where + f"d0 must be >= 0, got {co.d0:g}")
            if not 2 <= co.n <= 32:
                raise ValueError(where + f"n must be an integer in 2 .. 32, got {co.n}")
            if co.r_max is not None and not co.r_max > co.d0:
                raise ValueError(where + f"r_max must be > d0 = {co.d0:g}, got {co.r_max:g}")
            if any(periodic) and co.r_max is None:
                raise ValueError(where + "a periodic cell needs r_max (the minimum image is the nearest one only within half "
                                 "the cell)")
            if co.r_max is not None and co.r_max > half_width:
                raise ValueError(where + f"r_max = {co.r_max:g} exceeds half the smallest perpendicular width of the cell over "
                                 f"its periodic directions, {half_width:g}")
            r_max = math.inf if co.r_max is None else co.r_max
            b = 0.0 if co.r_max is None else switch_base(co.r_max, co.r0, co.d0, co.n)
            for c in here:
                v = take(c, 2)
                slots[c] = v
                q = len(coord)
                site_kind[c, v], site_kind[c, v + 1] = _lib.MD_SITE_ANCHOR, _lib.MD_SITE_VALUE
                site_ref[c, v] = site_ref[c, v + 1] = q
                coord.append([c, add_group(c, rows_a[c], None), add_group(c, rows_b[c], None), v + 1, co.n])
                coord_params.append([co.r0, co.d0, r_max, b])
                zeros = torch.zeros(max(rows_a[c].numel(), rows_b[c].numel()), dtype=torch.float64)
                memb.append((rows_a[c] + c * A, v + 1, _lib.MD_SITE_ROLE_A, zeros[:rows_a[c].numel()]))
                memb.append((rows_b[c] + c * A, v + 1, _lib.MD_SITE_ROLE_B, zeros[:rows_b[c].numel()]))
        slot_of.append(slots)
    V = max(count)
    if V == 0:   # no entry has any of the sites: every CV on them is absent everywhere
        V = 1
    site_kind, site_ref = site_kind[:, :V].contiguous(), site_ref[:, :V].contiguous()
    sizes = torch.tensor([g.numel() for g in group_lists], dtype=torch.int64)
    group_offset = torch.zeros(len(group_lists) + 1, dtype=torch.int64)
    group_offset[1:] = torch.cumsum(sizes, 0)
    cat = lambda xs, dt: torch.cat(xs) if xs else torch.zeros(0, dtype=dt)   # noqa: E731
    group_atoms, group_weights = cat(group_lists, torch.int64), cat(weight_lists, torch.float64)
    # the inverse CSR: the rows of every atom in ascending slot order, side A before side B
    m_atom = cat([g for g, _, _, _ in memb], torch.int64)
    m_slot = cat([torch.full((g.numel(),), v, dtype=torch.int64) for g, v, _, _ in memb], torch.int64)
    m_role = cat([torch.full((g.numel(),), r, dtype=torch.int64) for g, _, r, _ in memb], torch.int64)
    m_w = cat([w for _, _, _, w in memb], torch.float64)
    order = torch.argsort((m_atom * _lib.MD_SITES_MAX + m_slot) * 4 + m_role, stable=True)
    member_offset = torch.zeros(Cn * A + 1, dtype=torch.int64)
    member_offset[1:] = torch.cumsum(torch.bincount(m_atom, minlength=Cn * A), 0)
    member_site = torch.stack([m_slot[order], m_role[order]], dim=1).to(torch.int32).contiguous()
    species_ext = torch.cat([species, torch.where(site_kind != 0, 0, -1).to(species.dtype)], dim=1)
    tables = SiteTables(
        V, site_kind, site_ref, group_offset.to(torch.int32), group_atoms.to(torch.int32), group_weights,
        torch.tensor(coord, dtype=torch.int32).view(-1, 5), torch.tensor(coord_params, dtype=torch.float64).view(-1, 4),
        member_offset.to(torch.int32), member_site, m_w[order].contiguous(), tuple(periodic),
        tuple(h.reshape(9).tolist()) if h is not None else (0.0,) * 9,
        tuple(inv.reshape(9).tolist()) if inv is not None else (0.0,) * 9, species_ext)
    # the CVs with every site resolved to its atom of the extended entry
    resolved: tp.Dict[int, CV] = {}
    for cv in cvs:
        if id(cv) in resolved:
            continue
        atoms = []
        for i in cv.atoms:
            if isinstance(i, Site):
                u = [k for k, unit in enumerate(units) if unit is (i if i.kind == "center" else i.coordination)][0]
                slot = slot_of[u] + (1 if i.kind == "value" else 0)
                atoms.append(torch.where(slot_of[u] >= 0, A + slot, -1))
            else:
                atoms.append(i)
        resolved[id(cv)] = CV(cv.kind, tuple(atoms))
    new_items = []
    for b in items:
        b2 = copy.copy(b)
        if isinstance(b, Restraint):
            b2.cv = resolved[id(b.cv)]
        elif isinstance(b, Metadynamics):
            b2.cvs = tuple(resolved[id(cv)] for cv in b.cvs)
        new_items.append(b2)
    fixed_ext = None if fixed is None else torch.cat([fixed.detach().cpu().to(torch.bool),
                                                      torch.zeros((Cn, V), dtype=torch.bool)], dim=1)
    return tables, build_bias_tables(species_ext, fixed_ext, new_items, temperature)


class DeviceBias:
    """The tables on the device, the hill lists and the outputs of anihip_md_bias_apply.  The host keeps every hill count
    (preloaded + deposits x members), so no call here reads the device.  With ``sites`` (``build_site_tables``) it also owns
    the extended arrays, and ``apply`` is anihip_md_sites_gather, anihip_md_bias_apply on them, anihip_md_sites_spread."""

    def __init__(self, tables: BiasTables, n_mol: int, atoms_per_mol: int, device: torch.device,
                 sites: tp.Optional[SiteTables] = None) -> None:
        self.sites = sites
        if sites is not None:
            s, A, Ax = sites, atoms_per_mol, atoms_per_mol + sites.max_sites
            self._site_held = [x.to(device).contiguous() for x in (
                s.site_kind, s.site_ref, s.group_offset, s.group_atoms, s.group_weights, s.coord, s.coord_params,
                s.member_offset, s.member_site, s.member_weight)]
            self.site_status = torch.zeros(n_mol, dtype=torch.int32, device=device)
            self.coordinates_ext = torch.zeros((n_mol, Ax, 3), dtype=torch.float32, device=device)
            self.coordinates_lo_ext = torch.zeros_like(self.coordinates_ext)
            self.forces_ext = torch.zeros_like(self.coordinates_ext)
            self.site_struct = _lib.MdSites(
                n_mol, s.max_sites, s.group_offset.numel() - 1, s.group_atoms.numel(), s.coord.shape[0], s.member_site.shape[0],
                (C.c_int32 * 3)(*s.pbc), 0, (C.c_double * 9)(*s.cell), (C.c_double * 9)(*s.inv_cell),
                *(x.data_ptr() if x.numel() else None for x in self._site_held), self.site_status.data_ptr())
            self.site_params = _lib.MdParams(n_mol, A, 0, 0, 1.0, 0, 0)
            nbytes = _lib.lib().anihip_md_sites_workspace_bytes(C.byref(self.site_params), C.byref(self.site_struct))
            self.site_workspace = torch.empty(max(1, nbytes), dtype=torch.uint8, device=device)
            atoms_per_mol = Ax   # (what the bias kernels see)
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
        x, x_lo, f = coordinates, coordinates_lo, forces
        if self.sites is not None:   # the sites appended to every entry; the bias kernels then work on the extended arrays
            x, x_lo, f = self.coordinates_ext, self.coordinates_lo_ext, self.forces_ext
            _lib.check(_lib.lib().anihip_md_sites_gather(
                _stream(), C.byref(self.site_params), C.byref(self.site_struct), coordinates.data_ptr(),
                coordinates_lo.data_ptr(), forces.data_ptr(), x.data_ptr(), x_lo.data_ptr(), f.data_ptr(),
                self.site_workspace.data_ptr(), self.site_workspace.numel()))
        _lib.check(_lib.lib().anihip_md_bias_apply(
            _stream(), C.byref(self.params), C.byref(self.struct), x.data_ptr(), x_lo.data_ptr(),
            f.data_ptr(), self.bias_energies.data_ptr(), self.meta_energies.data_ptr(), self.cv_values.data_ptr(),
            self.workspace.data_ptr(), self.workspace.numel()))
        if self.sites is not None:
            _lib.check(_lib.lib().anihip_md_sites_spread(
                _stream(), C.byref(self.site_params), C.byref(self.site_struct), coordinates.data_ptr(),
                coordinates_lo.data_ptr(), f.data_ptr(), forces.data_ptr()))

    def raise_on_bad_sites(self) -> None:
        """Raise if the kernels found a site table of an entry out of range (one host synchronization)."""
        if self.sites is None:
            return
        bad = self.site_status.nonzero()
        if bad.numel():
            c = int(bad[0])
            raise RuntimeError(f"entry {c}: the site tables are out of range (ANIHIP_MD_SITES_BAD_* bits "
                               f"{int(self.site_status[c])}): its forces carry no bias")

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
