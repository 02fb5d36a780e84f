"""Group CVs of biased MD (csrc/md_sites.hip, md.center and md.coordination) on the MI355X against the fp64 reference of
tests/_md_sites_ref.py: the gather and the spread through the C ABI on their own, the whole chain through the unchanged
anihip_md_bias_apply, broken tables, and the class in lock-step with the reference on Lennard-Jones and ANI-2x, without host
synchronization, bit-identical without sites, and under replica exchange.

Gates, derived and not measured (the conventions of tests/test_gpu_md_bias.py): an fp64 sum within 1e-11 of the sum of its
absolute terms; a force component within one fp32 ulp of the reference's fp32 value when the reference is fed the device's own
fp32 site forces (both round the same fp64 sum, which differs by fp64 rounding alone); the final forces within 2 x 2^-24 x
(|model force| + sum |bias terms|) of the all-fp64 reference (one fp32 rounding of the site force, one of the result)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _md_bias_ref as br
import _md_ref as ref
import _md_replica_exchange_ref as rx
import _md_sites_ref as sr
from test_gpu_md_device import SEED, _stream
from test_gpu_md_replica_exchange import _ani_replicas, _lj_replicas

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
GUARD = 16
SUM_GATE = 1e-11
L_BOX = 9.0
CELLS = {
    "open": (None, (0, 0, 0)),
    "orthorhombic": (np.diag([10.0, 11.0, 12.0]), (1, 1, 1)),
    "triclinic": (np.array([[10.0, 0.0, 0.0], [2.5, 10.5, 0.0], [-1.5, 2.0, 11.0]]), (1, 1, 1)),
    "mixed": (np.array([[10.0, 0.0, 0.0], [2.5, 10.5, 0.0], [-1.5, 2.0, 11.0]]), (1, 0, 1)),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from torchani_amd import _lib

    _lib.lib()
    return torch.device("cuda:0")


def _guarded(dev, shape, dtype, fill=SENTINEL):
    """A tensor of ``shape`` filled with ``fill`` in front of GUARD elements of it: (the view, the whole buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device=dev)
    return buf[:n].view(*shape), buf


class Abi:
    """The three calls of one evaluation on the tables of ``build_site_tables``: device copies (``broken`` swaps tables for
    broken ones), the extended arrays, the outputs and the workspaces, every buffer the kernels write followed by guards."""

    def __init__(self, dev, site_tables, bias_tables, Cn, A, **broken):
        from torchani_amd import _lib

        self.lib, self._lib, self.dev, self.Cn, self.A, self.V = _lib.lib(), _lib, dev, Cn, A, site_tables.max_sites
        s, V, Ax = site_tables, site_tables.max_sites, A + site_tables.max_sites
        t = s._asdict()
        t.update(broken)
        names = ("site_kind", "site_ref", "group_offset", "group_atoms", "group_weights", "coord", "coord_params",
                 "member_offset", "member_site", "member_weight")
        self.t = {k: t[k].to(dev).contiguous() for k in names}
        self.guards = []
        self.status, buf = _guarded(dev, (Cn,), torch.int32, -1)
        self.guards.append((buf, Cn, -1))
        for name in ("xe", "loe", "fe"):
            view, buf = _guarded(dev, (Cn, Ax, 3), torch.float32)
            setattr(self, name, view)
            self.guards.append((buf, Cn * Ax * 3, SENTINEL))
        self.f, buf = _guarded(dev, (Cn, A, 3), torch.float32)
        self.guards.append((buf, Cn * A * 3, SENTINEL))
        ptr = lambda x: x.data_ptr() if x.numel() else None   # noqa: E731
        self.s = _lib.MdSites(Cn, V, s.group_offset.numel() - 1, s.group_atoms.numel(), s.coord.shape[0], s.member_site.shape[0],
                              (C.c_int32 * 3)(*s.pbc), 0, (C.c_double * 9)(*s.cell), (C.c_double * 9)(*s.inv_cell),
                              *(ptr(self.t[k]) for k in names), self.status.data_ptr())
        self.P = _lib.MdParams(Cn, A, 0, 0, 1.0, 0, 0)
        self.ws_bytes = self.lib.anihip_md_sites_workspace_bytes(C.byref(self.P), C.byref(self.s))
        assert self.ws_bytes == s.coord.shape[0] * ((A + 255) // 256) ** 2 * 8
        self.ws, buf = _guarded(dev, (max(1, self.ws_bytes // 8),), torch.float64)
        self.guards.append((buf, max(1, self.ws_bytes // 8), SENTINEL))
        # the unchanged bias kernels on entries of A + V atoms
        b = bias_tables
        bnames = ("cv_offset", "kind", "atoms", "restraint", "meta_cv", "inv_sigma2", "height", "list", "rank_in_list", "members",
                  "list_entry", "bias_factor")
        self.bt = {k: getattr(b, k).to(dev).contiguous() for k in bnames}
        G, cap = int(b.members.numel()), int(b.capacity) if b.members.numel() else 0
        self.used = b.used.to(dev).contiguous()
        self.dropped = torch.zeros(G, dtype=torch.int32, device=dev)
        self.centers = torch.zeros((G, 2, cap), dtype=torch.float64, device=dev)
        self.heights = torch.zeros((G, cap), dtype=torch.float64, device=dev)
        n0 = b.heights.shape[1]
        if G and n0:
            self.centers[:, :, :n0], self.heights[:, :n0] = b.centers.to(dev), b.heights.to(dev)
        ncv = int(b.kind.numel())
        self.bias_status = torch.full((Cn,), -1, dtype=torch.int32, device=dev)
        self.cv_values = torch.full((max(1, ncv),), SENTINEL, dtype=torch.float64, device=dev)
        self.e_bias = torch.full((Cn,), SENTINEL, dtype=torch.float64, device=dev)
        self.e_meta = torch.full((Cn,), SENTINEL, dtype=torch.float64, device=dev)
        self.b = _lib.MdBias(ncv, G, cap, 0, 0, Cn, *(ptr(self.bt[k]) for k in bnames), ptr(self.used), ptr(self.dropped),
                             ptr(self.centers), ptr(self.heights), self.bias_status.data_ptr())
        self.Px = _lib.MdParams(Cn, Ax, 0, 0, 1.0, 0, 0)
        self.bws = torch.empty(max(8, self.lib.anihip_md_bias_workspace_bytes(C.byref(self.Px), C.byref(self.b))),
                               dtype=torch.uint8, device=dev)

    def set_x(self, x64):
        """Two-float coordinates of the fp64 positions; returns what the kernels read, exactly."""
        hi = x64.astype(np.float32)
        self.x = torch.from_numpy(hi).to(self.dev)
        self.lo = torch.from_numpy((x64 - hi.astype(np.float64)).astype(np.float32)).to(self.dev)
        return self.x.double().cpu().numpy() + self.lo.double().cpu().numpy()

    def gather(self, forces):
        self.f.copy_(torch.from_numpy(np.ascontiguousarray(forces, dtype=np.float32)))
        self._lib.check(self.lib.anihip_md_sites_gather(
            _stream(), C.byref(self.P), C.byref(self.s), self.x.data_ptr(), self.lo.data_ptr(), self.f.data_ptr(),
            self.xe.data_ptr(), self.loe.data_ptr(), self.fe.data_ptr(), self.ws.data_ptr(), self.ws_bytes))
        return {"coords": self.xe.cpu().numpy(), "coords_lo": self.loe.cpu().numpy(), "forces": self.fe.cpu().numpy(),
                "status": self.status.cpu().numpy()}

    def bias(self):
        self._lib.check(self.lib.anihip_md_bias_apply(
            _stream(), C.byref(self.Px), C.byref(self.b), self.xe.data_ptr(), self.loe.data_ptr(), self.fe.data_ptr(),
            self.e_bias.data_ptr(), self.e_meta.data_ptr(), self.cv_values.data_ptr(), self.bws.data_ptr(), self.bws.numel()))

    def spread(self, forces_ext=None):
        if forces_ext is not None:
            self.fe.copy_(torch.from_numpy(np.ascontiguousarray(forces_ext, dtype=np.float32)))
        self._lib.check(self.lib.anihip_md_sites_spread(
            _stream(), C.byref(self.P), C.byref(self.s), self.x.data_ptr(), self.lo.data_ptr(), self.fe.data_ptr(),
            self.f.data_ptr()))
        return self.f.cpu().numpy()

    def chain(self, forces):
        g = self.gather(forces)
        self.bias()
        fe = self.fe.cpu().numpy()
        out = {"forces": self.spread(), "forces_ext": fe, "cv_values": self.cv_values.cpu().numpy(),
               "bias_energies": self.e_bias.cpu().numpy(), "meta_energies": self.e_meta.cpu().numpy(), "status": g["status"],
               "bias_status": self.bias_status.cpu().numpy()}
        return out

    def guards_untouched(self):
        return all(bool((buf[n:] == fill).all()) for buf, n, fill in self.guards)


# ---- the case -------------------------------------------------------------------------------------------------------------------

def _twisted(phi):
    """Four points with a dihedral of +-phi."""
    return np.array([[-0.5, 1.0, 0.0], [0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [2.0, math.cos(phi), math.sin(phi)]])


_CASES = {}


def _case(Cn, A, cell_kind="open", perm=None, displaced=False):
    """Species (entry 1 with 9 padding atoms; with C = 3 the last entry without sites), fp64 positions, incoming forces, the
    bias, the cell and what the tests need to know of the groups.  Entry 0 carries the sizes the issue names; ``perm`` puts
    entry perm[c] of the unpermuted case at batch position c; ``displaced`` moves every atom by whole lattice vectors along
    the periodic directions."""
    from torchani_amd import md

    key = (Cn, A, cell_kind, None if perm is None else tuple(perm), displaced)
    if key in _CASES:
        return _CASES[key]
    cell, pbc = CELLS[cell_kind]
    rs = np.random.RandomState(100 + A)
    x = rs.uniform(0.0, L_BOX, (Cn, A, 3)).astype(np.float32).astype(np.float64)
    lo = rs.uniform(-1e-7, 1e-7, x.shape)
    f0 = rs.normal(0.0, 0.05, (Cn, A, 3)).astype(np.float32)
    species = np.zeros((Cn, A), dtype=np.int64)
    species[1, A - 9:] = -1
    masses = rs.choice([1.008, 12.011, 14.007, 15.999], (Cn, A)).astype(np.float32)
    big = A > 256
    # constructed geometry in entry 0, two-float pairs with a zero low word
    e = A - 20   # twelve atoms nobody else uses: four pairs around the points of a dihedral near pi, an edge case
    pts = _twisted(math.pi - 0.03) + np.array([3.0, 3.0, 3.0])
    for k in range(4):
        delta = np.array([0.25, 0.125 * (k + 1), -0.25])
        x[0, e + 2 * k], x[0, e + 2 * k + 1] = pts[k] + delta, pts[k] - delta
    d0_edge, r_max = 1.5, 4.0
    x[0, e + 8] = (1.0, 1.0, 1.0)
    x[0, e + 9] = (1.0 + d0_edge, 1.0, 1.0)   # exactly at r = d0: sw = 1, no force
    x[0, e + 10] = (1.0, 1.0 + r_max, 1.0)    # exactly at r = r_max: sw = 0, no force
    x[0, e:e + 11] = x[0, e:e + 11].astype(np.float32)
    lo[0, e:e + 11] = 0.0
    x = x + lo
    if displaced:
        shift = rs.randint(-2, 3, (Cn, A, 3)) * np.asarray(pbc)
        shift[0, e + 8:e + 11] = shift[0, e + 8]   # (the constructed pairs move together)
        shift[0, e:e + 8] = 0                      # (centres take no minimum image: the dihedral over them stays)
        x = x + shift @ cell
    perm = list(range(Cn)) if perm is None else list(perm)
    inv = {old: new for new, old in enumerate(perm)}

    def rows(by_old):
        """A [C, A] mask with the atoms by_old[old] in the row of old entry ``old``."""
        m = torch.zeros((Cn, A), dtype=torch.bool)
        for old, atoms in by_old.items():
            m[inv[old], list(atoms)] = True
        return m

    def only(by_old, dtype=torch.int64, default=-1):
        t = torch.full((Cn,), default, dtype=dtype)
        for old, v in by_old.items():
            if old in inv:   # (C = 2 has no third entry)
                t[inv[old]] = v
        return t

    R = lambda a, b: range(a, b)   # noqa: E731
    cut = None if cell is None else r_max   # (an open cell also runs the switching function without a cut)
    if big:
        centre_groups = {"c255": R(0, 255), "c256": R(100, 356), "c257": R(300, 557), "c513": R(40, 553)}
        coords = {"3x257": (R(1, 4), R(300, 557), dict(r0=2.0, n=6, r_max=r_max)),
                  "256x256": (R(0, 256), R(256, 512), dict(r0=1.8, d0=0.4, n=8, r_max=r_max)),
                  "300x300": (R(150, 450), R(150, 450), dict(r0=2.0, n=6, r_max=3.5))}
        ca, cb, cc = "c255", "c256", "c513"
        meta_coord = "3x257"
    else:
        centre_groups = {"c1": [3], "c2": [4, 10], "c64": R(0, 64)}
        coords = {"1x1": ([5], [9], dict(r0=3.0, n=2, r_max=cut)),
                  "overlap": (R(10, 30), R(20, 45), dict(r0=1.6, d0=0.5, n=12, r_max=r_max))}
        ca, cb, cc = "c1", "c2", "c64"
        meta_coord = "overlap"
    # entry 1 (the one with padding) has a centre of two, one of forty, and a coordination number of its own
    site = {name: md.center(rows({0: g, 1: [2, 6]} if name == cb else {0: g, 1: R(0, 40)} if name == cc else {0: g}),
                            "mass" if name != ca else None) for name, g in centre_groups.items()}
    cvs = {name: md.coordination(rows({0: a, 1: R(0, 12)} if name == meta_coord else {0: a}),
                                 rows({0: b, 1: R(8, 30)} if name == meta_coord else {0: b}), **kw)
           for name, (a, b, kw) in coords.items()}
    cvs["edge"] = md.coordination(rows({0: [e + 8]}), rows({0: [e + 9, e + 10]}), 1.0, d0=d0_edge, n=6, r_max=r_max)
    quad = [md.center(rows({0: [e + 2 * k, e + 2 * k + 1]}), None) for k in range(4)]
    cvs["com"] = md.distance(site[cb], site[cc])
    cvs["com2"] = md.distance(site[ca], site[cb])
    cvs["angle"] = md.angle(only({0: 7, 1: 50}), site[cb], site[cc])   # (atom, centre, centre)
    cvs["dihedral"] = md.dihedral(*quad)
    cvs["plain"] = md.distance(only({0: 10, 1: 3, 2: 0}), only({0: 31, 1: 4, 2: 1}))   # atom 10 is in two centres and a group
    groups = {"centres": centre_groups, "coords": {k: (list(a), list(b)) for k, (a, b, _) in coords.items()}}
    # values at the start, for centres and hills that matter
    x0 = x[0]
    w = {name: (masses[0][list(g)].astype(np.float64) if name != ca else np.ones(len(g))) for name, g in centre_groups.items()}
    pos = {name: sr.center(x0, list(g), w[name] / w[name].sum())[0] for name, g in centre_groups.items()}
    d_com = np.linalg.norm(pos[cb] - pos[cc])
    a, b, kw = coords[meta_coord]
    p = (kw["r0"], kw.get("d0", 0.0), math.inf if kw.get("r_max") is None else kw["r_max"], kw["n"])
    s_meta = sr.coordination(x0, list(a), list(b), p, cell, pbc)[0]
    s_dih = br.cv(br.DIHEDRAL, np.stack([(x0[e + 2 * k] + x0[e + 2 * k + 1]) / 2 for k in range(4)]))[0]
    assert abs(s_dih) > math.pi - 0.05 and s_meta > 1.0 and d_com > 0.05
    bias = [md.Restraint(cvs["com"], only({0: d_com + 0.7, 1: 3.0}, torch.float64, 0.0), 0.05),
            md.Restraint(cvs["com2"], 2.0, 0.02, 0.1),
            md.Restraint(cvs["angle"], 1.2, 0.04),
            md.Restraint(cvs["dihedral"], -s_dih + math.copysign(0.01, s_dih), 0.3),   # across the seam: it wraps
            md.Restraint(cvs[meta_coord], only({0: 0.8 * s_meta, 1: 5.0}, torch.float64, 0.0), 2e-3 / max(1.0, s_meta)),
            md.Restraint(cvs["edge"], 3.0, 0.01),
            md.Restraint(cvs["plain"], 4.0, 0.01)]
    bias += [md.Restraint(cvs[name], 0.5 * sr.coordination(x0, list(a), list(b), (
        kw["r0"], kw.get("d0", 0.0), math.inf if kw.get("r_max") is None else kw["r_max"], kw["n"]), cell, pbc)[0] + 0.3,
        1e-3 / len(a)) for name, (a, b, kw) in coords.items() if name != meta_coord]
    n0 = 40
    centers = np.stack([d_com + rs.uniform(-0.3, 0.3, n0), s_meta * (1.0 + rs.uniform(-0.1, 0.1, n0))])[None]
    heights = rs.uniform(0.5e-3, 2e-3, (1, n0))
    bias.append(md.Metadynamics([cvs["com"], cvs[meta_coord]], (0.2, 0.1 * s_meta), 1e-3, 1, walkers=only({0: 7}),
                                max_hills=64, hills=(torch.from_numpy(centers), torch.from_numpy(heights))))
    st, bt = md.build_site_tables(torch.from_numpy(species[perm]), None, bias, masses=torch.from_numpy(masses[perm]),
                                  cell=None if cell is None else torch.from_numpy(cell), pbc=pbc)
    out = {"species": species[perm], "x": x[perm], "f0": f0[perm], "sites": st, "bias": bt, "groups": groups, "edge": e,
           "inv": inv, "cvs": cvs, "names": [ca, cb, cc, meta_coord]}
    _CASES[key] = out
    return out


_WANT = {}


def _reference(case_key, k, case):
    """The reference chain of a case, computed once at the positions the kernels read."""
    if case_key not in _WANT:
        xk = k.set_x(case["x"])
        sites = sr.Sites(case["sites"], case["x"].shape[1])
        _WANT[case_key] = (xk, sites, sites.apply(br.Bias(case["bias"]), xk, case["f0"]))
    else:
        k.set_x(case["x"])
    return _WANT[case_key]


SHAPES = [(3, 70), (2, 600)]


# ---- the gather -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell_kind", list(CELLS))
@pytest.mark.parametrize("Cn,A", SHAPES)
def test_gather_matches_reference(dev, Cn, A, cell_kind):
    case = _case(Cn, A, cell_kind)
    st = case["sites"]
    V = st.max_sites
    k = Abi(dev, st, case["bias"], Cn, A)
    xk, sites, want = _reference((Cn, A, cell_kind), k, case)
    g = want["gather"]
    got = k.gather(case["f0"])
    assert (got["status"] == 0).all()
    # real atoms and their forces bit for bit
    assert np.array_equal(got["coords"][:, :A], k.x.cpu().numpy()) and np.array_equal(got["coords_lo"][:, :A], k.lo.cpu().numpy())
    assert np.array_equal(got["forces"][:, :A], case["f0"])
    kind = st.site_kind.numpy()
    pair = got["coords"][:, A:].astype(np.float64) + got["coords_lo"][:, A:].astype(np.float64)
    worst_c = worst_s = 0.0
    for c in range(Cn):
        for v in range(V):
            if kind[c, v] == sr.NONE:   # inactive slots untouched
                assert (got["coords"][c, A + v] == SENTINEL).all() and (got["coords_lo"][c, A + v] == SENTINEL).all()
                assert (got["forces"][c, A + v] == SENTINEL).all()
                continue
            assert (got["forces"][c, A + v] == 0.0).all()
            # the pair is hi = (float)x, lo = (float)(x - hi) of some x
            assert np.array_equal(got["coords"][c, A + v], pair[c, v].astype(np.float32))
            if kind[c, v] == sr.CENTER:
                err = np.abs(pair[c, v] - g["sites"][c, v]) / g["scale"][c, v]
                worst_c = max(worst_c, err.max())
                assert (err <= SUM_GATE).all()
            elif kind[c, v] == sr.ANCHOR:
                assert (got["coords"][c, A + v] == 0.0).all() and (got["coords_lo"][c, A + v] == 0.0).all()
            else:
                s, scale = g["sites"][c, v, 0], g["scale"][c, v, 0]
                err = abs(pair[c, v, 0] - max(s, sr.FLOOR)) / max(scale, sr.FLOOR)
                worst_s = max(worst_s, err)
                assert err <= SUM_GATE and (pair[c, v, 1:] == 0.0).all()
    # the pair exactly at r = d0 counts 1, the one at r = r_max nothing: s = 1 exactly, whatever the cell
    q_edge = [q for q in range(st.coord.shape[0]) if st.coord[q, 4] == 6 and st.coord_params[q, 1] == 1.5][0]
    c, v = int(st.coord[q_edge, 0]), int(st.coord[q_edge, 3])
    assert pair[c, v, 0] == 1.0 and g["sites"][c, v, 0] == 1.0
    sizes = sorted({int(n) for n in np.diff(st.group_offset.numpy())})
    print(f"md sites, gather, C = {Cn}, A = {A}, {cell_kind} cell: centres |d| / sum|terms| {worst_c:.1e}, coordination numbers "
          f"|ds| / sum|terms| {worst_s:.1e} (values up to {g['sites'][:, :, 0][kind == sr.VALUE].max():.1f}); group sizes {sizes}")
    again = k.gather(case["f0"])
    for key in got:
        assert np.array_equal(got[key], again[key]), key
    assert k.guards_untouched()


@pytest.mark.parametrize("Cn,A", SHAPES)
def test_minimum_image_gives_the_number_of_the_undisplaced_copy(dev, Cn, A):
    """Mixed periodic flags, every atom moved by whole lattice vectors along the periodic directions."""
    values = []
    for displaced in (False, True):
        case = _case(Cn, A, "mixed", displaced=displaced)
        st = case["sites"]
        k = Abi(dev, st, case["bias"], Cn, A)
        xk = k.set_x(case["x"])
        got = k.gather(case["f0"])
        assert (got["status"] == 0).all()
        vals = (got["coords"][:, A:, 0].astype(np.float64) + got["coords_lo"][:, A:, 0].astype(np.float64))[
            st.site_kind.numpy() == sr.VALUE]
        if displaced:   # also against the reference at the displaced positions
            g = sr.Sites(st, A).gather(xk, case["f0"])
            sel = st.site_kind.numpy() == sr.VALUE
            assert (np.abs(vals - np.maximum(g["sites"][:, :, 0][sel], sr.FLOOR)) <= SUM_GATE * g["scale"][:, :, 0][sel]).all()
            scale = g["scale"][:, :, 0][sel]
            assert np.abs(case["x"] - _case(Cn, A, "mixed")["x"]).max() > 9.0
        values.append(vals)
    diff = np.abs(values[0] - values[1])
    err = diff / np.maximum(scale, sr.FLOOR)   # (a number of no pair within reach is the floor in both copies)
    print(f"md sites, minimum image, C = {Cn}, A = {A}: coordination numbers of the displaced copy within {err.max():.1e} of "
          f"sum|terms| of the undisplaced one ({values[0].size} numbers up to {values[0].max():.1f})")
    assert (diff <= SUM_GATE * scale).all()


# ---- the spread -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell_kind", ["open", "triclinic"])
@pytest.mark.parametrize("Cn,A", SHAPES)
def test_spread_matches_reference(dev, Cn, A, cell_kind):
    case = _case(Cn, A, cell_kind)
    st = case["sites"]
    V = st.max_sites
    k = Abi(dev, st, case["bias"], Cn, A)
    xk, sites, _ = _reference((Cn, A, cell_kind), k, case)
    rs = np.random.RandomState(4)
    fe = rs.normal(0.0, 0.05, (Cn, A + V, 3)).astype(np.float32)   # random site forces too
    k.gather(case["f0"])   # (the status the spread reads)
    got = k.spread(fe)
    want, _ = sites.spread(xk, fe)
    ulps = sr.ulps32(got, want)
    off = st.member_offset.numpy()
    member = (np.diff(off) > 0).reshape(Cn, A)
    print(f"md sites, spread, C = {Cn}, A = {A}, {cell_kind} cell: forces within {ulps.max():.2f} fp32 ulp on {int(member.sum())} "
          f"atoms of groups (up to {int(np.diff(off).max())} memberships; largest force {np.abs(want).max():.2e} Ha/A)")
    assert (ulps <= 1.0).all()
    assert member.any() and (~member).any() and np.array_equal(got[~member], fe[:, :A][~member])
    assert (np.abs(got.astype(np.float64) - fe[:, :A])[member].max(axis=-1) > 0).mean() > 0.9
    if not A > 256:   # the shared atom: two centres and a coordination group, in slot order
        gi = case["inv"][0] * A + 10
        rows_ = st.member_site.numpy()[off[gi]:off[gi + 1]]
        assert rows_.shape[0] >= 3 and (np.diff(rows_[:, 0]) >= 0).all() and sorted(rows_[:, 1])[:2] == [0, 0] and rows_[:, 1].max() >= 1
    again = k.spread(fe)
    assert np.array_equal(got, again) and k.guards_untouched()


# ---- the whole chain through anihip_md_bias_apply -------------------------------------------------------------------------------

def _compare_chain(got, want, sites, xk, what):
    """Prints every figure, then asserts the gates of the module docstring."""
    ncv = want["cv_values"].size
    dcv = np.abs(got["cv_values"][:ncv] - want["cv_values"])
    scale = want["energy_scale"]
    de = np.abs(got["bias_energies"] - want["bias_energies"])
    dm = np.abs(got["meta_energies"] - want["meta_energies"])
    fed, _ = sites.spread(xk, got["forces_ext"])   # the reference fed the device's own fp32 site forces
    ulps = sr.ulps32(got["forces"], fed)
    d64 = np.abs(got["forces"].astype(np.float64) - want["forces64"])
    bound = 2.0 * 2.0 ** -24 * want["force_scale"]
    biased = np.abs(want["forces64"] - want["gather"]["forces"][:, :sites.A]).sum(axis=-1) > 0
    print(f"md sites, {what}: max |d cv| / max(1, |cv|) {np.max(dcv / np.maximum(1.0, np.abs(want['cv_values']))):.1e}, max |dE| / "
          f"sum|terms| {np.max(de / np.maximum(scale, 1e-300)):.1e}, forces within {ulps.max():.2f} fp32 ulp of the reference fed "
          f"the device's site forces and {np.max(d64 / np.maximum(bound, 1e-300)):.2f} of the all-fp64 bound on {int(biased.sum())} "
          f"biased atoms (largest bias force {np.abs(want['forces64'] - want['gather']['forces'][:, :sites.A]).max():.2e} Ha/A)")
    # a CV is a few operations on sums at the sum gate: the gate against its own magnitude
    assert (dcv <= SUM_GATE * np.maximum(1.0, np.abs(want["cv_values"]))).all()
    assert (de <= SUM_GATE * scale).all() and (dm <= SUM_GATE * scale).all()
    assert (ulps <= 1.0).all()
    assert (d64 <= bound).all()
    return biased


@pytest.mark.parametrize("cell_kind", ["open", "orthorhombic"])
@pytest.mark.parametrize("Cn,A", SHAPES)
def test_chain_matches_reference(dev, Cn, A, cell_kind):
    case = _case(Cn, A, cell_kind)
    k = Abi(dev, case["sites"], case["bias"], Cn, A)
    xk, sites, want = _reference((Cn, A, cell_kind), k, case)
    # what the case promises: hills that matter, a dihedral over four centres at the seam, restraints that pull
    bt = case["bias"]
    c0 = case["inv"][0]
    lo, hi = bt.cv_offset[c0], bt.cv_offset[c0 + 1]
    kinds, vals = bt.kind.numpy()[lo:hi], want["cv_values"][lo:hi]
    assert (np.abs(vals[kinds == br.DIHEDRAL]) > math.pi - 0.05).any() and want["meta_energies"][c0] > 1e-4
    assert hi - lo >= 8 and np.isfinite(want["forces64"]).all()
    got = k.chain(case["f0"])
    assert (got["status"] == 0).all() and (got["bias_status"] == 0).all()
    biased = _compare_chain(got, want, sites, xk, f"chain, C = {Cn}, A = {A}, {cell_kind} cell")
    assert np.array_equal(got["forces"][~biased], case["f0"][~biased]) and biased.sum() > A // 2
    if Cn == 3:   # the entry without sites carries its plain-atom CV through the extended arrays
        c2 = case["inv"][2]
        assert biased[c2].sum() == 2 and got["bias_energies"][c2] > 0.0
    again = k.chain(case["f0"])
    for key in got:
        assert np.array_equal(got[key], again[key]), key
    assert k.guards_untouched()


def test_an_entry_gives_the_same_bits_elsewhere_in_the_batch(dev):
    Cn, A = 3, 70
    out = {}
    for perm in ((0, 1, 2), (2, 0, 1)):
        case = _case(Cn, A, "triclinic", perm=perm)
        k = Abi(dev, case["sites"], case["bias"], Cn, A)
        k.set_x(case["x"])
        got = k.chain(case["f0"])
        assert (got["status"] == 0).all()
        off = case["bias"].cv_offset.numpy()
        V = case["sites"].max_sites
        out[perm] = {old: (got["forces"][new], got["bias_energies"][new], got["meta_energies"][new],
                           got["cv_values"][off[new]:off[new + 1]]) for new, old in enumerate(perm)}
        assert V >= 12
    for old in range(Cn):
        for a, b in zip(out[(0, 1, 2)][old], out[(2, 0, 1)][old]):
            assert np.array_equal(a, b)


# ---- broken tables --------------------------------------------------------------------------------------------------------------

def test_broken_tables_flag_the_entry_and_move_nothing_of_it(dev):
    from torchani_amd import _lib

    Cn, A = 3, 70
    case = _case(Cn, A, "open")
    st = case["sites"]
    good = Abi(dev, st, case["bias"], Cn, A)
    good.set_x(case["x"])
    want = good.chain(case["f0"])
    kind, refs, off = st.site_kind.numpy(), st.site_ref.numpy(), st.group_offset.numpy()

    def broken(name, index, value):
        t = getattr(st, name).clone()
        t[index] = value
        return {name: t}

    # a group atom of entry 0 that lies in entry 1
    g0 = max((int(refs[0, v]) for v in np.nonzero(kind[0] == sr.CENTER)[0]), key=lambda g: off[g + 1] - off[g])
    assert off[g0 + 1] - off[g0] == 64
    # a centre of entry 1 whose group does not exist
    v1 = int(np.nonzero(kind[1] == sr.CENTER)[0][0])
    # the end of the last group below its start: its owner is the last coordination number's entry
    last = off.size - 2
    owner = int(st.coord[[q for q in range(st.coord.shape[0]) if last in st.coord[q, 1:3].tolist()][0], 0])
    cases = [(broken("group_atoms", int(off[g0]) + 5, A + 3), 0, _lib.MD_SITES_BAD_GROUP),
             (broken("group_atoms", int(off[g0]), -4), 0, _lib.MD_SITES_BAD_GROUP),
             (broken("site_ref", (1, v1), 999), 1, _lib.MD_SITES_BAD_SITE),
             (broken("site_ref", (1, v1), -1), 1, _lib.MD_SITES_BAD_SITE),
             (broken("site_kind", (1, v1), 9), 1, _lib.MD_SITES_BAD_SITE | _lib.MD_SITES_BAD_MEMBER),
             (broken("group_offset", last + 1, int(off[last]) - 1), owner, _lib.MD_SITES_BAD_SITE),
             (broken("group_offset", last + 1, int(off[-1]) + 1000), owner, _lib.MD_SITES_BAD_SITE),
             (broken("member_offset", 1 * A + 4, int(st.member_offset[-1]) + 7), 1, _lib.MD_SITES_BAD_MEMBER)]
    for tab, flagged, bit in cases:
        k = Abi(dev, st, case["bias"], Cn, A, **tab)
        k.set_x(case["x"])
        got = k.chain(case["f0"])
        assert got["status"][flagged] == bit and (np.delete(got["status"], flagged) == 0).all(), (tab.keys(), got["status"])
        assert np.array_equal(got["forces"][flagged], case["f0"][flagged])   # the model's forces, bit for bit
        # its sites stand at (v + 1, 0, 0): finite positions for the bias kernels
        xe = k.xe.cpu().numpy()[flagged, A:]
        for v in range(st.max_sites):
            if k.t["site_kind"][flagged, v] != 0:
                assert xe[v].tolist() == [v + 1.0, 0.0, 0.0]
        for c in range(Cn):
            if c != flagged:   # the others as if nothing were wrong
                assert np.array_equal(got["forces"][c], want["forces"][c]) and got["bias_energies"][c] == want["bias_energies"][c]
        assert k.guards_untouched()


# ---- through the class ----------------------------------------------------------------------------------------------------------

def _lock_step(dyn, n_steps, what):
    """``n_steps`` steps of ``dyn`` with the reference recomputing the sites, CVs, energies, forces and deposits from the
    device's coordinates after each; hill tables exact in count and centres."""
    b = dyn._bias
    A = dyn.species.shape[1]
    sites, model = sr.Sites(b.sites, A), br.Bias(b.tables)
    deposits = 0
    for s in range(n_steps):
        dyn.step()
        x = dyn.coordinates.double().cpu().numpy() + dyn.coordinates_lo.double().cpu().numpy()
        _, f_model = dyn._model_eval(dyn.coordinates)   # (bit-reproducible evaluators: the forces the bias was added to)
        want = sites.apply(model, x, f_model.cpu().numpy())
        got = {"forces": dyn.forces.cpu().numpy(), "forces_ext": b.forces_ext.cpu().numpy(), "cv_values": b.cv_values.cpu().numpy(),
               "bias_energies": dyn.bias_energies.cpu().numpy(), "meta_energies": b.meta_energies.cpu().numpy()}
        _compare_chain(got, want, sites, x, f"{what}, step {s + 1}")
        assert int(b.site_status.abs().max()) == 0
        cvs = dyn.collective_variables().cpu().numpy()
        idx = b.tables.cv_index.numpy()
        assert np.array_equal(cvs[idx >= 0], got["cv_values"][idx[idx >= 0]]) and np.isnan(cvs[idx < 0]).all()
        if b.n_lists and b.pace and (s + 1) % b.pace == 0:
            kT = torch.mul(dyn.temperature, ref.KB_HARTREE).cpu().numpy()
            # (the reference deposits at the device's CV values: the tables then agree exactly)
            model.deposit(kT, got["cv_values"], got["meta_energies"])
            deposits += 1
        if b.n_lists:
            centers, heights, used = (t.cpu().numpy() for t in dyn.hills())
            assert np.array_equal(used, model.used) and list(used) == b.counts
            for g in range(b.n_lists):
                n = used[g]
                assert np.array_equal(centers[g][:, :n], model.centers[g][:, :n])
                assert (np.abs(heights[g][:n] - model.heights[g][:n]) <= 4.0 * np.spacing(model.heights[g][:n])).all()
                assert (heights[g][n:] == 0.0).all()
    return deposits


def _lj_bias(md):
    """Umbrella windows on the distance between the centres of two faces of the cube, and a coordination restraint."""
    com = md.distance(md.center([0, 1, 2, 3]), md.center([4, 5, 6, 7]))
    window = torch.linspace(1.0, 1.4, 5, dtype=torch.float64)
    return com, [md.Restraint(com, window, 0.05),
                 md.Restraint(md.coordination([0, 1, 2, 3], [4, 5, 6, 7], 1.3, d0=0.2, n=6, r_max=3.0), 5.0, 0.002)]


def test_class_on_lennard_jones_conserves_energy_in_lock_step(dev):
    from torchani_amd import md

    lj, sp, x, mass = _lj_replicas(dev)
    _, bias = _lj_bias(md)
    dyn = md.BatchedDynamics(lj, sp, x, dt=1.0, masses=mass, seed=7, bias=bias)
    dyn.set_temperature(100.0)
    assert dyn._bias.sites is not None and dyn._bias.sites.max_sites == 4
    e0, bias0 = dyn.total_energies().clone(), dyn.bias_energies.clone()
    _lock_step(dyn, 6, "Lennard-Jones cube x 5, NVE, umbrella windows on a COM distance and a coordination restraint")
    assert float(dyn.bias_energies.min()) > 0.0
    drift = (dyn.total_energies() - e0).abs().max().item()
    moved = float((dyn.bias_energies - bias0).abs().max())
    print(f"md sites, LJ cube NVE: |d(total energy)| after 6 steps {drift:.1e} Ha; the bias energies (up to "
          f"{dyn.bias_energies.max().item():.1e} Ha) changed by up to {moved:.1e} Ha")
    assert drift < 0.1 * moved
    dyn.run(2)   # (the periodic host checks read the site status)


def _ani_bias(md, sp):
    """Sites and plain atoms mixed: a restraint on (atom, centre, centre), and 2-CV well-tempered hills of two walkers on
    (distance of an atom from the centre of the molecule, a coordination number of the first atoms against the rest)."""
    real = (sp >= 0).cpu()
    n_real = real.sum(dim=1)
    first = real & (torch.arange(sp.shape[1]).view(1, -1) < (n_real // 2).view(-1, 1))
    whole, half, rest = md.center(real), md.center(first, None), real & ~first
    dist = md.distance(0, whole)
    coord = md.coordination(first, rest, 2.0, d0=0.3, n=6, r_max=6.0)
    return [md.Restraint(md.angle(1, half, whole), 1.5, 0.05, torch.tensor([0.0, 0.1, 0.0, 0.05, 0.0, 0.2], dtype=torch.float64)),
            md.Restraint(md.distance(0, 2), 2.0, 0.02),
            md.Restraint(coord, 3.0, 1e-3),
            md.Metadynamics([dist, coord], (0.1, 0.3), 2e-4, 2, bias_factor=6.0, walkers=torch.tensor([4, 4, -1, 9, -1, -1]),
                            max_hills=16)]


def test_class_on_ani2x_in_lock_step_with_reference(dev):
    from torchani_amd import md

    model, sp, x, mass = _ani_replicas(dev)
    model.deterministic_forces = True   # (force sums in fixed point: a second evaluation gives the same bits)
    T = torch.tensor([300.0, 320.0, 340.0, 300.0, 310.0, 330.0], dtype=torch.float64)
    dyn = md.BatchedDynamics(model, sp, x, dt=0.5, masses=mass, temperature=T, friction=0.05, seed=SEED, bias=_ani_bias(md, sp))
    dyn.set_temperature(T)
    b = dyn._bias
    assert b.n_lists == 2 and b.members == [2, 1] and b.counts == [0, 0] and b.sites.max_sites == 4
    assert tuple(dyn.collective_variables().shape) == (6, 4)
    deposits = _lock_step(dyn, 6, "ANI-2x x 6, Langevin, sites and atoms mixed, 2-CV well-tempered hills of two walkers")
    assert deposits == 3 and b.counts == [6, 3] and dyn.steps_done == 6
    assert float(b.meta_energies[[0, 1, 3]].min()) > 0.0 and float(b.meta_energies[[2, 4, 5]].abs().max()) == 0.0


def test_step_and_observables_do_not_synchronize(dev):
    from torchani_amd import md

    model, sp, x, mass = _ani_replicas(dev)
    T = torch.full((6,), 300.0, dtype=torch.float64)
    dyn = md.BatchedDynamics(model, sp, x, masses=mass, temperature=T, seed=1, bias=_ani_bias(md, sp))
    dyn.set_temperature(T)
    for _ in range(3):   # (the third evaluation captures the automatic HIP graph)
        dyn.step()
    values = torch.tensor([[2.0, 3.0], [2.5, 4.0]], dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(4):   # deposits after steps 4 and 6
            dyn.step()
        dyn.collective_variables(), dyn.hills(), dyn.metadynamics_bias(values, list=1), dyn.free_energies(values)
        dyn.total_energies(), dyn.bias_energies.sum()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert dyn.steps_done == 7 and dyn._bias.counts == [6, 3] and int(dyn._bias.site_status.abs().max()) == 0


def test_without_sites_the_parent_path_runs_bit_for_bit(dev, monkeypatch):
    """A bias without sites, and bias=None, against a dynamics built the way the tables were built before there were sites:
    ``build_bias_tables`` on the species and a ``DeviceBias`` without site tables.  Nothing new is allocated or launched."""
    from torchani_amd import md, md_bias

    lj, sp, x, mass = _lj_replicas(dev)
    plain = [md.Restraint(md.distance(0, 7), torch.linspace(1.0, 1.4, 5, dtype=torch.float64), 0.05),
             md.Metadynamics(md.angle(0, 1, 2), 0.1, 1e-4, 2)]
    kw = dict(dt=1.0, masses=mass, temperature=120.0, friction=0.05, seed=SEED)
    new = [md.BatchedDynamics(lj, sp, x, bias=plain, **kw), md.BatchedDynamics(lj, sp, x, bias=None, **kw)]
    monkeypatch.setattr(md, "build_site_tables", lambda species, fixed, bias, temperature=None, **_: (
        None, md_bias.build_bias_tables(species, fixed, bias, temperature)))
    old = [md.BatchedDynamics(lj, sp, x, bias=plain, **kw), md.BatchedDynamics(lj, sp, x, **kw)]
    assert new[0]._bias.sites is None and not hasattr(new[0]._bias, "forces_ext") and new[1]._bias is None
    for d in new + old:
        d.set_temperature(120.0)
        d.run(8)
    for a, b in zip(new, old):
        for name in ("coordinates", "coordinates_lo", "velocities", "forces", "potential_energies", "bias_energies"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(new[0].hills()[0], old[0].hills()[0]) and float(new[0].bias_energies.min()) > 0.0


def test_replica_exchange_takes_potential_plus_bias_of_a_centre_restraint(dev):
    """In lock-step with the reference ladders of the replica-exchange tests, fed potential + bias energies."""
    from torchani_amd import md

    lj, sp, x, mass = _lj_replicas(dev)
    T = md.temperature_ladder(60.0, 240.0, 5)
    center = torch.tensor([1.0, 1.3, 0.9, 1.5, 1.1], dtype=torch.float64)
    com, _ = _lj_bias(md)
    dyn = md.ReplicaExchangeDynamics(lj, sp, x, dt=1.0, masses=mass, temperature=T, friction=0.02, exchange_every=2, seed=7,
                                     bias=[md.Restraint(com, center, 0.3)])
    dyn.set_temperature(T)
    assert dyn._bias.sites.max_sites == 2
    lad = rx.Ladders(np.arange(5)[None], ref.KB_HARTREE * dyn.rung_temperatures.cpu().numpy(), 5)
    accepted = differs = 0
    for s in range(8):
        dyn.step()
        if (s + 1) % 2:
            continue
        n = (s + 1) // 2 - 1
        both = (dyn.potential_energies + dyn.bias_energies).cpu().numpy()
        accepted += lad.attempt(n, dyn.seed, both)
        assert lad.margin >= 1e-6, lad.margin
        assert np.array_equal(dyn.replicas_at_rungs().cpu().numpy(), lad.slot)
        assert np.array_equal(dyn.exchange_accepts.cpu().numpy(), lad.accepts)
        differs = max(differs, np.abs(np.diff(dyn.bias_energies.cpu().numpy())).max())
    assert differs > 1e-4, "the restraint energies must matter to the decisions"
    print(f"md sites, replica exchange with a COM-distance restraint, LJ cube x 5: {accepted} swaps accepted in 4 attempts, bias "
          f"energies of neighbors up to {differs:.1e} Ha apart")
