"""Phonons on the MI355X (torchani_amd.phonons): anihip_phonon_fold, anihip_phonon_dynmat and anihip_phonon_dos entry by entry
against the fp64 numpy restatement of tests/_phonon_ref.py on hand-built block Hessians, the closed-form lattices (which also
decide the default eigensolver), the acoustic sum rule, ANI-2x supercells against their own dense Hessians, the refusal of a
general q on a narrow supercell, determinism, and that the first-order and Hessian calls launch none of the new kernels.

Measured on an MI355X (profiles/phonons_tests.txt): see the figures quoted in DESIGN 8.4."""
import os

import numpy as np
import pytest
import torch

import _phonon_ref as ref
from _util import load_golden, seeded_state

pytestmark = pytest.mark.gpu

REPORT = os.environ.get("TORCHANI_AMD_PHONON_REPORT")
NOISE = 1e-4          # relative fp32 noise per block of the hand-built Hessians: every cell differs
HESSIAN_GATE = 2e-5   # the project's per-entry gate of fp32 Hessian blocks against fp64, of max |H|


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


# ---- hand-built Hessians -------------------------------------------------------------------------------------------------------
def _edge_springs(n):
    """Atoms 0, 1, 2 of a 65-atom basis coupled to 62, 63 and 64 others: columns of 63, 64 and 65 blocks."""
    rs = np.random.RandomState(17)
    out = []

    def sym():
        k = rs.uniform(-1, 1, (3, 3))
        return 0.5 * (k + k.T) + np.eye(3)

    zero, one = np.zeros(3, dtype=np.int64), np.array([1, 0, 0])
    for b, extra in ((0, 0), (1, 1), (2, 2)):
        out += [(b, bp, zero, sym()) for bp in range(3, n)]
        out += [(b, 3 + e, one, sym()) for e in range(extra)]
    out += [(b, bp, nv, K) for b, bp, nv, K in ref.random_springs(23, n, per_atom=1) if b > 2 and bp > 2]
    return out


CASES = {
    # name: (n, repeats, springs, noise)
    "isolated": (1, (1, 1, 1), lambda: ref.random_springs(1, 1), NOISE),
    "aliased_n2": (2, (2, 1, 3), lambda: ref.random_springs(2, 2), NOISE),
    "edges_n65": (65, (2, 1, 3), lambda: _edge_springs(65), NOISE),
    "hub_n65": (65, (3, 3, 3), lambda: ref.random_springs(4, 65, per_atom=2, hub=(0, 300)), NOISE),
    "n1": (1, (3, 3, 3), lambda: ref.random_springs(5, 1, per_atom=5), NOISE),
    "n3": (3, (3, 3, 3), lambda: ref.random_springs(6, 3), NOISE),
    "n3_clean": (3, (3, 3, 3), lambda: ref.random_springs(6, 3), 0.0),
}
_BUILT = {}


def _built(name, dev, delete=False):
    """dict of the numpy model (tau, a, masses, index, blocks32) and its device twins (hessian, supercell, masses_t)."""
    key = (name, delete)
    if key in _BUILT:
        return _BUILT[key]
    from torchani_amd import phonons
    from torchani_amd.tuples import BlockHessian

    n, repeats, springs, noise = CASES[name]
    tau, a, masses = ref.random_crystal(len(name), n)
    index, blocks = ref.spring_blocks(n, repeats, springs())
    rs = np.random.RandomState(31)
    blocks32 = (blocks * (1.0 + noise * rs.standard_normal(blocks.shape))).astype(np.float32)
    N = n * int(np.prod(repeats))
    deleted = None
    if delete:   # one pair (i, j), (j, i) between different basis atoms, neither in the home cell (whose columns are the pattern)
        cand = np.nonzero((index[1] // n == 5) & (index[0] // n != 0) & (index[0] % n != index[1] % n))[0]
        i, j = index[0][cand[0]], index[1][cand[0]]
        keep = ~(((index[0] == i) & (index[1] == j)) | ((index[0] == j) & (index[1] == i)))
        assert keep.sum() == len(keep) - 2
        index, blocks32, deleted = index[:, keep], blocks32[keep], (int(i), int(j))
    H = BlockHessian(torch.from_numpy(index).to(dev), torch.from_numpy(blocks32).to(dev), 1, N)
    sc = phonons.supercell(torch.zeros((1, n), dtype=torch.int64, device=dev), torch.from_numpy(tau).to(dev).unsqueeze(0),
                           torch.from_numpy(a).to(dev), repeats)
    out = dict(n=n, repeats=repeats, tau=tau, a=a, masses=masses, index=index, blocks32=blocks32, hessian=H, supercell=sc,
               masses_t=torch.from_numpy(masses).to(dev), deleted=deleted, N=N)
    _BUILT[key] = out
    return out


def _fc(name, dev, asr=True, delete=False, reach=None):
    from torchani_amd import phonons

    c = _built(name, dev, delete)
    return phonons.force_constants_from_hessian(c["hessian"], c["supercell"], c["masses_t"], acoustic_sum_rule=asr, reach=reach)


_REF = {}


def _ref(name, dev, asr=True, delete=False):
    key = (name, asr, delete)
    if key not in _REF:
        c = _built(name, dev, delete)
        _REF[key] = ref.compact_from_blocks(c["index"], c["blocks32"], c["tau"], c["a"], c["repeats"], asr=asr)
    return _REF[key]


@pytest.mark.parametrize("name,asr,delete", [("isolated", True, False), ("aliased_n2", False, False), ("aliased_n2", True, False),
                                             ("edges_n65", True, False), ("hub_n65", False, False), ("hub_n65", True, True),
                                             ("n1", True, False), ("n3", False, False)])
def test_fold_entry_by_entry(dev, name, asr, delete):
    from torchani_amd import phonons
    from torchani_amd.engine import block_hessian_prepare, phonon_fold

    c, want = _built(name, dev, delete), _ref(name, dev, asr, delete)
    n, N = c["n"], c["N"]
    col_len = np.bincount(c["index"][1], minlength=N)
    if name == "isolated":
        assert col_len.tolist() == [1]
    if name == "edges_n65":
        assert col_len[:3].tolist() == [63, 64, 65]
    if name == "hub_n65":
        assert col_len.max() > 256
    fc = _fc(name, dev, asr, delete)
    for got, key in ((fc.ent_b, "ent_b"), (fc.ent_bp, "ent_bp"), (fc.nvec, "nvec"), (fc.boff, "boff"), (fc.poff, "poff")):
        assert np.array_equal(got.cpu().numpy().astype(np.int64), want[key]), key
    assert np.allclose(fc.rvec.cpu().numpy(), want["rvec"], rtol=0, atol=1e-13)
    scale = np.abs(want["phi"]).max() if want["phi"].size and np.abs(want["phi"]).max() > 0 else 1.0
    err = np.abs(fc.phi.cpu().numpy() - want["phi"]).max()
    # the kernel's own missing and defect vectors, through the engine wrapper
    H = c["hessian"]
    op = block_hessian_prepare(H.index, H.blocks, torch.ones(N, dtype=torch.float64, device=dev))
    eb, ej, boff, poff, diag = phonons._compact_pattern(H.index, n, N)
    assert np.array_equal(diag.cpu().numpy().astype(np.int64), want["diag"])
    phi, missing, defect = phonon_fold(op, n, c["repeats"], eb.int().contiguous(), ej.int().contiguous(),
                                       *((boff, diag) if asr else (None, None)))
    assert torch.equal(phi, fc.phi)
    derr = np.abs(defect.cpu().numpy() - want["defect"]).max()
    report(f"fold {name} asr={asr} delete={delete}: {N} atoms, {len(want['ent_b'])} entries, longest column {col_len.max()}, "
           f"max |Phi - ref| {err / scale:.1e}, max |defect - ref| {derr / scale:.1e} of max |Phi|; missing {int(missing.sum())}")
    assert err <= 1e-13 * scale and derr <= 1e-13 * scale
    assert np.array_equal(missing.cpu().numpy().astype(np.int64), want["missing"])
    assert fc.n_missing == int(want["missing"].sum())
    pmax = np.abs(want["phi"]).max()
    assert abs(fc.translation_defect - (want["defect"].max() / pmax if pmax > 0 else 0.0)) <= 1e-12
    if delete:
        i, j = c["deleted"]
        hit = np.nonzero(((want["ent_b"] == i % n) & (want["ent_bp"] == j % n)) | ((want["ent_b"] == j % n) & (want["ent_bp"] == i % n)))[0]
        assert fc.n_missing == 2 and sorted(want["missing"][hit].tolist())[-2:] == [1, 1] and want["missing"].max() == 1
        # the mean counts the missing block as zero: it is (N_c - 1) / N_c of the mean over the stored ones, to the noise
        full = _ref(name, dev, False, False)
        e = np.nonzero(want["missing"] == 1)[0][0]
        nc = int(np.prod(c["repeats"]))
        if not asr or want["diag"][want["ent_b"][e]] != e:
            assert np.abs(want["phi"][e] * nc / (nc - 1) - full["phi"][e]).max() <= 10 * NOISE * np.abs(full["phi"][e]).max()
    else:
        assert fc.n_missing == 0


def _q_set(Q, seed=0):
    q = np.random.RandomState(seed).uniform(-0.5, 0.5, (Q, 3))
    out = np.array([1.3, -2.7, 0.4])          # outside the first zone
    if Q == 1:
        q[0] = out
    else:
        q[0], q[1], q[2 % Q] = 0.0, out, -out
        if Q == 2:
            q[0] = -out
    return q


@pytest.mark.parametrize("name", ["n1", "n3", "hub_n65"])
def test_dynmat_and_derivatives_entry_by_entry(dev, name):
    from torchani_amd import phonons

    c, want = _built(name, dev), _ref(name, dev)
    fc = _fc(name, dev, reach=0.0)            # (hand-built: general q is the point here, so the supercell is declared exact)
    phi = fc.phi.cpu().numpy()
    assert fc.exact
    for Q in (1, 63, 64, 65, 257):
        q = _q_set(Q, seed=Q)
        D, dD = phonons.dynamical_matrices(fc, torch.from_numpy(q).to(dev), derivatives=True)
        assert D.dtype == torch.complex128 and D.shape == (Q, 3 * c["n"], 3 * c["n"]) and dD.shape == (Q, 3, 3 * c["n"], 3 * c["n"])
        Dr, dDr = ref.dynmat(phi, want["nvec"], want["ent_b"], want["ent_bp"], c["masses"], q, want["rvec"])
        D, dD = D.cpu().numpy(), dD.cpu().numpy()
        g, gd = ref.gershgorin(Dr), ref.gershgorin(dDr)
        err, derr = np.abs(D - Dr).max() / g, np.abs(dD - dDr).max() / gd
        herm = np.abs(D - D.conj().transpose(0, 2, 1)).max() / g
        hermd = np.abs(dD - dD.conj().transpose(0, 1, 3, 2)).max() / gd
        report(f"dynmat {name} Q={Q}: max |D - ref| {err:.1e}, |dD - ref| {derr:.1e}, |D - D^H| {herm:.1e}, |dD - dD^H| {hermd:.1e} "
               "of the Gershgorin row sums")
        assert err <= 1e-12 and derr <= 1e-12 and herm <= 1e-12 and hermd <= 1e-12
        only = phonons.dynamical_matrices(fc, torch.from_numpy(q).to(dev))
        assert np.array_equal(only.cpu().numpy(), D)                      # the kernel without derivatives: the same bits
        if Q >= 3:                                                        # D(-q) = conj D(q), and Gamma is real
            assert np.abs(D[2] - D[1].conj()).max() <= 1e-12 * g and np.abs(D[0].imag).max() == 0.0
    # D(q + G) = D(q)
    q = _q_set(65, seed=3)
    G = np.array([2.0, -1.0, 3.0])
    a_ = phonons.dynamical_matrices(fc, torch.from_numpy(q).to(dev)).cpu().numpy()
    b_ = phonons.dynamical_matrices(fc, torch.from_numpy(q + G).to(dev)).cpu().numpy()
    assert np.abs(a_ - b_).max() <= 1e-12 * ref.gershgorin(a_)


# ---- closed forms: these also decide the default eigensolver ---------------------------------------------------------------------
K_CUBIC = ((1.0, 0.3125, 0.1875), (0.25, 0.90625, 0.15625), (0.109375, 0.34375, 0.796875))   # exact in fp32, sums included


def _closed_form_fc(dev, which):
    from torchani_amd import phonons
    from torchani_amd.tuples import BlockHessian

    if which == "cubic":
        tau, a, masses, springs, k = ref.cubic_lattice(k=K_CUBIC)
        repeats, reach = (3, 3, 3), 2.5
    else:
        tau, a, masses, springs = ref.diatomic_chain(k=0.75)
        repeats, reach, k = (4, 1, 1), 1.5, None
    n = len(tau)
    index, blocks = ref.spring_blocks(n, repeats, springs)
    assert np.array_equal(blocks.astype(np.float32).astype(np.float64), blocks)
    H = BlockHessian(torch.from_numpy(index).to(dev), torch.from_numpy(blocks.astype(np.float32)).to(dev), 1, n * int(np.prod(repeats)))
    sc = phonons.supercell(torch.zeros((1, n), dtype=torch.int64, device=dev), torch.from_numpy(tau).to(dev).unsqueeze(0),
                           torch.from_numpy(a).to(dev), repeats)
    fc = phonons.force_constants_from_hessian(H, sc, torch.from_numpy(masses).to(dev), reach=reach)
    assert fc.exact and fc.n_missing == 0 and fc.translation_defect == 0.0
    return fc, a, masses, k


@pytest.mark.parametrize("eigensolver", ["device", "host"])
def test_cubic_lattice_closed_form(dev, eigensolver):
    from torchani_amd import phonons, units

    fc, a, masses, k = _closed_form_fc(dev, "cubic")
    q = np.random.RandomState(7).uniform(-0.5, 0.5, (33, 3))              # generic: not commensurate with (3, 3, 3)
    md = phonons.modes(fc, torch.from_numpy(q).to(dev), group_velocities=True, eigenvectors=True, eigensolver=eigensolver)
    lam, dlam = ref.cubic_closed_form(q, a[0, 0], masses[0], k)
    order = np.argsort(lam, axis=1)
    lam = np.take_along_axis(lam, order, axis=1)
    dlam = np.take_along_axis(dlam, order[:, :, None], axis=1)
    gap = np.diff(lam, axis=1).min()
    assert gap > 1e-3 * lam.max()                                         # no degenerate set: every velocity is defined
    freq = units.sqrt_mhessian2invcm(np.sqrt(lam) / (2 * np.pi))
    vel = ref.SQRT_MHESSIAN_TO_RAD_PER_FS * dlam / (2.0 * np.sqrt(lam))[:, :, None]
    ef = np.abs(md.frequencies.cpu().numpy() - freq).max() / freq.max()
    ev = np.abs(md.group_velocities.cpu().numpy() - vel).max() / np.abs(vel).max()
    report(f"cubic lattice, eigh on the {eigensolver}: max frequency error {ef:.1e}, group velocity error {ev:.1e} (relative to "
           f"the largest; {freq.max():.1f} cm^-1, {np.abs(vel).max():.2e} A/fs)")
    assert md.frequencies.shape == (33, 3) and md.group_velocities.shape == (33, 3, 3) and md.eigenvectors.dtype == torch.complex128
    assert ef <= 1e-9 and ev <= 1e-9
    gamma = phonons.modes(fc, [[0.0, 0.0, 0.0], [0.5, 0.5, 0.5]], group_velocities=True, eigensolver=eigensolver)
    assert gamma.eigenvalues[0].abs().max().item() <= 1e-14 and gamma.group_velocities[0].abs().max().item() == 0.0
    assert gamma.group_velocities[1].abs().max().item() <= 1e-12 * np.abs(vel).max()   # zone corner: sin(pi) = 0


@pytest.mark.parametrize("eigensolver", ["device", "host"])
def test_diatomic_chain_closed_form(dev, eigensolver):
    from torchani_amd import phonons, units

    fc, a, masses, _ = _closed_form_fc(dev, "chain")
    q = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.237, 0.41, -0.3], [0.5, 0.0, 0.0], [-0.37, 0.2, 0.1]])
    md = phonons.modes(fc, torch.from_numpy(q).to(dev), eigensolver=eigensolver)
    lo, hi = ref.chain_closed_form(q[:, 0], masses[0], masses[1], 0.75)
    lam, f = md.eigenvalues.cpu().numpy(), md.frequencies.cpu().numpy()
    to = lambda x: units.sqrt_mhessian2invcm(np.sqrt(x) / (2 * np.pi))   # noqa: E731
    assert np.abs(lam[:, :4]).max() <= 1e-14 * hi.max() and abs(lam[0, 4]) <= 1e-14 * hi.max()      # y, z rows; acoustic at Gamma
    ea = np.abs(f[1:, 4] - to(lo[1:])).max() / to(hi).max()
    eo = np.abs(f[:, 5] - to(hi)).max() / to(hi).max()
    report(f"diatomic chain, eigh on the {eigensolver}: acoustic branch error {ea:.1e}, optical {eo:.1e} of the largest frequency")
    assert ea <= 1e-9 and eo <= 1e-9


def test_acoustic_sum_rule(dev):
    from torchani_amd import phonons

    for name in ("n3", "hub_n65"):
        on, off = _fc(name, dev, asr=True, reach=0.0), _fc(name, dev, asr=False, reach=0.0)
        D = phonons.dynamical_matrices(on, [[0.0, 0.0, 0.0]])
        g = ref.gershgorin(D.cpu().numpy())
        low_on = np.sort(np.abs(np.linalg.eigvalsh(D[0].cpu().numpy())))[:3]
        low_off = np.sort(np.abs(np.linalg.eigvalsh(phonons.dynamical_matrices(off, [[0.0, 0.0, 0.0]])[0].cpu().numpy())))[:3]
        report(f"acoustic sum rule {name}: three lowest |eigenvalues| at Gamma {low_on.max() / g:.1e} with, {low_off.max() / g:.1e} "
               "without, of the Gershgorin bound")
        assert low_on.max() <= 1e-10 * g and low_off.max() > 1e-10 * g
        # the rule touches the diagonal entries alone
        d = on.boff.new_tensor(_ref(name, dev)["diag"]).long()
        mask = torch.ones(on.phi.shape[0], dtype=torch.bool, device=dev)
        mask[d] = False
        assert torch.equal(on.phi[mask], off.phi[mask]) and not torch.equal(on.phi[d], off.phi[d])


# ---- a real model ----------------------------------------------------------------------------------------------------------------
_REAL = {}


def _water(dev, repeats):
    """(ForceConstants without the sum rule, BlockHessian, masses [N] fp64 numpy, supercell) of the water fixture."""
    if repeats in _REAL:
        return _REAL[repeats]
    from torchani_amd import grad, phonons
    from torchani_amd.extras.io import PERIODIC_TABLE
    from torchani_amd.models import ANI2x
    from torchani_amd.utils import atomic_numbers_to_masses

    g = load_golden("water_pbc_ani2x")
    if "model" not in _REAL:
        _REAL["model"] = ANI2x(state_dict=seeded_state("ani2x", 8, g["seed"]), device=dev, periodic_table_index=False,
                               cutoff_fn=g["cutoff_fn"], row_capacity=256)
    model = _REAL["model"]
    sp = torch.from_numpy(g["species"].astype(np.int64)).to(dev)
    x = torch.from_numpy(g["coords"]).to(dev)
    cell = torch.from_numpy(g["cell"]).to(dev)
    z = torch.tensor([PERIODIC_TABLE.index(s) for s in g["symbols"]], device=dev)[sp.reshape(-1)]
    masses = atomic_numbers_to_masses(z, dtype=torch.float64)
    sc = phonons.supercell(sp, x, cell, repeats)
    out = grad.energies_forces_and_sparse_hessians(model, sc.species, sc.coordinates, cell=sc.cell,
                                                   pbc=torch.ones(3, dtype=torch.bool, device=dev))
    fc = phonons.force_constants_from_hessian(out.hessians, sc, masses, acoustic_sum_rule=False, reach=2.0 * float(model.cutoff))
    _REAL[repeats] = (fc, out.hessians, masses.cpu().numpy(), sc, (sp, x, cell, out))
    return _REAL[repeats]


def test_ani2x_supercell_spectrum(dev):
    from torchani_amd import phonons

    repeats = (2, 2, 2)
    fc, H, masses, sc, (sp, x, cell, out) = _water(dev, repeats)
    n, N = fc.n_basis, H.n_atoms
    assert N == 240 and not fc.exact
    index, blocks32 = H.index.cpu().numpy(), H.blocks.cpu().numpy()
    want = ref.compact_from_blocks(index, blocks32, sc.primitive_coordinates.cpu().numpy(), sc.primitive_cell.cpu().numpy(), repeats)
    assert len(want["ent_b"]) * 8 == H.nnz                                 # the pattern is the same in every cell
    delta = want["defect"].max()
    pmax = np.abs(want["phi"]).max()
    assert fc.n_missing == 0 and want["missing"].sum() == 0
    assert abs(fc.translation_defect - delta / pmax) <= 1e-10 * delta / pmax
    Hd = H.to_dense()[0].double().cpu().numpy()
    w = 1.0 / np.sqrt(np.repeat(np.tile(masses, 8), 3))
    A = 0.5 * (Hd + Hd.T) * w[:, None] * w[None, :]
    lam_ref = np.linalg.eigvalsh(A)
    md = phonons.modes(fc, torch.from_numpy(ref.commensurate_q(repeats)).to(dev))
    lam = np.sort(md.eigenvalues.cpu().numpy().reshape(-1))
    col = int(np.bincount(index[1]).max())
    gersh = np.abs(A).sum(axis=1).max()
    gate = 3 * col * delta / masses.min() + 1e-12 * gersh
    err = np.abs(lam - lam_ref).max()
    report(f"water (2, 2, 2), 240 atoms: n_missing {fc.n_missing}, translation_defect {fc.translation_defect:.3e} (delta {delta:.3e} "
           f"Ha/A^2, max |Phi| {pmax:.3f}); max |eigenvalue(D(q)) - eigenvalue(dense)| {err:.3e} against the Weyl gate {gate:.3e} "
           f"(longest column {col}, ||A||_G {gersh:.3f})")
    assert err <= gate
    # the one-call entry gives the same force constants up to the sum rule, and the supercell's energy and largest force
    full = phonons.force_constants(_REAL["model"], sp, x, cell, repeats, acoustic_sum_rule=False)
    assert np.abs(full.phi.cpu().numpy() - fc.phi.cpu().numpy()).max() <= 2 * HESSIAN_GATE * np.abs(blocks32).max()
    assert torch.equal(full.masses.cpu(), torch.from_numpy(masses[:n])) and torch.equal(full.nvec, fc.nvec)
    assert abs(full.energy.item() - out.energies.item()) <= 1e-9 * abs(out.energies.item())
    assert abs(full.max_force.item() - out.forces.abs().max().item()) <= 1e-4 * out.forces.abs().max().item()
    # a narrow supercell: commensurate q pass, general q raise unless waived
    phonons.modes(fc, [[0.5, 0.0, 0.0]])
    with pytest.raises(ValueError, match="exact only at q commensurate"):
        phonons.modes(fc, [[0.3, 0.0, 0.0]])
    phonons.modes(fc, [[0.3, 0.0, 0.0]], allow_aliasing=True)


def test_ani2x_general_q(dev):
    from torchani_amd import phonons

    big, Hb, masses, _, _ = _water(dev, (3, 3, 3))
    small, _, _, _, _ = _water(dev, (2, 1, 1))
    assert Hb.n_atoms == 810 and big.exact and not small.exact and big.n_missing == 0 and small.n_missing == 0
    assert not bool(phonons.is_commensurate(torch.tensor([[0.5, 0.0, 0.0]]), (3, 3, 3)).all())
    q = torch.tensor([[0.5, 0.0, 0.0]], dtype=torch.float64, device=dev)
    a, b = phonons.modes(big, q), phonons.modes(small, q)
    hmax = Hb.blocks.abs().max().item()
    col = int(torch.bincount(Hb.index[1]).max())
    gate = 2 * HESSIAN_GATE * hmax * 3 * col / masses.min()
    err = (a.eigenvalues - b.eigenvalues).abs().max().item()
    ferr = (a.frequencies - b.frequencies).abs().max().item()
    report(f"water q = (1/2, 0, 0): (3, 3, 3) (810 atoms, general q) against (2, 1, 1) (commensurate): max eigenvalue deviation "
           f"{err:.3e} = {err / gate:.2e} x the Weyl gate {gate:.3e} (max |H| {hmax:.3f}, longest column {col}); max frequency "
           f"deviation {ferr:.3e} cm^-1 of {a.frequencies.abs().max().item():.1f}"
           + ("" if err < 0.1 * gate else "; within 10 x of the gate: the gate is too loose to show a wrong image choice"))
    assert err <= gate


# ---- DOS and thermodynamics --------------------------------------------------------------------------------------------------------
def test_dos_and_thermodynamics(dev):
    from torchani_amd import phonons

    fc = _fc("n3", dev, reach=0.0)
    pm = phonons.mesh(fc, (4, 4, 3))
    f, w = pm.frequencies.cpu().numpy(), pm.weights.cpu().numpy()
    assert f.shape == (len(w), 9) and abs(w.sum() - 1.0) < 1e-14 and pm.unit == "cm^-1"
    lo, hi = f.min(), f.max()
    sigma = (hi - lo) / 40.0
    bins = 3 * 52
    centres, g = pm.dos(bins, f_min=lo - 6 * sigma, f_max=hi + 6 * sigma, sigma=sigma)
    df = (hi - lo + 12 * sigma) / bins
    fk, want = ref.dos(f, w, lo - 6 * sigma + 0.5 * df, df, sigma, bins)
    err = np.abs(g.cpu().numpy() - want).max() / want.max()
    integral = float(g.sum().item() * df)
    report(f"dos: {f.size} modes, {bins} bins, max |g - ref| {err:.1e} of max g; integral {integral:.12f} for 3 n = 9")
    assert np.abs(centres.cpu().numpy() - fk).max() <= 1e-12 * hi and err <= 1e-12
    assert abs(integral - 9.0) <= 1e-8 * 9.0
    again = pm.dos(bins, f_min=lo - 6 * sigma, f_max=hi + 6 * sigma, sigma=sigma)[1]
    assert torch.equal(again, g)
    d2 = pm.dos(64)                                                      # the defaults: from 0 to 1.05 max f, sigma two bins
    assert d2[0].shape == (64,) and abs(d2[0][0].item() - 0.5 * 1.05 * hi / 64) <= 1e-12 * hi
    T = [10.0, 300.0, 1000.0]
    th = pm.thermodynamics(T)
    z, F, S, Cv, nim = ref.thermodynamics(pm.eigenvalues.cpu().numpy(), w, T)
    assert th.n_imaginary == nim and abs(th.zero_point_energy.item() - z) <= 1e-13 * z
    for got, ref_ in ((th.free_energy, F), (th.entropy, S), (th.heat_capacity, Cv)):
        assert np.allclose(got.cpu().numpy(), ref_, rtol=1e-11, atol=0)


# ---- determinism and isolation -------------------------------------------------------------------------------------------------------
def test_bit_identical_across_calls(dev):
    from torchani_amd import phonons

    a, b = _fc("hub_n65", dev, reach=0.0), _fc("hub_n65", dev, reach=0.0)
    assert torch.equal(a.phi, b.phi) and a.translation_defect == b.translation_defect
    q = torch.from_numpy(_q_set(257, seed=9)).to(dev)
    D1, dD1 = phonons.dynamical_matrices(a, q, derivatives=True)
    D2, dD2 = phonons.dynamical_matrices(b, q, derivatives=True)
    assert torch.equal(torch.view_as_real(D1), torch.view_as_real(D2)) and torch.equal(torch.view_as_real(dD1), torch.view_as_real(dD2))


def test_first_order_and_hessian_calls_launch_no_phonon_kernels(dev, monkeypatch):
    from torchani_amd import engine, grad, phonons

    calls = {}

    def counting(name):
        orig = getattr(engine, name)

        def f(*a, **k):
            calls[name] = calls.get(name, 0) + 1
            return orig(*a, **k)

        monkeypatch.setattr(engine, name, f)

    for name in ("phonon_fold", "phonon_dynmat", "phonon_dos"):
        counting(name)
    from torchani_amd.models import ANI2x

    g = load_golden("water_pbc_ani2x")
    model = ANI2x(state_dict=seeded_state("ani2x", 8, g["seed"]), device=dev, periodic_table_index=False, row_capacity=256)
    sp = torch.from_numpy(g["species"].astype(np.int64)).to(dev)
    x = torch.from_numpy(g["coords"]).to(dev)
    cell = torch.from_numpy(g["cell"]).to(dev)
    pbc = torch.ones(3, dtype=torch.bool, device=dev)
    grad.energies_and_forces(model, sp, x, cell=cell, pbc=pbc)
    grad.energies_forces_and_sparse_hessians(model, sp, x, cell=cell, pbc=pbc)
    assert sum(calls.values()) == 0
    fc = phonons.force_constants(model, sp, x, cell, (1, 1, 1))
    pm = phonons.mesh(fc, (1, 1, 1))
    pm.dos(8)
    assert calls == {"phonon_fold": 1, "phonon_dynmat": 1, "phonon_dos": 1}
