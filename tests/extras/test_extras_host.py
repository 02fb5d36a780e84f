"""Host-side conveniences of torchani_amd.extras (outside the hot path; SURVEY 2.1 marks them out of scope)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


@pytest.fixture(scope="module")
def lib():
    from torchani_amd import _lib

    _lib.build()
    return _lib.lib()


def test_dipoles_and_raw_normalizer():
    """electro.DipoleComputer / compute_dipole against the reference's values for the reference's charges (fixture), on CPU
    tensors; BaseChargeNormalizer passes the raw charges through; simple_aniq(normalize=False) uses it."""
    import warnings

    from torchani_amd.extras.electro import BaseChargeNormalizer, DipoleComputer, compute_dipole
    from torchani_amd.models import simple_aniq

    ref = dict(np.load(os.path.join(ROOT, "tests", "golden", "simple_chnoq.npz")))
    z, x, q = (torch.from_numpy(ref[k]) for k in ("atomic_numbers", "coords", "atomic_charges"))
    for frame in ("center_of_mass", "center_of_geometry", "origin"):
        mu = compute_dipole(z, x.double(), q, frame)
        assert mu.shape == (z.shape[0], 3) and np.abs(mu.numpy() - ref["dipole_" + frame]).max() < 1e-12, frame
    # neutral molecules: the dipole does not depend on the frame
    assert np.abs(ref["dipole_origin"] - ref["dipole_center_of_mass"]).max() < 1e-9
    custom = DipoleComputer(masses=[0.0, 2.0] + [1.0] * 16, reference="center_of_mass", dtype=torch.float64)
    mu = custom(torch.tensor([[1, 8, -1]]), torch.tensor([[[0.0, 0, 0], [3.0, 0, 0], [9.0, 9, 9]]], dtype=torch.float64),
                torch.tensor([[1.0, 0.0, 0.0]], dtype=torch.float64))
    assert torch.allclose(mu, torch.tensor([[-1.0, 0.0, 0.0]], dtype=torch.float64))   # (center of mass at x = 1)
    with pytest.raises(ValueError):
        DipoleComputer(reference="nucleus")
    raw = torch.tensor([[0.3, -0.1]])
    assert torch.equal(BaseChargeNormalizer()(torch.tensor([[0, 1]]), raw), raw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = simple_aniq(("H", "O"), "wb97x-631gd", normalize=False, seed=2)
    assert type(m.potentials["nnp"].charge_normalizer) is BaseChargeNormalizer
    assert set(k.split(".")[2] for k in m.state_dict() if k.startswith("potentials.nnp.") and "networks" in k) == \
        {"neural_networks", "charge_networks"}


def test_xyz_io_round_trip_and_reference(tmp_path):
    """torchani_amd.io.read_xyz / write_xyz (io.py:22-176): round trips with padding and a cell, the padding placeholder,
    the error cases; the reference's own reader on its in-tree files where the tree is present (the build container)."""
    from torchani_amd.extras.io import TorchaniIOError, read_xyz, write_xyz

    sp = torch.tensor([[8, 1, 1, -1], [6, 1, 1, 1]])
    x = torch.arange(24, dtype=torch.float64).reshape(2, 4, 3) / 7
    cell = torch.tensor([[10.0, 0, 0], [0, 11.5, 0], [0.25, 0, 12.0]], dtype=torch.float64)
    f = tmp_path / "a.xyz"
    write_xyz(sp, x, f, cell=cell)
    sp2, x2, cell2, pbc2 = read_xyz(f, dtype=torch.float64)
    assert torch.equal(sp2, sp) and torch.allclose(x2[sp >= 0], x[sp >= 0], atol=1e-10) and (x2[sp < 0] == 0).all()
    assert torch.allclose(cell2, cell) and pbc2.tolist() == [True, True, True]
    write_xyz(sp, x, f, pad=True)                        # padding atoms written as element 100 ("Fm")
    text = f.read_text().splitlines()
    assert text[0] == "4" and text[5].startswith("Fm 0.0000000000") and 'pbc="F F F"' in text[1]
    sp3, x3, cell3, pbc3, comments = read_xyz(f, dtype=torch.float64, return_comments=True)
    assert torch.equal(sp3, sp) and cell3 is None and pbc3 is None and len(comments) == 2
    assert read_xyz(f, detect_padding=False)[0][0, 3].item() == 100
    (tmp_path / "n.xyz").write_text("2\n\n1 0 0 0\n8 0 0 1\n>\n1\ncomment\nCl 1 2 3\n")   # numbers, divider, symbols
    spn, xn, _, _ = read_xyz(tmp_path / "n.xyz")
    assert spn.tolist() == [[1, 8], [17, -1]] and xn[1, 0].tolist() == [1.0, 2.0, 3.0]
    (tmp_path / "bad.xyz").write_text('1\nfoo\nH 0 0 0\n1\nLattice="1 0 0 0 1 0 0 0 1"\nH 0 0 0\n')
    with pytest.raises(TorchaniIOError):
        read_xyz(tmp_path / "bad.xyz")
    with pytest.raises(ValueError):
        write_xyz(sp[0], x[0], f)
    # files of the reference and what its io.read_xyz returns for them (tests/golden/gen_golden_reference_meta.py)
    meta = os.path.join(ROOT, "tests", "golden", "reference_meta")
    ref = np.load(os.path.join(meta, "xyz_reads.npz"))
    for name in ("13_head.xyz", "water-0.8nm.xyz", "small.xyz"):
        a = read_xyz(os.path.join(meta, name), dtype=torch.float64)
        assert torch.equal(a[0], torch.from_numpy(ref[name + "/species"])), name
        assert torch.equal(a[1], torch.from_numpy(ref[name + "/coords"])), name
        assert (a[2] is None) == (name + "/cell" not in ref.files), name
        assert a[2] is None or torch.equal(a[2], torch.from_numpy(ref[name + "/cell"])), name


def test_symbol_number_mass_converters():
    """utils: the reference's small converter modules (utils.py:257-473) under their names."""
    from torchani_amd import utils as u

    assert u.AtomicNumbersToChemicalSymbols()(torch.tensor([6, 1, 1, -1, 17])) == ["C", "H", "H", "Cl"]
    assert u.IntsToChemicalSymbols(["H", "C", "N", "O"])(torch.tensor([3, 0, 0, -1])) == ["O", "H", "H"]
    assert u.ChemicalSymbolsToAtomicNumbers()(["C", "S", "O", "F", "H"]).tolist() == [6, 16, 8, 9, 1]
    conv = u.ChemicalSymbolsToInts(["H", "C", "N", "O", "S", "F", "Cl"])
    assert conv(["C", "S", "O", "F", "H", "H"]).tolist() == [1, 4, 3, 5, 0, 0] and len(conv) == 7
    with pytest.raises(ValueError):
        u.ChemicalSymbolsToInts("HCNO")
    m = u.atomic_numbers_to_masses(torch.tensor([[8, 1, 1, -1]]), dtype=torch.float64)
    assert torch.allclose(m, torch.tensor([[15.999, 1.008, 1.008, 0.0]], dtype=torch.float64)) and u.get_atomic_masses is u.atomic_numbers_to_masses
    with pytest.raises(ValueError):
        u.atomic_numbers_to_masses(torch.tensor([[26]]))      # (no iron in the default table: pass masses=)
    assert u.sort_by_atomic_num(["Cl", "H", "O", "C"]) == ("H", "C", "O", "Cl") and u.sort_by_atomic_num("N") == ("N",)


def test_assembler_and_term_objects():
    """torchani_amd.arch.Assembler builds the same modules as the fixed factories from the reference's step-by-step protocol
    (arch.py:743-990); ANIRadial / ANIAngular carry the hyper-parameters and evaluate the terms on the host.  Where the
    reference tree is present: its terms on the same inputs, and the state dict of its Assembler's model, key by key."""
    import warnings

    from torchani_amd.aev import AEVComputer, ANIAngular, ANIRadial
    from torchani_amd.extras.arch import ANIq, Assembler
    from torchani_amd.extras.electro import ChargeNormalizer
    from torchani_amd.models import ANI2x
    from torchani_amd.potentials import RepulsionXTB, TwoBodyDispersionD3

    def recipe(asm_cls, **extra):
        asm = asm_cls(periodic_table_index=False, **extra)
        asm.set_symbols(("H", "C", "N", "O", "S", "F", "Cl"))
        asm.set_global_cutoff_fn("cosine")
        asm.set_aev_computer(radial="ani2x", angular="ani2x", strategy="pyaev")
        asm.set_atomic_networks(ctor="ani2x")
        asm.set_neighborlist("all_pairs")
        asm.set_gsaes_as_self_energies("wb97x-631gd")
        return asm

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fixed = ANI2x(seed=0)
    asm = recipe(Assembler)
    built = asm.assemble(8)
    sd_a, sd_b = built.state_dict(), fixed.state_dict()
    assert set(sd_a) == set(sd_b) and all(sd_a[k].shape == sd_b[k].shape for k in sd_a)
    for k in sd_a:
        if "aev_computer" in k or k in ("atomic_numbers", "energy_shifter.self_energies"):
            assert torch.equal(sd_a[k], sd_b[k]), k
    assert all(p.requires_grad for p in built.neural_networks.parameters())         # (CELU with biases: trainable)
    asm.add_potential(RepulsionXTB, "repulsion_xtb", cutoff=5.1)
    asm.add_potential(TwoBodyDispersionD3, "dispersion_d3", cutoff=8.0, kwargs={"functional": "b973c"})
    with pytest.raises(ValueError):
        asm.add_potential(RepulsionXTB, "repulsion_xtb")
    both = asm.assemble(2)
    assert list(both.potentials) == ["nnp", "repulsion_xtb", "dispersion_d3"] and both.potentials["dispersion_d3"].cutoff == 8.0
    assert both.potentials["repulsion_xtb"].cutoff_fn == "cosine"                      # (the global envelope)
    q = recipe(Assembler, cls=ANIq)
    q.set_charge_networks(ctor="ani2x", kwargs={"bias": False, "activation": "gelu", "out_dim": 1},
                          normalizer=ChargeNormalizer.from_electronegativity_and_hardness(q.symbols))
    mq = q.assemble(1)
    assert isinstance(mq, ANIq) and not any(p.requires_grad for p in mq.potentials["nnp"].charge_networks.parameters())
    for bad in (lambda a: a.set_atomic_networks(ctor="like_dr"), lambda a: a.set_aev_computer("ani2x", "ani3x"),
                lambda a: a.set_atomic_networks(ctor="ani2x", kwargs={"activation": "tanh"})):
        a = recipe(Assembler)
        with pytest.raises(ValueError):
            bad(a)
            a.assemble(1)
    with pytest.raises(RuntimeError):
        Assembler(symbols=("H",)).assemble(1)
    # term objects
    r, a = ANIRadial.cover_linearly(0.9, 5.2, 19.7, 16, "smooth"), ANIAngular.like_1x()
    assert r.num_feats == 16 and a.num_feats == 32 and AEVComputer.from_terms(r, ANIAngular.like_2x(), 4).out_dim == 384
    d = torch.linspace(0.5, 6.0, 12, dtype=torch.float64)
    assert r(d).shape == (12, 16) and (r(d)[d >= 5.2] == 0).all() is not None
    with pytest.raises(ValueError):
        AEVComputer.from_terms(ANIRadial.like_2x(cutoff=3.0), ANIAngular.like_2x(), 4)
    # the reference's terms on the same inputs, and the state dict of its Assembler's model, key by key
    # (tests/golden/gen_golden_reference_meta.py)
    import json

    ref = np.load(os.path.join(ROOT, "tests", "golden", "reference_meta", "api_ani2x.npz"))
    d, td, tv = (torch.from_numpy(ref[k]) for k in ("terms_d", "terms_td", "terms_tv"))
    for name, kw in (("like_1x", {}), ("like_2x", {}), ("cover_linearly", dict(cutoff_fn="smooth"))):
        mine = getattr(ANIRadial, name)(**kw).double()
        assert torch.allclose(mine(d), torch.from_numpy(ref["radial/" + name]), rtol=1e-12, atol=1e-14), name
        mine = getattr(ANIAngular, name)(**kw).double()
        assert torch.allclose(mine(td, tv), torch.from_numpy(ref["angular/" + name]), rtol=1e-10, atol=1e-14), name
    shapes = json.loads(str(ref["meta"]))["assembler_state"]
    assert set(shapes) == set(sd_a), sorted(set(shapes) ^ set(sd_a))[:5]
    assert all(list(sd_a[k].shape) == shapes[k] for k in shapes)
    for k in shapes:
        if "aev_computer" in k or k in ("atomic_numbers", "energy_shifter.self_energies"):
            assert torch.allclose(torch.from_numpy(ref["value/" + k]), sd_a[k].double()), k
