"""Host-side parts of the pair-potential Hessians (no GPU): the C declarations of include/anihip.h against the ctypes
symbol list, which pair potentials the Hessian entry points refuse, and vibrational analysis of the reference's ANI-2xr
Hessian (tests/golden/hess_x2r_vib_ani2xr.npz, gen_golden_hessians_pairs.py)."""
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_exported_symbols():
    from torchani_amd import _lib

    with open(os.path.join(ROOT, "include", "anihip.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(anihip_\w+)\s*\(", src))
    assert "anihip_pair_analytic_hvp" in declared
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    assert len(_lib.EXPORTED_SYMBOLS) == len(set(_lib.EXPORTED_SYMBOLS))
    assert _lib.ABI_VERSION == 13


def test_only_d3_has_no_hessian():
    from torchani_amd import grad
    from torchani_amd import potentials as P

    symbols = ("H", "C", "N", "O")
    pots = torch.nn.ModuleDict({
        "xtb": P.RepulsionXTB(symbols), "zbl": P.RepulsionZBL(symbols), "lj": P.LennardJones(symbols),
        "lj_rep": P.RepulsionLJ(symbols), "lj_disp": P.DispersionLJ(symbols),
        "coulomb": P.FixedCoulomb(symbols, charges=(0.3, -0.1, -0.2, -0.4)),
        "mnok": P.FixedMNOK(symbols, charges=(0.3, -0.1, -0.2, -0.4), eta=(0.5, 0.4, 0.5, 0.5)),
        "d3": P.TwoBodyDispersionD3.from_functional(symbols, "b973c"),
    })

    class Model:
        potentials = pots

    assert grad._pair_potentials_without_hessians(Model()) == ["TwoBodyDispersionD3"]
    pots["d3"]._enabled = False
    assert grad._pair_potentials_without_hessians(Model()) == []
    for name, pot in pots.items():
        want = ["TwoBodyDispersionD3"] if name == "d3" else []
        assert grad._pair_potentials_without_hessians(pot) == want


@pytest.mark.parametrize("mode_kind", ["mdu", "mdn", "mwn"])
def test_vibrational_analysis_of_ani2xr_hessian(mode_kind):
    from torchani_amd.grad import vibrational_analysis

    with np.load(os.path.join(ROOT, "tests", "golden", "hess_x2r_vib_ani2xr.npz")) as z:
        g = {k: z[k] for k in z.files}
    va = vibrational_analysis(torch.from_numpy(g["masses"]), torch.from_numpy(g["hess"]), mode_kind=mode_kind)
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()   # noqa: E731
    assert rel(va.freqs.numpy(), g["freqs_" + mode_kind]) < 1e-8
    assert rel(va.fconstants.numpy(), g["fconstants_" + mode_kind]) < 1e-8
    assert rel(va.rmasses.numpy(), g["rmasses_" + mode_kind]) < 1e-8
    ev = np.sign(g["freqs_" + mode_kind]) * g["freqs_" + mode_kind] ** 2
    gap = np.abs(np.diff(ev))
    checked = 0
    for k in range(ev.size):
        if min(gap[k - 1] if k > 0 else math.inf, gap[k] if k < gap.size else math.inf) < 1e-6 * np.abs(ev).max():
            continue
        m, r = va.modes[k].numpy(), g["modes_" + mode_kind][k]
        assert np.abs(np.sign((m * r).sum()) * m - r).max() < 1e-7 * np.abs(r).max()
        checked += 1
    assert checked >= ev.size // 2
