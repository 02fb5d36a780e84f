"""Host-side parts of the Hessian feature (no GPU): vibrational analysis and unit conversions against the reference's own
outputs (tests/golden/hess_*.npz, gen_golden_hessians.py), and the chunk-size rule of grad.energies_forces_and_hessians."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VIB_BASES = ("ch4_ani1x", "triclinic_pbc_ani2x")


def _load(base):
    with np.load(os.path.join(GOLDEN, "hess_" + base + ".npz")) as z:
        return {k: z[k] for k in z.files}


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("base", VIB_BASES)
@pytest.mark.parametrize("mode_kind", ["mdu", "mdn", "mwn"])
@pytest.mark.parametrize("unit", ["cm^-1", "meV"])
def test_vibrational_analysis_matches_reference(base, mode_kind, unit):
    from torchani_amd.grad import vibrational_analysis

    g = _load(base)
    tag = f"{mode_kind}_{'invcm' if unit == 'cm^-1' else 'mev'}"
    va = vibrational_analysis(torch.from_numpy(g["masses"]), torch.from_numpy(g["hess"]), mode_kind=mode_kind, unit=unit)
    assert _rel(va.freqs.numpy(), g["freqs_" + tag]) < 1e-8
    assert _rel(va.fconstants.numpy(), g["fconstants_" + tag]) < 1e-8
    assert _rel(va.rmasses.numpy(), g["rmasses_" + tag]) < 1e-8
    # modes up to sign, wherever the eigenvalue is non-degenerate
    ev = np.sign(g["freqs_" + tag]) * g["freqs_" + tag] ** 2
    modes, ref = va.modes.numpy(), g["modes_" + tag]
    assert modes.shape == ref.shape
    gap = np.abs(np.diff(ev))
    scale = np.abs(ev).max()
    checked = 0
    for k in range(ev.size):
        lo = gap[k - 1] if k > 0 else np.inf
        hi = gap[k] if k < gap.size else np.inf
        if min(lo, hi) < 1e-6 * scale:
            continue
        s = np.sign((modes[k] * ref[k]).sum())
        assert np.abs(s * modes[k] - ref[k]).max() < 1e-7 * np.abs(ref[k]).max()
        checked += 1
    assert checked >= ev.size // 2


def test_vibrational_analysis_errors():
    from torchani_amd.grad import vibrational_analysis

    g = _load("ch4_ani1x")
    m, h = torch.from_numpy(g["masses"]), torch.from_numpy(g["hess"])
    with pytest.raises(ValueError, match="meV and cm"):
        vibrational_analysis(m, h, unit="Hz")
    with pytest.raises(ValueError, match="Incorrect mode kind"):
        vibrational_analysis(m, h, mode_kind="abc")
    with pytest.raises(AssertionError):
        vibrational_analysis(m.repeat(2, 1), h.repeat(2, 1, 1))


def test_units_match_reference():
    from torchani_amd import units

    g = _load("ch4_ani1x")
    names = [k[len("unit_"):] for k in g if k.startswith("unit_")]
    assert len(names) >= 10
    for name in names:
        assert abs(getattr(units, name)(1.7) / float(g["unit_" + name]) - 1) < 1e-12, name


@pytest.mark.parametrize("C,A,L,row", [(1, 5, 384, 60000), (6, 7, 1008, 80000), (1, 264, 1008, 80000),
                                       (1, 973, 1008, 80000), (1, 2000, 1008, 80000), (4, 30000, 1008, 80000)])
def test_chunk_size_rule(C, A, L, row):
    from torchani_amd.grad import HESSIAN_BUDGET_BYTES, hessian_chunk_size, hessian_direction_bytes

    K = hessian_chunk_size(C, A, L, row)
    per = hessian_direction_bytes(C * A, L, row)
    assert 1 <= K <= 3 * A
    assert K * per <= HESSIAN_BUDGET_BYTES or K == 1
    chunks = [(j0, min(3 * A, j0 + K)) for j0 in range(0, 3 * A, K)]
    assert len(chunks) == -(-3 * A // K)
    assert sum(j1 - j0 for j0, j1 in chunks) == 3 * A and chunks[-1][1] == 3 * A
    if K < 3 * A:   # (as many as fit)
        assert (K + 1) * per > HESSIAN_BUDGET_BYTES


def test_tuples_have_reference_fields():
    from torchani_amd.tuples import EnergiesForcesHessians, ForcesHessians, VibAnalysis

    assert EnergiesForcesHessians._fields == ("energies", "forces", "hessians")
    assert ForcesHessians._fields == ("forces", "hessians")
    assert VibAnalysis._fields == ("freqs", "modes", "fconstants", "rmasses")
