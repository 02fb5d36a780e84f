"""Virials of the pair potentials and of the ANI-2xr / ANI-2dr models against the reference's fp64 scaling virials
(tests/golden/gen_golden_pair_virials.py) on the cases of tests/_pair_virial_cases.py: k_pair<KIND> (xTB, ZBL, the three
Lennard-Jones terms, Coulomb, MNOK), k_d3_pair + k_d3_cngrad, the sums of ANI._pair_terms / _local_stage and their shards.

Gate of a potential: |W - W_ref|max <= rel x A, A = sum over pairs |dE / d d_p| |d_p| (stored with the fixture), rel = 5e-6
(xTB), 1e-5 (analytic family), 2e-5 (D3): 4 x the error of the reference's own float32 evaluation, capped by the relative
force gate of the same loop -- tests/test_pair_virials_host.py derives them and proves that own images dropped, xz / yz
swapped, a missing transpose entry or a missing 1/2 each miss them by 10 x or more.  profiles/pair_virial_tests.txt has what
the kernels measure: at worst 1.26e-6 A (xTB, own1), 7.5e-7 A (analytic, lj_rep on triclinic_pbc_ani2x) and 1.29e-6 A (D3,
chunk129_pbc/built), where the reference's float32 has 1.19e-6, 6.97e-6 and 1.91e-5; the models 1.9e-5 Ha of 115 Ha.

The tests found two bugs in csrc/pair.hip, fixed with them: the D3 virial asked for without a gradient buffer lacked its
coordination-number term (100 to 13 000 gates), and an atom's own images went into the gradient as two terms that cancel
only up to rounding (1.2e-16 Ha/A on own1 instead of 0.0).

D3 at 8 A on own4 needs rows of 284 to 286 entries, more than a row holds (256): D3 runs there with a 7.5 A cutoff (key
d3_r75, rows of 222 to 227 entries; ANI-2dr's dispersion term likewise), and test_rows_over_256_entries_are_refused asserts
that the engine refuses the 8 A rows instead of returning a virial without them.
"""
import os

import numpy as np
import pytest
import torch

import _pair_virial_cases as pv
from _util import seeded_state
from test_gpu_parity import E_ATOM_TOL, F_TOL, report

pytestmark = pytest.mark.gpu

SHARD_TOL = 1e-6                    # x max(1, max |W|): tests/test_gpu_md.py::test_virial_matches_reference_stress


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from torchani_amd import _lib

    _lib.lib()
    return torch.device("cuda:0")


_row_models = {}


def row_model(mode, dev):
    """An ANI-2x model whose _pair_rows builds the potentials' rows in the given neighbor mode (seven species)."""
    from torchani_amd.models import ANI2x

    if mode not in _row_models:
        _row_models[mode] = ANI2x(state_dict=seeded_state("ani2x", 8, 31), device=dev, periodic_table_index=False,
                                  neighborlist=mode, row_capacity=256)
    return _row_models[mode]


def make_potential(key, symbols, dev):
    from torchani_amd import potentials as P

    if key in pv.XTB_KW:
        pot = P.RepulsionXTB(symbols, **pv.XTB_KW[key])
    elif key in pv.D3_KW:
        kw = pv.D3_KW[key]
        pot = P.TwoBodyDispersionD3.from_functional(symbols, kw["functional"], cutoff=kw["cutoff"], cutoff_fn=kw["cutoff_fn"])
    else:
        cls, kw = pv.analytic_kwargs(symbols)[key]
        pot = getattr(P, cls)(symbols, **kw)
    return pot.to(dev)


def to_dev(case, dev):
    sp32 = torch.from_numpy(case.species).to(dev).to(torch.int32).contiguous()
    return sp32, torch.from_numpy(case.coords).to(dev), torch.from_numpy(case.cell).to(dev), case.pbc


def accumulate(pot, sp32, rows, dev, energies=True, virial=True, into=None, **kw):
    n = sp32.numel()
    ae = torch.zeros(n, dtype=torch.float32, device=dev) if energies else None
    gc = torch.zeros((n, 3), dtype=torch.float32, device=dev) if energies else None
    w = (torch.zeros((3, 3), dtype=torch.float64, device=dev) if into is None else into) if virial else None
    pot.accumulate(sp32, rows, ae, gc, w, **kw)
    return ae, gc, w


@pytest.mark.parametrize("case_name", pv.CASE_NAMES)
def test_standalone_virials_match_reference(dev, case_name):
    """pot.accumulate(..., virial=w) on the engine's rows, batch and cell mode: all nine components within the gate, w
    symmetric bit for bit, energies and gradient untouched by asking for it, the same virial without them, += on a second
    call; on own1 the gradient is exactly zero while W is made of own images alone."""
    case, ref = pv.case_by_name(case_name), pv.load_virials(case_name)
    sp32, x, cell, pbc = to_dev(case, dev)
    for key in pv.keys_of(case_name):
        pot = make_potential(key, list(case.symbols), dev)
        w_ref, a = ref[key + "_virial"], float(ref[key + "_abs"])
        gate = pv.GATE_REL[pv.FAMILY[key]] * a
        for mode in ("batch", "cell"):
            rows = row_model(mode, dev)._pair_rows(pot, sp32, x, cell, pbc)
            rows.raise_on_overflow()
            ae0, gc0, _ = accumulate(pot, sp32, rows, dev, virial=False)
            ae, gc, w = accumulate(pot, sp32, rows, dev)
            _, _, w_only = accumulate(pot, sp32, rows, dev, energies=False)
            torch.cuda.synchronize()
            wn = w.cpu().numpy()
            err = float(np.abs(wn - w_ref).max())
            own = int(ref[key + "_pairs"][1])
            report(f"pairvir {case_name:20s} {key:8s} {mode:5s} |W - W_ref|max / A = {err / a:.2e} (gate "
                   f"{pv.GATE_REL[pv.FAMILY[key]]:.0e}; fp32 reference "
                   f"{np.abs(ref[key + '_virial_f32'] - w_ref).max() / a:.2e})  max|W| = {np.abs(w_ref).max():.3e}  A = {a:.3e}"
                   f"  own images {own}/{int(ref[key + '_pairs'][0])}")
            if (key, case_name) not in pv.EXCLUDED:   # (the counting condition of the host test)
                assert err <= gate, f"{key} on {case_name} ({mode}): off by {err / a:.2e} A\n{wn}\n{w_ref}"
            assert torch.equal(w, w.T)
            assert torch.equal(ae, ae0) and torch.equal(gc, gc0)
            wmax = float(w.abs().max())
            assert float((w_only - w).abs().max()) <= 1e-12 * wmax, (key, mode)
            accumulate(pot, sp32, rows, dev, into=w)
            assert float((w - 2.0 * w_only).abs().max()) <= 2e-12 * wmax, (key, mode)
            if case_name == "own1":
                assert float(gc.abs().max()) == 0.0, (key, mode, gc)
            elif case_name == "own4":   # (no older fixture has this cell: the force gates of tests/test_gpu_parity.py)
                f_ref = ref[key + "_forces"].reshape(-1, 3)
                fe = float(np.abs(-gc.cpu().numpy() - f_ref).max())
                report(f"pairvir {case_name:20s} {key:8s} {mode:5s} |F err| = {fe:.2e} (scale {np.abs(f_ref).max():.1e})")
                assert fe <= pv.GATE_CAP[pv.FAMILY[key]] * max(1e-3, np.abs(f_ref).max()), (key, mode)


@pytest.mark.parametrize("case_name", [c for c in pv.CASE_NAMES if c != "own1"])
def test_virial_shards_add_up(dev, case_name):
    """Three unequal shards: D3 on rows of all atoms with lo / hi, Lennard-Jones on rows built for lo .. hi."""
    case = pv.case_by_name(case_name)
    sp32, x, cell, pbc = to_dev(case, dev)
    n = case.n_atoms
    bounds = [0, max(1, n // 5), n // 2 + 1, n]
    assert len(set(np.diff(bounds))) == 3 or n == 4
    model = row_model("batch", dev)
    for key in (pv.d3_key_of(case_name), "lj"):
        pot = make_potential(key, list(case.symbols), dev)
        rows = model._pair_rows(pot, sp32, x, cell, pbc)
        _, _, whole = accumulate(pot, sp32, rows, dev)
        parts = torch.zeros_like(whole)
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            if pv.FAMILY[key] == "d3":
                _, gc, wp = accumulate(pot, sp32, rows, dev, lo=lo, hi=hi)
            else:
                part_rows = model._pair_rows(pot, sp32, x, cell, pbc, lo, hi)
                assert (part_rows.lo, part_rows.hi) == (lo, hi)
                _, gc, wp = accumulate(pot, sp32, part_rows, dev)
            assert float(gc[:lo].abs().max() if lo else 0.0) == 0.0 and float(gc[hi:].abs().max() if hi < n else 0.0) == 0.0
            parts += wp
        d = float((parts - whole).abs().max())
        report(f"pairvir {case_name:20s} {key:8s} three shards {bounds}: |sum - whole|max = {d:.2e} (max|W| {float(whole.abs().max()):.3e})")
        assert d <= SHARD_TOL * max(1.0, float(whole.abs().max()))


PUSH_CASES = ("chunk129_open", "chunk256_open", "ang128_at_open")   # tests/test_gpu_neighbors_external.py CONSUMER_CASES


@pytest.mark.parametrize("name", PUSH_CASES)
def test_push_path_virial_of_an_isolated_system(dev, oracle64, name):
    """RepulsionZBL on rows from a full list (ANIHIP_PAIR_PUSH).  For an isolated system W = sum_k x_k (x) g_k: formed in fp64
    from the forces of the pairs2_* fixture, gate rel x A with A = sum_k |g_k| |x_k|."""
    import _nbr_cases as nc
    from test_gpu_neighbors_external import full_rows, listed_everything
    from torchani_amd import potentials as P
    from torchani_amd.constants import aev_constants_2x
    from torchani_amd.engine import AevEngine

    case = nc.case_by_name(name)
    n = case.n_atoms
    ref = dict(np.load(os.path.join(pv.GOLDEN_DIR, f"pairs2_{name}_built.npz")))
    sp = torch.from_numpy(case.species).to(dev).contiguous()
    x = torch.from_numpy(case.coords).to(dev).contiguous()
    x64 = case.coords.reshape(n, 3).astype(np.float64)
    pots = {"zbl": P.RepulsionZBL(list(pv.ANI2X_SYMBOLS), cutoff=5.2, cutoff_fn="smooth"),
            "zbl_cos": P.RepulsionZBL(list(pv.ANI2X_SYMBOLS), k=0.4685, cutoff=4.0, cutoff_fn="cosine")}
    for key, pot in pots.items():
        pot = pot.to(dev)
        eng = AevEngine(aev_constants_2x(7)._replace(Rcr=pot.cutoff, Rca=1e-3))
        rows = full_rows(eng, listed_everything(oracle64, case, pot.cutoff), dev, 256)
        assert rows.symmetric is False and not rows.overflowed()
        g = -ref[key + "_forces"].reshape(n, 3)
        w_ref = np.einsum("ka,kb->ab", x64, g)
        a = float((np.linalg.norm(g, axis=1) * np.linalg.norm(x64, axis=1)).sum())
        ws = []
        for r in (rows, eng.neighbors(sp, x, mode="batch", row_cap=256)):
            _, _, w = accumulate(pot, sp, r, dev)
            assert torch.equal(w, w.T)
            ws.append(w.cpu().numpy())
        err, dsym = float(np.abs(ws[0] - w_ref).max()), float(np.abs(ws[0] - ws[1]).max())
        report(f"pairvir push {name:16s} {key:8s} |W - sum x (x) g|max / A = {err / a:.2e} (gate {pv.GATE_REL['analytic']:.0e}); "
               f"from symmetric rows {dsym / a:.2e}; max|W| = {np.abs(w_ref).max():.3e}  A = {a:.3e}")
        assert np.abs(w_ref).max() >= 100.0 * pv.GATE_REL["analytic"] * a   # (the counting condition of the host test)
        assert err <= pv.GATE_REL["analytic"] * a and np.abs(ws[1] - w_ref).max() <= pv.GATE_REL["analytic"] * a


@pytest.mark.parametrize("kind,case_name,seed", pv.MODEL_CASES)
def test_model_virials_match_reference(dev, kind, case_name, seed):
    """energies_and_forces(stress=True) of ANI-2xr / ANI-2dr: networks + xTB (+ D3 on rows of all atoms) against the
    reference's builder in fp64, then the network part alone (own4: the AEV backward's virial on a cell with own images),
    the plain call, two shards, and the fixed-point accumulation."""
    from torchani_amd.models import ANI2dr, ANI2xr
    from torchani_amd.weights import random_state_dict

    ref = pv.load_model_virials(kind, case_name)
    sp = torch.from_numpy(ref["species"]).to(dev)
    x = torch.from_numpy(ref["coords"]).to(dev)
    cell = torch.from_numpy(ref["cell"]).to(dev)
    pbc = tuple(bool(b) for b in ref["pbc"])
    terms = pv.MODEL_PAIR_TERMS[kind]
    w_tot, w_nnp = ref["virial_total"], ref["virial_nnp"]
    pair_gate = sum(pv.GATE_REL[fam] * float(ref["abs_" + name]) for name, fam in terms)
    n = sp.shape[1]
    fscale = max(1.0, float(np.abs(ref["forces"]).max()))
    for mode in ("batch", "cell"):
        model = {"ani2xr": ANI2xr, "ani2dr": ANI2dr}[kind](
            state_dict=random_state_dict(kind, 8, seed), device=dev, periodic_table_index=False, neighborlist=mode,
            row_capacity=256)
        assert [str(s) for s in ref["symbols"]] == list(model.symbols)
        if "d3_cutoff" in ref and float(ref["d3_cutoff"]) != model.potentials["dispersion_d3"].cutoff:
            # own4: the dispersion term with the fixture's 7.5 A cutoff (the model's 8 A needs rows of 286 entries)
            from torchani_amd.potentials import TwoBodyDispersionD3

            model.add_pair_potential("dispersion_d3", TwoBodyDispersionD3.from_functional(
                list(model.symbols), "b973c", cutoff=float(ref["d3_cutoff"]), cutoff_fn="smooth").to(dev))
        out = model.energies_and_forces(sp, x, cell, pbc, stress=True)
        plain = model.energies_and_forces(sp, x, cell, pbc)
        parts = [model.energies_and_forces(sp, x, cell, pbc, shard=(r, 2), stress=True).virial for r in range(2)]
        torch.cuda.synchronize()
        vir = out.virial.cpu().numpy()
        gate = pv.NETWORK_VIRIAL_TOL * max(1.0, float(np.abs(w_tot).max())) + pair_gate
        err = float(np.abs(vir - w_tot).max())
        assert plain.virial is None and torch.equal(plain.energies, out.energies)
        # (fp32 atomics of the AEV backward arrive in any order; bit for bit in fixed point below)
        assert float((plain.forces - out.forces).abs().max()) <= 16 * np.finfo(np.float32).eps * fscale
        assert np.abs(vir - vir.T).max() == 0.0
        dsh = float((parts[0] + parts[1] - out.virial).abs().max())
        assert dsh <= SHARD_TOL * max(1.0, float(np.abs(vir).max()))
        assert abs(float(out.energies[0]) - float(ref["energies"][0])) <= E_ATOM_TOL * n
        assert np.abs(out.forces.cpu().numpy() - ref["forces"]).max() <= F_TOL * fscale
        # fixed-point accumulation: the same virial, energies and forces (to 2^-32 Ha/A and the rounding of the partial sums)
        model.deterministic_forces = True
        det = model.energies_and_forces(sp, x, cell, pbc, stress=True)
        model.deterministic_forces = False
        ddet = float((det.virial - out.virial).abs().max())
        assert ddet <= SHARD_TOL * max(1.0, float(np.abs(vir).max()))
        assert torch.equal(det.energies, out.energies)
        assert float((det.forces - out.forces).abs().max()) <= 16 * np.finfo(np.float32).eps * fscale + 2.0 ** -31
        # the network part alone
        for name, _ in terms:
            model.set_enabled(name, False)
        nnp = model.energies_and_forces(sp, x, cell, pbc, stress=True).virial.cpu().numpy()
        err_n = float(np.abs(nnp - w_nnp).max())
        gate_n = pv.NETWORK_VIRIAL_TOL * max(1.0, float(np.abs(w_nnp).max()))
        report(f"pairvir model {kind} {case_name:20s} {mode:5s} |W - W_ref|max = {err:.2e} Ha (gate {gate:.2e}: network "
               f"{gate - pair_gate:.1e} + pair terms {pair_gate:.1e}; max|W| {np.abs(w_tot).max():.3f}); network part alone "
               f"{err_n:.2e} (gate {gate_n:.1e}, max|W| {np.abs(w_nnp).max():.4f}); two shards {dsh:.1e}; fixed point {ddet:.1e}")
        assert err <= gate, f"{vir}\n{w_tot}"
        assert err_n <= gate_n, f"{nnp}\n{w_nnp}"


def test_rows_over_256_entries_are_refused(dev):
    """D3 with its usual 8 A cutoff on own4: 570 pairs of 4 atoms, rows of 284 to 286 entries where a row holds 256.  The
    builder flags the overflow, and ANI-2dr raises instead of returning energies, forces and a virial without those rows."""
    from torchani_amd.models import ANI2dr
    from torchani_amd.weights import random_state_dict

    case = pv.case_by_name("own4")
    sp32, x, cell, pbc = to_dev(case, dev)
    pot = make_potential("d3", list(case.symbols), dev)
    ref = pv.load_model_virials("ani2dr", "own4")
    for mode in ("batch", "cell"):
        assert row_model(mode, dev)._pair_rows(pot, sp32, x, cell, pbc).overflowed(), mode
        model = ANI2dr(state_dict=random_state_dict("ani2dr", 8, int(ref["seed"])), device=dev, periodic_table_index=False,
                       neighborlist=mode, row_capacity=256)
        assert model.potentials["dispersion_d3"].cutoff == 8.0
        with pytest.raises(RuntimeError, match="dispersion_d3"):
            model.energies_and_forces(torch.from_numpy(ref["species"]).to(dev), x, cell, pbc, stress=True)
