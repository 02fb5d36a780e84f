"""Golden virials of the pair potentials and of the ANI-2xr / ANI-2dr models, from the reference's own classes in float64 on
the cases of tests/_pair_virial_cases.py (the recipe of gen_golden_stress.py: coordinates and cell multiplied by a scaling
matrix, autograd with respect to it):

    python tests/golden/gen_golden_pair_virials.py    -> tests/golden/pairs_virial_<case>.npz,
                                                          tests/golden/x2r_virial_<kind>_<case>.npz

pairs_virial_<case>.npz, per potential key (xtb, xtb_cos, the seven of gen_golden_pairs2.cases, d3, d3_b973c):
  <key>_virial       [3, 3] the scaling virial dE / dS at S = 1 (Hartree)
  <key>_virial_self  [3, 3] the part of the pairwise sum carried by pairs (i, i): an atom and its own periodic image
  <key>_abs          A = sum over pairs |dE / d d_p| |d_p|, the sum without cancellation (the gates are relative to it)
  <key>_virial_f32   the scaling virial from the same class in float32
  <key>_pairs        [2] number of pairs inside the cutoff, and of those with i == i
  <key>_energy       the energy; <key>_forces for the two own-image cells, which no older fixture covers
The pairwise form sum_p d_p (x) dE / d d_p -- autograd on the difference vectors of the unscaled list, the form the kernels
use -- must agree with the scaling virial to 1e-9 A, and W with its transpose to 1e-10 A.

x2r_virial_<kind>_<case>.npz (self-contained like x2r_*.npz; parameters random_state_dict(kind, 8, seed)): symbols, species
in the model's order, coords, cell, pbc, seed, energies, forces, virial_total, virial_nnp with the pair terms switched off
(set_enabled), and abs_<term> = A of each pair term; virial_total = virial_nnp + the pairwise sums of the terms to 1e-9 A.
ANI-2dr also stores d3_cutoff: 8 A, on own4 7.5 A (tests/_pair_virial_cases.py says why).
ANI-r2s is not here: its repulsion has no cutoff, and with a cell the reference's all_pairs then lists
no image at all (ceil(inf / width) images per direction) while the engine's rows hold molecules only.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_d3 as g3  # noqa: E402,F401  (reference import + h5py stand-in)
import gen_golden_pairs2 as gp  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
import _pair_virial_cases as pv  # noqa: E402

import torch  # noqa: E402
from torchani.arch import simple_ani  # noqa: E402
from torchani.neighbors import Neighbors, all_pairs  # noqa: E402
from torchani.potentials import RepulsionXTB, TwoBodyDispersionD3  # noqa: E402

from torchani_amd.weights import arch_spec, random_state_dict  # noqa: E402

LOT = {"ani2xr": "wb97x-631gd", "ani2dr": "b973c-def2mtzvp"}


def inputs(case):
    """The case as tensors, checked against gen_golden_pairs2.load_inputs where that knows the name."""
    if case.name in ("water_pbc_ani2x", "triclinic_pbc_ani2x", "chunk129_pbc/built"):
        g = gp.load_inputs(case.name)
        assert tuple(str(s) for s in g["symbols"]) == case.symbols and np.array_equal(g["species"], case.species)
        assert np.array_equal(g["coords"], case.coords) and np.array_equal(g["cell"], case.cell)
        assert tuple(bool(b) for b in g["pbc"]) == case.pbc
    return (torch.from_numpy(case.species), torch.from_numpy(case.coords), torch.from_numpy(case.cell),
            torch.tensor(case.pbc))


def potentials(symbols):
    """key -> (constructor of the reference's class, cutoff)"""
    kw = pv.analytic_kwargs(symbols)
    out = {}
    for key, (cls, args) in gp.cases(symbols).items():
        assert cls.__name__ == kw[key][0] and args == kw[key][1], key   # (the table the GPU test builds its own from)
        out[key] = (lambda cls=cls, args=args: cls(symbols=symbols, **args), args["cutoff"])
    for key, args in pv.XTB_KW.items():
        out[key] = (lambda args=args: RepulsionXTB(symbols=symbols, **args), args["cutoff"])
    for key, args in pv.D3_KW.items():
        out[key] = (lambda args=args: TwoBodyDispersionD3.from_functional(symbols=symbols, **args), args["cutoff"])
    assert (gp.CHARGES, gp.ETA, gp.EPS, gp.SIGMA) == (pv.CHARGES, pv.ETA, pv.EPS, pv.SIGMA)
    return out


def scaling_virial(energy_of, coords, cell, dtype):
    s = torch.eye(3, dtype=dtype, requires_grad=True)
    x = coords.to(dtype).requires_grad_(True)
    e = energy_of(x @ s, cell.to(dtype) @ s)
    w, gx = torch.autograd.grad(e, (s, x))
    return float(e.detach()), w.numpy().astype(np.float64), -gx.numpy().astype(np.float64)


def run_pairs(case):
    elem, coords, cell, pbc = inputs(case)
    out = {}
    for key, (make, cutoff) in potentials(list(case.symbols)).items():
        if key not in pv.keys_of(case.name):
            continue

        def energy_of(pot):
            return lambda x, c: pot.compute_from_neighbors(elem, x, all_pairs(cutoff, elem, x, c, pbc)).energies.sum()

        pot = make().double()
        e, w, f = scaling_virial(energy_of(pot), coords, cell, torch.float64)
        _, w32, _ = scaling_virial(energy_of(make().float()), coords, cell, torch.float32)
        # the pairwise ("fdotr") form on the unscaled list
        nb = all_pairs(cutoff, elem, coords.double(), cell.double(), pbc)
        d = nb.diff_vectors.detach().clone().requires_grad_(True)
        e2 = pot.compute_from_neighbors(elem, coords.double(), Neighbors(nb.indices, d.norm(dim=1), d)).energies.sum()
        (g,) = torch.autograd.grad(e2, d)
        own = nb.indices[0] == nb.indices[1]
        w_pair = torch.einsum("pa,pb->ab", d.detach(), g).numpy()
        w_self = torch.einsum("pa,pb->ab", d.detach()[own], g[own]).numpy()
        a = float((g.norm(dim=1) * d.detach().norm(dim=1)).sum())
        assert abs(float(e2.detach()) - e) <=1e-12 * max(1.0, abs(e))
        assert np.abs(w - w.T).max() <= 1e-10 * a, (case.name, key, np.abs(w - w.T).max(), a)
        assert np.abs(w - w_pair).max() <= 1e-9 * a, (case.name, key, np.abs(w - w_pair).max(), a)
        out.update({key + "_virial": w, key + "_virial_self": w_self, key + "_abs": np.asarray(a), key + "_virial_f32": w32,
                    key + "_pairs": np.asarray([own.numel(), int(own.sum())]), key + "_energy": np.asarray(e)})
        if case.name in ("own4", "own1"):
            out[key + "_forces"] = f
        print(f"{case.name:20s} {key:8s} pairs {own.numel():5d} own {int(own.sum()):4d}  max|W| {np.abs(w).max():.3e}  "
              f"max|W_self| {np.abs(w_self).max():.3e}  A {a:.3e}  f32 err / A {np.abs(w32 - w).max() / a:.2e}  "
              f"|F|max {np.abs(f).max():.2e}")
    path = os.path.join(HERE, f"pairs_virial_{case.file_name}.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


def run_model(kind, case, seed):
    symbols = arch_spec(kind)[0]
    remap = np.asarray([symbols.index(s) for s in case.symbols] + [-1])
    species = remap[case.species]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = simple_ani(lot=LOT[kind], symbols=symbols, ensemble_size=8, dispersion=kind == "ani2dr", repulsion=True,
                           periodic_table_index=False)
    state = {k: torch.from_numpy(v) for k, v in random_state_dict(kind, 8, seed).items()}
    missing, unexpected = model.load_state_dict(state, strict=False)
    assert not [k for k in missing if "neural_networks" in k or "energy_shifter" in k], missing[:3]
    assert not unexpected, unexpected[:3]
    model = model.double()
    if kind == "ani2dr" and case.name == "own4":   # (at the model's 8 A the engine's rows would not hold the neighbors)
        model.potentials["dispersion_d3"].cutoff = pv.OWN4_D3_CUTOFF
    elem = torch.from_numpy(species.astype(np.int64))
    _, coords, cell, pbc = inputs(case)

    def energy_of(x, c):
        return model((elem, x), c, pbc).energies.sum()

    e, w, f = scaling_virial(energy_of, coords, cell, torch.float64)
    # the pair terms' pairwise sums and their A (the model test adds rel x A of the enabled terms to the network gate)
    w_pairs, a_of = np.zeros((3, 3)), {}
    for name, _ in pv.MODEL_PAIR_TERMS[kind]:
        pot = model.potentials[name]
        nb = all_pairs(pot.cutoff, elem, coords.double(), cell.double(), pbc)
        d = nb.diff_vectors.detach().clone().requires_grad_(True)
        ep = pot.compute_from_neighbors(elem, coords.double(), Neighbors(nb.indices, d.norm(dim=1), d)).energies.sum()
        (g,) = torch.autograd.grad(ep, d)
        w_pairs += torch.einsum("pa,pb->ab", d.detach(), g).numpy()
        a_of[name] = float((g.norm(dim=1) * d.detach().norm(dim=1)).sum())
        model.set_enabled(name, False)
    _, w_nnp, _ = scaling_virial(energy_of, coords, cell, torch.float64)
    assert np.abs(w - w.T).max() <= 1e-10 * max(1.0, np.abs(w).max())
    assert np.abs(w - w_nnp - w_pairs).max() <= 1e-9 * sum(a_of.values()), np.abs(w - w_nnp - w_pairs).max()
    out = dict(kind=np.asarray(kind), seed=np.asarray(seed), symbols=np.asarray(symbols), species=species.astype(np.int64),
               coords=case.coords, cell=case.cell, pbc=np.asarray(case.pbc), energies=np.asarray([e]), forces=f,
               virial_total=w, virial_nnp=w_nnp, **{"abs_" + k: np.asarray(v) for k, v in a_of.items()})
    if kind == "ani2dr":
        out["d3_cutoff"] = np.asarray(float(model.potentials["dispersion_d3"].cutoff))
    path = os.path.join(HERE, f"x2r_virial_{kind}_{case.file_name}.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: E={e:+.9f} |F|max={np.abs(f).max():.4f} max|W|={np.abs(w).max():.4f} max|W_nnp|={np.abs(w_nnp).max():.4f} "
          f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    torch.set_num_threads(8)
    only = sys.argv[1:]
    if not only or "pairs" in only:
        for nm in pv.CASE_NAMES:
            run_pairs(pv.case_by_name(nm))
    if not only or "models" in only:
        for kind, nm, seed in pv.MODEL_CASES:
            run_model(kind, pv.case_by_name(nm), seed)
