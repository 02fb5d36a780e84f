"""Golden fixtures for Hessians of models with closed-form pair potentials: the REFERENCE's own fp64 second derivatives.

    python tests/golden/gen_golden_hessians_pairs.py     (needs the reference torchani importable; the outputs are committed)

Full models (tests/golden/hess_x2r_<kind>_<base>.npz): ANI-2xr and ANI-r2s built as gen_golden_2xr.py builds them (the
reference's simple_ani with that generator's LOT / R2S_KW and random_state_dict parameters, build_model below) on the
coordinates of existing fixtures.  ``torchani.grad.hessians``
differentiates the forces of the whole model (``hess``) and of its RepulsionXTB term alone (``hess_pair``), on the rows
``hess_rows`` of H (every row, or a seeded sample for the larger bases).  One ANI-2xr molecule (hess_x2r_vib_ani2xr.npz)
stores its whole H and the reference's ``vibrational_analysis`` for every mode kind.

Standalone potentials (tests/golden/hess_pairs_<base>.npz): RepulsionXTB (cosine / smooth, finite cutoff; infinite
cutoffs on the molecules), and the potentials and constructor arguments of gen_golden_pairs2.cases, on the reference's
all_pairs list with the potential's cutoff, as in gen_golden_pairs2: ``<key>_hess`` on the sampled rows ``hess_rows``.

Long rows (tests/golden/hess_pairs_<case>.npz, ``/`` of the case name replaced by ``_``): the same standalone potentials
on two cases of tests/_aev_cases.py whose rows hold up to 256 entries (species index -> symbol in the ANI-2x order), with
the three rows of the centre (the atom with the long row) among the stored ones; 257 atoms make 12 rows of 11 potentials
300 KiB.

H is stored in float32 (the rounding, 6e-8 of an entry, is far below the tests' gate of 2e-5 of max |H|) to keep every file
in the tens of KiB (the long-row cases: see above).
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_2xr as g2  # noqa: E402  (recipes of the ANI-2xr family; sets up the reference import)
import gen_golden_pairs2 as gp  # noqa: E402

import torch  # noqa: E402
from torchani import grad as rgrad  # noqa: E402
from torchani.neighbors import all_pairs  # noqa: E402
from torchani.potentials import RepulsionXTB  # noqa: E402
from torchani.utils import AtomicNumbersToMasses  # noqa: E402

from torchani_amd.weights import arch_spec  # noqa: E402

# (kind, base, seed of gen_golden_2xr, rows of H stored: None = all)
MODELS = (("ani2xr", "rand_batch_ani2x", 21, 12), ("ani2xr", "water_pbc_ani2x", 22, 24), ("ani2xr", "small_ani2x", 23, 8),
          ("anir2s", "rand_batch_ani2x", 24, 12), ("anir2s", "dense90_ani2x", 25, 16))
VIB = ("ani2xr", "rand_batch_ani2x", 21, 0)   # the molecule whose whole H and vibrational analysis are stored
STANDALONE = {"rand_batch_ani2x": 6, "water_pbc_ani2x": 12, "triclinic_pbc_ani2x": 12}   # base: sampled rows
LONG_ROWS = {name: 12 for name in gp.LONG_ROWS}   # rows stored: the three of the centre (atom 0), then a seeded sample
ZNUM = {"H": 1, "C": 6, "N": 7, "O": 8, "S": 16, "F": 9, "Cl": 17}


def load(base):
    return gp.load_inputs(base)


def standalone_cases(symbols, periodic):
    out = {"xtb_cos": (RepulsionXTB, dict(cutoff=5.2, cutoff_fn="cosine")),
           "xtb_smooth": (RepulsionXTB, dict(cutoff=5.2, cutoff_fn="smooth"))}
    if not periodic:   # (an infinite cutoff has no finite list of periodic images)
        out["xtb_inf"] = (RepulsionXTB, dict(cutoff=math.inf, cutoff_fn="smooth"))
        out["xtb_inf_cos"] = (RepulsionXTB, dict(cutoff=math.inf, cutoff_fn="cosine"))
    out.update(gp.cases(symbols))
    return out


def sample_rows(n, count, seed=5):
    if count is None or count >= n:
        return np.arange(n, dtype=np.int64)
    return np.sort(np.random.RandomState(seed).choice(n, count, replace=False)).astype(np.int64)


def hessian_rows(energy_fn, coords, rows):
    """Rows of H = d^2 (sum of the energies) / d coords^2 [C, len(rows), 3A] through the reference's autograd."""
    C = coords.shape[0]
    x = coords.detach().clone().requires_grad_(True)
    f = rgrad.forces(energy_fn(x), x, retain_graph=True, create_graph=True)
    if len(rows) == 3 * coords.shape[1]:
        return rgrad.hessians(f, x)
    flat = f.reshape(C, -1)
    out = []
    for j in rows:
        (gj,) = torch.autograd.grad(flat[:, j].sum(), x, retain_graph=True)
        out.append(-gj.reshape(C, 1, -1))
    return torch.cat(out, dim=1)


def model_inputs(kind, base):
    g = load(base)
    symbols = arch_spec(kind)[0]
    remap = np.asarray([symbols.index(str(s)) for s in g["symbols"]] + [-1])
    species = remap[g["species"]]
    elem = torch.from_numpy(species.astype(np.int64))
    coords = torch.from_numpy(g["coords"]).double()
    cell = torch.from_numpy(g["cell"]).double() if "cell" in g else None
    pbc = torch.from_numpy(g["pbc"]) if "pbc" in g else None
    return g, symbols, species, elem, coords, cell, pbc


def build_model(kind, seed):
    """The reference's model of ``kind`` in float64 with random_state_dict(kind, 8, seed): the construction of
    gen_golden_2xr.run, with its constants (the x2r_*.npz fixtures of that generator check it, see main)."""
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = g2.simple_ani(lot=g2.LOT[kind], symbols=arch_spec(kind)[0], ensemble_size=8, dispersion=kind == "ani2dr",
                              repulsion=True, periodic_table_index=False, **(g2.R2S_KW if kind == "anir2s" else {}))
    state = {k: torch.from_numpy(v) for k, v in g2.random_state_dict(kind, 8, seed).items()}
    missing, unexpected = model.load_state_dict(state, strict=False)
    assert not [k for k in missing if "neural_networks" in k or "energy_shifter" in k], missing[:3]
    assert not unexpected, unexpected[:3]
    return model.double()


def check_builder(kind, base, seed):
    """build_model reproduces the energies of gen_golden_2xr's fixture x2r_<kind>_<base>.npz."""
    _, _, _, elem, coords, cell, pbc = model_inputs(kind, base)
    with np.load(os.path.join(HERE, f"x2r_{kind}_{base}.npz")) as z:
        ref = z["energies"]
    e = build_model(kind, seed)((elem, coords), cell, pbc).energies.detach().numpy()
    assert np.abs(e - ref).max() < 1e-9, (kind, base, np.abs(e - ref).max())


def run_model(kind, base, seed, count):
    g, symbols, species, elem, coords, cell, pbc = model_inputs(kind, base)
    model = build_model(kind, seed)
    pot = model.potentials["repulsion_xtb"]
    rows = sample_rows(3 * coords.shape[1], count)
    H = hessian_rows(lambda x: model((elem, x), cell, pbc).energies, coords, rows)
    Hp = hessian_rows(lambda x: pot(elem, x, cell, pbc, atomic_nums_input=False), coords, rows)
    out = dict(kind=np.asarray(kind), base=np.asarray(base), seed=np.asarray(seed), symbols=np.asarray(symbols),
               species=species.astype(np.int64), coords=g["coords"], hess_rows=rows,
               hess=H.detach().numpy().astype(np.float32), hess_pair=Hp.detach().numpy().astype(np.float32))
    if "cell" in g:
        out["cell"], out["pbc"] = g["cell"], g["pbc"]
    path = os.path.join(HERE, f"hess_x2r_{kind}_{base}.npz")
    np.savez_compressed(path, **out)
    print(f"{os.path.basename(path)}: {tuple(H.shape)} |H|max={H.abs().max().item():.4e} "
          f"|H_pair|max={Hp.abs().max().item():.4e} -> {os.path.getsize(path) / 1024:.0f} KiB")


def run_vib(kind, base, seed, mol):
    g, symbols, species, elem, coords, cell, pbc = model_inputs(kind, base)
    keep = species[mol] >= 0
    species1 = species[mol:mol + 1, keep]
    elem1 = torch.from_numpy(species1.astype(np.int64))
    coords1 = coords[mol:mol + 1, torch.from_numpy(keep)]
    model = build_model(kind, seed)
    H = hessian_rows(lambda x: model((elem1, x)).energies, coords1, np.arange(3 * coords1.shape[1]))
    znum = torch.as_tensor([[ZNUM[symbols[s]] for s in species1[0]]])
    masses = AtomicNumbersToMasses(dtype=torch.double)(znum)
    out = dict(kind=np.asarray(kind), base=np.asarray(base), seed=np.asarray(seed), symbols=np.asarray(symbols),
               species=species1.astype(np.int64), coords=coords1.numpy(), hess=H.detach().numpy(), masses=masses.numpy())
    for mk in ("mdu", "mdn", "mwn"):
        va = rgrad.vibrational_analysis(masses, H.detach(), mode_kind=mk, unit="cm^-1")
        out["freqs_" + mk] = va.freqs.numpy()
        out["modes_" + mk] = va.modes.numpy()
        out["fconstants_" + mk] = va.fconstants.numpy()
        out["rmasses_" + mk] = va.rmasses.numpy()
    path = os.path.join(HERE, f"hess_x2r_vib_{kind}.npz")
    np.savez_compressed(path, **out)
    print(f"{os.path.basename(path)}: {tuple(H.shape)} freqs {np.round(out['freqs_mdu'][-3:], 1)} "
          f"-> {os.path.getsize(path) / 1024:.0f} KiB")


def run_standalone(base, count):
    g = load(base)
    symbols = [str(s) for s in g["symbols"]]
    elem = torch.from_numpy(g["species"].astype(np.int64))
    coords = torch.from_numpy(g["coords"]).double()
    cell = torch.from_numpy(g["cell"]).double() if "cell" in g else None
    pbc = torch.from_numpy(g["pbc"]) if "pbc" in g else None
    rows = sample_rows(3 * coords.shape[1], count)
    if base in LONG_ROWS:   # the centre's walk is the long one: its three rows, then a sample of the others
        rows = np.concatenate([np.arange(3), 3 + sample_rows(3 * coords.shape[1] - 3, count - 3)]).astype(np.int64)
    out = {"base": np.asarray(base), "hess_rows": rows}
    for key, (cls, kw) in standalone_cases(symbols, cell is not None).items():
        pot = cls(symbols=symbols, **kw).double()

        def energy(x, pot=pot, cut=kw["cutoff"]):
            return pot.compute_from_neighbors(elem, x, all_pairs(cut, elem, x, cell, pbc), atomic=True).energies.sum(dim=1)

        H = hessian_rows(energy, coords, rows)
        out[key + "_hess"] = H.detach().numpy().astype(np.float32)
        print(f"hess_pairs_{base} {key:12s} |H|max={H.abs().max().item():.4e}")
    if base in LONG_ROWS:
        out["species"], out["coords"] = g["species"], g["coords"]
    path = os.path.join(HERE, f"hess_pairs_{gp.file_name(base)}.npz")
    np.savez_compressed(path, **out)
    print(f"{os.path.basename(path)} -> {os.path.getsize(path) / 1024:.0f} KiB")


def main():
    torch.set_num_threads(8)
    only = sys.argv[1:]
    if not only or "standalone" in only:
        for base, count in STANDALONE.items():
            run_standalone(base, count)
    if not only or "long_rows" in only:
        for base, count in LONG_ROWS.items():
            run_standalone(base, count)
    if not only or "vib" in only:
        run_vib(*VIB)
    for kind, base, seed, count in MODELS:
        if not only or kind in only:
            check_builder(kind, base, seed)
            run_model(kind, base, seed, count)


if __name__ == "__main__":
    main()
