"""Golden strain second derivatives: the REFERENCE's fp64 double autograd of E(x S, cell S) with respect to the strain S at
S = I, in its "scaling" convention (ase.py:170-173, as gen_golden_stress.py: coordinates are row vectors, x -> x S,
cell -> cell S), one S per molecule.

    python tests/golden/gen_golden_strain_hessians.py     (needs the reference torchani importable; outputs are committed)

Stored in tests/golden/hess_strain_<name>.npz, all per molecule:
  virial [C, 3, 3]                  d E_c / d S_ab
  strain_hessians [C, 3, 3, 3, 3]   d^2 E_c / d S_ab d S_pq
  internal_strain [C, A, 3, 3, 3]   d^2 E_c / d x_iy d S_ab   (x the unstrained coordinates)
ANI-2x on the base fixtures (their kind, seed and cutoff function, gen_golden.build_reference), and ANI-2xr / ANI-r2s
built with gen_golden_hessians_pairs.build_model; those files also carry species, coordinates, cell and pbc.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402  (puts the reference on the path)
import gen_golden_hessians_pairs as ghp  # noqa: E402

import torch  # noqa: E402

ANI_BASES = ("water_pbc_ani2x", "water_pbc_smooth_ani2x", "triclinic_pbc_ani2x", "benzene_pbc_ani2x", "rand_batch_ani2x")
X2R = (("ani2xr", "water_pbc_ani2x", 22), ("anir2s", "rand_batch_ani2x", 24))   # (kind, base, seed of gen_golden_2xr)


def strain_derivatives(energy_fn, coords, cell):
    """(virial, strain_hessians, internal_strain) of energy_fn(x, cell) -> [C] energies, one strain per molecule."""
    C = coords.shape[0]
    S = torch.eye(3, dtype=torch.float64).repeat(C, 1, 1).requires_grad_(True)
    x = coords.detach().clone().requires_grad_(True)
    xs = torch.einsum("cia,cab->cib", x, S)
    cs = None if cell is None else cell @ S[0]   # (periodic fixtures hold one molecule)
    e = energy_fn(xs, cs)
    (vir,) = torch.autograd.grad(e.sum(), S, create_graph=True)
    sh = torch.zeros((C, 3, 3, 3, 3), dtype=torch.float64)
    ist = torch.zeros((C,) + tuple(coords.shape[1:]) + (3, 3), dtype=torch.float64)
    for a in range(3):
        for b in range(3):
            gS, gx = torch.autograd.grad(vir[:, a, b].sum(), (S, x), retain_graph=True, allow_unused=True)
            sh[:, a, b] = gS.detach()
            if gx is not None:
                ist[:, :, :, a, b] = gx.detach()
    return vir.detach().numpy(), sh.numpy(), ist.numpy()


def save(name, vir, sh, ist, extra):
    path = os.path.join(HERE, f"hess_strain_{name}.npz")
    np.savez_compressed(path, virial=vir, strain_hessians=sh, internal_strain=ist, **extra)
    W = sh.reshape(sh.shape[0], 9, 9)
    print(f"{os.path.basename(path)}: max|W| {np.abs(W).max():.4e} asym {np.abs(W - W.transpose(0, 2, 1)).max():.1e} "
          f"sum rule {np.abs(ist.sum(axis=1)).max():.1e} -> {os.path.getsize(path) / 1024:.0f} KiB")


def run_ani(base):
    with np.load(os.path.join(HERE, base + ".npz")) as z:
        b = {k: z[k] for k in z.files}
    gg.CUTOFF_FN = str(b["cutoff_fn"]) if "cutoff_fn" in b else "cosine"
    model = gg.build_reference(str(b["kind"]), int(b["seed"]))
    elem = torch.as_tensor(b["species"].astype(np.int64))
    coords = torch.as_tensor(b["coords"]).double()
    cell = torch.as_tensor(b["cell"]).double() if "cell" in b else None
    pbc = torch.as_tensor(b["pbc"]) if "pbc" in b else None

    nets = model.potentials["nnp"].neural_networks if hasattr(model, "potentials") else model.neural_networks

    def energy(x, c):   # (as gen_golden_stress.py: the self energies do not depend on the strain)
        return nets(elem, model.aev_computer(elem, x, c, pbc))

    save(base, *strain_derivatives(energy, coords, cell), {"base": np.asarray(base)})


def run_x2r(kind, base, seed):
    g, symbols, species, elem, coords, cell, pbc = ghp.model_inputs(kind, base)
    model = ghp.build_model(kind, seed)

    def energy(x, c):
        return model((elem, x), c, pbc).energies if c is not None else model((elem, x)).energies

    extra = dict(kind=np.asarray(kind), base=np.asarray(base), seed=np.asarray(seed), symbols=np.asarray(symbols),
                 species=species.astype(np.int64), coords=g["coords"])
    if "cell" in g:
        extra["cell"], extra["pbc"] = g["cell"], g["pbc"]
    save(f"x2r_{kind}_{base}", *strain_derivatives(energy, coords, cell), extra)


def main():
    torch.set_num_threads(8)
    for base in ANI_BASES:
        run_ani(base)
    for kind, base, seed in X2R:
        ghp.check_builder(kind, base, seed)
        run_x2r(kind, base, seed)


if __name__ == "__main__":
    main()
