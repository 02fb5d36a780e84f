"""Golden fixtures for Hessians with respect to the coordinates: the REFERENCE's own second derivatives.

    python tests/golden/gen_golden_hessians.py      (needs the reference torchani importable; the outputs are committed)

For a base fixture the reference model (fp64, pyaev, seeded parameters, frozen) gives forces with ``create_graph=True`` and
``torchani.grad.hessians`` differentiates them once more: H [C, 3A, 3A] of the network energy (the self energies are
constant).  Large bases store only ``hess_rows`` sampled rows of H (``hess`` [C, R, 3A]).  The bases of VIB also store
the reference's ``vibrational_analysis`` of H with the masses of ``torchani.utils.AtomicNumbersToMasses``, for every mode
kind and both units, and every fixture the values of the reference's ``torchani.units`` functions at 1.7.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402

BASES = ("ch4_ani1x", "rand_batch_ani2x", "water_pbc_ani2x", "water_pbc_smooth_ani2x", "triclinic_pbc_ani2x",
         "dense90_ani2x", "small_ani2x")
SAMPLED = {"small_ani2x": 24, "dense90_ani2x": 32}   # bases too large to store whole: this many rows of H
VIB = ("ch4_ani1x", "triclinic_pbc_ani2x")   # bases with the reference's vibrational analysis stored
UNIT_FUNCS = ("angstrom2bohr", "bohr2angstrom", "sqrt_mhessian2invcm", "sqrt_mhessian2milliev", "mhessian2fconst",
              "hartree2ev", "ev2kjoulepermol", "ev2kcalpermol", "hartree2kjoulepermol", "hartree2kcalpermol", "ea2debye")


def run_case(base):
    torch = gg.torch
    import torchani
    from torchani import grad as rgrad
    from torchani import units as runits
    from torchani.utils import AtomicNumbersToMasses

    with np.load(os.path.join(gg.HERE, base + ".npz")) as z:
        b = {k: z[k] for k in z.files}
    kind, seed = str(b["kind"]), int(b["seed"])
    gg.CUTOFF_FN = str(b["cutoff_fn"]) if "cutoff_fn" in b else "cosine"
    model = gg.build_reference(kind, seed)
    nets = model.potentials["nnp"].neural_networks if hasattr(model, "potentials") else model.neural_networks
    elem = torch.as_tensor(b["species"].astype(np.int64))
    coords = torch.as_tensor(b["coords"]).double().requires_grad_(True)
    cell = torch.as_tensor(b["cell"]).double() if "cell" in b else None
    pbc = torch.as_tensor(b["pbc"]) if "pbc" in b else None
    C, A = elem.shape
    e = nets(elem, model.aev_computer(elem, coords, cell, pbc))
    f = rgrad.forces(e, coords, retain_graph=True, create_graph=True)
    out = {"base": np.asarray(base)}
    if base in SAMPLED:
        rs = np.random.RandomState(5)
        rows = np.sort(rs.choice(3 * A, SAMPLED[base], replace=False))
        flat = f.reshape(C, 3 * A)
        hess = []
        for j in rows:
            (gj,) = torch.autograd.grad(flat[:, j].sum(), coords, retain_graph=True)
            hess.append(-gj.reshape(C, 1, 3 * A))
        H = torch.cat(hess, dim=1)
        out["hess_rows"] = rows.astype(np.int64)
    else:
        H = rgrad.hessians(f, coords)
        out["hess_rows"] = np.arange(3 * A, dtype=np.int64)
    out["hess"] = H.detach().numpy()
    out["forces"] = f.detach().numpy()
    if base in VIB:
        symbols = [str(s) for s in b["symbols"]]
        znum = torch.as_tensor([[gg.ZNUM[symbols[s]] for s in b["species"][0]]])
        masses = AtomicNumbersToMasses(dtype=torch.double)(znum)
        out["masses"] = masses.numpy()
        for kind_ in ("mdu", "mdn", "mwn"):
            for unit in ("cm^-1", "meV"):
                va = rgrad.vibrational_analysis(masses, H, mode_kind=kind_, unit=unit)
                tag = f"{kind_}_{'invcm' if unit == 'cm^-1' else 'mev'}"
                out["freqs_" + tag] = va.freqs.detach().numpy()
                out["modes_" + tag] = va.modes.detach().numpy()
                out["fconstants_" + tag] = va.fconstants.detach().numpy()
                out["rmasses_" + tag] = va.rmasses.detach().numpy()
    for name in UNIT_FUNCS:
        out["unit_" + name] = np.asarray(float(getattr(runits, name)(1.7)))
    path = os.path.join(gg.HERE, "hess_" + base + ".npz")
    np.savez_compressed(path, **out)
    Hn = out["hess"]
    print(f"hess_{base}: {Hn.shape} |H|max={np.abs(Hn).max():.4e} torchani {torchani.__version__ if hasattr(torchani, '__version__') else ''}"
          f" -> {os.path.getsize(path) / 1024:.0f} KiB")


def main():
    gg.torch.set_num_threads(8)
    for base in (sys.argv[1:] or BASES):
        run_case(base)


if __name__ == "__main__":
    main()
