"""Records what the host-side tests compare against the reference package into tests/golden/reference_meta/, so that they
run from this repository alone:

    python tests/golden/gen_golden_reference_meta.py REFERENCE_ROOT     (a checkout of the reference; the outputs are committed)

  api_ani2x.npz        signatures of the reference's grad helpers, EnergiesForces fields, grad.__all__, the state-dict
                       layout of its ANI-2x Assembler models (with the values of the non-network entries), and its ANIRadial /
                       ANIAngular terms evaluated on seeded distances and vectors
  d3_tables.npz        the c6 / cn_a / cn_b tables of resources/c6.h5 (first 19 x 19 elements, as the byte-level HDF5 reader
                       below finds them) and the covalent radii / sqrt empirical charges of resources/atomic_constants.json
  *.xyz, xyz_reads.npz three xyz files of the reference (the first 64 frames of dataset/xyz_files/13.xyz) and what the
                       reference's io.read_xyz returns for them
"""
import inspect
import json
import os
import shutil
import struct
import sys
import types
import warnings

import numpy as np
import torch

sys.dont_write_bytecode = True
REF = os.path.abspath(sys.argv[1])
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_meta")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def import_reference():
    class _Any:
        def __class_getitem__(cls, k):
            return cls

    for name in ("h5py", "zarr"):   # (optional imports of the reference that these records do not need)
        if name not in sys.modules:
            m = types.ModuleType(name)
            for k in ("File", "Group", "Dataset", "Datatype"):
                setattr(m, k, type(k, (_Any,), {}))
            sys.modules[name] = m
    os.environ["TORCHANI_NO_WARN_EXTENSIONS"] = "1"
    sys.path.insert(0, REF)


def recipe(asm, neighborlist="all_pairs"):
    from torchani.utils import SYMBOLS_2X

    asm.set_symbols(SYMBOLS_2X)
    asm.set_global_cutoff_fn("cosine")
    asm.set_aev_computer(radial="ani2x", angular="ani2x", strategy="pyaev")
    asm.set_atomic_networks(ctor="ani2x")
    asm.set_neighborlist(neighborlist)
    asm.set_gsaes_as_self_energies("wb97x-631gd")
    return asm


def api():
    import torchani
    from torchani.aev import ANIAngular, ANIRadial
    from torchani.arch import Assembler

    meta = {"grad_signatures": {}, "energies_forces_fields": list(torchani.tuples.EnergiesForces._fields),
            "grad_all": list(torchani.grad.__all__)}
    for fn in ("forces", "grads", "forces_for_training", "energies_and_forces", "single_point"):
        meta["grad_signatures"][fn] = [[p.name, repr(p.default)]
                                       for p in inspect.signature(getattr(torchani.grad, fn)).parameters.values()]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = recipe(Assembler()).assemble(8)
        no_pti = recipe(Assembler(periodic_table_index=False)).assemble(8)
    meta["section_a_state"] = {k: list(v.shape) for k, v in plain.state_dict().items()}
    meta["section_a_dtypes"] = {k: str(v.dtype).replace("torch.", "") for k, v in plain.state_dict().items()}
    sd = no_pti.state_dict()
    meta["assembler_state"] = {k: list(v.shape) for k, v in sd.items()}
    arrays = {"value/" + k: v.double().numpy() for k, v in sd.items()
              if "aev_computer" in k or k in ("atomic_numbers", "energy_shifter.self_energies")}
    torch.manual_seed(0)
    td, tv = torch.rand(2, 40, dtype=torch.float64) * 3.4 + 0.4, torch.randn(2, 40, 3, dtype=torch.float64)
    tv = tv / tv.norm(dim=-1, keepdim=True) * td.unsqueeze(-1)
    d = torch.linspace(0.5, 6.0, 12, dtype=torch.float64)
    arrays.update(terms_d=d.numpy(), terms_td=td.numpy(), terms_tv=tv.numpy())
    for name, kw in (("like_1x", {}), ("like_2x", {}), ("cover_linearly", dict(cutoff_fn="smooth"))):
        arrays["radial/" + name] = getattr(ANIRadial, name)(**kw).double()(d).numpy()
        arrays["angular/" + name] = getattr(ANIAngular, name)(**kw).double()(td, tv).numpy()
    np.savez_compressed(os.path.join(OUT, "api_ani2x.npz"), meta=json.dumps(meta), **arrays)


def d3_tables():
    b = open(os.path.join(REF, "torchani", "resources", "c6.h5"), "rb").read()
    nbytes = 4 * 95 * 95 * 25
    addrs, i = [], b.find(struct.pack("<Q", nbytes))
    while i >= 0:   # contiguous-layout messages (version 3, class 1) whose size is that of a 95 x 95 x 5 x 5 float32 table
        if b[i - 10] == 3 and b[i - 9] == 1:
            addrs.append(struct.unpack("<Q", b[i - 8:i])[0])
        i = b.find(struct.pack("<Q", nbytes), i + 1)
    assert len(addrs) == 3, addrs
    tabs = [np.frombuffer(b, dtype="<f4", count=nbytes // 4, offset=a).reshape(95, 95, 5, 5)[:19, :19].copy()
            for a in sorted(addrs)]
    ac = json.load(open(os.path.join(REF, "torchani", "resources", "atomic_constants.json")))
    symbols = ["H", "He", "Li", "Be", "B", "C", "N", "O", "F", "Ne", "Na", "Mg", "Al", "Si", "P", "S", "Cl", "Ar"]
    np.savez_compressed(os.path.join(OUT, "d3_tables.npz"), c6=tabs[0], cn_a=tabs[1], cn_b=tabs[2], symbols=np.array(symbols),
                        covalent_radius=np.array([ac[s]["covalent_radius"] for s in symbols], dtype=np.float64),
                        sqrt_empirical_charge=np.array([ac[s]["sqrt_empirical_charge"] for s in symbols], dtype=np.float64))


def xyz_reads():
    from torchani.io import read_xyz

    with open(os.path.join(REF, "dataset", "xyz_files", "13.xyz")) as fh:
        lines = fh.read().splitlines(keepends=True)
    head, k = [], 0
    for _ in range(64):
        n = int(lines[k])
        head += lines[k:k + n + 2]
        k += n + 2
    with open(os.path.join(OUT, "13_head.xyz"), "w") as fh:
        fh.writelines(head)
    for name in ("water-0.8nm.xyz", "small.xyz"):
        shutil.copyfile(os.path.join(REF, "tests", "resources", name), os.path.join(OUT, name))
    arrays = {}
    for name in ("13_head.xyz", "water-0.8nm.xyz", "small.xyz"):
        sp, x, cell, _ = read_xyz(os.path.join(OUT, name), dtype=torch.float64)
        arrays[name + "/species"], arrays[name + "/coords"] = sp.numpy(), x.numpy()
        if cell is not None:
            arrays[name + "/cell"] = cell.numpy()
    np.savez_compressed(os.path.join(OUT, "xyz_reads.npz"), **arrays)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    import_reference()
    api()
    d3_tables()
    xyz_reads()
