"""Golden fixtures for constant sets OFF the published models' on the grid sizes the tuned kernels take (16 radial shifts,
8 x 4 or 4 x 8 angular terms), from the REFERENCE's ``AEVComputer.from_constants`` (aev/_computer.py:602-666, pyaev
strategy, float64): AEV rows, the vector-Jacobian product of a seeded cotangent and the forward-mode derivative J t.  The
sets and geometries are those of tests/_aev_constants.py (GOLDEN_RUNS): one boundary set, the 4 x 8 grid with Zeta = 1 and
Rca = Rcr.  The reference's computer accepts Rca = Rcr when it is built but refuses to evaluate it (aev/_computer.py:233
asserts Rca < Rcr in forward), so that fixture is written with Rca one fp32 step below Rcr -- the closest the reference
speaks to; the fixture holds the constants it was written with, and no pair of its geometry lies between the two values.
Run only where /root/reference exists; the *.npz are committed.

    python tests/golden/gen_golden_tuned_constants.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as gg  # noqa: E402,F401  (stubs h5py / zarr and puts /root/reference on the path)

import torch  # noqa: E402
from torchani.aev import AEVComputer  # noqa: E402

import _aev_constants as kc  # noqa: E402
from gen_golden_fgrads import direction  # noqa: E402


def save(run, seed):
    cset, geom = kc.set_by_name(run[0]), kc.geometry_of(run)
    if cset.Rca == cset.Rcr:
        cset = cset._replace(Rca=float(np.nextafter(np.float32(cset.Rca), np.float32(0.0))))
    aevc = AEVComputer.from_constants(cset.Rcr, cset.Rca, cset.EtaR, list(cset.ShfR), cset.EtaA, cset.Zeta, list(cset.ShfA),
                                      list(cset.ShfZ), cset.num_species, cutoff_fn=cset.cutoff_fn,
                                      neighborlist="all_pairs").double()
    sp = torch.as_tensor(geom.species, dtype=torch.long)
    x = torch.as_tensor(geom.coords).double().requires_grad_(True)
    cell_t = None if geom.cell is None else torch.as_tensor(geom.cell).double()
    pbc_t = None if geom.pbc is None else torch.as_tensor(geom.pbc, dtype=torch.bool)
    aev = aevc(sp, x, cell_t, pbc_t)
    w = np.random.RandomState(seed).uniform(-1.0, 1.0, tuple(aev.shape)).astype(np.float32)   # (fp32-representable)
    (vjp,) = torch.autograd.grad((aev * torch.as_tensor(w.astype(np.float64))).sum(), x)
    C, A = geom.species.shape
    t = torch.as_tensor(direction(C, A)) * (sp >= 0).unsqueeze(-1)
    _, jt = torch.autograd.functional.jvp(lambda y: aevc(sp, y, cell_t, pbc_t), x.detach(), t)
    f32 = lambda v: np.asarray(v, dtype=np.float32)   # noqa: E731  (the table's constants are fp32 values already)
    out = dict(num_species=np.asarray(cset.num_species), Rcr=f32(cset.Rcr), Rca=f32(cset.Rca), EtaR=f32(cset.EtaR),
               ShfR=f32(cset.ShfR), EtaA=f32(cset.EtaA), Zeta=f32(cset.Zeta), ShfA=f32(cset.ShfA), ShfZ=f32(cset.ShfZ),
               cutoff_fn=np.asarray(cset.cutoff_fn), species=geom.species.astype(np.int32), coords=geom.coords,
               aev=aev.detach().numpy(), cotangent=w, aev_vjp=vjp.numpy(), aev_jvp=jt.detach().numpy())
    if geom.cell is not None:
        out["cell"] = np.asarray(geom.cell, dtype=np.float32)
        out["pbc"] = np.asarray(geom.pbc, dtype=bool)
    path = os.path.join(HERE, f"grid_tuned_{run[0]}.npz")
    np.savez_compressed(path, **out)
    print(f"grid_tuned_{run[0]} on {run[1]}: L={aev.shape[-1]} |aev|max={np.abs(out['aev']).max():.3f} "
          f"|vjp|max={np.abs(out['aev_vjp']).max():.3f} -> {os.path.getsize(path) / 1024:.0f} KiB")


def main():
    torch.set_num_threads(8)
    for k, run in enumerate(kc.GOLDEN_RUNS):
        save(run, 201 + k)


if __name__ == "__main__":
    main()
