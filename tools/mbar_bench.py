"""Time per self-consistent MBAR iteration (anihip_mbar_iterate, csrc/mbar.hip) beside the same iteration written with
torch.logsumexp on a materialised reduced-potential matrix.

    python tools/mbar_bench.py [--states 256] [--log2-samples 20] [--dense-log2-samples 18] [--repeats 7] [--out profiles/mbar_bench.txt]

Umbrella-like problems: K windows on R distance columns at one temperature, samples drawn around the window centres.  Every timing
is a pair of device events around ``--iterations`` iterations queued in one call (kernel) or one after the other (torch), after a
warm-up of the same call: the median with the fastest and the slowest of ``--repeats``.  Pairs per second counts K N (state,
sample) pairs per iteration.  The share of the fp64 vector peak (78.6 TFLOP/s, half the 157.3 TFLOP/s fp32 vector peak of the
MI355X) counts, per pair and iteration, three evaluations of u (one in launch 1, two in launch 2) of 8 R + 2 operations each
(subtract, absolute value, subtract, maximum, three multiplies and an add per column; an add and a multiply for beta (E + bias)),
five more additions and subtractions, and two exp counted as ONE operation each: it is a lower bound of the arithmetic done, an
fp64 exp being some twenty instructions.  The lines are printed and written to --out."""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_VECTOR_PEAK = 78.6e12


def timed(fn, repeats):
    """ms per call by device events: (median, fastest, slowest) after one warm call."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), min(ts), max(ts)


def problem(K, R, N, dev):
    from torchani_amd import md

    g = torch.Generator().manual_seed(K + R + N)
    centers = 3.0 + 2.5 * torch.rand((K, R), generator=g, dtype=torch.float64)
    states = md.ThermodynamicStates(300.0, centers, 0.05)
    window = torch.arange(N) % K
    cv = (centers[window] + 0.15 * torch.randn((N, R), generator=g, dtype=torch.float64)).to(dev)
    n_k = torch.bincount(window, minlength=K)
    return states, n_k, cv


def torch_iteration(u, ln_n, f):
    d = torch.logsumexp(ln_n[:, None] + f[:, None] - u, dim=0)
    new = -torch.logsumexp(-u - d[None, :], dim=1)
    return new - new[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=256)
    ap.add_argument("--log2-samples", type=int, default=20)
    ap.add_argument("--dense-log2-samples", type=int, default=18)
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mbar_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mbar_bench needs the GPU"
    from torchani_amd import _lib, md
    from torchani_amd.engine import _stream

    dev = torch.device("cuda:0")
    K, it = args.states, args.iterations
    lines = [f"mbar_bench: K = {K}, {it} iterations per timed call, {args.repeats} repeats, device events; median (fastest .. slowest)"]

    def report(what, K, R, N, ms):
        per = [t / it for t in ms]
        pairs = K * N / (per[0] * 1e-3)
        ops = 3 * (8 * R + 2) + 5 + 2
        lines.append(f"{what:<34} N = 2^{int(np.log2(N)):<2} R = {R}: {per[0]:8.3f} ms / iteration ({per[1]:.3f} .. {per[2]:.3f}), "
                     f"{pairs:.3e} pairs/s, {ops} counted operations per pair = {100.0 * pairs * ops / FP64_VECTOR_PEAK:.1f} % of "
                     "the fp64 vector peak")
        print(lines[-1], flush=True)

    def run_kernel(m):
        def fn():
            _lib.check(_lib.lib().anihip_mbar_iterate(_stream(), C.byref(m._problem), m.f.data_ptr(), it, m.f.data_ptr(),
                                                      m._delta.data_ptr(), m._workspace.data_ptr(), m._workspace.numel()))
        return timed(fn, args.repeats)

    def run_torch(u, n_k):
        ln_n = n_k.double().log().to(dev)
        state = {"f": torch.zeros(u.shape[0], dtype=torch.float64, device=dev)}

        def fn():
            for _ in range(it):
                state["f"] = torch_iteration(u, ln_n, state["f"])
        return timed(fn, args.repeats)

    for R in (1, 2):
        for log2n in sorted({args.dense_log2_samples, args.log2_samples}):
            N = 1 << log2n
            states, n_k, cv = problem(K, R, N, dev)
            m = md.MBAR(states, n_k, cv)
            report("structured kernel", K, R, N, run_kernel(m))
            if R == 1:
                u = torch.empty((K, N), dtype=torch.float64, device=dev)
                rows = states.restraint.to(dev)
                for k in range(K):   # (row by row: no second N x K temporary)
                    u[k] = states.beta[k] * 0.5 * rows[k, 0, 1] * (cv[:, 0] - rows[k, 0, 0]) ** 2
                if log2n == args.dense_log2_samples:
                    dense = md.MBAR.from_reduced_potentials(u, n_k)
                    report("dense kernel", K, R, N, run_kernel(dense))
                    gap = float((dense.f - m.f).abs().max())
                    lines.append(f"    dense and structured f after {it * (args.repeats + 1)} iterations differ by at most {gap:.1e}")
                    print(lines[-1], flush=True)
                    del dense
                try:
                    report("torch.logsumexp, matrix held", K, R, N, run_torch(u, n_k))
                except torch.OutOfMemoryError:
                    lines.append(f"torch.logsumexp, matrix held        N = 2^{log2n}: out of memory")
                    print(lines[-1], flush=True)
                del u
            del m, cv
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
