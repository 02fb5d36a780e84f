"""Host-side parts of the L-BFGS geometry optimizer (no GPU): the fp64 two-loop reference of the GPU tests against dense BFGS,
argument validation before any device work, and the workspace size of the Python layer against the library's."""
import numpy as np
import pytest
import torch

from _geomopt_ref import LbfgsReference


def test_reference_equals_dense_bfgs_on_a_quadratic():
    """For its first `memory` steps L-BFGS is BFGS: p_k = -H_k g_k with H_0 = I / alpha and the dense inverse update
    H+ = (I - rho s y^T) H (I - rho y s^T) + rho s s^T, on E = x^T Q x / 2 - b^T x with Q SPD (every curvature positive)."""
    rs = np.random.RandomState(3)
    A, memory, alpha = 6, 9, 3.0
    n = 3 * A
    M = rs.randn(n, n)
    Q = M @ M.T / n + 0.5 * np.eye(n)
    b = rs.randn(n)
    x = rs.randn(n)
    ref = LbfgsReference(1, memory=memory, maxstep=1e9, alpha=alpha, damping=1.0, fmax=0.0)
    H = np.eye(n) / alpha
    x_prev = f_prev = None
    for k in range(memory + 1):
        f = b - Q @ x
        dr = ref.step(x.reshape(1, A, 3), f.reshape(1, A, 3), np.ones((1, A), dtype=bool))[0].ravel()
        if k > 0:
            s, y = x - x_prev, f_prev - f
            rho = 1.0 / (y @ s)
            V = np.eye(n) - rho * np.outer(y, s)
            H = V.T @ H @ V + rho * np.outer(s, s)
        p = H @ f
        assert np.abs(dr - p).max() <= 1e-9 * np.abs(p).max(), k
        x_prev, f_prev, x = x, f, x + dr
    assert len(ref.pairs[0]) == memory


def test_reference_skips_negative_curvature_and_scales_to_maxstep():
    ref = LbfgsReference(1, memory=3, maxstep=0.1, alpha=1.0, damping=0.5, fmax=0.0)
    act = np.ones((1, 1), dtype=bool)
    x = np.zeros((1, 1, 3))
    f = np.array([[[1.0, 0.0, 0.0]]])
    dr = ref.step(x, f, act)                                   # p = f / alpha, |p| = 1 -> scaled to 0.1, damped
    assert np.allclose(dr[0, 0], [0.05, 0.0, 0.0])
    dr = ref.step(x + dr, np.array([[[2.0, 0.0, 0.0]]]), act)  # y = f_prev - f = -1 along s: s.y < 0, not stored
    assert ref.pairs[0] == [] and np.allclose(dr[0, 0], [0.05, 0.0, 0.0])


def test_reference_freezes_converged_molecules():
    ref = LbfgsReference(2, memory=3, maxstep=0.2, alpha=1.0, damping=1.0, fmax=1e-3)
    x = np.zeros((2, 2, 3))
    f = np.zeros((2, 2, 3))
    f[1, 0, 0] = 0.5
    f[0, 1, 2] = 9.0                                            # a padding / fixed atom: masked, does not count
    dr = ref.step(x, f, np.array([[True, False], [True, True]]))
    assert ref.converged.tolist() == [True, False] and np.all(dr[0] == 0) and ref.n_steps.tolist() == [0, 1]


def _cpu_inputs():
    return torch.zeros((2, 3), dtype=torch.long), torch.zeros((2, 3, 3))


@pytest.mark.parametrize("kw, match", [({"memory": 0}, "memory"), ({"memory": 257}, "memory"), ({"maxstep": 0.0}, "maxstep"),
                                       ({"maxstep": -1.0}, "maxstep"), ({"fixed": torch.zeros(3, dtype=torch.bool)}, "fixed"),
                                       ({"fixed": torch.zeros((3, 2), dtype=torch.bool)}, "fixed")])
def test_bad_arguments_raise_before_device_work(kw, match):
    from torchani_amd.geomopt import GeometryOptimizer, optimize_geometry

    sp, x = _cpu_inputs()
    with pytest.raises(ValueError, match=match):
        GeometryOptimizer(None, sp, x, **kw)
    with pytest.raises(ValueError, match=match):
        optimize_geometry(None, sp, x, **kw)


def test_negative_fmax_and_cpu_tensors_raise():
    from torchani_amd.geomopt import GeometryOptimizer, optimize_geometry

    sp, x = _cpu_inputs()
    with pytest.raises(ValueError, match="fmax"):
        optimize_geometry(None, sp, x, fmax=-1e-3)
    with pytest.raises(ValueError, match="ROCm"):
        GeometryOptimizer(None, sp, x)
    with pytest.raises(ValueError, match=r"\[C, A, 3\]"):
        GeometryOptimizer(None, sp, x[:, :2])


def test_defaults_are_ase_lbfgs_defaults():
    from torchani_amd import geomopt, units

    assert geomopt.DEFAULT_ALPHA * units.HARTREE_TO_EV == pytest.approx(70.0)
    assert geomopt.DEFAULT_FMAX * units.HARTREE_TO_EV == pytest.approx(0.05)


def test_workspace_bytes_match_library():
    from torchani_amd import _lib
    from torchani_amd.geomopt import lbfgs_workspace_bytes

    _lib.build()
    L = _lib.lib()
    for C, A, m in [(1, 1, 1), (6, 14, 5), (256, 28, 100), (2560, 28, 100), (1, 30, 100), (1, 46357, 100), (3, 700, 256),
                    (5, 22, 17)]:
        assert L.anihip_lbfgs_workspace_bytes(C, A, m) == lbfgs_workspace_bytes(C, A, m), (C, A, m)
    assert L.anihip_lbfgs_workspace_bytes(1, 10, 0) == 0 and b"memory" in L.anihip_last_error()
    assert L.anihip_lbfgs_workspace_bytes(1, 10, _lib.LBFGS_MAX_MEMORY + 1) == 0
