"""Host complex modes (hZZI): the dense coarse solve, DILU and aggregation
AMG in complex arithmetic. The host backend is the reference the device
complex tests compare against, so every test here also runs with numpy's
ComplexWarning and torch's UserWarning turned into errors: no path may cast
an imaginary part away."""

import warnings

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from amgx_amd import AMGConfig, CSRMatrix, create_solver
from amgx_amd.amg.coloring import MatrixColoring
from amgx_amd.ops import cpu as cpu_ops
from amgx_amd.problems import poisson_2d
from amgx_amd.resources import Resources

Z = torch.complex128
ComplexWarning = getattr(np, "ComplexWarning", None) or \
    np.exceptions.ComplexWarning


@pytest.fixture(autouse=True)
def casts_are_errors():
    with warnings.catch_warnings():
        warnings.simplefilter("error", ComplexWarning)
        warnings.simplefilter("error", UserWarning)
        yield


def shifted_poisson(nx, ny, shift):
    """poisson_2d(nx, ny) + 0.3j on the first super-diagonal - 0.2j on the
    first sub-diagonal + shift I (complex128, non-Hermitian), a manufactured
    solution and its right-hand side."""
    P = poisson_2d(nx, ny).to_scipy().astype(np.complex128)
    n = P.shape[0]
    K = sp.diags([0.3j * np.ones(n - 1), -0.2j * np.ones(n - 1)], [1, -1])
    S = (P + K + shift * sp.identity(n)).tocsr()
    S.sort_indices()
    rng = np.random.RandomState(5)
    xref = rng.randn(n) + 1j * rng.randn(n)
    return S, torch.from_numpy(xref), torch.from_numpy(S @ xref)


def solver(cfg):
    return create_solver(AMGConfig.from_dict(cfg).root_scope(),
                         resources=Resources("cpu"))


# ---------------------------------------------------------------- dense LU
def test_dense_lu_complex():
    S, _, b = shifted_poisson(8, 8, 0.5 + 0.8j)
    s = solver({"solver": "DENSE_LU_SOLVER"})
    s.setup(CSRMatrix.from_scipy(S, dtype=Z))
    assert s.Ainv.dtype == Z
    x = torch.zeros_like(b)
    s.solve(b, x, zero_initial_guess=True)
    r = b.numpy() - S @ x.numpy()
    assert np.linalg.norm(r) / np.linalg.norm(b.numpy()) < 1e-10


# ---------------------------------------------------------------- DILU
def test_dilu_against_dense_substitution():
    """Einv and one apply against M = (E + L) E^-1 (E + U) built densely:
    L / U the strict lower / upper parts in color order, E_i = a_ii -
    sum_{color(j) < color(i)} a_ij a_ji / E_j."""
    S, _, b = shifted_poisson(8, 8, 0.5 + 0.8j)
    n = S.shape[0]
    # fixed valid coloring of the 5-point stencil plus the +-1 couplings
    # that wrap a grid row: parity of (ix + iy) and of iy
    ix, iy = np.arange(n) % 8, np.arange(n) // 8
    colors = ((ix + iy) % 2) + 2 * (iy % 2)
    coloring = MatrixColoring(torch.from_numpy(colors.astype(np.int32)), 4)
    A = CSRMatrix.from_scipy(S, dtype=Z)
    assert coloring.validate(A)

    D = S.toarray()
    E = np.zeros(n, dtype=np.complex128)
    for c in range(4):
        for i in np.flatnonzero(colors == c):
            lower = np.flatnonzero((colors < c) & (D[i] != 0))
            E[i] = D[i, i] - sum(D[i, j] * D[j, i] / E[j] for j in lower)
    lo = colors[:, None] > colors[None, :]
    L, U = np.where(lo, D, 0), np.where(lo.T, D, 0)
    M = (np.diag(E) + L) @ np.diag(1 / E) @ (np.diag(E) + U)

    einv = cpu_ops.dilu_setup(A, coloring)
    assert einv.dtype == Z
    np.testing.assert_allclose(einv.numpy(), 1 / E, rtol=1e-12)

    x0 = torch.from_numpy(np.linspace(-1, 1, n) + 1j * np.linspace(2, 0.5, n))
    x = x0.clone()
    r = cpu_ops.residual(A, x, b)
    cpu_ops.dilu_solve(A, einv, coloring, r, 0.9, x)
    want = x0.numpy() + 0.9 * np.linalg.solve(M, r.numpy())
    np.testing.assert_allclose(x.numpy(), want, rtol=1e-12)


def test_dilu_rejects_coupled_rows_of_one_color():
    S, _, _ = shifted_poisson(8, 8, 0.5 + 0.8j)
    A = CSRMatrix.from_scipy(S, dtype=Z)
    one_color = MatrixColoring(torch.zeros(A.n_rows, dtype=torch.int32), 1)
    with pytest.raises(RuntimeError, match="valid distance-1 coloring"):
        cpu_ops.dilu_setup(A, one_color)


# ---------------------------------------------------------------- AMG
def amg_cfg(smoother="BLOCK_JACOBI", cycle="V", **over):
    amg = {"solver": "AMG", "algorithm": "AGGREGATION", "selector": "SIZE_2",
           "smoother": {"solver": smoother, "relaxation_factor": 0.8},
           "presweeps": 1, "postsweeps": 1, "cycle": cycle, "max_iters": 1,
           "min_coarse_rows": 8, "coarse_solver": "DENSE_LU_SOLVER"}
    amg.update(over)
    return amg


def krylov(S, b, precond):
    cfg = {"solver": "FGMRES" if precond else "GMRES", "max_iters": 300,
           "gmres_n_restart": 30, "monitor_residual": 1,
           "convergence": "RELATIVE_INI", "tolerance": 1e-10}
    if precond:
        cfg["preconditioner"] = precond
    s = solver(cfg)
    s.setup(CSRMatrix.from_scipy(S, dtype=Z))
    x = torch.zeros_like(b)
    st = s.solve(b, x, zero_initial_guess=True)
    return st, x


@pytest.fixture(scope="module")
def system40():
    S, xref, b = shifted_poisson(40, 40, 0.05 + 0.1j)
    st, _ = krylov(S, b, None)
    assert st.converged
    return S, xref, b, st.iterations


@pytest.mark.parametrize("smoother,cycle", [
    ("BLOCK_JACOBI", "V"), ("MULTICOLOR_GS", "V"), ("MULTICOLOR_DILU", "V"),
    ("BLOCK_JACOBI", "W"), ("BLOCK_JACOBI", "F")])
def test_fgmres_amg_complex(system40, smoother, cycle):
    S, xref, b, plain_iters = system40
    st, x = krylov(S, b, amg_cfg(smoother, cycle))
    print(f"{smoother} {cycle}: {st.iterations} iterations, "
          f"unpreconditioned GMRES(30) {plain_iters}")
    assert st.converged, st
    err = float(torch.linalg.vector_norm(x - xref)
                / torch.linalg.vector_norm(xref))
    assert err < 1e-7
    assert 2 * st.iterations <= plain_iters, (st.iterations, plain_iters)


# ---------------------------------------------------------------- rejections
@pytest.mark.parametrize("over", [
    {"cycle": "CG"}, {"cycle": "CGF"}, {"algorithm": "CLASSICAL"},
    {"smoother": "MULTICOLOR_ILU"}, {"smoother": "JACOBI_L1"},
    {"smoother": "CHEBYSHEV"}, {"smoother": "KACZMARZ"},
    {"error_scaling": 2}], ids=lambda o: "-".join(map(str, o.values())))
def test_out_of_scope_raises(over):
    S, _, _ = shifted_poisson(12, 12, 0.5 + 0.8j)
    s = solver(amg_cfg(**over))
    with pytest.raises((NotImplementedError, RuntimeError),
                       match="complex"):
        s.setup(CSRMatrix.from_scipy(S, dtype=Z))


def test_idr_raises():
    S, _, _ = shifted_poisson(12, 12, 0.5 + 0.8j)
    s = solver({"solver": "IDR", "max_iters": 10})
    with pytest.raises(NotImplementedError, match="IDR"):
        s.setup(CSRMatrix.from_scipy(S, dtype=Z))
