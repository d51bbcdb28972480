"""Device complex modes dZZI / dCCI / dZCI: the gfx950 complex kernels of the
Krylov + Jacobi path against the host backend (ops/cpu.py, complex128) on
the same inputs.

Pairs are (matrix, vector): (Z,Z) complex128 x complex128, (C,C) complex64 x
complex64, (C,Z) complex64 matrix x complex128 vectors. Tolerances are the
ones tests/test_gpu.py uses for the corresponding real kernels."""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu

from amgx_amd import AMGConfig, CSRMatrix, create_solver, ops
from amgx_amd.amg.coloring import MatrixColoring
from amgx_amd.ops import cpu as cpu_ops
from amgx_amd.problems import poisson_2d
from amgx_amd.resources import Resources

DEV = "cuda:0"
Z, C = torch.complex128, torch.complex64
PAIRS = {"ZZ": (Z, Z), "CC": (C, C), "CZ": (C, Z)}     # (matrix, vector)
pairs = pytest.mark.parametrize("pair", list(PAIRS))


def spmv_tol(pair):
    return dict(rtol=1e-12, atol=1e-12) if pair == "ZZ" \
        else dict(rtol=1e-5, atol=1e-6)


def jacobi_tol(pair):
    return dict(rtol=1e-12, atol=1e-12) if pair == "ZZ" \
        else dict(rtol=1e-4, atol=1e-5)


def close(got, ref, tol):
    """got (device, any complex dtype) against the complex128 host result."""
    return torch.allclose(got.cpu().to(Z), ref.to(Z), **tol)


def cvec(n, seed, shift=-0.3):
    """complex128 vector, both parts non-zero."""
    rng = np.random.RandomState(seed)
    return torch.from_numpy(rng.rand(n) + 1j * (rng.rand(n) + shift))


def rand_ccsr(n, density, seed):
    """sp.random real part + 1j * sp.random imaginary part, symmetrised,
    plus 4 I (scipy, complex128)."""
    rng = np.random.RandomState(seed)
    m = sp.random(n, n, density=density, random_state=rng, format="csr") \
        + 1j * sp.random(n, n, density=density, random_state=rng,
                         format="csr")
    m = (m + m.T + sp.identity(n) * 4.0).tocsr()
    m.sum_duplicates()
    m.sort_indices()
    return m


def on_gpu(m, mat_dtype):
    return CSRMatrix.from_scipy(m, device=DEV, dtype=mat_dtype)


N = 515          # no multiple of the 256-thread block or of a lane group
# average degree -> csrmv route: <= 16 thread-per-row, (16, 64] 8 lanes per
# row, > 64 32 lanes per row
ROUTES = {"tpr": 0.0039, "vec8": 0.0195, "vec32": 0.065}


@pytest.fixture(scope="module")
def mats():
    return {k: rand_ccsr(N, d, seed=3 + i)
            for i, (k, d) in enumerate(ROUTES.items())}


def avg_deg(m):
    return m.nnz / m.shape[0]


# ---------------------------------------------------------------- SpMV routes
def test_route_matrices_cover_all_three_kernels(mats):
    assert avg_deg(mats["tpr"]) <= 16
    assert 16 < avg_deg(mats["vec8"]) <= 64
    assert avg_deg(mats["vec32"]) > 64
    # thread-per-row: a row longer than the 8-entry peel runs the tail loop
    assert np.diff(mats["tpr"].indptr).max() > 8


@pairs
@pytest.mark.parametrize("route", list(ROUTES))
def test_spmv_routes(mats, route, pair):
    ta, tv = PAIRS[pair]
    m = mats[route]
    x = cvec(N, 1)
    assert float(x.imag.abs().min()) > 0
    ref = cpu_ops.spmv(CSRMatrix.from_scipy(m, dtype=Z), x)
    y = ops.spmv(on_gpu(m, ta), x.to(tv).to(DEV))
    assert y.dtype == tv
    assert close(y, ref, spmv_tol(pair))


# ------------------------------------------- window, coefficients, residual
@pairs
def test_spmv_window_and_complex_coefficients(mats, pair):
    ta, tv = PAIRS[pair]
    m = mats["tpr"]
    alpha, beta = 2 - 0.5j, -0.5 + 0.25j
    x, y0 = cvec(N, 2), cvec(N, 3)
    ref = y0.clone()
    cpu_ops.spmv(CSRMatrix.from_scipy(m, dtype=Z), x, ref, alpha=alpha,
                 beta=beta, row_begin=100, row_end=300)
    y0d = y0.to(tv)
    yg = y0d.to(DEV)
    ops.spmv(on_gpu(m, ta), x.to(tv).to(DEV), yg, alpha=alpha, beta=beta,
             row_begin=100, row_end=300)
    out = yg.cpu()
    assert close(yg, ref, spmv_tol(pair))
    # rows outside the window are untouched, bit for bit
    assert torch.equal(torch.view_as_real(out[:100]),
                       torch.view_as_real(y0d[:100]))
    assert torch.equal(torch.view_as_real(out[300:]),
                       torch.view_as_real(y0d[300:]))


@pairs
@pytest.mark.parametrize("route", list(ROUTES))
def test_residual(mats, route, pair):
    ta, tv = PAIRS[pair]
    m = mats[route]
    x, b = cvec(N, 4), cvec(N, 5)
    ref = cpu_ops.residual(CSRMatrix.from_scipy(m, dtype=Z), x, b)
    r = ops.residual(on_gpu(m, ta), x.to(tv).to(DEV), b.to(tv).to(DEV))
    assert close(r, ref, spmv_tol(pair))


@pairs
def test_empty_rows_give_beta_y_plus_gamma_b(mats, pair):
    from amgx_amd import _core
    ta, tv = PAIRS[pair]
    m = mats["tpr"].copy()
    empty = np.array([0, 7, 8, 255, 256, 300, N - 1])
    # zero the row_offsets spans of the chosen rows
    keep = np.ones(N)
    keep[empty] = 0.0
    m = (sp.diags(keep) @ m).tocsr()
    m.eliminate_zeros()
    m.sort_indices()
    assert (np.diff(m.indptr)[empty] == 0).all()
    alpha, beta, gamma = 1.5 + 0.5j, -0.5 + 0.25j, 0.75 - 2j
    x, y0, b = cvec(N, 6), cvec(N, 7), cvec(N, 8)
    ref = alpha * (m @ x.numpy()) + beta * y0.numpy() + gamma * b.numpy()
    A = on_gpu(m, ta)
    yg = y0.to(tv).to(DEV)
    _core.csrmv(A.row_offsets, A.col_indices, A.values, 1, x.to(tv).to(DEV),
                yg, b.to(tv).to(DEV), alpha, beta, gamma, 0, N)
    assert close(yg, torch.from_numpy(ref), spmv_tol(pair))
    want = torch.from_numpy((beta * y0.numpy() + gamma * b.numpy())[empty])
    assert close(yg[torch.as_tensor(empty, device=DEV)], want, spmv_tol(pair))


# ---------------------------------------------------------------- reductions
RED_N = [1, 63, 257, 300001]    # the last one > NPART * 256 = 262144: the
                                # grid-stride loop takes a second trip


def red_bound(dtype, scale):
    """|device - host| bound. complex128: rtol 1e-12 of the result (the bound
    of the real fp64 reductions). complex64 (left to this test): the
    reduction adds at most 2 elements per thread and then 18 tree levels, so
    the sum carries at most ~20 roundings, each <= eps32 * sum|terms|; 32
    eps32 * sum|terms| bounds it."""
    if dtype == Z:
        return 1e-12 * scale["result"]
    return 32 * float(torch.finfo(torch.float32).eps) * scale["terms"]


@pytest.mark.parametrize("dtype", [Z, C], ids=["Z", "C"])
@pytest.mark.parametrize("n", RED_N)
def test_reductions(n, dtype):
    # independent x, y; the shifts give Im(conj(x).y) a non-zero mean
    x, y = cvec(n, 10).to(dtype), cvec(n, 11, shift=0.5).to(dtype)
    x64, y64 = x.to(Z), y.to(Z)          # same (rounded) inputs on the host
    xg, yg = x.to(DEV), y.to(DEV)

    ref = complex(torch.vdot(x64, y64))
    swapped = complex(torch.vdot(y64, x64))
    terms = float((x64.abs() * y64.abs()).sum())
    tol = red_bound(dtype, {"result": abs(ref), "terms": terms})
    got = ops.dot(xg, yg)
    assert isinstance(got, complex)
    assert abs(got - ref) <= tol, (got, ref)
    # conj(x).y, not conj(y).x: the swapped product must miss the tolerance
    assert abs(swapped - ref) > tol
    assert abs(got - swapped) > tol

    for name in ("nrm2", "nrm1", "nrmmax"):
        want = getattr(cpu_ops, name)(x64)
        val = getattr(ops, name)(xg)
        assert isinstance(val, float)
        if name == "nrm2":
            # sqrt halves the relative error of the squared sum
            bound = red_bound(dtype, {"result": want, "terms": want})
        else:
            bound = red_bound(dtype, {"result": want,
                                      "terms": float(x64.abs().sum())})
        assert abs(val - want) <= bound, (name, val, want)
        assert val >= 0.0

    # <x, x> is exactly real; every reduction is bitwise reproducible
    d = ops.dot(xg, xg)
    assert d.imag == 0.0 and d.real >= 0.0
    assert ops.dot(xg, yg) == got
    for name in ("nrm2", "nrm1", "nrmmax"):
        assert getattr(ops, name)(xg) == getattr(ops, name)(xg)


def test_reduce_op_result_dtypes():
    from amgx_amd import _core
    from amgx_amd.ops import gpu as gpu_ops
    for dtype, real in ((Z, torch.float64), (C, torch.float32)):
        x = cvec(100, 12).to(dtype).to(DEV)
        for op, want in ((0, dtype), (1, real), (2, real), (3, real)):
            out = _core.reduce_op(x, x if op == 0 else None, op)
            assert out.dtype == want and out.shape == (1,)
        with pytest.raises(TypeError):
            gpu_ops.dot_async(x, x)         # device-scalar path is real-only


# ---------------------------------------------------------------- BLAS-1
@pytest.mark.parametrize("dtype", [Z, C], ids=["Z", "C"])
@pytest.mark.parametrize("coefs", [(0.7 - 1.3j, -0.4 + 0.9j), (0.7, -0.4)],
                         ids=["complex", "real"])
def test_blas1(dtype, coefs):
    a, b = coefs
    tol = dict(rtol=1e-12, atol=1e-12) if dtype == Z \
        else dict(rtol=1e-5, atol=1e-6)
    n = 1000
    x, y = cvec(n, 13), cvec(n, 14)

    def dev(v):
        return v.to(dtype).to(DEV).clone()   # the ops update in place

    got = ops.axpy(dev(y), dev(x), a)
    assert close(got, cpu_ops.axpy(y.clone(), x, a), tol)
    got = ops.axpby(dev(y), dev(x), a, b)
    assert close(got, cpu_ops.axpby(y.clone(), x, a, b), tol)
    got = ops.scal(dev(x), a)
    assert close(got, cpu_ops.scal(x.clone(), a), tol)


# ---------------------------------------------------------------- Jacobi
@pairs
def test_jacobi(mats, pair):
    ta, tv = PAIRS[pair]
    m = mats["tpr"].copy()
    row = slice(m.indptr[17], m.indptr[18])
    k = m.indptr[17] + int(np.flatnonzero(m.indices[row] == 17)[0])
    m.data[k] = 0.0                      # stays stored: the |d| == 0 guard
    Ah = CSRMatrix.from_scipy(m, dtype=Z)
    Ag = on_gpu(m, ta)
    tol = jacobi_tol(pair)

    dg = ops.extract_diagonal(Ag)
    assert dg.dtype == ta
    assert close(dg, cpu_ops.extract_diagonal(Ah), tol)

    dinv_h = cpu_ops.jacobi_dinv(Ah)
    dinv_g = ops.jacobi_dinv(Ag)
    assert dinv_g.dtype == ta
    assert close(dinv_g, dinv_h, tol)
    assert complex(dinv_g[17].cpu()) == 1.0

    b, x = cvec(N, 15), cvec(N, 16)
    ref = cpu_ops.jacobi_smooth(Ah, dinv_h, b, x, torch.zeros_like(x), 0.9)
    xo = torch.zeros(N, dtype=tv, device=DEV)
    ops.jacobi_smooth(Ag, dinv_g, b.to(tv).to(DEV), x.to(tv).to(DEV), xo, 0.9)
    assert close(xo, ref, tol)

    with pytest.raises(NotImplementedError, match="JACOBI_L1"):
        ops.jacobi_dinv(Ag, l1=True)


# ---------------------------------------------------------------- rejections
def test_unsupported_pairs_and_kernels_raise(mats):
    m = mats["tpr"]
    Ag = on_gpu(m, Z)
    xr = torch.rand(N, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.spmv(Ag, xr)                                  # complex x real
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.spmv(on_gpu(m.real.tocsr(), torch.float64),   # real x complex
                 cvec(N, 17).to(DEV))
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.spmv(Ag, cvec(N, 17).to(C).to(DEV))           # Z matrix x C vector
    coloring = MatrixColoring(torch.zeros(N, dtype=torch.int32, device=DEV), 1)
    with pytest.raises(RuntimeError):
        ops.dilu_setup(Ag, coloring)


# ---------------------------------------------------------------- solvers
def helmholtz_like():
    """S = poisson_2d(12, 12) + K + (0.5 + 0.8j) I, K = 0.3j on the first
    super-diagonal and -0.2j on the first sub-diagonal: n = 144,
    non-Hermitian."""
    P = poisson_2d(12, 12).to_scipy().astype(np.complex128)
    n = P.shape[0]
    K = sp.diags([0.3j * np.ones(n - 1), -0.2j * np.ones(n - 1)], [1, -1])
    S = (P + K + (0.5 + 0.8j) * sp.identity(n)).tocsr()
    rng = np.random.RandomState(5)
    xref = rng.randn(n) + 1j * rng.randn(n)
    return S, torch.from_numpy(xref), torch.from_numpy(S @ xref)


BJ = {"solver": "BLOCK_JACOBI", "max_iters": 1}      # one sweep per apply
CONFIGS = {
    "GMRES": {"solver": "GMRES"},
    "FGMRES_BJ": {"solver": "FGMRES", "preconditioner": BJ},
    "BICGSTAB": {"solver": "BICGSTAB"},
    "PBICGSTAB_BJ": {"solver": "PBICGSTAB", "preconditioner": BJ},
    "PCG_BJ": {"solver": "PCG", "preconditioner": BJ},
}


def run(cfg_name, S, b, device, ta, tv, tolerance, restart=30):
    cfg = dict(CONFIGS[cfg_name], max_iters=300, gmres_n_restart=restart,
               monitor_residual=1, convergence="RELATIVE_INI",
               tolerance=tolerance)
    s = create_solver(AMGConfig.from_dict(cfg).root_scope(),
                      resources=Resources(device))
    A = CSRMatrix.from_scipy(S, device=device, dtype=ta)
    bd = b.to(tv).to(device)
    x = torch.zeros_like(bd)
    s.setup(A)
    st = s.solve(bd, x, zero_initial_guess=True)
    return st, x.cpu().to(Z)


def rel_err(x, xref):
    return float(torch.linalg.vector_norm(x - xref)
                 / torch.linalg.vector_norm(xref))


@pytest.mark.parametrize("cfg_name", ["GMRES", "FGMRES_BJ", "BICGSTAB",
                                      "PBICGSTAB_BJ"])
def test_solvers_complex128(cfg_name):
    S, xref, b = helmholtz_like()
    st_h, _ = run(cfg_name, S, b, "cpu", Z, Z, 1e-10)
    st_d, x_d = run(cfg_name, S, b, DEV, Z, Z, 1e-10)
    assert st_h.converged
    assert st_d.converged, st_d
    assert rel_err(x_d, xref) < 1e-7
    # only the reduction order differs from the host run
    assert abs(st_d.iterations - st_h.iterations) <= 1, (st_d, st_h)


def test_pcg_hermitian_positive_definite():
    """The matrix of test_complex_mode_cg_and_gmres, PCG + BLOCK_JACOBI."""
    rng = np.random.RandomState(11)
    n = 60
    B = sp.random(n, n, density=0.06, random_state=rng, format="csr")
    Cm = sp.random(n, n, density=0.06, random_state=rng, format="csr")
    M = B + 1j * Cm
    H = ((M + M.conj().T) * 0.5 + sp.identity(n) * 8.0).tocsr()
    xref = torch.from_numpy(rng.randn(n) + 1j * rng.randn(n))
    b = torch.from_numpy(H @ xref.numpy())
    st_h, _ = run("PCG_BJ", H, b, "cpu", Z, Z, 1e-10, restart=40)
    st_d, x_d = run("PCG_BJ", H, b, DEV, Z, Z, 1e-10, restart=40)
    assert st_h.converged
    assert st_d.converged, st_d
    assert rel_err(x_d, xref) < 1e-7
    assert abs(st_d.iterations - st_h.iterations) <= 1, (st_d, st_h)


@pytest.mark.parametrize("pair", ["CC", "CZ"])
@pytest.mark.parametrize("cfg_name", ["GMRES", "PBICGSTAB_BJ"])
def test_solvers_complex64_and_mixed(cfg_name, pair):
    ta, tv = PAIRS[pair]
    S, _, b = helmholtz_like()

    def true_res(x):
        r = b.numpy() - S @ x.numpy()
        return float(np.linalg.norm(r) / np.linalg.norm(b.numpy()))

    st_h, x_h = run(cfg_name, S, b, "cpu", ta, tv, 1e-5)
    st_d, x_d = run(cfg_name, S, b, DEV, ta, tv, 1e-5)
    assert st_h.converged
    assert st_d.converged, st_d
    res_h, res_d = true_res(x_h), true_res(x_d)
    print(f"{cfg_name} {pair}: true residual host {res_h:.3e} "
          f"device {res_d:.3e}")
    # both stop on the same recurrence tolerance; a conjugation or sign
    # error leaves an O(1) residual
    assert res_d <= 10 * res_h, (res_d, res_h)


# ---------------------------------------------------------------- API
def test_capi_dZZI():
    """test_complex_mode_capi's 4x4 system with device handles."""
    from amgx_amd import capi as A

    def solve(mode):
        A.AMGX_initialize()
        rc, cfg = A.AMGX_config_create(
            "config_version=2, solver=PCG, preconditioner=BLOCK_JACOBI,"
            " max_iters=300, tolerance=1e-10, convergence=RELATIVE_INI,"
            " monitor_residual=1")
        assert rc == A.RC_OK
        rc, res = A.AMGX_resources_create_simple(cfg)
        assert rc == A.RC_OK
        rc, m = A.AMGX_matrix_create(res, mode)
        assert rc == A.RC_OK
        n = 4
        ro = [0, 2, 4, 6, 8]
        ci = [0, 1, 0, 1, 2, 3, 2, 3]
        va = np.asarray([4.0, 1 - 1j, 1 + 1j, 4.0, 5.0, 2j, -2j, 5.0],
                        dtype=np.complex128)
        assert A.AMGX_matrix_upload_all(m, n, 8, 1, 1, ro, ci, va) == A.RC_OK
        rc, bh = A.AMGX_vector_create(res, mode)
        assert rc == A.RC_OK
        rc, xh = A.AMGX_vector_create(res, mode)
        assert rc == A.RC_OK
        rhs = np.asarray([1 + 0.5j, -1j, 2.0, 0.25 - 0.75j])
        assert A.AMGX_vector_upload(bh, n, 1, rhs) == A.RC_OK
        assert A.AMGX_vector_upload(xh, n, 1,
                                    np.zeros(n, dtype=np.complex128)) == A.RC_OK
        rc, s = A.AMGX_solver_create(res, mode, cfg)
        assert rc == A.RC_OK
        assert A.AMGX_solver_setup(s, m) == A.RC_OK
        assert A.AMGX_solver_solve(s, bh, xh) == A.RC_OK
        rc, nrm = A.AMGX_solver_calculate_residual_norm(s, m, bh, xh)
        assert rc == A.RC_OK and nrm < 1e-8
        rc, out = A.AMGX_vector_download(xh)
        assert rc == A.RC_OK
        return m, xh, out

    m, xh, x_dev = solve("dZZI")
    assert m.A.values.is_cuda and m.A.values.dtype == Z
    assert xh.v.is_cuda
    assert np.iscomplexobj(x_dev)
    _, _, x_host = solve("hZZI")
    assert np.abs(x_dev - x_host).max() <= 1e-10
