"""Color-aware ILU(1) on the device: the LDS-hash pattern kernels and the
embed kernel against the host builder (exact), the ILU factor/apply kernels
on the colored pattern against the host, and MULTICOLOR_ILU level 1 end to
end in dDDI."""

import json
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu

from amgx_amd import AMGConfig, CSRMatrix, create_solver, ops
from amgx_amd.amg.coloring import MatrixColoring
from amgx_amd.config import ConfigScope
from amgx_amd.ops import cpu as cpu_ops
from amgx_amd.problems import block_laplacian, poisson_2d
from amgx_amd.resources import Resources

CONFIG = os.path.join(os.path.dirname(__file__), "..", "configs",
                      "FGMRES_ILU1_COLORED.json")


def colorings(A, level):
    """(device matrix, device coloring, the same coloring on the host)"""
    Ag = A.to("cuda:0")
    colg = MatrixColoring.create(
        Ag, ConfigScope(None, {"matrix_coloring_scheme": "MIN_MAX",
                               "coloring_level": level}))
    return Ag, colg, MatrixColoring(colg.colors.cpu(), colg.num_colors)


def assert_same_matrix(Fg, F):
    assert Fg.is_cuda and Fg.block_dim == F.block_dim
    assert Fg.n_cols == F.n_cols and Fg.dtype == F.dtype
    assert torch.equal(Fg.row_offsets.cpu(), F.row_offsets)
    assert torch.equal(Fg.col_indices.cpu(), F.col_indices)
    assert torch.equal(Fg.values.cpu(), F.values)


def arrow(n):
    """Dense first row and column plus a tridiagonal."""
    i = np.arange(1, n)
    rows = np.concatenate([np.arange(n), np.zeros(n - 1, int), i,
                           i[:-1], i[1:]])
    cols = np.concatenate([np.arange(n), i, np.zeros(n - 1, int),
                           i[1:], i[:-1]])
    vals = np.where(rows == cols, 4.0 + n, -1.0 - 1e-3 * (rows + 2 * cols))
    return CSRMatrix.from_scipy(sp.csr_matrix((vals, (rows, cols)),
                                              shape=(n, n)))


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("make", [
    lambda: poisson_2d(12, 12),
    lambda: block_laplacian(10, 10, block_dim=3)], ids=["scalar", "block3"])
def test_pattern_first_tier(make, level):
    A = make()
    Ag, colg, col = colorings(A, level)
    F = cpu_ops.ilu1_pattern(A, col)
    assert int(torch.diff(F.row_offsets).max()) <= 64
    assert_same_matrix(ops.ilu1_pattern(Ag, colg), F)


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("n,lo,hi", [(100, 64, 512), (700, 512, 8192)],
                         ids=["tier512", "top_tier"])
def test_pattern_upper_tiers(n, lo, hi, level):
    A = arrow(n)
    Ag, colg, col = colorings(A, level)
    F = cpu_ops.ilu1_pattern(A, col)
    widest = int(torch.diff(F.row_offsets).max())
    print(f"arrow n={n} coloring_level={level}: nnz {F.nnz}, widest {widest}")
    assert lo < widest <= hi
    assert_same_matrix(ops.ilu1_pattern(Ag, colg), F)


def test_pattern_overflow_falls_back_to_host():
    """A row past the top tier: the binding reports it and the device op
    returns the host builder's pattern, uploaded."""
    from amgx_amd import _core
    n = _core.ILU1_TOP_CAP + 8
    A = arrow(n)
    # row 0 eliminated last, so its width creates no fill elsewhere
    colors = torch.ones(n, dtype=torch.int32)
    colors[0] = 2
    colors[2::2] = 0
    col = MatrixColoring(colors, 3)
    Ag = A.to("cuda:0")
    colg = MatrixColoring(colors.cuda(), 3)
    ro, ci, big = _core.ilu1_pattern(Ag.row_offsets, Ag.col_indices,
                                     colg.colors, n)
    assert big.numel() == 0
    assert int(ro[0]) == -1 and ci.numel() == 0
    assert_same_matrix(ops.ilu1_pattern(Ag, colg),
                       cpu_ops.ilu1_pattern(A, col))


def test_embed_a_to_lu():
    from amgx_amd import _core
    for A in (poisson_2d(9, 7), block_laplacian(5, 6, block_dim=3)):
        Ag, colg, col = colorings(A, 2)
        bb = A.block_dim ** 2
        ro, ci, big = _core.ilu1_pattern(Ag.row_offsets, Ag.col_indices,
                                         colg.colors.to(torch.int32),
                                         A.n_rows)
        assert big.numel() == 0 and ci.numel() > A.nnz
        va, a_to_lu = _core.ilu1_embed(Ag.row_offsets, Ag.col_indices,
                                       Ag.values.reshape(-1), bb, ro, ci)
        assert a_to_lu.dtype == torch.int32 and a_to_lu.numel() == A.nnz
        slots = a_to_lu.cpu().to(torch.int64)
        assert slots.unique().numel() == A.nnz
        lu = va.cpu().view(-1, bb)
        assert torch.equal(lu[slots], A.values.reshape(-1, bb))
        rest = torch.ones(lu.shape[0], dtype=torch.bool)
        rest[slots] = False
        assert rest.sum() == ci.numel() - A.nnz
        assert (lu[rest] == 0).all()
        assert torch.equal(ci.cpu()[slots], A.col_indices)


def test_scalar_factor_and_apply():
    A = poisson_2d(12, 12)
    Ag, colg, col = colorings(A, 2)
    F = cpu_ops.ilu1_pattern(A, col)
    Fg = ops.ilu1_pattern(Ag, colg)
    lu_ref = cpu_ops.ilu0_setup(F, col)
    lu_gpu = ops._backend(Fg).ilu0_setup(Fg, colg)
    print("lu max dev", (lu_gpu.cpu() - lu_ref).abs().max().item())
    assert torch.allclose(lu_gpu.cpu(), lu_ref, rtol=1e-12, atol=1e-13)
    r = torch.rand(A.n_rows, dtype=torch.float64,
                   generator=torch.Generator().manual_seed(3))
    x1 = torch.zeros_like(r)
    x2 = x1.cuda()
    cpu_ops.ilu0_solve(F, lu_ref, col, r, x1, 1.0)
    ops._backend(Fg).ilu0_solve(Fg, lu_gpu, colg, r.cuda(), x2, 1.0)
    print("solve max dev", (x2.cpu() - x1).abs().max().item())
    assert torch.allclose(x2.cpu(), x1, rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("make,relax", [
    (lambda: block_laplacian(10, 10, block_dim=3, seed=5), 1.0),
    (lambda: block_laplacian(8, 8, block_dim=4, seed=6), 0.9)],
    ids=["b3", "b4"])
def test_block_factor_and_apply(make, relax):
    A = make()
    Ag, colg, col = colorings(A, 2)
    F = cpu_ops.ilu1_pattern(A, col)
    Fg = ops.ilu1_pattern(Ag, colg)
    assert F.nnz > A.nnz
    f_ref = cpu_ops.ilu0_setup(F, col)
    f_gpu = ops._backend(Fg).ilu0_setup(Fg, colg)
    r = torch.rand(A.n_rows * A.block_dim, dtype=torch.float64,
                   generator=torch.Generator().manual_seed(4))
    x1 = torch.zeros_like(r)
    x2 = x1.cuda()
    cpu_ops.ilu0_solve(F, f_ref, col, r, x1, relax)
    ops._backend(Fg).ilu0_solve(Fg, f_gpu, colg, r.cuda(), x2, relax)
    print("solve max dev", (x2.cpu() - x1).abs().max().item())
    assert torch.allclose(x2.cpu(), x1, rtol=1e-9, atol=1e-10)


def test_mixed_precision_factor_and_apply():
    """fp32 matrix, fp64 vectors (dDFI) against the fp64 host factors."""
    A = poisson_2d(12, 12)
    Ag, colg, col = colorings(A, 2)
    A32g = CSRMatrix(Ag.row_offsets, Ag.col_indices,
                     Ag.values.to(torch.float32), n_cols=A.n_cols)
    F = cpu_ops.ilu1_pattern(A, col)
    F32g = ops.ilu1_pattern(A32g, colg)
    assert F32g.dtype == torch.float32
    assert torch.equal(F32g.col_indices.cpu(), F.col_indices)
    assert torch.equal(F32g.values.cpu(), F.values.to(torch.float32))
    lu_ref = cpu_ops.ilu0_setup(F, col)
    lu_gpu = ops._backend(F32g).ilu0_setup(F32g, colg)
    r = torch.rand(A.n_rows, dtype=torch.float64,
                   generator=torch.Generator().manual_seed(5))
    x1 = torch.zeros_like(r)
    x2 = x1.cuda()
    cpu_ops.ilu0_solve(F, lu_ref, col, r, x1, 1.0)
    ops._backend(F32g).ilu0_solve(F32g, lu_gpu, colg, r.cuda(), x2, 1.0)
    print("solve max dev", (x2.cpu() - x1).abs().max().item())
    assert x2.dtype == torch.float64
    assert torch.allclose(x2.cpu(), x1, rtol=1e-4, atol=1e-5)


def test_block4_ilu1_end_to_end():
    A = block_laplacian(8, 8, block_dim=4, seed=6).to("cuda:0")

    def iters(level):
        with open(CONFIG) as f:
            shipped = json.load(f)
        shipped["solver"]["preconditioner"]["ilu_sparsity_level"] = level
        cfg = AMGConfig.from_dict(shipped)
        s = create_solver(cfg.root_scope(), resources=Resources("cuda:0"))
        b = torch.ones(A.n_rows * 4, dtype=torch.float64, device="cuda:0")
        x = torch.zeros_like(b)
        s.setup(A)
        st = s.solve(b, x, zero_initial_guess=True)
        rel = float(ops.nrm2(ops.residual(A, x, b)) / ops.nrm2(b))
        assert st.converged and rel < 1e-8, f"ILU({level}): {st} rel={rel}"
        return st.iterations

    it0, it1 = iters(0), iters(1)
    print(f"FGMRES iterations: ILU(0) {it0}, ILU(1) {it1}")
    assert it1 <= it0


def test_block4_ilu1_capi():
    from amgx_amd import capi as C
    P = block_laplacian(8, 8, block_dim=4, seed=6)
    n = P.n_rows
    C.AMGX_initialize()
    rc, cfg = C.AMGX_config_create_from_file(CONFIG)
    assert rc == C.RC_OK
    rc, res = C.AMGX_resources_create_simple(cfg)
    rc, m = C.AMGX_matrix_create(res, "dDDI")
    rc, bh = C.AMGX_vector_create(res, "dDDI")
    rc, xh = C.AMGX_vector_create(res, "dDDI")
    assert C.AMGX_matrix_upload_all(
        m, n, P.nnz, 4, 4, P.row_offsets.numpy(), P.col_indices.numpy(),
        P.values.numpy().reshape(-1)) == C.RC_OK
    C.AMGX_vector_upload(bh, n, 4, np.ones(n * 4))
    C.AMGX_vector_set_zero(xh, n, 4)
    rc, s = C.AMGX_solver_create(res, "dDDI", cfg)
    assert rc == C.RC_OK
    assert C.AMGX_solver_setup(s, m) == C.RC_OK
    assert C.AMGX_solver_solve(s, bh, xh) == C.RC_OK
    rc, status = C.AMGX_solver_get_status(s)
    assert rc == C.RC_OK and status == 0
    assert m.A.values.is_cuda and m.A.block_dim == 4
    rc, nrm = C.AMGX_solver_calculate_residual_norm(s, m, bh, xh)
    assert rc == C.RC_OK and nrm < 1e-8 * np.sqrt(n * 4)
