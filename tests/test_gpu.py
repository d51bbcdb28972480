"""GPU numerics tests: every gfx950 kernel vs the plain CPU/scipy fp64
reference (same op, same inputs)."""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu

from amgx_amd import AMGConfig, CSRMatrix, create_solver, ops
from amgx_amd.amg.coloring import MatrixColoring
from amgx_amd.resources import Resources
from amgx_amd.problems import poisson_2d, poisson_3d, block_laplacian


def to_gpu(A):
    return A.to("cuda:0")


def rand_csr(n=500, density=0.02, seed=3):
    rng = np.random.RandomState(seed)
    m = sp.random(n, n, density=density, random_state=rng, format="csr")
    m = m + m.T + sp.identity(n) * 4.0
    m = m.tocsr()
    m.sum_duplicates()
    m.sort_indices()
    return CSRMatrix.from_scipy(m)


def test_native_extension_loaded():
    """The HIP extension must be the running path on GPU machines."""
    from amgx_amd import _core
    assert hasattr(_core, "csrmv")


def test_mfma4_fragment_layout():
    """Validates the v_mfma_f64_4x4x4f64 fragment layout decoded on
    hardware (profiles/mfma_discover.py 64x64 one-hot probe) and assumed by
    kernels_mfma.hip: blocks interleaved by quads —
    A[b][m][k] at lane 16k+4b+m, B[b][k][n] at 16k+4b+n,
    C[b][m][n] at 16m+4b+n."""
    from amgx_amd import _core
    g = torch.Generator().manual_seed(7)
    Am = torch.rand(4, 4, 4, generator=g, dtype=torch.float64)  # per block
    Bm = torch.rand(4, 4, 4, generator=g, dtype=torch.float64)
    a_frag = torch.empty(64, dtype=torch.float64)
    b_frag = torch.empty(64, dtype=torch.float64)
    for lane in range(64):
        blk = (lane // 4) % 4
        outer = lane // 16
        inner = lane % 4
        a_frag[lane] = Am[blk][inner][outer]   # A[b][m=inner][k=outer]
        b_frag[lane] = Bm[blk][outer][inner]   # B[b][k=outer][n=inner]
    c_frag = _core.mfma4_probe(a_frag.cuda(), b_frag.cuda()).cpu()
    C = torch.einsum("bmk,bkn->bmn", Am, Bm)
    got = torch.empty_like(C)
    for lane in range(64):
        blk = (lane // 4) % 4
        got[blk][lane // 16][lane % 4] = c_frag[lane]   # C[b][m=o][n=inner]
    assert torch.allclose(got, C, atol=1e-12), \
        f"MFMA layout mismatch:\nexpected {C[0]}\ngot {got[0]}"


def test_spmv_scalar():
    A = rand_csr()
    x = torch.rand(A.n_rows, dtype=torch.float64)
    ref = ops.spmv(A, x)
    Ag = to_gpu(A)
    y = ops.spmv(Ag, x.cuda())
    assert torch.allclose(y.cpu(), ref, rtol=1e-12, atol=1e-12)


def test_spmv_window_and_beta():
    A = rand_csr()
    x = torch.rand(A.n_rows, dtype=torch.float64)
    y0 = torch.rand(A.n_rows, dtype=torch.float64)
    ref = y0.clone()
    ops.spmv(A, x, ref, alpha=2.0, beta=-0.5, row_begin=100, row_end=300)
    yg = y0.cuda()
    ops.spmv(to_gpu(A), x.cuda(), yg, alpha=2.0, beta=-0.5,
             row_begin=100, row_end=300)
    assert torch.allclose(yg.cpu(), ref, rtol=1e-12, atol=1e-12)


def test_spmv_block():
    A = block_laplacian(10, 8, block_dim=4)
    x = torch.rand(A.n_rows * 4, dtype=torch.float64)
    ref = ops.spmv(A, x)
    y = ops.spmv(to_gpu(A), x.cuda())
    assert torch.allclose(y.cpu(), ref, rtol=1e-12, atol=1e-12)


def test_spmv_block_all_sizes():
    """Generic wave bsrmv (b=2..8, coalesced block loads + shuffle folds)
    against the CPU reference."""
    for b in (2, 3, 5, 6, 7, 8):
        A = block_laplacian(9, 7, block_dim=b, seed=b)
        x = torch.rand(A.n_rows * b, dtype=torch.float64)
        ref = ops.spmv(A, x)
        y = ops.spmv(to_gpu(A), x.cuda())
        assert torch.allclose(y.cpu(), ref, rtol=1e-12, atol=1e-12), b
        # alpha/beta path
        y0 = torch.rand(A.n_rows * b, dtype=torch.float64)
        r1 = y0.clone()
        ops.spmv(A, x, r1, alpha=1.5, beta=-0.25)
        r2 = y0.cuda()
        ops.spmv(to_gpu(A), x.cuda(), r2, alpha=1.5, beta=-0.25)
        assert torch.allclose(r2.cpu(), r1, rtol=1e-12, atol=1e-12), b


def test_residual_and_reductions():
    A = rand_csr()
    x = torch.rand(A.n_rows, dtype=torch.float64)
    b = torch.rand(A.n_rows, dtype=torch.float64)
    r_ref = ops.residual(A, x, b)
    Ag = to_gpu(A)
    r = ops.residual(Ag, x.cuda(), b.cuda())
    assert torch.allclose(r.cpu(), r_ref, rtol=1e-12, atol=1e-12)
    assert np.isclose(ops.nrm2(r), ops.nrm2(r_ref), rtol=1e-12)
    assert np.isclose(ops.nrm1(r), ops.nrm1(r_ref), rtol=1e-12)
    assert np.isclose(ops.nrmmax(r), ops.nrmmax(r_ref), rtol=1e-12)
    assert np.isclose(ops.dot(r, r), ops.dot(r_ref, r_ref), rtol=1e-12)


RED_N = [1, 63, 257, 300001]    # the last one > NPART * 256 = 262144: the
                                # grid-stride loop takes a second trip


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32],
                         ids=["fp64", "fp32"])
@pytest.mark.parametrize("n", RED_N)
def test_real_reductions(n, dtype):
    """dot / nrm2 / nrm1 / nrmmax on signed data against the host backend in
    fp64 on the same (rounded) inputs. Bound, as derived at red_bound in
    test_gpu_complex.py: the reduction adds at most 2 elements per thread and
    then 18 tree levels, about 20 roundings of at most eps * sum|terms| each,
    so 32 eps * sum|terms|; the square root halves the relative error of
    nrm2, so 32 eps * nrm2 bounds it as well."""
    from amgx_amd.ops import cpu as cpu_ops, gpu as gpu_ops
    g = torch.Generator().manual_seed(1000 + n)
    x = torch.randn(n, generator=g, dtype=torch.float64).to(dtype)
    y = torch.randn(n, generator=g, dtype=torch.float64).to(dtype)
    x64, y64 = x.double(), y.double()
    xg, yg = x.cuda(), y.cuda()
    eps = float(torch.finfo(dtype).eps)

    want = {"dot": cpu_ops.dot(x64, y64), "nrm2": cpu_ops.nrm2(x64),
            "nrm1": cpu_ops.nrm1(x64), "nrmmax": cpu_ops.nrmmax(x64)}
    bound = {"dot": 32 * eps * float((x64.abs() * y64.abs()).sum()),
             "nrm2": 32 * eps * want["nrm2"],
             "nrm1": 32 * eps * want["nrm1"],
             "nrmmax": 0.0}

    def run():
        return {"dot": ops.dot(xg, yg), "nrm2": ops.nrm2(xg),
                "nrm1": ops.nrm1(xg), "nrmmax": ops.nrmmax(xg)}

    got = run()
    for name, val in got.items():
        print(f"{name} n={n} {dtype}: got {val!r} want {want[name]!r} "
              f"err {abs(val - want[name]):.3e} bound {bound[name]:.3e}")
        assert isinstance(val, float)
        assert abs(val - want[name]) <= bound[name], (name, val, want[name])
    assert got == run()                     # bitwise reproducible

    d = gpu_ops.dot_async(xg, yg)
    assert d.is_cuda and d.shape == (1,) and d.dtype == dtype
    assert float(d.item()) == got["dot"]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32,
                                   torch.complex128, torch.complex64],
                         ids=["fp64", "fp32", "Z", "C"])
def test_reduce_op_rejects_unknown_ops_and_lengths(dtype):
    from amgx_amd import _core
    x = torch.ones(100, dtype=dtype, device="cuda:0")
    # op 3 (sum|x|^2) exists for complex x only; op 4 for nobody
    for op in ((4,) if dtype.is_complex else (3, 4)):
        with pytest.raises(RuntimeError, match="unknown op"):
            _core.reduce_op(x, None, op)
    with pytest.raises(RuntimeError, match="differ in length"):
        _core.reduce_op(x, x[:99], 0)


def test_blas1():
    x = torch.rand(10000, dtype=torch.float64)
    y = torch.rand(10000, dtype=torch.float64)
    xg, yg = x.cuda(), y.cuda()
    ops.axpy(y, x, 0.7)
    ops.axpy(yg, xg, 0.7)
    assert torch.allclose(yg.cpu(), y, rtol=1e-14)
    ops.axpby(y, x, 1.3, -0.2)
    ops.axpby(yg, xg, 1.3, -0.2)
    assert torch.allclose(yg.cpu(), y, rtol=1e-13)


def test_diag_and_jacobi():
    A = rand_csr()
    Ag = to_gpu(A)
    assert torch.equal(Ag.diag_index().cpu(), A.diag_index())
    assert torch.allclose(Ag.diagonal().cpu(), A.diagonal())
    for l1 in (False, True):
        dref = ops.jacobi_dinv(A, l1=l1)
        dg = ops.jacobi_dinv(Ag, l1=l1)
        assert torch.allclose(dg.cpu(), dref, rtol=1e-12), f"l1={l1}"
    b = torch.rand(A.n_rows, dtype=torch.float64)
    x = torch.rand(A.n_rows, dtype=torch.float64)
    out_ref = torch.zeros_like(x)
    out_g = torch.zeros_like(x).cuda()
    ops.jacobi_smooth(A, dref, b, x, out_ref, 0.8)
    ops.jacobi_smooth(Ag, dg, b.cuda(), x.cuda(), out_g, 0.8)
    assert torch.allclose(out_g.cpu(), out_ref, rtol=1e-12, atol=1e-13)


def test_jacobi_block():
    A = block_laplacian(8, 8, block_dim=4)
    Ag = to_gpu(A)
    dref = ops.jacobi_dinv(A)
    dg = ops.jacobi_dinv(Ag)
    assert torch.allclose(dg.cpu(), dref.to(dg.dtype), rtol=1e-10, atol=1e-12)
    n = A.n_rows * 4
    b = torch.rand(n, dtype=torch.float64)
    x = torch.rand(n, dtype=torch.float64)
    o1, o2 = torch.zeros_like(x), torch.zeros_like(x).cuda()
    ops.jacobi_smooth(A, dref, b, x, o1, 0.8)
    ops.jacobi_smooth(Ag, dg, b.cuda(), x.cuda(), o2, 0.8)
    assert torch.allclose(o2.cpu(), o1, rtol=1e-10, atol=1e-12)


def test_coloring_valid_gpu():
    A = to_gpu(poisson_2d(50, 40))
    col = MatrixColoring.create(A)
    assert col.validate(A)
    assert col.num_colors <= 12
    assert sum(col.bounds[c + 1] - col.bounds[c]
               for c in range(col.num_colors)) == A.n_rows


def test_gs_sweep_matches_cpu():
    # same coloring on both devices => identical sweep order => same numbers
    A = poisson_2d(20, 20)
    Ag = to_gpu(A)
    colg = MatrixColoring.create(Ag)
    col_cpu = MatrixColoring(colg.colors.cpu(), colg.num_colors)
    dinv = ops.jacobi_dinv(A)
    b = torch.ones(A.n_rows, dtype=torch.float64)
    x1 = torch.zeros(A.n_rows, dtype=torch.float64)
    x2 = x1.clone().cuda()
    ops.gs_sweep(A, dinv, b, x1, col_cpu, 1.0)
    ops.gs_sweep(Ag, ops.jacobi_dinv(Ag), b.cuda(), x2, colg, 1.0)
    assert torch.allclose(x2.cpu(), x1, rtol=1e-12, atol=1e-13)


def test_dilu_matches_cpu():
    A = poisson_2d(16, 16)
    Ag = to_gpu(A)
    colg = MatrixColoring.create(Ag)
    col_cpu = MatrixColoring(colg.colors.cpu(), colg.num_colors)
    e_ref = ops.dilu_setup(A, col_cpu)
    e_gpu = ops.dilu_setup(Ag, colg)
    assert torch.allclose(e_gpu.cpu(), e_ref, rtol=1e-12, atol=1e-13)
    r = torch.rand(A.n_rows, dtype=torch.float64)
    x1 = torch.zeros(A.n_rows, dtype=torch.float64)
    x2 = x1.clone().cuda()
    ops.dilu_solve(A, e_ref, col_cpu, r, 0.9, x1)
    ops.dilu_solve(Ag, e_gpu, colg, r.cuda(), 0.9, x2)
    assert torch.allclose(x2.cpu(), x1, rtol=1e-11, atol=1e-12)


def test_dilu_block_gpu():
    A = block_laplacian(8, 8, block_dim=4)
    Ag = to_gpu(A)
    colg = MatrixColoring.create(Ag)
    col_cpu = MatrixColoring(colg.colors.cpu(), colg.num_colors)
    e_ref = ops.dilu_setup(A, col_cpu)
    e_gpu = ops.dilu_setup(Ag, colg)
    assert torch.allclose(e_gpu.cpu(), e_ref, rtol=1e-9, atol=1e-11)
    r = torch.rand(A.n_rows * 4, dtype=torch.float64)
    x1 = torch.zeros_like(r)
    x2 = x1.clone().cuda()
    ops.dilu_solve(A, e_ref, col_cpu, r, 1.0, x1)
    ops.dilu_solve(Ag, e_gpu, colg, r.cuda(), 1.0, x2)
    assert torch.allclose(x2.cpu(), x1, rtol=1e-9, atol=1e-11)


def test_size2_and_galerkin():
    A = poisson_2d(30, 30)
    Ag = to_gpu(A)
    agg, nc = ops.size2_matching(Ag)
    agg_c = agg.cpu().numpy()
    assert agg_c.min() >= 0 and agg_c.max() == nc - 1
    assert A.n_rows // 4 <= nc <= A.n_rows * 3 // 4
    Ac = ops.galerkin_aggregation(Ag, agg, nc)
    n = A.n_rows
    P = sp.csr_matrix((np.ones(n), (np.arange(n), agg_c)), shape=(n, nc))
    ref = (P.T @ A.to_scipy() @ P).toarray()
    assert np.allclose(Ac.to_scipy().toarray(), ref, rtol=1e-12, atol=1e-12)


def test_galerkin_block_gpu():
    A = block_laplacian(10, 10, block_dim=3)
    Ag = to_gpu(A)
    agg, nc = ops.size2_matching(Ag)
    Ac = ops.galerkin_aggregation(Ag, agg, nc)
    ref = (__import__("amgx_amd.ops.cpu", fromlist=["cpu"])
           .galerkin_aggregation(A, agg.cpu(), nc))
    assert np.allclose(Ac.to_scipy().toarray(), ref.to_scipy().toarray(),
                       rtol=1e-12, atol=1e-12)


def test_restrict_prolongate_gpu():
    A = to_gpu(poisson_2d(20, 20))
    agg, nc = ops.size2_matching(A)
    r = torch.rand(A.n_rows, dtype=torch.float64, device="cuda")
    rc = ops.restrict_agg(r, agg, nc)
    P = sp.csr_matrix((np.ones(A.n_rows),
                       (np.arange(A.n_rows), agg.cpu().numpy())),
                      shape=(A.n_rows, nc))
    assert np.allclose(rc.cpu().numpy(), P.T @ r.cpu().numpy())
    x = torch.zeros(A.n_rows, dtype=torch.float64, device="cuda")
    xc = torch.rand(nc, dtype=torch.float64, device="cuda")
    ops.prolongate_agg(x, xc, agg)
    assert np.allclose(x.cpu().numpy(), P @ xc.cpu().numpy())


def test_spgemm_transpose_gpu():
    A = rand_csr(300, seed=1)
    B = rand_csr(300, seed=2)
    Ag, Bg = to_gpu(A), to_gpu(B)
    C = ops.spgemm(Ag, Bg)
    ref = (A.to_scipy() @ B.to_scipy()).toarray()
    assert np.allclose(C.to_scipy().toarray(), ref, rtol=1e-12, atol=1e-12)
    At = ops.transpose(Ag)
    assert np.allclose(At.to_scipy().toarray(), A.to_scipy().T.toarray())


def test_dense_lu_gpu():
    A = poisson_2d(8, 8)
    cfg = AMGConfig.from_dict({"solver": "DENSE_LU_SOLVER"})
    s = create_solver(cfg.root_scope(), resources=Resources("cuda:0"))
    Ag = to_gpu(A)
    s.setup(Ag)
    b = torch.rand(A.n_rows, dtype=torch.float64, device="cuda")
    x = torch.zeros_like(b)
    s.solve(b, x)
    r = ops.residual(Ag, x, b)
    assert ops.nrm2(r) < 1e-10


def _solve_gpu(cfg_dict, A, tol=1e-6):
    cfg = AMGConfig.from_dict(cfg_dict)
    s = create_solver(cfg.root_scope(), resources=Resources("cuda:0"))
    b = torch.ones(A.n_rows * A.block_dim, dtype=A.dtype, device=A.device)
    x = torch.zeros_like(b)
    s.setup(A)
    st = s.solve(b, x, zero_initial_guess=True)
    rel = ops.nrm2(ops.residual(A, x, b)) / ops.nrm2(b)
    return st, rel


def test_fgmres_agg_poisson3d_gpu():
    from tests.test_amg import FGMRES_AGG
    A = to_gpu(poisson_3d(24, 24, 24))
    st, rel = _solve_gpu(FGMRES_AGG, A)
    assert st.converged and rel < 1e-5
    assert st.iterations <= 30


def test_pcg_amg_gpu():
    cfg = {
        "solver": {
            "preconditioner": {
                "solver": "AMG", "algorithm": "AGGREGATION",
                "smoother": "MULTICOLOR_GS", "presweeps": 1, "postsweeps": 1,
                "max_iters": 1, "min_coarse_rows": 32, "cycle": "V",
            },
            "solver": "PCG", "max_iters": 100, "monitor_residual": 1,
            "convergence": "RELATIVE_INI", "tolerance": 1e-8,
        }
    }
    A = to_gpu(poisson_3d(16, 16, 16))
    st, rel = _solve_gpu(cfg, A, tol=1e-8)
    assert st.converged and rel < 1e-7


def test_block_jacobi_pcg_gpu():
    A = to_gpu(block_laplacian(12, 12, block_dim=4))
    cfg = {"solver": {"solver": "PCG", "preconditioner": "BLOCK_JACOBI",
                      "max_iters": 500, "monitor_residual": 1,
                      "tolerance": 1e-8, "convergence": "RELATIVE_INI"}}
    st, rel = _solve_gpu(cfg, A)
    assert st.converged and rel < 1e-6


def test_classical_setup_gpu():
    """GPU strength/PMIS/D1 against the host reference semantics."""
    from amgx_amd.ops import cpu as cpu_ops
    A = poisson_2d(20, 20)
    Ag = to_gpu(A)
    Sg = ops._backend(Ag).strength_ahat(Ag, 0.25, 1.1)
    S_ref = cpu_ops.strength_ahat(A, 0.25, 1.1)
    assert torch.equal(Sg.cpu().bool(), S_ref)
    cf_g, nc_g = ops._backend(Ag).pmis_select(Ag, Sg)
    # PMIS tie-breaking differs host/device; check structural validity:
    cf = cf_g.cpu().numpy()
    assert 0 < nc_g < A.n_rows
    assert (np.sort(cf[cf >= 0]) == np.arange(nc_g)).all()
    # every F point with strong connections has a strong C neighbor
    Pg = ops._backend(Ag).interp_d1(Ag, Sg, cf_g, nc_g)
    rowsum = np.asarray(Pg.to_scipy().sum(axis=1)).ravel()
    assert np.allclose(rowsum[cf >= 0], 1.0)
    # full classical PCG solve on GPU
    from tests.test_amg import PCG_CLASSICAL
    A3 = to_gpu(poisson_3d(12, 12, 12))
    st, rel = _solve_gpu(PCG_CLASSICAL, A3, tol=1e-6)
    assert st.converged and rel < 1e-5


def test_ilu0_gpu_matches_cpu():
    from amgx_amd.ops import cpu as cpu_ops
    from amgx_amd.amg.coloring import MatrixColoring
    A = poisson_2d(12, 12)
    Ag = to_gpu(A)
    colg = MatrixColoring.create(Ag)
    col_cpu = MatrixColoring(colg.colors.cpu(), colg.num_colors)
    lu_ref = cpu_ops.ilu0_setup(A, col_cpu)
    lu_gpu = ops._backend(Ag).ilu0_setup(Ag, colg)
    assert torch.allclose(lu_gpu.cpu(), lu_ref, rtol=1e-12, atol=1e-13)
    r = torch.rand(A.n_rows, dtype=torch.float64)
    x1 = torch.zeros(A.n_rows, dtype=torch.float64)
    x2 = x1.clone().cuda()
    cpu_ops.ilu0_solve(A, lu_ref, col_cpu, r, x1, 1.0)
    ops._backend(Ag).ilu0_solve(Ag, lu_gpu, colg, r.cuda(), x2, 1.0)
    assert torch.allclose(x2.cpu(), x1, rtol=1e-11, atol=1e-12)


def test_ilu0_block_gpu_matches_cpu():
    """Device block ILU(0) (kernels_classical.hip block path) against the
    host block reference (close ops/gpu.py guard)."""
    from amgx_amd.ops import cpu as cpu_ops
    from amgx_amd.amg.coloring import MatrixColoring
    A = block_laplacian(10, 10, block_dim=3, seed=5)
    Ag = to_gpu(A)
    colg = MatrixColoring.create(Ag)
    col_cpu = MatrixColoring(colg.colors.cpu(), colg.num_colors)
    f_ref = cpu_ops.ilu0_setup(A, col_cpu)
    f_gpu = ops._backend(Ag).ilu0_setup(Ag, colg)
    r = torch.rand(A.n_rows * 3, dtype=torch.float64)
    x1 = torch.zeros_like(r)
    x2 = x1.clone().cuda()
    cpu_ops.ilu0_solve(A, f_ref, col_cpu, r, x1, 1.0)
    ops._backend(Ag).ilu0_solve(Ag, f_gpu, colg, r.cuda(), x2, 1.0)
    assert torch.allclose(x2.cpu(), x1, rtol=1e-9, atol=1e-10), \
        f"max dev {(x2.cpu() - x1).abs().max()}"
    # b=4 as well (no MFMA in ILU yet, but the dispatch must be correct)
    A4 = block_laplacian(8, 8, block_dim=4, seed=6)
    A4g = to_gpu(A4)
    c4g = MatrixColoring.create(A4g)
    c4 = MatrixColoring(c4g.colors.cpu(), c4g.num_colors)
    fr = cpu_ops.ilu0_setup(A4, c4)
    fg = ops._backend(A4g).ilu0_setup(A4g, c4g)
    r4 = torch.rand(A4.n_rows * 4, dtype=torch.float64)
    y1 = torch.zeros_like(r4)
    y2 = y1.clone().cuda()
    cpu_ops.ilu0_solve(A4, fr, c4, r4, y1, 0.9)
    ops._backend(A4g).ilu0_solve(A4g, fg, c4g, r4.cuda(), y2, 0.9)
    assert torch.allclose(y2.cpu(), y1, rtol=1e-9, atol=1e-10)


def test_fgmres_ilu0_gpu():
    cfg = {"solver": {"solver": "FGMRES", "preconditioner": "MULTICOLOR_ILU",
                      "gmres_n_restart": 20, "max_iters": 200,
                      "monitor_residual": 1, "tolerance": 1e-8,
                      "convergence": "RELATIVE_INI"}}
    A = to_gpu(poisson_3d(12, 12, 12))
    st, rel = _solve_gpu(cfg, A)
    assert st.converged and rel < 1e-6


def test_hipgraph_cycle_matches_eager():
    """The graph-captured V-cycle must give the same FGMRES iteration count
    as the eager path (the capture self-validates; on mismatch it falls back,
    so equality of iteration counts is the end-to-end check)."""
    from tests.test_amg import FGMRES_AGG
    import copy
    A = to_gpu(poisson_3d(20, 20, 20))
    iters = {}
    for use_graph in (0, 1):
        cfg_d = copy.deepcopy(FGMRES_AGG)
        cfg_d["solver"]["preconditioner"]["use_hip_graph"] = use_graph
        cfg = AMGConfig.from_dict(cfg_d)
        s = create_solver(cfg.root_scope(), resources=Resources("cuda:0"))
        b = torch.ones(A.n_rows, dtype=torch.float64, device="cuda")
        x = torch.zeros_like(b)
        s.setup(A)
        st = s.solve(b, x, zero_initial_guess=True)
        assert st.converged
        iters[use_graph] = st.iterations
    assert iters[0] == iters[1], iters


def test_classical_pcg_full_gpu():
    """Full classical solve (PMIS+D1 kernels at setup, color-GS at solve)."""
    cfg = {
        "solver": {
            "preconditioner": {
                "solver": "AMG", "algorithm": "CLASSICAL",
                "smoother": "MULTICOLOR_GS", "presweeps": 1, "postsweeps": 1,
                "max_iters": 1, "min_coarse_rows": 16, "cycle": "V",
            },
            "solver": "PCG", "max_iters": 100, "monitor_residual": 1,
            "convergence": "RELATIVE_INI", "tolerance": 1e-8,
        }
    }
    A = to_gpu(poisson_3d(16, 16, 16))
    st, rel = _solve_gpu(cfg, A, tol=1e-8)
    assert st.converged and rel < 1e-7


def test_d2_setup_stays_on_device():
    """Device-resident D2 interpolation (VERDICT r01 item 7 done-criterion):
    audit that building P from a device matrix performs no device->host
    tensor transfer (monkeypatched Tensor.cpu/.numpy counters)."""
    from amgx_amd.amg.classical import (SELECTOR_REGISTRY, STRENGTH_REGISTRY,
                                        INTERP_REGISTRY)
    from amgx_amd.config import ConfigScope
    A = to_gpu(poisson_3d(10, 10, 10))
    scope = ConfigScope(None, {"strength_threshold": 0.25})
    S = STRENGTH_REGISTRY["AHAT"](A, scope)
    cf, nc = SELECTOR_REGISTRY["PMIS"](A, S, scope)
    transfers = []
    orig_cpu = torch.Tensor.cpu

    def audit_cpu(self, *a, **k):
        if self.is_cuda:
            transfers.append(self.shape)
        return orig_cpu(self, *a, **k)

    torch.Tensor.cpu = audit_cpu
    try:
        P = INTERP_REGISTRY["D2"](A, S, cf, nc, scope)
    finally:
        torch.Tensor.cpu = orig_cpu
    assert P.values.is_cuda
    assert not transfers, f"D2 setup pulled tensors to host: {transfers[:5]}"
    # MULTIPASS: item-count syncs are fine, no bulk transfers
    cf2, nc2 = SELECTOR_REGISTRY["AGGRESSIVE_PMIS"](A, S, scope)
    transfers.clear()
    torch.Tensor.cpu = audit_cpu
    try:
        P2 = INTERP_REGISTRY["MULTIPASS"](A, S, cf2, nc2, scope)
    finally:
        torch.Tensor.cpu = orig_cpu
    assert P2.values.is_cuda
    big = [s for s in transfers if len(s) and int(torch.tensor(s).prod()) > 4]
    assert not big, f"MULTIPASS setup pulled tensors to host: {big[:5]}"


def test_classical_d2_and_aggressive_gpu():
    """Host-pass components (D2 interp, aggressive PMIS) drive a GPU solve:
    tensors must land back on device and converge."""
    for overrides in ({"interpolator": "D2"},
                      {"aggressive_levels": 1,
                       "aggressive_interpolator": "MULTIPASS"},
                      {"selector": "HMIS"}):
        node = {
            "preconditioner": {
                "solver": "AMG", "algorithm": "CLASSICAL",
                "smoother": "MULTICOLOR_GS", "presweeps": 1, "postsweeps": 1,
                "max_iters": 1, "min_coarse_rows": 16, "cycle": "V",
            },
            "solver": "PCG", "max_iters": 100, "monitor_residual": 1,
            "convergence": "RELATIVE_INI", "tolerance": 1e-8,
        }
        node["preconditioner"].update(overrides)
        A = to_gpu(poisson_3d(12, 12, 12))
        st, rel = _solve_gpu({"solver": node}, A, tol=1e-8)
        assert st.converged and rel < 1e-7, f"{overrides}: {st}"


def test_block4_dilu_fgmres_gpu():
    """Block-4 DILU on device (BASELINE config #4 single-GPU shape)."""
    A = to_gpu(block_laplacian(12, 12, block_dim=4))
    cfg = {"solver": {
        "preconditioner": {"solver": "MULTICOLOR_DILU", "max_iters": 2,
                           "relaxation_factor": 1.0, "scope": "dilu"},
        "solver": "FGMRES", "max_iters": 200, "gmres_n_restart": 30,
        "monitor_residual": 1, "convergence": "RELATIVE_INI",
        "tolerance": 1e-8,
    }}
    st, rel = _solve_gpu(cfg, A, tol=1e-8)
    assert st.converged and rel < 1e-7


def test_coloring_schemes_gpu():
    """Host coloring schemes attach to device matrices; MIN_MAX runs the
    gfx950 kernel."""
    from amgx_amd.amg.coloring import COLORING_REGISTRY
    A = to_gpu(poisson_3d(8, 8, 4))
    for scheme in ("MIN_MAX", "PARALLEL_GREEDY", "MULTI_HASH",
                   "MIN_MAX_2RING"):
        cfg = AMGConfig.from_dict({"solver": {
            "solver": "MULTICOLOR_GS", "matrix_coloring_scheme": scheme}})
        col = MatrixColoring.create(A, cfg.root_scope())
        assert col.colors.device.type == "cuda"
        assert col.validate(A, level=2 if "2RING" in scheme else 1)


def test_eigensolver_gpu():
    from amgx_amd.config import ConfigScope
    from amgx_amd.eigensolvers import create_eigensolver
    A = to_gpu(poisson_2d(16, 16))
    es = create_eigensolver(ConfigScope(None, {"eig_solver": "LANCZOS",
                                               "eig_max_iters": 300,
                                               "eig_tolerance": 1e-8}),
                            resources=Resources("cuda:0"))
    es.setup(A)
    st = es.solve()
    # dense reference
    dense = A.to("cpu").to_scipy().toarray()
    lam_ref = float(np.linalg.eigvalsh(dense).max())
    assert st.converged
    assert abs(st.eigenvalues[-1] - lam_ref) < 1e-5 * abs(lam_ref)


def test_binary_io_gpu(tmp_path):
    from amgx_amd.io.binary import read_system_binary, write_system_binary
    A = to_gpu(poisson_3d(6, 6, 6))
    b = torch.rand(A.n_rows, dtype=torch.float64, device="cuda:0")
    p = str(tmp_path / "sys.bin")
    write_system_binary(p, A, b, None)
    A2, b2, _ = read_system_binary(p, device="cuda:0")
    assert A2.row_offsets.device.type == "cuda"
    assert torch.allclose(b2, b)
    y1 = ops.spmv(A, b)
    y2 = ops.spmv(A2, b2)
    assert torch.allclose(y1, y2)


def test_ilu1_gpu():
    """ILU(1) extended-pattern factorization through the gfx950 ILU kernels
    matches CPU and preconditions FGMRES."""
    from amgx_amd.problems import poisson_2d
    A = to_gpu(poisson_2d(12, 12))
    cfg = {"solver": {
        "preconditioner": {"solver": "MULTICOLOR_ILU", "max_iters": 1,
                           "ilu_sparsity_level": 1, "scope": "ilu"},
        "solver": "FGMRES", "max_iters": 120, "gmres_n_restart": 30,
        "monitor_residual": 1, "convergence": "RELATIVE_INI",
        "tolerance": 1e-9,
    }}
    st, rel = _solve_gpu(cfg, A, tol=1e-9)
    assert st.converged and rel < 1e-8


def test_poisson_3d_device_assembly():
    """On-device Poisson assembly matches the host construction."""
    from amgx_amd.problems import poisson_3d, poisson_3d_local_device
    Ah = poisson_3d(6, 5, 4)
    Ad = poisson_3d(6, 5, 4, device="cuda:0")
    assert Ad.row_offsets.device.type == "cuda"
    assert torch.equal(Ad.row_offsets.cpu(), Ah.row_offsets)
    assert torch.equal(Ad.col_indices.cpu(), Ah.col_indices)
    assert torch.allclose(Ad.values.cpu(), Ah.values)
    ro, cols, vals, rs = poisson_3d_local_device(4, 4, 4, 0, 1,
                                                 device="cuda:0")
    A2 = poisson_3d(4, 4, 4)
    assert torch.equal(ro.cpu().to(torch.int32), A2.row_offsets)
    assert torch.equal(cols.cpu().to(torch.int32), A2.col_indices)


def test_determinism_gpu():
    """Two identical GPU setups+solves produce bitwise-identical results
    (deterministic reductions/sorts; reference determinism_flag)."""
    from amgx_amd.utils import DeterminismChecker

    def run():
        from tests.test_amg import FGMRES_AGG
        A = to_gpu(poisson_3d(12, 12, 12))
        cfg = AMGConfig.from_dict(FGMRES_AGG)
        s = create_solver(cfg.root_scope(), resources=Resources("cuda:0"))
        b = torch.ones(A.n_rows, dtype=torch.float64, device="cuda:0")
        x = torch.zeros_like(b)
        s.setup(A)
        s.solve(b, x, zero_initial_guess=True)
        chk = DeterminismChecker()
        h = s.precond.hierarchy
        for i, lvl in enumerate(h.levels):
            chk.checkpoint(f"level{i}", lvl.A.row_offsets, lvl.A.col_indices,
                           lvl.A.values)
            sm = getattr(lvl, "smoother", None)
            einv = getattr(sm, "Einv", None)
            einv = getattr(einv, "einv", einv)   # DiluState unwrap
            if einv is not None:
                chk.checkpoint(f"einv{i}", einv)
            col = getattr(lvl.A, "coloring", None)
            if col is not None:
                chk.checkpoint(f"colors{i}", col.colors)
        st = s.status
        res = torch.tensor(st.residuals[:8] if st.residuals else [0.0])
        chk.checkpoint("res_head", res)
        chk.checkpoint("x", x)
        return chk

    c1, c2 = run(), run()
    assert c1.same_as(c2), c1.diff(c2)[:6]


def test_truncate_rows_gpu():
    """GPU factor truncation matches the host reference (drop + row-sum
    rescale; reference src/truncate.cu truncateAndScale_kernel)."""
    from amgx_amd.ops import cpu as cpu_ops
    from amgx_amd.ops import gpu as gpu_ops
    A = rand_csr(300, 0.04, seed=9)
    ref = cpu_ops.truncate_rows(A, trunc_factor=0.4)
    got = gpu_ops.truncate_rows(to_gpu(A), trunc_factor=0.4)
    assert torch.equal(got.row_offsets.cpu(), ref.row_offsets)
    assert torch.equal(got.col_indices.cpu(), ref.col_indices)
    assert torch.allclose(got.values.cpu(), ref.values, atol=1e-13)
    # device top-k cap (interp_max_elements) vs the host stable-argsort ref
    for tf, me in ((0.0, 3), (0.2, 4), (0.4, 2)):
        ref = cpu_ops.truncate_rows(A, trunc_factor=tf, max_elements=me)
        got = gpu_ops.truncate_rows(to_gpu(A), trunc_factor=tf,
                                    max_elements=me)
        assert torch.equal(got.row_offsets.cpu(), ref.row_offsets), (tf, me)
        assert torch.equal(got.col_indices.cpu(), ref.col_indices), (tf, me)
        assert torch.allclose(got.values.cpu(), ref.values, atol=1e-13)


def test_wf_cycles_gpu():
    """W and F cycles on device converge (reference src/cycles/)."""
    for cyc in ("W", "F", "CG"):
        cfg = {"solver": {
            "preconditioner": {
                "solver": "AMG", "algorithm": "AGGREGATION",
                "smoother": "BLOCK_JACOBI", "presweeps": 1, "postsweeps": 1,
                "max_iters": 1, "min_coarse_rows": 16, "cycle": cyc,
            },
            "solver": "PCG", "max_iters": 100, "monitor_residual": 1,
            "convergence": "RELATIVE_INI", "tolerance": 1e-8,
        }}
        A = to_gpu(poisson_3d(10, 10, 10))
        st, rel = _solve_gpu(cfg, A, tol=1e-8)
        assert st.converged and rel < 1e-7, f"{cyc}: {st}"


def test_structure_reuse_gpu():
    """Resetup on device keeps hierarchy structure, updates values."""
    cfg = AMGConfig.from_dict({"solver": {
        "preconditioner": {
            "solver": "AMG", "algorithm": "AGGREGATION",
            "smoother": "BLOCK_JACOBI", "max_iters": 1,
            "min_coarse_rows": 16, "cycle": "V",
            "structure_reuse_levels": -1, "scope": "amg",
        },
        "solver": "PCG", "max_iters": 100, "monitor_residual": 1,
        "convergence": "RELATIVE_INI", "tolerance": 1e-8,
    }})
    A = to_gpu(poisson_3d(8, 8, 8))
    s = create_solver(cfg.root_scope(), resources=Resources("cuda:0"))
    b = torch.ones(A.n_rows, dtype=torch.float64, device="cuda:0")
    x = torch.zeros_like(b)
    s.setup(A)
    st1 = s.solve(b, x, zero_initial_guess=True)
    h1 = s.precond.hierarchy
    A2 = CSRMatrix(A.row_offsets, A.col_indices, A.values * 2.0,
                   n_cols=A.n_cols)
    s.resetup(A2)
    assert s.precond.hierarchy is h1
    x2 = torch.zeros_like(b)
    st2 = s.solve(b, x2, zero_initial_guess=True)
    assert st1.converged and st2.converged
    assert torch.allclose(x2, x / 2.0, atol=1e-6)


def test_scaler_gpu():
    """Scaler lifecycle on device: matrix restored after solve."""
    cfg = AMGConfig.from_dict({"solver": {
        "solver": "PCG", "max_iters": 200, "monitor_residual": 1,
        "convergence": "RELATIVE_INI", "tolerance": 1e-8,
        "scaling": "BINORMALIZATION",
        "preconditioner": {"solver": "BLOCK_JACOBI", "max_iters": 1},
    }})
    A = to_gpu(poisson_3d(8, 8, 8))
    vals_before = A.values.clone()
    s = create_solver(cfg.root_scope(), resources=Resources("cuda:0"))
    b = torch.ones(A.n_rows, dtype=torch.float64, device="cuda:0")
    x = torch.zeros_like(b)
    s.setup(A)
    st = s.solve(b, x, zero_initial_guess=True)
    assert st.converged
    assert torch.allclose(A.values, vals_before, atol=1e-12)
    r = ops.residual(A, x, b)
    assert float(torch.linalg.vector_norm(r)) < 1e-5


def test_kaczmarz_gpu():
    """Kaczmarz color sweeps on device: error-norm contraction (the method
    is GS on A*A^T, so its rate goes with cond(A)^2 — the residual 2-norm is
    NOT a fast-contraction metric for it) and bitwise parity with the CPU
    path under the same distance-2 schedule."""
    import numpy as np

    from amgx_amd.config import ConfigScope
    A = to_gpu(poisson_2d(12, 12))
    s = create_solver(ConfigScope(None, {"solver": "KACZMARZ",
                                         "max_iters": 20,
                                         "relaxation_factor": 1.0}),
                      resources=Resources("cuda:0"))
    b = torch.ones(A.n_rows, dtype=torch.float64, device="cuda:0")
    x = torch.zeros_like(b)
    s.setup(A)
    s.solve(b, x)
    # error norm must strictly decrease (Kaczmarz is monotone in ||e|| for
    # omega in (0,2) on consistent systems)
    xstar = np.linalg.solve(A.to("cpu").to_scipy().toarray(),
                            np.ones(A.n_rows))
    e0 = np.linalg.norm(xstar)
    e1 = np.linalg.norm(xstar - x.cpu().numpy())
    assert e1 < 0.99 * e0, f"{e1} !< 0.99*{e0}"
    # CPU cross-check with identical config
    Ah = A.to("cpu")
    sh = create_solver(ConfigScope(None, {"solver": "KACZMARZ",
                                          "max_iters": 20,
                                          "relaxation_factor": 1.0}),
                       resources=Resources("cpu"))
    bh = torch.ones(Ah.n_rows, dtype=torch.float64)
    xh = torch.zeros_like(bh)
    sh.setup(Ah)
    sh.solve(bh, xh)
    assert torch.allclose(x.cpu(), xh, atol=1e-10)


def test_mixed_precision_kernels_gpu():
    """dDFI device kernels: fp32 matrix x fp64 vectors against the fp64 CPU
    reference (csrmv, GS sweep, DILU apply, dense GEMV)."""
    from amgx_amd.ops import cpu as cpu_ops
    A64 = poisson_2d(16, 16)
    A32g = CSRMatrix(A64.row_offsets, A64.col_indices,
                     A64.values.to(torch.float32),
                     n_cols=A64.n_cols).to("cuda:0")
    x = torch.rand(A64.n_rows, dtype=torch.float64)
    # csrmv
    y = ops.spmv(A32g, x.cuda())
    assert y.dtype == torch.float64
    ref = ops.spmv(A64, x)
    assert torch.allclose(y.cpu(), ref, rtol=1e-5, atol=1e-6)
    # GS sweep (same coloring both sides)
    colg = MatrixColoring.create(A32g)
    col_cpu = MatrixColoring(colg.colors.cpu(), colg.num_colors)
    dg = ops.jacobi_dinv(A32g)
    assert dg.dtype == torch.float32
    b = torch.ones(A64.n_rows, dtype=torch.float64)
    xg = torch.zeros(A64.n_rows, dtype=torch.float64, device="cuda")
    xr = torch.zeros(A64.n_rows, dtype=torch.float64)
    ops.gs_sweep(A32g, dg, b.cuda(), xg, colg, 1.0)
    cpu_ops.gs_sweep(A64, cpu_ops.jacobi_dinv(A64), b, xr, col_cpu, 1.0)
    assert torch.allclose(xg.cpu(), xr, rtol=1e-4, atol=1e-5)
    # DILU apply
    eg = ops.dilu_setup(A32g, colg)
    r = torch.rand(A64.n_rows, dtype=torch.float64)
    w1 = torch.zeros(A64.n_rows, dtype=torch.float64)
    w2 = w1.clone().cuda()
    e_ref = cpu_ops.dilu_setup(A64, col_cpu)
    cpu_ops.dilu_solve(A64, e_ref, col_cpu, r, 0.9, w1)
    ops.dilu_solve(A32g, eg, colg, r.cuda(), 0.9, w2)
    assert torch.allclose(w2.cpu(), w1, rtol=1e-4, atol=1e-5)


def test_mixed_precision_solve_gpu():
    """dDFI end-to-end on device: FGMRES + aggregation AMG with an fp32
    hierarchy and fp64 vectors converges to 1e-6."""
    from tests.test_amg import FGMRES_AGG
    import copy
    A64 = poisson_3d(16, 16, 16)
    A = CSRMatrix(A64.row_offsets, A64.col_indices,
                  A64.values.to(torch.float32),
                  n_cols=A64.n_cols).to("cuda:0")
    cfg_d = copy.deepcopy(FGMRES_AGG)
    cfg_d["solver"]["tolerance"] = 1e-6
    cfg = AMGConfig.from_dict(cfg_d)
    s = create_solver(cfg.root_scope(), resources=Resources("cuda:0"))
    b = torch.ones(A.n_rows, dtype=torch.float64, device="cuda")
    x = torch.zeros_like(b)
    s.setup(A)
    st = s.solve(b, x, zero_initial_guess=True)
    rel = ops.nrm2(ops.residual(A, x, b)) / ops.nrm2(b)
    assert st.converged and rel < 1e-5, (st, rel)


def test_all_smoothers_gpu():
    """Every registered smoother reduces the Poisson residual ON DEVICE
    (catches any silently host-bound path)."""
    from amgx_amd.config import ConfigScope
    A = to_gpu(poisson_2d(14, 14))
    for name in ("BLOCK_JACOBI", "JACOBI_L1", "GS", "MULTICOLOR_GS",
                 "FIXCOLOR_GS", "MULTICOLOR_DILU", "MULTICOLOR_ILU",
                 "CHEBYSHEV", "CHEBYSHEV_POLY", "POLYNOMIAL",
                 "KPZ_POLYNOMIAL", "KACZMARZ", "CF_JACOBI"):
        s = create_solver(ConfigScope(None, {"solver": name,
                                             "max_iters": 12}),
                          resources=Resources("cuda:0"))
        b = torch.ones(A.n_rows, dtype=torch.float64, device="cuda")
        x = torch.zeros_like(b)
        s.setup(A)
        r0 = ops.nrm2(ops.residual(A, x, b))
        s.solve(b, x)
        r1 = ops.nrm2(ops.residual(A, x, b))
        if name == "KACZMARZ":
            # GS on A*A^T: rate goes with cond(A)^2, so the residual only
            # creeps down — assert no blow-up plus error contraction
            # (test_kaczmarz_gpu checks the error norm properly)
            assert r1 < 1.5 * r0, f"{name}: {r1} blow-up vs {r0}"
        else:
            assert r1 < 0.8 * r0, f"{name}: {r1} !< 0.8*{r0}"


def test_eigensolvers_gpu_more():
    """POWER_ITERATION and LOBPCG on device against the dense reference."""
    from amgx_amd.config import ConfigScope
    from amgx_amd.eigensolvers import create_eigensolver
    A = to_gpu(poisson_2d(12, 12))
    dense = A.to("cpu").to_scipy().toarray()
    evs = np.linalg.eigvalsh(dense)
    es = create_eigensolver(ConfigScope(None, {
        "eig_solver": "POWER_ITERATION", "eig_max_iters": 4000,
        "eig_tolerance": 1e-8}), resources=Resources("cuda:0"))
    es.setup(A)
    st = es.solve()
    assert st.converged
    assert abs(st.eigenvalues[-1] - evs[-1]) < 1e-4 * evs[-1]
    es = create_eigensolver(ConfigScope(None, {
        "eig_solver": "LOBPCG", "eig_max_iters": 400,
        "eig_tolerance": 1e-7}), resources=Resources("cuda:0"))
    es.setup(A)
    st = es.solve()
    assert st.converged
    assert abs(st.eigenvalues[0] - evs[0]) < 1e-4 * abs(evs[0])


def test_nccl_world1_smoke():
    """RCCL-backend smoke at world_size=1 on one GPU: init_process_group
    with the nccl(=RCCL) backend, distributed upload, halo-split spmv path,
    all-reduced dots, and a distributed classical PCG solve — covers the
    NCCL-specific branches (device comm buffers, all_reduce on stream) that
    gloo CPU tests cannot."""
    import subprocess
    import sys
    script = r'''
import os, sys, torch
sys.path.insert(0, ".")
import torch.distributed as dist
os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
os.environ.setdefault("MASTER_PORT", "29431")
dist.init_process_group("nccl", rank=0, world_size=1)
torch.cuda.set_device(0)
from amgx_amd.distributed.manager import DistributedManager
from amgx_amd.problems import poisson_3d
from amgx_amd.config import AMGConfig
from amgx_amd.resources import Resources
from amgx_amd.solvers import create_solver
from amgx_amd import ops
import numpy as np
Ah = poisson_3d(12, 12, 12)
ro = Ah.row_offsets.numpy().astype(np.int64)
A = DistributedManager.upload_global_csr(
    ro, Ah.col_indices.numpy().astype(np.int64), Ah.values.numpy(),
    Ah.n_rows, 0, Ah.n_rows, device="cuda:0")
mgr = A.manager
b_user = torch.rand(Ah.n_rows, dtype=torch.float64).cuda()
b = mgr.permute_in(b_user)
x = torch.zeros_like(b)
cfg = AMGConfig.from_dict({
    "config_version": 2,
    "solver": {"preconditioner": {"algorithm": "CLASSICAL", "solver": "AMG",
                                  "smoother": "MULTICOLOR_GS", "presweeps": 1,
                                  "postsweeps": 1, "max_iters": 1,
                                  "min_coarse_rows": 24, "scope": "amg",
                                  "cycle": "V"},
               "solver": "PCG", "max_iters": 100, "monitor_residual": 1,
               "convergence": "RELATIVE_INI", "tolerance": 1e-8}})
res = Resources("cuda:0", distributed=True)
s = create_solver(cfg.root_scope(), resources=res)
s.setup(A)
st = s.solve(b, x, zero_initial_guess=True)
rel = ops.nrm2(ops.residual(A, x, b)) / ops.nrm2(b)
assert st.converged and rel < 1e-6, (st, rel)
# spmv halo path + all-reduced dot
y = ops.spmv(A, x)
d = s.dot(x, y)
assert d == d
dist.destroy_process_group()
print("NCCL_SMOKE_OK")
'''
    env = dict(__import__("os").environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run([sys.executable, "-c", script], capture_output=True,
                       text=True, timeout=600, env=env,
                       cwd=__import__("os").path.dirname(
                           __import__("os").path.dirname(
                               __import__("os").path.abspath(__file__))))
    assert r.returncode == 0 and "NCCL_SMOKE_OK" in r.stdout, \
        r.stdout[-2000:] + r.stderr[-2000:]


def test_device_2ring_colorings():
    """Distance-2 colorings stay device-resident: the *_2RING schemes (and
    coloring_level=2 of MIN_MAX/PARALLEL_GREEDY/MULTI_HASH) square the
    graph with the device hash SpGEMM and color it with the gfx950 kernel
    (reference src/matrix_coloring/min_max_2ring.cu role)."""
    A = to_gpu(poisson_3d(8, 7, 6))
    for scheme in ("MIN_MAX_2RING", "GREEDY_MIN_MAX_2RING"):
        cfg = AMGConfig.from_dict({"solver": {
            "solver": "MULTICOLOR_GS", "matrix_coloring_scheme": scheme}})
        col = MatrixColoring.create(A, cfg.root_scope())
        assert col.colors.is_cuda
        assert col.validate(A, level=2), scheme
    for scheme in ("MIN_MAX", "PARALLEL_GREEDY", "MULTI_HASH"):
        cfg = AMGConfig.from_dict({"solver": {
            "solver": "MULTICOLOR_GS", "matrix_coloring_scheme": scheme,
            "coloring_level": 2}})
        col = MatrixColoring.create(A, cfg.root_scope())
        assert col.colors.is_cuda
        assert col.validate(A, level=2), scheme


def test_coarse_generators_agree():
    """The LDS-hash LOW_DEG generator and the one-sort THRUST generator
    produce the same Galerkin coarse matrix for the same matching
    (reference coarseAgenerators family contract)."""
    from amgx_amd.ops import size2_matching
    A = to_gpu(poisson_3d(12, 12, 12))
    agg, nagg = size2_matching(A)
    C1 = ops.galerkin_aggregation(A, agg, nagg)                      # LOW_DEG hash
    C2 = ops.galerkin_aggregation(A, agg, nagg, generator="THRUST")  # one-sort
    assert torch.equal(C1.row_offsets, C2.row_offsets)
    assert torch.equal(C1.col_indices, C2.col_indices)
    assert torch.allclose(C1.values, C2.values, atol=1e-12)


# ---------------------------------------------------------------- sweeps
def _cpu_coloring(colg):
    return MatrixColoring(colg.colors.cpu(), colg.num_colors)


def _cpu_dilu_smooth(A, einv, col, b, x, relax):
    """CPU reference of the fused smoother: residual, then DILU apply."""
    from amgx_amd.ops import cpu as cpu_ops
    cpu_ops.dilu_solve(A, einv, col, cpu_ops.residual(A, x, b), relax, x)
    return x


@pytest.fixture(scope="module")
def big_level():
    """One scalar level just above the single-workgroup threshold, so the
    sweeps take the one-launch-per-color kernels (the path of the fine
    benchmark levels), with the CPU DILU / ILU(0) factors every test of that
    path compares against. Nothing here is modified by the tests."""
    from types import SimpleNamespace
    from amgx_amd import _core
    from amgx_amd.ops import cpu as cpu_ops
    A = poisson_2d(129, 128)
    assert A.n_rows > _core.SMALL_LEVEL_ROWS
    Ag = to_gpu(A)
    colg = MatrixColoring.create(Ag)
    col = _cpu_coloring(colg)
    g = torch.Generator().manual_seed(11)
    return SimpleNamespace(
        A=A, Ag=Ag, colg=colg, col=col,
        b=torch.rand(A.n_rows, generator=g, dtype=torch.float64),
        x0=torch.rand(A.n_rows, generator=g, dtype=torch.float64),
        dinv=cpu_ops.jacobi_dinv(A),
        einv=cpu_ops.dilu_setup(A, col),
        lu=cpu_ops.ilu0_setup(A, col))


@pytest.mark.parametrize("symmetric", [False, True])
def test_gs_sweep_per_color_path(big_level, symmetric):
    from amgx_amd.ops import cpu as cpu_ops
    L = big_level
    x1 = L.x0.clone()
    x2 = L.x0.cuda()
    cpu_ops.gs_sweep(L.A, L.dinv, L.b, x1, L.col, 1.0, symmetric)
    ops.gs_sweep(L.Ag, ops.jacobi_dinv(L.Ag), L.b.cuda(), x2, L.colg, 1.0,
                 symmetric)
    print("max dev", (x2.cpu() - x1).abs().max().item())
    assert torch.allclose(x2.cpu(), x1, rtol=1e-12, atol=1e-13)


def test_dilu_per_color_path(big_level):
    from amgx_amd.ops import cpu as cpu_ops
    from amgx_amd.ops import gpu as gpu_ops
    L = big_level
    e_gpu = ops.dilu_setup(L.Ag, L.colg)
    print("setup max dev", (e_gpu.cpu() - L.einv).abs().max().item())
    assert torch.allclose(e_gpu.cpu(), L.einv, rtol=1e-12, atol=1e-13)
    x1 = torch.zeros_like(L.b)
    x2 = x1.cuda()
    cpu_ops.dilu_solve(L.A, L.einv, L.col, L.b, 0.9, x1)
    ops.dilu_solve(L.Ag, e_gpu, L.colg, L.b.cuda(), 0.9, x2)
    print("solve max dev", (x2.cpu() - x1).abs().max().item())
    assert torch.allclose(x2.cpu(), x1, rtol=1e-11, atol=1e-12)
    # fused-residual smoother from a nonzero iterate
    y1 = _cpu_dilu_smooth(L.A, L.einv, L.col, L.b, L.x0.clone(), 0.9)
    y2 = L.x0.cuda()
    assert gpu_ops.dilu_smooth(L.Ag, e_gpu, L.colg, L.b.cuda(), y2, 0.9) \
        is True
    print("smooth max dev", (y2.cpu() - y1).abs().max().item())
    assert torch.allclose(y2.cpu(), y1, rtol=1e-11, atol=1e-12)


def test_ilu0_per_color_path(big_level):
    from amgx_amd.ops import cpu as cpu_ops
    from amgx_amd.ops import gpu as gpu_ops
    L = big_level
    lu_gpu = gpu_ops.ilu0_setup(L.Ag, L.colg)
    print("setup max dev", (lu_gpu.cpu() - L.lu).abs().max().item())
    assert torch.allclose(lu_gpu.cpu(), L.lu, rtol=1e-12, atol=1e-13)
    x1 = torch.zeros_like(L.b)
    x2 = x1.cuda()
    cpu_ops.ilu0_solve(L.A, L.lu, L.col, L.b, x1, 1.0)
    gpu_ops.ilu0_solve(L.Ag, lu_gpu, L.colg, L.b.cuda(), x2, 1.0)
    print("solve max dev", (x2.cpu() - x1).abs().max().item())
    assert torch.allclose(x2.cpu(), x1, rtol=1e-11, atol=1e-12)


def test_mixed_precision_per_color_path(big_level):
    """fp32 matrix x fp64 vectors through the per-color GS and DILU kernels
    against the fp64 CPU reference."""
    from amgx_amd.ops import cpu as cpu_ops
    L = big_level
    A32g = CSRMatrix(L.A.row_offsets, L.A.col_indices,
                     L.A.values.to(torch.float32),
                     n_cols=L.A.n_cols).to("cuda:0")
    x1 = torch.zeros_like(L.b)
    x2 = x1.cuda()
    cpu_ops.gs_sweep(L.A, L.dinv, L.b, x1, L.col, 1.0)
    ops.gs_sweep(A32g, ops.jacobi_dinv(A32g), L.b.cuda(), x2, L.colg, 1.0)
    print("gs max dev", (x2.cpu() - x1).abs().max().item())
    assert x2.dtype == torch.float64
    assert torch.allclose(x2.cpu(), x1, rtol=1e-4, atol=1e-5)
    w1 = torch.zeros_like(L.b)
    w2 = w1.cuda()
    cpu_ops.dilu_solve(L.A, L.einv, L.col, L.b, 0.9, w1)
    ops.dilu_solve(A32g, ops.dilu_setup(A32g, L.colg), L.colg, L.b.cuda(),
                   0.9, w2)
    print("dilu max dev", (w2.cpu() - w1).abs().max().item())
    assert torch.allclose(w2.cpu(), w1, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("make,rtol,atol", [
    (lambda: poisson_2d(16, 16), 1e-11, 1e-12),
    (lambda: block_laplacian(8, 8, block_dim=4), 1e-9, 1e-11),
], ids=["scalar", "block4"])
def test_dilu_smooth_small_levels(make, rtol, atol):
    """Fused-residual smoother entry point against CPU residual + apply."""
    from amgx_amd.ops import cpu as cpu_ops
    from amgx_amd.ops import gpu as gpu_ops
    A = make()
    Ag = to_gpu(A)
    colg = MatrixColoring.create(Ag)
    col = _cpu_coloring(colg)
    g = torch.Generator().manual_seed(5)
    n = A.n_rows * A.block_dim
    b = torch.rand(n, generator=g, dtype=torch.float64)
    x1 = torch.rand(n, generator=g, dtype=torch.float64)
    x2 = x1.cuda()
    _cpu_dilu_smooth(A, cpu_ops.dilu_setup(A, col), col, b, x1, 0.9)
    done = gpu_ops.dilu_smooth(Ag, ops.dilu_setup(Ag, colg), colg, b.cuda(),
                               x2, 0.9)
    assert done is True
    print("max dev", (x2.cpu() - x1).abs().max().item())
    assert torch.allclose(x2.cpu(), x1, rtol=rtol, atol=atol)


@pytest.mark.parametrize("bd", [2, 3, 5])
def test_dilu_generic_block_gpu(bd):
    """Sorted block kernels for block sizes without a specialised path."""
    A = block_laplacian(9, 7, block_dim=bd, seed=bd)
    Ag = to_gpu(A)
    colg = MatrixColoring.create(Ag)
    col = _cpu_coloring(colg)
    e_ref = ops.dilu_setup(A, col)
    e_gpu = ops.dilu_setup(Ag, colg)
    print("setup max dev", (e_gpu.cpu() - e_ref).abs().max().item())
    assert torch.allclose(e_gpu.cpu(), e_ref, rtol=1e-9, atol=1e-11)
    r = torch.rand(A.n_rows * bd, dtype=torch.float64)
    x1 = torch.zeros_like(r)
    x2 = x1.cuda()
    ops.dilu_solve(A, e_ref, col, r, 1.0, x1)
    ops.dilu_solve(Ag, e_gpu, colg, r.cuda(), 1.0, x2)
    print("solve max dev", (x2.cpu() - x1).abs().max().item())
    assert torch.allclose(x2.cpu(), x1, rtol=1e-9, atol=1e-11)


def test_slab_cache_follows_coloring():
    """A matrix swept under a second coloring must not serve slabs or
    elimination positions of the first."""
    from amgx_amd.ops import cpu as cpu_ops
    from amgx_amd.ops import gpu as gpu_ops
    A = poisson_2d(16, 16)
    Ag = to_gpu(A)
    c1 = MatrixColoring.create(Ag)
    c2 = MatrixColoring(c1.num_colors - 1 - c1.colors, c1.num_colors)
    assert c2.validate(Ag)
    r = torch.rand(A.n_rows, dtype=torch.float64)
    for colg in (c1, c2):
        Ag.coloring = colg
        col = _cpu_coloring(colg)
        x1 = torch.zeros_like(r)
        x2 = x1.cuda()
        cpu_ops.dilu_solve(A, cpu_ops.dilu_setup(A, col), col, r, 0.9, x1)
        gpu_ops.dilu_solve(Ag, gpu_ops.dilu_setup(Ag, colg), colg, r.cuda(),
                           0.9, x2)
        assert torch.allclose(x2.cpu(), x1, rtol=1e-11, atol=1e-12)
        y1 = torch.zeros_like(r)
        y2 = y1.cuda()
        cpu_ops.ilu0_solve(A, cpu_ops.ilu0_setup(A, col), col, r, y1, 1.0)
        gpu_ops.ilu0_solve(Ag, gpu_ops.ilu0_setup(Ag, colg), colg, r.cuda(),
                           y2, 1.0)
        assert torch.allclose(y2.cpu(), y1, rtol=1e-11, atol=1e-12)
