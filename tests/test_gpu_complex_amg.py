"""Aggregation AMG in the device complex modes dZZI / dCCI / dZCI: the
complex instantiations of the setup kernels (SIZE_2 matching, LDS-hash and
one-sort Galerkin, SpGEMM), the transfer operators, the multicolor GS / DILU
sweeps and the dense coarse solve, each against the host backend
(ops/cpu.py) in complex128 on the same rounded inputs; then whole solves.

Pairs are (matrix, vector) as in tests/test_gpu_complex.py. ZZ compares at
rtol / atol 1e-12; CC and CZ at the tolerance tests/test_gpu.py and
tests/test_gpu_complex.py apply to the fp32 / complex64 kernel of the same
family (spmv_tol for the products, jacobi_tol = the fp32 cases of
test_mixed_precision_per_color_path for the sweeps)."""

from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu

from amgx_amd import AMGConfig, CSRMatrix, _core, create_solver, ops
from amgx_amd.amg.coloring import MatrixColoring
from amgx_amd.ops import cpu as cpu_ops
from amgx_amd.ops import gpu as gpu_ops
from amgx_amd.problems import poisson_2d
from amgx_amd.resources import Resources

from tests.test_gpu_complex import (C, DEV, PAIRS, Z, close, cvec, jacobi_tol,
                                    on_gpu, pairs, rand_ccsr, rel_err,
                                    spmv_tol)

mat_dtypes = pytest.mark.parametrize("ta", [Z, C], ids=["Z", "C"])


def type_tol(dtype, tol):
    return tol("ZZ" if dtype == Z else "CC")


def dtype_name(dtype):
    return str(dtype).split(".")[-1]


def rounded(m, ta):
    """scipy complex128 copy of m with its values rounded to ta: the inputs
    the device sees, for the host reference."""
    out = m.astype(np.complex128).copy()
    out.data = torch.from_numpy(out.data).to(ta).to(Z).numpy()
    return out


def shifted_poisson(nx, ny, shift):
    """tests/test_gpu_complex.py:helmholtz_like on an nx x ny grid with the
    given diagonal shift, with a manufactured solution."""
    P = poisson_2d(nx, ny).to_scipy().astype(np.complex128)
    n = P.shape[0]
    K = sp.diags([0.3j * np.ones(n - 1), -0.2j * np.ones(n - 1)], [1, -1])
    S = (P + K + shift * sp.identity(n)).tocsr()
    S.sort_indices()
    rng = np.random.RandomState(5)
    xref = rng.randn(n) + 1j * rng.randn(n)
    return S, torch.from_numpy(xref), torch.from_numpy(S @ xref)


# ---------------------------------------------------------------- matching
def gaussian_integer_matrix(seed):
    """poisson_2d(30, 30) structure; entries z * 2^k with z a Gaussian
    integer of integral modulus, so |entry| is exact in fp32 and fp64.
    Returns the complex matrix and the real matrix of the moduli."""
    P = poisson_2d(30, 30).to_scipy().tocsr()
    P.sort_indices()
    triples = np.array([(3, 4, 5), (5, 12, 13), (8, 15, 17), (20, 21, 29),
                        (7, 24, 25)], dtype=np.float64)
    rng = np.random.RandomState(seed)
    t = triples[rng.randint(len(triples), size=P.nnz)]
    swap = rng.rand(P.nnz) < 0.5
    re = np.where(swap, t[:, 1], t[:, 0]) * rng.choice([-1.0, 1.0], P.nnz)
    im = np.where(swap, t[:, 0], t[:, 1]) * rng.choice([-1.0, 1.0], P.nnz)
    scale = 2.0 ** rng.randint(-2, 3, size=P.nnz)
    cm = sp.csr_matrix(((re + 1j * im) * scale, P.indices, P.indptr),
                       shape=P.shape)
    rm = sp.csr_matrix((t[:, 2] * scale, P.indices, P.indptr), shape=P.shape)
    assert np.array_equal(np.abs(cm.data), rm.data)
    return cm, rm


@mat_dtypes
def test_size2_matching_uses_the_modulus(ta):
    cm, rm = gaussian_integer_matrix(seed=2)
    n = cm.shape[0]
    agg_c, nc_c = ops.size2_matching(on_gpu(cm, ta))
    agg_r, nc_r = ops.size2_matching(
        CSRMatrix.from_scipy(rm, device=DEV, dtype=torch.float64))
    assert nc_c == nc_r
    assert torch.equal(agg_c, agg_r)
    a = agg_c.cpu().numpy()
    assert a.min() >= 0 and a.max() == nc_c - 1
    assert n // 4 <= nc_c <= n * 3 // 4


# ---------------------------------------------------------------- Galerkin
def tiered_matrix(n, seed=7):
    """Random complex matrix, about 6 entries per row plus the diagonal,
    symmetrised structure; row 0 filled in all n columns and row 2 in
    columns 0..399. With aggregates i // 2 coarse row 0 has n / 2 entries
    and coarse row 1 about 200."""
    rng = np.random.RandomState(seed)
    rows = np.repeat(np.arange(n), 3)       # 3 random entries per row
    cols = rng.randint(n, size=3 * n)
    vals = rng.rand(3 * n) + 1j * (rng.rand(3 * n) - 0.3)
    m = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    m = (m + m.T + sp.identity(n) * (4.0 + 1.0j)).tolil()
    m[0, :] = rng.rand(n) + 1j * (rng.rand(n) - 0.4)
    m[2, :400] = rng.rand(400) - 1j * (rng.rand(400) + 0.2)
    m = m.tocsr()
    m.sum_duplicates()
    m.sort_indices()
    return m


def host_galerkin(m, agg, nc):
    n = m.shape[0]
    P = sp.csr_matrix((np.ones(n), (np.arange(n), agg)), shape=(n, nc))
    ref = (P.T @ m @ P).tocsr()
    ref.sort_indices()
    return ref


def check_galerkin(Ac, ref, tol):
    ro = Ac.row_offsets.cpu().numpy()
    ci = Ac.col_indices.cpu().numpy()
    assert np.array_equal(ro, ref.indptr)
    assert np.array_equal(ci, ref.indices)
    for i in range(len(ro) - 1):
        assert (np.diff(ci[ro[i]:ro[i + 1]]) > 0).all(), f"row {i} unsorted"
    assert close(Ac.values, torch.from_numpy(ref.data), tol)


@mat_dtypes
@pytest.mark.parametrize("generator", [None, "THRUST"])
def test_galerkin_every_hash_tier(ta, generator):
    n = 1400
    nc = n // 2
    m = rounded(tiered_matrix(n), ta)
    agg = np.arange(n) // 2
    ref = host_galerkin(m, agg, nc)
    width = np.diff(ref.indptr)
    assert width[0] > 512                       # top tier
    assert 65 <= width[1] <= 512                # 512-entry tier
    assert width[2:].max() <= 64                # 64-entry tier
    assert m.nnz <= 48 * nc                     # 64-entry tier entered first
    Ac = ops.galerkin_aggregation(
        on_gpu(m, ta), torch.from_numpy(agg.astype(np.int32)).to(DEV), nc,
        generator=generator)
    assert Ac.values.dtype == ta
    check_galerkin(Ac, ref, type_tol(ta, spmv_tol))


@mat_dtypes
def test_galerkin_row_wider_than_top_tier_falls_back(ta):
    cap = _core.SPGEMM_HASH_TOP_CAP[dtype_name(ta)]
    assert cap == (4096 if ta == Z else 8192)
    nc = cap + 1                 # coarse row 0: one entry past the top tier
    n = 2 * nc
    m = rounded(tiered_matrix(n), ta)
    agg = np.arange(n) // 2
    ref = host_galerkin(m, agg, nc)
    assert np.diff(ref.indptr)[0] == cap + 1
    A = on_gpu(m, ta)
    aggd = torch.from_numpy(agg.astype(np.int32)).to(DEV)
    # the hash path itself reports the overflow ...
    ro = _core.spgemm_hash(
        torch.arange(0, n + 1, 2, dtype=torch.int32, device=DEV),
        torch.arange(n, dtype=torch.int32, device=DEV), A.values,
        A.row_offsets, A.col_indices, A.values, aggd, 1, A.nnz, 64)[0]
    assert int(ro[0]) == -1
    # ... and the dispatcher still returns the product
    check_galerkin(ops.galerkin_aggregation(A, aggd, nc), ref,
                   type_tol(ta, spmv_tol))


@mat_dtypes
def test_spgemm(ta):
    a = rounded(rand_ccsr(300, 0.02, seed=21), ta)
    b = rounded(rand_ccsr(300, 0.02, seed=22), ta)
    ref = (a @ b).tocsr()
    ref.sum_duplicates()
    ref.sort_indices()
    Cm = ops.spgemm(on_gpu(a, ta), on_gpu(b, ta))
    assert Cm.values.dtype == ta
    check_galerkin(Cm, ref, type_tol(ta, spmv_tol))


# ---------------------------------------------------------------- transfers
@pytest.mark.parametrize("tv", [Z, C], ids=["Z", "C"])
def test_restrict_prolongate(tv):
    n = 515
    A = on_gpu(rand_ccsr(n, 0.0039, seed=3), Z)
    agg, nc = ops.size2_matching(A)
    a = agg.cpu().numpy().astype(np.int64)
    P = sp.csr_matrix((np.ones(n), (np.arange(n), a)), shape=(n, nc))
    tol = type_tol(tv, spmv_tol)
    r = cvec(n, 31).to(tv)
    assert float(r.imag.abs().min()) > 0 and float(r.real.abs().min()) > 0
    want = torch.from_numpy(P.T @ r.to(Z).numpy())
    # atomic path
    rc = ops.restrict_agg(r.to(DEV), agg, nc)
    assert rc.dtype == tv
    assert close(rc, want, tol)
    # deterministic path over the aggregate CSR
    order = torch.argsort(agg.to(torch.int64), stable=True).to(torch.int32)
    off = torch.zeros(nc + 1, dtype=torch.int64, device=DEV)
    off[1:] = torch.cumsum(torch.bincount(agg.to(torch.int64), minlength=nc),
                           0)
    rc2 = ops.restrict_agg(r.to(DEV), agg, nc,
                           structure=(off.to(torch.int32), order))
    assert close(rc2, want, tol)
    x, xc = cvec(n, 32).to(tv), cvec(nc, 33, shift=0.4).to(tv)
    xg = x.to(DEV)
    ops.prolongate_agg(xg, xc.to(DEV), agg)
    assert close(xg, torch.from_numpy(x.to(Z).numpy()
                                      + P @ xc.to(Z).numpy()), tol)


# ---------------------------------------------------------------- sweeps
def make_level(nx, ny):
    """One level with the device coloring copied to the host; one diagonal
    entry of the first color is stored as zero (the d == 0 guards)."""
    S, _, _ = shifted_poisson(nx, ny, 0.5 + 0.8j)
    n = S.shape[0]
    colg = MatrixColoring.create(on_gpu(S, Z))
    col = MatrixColoring(colg.colors.cpu(), colg.num_colors)
    zrow = int(col.rows_of(0)[n // 3 % len(col.rows_of(0))])
    row = slice(S.indptr[zrow], S.indptr[zrow + 1])
    k = S.indptr[zrow] + int(np.flatnonzero(S.indices[row] == zrow)[0])
    S.data[k] = 0.0                      # stays stored
    return SimpleNamespace(S=S, n=n, colg=colg, col=col, zrow=zrow,
                           b=cvec(n, 41), x0=cvec(n, 42, shift=0.6))


@pytest.fixture(scope="module")
def levels():
    big, small = make_level(129, 128), make_level(12, 12)
    assert big.n > _core.SMALL_LEVEL_ROWS          # per-color slab kernels
    assert small.n <= _core.SMALL_LEVEL_ROWS       # single-workgroup kernels
    return {"per_color": big, "single_wg": small}


def host_level(L, ta):
    """Host matrix (complex128, values rounded to ta) of level L."""
    return CSRMatrix.from_scipy(rounded(L.S, ta), dtype=Z)


@pairs
@pytest.mark.parametrize("path", ["per_color", "single_wg"])
@pytest.mark.parametrize("symmetric", [False, True])
def test_gs_sweep(levels, path, symmetric, pair):
    ta, tv = PAIRS[pair]
    L = levels[path]
    Ah, Ag = host_level(L, ta), on_gpu(L.S, ta)
    b, x0 = L.b.to(tv), L.x0.to(tv)
    x1 = x0.to(Z).clone()            # the host sweep works in place
    cpu_ops.gs_sweep(Ah, cpu_ops.jacobi_dinv(Ah), b.to(Z), x1, L.col, 0.9,
                     symmetric)
    x2 = x0.to(DEV)
    ops.gs_sweep(Ag, ops.jacobi_dinv(Ag), b.to(DEV), x2, L.colg, 0.9,
                 symmetric)
    assert x2.dtype == tv
    print("max dev", (x2.cpu().to(Z) - x1).abs().max().item())
    assert close(x2, x1, jacobi_tol(pair))


@pairs
@pytest.mark.parametrize("path", ["per_color", "single_wg"])
def test_dilu(levels, path, pair):
    ta, tv = PAIRS[pair]
    L = levels[path]
    Ah, Ag = host_level(L, ta), on_gpu(L.S, ta)
    tol = jacobi_tol(pair)
    e_ref = cpu_ops.dilu_setup(Ah, L.col)
    e_gpu = ops.dilu_setup(Ag, L.colg)
    assert e_gpu.einv.dtype == ta
    print("setup max dev", (e_gpu.cpu().to(Z) - e_ref).abs().max().item())
    assert close(e_gpu.einv, e_ref, tol)
    # zero diagonal in the first color: E = 0 falls back to 1 on both sides
    assert complex(e_ref[L.zrow]) == 1.0
    assert complex(e_gpu.einv[L.zrow].cpu()) == 1.0
    b, x0 = L.b.to(tv), L.x0.to(tv)
    x1 = x0.to(Z).clone()            # the host sweep works in place
    cpu_ops.dilu_solve(Ah, e_ref, L.col, cpu_ops.residual(Ah, x1, b.to(Z)),
                       0.9, x1)
    x2 = x0.to(DEV)
    assert gpu_ops.dilu_smooth(Ag, e_gpu, L.colg, b.to(DEV), x2, 0.9) is True
    print("smooth max dev", (x2.cpu().to(Z) - x1).abs().max().item())
    assert close(x2, x1, tol)
    # plain apply (the unfused entry point)
    y1 = torch.zeros(L.n, dtype=Z)
    cpu_ops.dilu_solve(Ah, e_ref, L.col, b.to(Z), 0.9, y1)
    y2 = torch.zeros(L.n, dtype=tv, device=DEV)
    ops.dilu_solve(Ag, e_gpu, L.colg, b.to(DEV), 0.9, y2)
    assert close(y2, y1, tol)


@mat_dtypes
def test_dilu_rejects_coupled_rows_of_one_color(levels, ta):
    """Two coupled rows of one color would be skipped by the factor and
    raced on by the sweeps: the complex setup refuses such a coloring on
    both backends."""
    L = levels["single_wg"]
    Ag = on_gpu(L.S, ta)
    one_color = MatrixColoring(
        torch.zeros(L.n, dtype=torch.int32, device=DEV), 1)
    with pytest.raises(RuntimeError, match="valid distance-1 coloring"):
        ops.dilu_setup(Ag, one_color)
    with pytest.raises(RuntimeError, match="valid distance-1 coloring"):
        cpu_ops.dilu_setup(host_level(L, ta),
                           MatrixColoring(one_color.colors.cpu(), 1))


@pairs
def test_unsorted_gs_rows(levels, pair):
    """gs_smooth_color: the row-list kernel on the unsorted matrix."""
    ta, tv = PAIRS[pair]
    L = levels["single_wg"]
    Ah, Ag = host_level(L, ta), on_gpu(L.S, ta)
    b, x0 = L.b.to(tv), L.x0.to(tv)
    x1, x2 = x0.to(Z).clone(), x0.to(DEV)
    cpu_ops.gs_smooth_color(Ah, cpu_ops.jacobi_dinv(Ah), b.to(Z), x1,
                            L.col.rows_of(1), 0.9)
    ops.gs_smooth_color(Ag, ops.jacobi_dinv(Ag), b.to(DEV), x2,
                        L.colg.rows_of(1), 0.9)
    assert close(x2, x1, jacobi_tol(pair))


# ---------------------------------------------------------------- solvers
def run(cfg, S, b, device, ta, tv):
    s = create_solver(AMGConfig.from_dict(cfg).root_scope(),
                      resources=Resources(device))
    A = CSRMatrix.from_scipy(S, device=device, dtype=ta)
    bd = b.to(tv).to(device)
    x = torch.zeros_like(bd)
    s.setup(A)
    st = s.solve(bd, x, zero_initial_guess=True)
    return st, x.cpu().to(Z)


def true_res(S, b, x):
    r = b.numpy() - S @ x.numpy()
    return float(np.linalg.norm(r) / np.linalg.norm(b.numpy()))


@pairs
def test_dense_lu(pair):
    ta, tv = PAIRS[pair]
    S, _, b = shifted_poisson(8, 8, 0.5 + 0.8j)
    cfg = {"solver": "DENSE_LU_SOLVER"}
    _, x_h = run(cfg, S, b, "cpu", ta, tv)
    _, x_d = run(cfg, S, b, DEV, ta, tv)
    res_h, res_d = true_res(S, b, x_h), true_res(S, b, x_d)
    print(f"{pair}: residual host {res_h:.3e} device {res_d:.3e}")
    if pair == "ZZ":
        assert res_d < 1e-10
    else:
        assert res_d <= 10 * res_h


def amg_cfg(selector="DUMMY", smoother="BLOCK_JACOBI", cycle="V", **over):
    amg = {"solver": "AMG", "algorithm": "AGGREGATION", "selector": selector,
           "smoother": {"solver": smoother, "relaxation_factor": 0.8},
           "presweeps": 1, "postsweeps": 1, "cycle": cycle, "max_iters": 1,
           "min_coarse_rows": 8, "coarse_solver": "DENSE_LU_SOLVER"}
    if selector == "DUMMY":
        amg["aggregate_size"] = 2
    amg.update(over)
    return amg


def fgmres(precond, tolerance=1e-10):
    cfg = {"solver": "FGMRES" if precond else "GMRES", "max_iters": 300,
           "gmres_n_restart": 30, "monitor_residual": 1,
           "convergence": "RELATIVE_INI", "tolerance": tolerance}
    if precond:
        cfg["preconditioner"] = precond
    return cfg


@pytest.fixture(scope="module")
def systems():
    out = {}
    for name, (nx, ny) in {"40x40": (40, 40), "136x128": (136, 128)}.items():
        S, xref, b = shifted_poisson(nx, ny, 0.05 + 0.1j)
        out[name] = SimpleNamespace(S=S, xref=xref, b=b)
    assert out["136x128"].S.shape[0] == 17408 > _core.SMALL_LEVEL_ROWS
    st, _ = run(fgmres(None), out["40x40"].S, out["40x40"].b, DEV, Z, Z)
    assert st.converged
    out["40x40"].plain_iters = st.iterations
    return out


@pytest.mark.parametrize("name", ["40x40", "136x128"])
def test_fgmres_amg_same_hierarchy_as_host(systems, name):
    """DUMMY aggregates and Jacobi smoothing: the hierarchy is the same on
    both backends, only reduction orders differ."""
    P = systems[name]
    cfg = fgmres(amg_cfg())
    st_h, _ = run(cfg, P.S, P.b, "cpu", Z, Z)
    st_d, x_d = run(cfg, P.S, P.b, DEV, Z, Z)
    assert st_h.converged
    assert st_d.converged, st_d
    assert rel_err(x_d, P.xref) < 1e-7
    assert abs(st_d.iterations - st_h.iterations) <= 1, (st_d, st_h)


@pytest.mark.parametrize("name", ["40x40", "136x128"])
@pytest.mark.parametrize("smoother", ["BLOCK_JACOBI", "MULTICOLOR_GS",
                                      "MULTICOLOR_DILU"])
@pytest.mark.parametrize("selector", ["SIZE_2", "SIZE_4"])
def test_fgmres_amg_device_hierarchy(systems, name, smoother, selector):
    P = systems[name]
    st, x = run(fgmres(amg_cfg(selector, smoother)), P.S, P.b, DEV, Z, Z)
    print(f"{name} {selector} {smoother}: {st.iterations} iterations")
    assert st.converged, st
    assert rel_err(x, P.xref) < 1e-7
    if name == "40x40":
        assert 2 * st.iterations <= P.plain_iters, (st, P.plain_iters)


@pytest.mark.parametrize("cycle", ["W", "F"])
def test_fgmres_amg_cycles(systems, cycle):
    P = systems["40x40"]
    st, x = run(fgmres(amg_cfg("SIZE_2", "MULTICOLOR_DILU", cycle)), P.S, P.b,
                DEV, Z, Z)
    assert st.converged, st
    assert rel_err(x, P.xref) < 1e-7
    assert 2 * st.iterations <= P.plain_iters, (st, P.plain_iters)


@pytest.mark.parametrize("pair", ["CC", "CZ"])
@pytest.mark.parametrize("name,smoother", [
    ("40x40", "BLOCK_JACOBI"), ("40x40", "MULTICOLOR_GS"),
    ("40x40", "MULTICOLOR_DILU"), ("136x128", "BLOCK_JACOBI")])
def test_fgmres_amg_complex64_and_mixed(systems, name, smoother, pair):
    ta, tv = PAIRS[pair]
    P = systems[name]
    cfg = fgmres(amg_cfg("DUMMY", smoother), tolerance=1e-5)
    st_h, x_h = run(cfg, P.S, P.b, "cpu", ta, tv)
    st_d, x_d = run(cfg, P.S, P.b, DEV, ta, tv)
    assert st_h.converged
    assert st_d.converged, st_d
    res_h, res_d = true_res(P.S, P.b, x_h), true_res(P.S, P.b, x_d)
    print(f"{name} {smoother} {pair}: true residual host {res_h:.3e} "
          f"device {res_d:.3e}")
    assert res_d <= 10 * res_h, (res_d, res_h)


def test_amg_as_solver_reduces_the_residual_monotonically(systems):
    P = systems["40x40"]
    cfg = dict(amg_cfg("SIZE_2", "MULTICOLOR_DILU"), max_iters=50,
               monitor_residual=1, store_res_history=1,
               convergence="RELATIVE_INI", tolerance=1e-12)
    st, x = run(cfg, P.S, P.b, DEV, Z, Z)
    res = [float(r) for r in st.residuals]
    assert len(res) >= 10
    assert all(b < a for a, b in zip(res, res[1:])), res
    assert res[-1] < 1e-3 * res[0]


# ---------------------------------------------------------------- API
def test_capi_dZZI_aggregation_dilu(systems):
    import os
    from amgx_amd import capi as A
    P = systems["40x40"]
    path = os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "configs", "FGMRES_AGGREGATION_DILU.json")
    A.AMGX_initialize()
    rc, cfg = A.AMGX_config_create_from_file(path)
    assert rc == A.RC_OK
    rc, res = A.AMGX_resources_create_simple(cfg)
    assert rc == A.RC_OK
    rc, m = A.AMGX_matrix_create(res, "dZZI")
    assert rc == A.RC_OK
    n = P.S.shape[0]
    assert A.AMGX_matrix_upload_all(m, n, P.S.nnz, 1, 1, P.S.indptr,
                                    P.S.indices, P.S.data) == A.RC_OK
    rc, bh = A.AMGX_vector_create(res, "dZZI")
    assert rc == A.RC_OK
    rc, xh = A.AMGX_vector_create(res, "dZZI")
    assert rc == A.RC_OK
    assert A.AMGX_vector_upload(bh, n, 1, P.b.numpy()) == A.RC_OK
    assert A.AMGX_vector_upload(xh, n, 1,
                                np.zeros(n, dtype=np.complex128)) == A.RC_OK
    rc, s = A.AMGX_solver_create(res, "dZZI", cfg)
    assert rc == A.RC_OK
    assert A.AMGX_solver_setup(s, m) == A.RC_OK
    assert A.AMGX_solver_solve(s, bh, xh) == A.RC_OK
    rc, nrm = A.AMGX_solver_calculate_residual_norm(s, m, bh, xh)
    assert rc == A.RC_OK
    assert m.A.values.is_cuda and m.A.values.dtype == Z
    assert nrm < 1e-6 * float(torch.linalg.vector_norm(P.b))


# ---------------------------------------------------------------- rejections
@pytest.mark.parametrize("over", [
    {"algorithm": "CLASSICAL"}, {"cycle": "CG"}, {"hipgraph_cycle": 1},
    {"use_hip_graph": 1}, {"smoother": "MULTICOLOR_ILU"},
    {"smoother": "JACOBI_L1"}], ids=lambda o: "-".join(map(str, o.values())))
def test_out_of_scope_raises(over):
    S, _, _ = shifted_poisson(12, 12, 0.5 + 0.8j)
    s = create_solver(AMGConfig.from_dict(amg_cfg("SIZE_2", **over))
                      .root_scope(), resources=Resources(DEV))
    with pytest.raises((NotImplementedError, RuntimeError), match="complex"):
        s.setup(on_gpu(S, Z))


def test_complex_block_matrix_raises():
    rng = np.random.RandomState(3)
    P = poisson_2d(6, 6).to_scipy().tocsr()
    vals = (rng.rand(P.nnz, 2, 2) + 1j * rng.rand(P.nnz, 2, 2))
    A = CSRMatrix(torch.from_numpy(P.indptr.astype(np.int32)),
                  torch.from_numpy(P.indices.astype(np.int32)),
                  torch.from_numpy(vals), n_cols=P.shape[1],
                  block_dim=2).to(DEV)
    s = create_solver(AMGConfig.from_dict(amg_cfg("SIZE_2")).root_scope(),
                      resources=Resources(DEV))
    with pytest.raises((NotImplementedError, RuntimeError), match="complex"):
        s.setup(A)
    with pytest.raises((NotImplementedError, RuntimeError), match="complex"):
        ops.size2_matching(A)
    agg = torch.zeros(A.n_rows, dtype=torch.int32, device=DEV)
    with pytest.raises((NotImplementedError, RuntimeError), match="complex"):
        ops.galerkin_aggregation(A, agg, 1)


def test_real_matrix_with_complex_vectors_still_raises():
    S, _, b = shifted_poisson(12, 12, 0.5 + 0.8j)
    A = CSRMatrix.from_scipy(S.real.tocsr(), device=DEV, dtype=torch.float64)
    colg = MatrixColoring.create(A)
    x = torch.zeros(A.n_rows, dtype=Z, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        ops.gs_sweep(A, ops.jacobi_dinv(A), b.to(DEV), x, colg, 1.0)
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        gpu_ops.dilu_smooth(A, ops.dilu_setup(A, colg), colg, b.to(DEV), x,
                            0.9)
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        _core.dense_gemv(torch.eye(4, dtype=torch.float64, device=DEV),
                         torch.zeros(4, dtype=Z, device=DEV),
                         torch.zeros(4, dtype=Z, device=DEV))
