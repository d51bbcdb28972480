"""Scalar per-color DILU over the strict color-split slabs (U / L parts of
the color-sorted slab, in-place backward sweep with the x update folded in)
against the host backend (ops/cpu.py) under the device coloring copied to the
host, and the V-cycle's skipped residual of a zero guess.

Tolerances are those of the per-color tests of tests/test_gpu.py: rtol 1e-11 /
atol 1e-12 in fp64, 1e-4 / 1e-5 with an fp32 matrix; the complex case uses
the 1e-12 / 1e-12 of tests/test_gpu_complex_amg.py. Shapes are the smallest
past the single-workgroup size."""

from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from amgx_amd import AMGConfig, CSRMatrix, create_solver, ops
from amgx_amd.amg.coloring import MatrixColoring
from amgx_amd.ops import cpu as cpu_ops
from amgx_amd.problems import poisson_2d, poisson_3d
from amgx_amd.resources import Resources

gpu = pytest.mark.gpu
DEV = "cuda:0"
F64 = dict(rtol=1e-11, atol=1e-12)
F32 = dict(rtol=1e-4, atol=1e-5)
RELAX = 0.9


def small_rows():
    from amgx_amd import _core
    return _core.SMALL_LEVEL_ROWS


def gpu_ops():
    from amgx_amd.ops import gpu
    return gpu


def host_coloring(colg):
    return MatrixColoring(colg.colors.cpu(), colg.num_colors)


def ext(v, n_cols):
    """v with a halo tail of zeros up to n_cols entries."""
    out = torch.zeros(n_cols, dtype=v.dtype)
    out[:v.numel()] = v
    return out


def make_level(A, seed):
    """Host matrix A, its device copy, the device coloring on both sides, the
    host factor and column-extended b / x0 (zero halo tails)."""
    assert A.n_rows > small_rows()
    Ag = A.to(DEV)
    colg = MatrixColoring.create(Ag)
    col = host_coloring(colg)
    g = torch.Generator().manual_seed(seed)
    b = torch.rand(A.n_rows, generator=g, dtype=torch.float64)
    x0 = torch.rand(A.n_rows, generator=g, dtype=torch.float64) - 0.5
    return SimpleNamespace(A=A, Ag=Ag, colg=colg, col=col,
                           einv=cpu_ops.dilu_setup(A, col),
                           b=ext(b, A.n_cols), x0=ext(x0, A.n_cols))


def halo_matrix(P, n_rows):
    """The first n_rows rows of P; the remaining columns are a halo tail."""
    m = P.to_scipy().tocsr()[:n_rows, :]
    return CSRMatrix.from_scipy(m)


@pytest.fixture(scope="module")
def levels():
    """Per-color levels shared by the tests; nothing here is modified."""
    out = {"2d": make_level(poisson_2d(129, 128), 21),
           "3d": make_level(poisson_3d(26, 26, 26), 22),
           "halo": make_level(halo_matrix(poisson_2d(129, 256), 129 * 128),
                              23)}
    assert out["2d"].A.n_rows == 16512 and out["3d"].A.n_rows == 17576
    assert out["halo"].A.n_cols == 2 * out["halo"].A.n_rows
    return out


def host_smooth(L, x, relax=RELAX, A=None, einv=None):
    A = L.A if A is None else A
    einv = L.einv if einv is None else einv
    cpu_ops.dilu_solve(A, einv, L.col, cpu_ops.residual(A, x, L.b), relax, x)
    return x


def show(tag, got, ref):
    print(tag, "max dev", (got.cpu() - ref).abs().max().item())


# ---------------------------------------------------------------- sweeps
@gpu
@pytest.mark.parametrize("name", ["2d", "3d", "halo"])
def test_fused_smoother_three_sweeps(levels, name):
    """x carried through three sweeps: a value the in-place backward sweep
    left in w would enter the next forward sweep."""
    L = levels[name]
    e_gpu = ops.dilu_setup(L.Ag, L.colg)
    x1, x2, bg = L.x0.clone(), L.x0.to(DEV), L.b.to(DEV)
    for sweep in range(3):
        host_smooth(L, x1)
        assert gpu_ops().dilu_smooth(L.Ag, e_gpu, L.colg, bg, x2, RELAX) \
            is True
        show(f"sweep {sweep}", x2, x1)
        assert torch.allclose(x2.cpu(), x1, **F64)
    assert not bool(x2[L.A.n_rows:].any())        # the halo tail stays zero


@gpu
@pytest.mark.parametrize("name", ["2d", "3d", "halo"])
@pytest.mark.parametrize("start", ["zero", "nonzero"])
def test_unfused_apply(levels, name, start):
    """dilu_solve accumulates into x."""
    L = levels[name]
    e_gpu = ops.dilu_setup(L.Ag, L.colg)
    x1 = torch.zeros_like(L.x0) if start == "zero" else L.x0.clone()
    x2 = x1.to(DEV)
    cpu_ops.dilu_solve(L.A, L.einv, L.col, L.b, RELAX, x1)
    ops.dilu_solve(L.Ag, e_gpu, L.colg, L.b.to(DEV), RELAX, x2)
    show("solve", x2, x1)
    assert torch.allclose(x2.cpu(), x1, **F64)
    # a second apply on the same state: w starts from the last apply's z
    cpu_ops.dilu_solve(L.A, L.einv, L.col, L.b, RELAX, x1)
    ops.dilu_solve(L.Ag, e_gpu, L.colg, L.b.to(DEV), RELAX, x2)
    assert torch.allclose(x2.cpu(), x1, **F64)


@gpu
def test_halo_columns_small_level():
    """The first 129 * 64 rows of poisson_2d(129, 128) with the other columns
    as a halo tail: the single-workgroup path on a rectangular matrix."""
    A = halo_matrix(poisson_2d(129, 128), 129 * 64)
    assert A.n_rows <= small_rows() and A.n_cols == 2 * A.n_rows
    Ag = A.to(DEV)
    colg = MatrixColoring.create(Ag)
    col = host_coloring(colg)
    einv = cpu_ops.dilu_setup(A, col)
    e_gpu = ops.dilu_setup(Ag, colg)
    g = torch.Generator().manual_seed(24)
    b = ext(torch.rand(A.n_rows, generator=g, dtype=torch.float64), A.n_cols)
    x1 = ext(torch.rand(A.n_rows, generator=g, dtype=torch.float64),
             A.n_cols)
    x2 = x1.to(DEV)
    cpu_ops.dilu_solve(A, einv, col, cpu_ops.residual(A, x1, b), RELAX, x1)
    assert gpu_ops().dilu_smooth(Ag, e_gpu, colg, b.to(DEV), x2, RELAX) \
        is True
    assert torch.allclose(x2.cpu(), x1, **F64)
    cpu_ops.dilu_solve(A, einv, col, b, RELAX, x1)
    ops.dilu_solve(Ag, e_gpu, colg, b.to(DEV), RELAX, x2)
    assert torch.allclose(x2.cpu(), x1, **F64)


# ---------------------------------------------------------------- slabs
def host_parts(A, col):
    """(offsets, columns, values) of U and L in slot order, entries in row
    order, from the colors alone."""
    ro = A.row_offsets.numpy().astype(np.int64)
    ci = A.col_indices.numpy().astype(np.int64)
    va = A.values.numpy()
    colors = col.colors.numpy().astype(np.int64)
    n = A.n_rows
    parts = {}
    for name, sign in (("U", 1), ("L", -1)):
        offs, cols, vals = [0], [], []
        for i in col.rows_sorted.numpy():
            k = np.arange(ro[i], ro[i + 1])
            j = ci[k]
            local = j < n
            keep = np.zeros(k.size, dtype=bool)
            keep[local] = sign * (colors[j[local]] - colors[i]) > 0
            cols.append(j[keep])
            vals.append(va[k[keep]])
            offs.append(offs[-1] + int(keep.sum()))
        parts[name] = (np.asarray(offs), np.concatenate(cols),
                       np.concatenate(vals))
    return parts


@gpu
@pytest.mark.parametrize("name", ["3d", "halo"])
def test_slab_contents(levels, name):
    L = levels[name]
    G = gpu_ops()
    e_gpu = ops.dilu_setup(L.Ag, L.colg)
    # the L values are gathered by the first unfused apply
    assert e_gpu.va_l is None
    ops.dilu_solve(L.Ag, e_gpu, L.colg, L.b.to(DEV), RELAX, L.x0.to(DEV))
    st = G._slabs(L.Ag, L.colg)
    want = host_parts(L.A, L.col)
    got = {"U": (st.upper, e_gpu.va_u), "L": (st.lower, e_gpu.va_l)}
    n = L.A.n_rows
    for key in ("U", "L"):
        (ro_x, ci_x, map_x), va_x = got[key]
        offs, cols, vals = want[key]
        assert ro_x.dtype == ci_x.dtype == map_x.dtype == torch.int32
        assert np.array_equal(ro_x.cpu().numpy(), offs)
        assert np.array_equal(ci_x.cpu().numpy(), cols)
        assert np.array_equal(va_x.cpu().numpy(), vals)
        # the map points at the same entry of the full slab
        assert torch.equal(st.ci_s[map_x.long()], ci_x)
        assert int(ci_x.max()) < n
    b = L.col.bounds
    nc = L.col.num_colors
    ro_u, ro_l = want["U"][0], want["L"][0]
    assert nc > 1
    assert ro_u[b[nc - 1]] == ro_u[b[nc]]          # last color: U rows empty
    assert ro_l[b[0]] == ro_l[b[1]] == 0           # color 0: L rows empty
    local_nnz = int((L.A.col_indices < n).sum())
    assert ro_u[-1] + ro_l[-1] + n == local_nnz
    if name == "3d":
        assert local_nnz == L.A.nnz                # square: every entry


@gpu
def test_one_color():
    """A diagonal matrix just past the single-workgroup size: one color, both
    parts empty, x + relax Einv (b - D x)."""
    n = small_rows() + 1
    g = torch.Generator().manual_seed(25)
    d = torch.rand(n, generator=g, dtype=torch.float64) + 0.5
    idx = torch.arange(n + 1, dtype=torch.int32)
    Ag = CSRMatrix(idx, idx[:n].clone(), d.clone()).to(DEV)
    colg = MatrixColoring.create(Ag)
    assert colg.num_colors == 1
    e_gpu = ops.dilu_setup(Ag, colg)
    b = torch.rand(n, generator=g, dtype=torch.float64)
    x0 = torch.rand(n, generator=g, dtype=torch.float64)
    x = x0.to(DEV)
    assert gpu_ops().dilu_smooth(Ag, e_gpu, colg, b.to(DEV), x, RELAX) is True
    assert torch.allclose(x.cpu(), x0 + RELAX * (b - d * x0) / d, **F64)
    y = x0.to(DEV)
    ops.dilu_solve(Ag, e_gpu, colg, b.to(DEV), RELAX, y)
    assert torch.allclose(y.cpu(), x0 + RELAX * b / d, **F64)
    st = gpu_ops()._slabs(Ag, colg)
    for part in (st.upper, st.lower):
        assert part[1].numel() == 0 and part[2].numel() == 0
        assert int(part[0].abs().max()) == 0


@gpu
def test_coefficient_replacement(levels):
    """Values scaled in place, setup again on the same coloring: the parts'
    structure is reused and their values follow the matrix."""
    L = levels["2d"]
    G = gpu_ops()
    Ag = L.A.to(DEV)                     # a copy this test may modify
    e0 = ops.dilu_setup(Ag, L.colg)
    xg = L.x0.to(DEV)
    ops.dilu_solve(Ag, e0, L.colg, L.b.to(DEV), RELAX, xg)   # builds L too
    st = G._slabs(Ag, L.colg)
    upper, lower = st.upper, st.lower
    # symmetric positive scaling s_i a_ij s_j keeps the matrix an M-matrix
    g = torch.Generator().manual_seed(26)
    s = torch.rand(L.A.n_rows, generator=g, dtype=torch.float64) + 0.5
    ro = L.A.row_offsets.long()
    rows = torch.repeat_interleave(torch.arange(L.A.n_rows), ro[1:] - ro[:-1])
    scale = s[rows] * s[L.A.col_indices.long()]
    Ag.values.mul_(scale.to(DEV))
    A2 = CSRMatrix(L.A.row_offsets, L.A.col_indices, L.A.values * scale)
    einv2 = cpu_ops.dilu_setup(A2, L.col)
    e1 = ops.dilu_setup(Ag, L.colg)
    st1 = G._slabs(Ag, L.colg)
    assert st1 is st and st1.upper is upper and st1.lower is lower
    assert torch.allclose(e1.einv.cpu(), einv2, rtol=1e-12, atol=1e-13)
    x1, x2 = L.x0.clone(), L.x0.to(DEV)
    host_smooth(L, x1, A=A2, einv=einv2)
    assert G.dilu_smooth(Ag, e1, L.colg, L.b.to(DEV), x2, RELAX) is True
    assert torch.allclose(x2.cpu(), x1, **F64)
    cpu_ops.dilu_solve(A2, einv2, L.col, L.b, RELAX, x1)
    ops.dilu_solve(Ag, e1, L.colg, L.b.to(DEV), RELAX, x2)
    assert torch.allclose(x2.cpu(), x1, **F64)


# ---------------------------------------------------------------- type pairs
@gpu
def test_fp32_matrix_fp64_vectors(levels):
    L = levels["2d"]
    A32g = CSRMatrix(L.A.row_offsets, L.A.col_indices,
                     L.A.values.to(torch.float32),
                     n_cols=L.A.n_cols).to(DEV)
    e_gpu = ops.dilu_setup(A32g, L.colg)
    assert e_gpu.va_u.dtype == torch.float32
    x1, x2 = L.x0.clone(), L.x0.to(DEV)
    for _ in range(3):
        host_smooth(L, x1)
        assert gpu_ops().dilu_smooth(A32g, e_gpu, L.colg, L.b.to(DEV), x2,
                                     RELAX) is True
    assert x2.dtype == torch.float64
    show("smooth", x2, x1)
    assert torch.allclose(x2.cpu(), x1, **F32)
    cpu_ops.dilu_solve(L.A, L.einv, L.col, L.b, RELAX, x1)
    ops.dilu_solve(A32g, e_gpu, L.colg, L.b.to(DEV), RELAX, x2)
    show("solve", x2, x1)
    assert torch.allclose(x2.cpu(), x1, **F32)


@gpu
def test_complex_dZZI():
    Z = torch.complex128
    tol = dict(rtol=1e-12, atol=1e-12)
    P = poisson_2d(129, 128).to_scipy().astype(np.complex128)
    n = P.shape[0]
    K = sp.diags([0.3j * np.ones(n - 1), -0.2j * np.ones(n - 1)], [1, -1])
    S = (P + K + (0.5 + 0.8j) * sp.identity(n)).tocsr()
    Ah = CSRMatrix.from_scipy(S, dtype=Z)
    Ag = CSRMatrix.from_scipy(S, device=DEV, dtype=Z)
    assert n > small_rows()
    colg = MatrixColoring.create(Ag)
    col = host_coloring(colg)
    rng = np.random.RandomState(27)
    b = torch.from_numpy(rng.rand(n) + 1j * (rng.rand(n) - 0.3))
    x0 = torch.from_numpy(rng.rand(n) + 1j * (rng.rand(n) + 0.6))
    e_ref = cpu_ops.dilu_setup(Ah, col)
    e_gpu = ops.dilu_setup(Ag, colg)
    x1, x2 = x0.clone(), x0.to(DEV)
    cpu_ops.dilu_solve(Ah, e_ref, col, cpu_ops.residual(Ah, x1, b), RELAX, x1)
    assert gpu_ops().dilu_smooth(Ag, e_gpu, colg, b.to(DEV), x2, RELAX) \
        is True
    assert x2.dtype == Z
    show("smooth", x2, x1)
    assert torch.allclose(x2.cpu(), x1, **tol)
    y1 = torch.zeros(n, dtype=Z)
    y2 = y1.to(DEV)
    cpu_ops.dilu_solve(Ah, e_ref, col, b, RELAX, y1)
    ops.dilu_solve(Ag, e_gpu, colg, b.to(DEV), RELAX, y2)
    show("solve", y2, y1)
    assert torch.allclose(y2.cpu(), y1, **tol)


# ---------------------------------------------------------------- cycle
def cycle_with_and_without_skip(device, monkeypatch):
    """One flagship V-cycle from a zero guess with the residual of the zero
    vector skipped and computed: (x_skip, x_full, calls_skip, calls_full,
    number of non-coarsest levels)."""
    from bench import FGMRES_AGG
    from amgx_amd.amg import amg as amg_mod
    A = poisson_3d(20, 20, 20, device=device)
    s = create_solver(AMGConfig.from_dict(FGMRES_AGG).root_scope(),
                      resources=Resources(device))
    s.setup(A)
    hier = s.precond.hierarchy
    assert hier.presweeps == 0 and hier._skip_zero_residual
    calls = [0]
    real = amg_mod.ops.residual

    def counting(*args, **kwargs):
        calls[0] += 1
        return real(*args, **kwargs)
    monkeypatch.setattr(amg_mod.ops, "residual", counting)
    g = torch.Generator().manual_seed(28)
    b = torch.rand(A.n_rows, generator=g, dtype=torch.float64).to(device)
    out = []
    for skip in (True, False):
        hier._skip_zero_residual = skip
        calls[0] = 0
        x = torch.full_like(b, 7.0)      # a zero guess ignores what x holds
        hier.cycle(b, x, zero_initial_guess=True)
        out.append((x.cpu(), calls[0]))
    hier._skip_zero_residual = True
    (x_skip, c_skip), (x_full, c_full) = out
    return x_skip, x_full, c_skip, c_full, len(hier.levels) - 1


def check_cycle(device, monkeypatch):
    x_skip, x_full, c_skip, c_full, n_fine = \
        cycle_with_and_without_skip(device, monkeypatch)
    assert n_fine >= 2
    rel = float(torch.linalg.vector_norm(x_skip - x_full)
                / torch.linalg.vector_norm(x_full))
    print("levels", n_fine + 1, "residual calls", c_skip, c_full, "rel", rel)
    assert rel <= 1e-13
    assert c_full - c_skip == n_fine


def test_cycle_skips_zero_residual_cpu(monkeypatch):
    check_cycle("cpu", monkeypatch)


@gpu
def test_cycle_skips_zero_residual_gpu(monkeypatch):
    check_cycle(DEV, monkeypatch)
