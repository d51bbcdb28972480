"""Color-aware ILU(1) fill (ilu_fill_pattern=COLORED) on the host: the
pattern rule against a plain triple loop, the factors against dense block
elimination, and MULTICOLOR_ILU level 1 on scalar and block matrices."""

import numpy as np
import pytest
import torch

from amgx_amd import AMGConfig, CSRMatrix, create_solver, ops
from amgx_amd.amg.coloring import MatrixColoring
from amgx_amd.config import ConfigScope
from amgx_amd.ops import cpu as cpu_ops
from amgx_amd.problems import block_laplacian, poisson_2d
from amgx_amd.resources import Resources
from amgx_amd.solvers.ilu import extended_sparsity


def coloring_of(A, level=1):
    return MatrixColoring.create(
        A, ConfigScope(None, {"matrix_coloring_scheme": "MIN_MAX",
                              "coloring_level": level}))


def oracle_pattern(A, colors):
    """The pattern rule, entry by entry: row i = A's row i + i + every local
    j reached through a local pivot k of row i with c[k] < c[i], (k, j) in A,
    c[j] > c[k] and c[j] != c[i]. Returns (offsets, columns, values)."""
    n = A.n_rows
    ro = A.row_offsets.tolist()
    ci = A.col_indices.tolist()
    c = colors.tolist()
    va = A.values
    offsets, columns, values = [0], [], []
    for i in range(n):
        own = {ci[a]: a for a in range(ro[i], ro[i + 1])}
        cols = set(own) | {i}
        for a in range(ro[i], ro[i + 1]):
            k = ci[a]
            if k >= n or not c[k] < c[i]:
                continue
            for t in range(ro[k], ro[k + 1]):
                j = ci[t]
                if j < n and c[j] > c[k] and c[j] != c[i]:
                    cols.add(j)
        for j in sorted(cols):
            columns.append(j)
            values.append(va[own[j]] if j in own else torch.zeros_like(va[0]))
        offsets.append(len(columns))
    return (torch.tensor(offsets, dtype=torch.int32),
            torch.tensor(columns, dtype=torch.int32), torch.stack(values))


def assert_is_oracle(A, coloring):
    F = cpu_ops.ilu1_pattern(A, coloring)
    ro, ci, va = oracle_pattern(A, coloring.colors)
    assert F.n_rows == A.n_rows and F.n_cols == A.n_cols
    assert F.block_dim == A.block_dim and F.dtype == A.dtype
    assert torch.equal(F.row_offsets, ro)
    assert torch.equal(F.col_indices, ci)
    assert torch.equal(F.values, va)
    return F


def missing_diagonal_matrix():
    m = poisson_2d(5, 5).to_scipy().tolil()
    m[7, 7] = 0.0
    m = m.tocsr()
    m.eliminate_zeros()
    return CSRMatrix.from_scipy(m)


def halo_matrix():
    """6 local rows, columns 6 and 7 are halo. Local graph: the path
    0-1-2-3-4-5 plus the edges (0,4) and (1,5)."""
    edges = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (0, 4), (1, 5)]
    rows, cols, vals = [], [], []
    for i in range(6):
        rows.append(i), cols.append(i), vals.append(4.0 + i)
    for t, (i, j) in enumerate(edges):
        rows += [i, j]
        cols += [j, i]
        vals += [-1.0 - 0.1 * t, -1.5 - 0.1 * t]
    for t, (i, h) in enumerate([(0, 7), (2, 6), (3, 6), (3, 7), (5, 6)]):
        rows.append(i), cols.append(h), vals.append(-0.25 - 0.01 * t)
    A = CSRMatrix.from_coo(rows, cols, vals, 6, 8)
    colors = torch.tensor([0, 1, 2, 0, 1, 2], dtype=torch.int32)
    return A, MatrixColoring(colors, 3)


@pytest.mark.parametrize("level", [1, 2])
def test_pattern_oracle_poisson(level):
    A = poisson_2d(6, 6)
    F = assert_is_oracle(A, coloring_of(A, level))
    assert F.nnz > A.nnz


@pytest.mark.parametrize("level", [1, 2])
def test_pattern_oracle_block(level):
    A = block_laplacian(4, 4, block_dim=3)
    col = coloring_of(A, level)
    F = assert_is_oracle(A, col)
    assert F.values.shape[1:] == (3, 3)
    # a two-colored grid has no fill at all: every fill candidate of a row
    # wears the row's own color
    assert F.nnz > A.nnz or col.num_colors == 2
    assert level == 1 or F.nnz > A.nnz


def test_pattern_oracle_missing_diagonal():
    A = missing_diagonal_matrix()
    assert int(A.diag_index()[7]) < 0
    F = assert_is_oracle(A, coloring_of(A))
    assert (F.diag_index() >= 0).all()
    assert F.values[F.diag_index()[7]] == 0.0


def test_pattern_oracle_halo_columns():
    A, col = halo_matrix()
    F = assert_is_oracle(A, col)
    assert F.nnz > A.nnz
    n = A.n_rows
    # the halo entries are carried over as they are ...
    rows_a = np.repeat(np.arange(n), np.diff(A.row_offsets.numpy()))
    rows_f = np.repeat(np.arange(n), np.diff(F.row_offsets.numpy()))
    ha, hf = A.col_indices >= n, F.col_indices >= n
    assert np.array_equal(rows_a[ha.numpy()], rows_f[hf.numpy()])
    assert torch.equal(A.col_indices[ha], F.col_indices[hf])
    assert torch.equal(A.values[ha], F.values[hf])
    # ... and change nothing in the local part: it is the pattern of the
    # local matrix alone (halo columns neither expanded nor pivots)
    keep = ~ha.numpy()
    local = CSRMatrix.from_coo(rows_a[keep], A.col_indices[~ha].numpy(),
                               A.values[~ha].numpy(), n, n)
    L = cpu_ops.ilu1_pattern(local, col)
    assert torch.equal(L.col_indices, F.col_indices[~hf])
    assert torch.equal(L.values, F.values[~hf])


@pytest.mark.parametrize("level", [1, 2])
def test_fill_counts(level):
    A = poisson_2d(14, 14)
    col = coloring_of(A, level)
    F = cpu_ops.ilu1_pattern(A, col)
    power = extended_sparsity(A, 1)
    print(f"coloring_level={level}: nnz(A)={A.nnz} colored={F.nnz} "
          f"colors={col.num_colors} power={power.nnz}")
    assert F.nnz > A.nnz
    assert F.nnz < power.nnz
    c = col.colors.numpy()
    rows = np.repeat(np.arange(A.n_rows), np.diff(F.row_offsets.numpy()))
    cols = F.col_indices.numpy()
    off = rows != cols
    assert not (c[rows[off]] == c[cols[off]]).any()


@pytest.mark.parametrize("level", [1, 2])
def test_factors_match_dense_block_elimination(level):
    """ilu0_setup on the colored pattern = dense IKJ block elimination in
    color order restricted to that pattern."""
    A = block_laplacian(4, 4, block_dim=2)
    col = coloring_of(A, level)
    F = cpu_ops.ilu1_pattern(A, col)
    assert level == 1 or F.nnz > A.nnz
    n, b = F.n_rows, F.block_dim
    order = np.lexsort((np.arange(n), col.colors.numpy()))
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n)
    rows = np.repeat(np.arange(n), np.diff(F.row_offsets.numpy()))
    cols = F.col_indices.numpy()
    D = np.zeros((n, n, b, b))
    M = np.zeros((n, n), dtype=bool)
    D[pos[rows], pos[cols]] = F.values.numpy()
    M[pos[rows], pos[cols]] = True
    for i in range(n):
        for k in range(i):
            if not M[i, k]:
                continue
            D[i, k] = D[i, k] @ np.linalg.inv(D[k, k])
            for j in range(k + 1, n):
                if M[i, j] and M[k, j]:
                    D[i, j] -= D[i, k] @ D[k, j]
    lu = cpu_ops.ilu0_setup(F, col).numpy()
    np.testing.assert_allclose(lu, D[pos[rows], pos[cols]], rtol=1e-12,
                               atol=1e-13)


def fgmres_ilu(A, level, **ilu):
    cfg = AMGConfig.from_dict({
        "solver": "FGMRES", "max_iters": 200, "gmres_n_restart": 40,
        "monitor_residual": 1, "tolerance": 1e-10,
        "convergence": "RELATIVE_INI",
        "preconditioner": dict({"solver": "MULTICOLOR_ILU", "max_iters": 1,
                                "ilu_sparsity_level": level}, **ilu)})
    s = create_solver(cfg.root_scope(), resources=Resources("cpu"))
    b = torch.ones(A.n_rows * A.block_dim, dtype=torch.float64)
    x = torch.zeros_like(b)
    s.setup(A)
    st = s.solve(b, x, zero_initial_guess=True)
    rel = float(ops.nrm2(ops.residual(A, x, b)) / ops.nrm2(b))
    assert st.converged and rel < 1e-8, f"ILU({level}) {ilu}: {st} rel={rel}"
    return st.iterations


@pytest.mark.parametrize("make", [
    lambda: block_laplacian(10, 10, block_dim=3, seed=5),
    lambda: block_laplacian(8, 8, block_dim=4, seed=6)], ids=["b3", "b4"])
def test_block_ilu1_preconditions_fgmres(make):
    A = make()
    it0 = fgmres_ilu(A, 0, coloring_level=2)
    it1 = fgmres_ilu(A, 1, coloring_level=2)
    print(f"FGMRES iterations: ILU(0) {it0}, ILU(1) {it1}")
    assert it1 <= it0


def test_fill_pattern_config():
    A = poisson_2d(14, 14)
    colored = fgmres_ilu(A, 1, ilu_fill_pattern="COLORED")
    default = fgmres_ilu(A, 1)
    auto = fgmres_ilu(A, 1, ilu_fill_pattern="AUTO")
    power = fgmres_ilu(A, 1, ilu_fill_pattern="POWER")
    print(f"iterations: colored {colored}, default {default}, power {power}")
    assert default == auto == power
    assert colored <= fgmres_ilu(A, 0)
    with pytest.raises(NotImplementedError, match="csr_sparsity_ilu1"):
        fgmres_ilu(A, 2, ilu_fill_pattern="COLORED")
    assert fgmres_ilu(A, 2, ilu_fill_pattern="POWER") <= power
    B = block_laplacian(4, 4, block_dim=2)
    with pytest.raises(NotImplementedError, match="scalar-only"):
        fgmres_ilu(B, 1, ilu_fill_pattern="POWER")
    with pytest.raises(ValueError):
        fgmres_ilu(A, 1, ilu_fill_pattern="DENSE")
