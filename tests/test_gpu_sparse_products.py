"""The device sparse-product family against a plain per-row reference, at the
edges of the LDS hash ladder (kernels_spgemm.hip: 64 -> 512 -> top cap ->
sort fallback): `ops.spgemm` and `_core.spgemm_hash` (mode 0), the ESC path
`_core.spgemm`, `ops.galerkin_aggregation` (mode 1), `ops.galerkin_rap`,
`ops.ilu1_pattern` and `ops.transpose`.

All values are small integers times 2^k (tests/sparse_product_inputs.py), so
every result is exact in every value type and every comparison here is
bitwise: row offsets, columns (strictly ascending in each row) and values
equal to the reference, which stores the STRUCTURAL product (an entry whose
terms cancel, or that comes from a stored zero, stays)."""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from amgx_amd import CSRMatrix, _core, ops
from amgx_amd.amg.coloring import MatrixColoring
from amgx_amd.ops import cpu as cpu_ops
from amgx_amd.ops import gpu as gpu_ops

from tests.sparse_product_inputs import (SHORT_ROWS, Csr, csr_from_rows,
                                         exact_values, overlapping_pieces,
                                         reference_product, take_rows,
                                         tier_edge_case, tier_edge_families,
                                         transpose_reference)
from tests.test_gpu_ilu1 import assert_same_matrix

DEV = "cuda:0"
REAL = [torch.float64, torch.float32]
ALL = REAL + [torch.complex128, torch.complex64]


def name(dtype):
    return str(dtype).split(".")[-1]


def ids(dtypes):
    return [name(d) for d in dtypes]


def idx(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def on_gpu(M, dtype):
    return CSRMatrix(idx(M.ro), idx(M.ci),
                     torch.from_numpy(M.va).to(dtype).to(DEV),
                     n_cols=M.n_cols)


def check_exact(ro, ci, va, ref, dtype):
    ro, ci, va = ro.cpu(), ci.cpu(), va.cpu()
    assert ro.dtype == torch.int32 and ci.dtype == torch.int32
    assert torch.equal(ro.to(torch.int64), torch.from_numpy(ref.ro))
    assert torch.equal(ci.to(torch.int64), torch.from_numpy(ref.ci))
    if ci.numel() > 1:          # strictly ascending inside every row
        ascending = np.diff(ci.numpy().astype(np.int64)) > 0
        starts = ro.numpy().astype(np.int64)[1:-1]
        starts = starts[(starts > 0) & (starts < ci.numel())]
        ascending[starts - 1] = True      # a row boundary, not a step
        assert ascending.all()
    assert va.dtype == dtype
    assert torch.equal(va, torch.from_numpy(ref.va).to(dtype))


def check_matrix(C, ref, dtype):
    assert C.is_cuda and C.block_dim == 1
    assert C.n_rows == len(ref.ro) - 1 and C.n_cols == ref.n_cols
    assert C.dtype == dtype
    check_exact(C.row_offsets, C.col_indices, C.values, ref, dtype)


def spgemm_hash(A, B, cap0):
    cap = max(gpu_ops._expansion_bound(A, B), 1)
    return _core.spgemm_hash(A.row_offsets, A.col_indices, A.values,
                             B.row_offsets, B.col_indices, B.values, None, 0,
                             cap, cap0)


def spgemm_esc(A, B):
    cap = max(gpu_ops._expansion_bound(A, B), 1)
    return _core.spgemm(A.row_offsets, A.col_indices, A.values,
                        B.row_offsets, B.col_indices, B.values, B.n_cols, cap)


# ------------------------------------------------------- structural pattern
def cancelling_pair():
    """Row 0: the terms of column 0 cancel. Row 1: a stored zero of A."""
    A = csr_from_rows([[0, 1], [0]], [[1.0, 1.0], [0.0]], 2, np.float64)
    B = csr_from_rows([[0, 1], [0, 2]], [[2.0, 1.0], [-2.0, 3.0]], 3,
                      np.float64)
    C = Csr(np.array([0, 3, 5]), np.array([0, 1, 2, 0, 1]),
            np.array([0.0, 1.0, 3.0, 0.0, 0.0]), 3)
    return A, B, C


def test_cancelled_and_stored_zero_entries_are_kept():
    A, B, C = cancelling_pair()
    ref = reference_product(A, B)
    assert all(np.array_equal(x, y) for x, y in zip(ref[:3], C[:3]))
    Ag, Bg = on_gpu(A, torch.float64), on_gpu(B, torch.float64)
    check_matrix(ops.spgemm(Ag, Bg), C, torch.float64)
    check_exact(*spgemm_esc(Ag, Bg), C, torch.float64)


# ------------------------------------------------------- a. tier edges
@functools.lru_cache(maxsize=None)
def edge_case(top_cap, cplx):
    """The tier-edge matrices with SHORT_ROWS short rows and their reference
    product, built once and never modified; its rows without the short
    ones; its rows without the short and the top-tier ones."""
    case = tier_edge_case(top_cap, cplx, short_rows=SHORT_ROWS)
    ref = reference_product(case.A, case.B)
    assert np.array_equal(np.diff(ref.ro), case.widths)
    long_rows = np.flatnonzero(~case.short)
    mid_rows = np.flatnonzero(~case.short & (case.widths < top_cap - 1))
    out = {"all": (case.A, ref, case.widths)}
    for key, rows in (("long", long_rows), ("below_top", mid_rows)):
        out[key] = (take_rows(case.A, rows), take_rows(ref, rows),
                    case.widths[rows])
    return case.B, out


def edge(dtype, part):
    top_cap = _core.SPGEMM_HASH_TOP_CAP[name(dtype)]
    assert top_cap == (4096 if dtype == torch.complex128 else 8192)
    B, parts = edge_case(top_cap, dtype.is_complex)
    A, ref, widths = parts[part]
    assert np.array_equal(np.diff(ref.ro), widths)
    assert B.n_cols == top_cap + 64
    return A, B, ref, widths, top_cap


def test_tier_edge_widths_are_the_intended_ones():
    A, B, ref, widths, top_cap = edge(torch.float64, "long")
    got = np.diff(ref.ro)
    for w, count in tier_edge_families(top_cap):
        assert np.count_nonzero(got == w) == count + (4 if w == 64 else 0)
    # empty rows of A at the start, in the middle and at the end; rows of A
    # that only hit empty rows of B
    empty_a = np.diff(A.ro) == 0
    assert empty_a[:2].all() and empty_a[-2:].all() and empty_a.sum() == 6
    assert np.count_nonzero((got == 0) & ~empty_a) == 3
    b_width = np.diff(B.ro)
    assert b_width[0] == 0 and b_width[-1] == 0
    assert np.count_nonzero(b_width[1:-1] == 0) >= 3
    # the map really accumulates: rows with more expanded terms than entries
    terms = np.add.reduceat(b_width[A.ci], A.ro[:-1][~empty_a])
    assert np.count_nonzero(terms > got[~empty_a]) > 300


@pytest.mark.parametrize("cap0", [64, 512])
@pytest.mark.parametrize("dtype", ALL, ids=ids(ALL))
def test_tier_edge_hash_ladder(dtype, cap0):
    A, B, ref, widths, top_cap = edge(dtype, "all")
    ro, ci, va, big = spgemm_hash(on_gpu(A, dtype), on_gpu(B, dtype), cap0)
    assert int(ro[0]) != -1
    # the top tier gets exactly the rows wider than 512, no false overflow
    assert np.array_equal(np.sort(big.cpu().numpy()),
                          np.flatnonzero(widths > 512))
    gpu_ops._sort_unsorted_rows(ro, ci, va, big)
    check_exact(ro, ci, va, ref, dtype)


@pytest.mark.parametrize("part,cap0", [("all", 64), ("long", 512)])
@pytest.mark.parametrize("dtype", ALL, ids=ids(ALL))
def test_tier_edge_ops_spgemm(dtype, part, cap0):
    A, B, ref, widths, top_cap = edge(dtype, part)
    Ag, Bg = on_gpu(A, dtype), on_gpu(B, dtype)
    # the first tier ops.spgemm's heuristic picks for this input
    bound = gpu_ops._expansion_bound(Ag, Bg)
    assert bound == int(np.diff(B.ro)[A.ci].sum())
    assert (64 if bound <= 48 * Ag.n_rows else 512) == cap0
    check_matrix(ops.spgemm(Ag, Bg), ref, dtype)


# ------------------------------------------------------- b. past the top
@pytest.mark.parametrize("dtype", ALL, ids=ids(ALL))
def test_row_past_the_top_tier_takes_the_sort_path(dtype):
    top_cap = _core.SPGEMM_HASH_TOP_CAP[name(dtype)]
    rng = np.random.RandomState(21)
    cplx = dtype.is_complex
    n_cols = top_cap + 64
    widths = [3, top_cap + 1, 0, 70]
    b_cols = [np.sort(rng.choice(n_cols, size=w, replace=False))
              for w in widths]
    B = csr_from_rows(b_cols, [exact_values(rng, w, cplx) for w in widths],
                      n_cols, np.complex128 if cplx else np.float64)
    a_cols = [[0], [1], [2], [0, 3], []]
    A = csr_from_rows(a_cols, [exact_values(rng, len(c), cplx)
                               for c in a_cols], 4, B.va.dtype)
    ref = reference_product(A, B)
    assert np.diff(ref.ro).max() == top_cap + 1
    Ag, Bg = on_gpu(A, dtype), on_gpu(B, dtype)
    ro, ci, va, big = spgemm_hash(Ag, Bg, 64)
    assert int(ro[0]) == -1 and ci.numel() == 0 and va.numel() == 0
    check_matrix(ops.spgemm(Ag, Bg), ref, dtype)


# ------------------------------------------------------- c. ESC directly
ESC_TYPES = REAL + [torch.complex128]


@pytest.mark.parametrize("dtype", ESC_TYPES, ids=ids(ESC_TYPES))
def test_esc_on_the_tier_edge_matrix(dtype):
    A, B, ref, widths, top_cap = edge(dtype, "below_top")
    assert widths.max() == 513
    check_exact(*spgemm_esc(on_gpu(A, dtype), on_gpu(B, dtype)), ref, dtype)


@pytest.mark.parametrize("dtype", ESC_TYPES, ids=ids(ESC_TYPES))
def test_esc_empty_leading_and_trailing_rows_and_empty_expansion(dtype):
    rng = np.random.RandomState(22)
    cplx = dtype.is_complex
    np_type = np.complex128 if cplx else np.float64
    b_cols = [[], [5, 1, 9], [], [9, 0, 3, 7], []]
    B = csr_from_rows(b_cols, [exact_values(rng, len(c), cplx)
                               for c in b_cols], 10, np_type)

    def product(a_cols):
        A = csr_from_rows(a_cols, [exact_values(rng, len(c), cplx)
                                   for c in a_cols], 5, np_type)
        ref = reference_product(A, B)
        got = spgemm_esc(on_gpu(A, dtype), on_gpu(B, dtype))
        check_exact(*got, ref, dtype)
        return np.diff(ref.ro)

    # rows 0, 1 and 5, 6 of C are empty: no entry of A, or empty rows of B
    w = product([[], [0, 2], [1, 3], [], [3], [4], []])
    assert w.tolist() == [0, 0, 6, 0, 4, 0, 0]
    # nnz(A) > 0 and nothing to expand
    w = product([[0], [2, 4], [], [4]])
    assert w.tolist() == [0, 0, 0, 0]


# ------------------------------------------------------- d. Galerkin, mode 1
@functools.lru_cache(maxsize=None)
def galerkin_case():
    """Fine matrix, aggregates of sizes 1, 2 and 5 and the reference
    P^T A P. For each size, three coarse rows of every width 60..64 and two
    of width 512; the other coarse rows are 1..8 wide. The members of an
    aggregate reach overlapping parts of the row, and a fine row holds two
    columns of one aggregate now and then (lanes with one key in a step)."""
    rng = np.random.RandomState(5)
    sizes = np.tile([1, 2, 5], 300)
    nc, n = sizes.size, int(sizes.sum())
    first = np.concatenate([[0], np.cumsum(sizes)])
    agg = np.repeat(np.arange(nc), sizes)
    intended = rng.randint(1, 9, size=nc)
    for cls in range(3):
        mine = np.arange(cls, nc, 3)
        edge_w = [w for w in range(60, 65) for _ in range(3)] + [512, 512]
        intended[rng.choice(mine, size=len(edge_w), replace=False)] = edge_w
    rows = [None] * n
    for I in range(nc):
        w, s = int(intended[I]), int(sizes[I])
        reach = rng.choice(nc, size=w, replace=False)
        parts = overlapping_pieces(rng, reach, min(s, w))
        while len(parts) < s:
            parts.append(rng.choice(reach, size=rng.randint(1, w + 1),
                                    replace=False))
        for f, part in zip(range(first[I], first[I + 1]), parts):
            cols = []
            for c in part:
                members = np.arange(first[c], first[c + 1])
                take = 2 if members.size > 1 and rng.rand() < 0.3 else 1
                cols += list(rng.choice(members, size=take, replace=False))
            rows[f] = np.sort(np.array(cols))
    A = csr_from_rows(rows, [exact_values(rng, len(c)) for c in rows], n,
                      np.float64)
    ones = np.ones(n)
    P = Csr(np.arange(n + 1), agg, ones, nc)
    ref = reference_product(transpose_reference(P), reference_product(A, P))
    assert np.array_equal(np.diff(ref.ro), intended)
    return A, agg, nc, ref, sizes


@pytest.mark.parametrize("generator", [None, "THRUST"])
@pytest.mark.parametrize("dtype", REAL, ids=ids(REAL))
def test_galerkin_aggregation_at_the_tier_edges(dtype, generator):
    A, agg, nc, ref, sizes = galerkin_case()
    width = np.diff(ref.ro)
    for s in (1, 2, 5):
        for w in (60, 61, 62, 63, 64, 512):
            assert np.count_nonzero((sizes == s) & (width == w)) >= 2
    assert len(A.ci) <= 48 * nc             # the ladder is entered at 64
    Ac = ops.galerkin_aggregation(on_gpu(A, dtype), idx(agg), nc,
                                  generator=generator)
    check_matrix(Ac, ref, dtype)


# ------------------------------------------------------- e. ILU(1) pattern
@functools.lru_cache(maxsize=None)
def ilu1_case():
    """Matrix, coloring and intended pattern width of its edge rows.
    Columns 0..1999 (color 1) have only their diagonal. An edge row is
    either 'direct' (color 0: no pivot, its pattern is its own row, with or
    without a stored diagonal) or 'fill' (color 2: its diagonal, a part of
    its columns of color 1, and one to three pivots of color 0 whose rows
    bring the overlapping rest as fill)."""
    rng = np.random.RandomState(9)
    n_low = 2000
    rows = [np.array([j]) for j in range(n_low)]
    colors = [1] * n_low
    intended = {}

    def add(color):
        rows.append(None)
        colors.append(color)
        return len(rows) - 1

    for w in [60, 61, 62, 63, 64, 512, 512]:
        for stored_diagonal in (True, False):
            i = add(0)
            low = rng.choice(n_low, size=w - 1, replace=False)
            rows[i] = np.sort(np.append(low, i) if stored_diagonal else low)
            intended[i] = w
        for t in (1, 2, 3):
            i = add(2)
            low = rng.choice(n_low, size=w - 1 - t, replace=False)
            parts = overlapping_pieces(rng, low, t + 1)
            pivots = []
            for part in parts[1:]:
                k = add(0)
                rows[k] = np.sort(np.append(part, k))
                pivots.append(k)
            rows[i] = np.sort(np.concatenate([parts[0], pivots, [i]]))
            intended[i] = w
    n = len(rows)
    A = csr_from_rows(rows, [exact_values(rng, len(c)) for c in rows], n,
                      np.float64)
    return A, np.array(colors, dtype=np.int32), intended


def test_ilu1_pattern_at_the_tier_edges():
    A, colors, intended = ilu1_case()
    Ah = CSRMatrix(torch.from_numpy(A.ro.astype(np.int32)),
                   torch.from_numpy(A.ci.astype(np.int32)),
                   torch.from_numpy(A.va), n_cols=A.n_cols)
    F = cpu_ops.ilu1_pattern(Ah, MatrixColoring(torch.from_numpy(colors), 3))
    width = torch.diff(F.row_offsets).numpy()
    for i, w in intended.items():
        assert width[i] == w
    # A's own row brings 60 and more columns in one step
    own = np.diff(A.ro)
    assert sum(1 for i in intended if 60 <= own[i] <= 64) >= 5
    Fg = ops.ilu1_pattern(on_gpu(A, torch.float64),
                          MatrixColoring(torch.from_numpy(colors).to(DEV), 3))
    assert_same_matrix(Fg, F)


# ------------------------------------------------------- f. transpose
def random_csr(rng, m, n, max_per_row, empty_rows=(), empty_cols=(),
               sort=True):
    allowed = np.setdiff1d(np.arange(n), empty_cols)
    rows = []
    for i in range(m):
        k = 0 if i in empty_rows else rng.randint(1, max_per_row + 1)
        cols = rng.choice(allowed, size=min(k, allowed.size), replace=False)
        rows.append(np.sort(cols) if sort else cols)
    return csr_from_rows(rows, [exact_values(rng, len(c)) for c in rows], n,
                         np.float64)


def sorted_rows(A):
    rows = np.repeat(np.arange(len(A.ro) - 1), np.diff(A.ro))
    order = np.lexsort((A.ci, rows))
    return Csr(A.ro, A.ci[order], A.va[order], A.n_cols)


TRANSPOSE_CASES = ["37x1000", "1000x37", "unsorted", "above_a_radix_block",
                   "1x1", "nnz0"]


@functools.lru_cache(maxsize=None)
def transpose_inputs():
    rng = np.random.RandomState(31)
    wide = random_csr(rng, 37, 1000, 40, empty_rows=(0, 17, 36),
                      empty_cols=(0, 1, 500, 501, 502, 998, 999))
    tall = random_csr(rng, 1000, 37, 6, empty_rows=(0, 1, 400, 999),
                      empty_cols=(0, 18, 36))
    unsorted = random_csr(rng, 50, 80, 30, empty_rows=(3,), sort=False)
    assert (np.diff(unsorted.ci)[:20] < 0).any()
    big = random_csr(rng, 400, 400, 400, empty_rows=(0, 399),
                     empty_cols=(0, 200, 399))
    assert len(big.ci) > 70000
    one = csr_from_rows([[0]], [[-1.5]], 1, np.float64)
    no_entries = csr_from_rows([[], [], []], [[], [], []], 5, np.float64)
    out = {"37x1000": wide, "1000x37": tall, "unsorted": unsorted,
           "above_a_radix_block": big, "1x1": one, "nnz0": no_entries}
    assert list(out) == TRANSPOSE_CASES
    return out


@pytest.mark.parametrize("case", TRANSPOSE_CASES)
@pytest.mark.parametrize("dtype", REAL, ids=ids(REAL))
def test_transpose(dtype, case):
    A = transpose_inputs()[case]
    At = ops.transpose(on_gpu(A, dtype))
    check_matrix(At, transpose_reference(A), dtype)
    check_matrix(ops.transpose(At), sorted_rows(A), dtype)


def test_transpose_rejects_complex_values():
    A = transpose_inputs()["37x1000"]
    with pytest.raises(RuntimeError, match="transpose: unsupported dtype"):
        ops.transpose(on_gpu(A, torch.complex128))


# ------------------------------------------------------- g. R A P
@functools.lru_cache(maxsize=None)
def rap_case():
    rng = np.random.RandomState(41)
    n, nc = 300, 90
    P = random_csr(rng, n, nc, 4, empty_rows=(0, 7, 150, 299),
                   empty_cols=(0, 44, 45, 89))
    A = random_csr(rng, n, n, 9)
    ref = reference_product(transpose_reference(P), reference_product(A, P))
    return P, A, ref


@pytest.mark.parametrize("dtype", REAL, ids=ids(REAL))
def test_galerkin_rap_rectangular(dtype):
    P, A, ref = rap_case()
    assert len(ref.ro) - 1 == 90 and ref.n_cols == 90
    assert (np.diff(ref.ro) == 0).sum() >= 4        # the empty columns of P
    Pg = on_gpu(P, dtype)
    R = ops.transpose(Pg)
    check_matrix(ops.galerkin_rap(R, on_gpu(A, dtype), Pg), ref, dtype)


# ------------------------------------------------------- h. degenerate
DEGENERATE = [torch.float64, torch.complex64]


@pytest.mark.parametrize("dtype", DEGENERATE, ids=ids(DEGENERATE))
def test_empty_products(dtype):
    rng = np.random.RandomState(51)
    cplx = dtype.is_complex
    np_type = np.complex128 if cplx else np.float64
    b_cols = [[1, 4], [0], [2, 3, 6]]
    B = csr_from_rows(b_cols, [exact_values(rng, len(c), cplx)
                               for c in b_cols], 7, np_type)
    B0 = csr_from_rows([[], [], []], [[], [], []], 7, np_type)
    a_cols = [[0, 2], [1], [], [2]]
    A = csr_from_rows(a_cols, [exact_values(rng, len(c), cplx)
                               for c in a_cols], 3, np_type)
    no_rows = csr_from_rows([], [], 3, np_type)
    no_entries = csr_from_rows([[]] * 4, [[]] * 4, 3, np_type)
    for a, b, m in ((no_rows, B, 0), (no_entries, B, 4), (A, B0, 4)):
        C = ops.spgemm(on_gpu(a, dtype), on_gpu(b, dtype))
        check_matrix(C, reference_product(a, b), dtype)
        assert C.n_rows == m and C.n_cols == 7 and C.nnz == 0
        assert C.row_offsets.cpu().tolist() == [0] * (m + 1)
        assert C.values.numel() == 0


# ------------------------------------------------------- i. reproducibility
def test_mode0_is_bitwise_reproducible():
    """Inexact values: the sums depend on their order, and for one key that
    order is the program order of one wave."""
    A, B, ref, widths, top_cap = edge(torch.float64, "long")
    rng = np.random.RandomState(61)
    Ag = on_gpu(A._replace(va=rng.rand(len(A.ci)) - 0.5), torch.float64)
    Bg = on_gpu(B._replace(va=rng.rand(len(B.ci)) - 0.5), torch.float64)
    first, second = ops.spgemm(Ag, Bg), ops.spgemm(Ag, Bg)
    assert torch.equal(first.row_offsets, second.row_offsets)
    assert torch.equal(first.col_indices, second.col_indices)
    assert torch.equal(first.values, second.values)
    assert torch.equal(first.col_indices.cpu().to(torch.int64),
                       torch.from_numpy(ref.ci))
