"""Dense-loop references of the block-CSR smoothers and of the SpMV family,
and the host backend (ops/cpu.py) against them on the inputs of
tests/block_inputs.py. tests/test_gpu_block.py holds the device against the
same loops.

The references are numpy loops over dense b x b blocks, row by row; they use
no sparse product and nothing of amgx_amd.ops. Each takes `dt`: float64 for
the reference proper, float32 to evaluate the same loops with every
intermediate rounded to float32. The largest deviation of the two, relative
to the largest magnitude of the float64 result, is d32 (rounding_scale), the
float32 rounding scale of one operation on one input; the tests bound a
float32 run by 8 * d32 and a float64 run by 8 * d32 * 2^-29 (unit roundoffs
2^-24 and 2^-53).

THE RULES both backends and these loops follow:
 * l1 sign: component r of a diagonal block takes the l1 norm s of the
   off-diagonal blocks of its row with its own sign: D_rr + s where
   D_rr >= 0, D_rr - s where D_rr < 0. A missing diagonal block is zero.
 * singular block (gauss_jordan_inv): Gauss-Jordan with partial pivoting
   (first largest magnitude); a pivot column that is exactly zero at its step
   gets a unit pivot, and counts as a pivot of magnitude 0.
 * block DILU fallback (dilu_block_inverse): with dmax = max|D_i| (0 where
   the row stores no diagonal block), the Gauss-Jordan inverse of E_i is kept
   only if max|E_i| <= 1e10 (dmax + 1) and the smallest pivot magnitude is
   >= tau * (dmax if dmax > 0 else 1), tau = 1e-10 for float64 matrices and
   1e-5 for float32 ones, a NaN failing either test. Otherwise Einv_i is the
   Gauss-Jordan inverse of D_i, or the identity where there is no D_i.
 * ILU(0): a pivot row without a diagonal block has a unit one; halo columns
   take no part."""

import functools

import numpy as np
import pytest
import torch

from amgx_amd import AMGConfig, CSRMatrix, create_solver
from amgx_amd.ops import cpu as cpu_ops
from tests import block_inputs as bi

BLOCK_SIZES = (2, 3, 4, 5, 8, 9, 16)
OMEGA = 0.75


# ------------------------------------------------------------------ helpers
def rounding_scale(f):
    """(float64 result, d32) of the reference f(dt)."""
    with np.errstate(all="ignore"):
        r64 = np.asarray(f(np.float64), dtype=np.float64)
        r32 = np.asarray(f(np.float32), dtype=np.float64)
    ok = np.isfinite(r64)
    assert (np.isfinite(r32) == ok).all()
    scale = np.abs(r64[ok]).max()
    return r64, float(np.abs(r64[ok] - r32[ok]).max() / scale)


def bound(d32, dtype):
    """Error bound of a device or host run in `dtype` arithmetic."""
    return 8.0 * d32 * (1.0 if dtype == torch.float32 else 2.0 ** -29)


def rel_err(got, ref, rows=None):
    """max|got - ref| over the finite entries of ref (optionally of block
    rows `rows`) relative to the largest finite |ref| of the whole result."""
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    ok = np.isfinite(ref)
    scale = np.abs(ref[ok]).max()
    if rows is not None:
        keep = np.zeros(ref.shape[0], dtype=bool)
        keep[rows] = True
        ok &= keep.reshape((-1,) + (1,) * (ref.ndim - 1))
    assert np.isfinite(got[ok]).all()
    return float(np.abs(got[ok] - ref[ok]).max() / scale)


def _arr(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) \
        else np.asarray(v)


def diag_pos(case):
    out = np.full(case.n_rows, -1, dtype=np.int64)
    for i in range(case.n_rows):
        for k in range(case.ro[i], case.ro[i + 1]):
            if case.ci[k] == i:
                out[i] = k
    return out


def trans_pos(case):
    where = {(i, int(case.ci[k])): k for i in range(case.n_rows)
             for k in range(case.ro[i], case.ro[i + 1])}
    return np.array([where.get((int(case.ci[k]), i), -1)
                     for i in range(case.n_rows)
                     for k in range(case.ro[i], case.ro[i + 1])],
                    dtype=np.int64)


def color_order(case):
    """Rows by colour, ascending row number within a colour."""
    return np.lexsort((np.arange(case.n_rows), case.colors))


def pivot_floor(dtype):
    return 1e-5 if dtype == torch.float32 else 1e-10


# ---------------------------------------------------------------- references
def ref_spmv(ro, ci, va, x, y, alpha=1.0, beta=0.0, gamma=0.0, bvec=None,
             r0=0, r1=None):
    """y[r0:r1] = alpha A x + beta y + gamma bvec in float64 / complex128,
    va (nnz, b, b); beta == 0 does not read y. Rows outside stay."""
    b = va.shape[1]
    wide = np.complex128 if (np.iscomplexobj(va) or np.iscomplexobj(x)) \
        else np.float64
    xb = np.asarray(x, dtype=wide).reshape(-1, b)
    out = np.array(y, dtype=wide).reshape(-1, b)
    for i in range(r0, len(ro) - 1 if r1 is None else r1):
        acc = np.zeros(b, dtype=wide)
        for k in range(ro[i], ro[i + 1]):
            acc += va[k].astype(wide) @ xb[ci[k]]
        row = alpha * acc
        if beta != 0:
            row = row + beta * out[i]
        if bvec is not None:
            row = row + gamma * np.asarray(bvec, dtype=wide).reshape(-1, b)[i]
        out[i] = row
    return out.reshape(-1)


def gauss_jordan_inv(M, dt=np.float64):
    """(inverse, smallest pivot magnitude) of one block by the singular-block
    rule of the module docstring."""
    m = np.array(M, dtype=dt)
    b = m.shape[0]
    inv = np.eye(b, dtype=dt)
    pmin = np.inf
    with np.errstate(all="ignore"):
        for k in range(b):
            piv, mx = k, abs(m[k, k])
            for r in range(k + 1, b):
                if abs(m[r, k]) > mx:
                    piv, mx = r, abs(m[r, k])
            if pmin == pmin and not mx >= pmin:
                pmin = float(mx)
            if mx == 0:
                m[k, k] = 1
            if piv != k:
                m[[k, piv]] = m[[piv, k]]
                inv[[k, piv]] = inv[[piv, k]]
            d = dt(1) / m[k, k]
            m[k] *= d
            inv[k] *= d
            for r in range(b):
                f = m[r, k]
                if r != k and f != 0:
                    m[r] -= f * m[k]
                    inv[r] -= f * inv[k]
    return inv, pmin


def dilu_block_inverse(E, D, tau, dt=np.float64):
    """(Einv_i, fell back?) by the block DILU fallback rule of the module
    docstring; D is None where the row stores no diagonal block."""
    dmax = float(np.abs(D).max()) if D is not None else 0.0
    emax = float(np.fmax.reduce(np.abs(E).ravel().astype(np.float64),
                                initial=0.0))
    inv, pmin = gauss_jordan_inv(E, dt)
    if emax <= 1e10 * (dmax + 1.0) \
            and pmin >= tau * (dmax if dmax > 0 else 1.0):
        return inv, False
    if D is None:
        return np.eye(E.shape[0], dtype=dt), True
    return gauss_jordan_inv(D, dt)[0], True


def ref_jacobi_dinv(case, l1, dt=np.float64):
    b, va = case.b, case.va.astype(dt)
    dp = diag_pos(case)
    out = np.zeros((case.n_rows, b, b), dtype=dt)
    for i in range(case.n_rows):
        D = va[dp[i]].copy() if dp[i] >= 0 else np.zeros((b, b), dtype=dt)
        if l1:
            s = np.zeros(b, dtype=dt)
            for k in range(case.ro[i], case.ro[i + 1]):
                if k != dp[i]:
                    s += np.abs(va[k]).sum(axis=1, dtype=dt)
            r = np.arange(b)
            D[r, r] += np.where(D[r, r] >= 0, s, -s)
        out[i] = gauss_jordan_inv(D, dt)[0]
    return out


def _row_product(case, va, i, v, skip_diag=False, keep=None):
    """sum_k A_ik v_k over row i (v in blocks), optionally without the
    diagonal block and over the local columns j with keep[j] only."""
    acc = np.zeros(case.b, dtype=v.dtype)
    for k in range(case.ro[i], case.ro[i + 1]):
        j = case.ci[k]
        if skip_diag and j == i:
            continue
        if keep is not None and (j >= case.n_rows or not keep[j]):
            continue
        acc += va[k] @ v[j]
    return acc


def ref_jacobi_smooth(case, dinv, rhs, x, omega, dt=np.float64):
    """One damped sweep; returns the n_rows * b owned entries."""
    va, dinv = case.va.astype(dt), np.asarray(dinv).astype(dt)
    xb = _arr(x).astype(dt).reshape(-1, case.b)
    rb = _arr(rhs).astype(dt).reshape(-1, case.b)
    out = xb[:case.n_rows].copy()
    for i in range(case.n_rows):
        res = rb[i] - _row_product(case, va, i, xb)
        out[i] = xb[i] + dt(omega) * (dinv[i] @ res)
    return out.reshape(-1)


def ref_gs_sweep(case, dinv, rhs, x, omega, symmetric, dt=np.float64):
    """One multicolour sweep, colours ascending (then descending); the rows
    of a colour are uncoupled, so their order is free. Returns all of x."""
    va, dinv = case.va.astype(dt), np.asarray(dinv).astype(dt)
    xb = _arr(x).astype(dt).reshape(-1, case.b)
    rb = _arr(rhs).astype(dt).reshape(-1, case.b)
    nc = int(case.colors.max()) + 1
    for c in list(range(nc)) + (list(range(nc - 1, -1, -1))
                                if symmetric else []):
        for i in np.nonzero(case.colors == c)[0]:
            res = rb[i] - _row_product(case, va, i, xb)
            xb[i] += dt(omega) * (dinv[i] @ res)
    return xb.reshape(-1)


def ref_dilu_setup(case, tau, dt=np.float64):
    """(Einv (n, b, b), rows that fell back, rows whose E_i was not finite):
    E_i = D_i - sum A_ij Einv_j A_ji over the local j of earlier colours
    whose transpose entry is stored."""
    b, va = case.b, case.va.astype(dt)
    dp, tp = diag_pos(case), trans_pos(case)
    einv = np.zeros((case.n_rows, b, b), dtype=dt)
    fell, nonfinite = [], []
    with np.errstate(all="ignore"):
        for i in color_order(case):
            D = va[dp[i]] if dp[i] >= 0 else None
            E = D.copy() if D is not None else np.zeros((b, b), dtype=dt)
            for k in range(case.ro[i], case.ro[i + 1]):
                j = case.ci[k]
                if j != i and j < case.n_rows and tp[k] >= 0 \
                        and case.colors[j] < case.colors[i]:
                    E -= va[k] @ einv[j] @ va[tp[k]]
            if not np.isfinite(E).all():
                nonfinite.append(int(i))
            einv[i], fb = dilu_block_inverse(E, D, tau, dt)
            if fb:
                fell.append(int(i))
    return einv, sorted(fell), sorted(nonfinite)


def ref_dilu_solve(case, einv, r, x, relax, dt=np.float64, sweeps=1,
                   smooth=False):
    """x += relax M^-1 r (smooth: r = rhs - A x first, rhs given as r),
    `sweeps` times; M = (E + L) E^-1 (E + U) in colour order. Returns x."""
    va, einv = case.va.astype(dt), np.asarray(einv).astype(dt)
    n, b = case.n_rows, case.b
    xb = _arr(x).astype(dt).reshape(-1, b)
    rhs = _arr(r).astype(dt).reshape(-1, b)
    order = color_order(case)
    for _ in range(sweeps):
        res = rhs
        if smooth:
            res = np.array([rhs[i] - _row_product(case, va, i, xb)
                            for i in range(n)])
        w = np.zeros((n, b), dtype=dt)
        done = np.zeros(n, dtype=bool)
        for c in range(int(case.colors.max()) + 1):
            rows = order[case.colors[order] == c]
            for i in rows:
                w[i] = einv[i] @ (res[i] - _row_product(case, va, i, w, True,
                                                        done))
            done[rows] = True
        z = np.zeros((n, b), dtype=dt)
        done[:] = False
        for c in range(int(case.colors.max()), -1, -1):
            rows = order[case.colors[order] == c]
            for i in rows:
                z[i] = w[i] - einv[i] @ _row_product(case, va, i, z, True,
                                                     done)
            done[rows] = True
        xb[:n] += dt(relax) * z
    return xb.reshape(-1)


def ref_ilu0_setup(case, dt=np.float64):
    """(lu (nnz, b, b), dinv (n, b, b)) of block ILU(0) in colour order:
    L_ik = A_ik U_kk^-1, A_ij -= L_ik U_kj on the stored local pattern."""
    b = case.b
    lu = case.va.astype(dt).copy()
    dp = diag_pos(case)
    order = color_order(case)
    pos = np.empty(case.n_rows, dtype=np.int64)
    pos[order] = np.arange(case.n_rows)
    dinv = np.zeros((case.n_rows, b, b), dtype=dt)
    for i in order:
        mine = {int(case.ci[k]): k
                for k in range(case.ro[i], case.ro[i + 1])}
        for pk, kidx in sorted((pos[j], k) for j, k in mine.items()
                               if j < case.n_rows and pos[j] < pos[i]):
            p = int(case.ci[kidx])
            lu[kidx] = lu[kidx] @ dinv[p]
            for k2 in range(case.ro[p], case.ro[p + 1]):
                j = int(case.ci[k2])
                if j < case.n_rows and pos[j] > pk and j in mine:
                    lu[mine[j]] -= lu[kidx] @ lu[k2]
        dinv[i] = gauss_jordan_inv(lu[dp[i]], dt)[0] if dp[i] >= 0 \
            else np.eye(b, dtype=dt)
    return lu, dinv


def ref_ilu0_solve(case, lu, dinv, r, x, relax, dt=np.float64):
    lu, dinv = np.asarray(lu).astype(dt), np.asarray(dinv).astype(dt)
    n, b = case.n_rows, case.b
    xb = _arr(x).astype(dt).reshape(-1, b)
    rb = _arr(r).astype(dt).reshape(-1, b)
    order = color_order(case)
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n)
    y = np.zeros((n, b), dtype=dt)
    z = np.zeros((n, b), dtype=dt)
    for i in order:
        y[i] = rb[i] - _row_product(case, lu, i, y, True, pos < pos[i])
    for i in order[::-1]:
        z[i] = dinv[i] @ (y[i] - _row_product(case, lu, i, z, True,
                                              pos > pos[i]))
    xb[:n] += dt(relax) * z
    return xb.reshape(-1)


# -------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def block_case(b, dtype, halo=False, fallback=False, kind="dominant"):
    return bi.colored_block_matrix(b, dtype, seed=3, kind=kind, halo=halo,
                                   fallback=fallback)


@functools.lru_cache(maxsize=None)
def vectors(b, n_cols, dtype):
    """(rhs, x0) of n_cols * b entries in [-1, 1], fixed per size."""
    rng = np.random.RandomState(100 + b)
    mk = lambda: torch.from_numpy(rng.uniform(-1, 1, n_cols * b)).to(dtype)
    return mk(), mk()


# ------------------------------------------------------ features are present
@pytest.mark.parametrize("halo", [False, True])
def test_constructed_features_exist(halo):
    c = block_case(4, torch.float64, halo)
    sp = c.special
    assert c.n_rows == 126 and bi.coloring_is_valid(c)
    assert sorted(np.bincount(c.colors)) == sorted(bi.COLOR_SIZES)
    assert sorted(np.bincount(c.colors)) == [1, 3, 4, 5, 15, 16, 17, 65]
    # the rows of a colour are scattered: rows_sorted is a real permutation
    assert (np.diff(c.coloring.rows_sorted.numpy()) < 0).any()
    assert bi.empty_rows(c) == [sp.empty]
    assert bi.missing_diag_rows(c) == sorted([sp.nodiag_first,
                                              sp.nodiag_notrans])
    assert c.colors[sp.nodiag_first] == 0 and c.colors[sp.nodiag_notrans] > 0
    assert bi.diag_only_rows(c) == [sp.diag_only]
    assert bi.long_rows(c) == [sp.long]
    width = c.ro[sp.long + 1] - c.ro[sp.long]
    assert width >= 38 and (halo or width == 38)   # 9 MFMA chunks and more
    for i, w in ((sp.diag_only, 1), (sp.singular_E[0], 2),
                 (sp.singular_D, 3), (sp.four, 4), (sp.five, 5),
                 (sp.eight, 8)):
        assert i in bi.rows_of_width(c, w, with_diag=True)
    miss = len(bi.missing_transpose_entries(c))
    assert 0.15 < miss / len(bi.local_offdiag_entries(c)) < 0.35
    tp = trans_pos(c)
    for k in range(c.ro[sp.nodiag_notrans], c.ro[sp.nodiag_notrans + 1]):
        assert tp[k] < 0
    assert len(bi.zero_blocks(c)) == 1
    assert len(bi.negative_diag_rows(c)) > 100
    for i in range(c.n_rows):            # ascending columns in every row
        assert (np.diff(c.ci[c.ro[i]:c.ro[i + 1]]) > 0).all()
    if halo:
        assert c.n_cols == c.n_rows + bi.N_HALO
        assert len(bi.halo_rows(c)) >= 20 and sp.long in bi.halo_rows(c)
        assert set(c.ci[c.ci >= c.n_rows]) == set(range(126, 135))
    else:
        assert c.n_cols == c.n_rows and not bi.halo_rows(c)
    # later rows really have earlier-colour neighbours with transposes, in
    # rows longer than two 4-entry chunks too
    used = [sum(1 for k in range(c.ro[i], c.ro[i + 1])
                if c.ci[k] != i and c.ci[k] < c.n_rows and tp[k] >= 0
                and c.colors[c.ci[k]] < c.colors[i])
            for i in range(c.n_rows)]
    assert used[sp.long] > 8 and sum(u > 0 for u in used) > 60


def test_same_structure_for_every_block_size_and_variant():
    a, b_ = block_case(2, torch.float64), block_case(9, torch.float32)
    assert (a.ci == b_.ci).all() and (a.colors == b_.colors).all()
    f = block_case(3, torch.float64, False, True)
    assert (a.ci == f.ci).all()


# ------------------------------------------------------------- exact inputs
@pytest.mark.parametrize("b", (2, 4, 8, 16, 17))
def test_exact_block_inputs_are_exact(b):
    c = block_case(b, torch.float32, True, False, "exact")
    x = bi.exact_vector(c.n_cols * b, torch.float32, 1).numpy()
    y = bi.exact_vector(c.n_rows * b, torch.float32, 2).numpy()
    bv = bi.exact_vector(c.n_rows * b, torch.float32, 3).numpy()
    for alpha, beta, gamma in ((1.0, 0.0, 0.0), (2.0, -0.5, 2.0),
                               (-0.5, 1.0, 2.0)):
        assert bi.prove_exact(c.ro, c.ci, c.va, x, y, bv, alpha, beta,
                              gamma) <= 24
    # the proof is no tautology: it fails on a format of fewer bits and on
    # an inexact datum
    with pytest.raises(AssertionError):
        bi.prove_exact(c.ro, c.ci, c.va, x, y, bv, 2.0, -0.5, 2.0, bits=8)
    with pytest.raises(AssertionError):
        bi.prove_exact(c.ro, c.ci, c.va, x * (1.0 / 3.0))


SCALAR_CASES = {
    # name: (rows, nnz): average degree exactly 16, just above, 64, above 64
    "deg16": (400, 6400), "deg16+": (400, 6401),
    "deg64": (400, 25600), "deg64+": (400, 25601),
}


@functools.lru_cache(maxsize=None)
def scalar_case(name, dtype):
    if name == "wide":                      # 37 x 300
        w = np.array([0, 1, 7, 8, 9, 31, 32, 33, 200, 300] * 3
                     + [16] * 7)
        return bi.scalar_matrix(w, 300, dtype, seed=5)
    if name == "tall":                      # 300 x 37
        w = np.random.RandomState(6).randint(0, 38, 300)
        w[:6] = (0, 1, 36, 37, 8, 9)
        return bi.scalar_matrix(w, 37, dtype, seed=6)
    rows, nnz = SCALAR_CASES[name]
    return bi.scalar_matrix(bi.scalar_routing_widths(rows, nnz), rows, dtype,
                            seed=rows + nnz)


@pytest.mark.parametrize("name", list(SCALAR_CASES) + ["wide", "tall"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.complex64])
def test_exact_scalar_inputs_are_exact(name, dtype):
    A, ro, ci, va = scalar_case(name, dtype)
    if name in SCALAR_CASES:
        rows, nnz = SCALAR_CASES[name]
        assert A.n_rows == rows and A.nnz == nnz
        widths = np.diff(ro)
        for w in bi.ROUTING_WIDTHS:
            assert (widths == w).any()
    else:
        assert (A.n_rows, A.n_cols) == ((37, 300) if name == "wide"
                                        else (300, 37))
    x = bi.exact_vector(A.n_cols, dtype, 1).numpy()
    y = bi.exact_vector(A.n_rows, dtype, 2).numpy()
    bv = bi.exact_vector(A.n_rows, dtype, 3).numpy()
    assert bi.prove_exact(ro, ci, va.reshape(-1, 1, 1), x, y, bv, 2.0, -0.5,
                          2.0) <= 24


def test_average_degrees_sit_on_the_routing_edges():
    for name, (rows, nnz) in SCALAR_CASES.items():
        A = scalar_case(name, torch.float64)[0]
        avg = A.nnz / A.n_rows
        assert (avg == 16.0, 16.0 < avg < 16.01, avg == 64.0,
                64.0 < avg < 64.01)[list(SCALAR_CASES).index(name)]


# ------------------------------------------------- host SpMV against the loops
@pytest.mark.parametrize("b", BLOCK_SIZES + (17,))
def test_host_block_spmv(b):
    c = block_case(b, torch.float64, True, False, "exact")
    x = bi.exact_vector(c.n_cols * b, torch.float64, 1)
    y = bi.exact_vector(c.n_rows * b, torch.float64, 2)
    for alpha, beta, (r0, r1) in ((1.0, 0.0, (0, 126)), (2.0, -0.5, (1, 125)),
                                  (-0.5, 1.0, (5, 6))):
        ref = ref_spmv(c.ro, c.ci, c.va, x.numpy(), y.numpy(), alpha, beta,
                       r0=r0, r1=r1)
        got = cpu_ops.spmv(c.A, x, y.clone(), alpha, beta, r0, r1)
        assert np.array_equal(got.numpy(), ref)


@pytest.mark.parametrize("name", list(SCALAR_CASES) + ["wide", "tall"])
def test_host_scalar_spmv(name):
    A, ro, ci, va = scalar_case(name, torch.float64)
    x = bi.exact_vector(A.n_cols, torch.float64, 1)
    y = bi.exact_vector(A.n_rows, torch.float64, 2)
    ref = ref_spmv(ro, ci, va.reshape(-1, 1, 1), x.numpy(), y.numpy(), 2.0,
                   -0.5, r0=1, r1=A.n_rows - 1)
    got = cpu_ops.spmv(A, x, y.clone(), 2.0, -0.5, 1, A.n_rows - 1)
    assert np.array_equal(got.numpy(), ref)


# ---------------------------------------------- host smoothers against the loops
def _check(got, ref, d32, rows=None):
    err = rel_err(got, ref, rows)
    limit = bound(d32, torch.float64)
    assert limit < 1e-9, "inputs too ill-conditioned for the float64 bound"
    assert err <= limit, (err, limit, d32)


@pytest.mark.parametrize("halo", [False, True])
@pytest.mark.parametrize("b", BLOCK_SIZES)
def test_host_jacobi(b, halo):
    c = block_case(b, torch.float64, halo)
    rhs, x0 = vectors(b, c.n_cols, torch.float64)
    for l1 in (False, True):
        ref, d32 = rounding_scale(lambda dt: ref_jacobi_dinv(c, l1, dt))
        dinv = cpu_ops.jacobi_dinv(c.A, l1)
        _check(dinv.numpy(), ref, d32)
    # rows without a diagonal block and the empty row: plain dinv = identity
    for i in bi.missing_diag_rows(c) + bi.empty_rows(c):
        assert np.array_equal(cpu_ops.jacobi_dinv(c.A)[i].numpy(), np.eye(b))
    dinv = ref_jacobi_dinv(c, False)
    ref, d32 = rounding_scale(
        lambda dt: ref_jacobi_smooth(c, dinv, rhs, x0, OMEGA, dt))
    out = torch.zeros_like(x0)
    cpu_ops.jacobi_smooth(c.A, torch.from_numpy(dinv), rhs, x0, out, OMEGA)
    _check(out.numpy()[:c.n_rows * b], ref, d32)


def test_l1_sign_follows_the_diagonal_entry():
    """A 2 x 2 block row by hand: D = diag(3, -3), off-diagonal l1 norms
    (2, 5): the l1 diagonal is diag(5, -8), not diag(5, 2)."""
    va = np.array([[[3.0, 0.0], [0.0, -3.0]], [[1.0, -1.0], [2.0, 3.0]]])
    A = CSRMatrix.from_bsr([0, 2, 2], [0, 1], va, n_cols=2)
    dinv = cpu_ops.jacobi_dinv(A, l1=True).numpy()
    assert np.allclose(dinv[0], np.diag([1 / 5.0, -1 / 8.0]), rtol=1e-15)
    # the scalar host path too, a zero diagonal counting as positive
    S = CSRMatrix.from_bsr([0, 2, 4, 5], [0, 1, 0, 1, 0],
                           np.array([-3.0, 2.0, 4.0, 0.0, 2.0]).reshape(
                               -1, 1, 1), n_cols=3)
    S = CSRMatrix(S.row_offsets, S.col_indices, S.values.reshape(-1),
                  n_cols=3)
    assert np.allclose(cpu_ops.jacobi_dinv(S, l1=True).numpy(),
                       [-1 / 5.0, 1 / 4.0, 1 / 2.0], rtol=1e-15)


@pytest.mark.parametrize("halo", [False, True])
@pytest.mark.parametrize("b", BLOCK_SIZES)
def test_host_gs(b, halo):
    c = block_case(b, torch.float64, halo)
    rhs, x0 = vectors(b, c.n_cols, torch.float64)
    dinv = ref_jacobi_dinv(c, False)
    for symmetric in (False, True):
        ref, d32 = rounding_scale(lambda dt: ref_gs_sweep(
            c, dinv, rhs, x0, OMEGA, symmetric, dt))
        x = x0.clone()
        cpu_ops.gs_sweep(c.A, torch.from_numpy(dinv), rhs, x, c.coloring,
                         OMEGA, symmetric)
        _check(x.numpy(), ref, d32)


@pytest.mark.parametrize("halo", [False, True])
@pytest.mark.parametrize("b", BLOCK_SIZES)
def test_host_dilu(b, halo):
    c = block_case(b, torch.float64, halo)
    rhs, x0 = vectors(b, c.n_cols, torch.float64)
    tau = pivot_floor(torch.float64)
    ref, d32 = rounding_scale(lambda dt: ref_dilu_setup(c, tau, dt)[0])
    einv64, fell, nonfinite = ref_dilu_setup(c, tau)
    # only the rows without a diagonal block fall back: their E_i is 0
    assert fell == sorted(bi.missing_diag_rows(c) + bi.empty_rows(c)) \
        and not nonfinite
    einv = cpu_ops.dilu_setup(c.A, c.coloring)
    _check(einv.numpy(), ref, d32)
    for sweeps in (1, 2):
        ref, d32 = rounding_scale(lambda dt: ref_dilu_solve(
            c, einv64, rhs, x0, 0.9, dt, sweeps))
        x = x0.clone()
        for _ in range(sweeps):
            cpu_ops.dilu_solve(c.A, torch.from_numpy(einv64), c.coloring,
                               rhs, 0.9, x)
        _check(x.numpy(), ref, d32)
    # the fused smoothing step is residual + solve
    ref, d32 = rounding_scale(lambda dt: ref_dilu_solve(
        c, einv64, rhs, x0, 0.9, dt, 1, True))
    x = x0.clone()
    cpu_ops.dilu_solve(c.A, torch.from_numpy(einv64), c.coloring,
                       cpu_ops.residual(c.A, x, rhs), 0.9, x)
    _check(x.numpy(), ref, d32)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("b", BLOCK_SIZES)
def test_host_dilu_fallback_cases(b, dtype):
    """Each side of the fallback rule, far from its thresholds: E exactly
    singular, E not finite, a singular fallback target, missing diagonal
    blocks, and every other row clearly regular."""
    c = block_case(b, dtype, False, True)
    sp = c.special
    tau = pivot_floor(dtype)
    ref, fell, nonfinite = ref_dilu_setup(c, tau)
    p, i_nf = sp.nonfinite_E
    expected = sorted([sp.singular_E[1], p, i_nf, sp.singular_D,
                       sp.nodiag_first, sp.nodiag_notrans, sp.empty])
    assert fell == expected
    assert nonfinite == sorted([p, i_nf])
    assert not np.isfinite(ref[p]).all()
    # far from the thresholds: the smallest pivot of every kept E_i is above
    # 1e3 tau dmax, every rejected one is 0 or NaN
    dp, tp = diag_pos(c), trans_pos(c)
    for i in range(c.n_rows):
        if i in fell:
            continue
        E = c.va[dp[i]].copy()
        for k in range(c.ro[i], c.ro[i + 1]):
            j = c.ci[k]
            if j != i and tp[k] >= 0 and c.colors[j] < c.colors[i]:
                E -= c.va[k] @ ref[j] @ c.va[tp[k]]
        dmax = np.abs(c.va[dp[i]]).max()
        assert gauss_jordan_inv(E)[1] > 1e3 * tau * dmax
        assert np.abs(E).max() < 1e-3 * 1e10 * (dmax + 1)
    # the singular rows take the inverse of D_i; the singular D_q its
    # patched Gauss-Jordan inverse; rows without a diagonal the identity
    s1 = sp.singular_E[1]
    assert np.allclose(ref[s1] @ c.va[dp[s1]], np.eye(b), atol=1e-14)
    S = np.eye(b)
    S[:2, :2] = [[1.0, 2.0], [2.0, 4.0]]
    patched, pmin = gauss_jordan_inv(S)
    assert pmin == 0.0 and np.array_equal(ref[sp.singular_D], patched)
    for i in (sp.nodiag_first, sp.nodiag_notrans, sp.empty):
        assert np.array_equal(ref[i], np.eye(b))
    assert np.array_equal(ref[i_nf], gauss_jordan_inv(c.va[dp[i_nf]])[0])
    einv = cpu_ops.dilu_setup(c.A, c.coloring).numpy().astype(np.float64)
    ref_r, d32 = rounding_scale(lambda dt: ref_dilu_setup(c, tau, dt)[0])
    rows = [i for i in range(c.n_rows) if i != p]
    if dtype == torch.float64:
        _check(einv, ref_r, d32, rows)
    else:       # the host computes in float64 and rounds the result once
        assert rel_err(einv, ref_r, rows) <= bound(d32, torch.float32)
    # the singular-block rule on the Jacobi side, same blocks
    dinv = cpu_ops.jacobi_dinv(c.A).numpy()
    assert np.array_equal(dinv[sp.singular_D], patched.astype(dinv.dtype))


@pytest.mark.parametrize("halo", [False, True])
@pytest.mark.parametrize("b", (3, 4, 8, 9, 16))
def test_host_ilu0(b, halo):
    c = block_case(b, torch.float64, halo)
    rhs, x0 = vectors(b, c.n_cols, torch.float64)
    ref, d32 = rounding_scale(lambda dt: ref_ilu0_setup(c, dt)[0])
    lu64, dinv64 = ref_ilu0_setup(c)
    local = c.ci < c.n_rows       # halo entries take no part in the factor
    lu = cpu_ops.ilu0_setup(c.A, c.coloring).numpy()
    assert rel_err(lu[local], ref[local]) <= bound(d32, torch.float64)
    ref, d32 = rounding_scale(lambda dt: ref_ilu0_solve(
        c, lu64, dinv64, rhs, x0, 0.9, dt))
    x = x0.clone()
    cpu_ops.ilu0_solve(c.A, torch.from_numpy(lu64), c.coloring, rhs, x, 0.9)
    _check(x.numpy(), ref, d32)


# ------------------------------------------------------------- whole solves
FGMRES_BLOCK_DILU = {
    "config_version": 2,
    "solver": {"solver": "FGMRES", "max_iters": 100, "tolerance": 1e-8,
               "convergence": "RELATIVE_INI", "norm": "L2",
               "gmres_n_restart": 100, "monitor_residual": 1,
               "preconditioner": {"solver": "MULTICOLOR_DILU",
                                  "max_iters": 1, "scope": "precond"}}}


def fgmres_block_dilu(case, device):
    """Iterations of FGMRES + block DILU on the case's system under the
    case's own colouring, on `device`."""
    from amgx_amd.resources import Resources
    A = case.A.to(device)
    A.coloring = type(case.coloring)(case.coloring.colors.to(device),
                                     case.coloring.num_colors)
    s = create_solver(AMGConfig.from_dict(FGMRES_BLOCK_DILU).root_scope(),
                      resources=Resources(device))
    # a consistent right-hand side: the matrix has an empty row
    x_true = vectors(case.b, case.n_cols, torch.float64)[1].numpy()
    rhs = torch.from_numpy(ref_spmv(case.ro, case.ci, case.va, x_true,
                                    np.zeros_like(x_true))).to(device)
    x = torch.zeros_like(rhs)
    s.setup(A)
    st = s.solve(rhs, x, zero_initial_guess=True)
    res = ref_spmv(case.ro, case.ci, case.va, x.cpu().numpy(),
                   rhs.cpu().numpy(), -1.0, 1.0)
    rel = np.linalg.norm(res) / np.linalg.norm(rhs.cpu().numpy())
    return st, rel


@pytest.mark.parametrize("b", (8, 9))
def test_host_fgmres_block_dilu(b):
    st, rel = fgmres_block_dilu(block_case(b, torch.float64), "cpu")
    assert st.converged and rel < 1e-7 and st.iterations <= 60
