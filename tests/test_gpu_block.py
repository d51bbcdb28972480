"""Device block-CSR kernels and the SpMV family against the dense loops of
tests/test_block_ref.py on the inputs of tests/block_inputs.py.

SpMV comparisons are bitwise: prove_exact (run by the host tests) shows that
every product of the "exact" inputs is exact in float32 in any order of
summation, so a lane dropped or counted twice cannot hide in a tolerance.
Everything with an inverse in it is held to the bounds derived from the
reference alone (test_block_ref.rounding_scale / bound): 8 * d32 for
float32 arithmetic, 8 * d32 * 2^-29 for float64 arithmetic. A factor (dinv,
Einv, LU) is stored in the matrix type and computed in it, so a setup is
bounded by the matrix type; an apply is handed the factor the device
computed, on both sides, and is bounded by the vector type."""

import numpy as np
import pytest
import torch

from amgx_amd import ops
from amgx_amd.amg.coloring import MatrixColoring
from tests import block_inputs as bi
from tests.test_block_ref import (OMEGA, SCALAR_CASES, block_case, bound,
                                  fgmres_block_dilu, gauss_jordan_inv,
                                  pivot_floor, ref_dilu_setup, ref_dilu_solve,
                                  ref_gs_sweep, ref_ilu0_setup,
                                  ref_ilu0_solve, ref_jacobi_dinv,
                                  ref_jacobi_smooth, ref_spmv, rel_err,
                                  rounding_scale, scalar_case, vectors)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64, C64, C128 = (torch.float32, torch.float64, torch.complex64,
                       torch.complex128)
REAL_PAIRS = [(F64, F64), (F32, F32), (F32, F64)]
CPLX_PAIRS = [(C128, C128), (C64, C64), (C64, C128)]
SMOOTHER_SIZES = (2, 3, 4, 5, 8, 9)
# (alpha, beta): beta == 0 runs over a y filled with NaN inside the window
COEFS = ((2.0, 0.0), (1.0, 1.0), (-0.5, -0.5))


def _pair_id(p):
    return "-".join(str(t).replace("torch.", "") for t in p)


def _windows(n):
    return ((0, n), (1, n - 1), (5, 6), (3, 3))


def _gpu_coloring(case):
    return MatrixColoring(case.coloring.colors.to(DEV),
                          case.coloring.num_colors)


def _check_spmv(A, ro, ci, va, tv, through_core=False):
    """Every window and coefficient pair of one matrix against the exact
    product, bitwise; rows outside the window keep their bits."""
    b = A.block_dim
    n = A.n_rows
    Ag = A.to(DEV)
    x = bi.exact_vector(A.n_cols * b, tv, 1)
    y0 = bi.exact_vector(n * b, tv, 2)
    bv = bi.exact_vector(n * b, tv, 3)
    zero = np.zeros(n * b)
    P = ref_spmv(ro, ci, va, x.numpy(), zero)        # A x, exact, once
    xg, bvg = x.to(DEV), bv.to(DEV)
    for r0, r1 in _windows(n):
        lo, hi = r0 * b, r1 * b
        for alpha, beta in COEFS:
            for gamma in ((None,) if not through_core else (0.0, 2.0)):
                y = y0.clone()
                if beta == 0.0:
                    y[lo:hi] = float("nan")
                ref = y0.numpy().astype(P.dtype)
                ref[lo:hi] = alpha * P[lo:hi] + beta * ref[lo:hi] \
                    + (gamma or 0.0) * bv.numpy()[lo:hi]
                ref = torch.from_numpy(ref).to(tv)
                yg = y.to(DEV)
                if through_core:
                    from amgx_amd import _core
                    _core.csrmv(Ag.row_offsets, Ag.col_indices, Ag.values, b,
                                xg, yg, bvg, alpha, beta, gamma, r0, r1)
                else:
                    ops.spmv(Ag, xg, yg, alpha, beta, r0, r1)
                got = yg.cpu()
                what = (r0, r1, alpha, beta, gamma)
                assert torch.equal(got, ref), what
                for s in (slice(0, lo), slice(hi, n * b)):
                    assert got[s].numpy().tobytes() == \
                        y0[s].numpy().tobytes(), what


# ------------------------------------------------------------- scalar SpMV
@pytest.mark.parametrize("pair", REAL_PAIRS + CPLX_PAIRS, ids=_pair_id)
@pytest.mark.parametrize("name", list(SCALAR_CASES) + ["wide", "tall"])
def test_scalar_spmv_exact(name, pair):
    """csrmv_tpr at average degree 16, csrmv_vec<8> just above 16 and at 64,
    csrmv_vec<32> just above 64, each on rows of 0, 1, 7, 8, 9, 31, 32, 33
    and 200 entries; a 37 x 300 and a 300 x 37 operator."""
    A, ro, ci, va = scalar_case(name, pair[0])
    _check_spmv(A, ro, ci, va.reshape(-1, 1, 1), pair[1])


@pytest.mark.parametrize("pair", [(F64, F64), (F32, F64), (C64, C128)],
                         ids=_pair_id)
@pytest.mark.parametrize("name", list(SCALAR_CASES) + ["wide"])
def test_scalar_spmv_bvec_gamma(name, pair):
    A, ro, ci, va = scalar_case(name, pair[0])
    _check_spmv(A, ro, ci, va.reshape(-1, 1, 1), pair[1], through_core=True)


# -------------------------------------------------------------- block SpMV
@pytest.mark.parametrize("pair", REAL_PAIRS, ids=_pair_id)
@pytest.mark.parametrize("b", (2, 3, 4, 5, 6, 7, 8, 9, 10, 16, 17))
def test_block_spmv_exact(b, pair):
    """bsrmv_b4, every bsrmv_bn case and bsrmv_generic (b >= 9; 17 is past
    the limit of the smoother kernels and must still work here), on the
    matrix with halo columns."""
    c = block_case(b, pair[0], True, False, "exact")
    _check_spmv(c.A, c.ro, c.ci, c.va, pair[1])


@pytest.mark.parametrize("b", (4, 5, 9))
def test_block_spmv_bvec_gamma(b):
    c = block_case(b, F32, True, False, "exact")
    _check_spmv(c.A, c.ro, c.ci, c.va, F64, through_core=True)


@pytest.mark.parametrize("pair", REAL_PAIRS, ids=_pair_id)
def test_bsrmv_generic_equals_mfma_path_at_b4(pair):
    from amgx_amd import _core
    c = block_case(4, pair[0], True, False, "exact")
    Ag = c.A.to(DEV)
    x = bi.exact_vector(c.n_cols * 4, pair[1], 1).to(DEV)
    y0 = bi.exact_vector(c.n_rows * 4, pair[1], 2).to(DEV)
    for alpha, beta in COEFS:
        ya, yb = y0.clone(), y0.clone()
        ops.spmv(Ag, x, ya, alpha, beta)
        _core.bsrmv_generic(Ag.row_offsets, Ag.col_indices,
                            Ag.values.reshape(-1), 4, x, yb, alpha, beta)
        assert torch.equal(ya, yb), (alpha, beta)


# ---------------------------------------------------------------- smoothers
def _within(got, ref, d32, dtype, rows=None):
    err, limit = rel_err(got.cpu().numpy(), ref, rows), bound(d32, dtype)
    print(f"d32 {d32:.3e} error {err:.3e} bound {limit:.3e}")
    assert dtype == F32 or limit < 1e-9
    assert err <= limit, (err, limit, d32)


smoother_cases = pytest.mark.parametrize(
    "halo", [False, True], ids=["plain", "halo"])
smoother_pairs = pytest.mark.parametrize("pair", REAL_PAIRS, ids=_pair_id)


@smoother_cases
@smoother_pairs
@pytest.mark.parametrize("b", SMOOTHER_SIZES)
def test_block_jacobi(b, pair, halo):
    ta, tv = pair
    c = block_case(b, ta, halo)
    Ag = c.A.to(DEV)
    rhs, x0 = vectors(b, c.n_cols, tv)
    for l1 in (True, False):
        ref, d32 = rounding_scale(lambda dt: ref_jacobi_dinv(c, l1, dt))
        dinv = ops.jacobi_dinv(Ag, l1)
        assert dinv.dtype == ta
        _within(dinv, ref, d32, ta)
    for i in bi.missing_diag_rows(c) + bi.empty_rows(c):
        assert torch.equal(dinv[i].cpu(), torch.eye(b, dtype=ta))
    factor = dinv.cpu().numpy().astype(np.float64)
    ref, d32 = rounding_scale(
        lambda dt: ref_jacobi_smooth(c, factor, rhs, x0, OMEGA, dt))
    out = torch.zeros(c.n_cols * b, dtype=tv, device=DEV)
    ops.jacobi_smooth(Ag, dinv, rhs.to(DEV), x0.to(DEV), out, OMEGA)
    _within(out[:c.n_rows * b], ref, d32, tv)


@smoother_cases
@smoother_pairs
@pytest.mark.parametrize("b", SMOOTHER_SIZES)
def test_block_gs(b, pair, halo):
    ta, tv = pair
    c = block_case(b, ta, halo)
    Ag, col = c.A.to(DEV), _gpu_coloring(c)
    rhs, x0 = vectors(b, c.n_cols, tv)
    dinv = ops.jacobi_dinv(Ag)
    factor = dinv.cpu().numpy().astype(np.float64)
    for symmetric in (False, True):
        ref, d32 = rounding_scale(lambda dt: ref_gs_sweep(
            c, factor, rhs, x0, OMEGA, symmetric, dt))
        x = x0.to(DEV)
        ops.gs_sweep(Ag, dinv, rhs.to(DEV), x, col, OMEGA, symmetric)
        _within(x, ref, d32, tv)


@smoother_cases
@smoother_pairs
@pytest.mark.parametrize("b", SMOOTHER_SIZES)
def test_block_dilu(b, pair, halo):
    ta, tv = pair
    c = block_case(b, ta, halo)
    Ag, col = c.A.to(DEV), _gpu_coloring(c)
    G = ops._backend(Ag)
    rhs, x0 = vectors(b, c.n_cols, tv)
    ref, d32 = rounding_scale(
        lambda dt: ref_dilu_setup(c, pivot_floor(ta), dt)[0])
    st = G.dilu_setup(Ag, col)
    assert st.einv.dtype == ta
    _within(st.einv, ref, d32, ta)
    factor = st.einv.cpu().numpy().astype(np.float64)
    for sweeps in (1, 2):
        ref, d32 = rounding_scale(lambda dt: ref_dilu_solve(
            c, factor, rhs, x0, 0.9, dt, sweeps))
        x = x0.to(DEV)
        G.dilu_solve(Ag, st, col, rhs.to(DEV), 0.9, x, sweeps=sweeps)
        _within(x, ref, d32, tv)
    # the fused smoothing step exists at b = 4 (MFMA) only; elsewhere the
    # wrapper says so instead of running something else
    x = x0.to(DEV)
    fused = G.dilu_smooth(Ag, st, col, rhs.to(DEV), x, 0.9)
    assert fused == (b == 4)
    if fused:
        ref, d32 = rounding_scale(lambda dt: ref_dilu_solve(
            c, factor, rhs, x0, 0.9, dt, 1, True))
        _within(x, ref, d32, tv)


@pytest.mark.parametrize("ta", [F64, F32], ids=["float64", "float32"])
@pytest.mark.parametrize("b", SMOOTHER_SIZES)
def test_block_dilu_setup_fallback_cases(b, ta):
    """Both sides of the fallback rule, far from its thresholds (asserted by
    the host tests): E_i exactly singular, E_i not finite, a singular
    fallback target, rows without a diagonal block, all other rows kept."""
    c = block_case(b, ta, False, True)
    sp = c.special
    tau = pivot_floor(ta)
    ref, d32 = rounding_scale(lambda dt: ref_dilu_setup(c, tau, dt)[0])
    einv = ops._backend(c.A.to(DEV)).dilu_setup(c.A.to(DEV),
                                                _gpu_coloring(c)).einv
    p, i_nf = sp.nonfinite_E
    # row p holds the inf itself: its own inverse is not finite and not
    # compared; every row after it is
    _within(einv, ref, d32, ta, [i for i in range(c.n_rows) if i != p])
    got = einv.cpu().numpy().astype(np.float64)
    S = np.eye(b)
    S[:2, :2] = [[1.0, 2.0], [2.0, 4.0]]
    assert np.array_equal(got[sp.singular_D], gauss_jordan_inv(S)[0])
    for i in (sp.nodiag_first, sp.nodiag_notrans, sp.empty):
        assert np.array_equal(got[i], np.eye(b))
    # E_s1 = S exactly: the inverse of D_s1 = S + I, not a patched S
    s1 = sp.singular_E[1]
    assert np.allclose(got[s1][:2, :2], np.array([[5.0, -2.0], [-2.0, 2.0]])
                       / 6.0, rtol=1e-6 if ta == F32 else 1e-14)
    assert np.isfinite(got[i_nf]).all()


@smoother_cases
@smoother_pairs
@pytest.mark.parametrize("b", (3, 4, 8, 9))
def test_block_ilu0(b, pair, halo):
    ta, tv = pair
    c = block_case(b, ta, halo)
    Ag, col = c.A.to(DEV), _gpu_coloring(c)
    rhs, x0 = vectors(b, c.n_cols, tv)
    local = c.ci < c.n_rows       # halo entries take no part in the factor
    for which in (0, 1):
        ref, d32 = rounding_scale(lambda dt: ref_ilu0_setup(c, dt)[which])
        if which == 0:
            lu, dinv = ops._backend(Ag).ilu0_setup(Ag, col)
            assert lu.dtype == ta and dinv.dtype == ta
            got = lu.reshape(-1, b, b)[torch.from_numpy(local).to(DEV)]
            _within(got, ref[local], d32, ta)
        else:
            _within(dinv.reshape(-1, b, b), ref, d32, ta)
    f_lu = lu.cpu().numpy().astype(np.float64).reshape(-1, b, b)
    f_dinv = dinv.cpu().numpy().astype(np.float64).reshape(-1, b, b)
    ref, d32 = rounding_scale(lambda dt: ref_ilu0_solve(
        c, f_lu, f_dinv, rhs, x0, 0.9, dt))
    x = x0.to(DEV)
    ops._backend(Ag).ilu0_solve(Ag, (lu, dinv), col, rhs.to(DEV), x, 0.9)
    _within(x, ref, d32, tv)


@pytest.mark.parametrize("b", (8, 9))
def test_fgmres_block_dilu_converges_as_on_the_host(b):
    c = block_case(b, F64)
    host, _ = fgmres_block_dilu(c, "cpu")
    st, rel = fgmres_block_dilu(c, DEV)
    assert host.converged and st.converged and rel < 1e-7
    assert st.iterations <= host.iterations


# --------------------------------------------------------- block-size guard
def test_block_dim_17_is_refused_by_the_smoother_entries():
    """The smoother kernels hold 16 components per thread; block_dim 17 is
    refused by every entry that would launch one, by the wrapper and by the
    binding, before anything runs. The block SpMV takes it
    (test_block_spmv_exact[17-*])."""
    from amgx_amd import _core
    b = 17
    c = block_case(b, F64, False, False, "exact")
    Ag, col = c.A.to(DEV), _gpu_coloring(c)
    G = ops._backend(Ag)
    v = torch.zeros(c.n_cols * b, dtype=F64, device=DEV)
    blocks = torch.zeros(c.n_rows, b, b, dtype=F64, device=DEV)
    state = G.DiluState(blocks, Ag.values.reshape(-1), blocks.reshape(-1))
    calls = {
        "jacobi_dinv": lambda: ops.jacobi_dinv(Ag),
        "gs_sweep": lambda: ops.gs_sweep(Ag, blocks, v, v.clone(), col, 1.0),
        "gs_smooth_color": lambda: G.gs_smooth_color(
            Ag, blocks, v, v.clone(), col.rows_of(0), 1.0),
        "dilu_setup": lambda: G.dilu_setup(Ag, col),
        "dilu_solve": lambda: G.dilu_solve(Ag, state, col, v, 1.0,
                                           v.clone()),
        "dilu_smooth": lambda: G.dilu_smooth(Ag, state, col, v, v.clone(),
                                             1.0),
        "ilu0_setup": lambda: ops._backend(Ag).ilu0_setup(Ag, col),
        "ilu0_solve": lambda: G.ilu0_solve(
            Ag, (Ag.values.reshape(-1), blocks.reshape(-1)), col, v,
            v.clone(), 1.0),
    }
    for name, call in calls.items():
        if name == "dilu_smooth":     # no fused kernel at this size: False,
            assert call() is False    # nothing launched
            continue
        with pytest.raises(ValueError, match="block_dim 17.*1\\.\\.16"):
            call()
    # the bindings refuse it on their own too
    ro, ci, va = Ag.row_offsets, Ag.col_indices, Ag.values
    idx = torch.zeros(c.n_rows, dtype=torch.int32, device=DEV)
    tix = torch.zeros(Ag.nnz, dtype=torch.int32, device=DEV)
    direct = {
        "jacobi_dinv": lambda: _core.jacobi_dinv(ro, ci, va, idx, c.n_rows, b,
                                                 False),
        "gs_smooth_rows": lambda: _core.gs_smooth_rows(
            ro, ci, va, b, blocks, v, v.clone(), col.rows_of(0), 1.0),
        "gs_sweep": lambda: _core.gs_sweep(
            ro, ci, va, b, blocks, v, v.clone(), col.rows_sorted, col.bounds,
            1.0, False),
        "dilu_setup": lambda: _core.dilu_setup(
            ro, ci, va, b, idx, tix, col.colors, col.rows_sorted,
            col.bounds),
        "dilu_sorted": lambda: _core.dilu_sorted(
            ro, ci, va.reshape(-1), b, blocks.reshape(-1), col.rows_sorted,
            col.bounds, col.bounds_dev, v, v.clone(), v.clone(), v.clone(),
            1.0, False, False),
        "ilu0_setup_block": lambda: _core.ilu0_setup_block(
            ro, ci, va.reshape(-1), b, idx, idx, col.rows_sorted,
            col.bounds),
        "ilu0_apply_block": lambda: _core.ilu0_apply_block(
            ro, ci, va.reshape(-1), blocks.reshape(-1), b, idx,
            col.rows_sorted, col.bounds, v, v.clone(), v.clone(), v.clone(),
            1.0),
    }
    for name, call in direct.items():
        with pytest.raises(RuntimeError, match="block_dim 17"):
            call()
