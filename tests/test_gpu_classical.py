"""Classical AMG setup on the device against the per-row float64 loops of
``tests/test_classical_ref.py``: AHAT strength, the transpose index, PMIS
(exact against the replayed algorithm, plus the PMIS properties), direct
interpolation with its count pass, truncation on tied values, and the D2 /
MULTIPASS formulations on the device SpGEMM against their host versions."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from amgx_amd.amg.classical import (SELECTOR_REGISTRY, _interp_d2_device,
                                    _interp_d2_host, _interp_multipass_device,
                                    interp_multipass)
from amgx_amd.config import ConfigScope
from amgx_amd.ops import cpu as cpu_ops
from tests.test_classical_ref import (D2_NAMES, SIGNED_NAMES, STRENGTH_PARAMS,
                                      TRUNC_PARAMS, ZOO_NAMES, assert_same_p,
                                      check_pmis_invariants, csr_matrix_to_p,
                                      d1_reference, emulate_pmis,
                                      ref_strength, ref_trans_index,
                                      ref_truncate, splits, tie_matrix, zoo)

DEV = "cuda:0"
DTYPES = pytest.mark.parametrize("dtype", [torch.float64, torch.float32],
                                 ids=["fp64", "fp32"])
# fp64: the project's convention for fp64 kernels. fp32: inputs and sums are
# exact, one division and the final cast round (fp32 epsilon is 6e-8).
TOL = {torch.float64: dict(rtol=1e-12, atol=1e-14),
       torch.float32: dict(rtol=1e-6, atol=0.0)}
_dev_cache = {}


def gpu_ops():
    from amgx_amd.ops import gpu
    return gpu


def on_device(name, dtype=torch.float64):
    key = (name, dtype)
    if key not in _dev_cache:
        m = tie_matrix() if name == "ties" else zoo(name)
        _dev_cache[key] = m.csr(dtype, DEV)
    return _dev_cache[key]


def u8(mask):
    return torch.from_numpy(np.asarray(mask).astype(np.uint8)).to(DEV)


def i32(a):
    return torch.from_numpy(np.asarray(a).astype(np.int32)).to(DEV)


# --------------------------------------------------------------------- strength
@pytest.mark.parametrize("theta,mrs", STRENGTH_PARAMS)
@DTYPES
@pytest.mark.parametrize("name", ZOO_NAMES)
def test_strength(name, dtype, theta, mrs):
    m = zoo(name)
    S = gpu_ops().strength_ahat(on_device(name, dtype), theta, mrs)
    assert S.dtype == torch.uint8 and S.numel() == m.ci.size
    assert np.array_equal(S.cpu().numpy().astype(bool),
                          ref_strength(m.ro, m.ci, m.va, theta, mrs))


# ------------------------------------------------------------------ trans_index
@pytest.mark.parametrize("name", ZOO_NAMES)
def test_trans_index(name):
    m = zoo(name)
    t = gpu_ops()._tidx(on_device(name))
    assert t.dtype == torch.int32
    assert np.array_equal(t.cpu().numpy(), ref_trans_index(m.ro, m.ci, m.n))


# ------------------------------------------------------------------------- PMIS
@pytest.mark.parametrize("name", ZOO_NAMES)
def test_pmis(name):
    """cf equal to the replayed algorithm (bitwise: every weight is exact in
    fp32). staircase140 needs 70 rounds, more than the 64 the device used to
    stop at; the signed matrices have strong (j, i) without a stored (i, j)."""
    m = zoo(name)
    S, cf_all, _ = splits(name)["pmis"]
    cf_ref = cf_all[:m.n]
    cf, nc = gpu_ops().pmis_select(on_device(name), u8(S))
    assert cf.dtype == torch.int32
    cf = cf.cpu().numpy()
    check_pmis_invariants(m.ro, m.ci, S, m.n, cf)
    assert nc == int((cf_ref >= 0).sum())
    assert np.array_equal(cf, cf_ref)


def test_pmis_raises_past_the_round_guard():
    from amgx_amd import _core
    m = zoo("staircase100")             # 50 rounds
    S = u8(splits("staircase100")["pmis"][0])
    A = on_device("staircase100")
    t = gpu_ops()._tidx(A)
    with pytest.raises(RuntimeError, match="PMIS failed to converge"):
        _core.pmis_select(A.row_offsets, A.col_indices, t, S, 49)
    state = _core.pmis_select(A.row_offsets, A.col_indices, t, S, 50)
    assert not bool((state == 0).any())
    assert m.n == state.numel()


# --------------------------------------------------------------------------- D1
@DTYPES
@pytest.mark.parametrize("split", ["pmis", "third"])
@pytest.mark.parametrize("name", ZOO_NAMES)
def test_interp_d1(name, split, dtype):
    """Weights against the loop, the lumping rows among them: a row whose
    diagonal is zero after lumping gets no weight, one whose zero diagonal
    lumping rescues gets the host's weights. On the halo matrix the column
    ids of halo columns come out of cf."""
    from amgx_amd import _core
    S, cf, nc, P_ref, counts, cls = d1_reference(name, split)
    if name in SIGNED_NAMES:
        assert cls["lumped_zero"] and cls["rescued"] and cls["missing_diag"]
    A = on_device(name, dtype)
    Sg, cfg = u8(S), i32(cf)
    cnt = _core.interp_d1_count(A.row_offsets, A.col_indices, Sg, cfg)
    assert np.array_equal(cnt.cpu().numpy(), counts)
    P = gpu_ops().interp_d1(A, Sg, cfg, nc)
    assert P.dtype == dtype and P.n_cols == nc
    assert np.array_equal(np.diff(P.row_offsets.cpu().numpy()), counts)
    assert bool(torch.isfinite(P.values).all())
    assert_same_p(csr_matrix_to_p(P), P_ref, **TOL[dtype])


# --------------------------------------------------------------------- truncate
@DTYPES
@pytest.mark.parametrize("factor,cap", TRUNC_PARAMS)
def test_truncate_rows_with_ties(factor, cap, dtype):
    m = tie_matrix()
    ro, ci, va = ref_truncate(m.ro, m.ci, m.va, factor, cap)
    T = gpu_ops().truncate_rows(on_device("ties", dtype), factor, cap)
    H = cpu_ops.truncate_rows(m.csr(dtype), factor, cap)
    assert T.dtype == dtype and T.n_cols == m.ncols
    for r, c, v in ((ro, ci, va),
                    (H.row_offsets.numpy(), H.col_indices.numpy(),
                     H.values.numpy().astype(np.float64))):
        assert np.array_equal(T.row_offsets.cpu().numpy(), r)
        assert np.array_equal(T.col_indices.cpu().numpy(), c)
        np.testing.assert_allclose(
            T.values.cpu().numpy().astype(np.float64), v, **TOL[dtype])


# ----------------------------------------------------------- D2 and MULTIPASS
SCOPE = ConfigScope(None, {"strength_threshold": 0.25})


def _max_abs_diff(P, Q):
    assert P.shape == Q.shape
    d = abs(P - Q)
    return d.max() if d.nnz else 0.0


@pytest.mark.parametrize("name", D2_NAMES)
def test_d2_on_device_matches_host(name):
    m = zoo(name)
    S = torch.from_numpy(ref_strength(m.ro, m.ci, m.va, 0.25, 1.1))
    cf, nc, _, _ = emulate_pmis(m.ro, m.ci, S.numpy(), m.n)
    cf = torch.from_numpy(cf)
    Ph = _interp_d2_host(m.csr(), S, cf, nc, SCOPE)
    Pd = _interp_d2_device(on_device(name), S, cf, nc, SCOPE)
    assert Pd.is_cuda and Ph.nnz > nc
    assert _max_abs_diff(Ph.to_scipy(), Pd.to_scipy()) < 1e-12


@pytest.mark.parametrize("name", D2_NAMES)
def test_multipass_on_device_matches_host(name):
    m = zoo(name)
    A = m.csr()
    S = torch.from_numpy(ref_strength(m.ro, m.ci, m.va, 0.25, 1.1))
    cf, nc = SELECTOR_REGISTRY["AGGRESSIVE_PMIS"](A, S, SCOPE)
    Ph = interp_multipass(A, S, cf, nc, SCOPE)
    Pd = _interp_multipass_device(on_device(name), S, cf, nc, SCOPE)
    assert Pd.is_cuda and Ph.nnz > nc
    assert _max_abs_diff(Ph.to_scipy(), Pd.to_scipy()) < 1e-12
