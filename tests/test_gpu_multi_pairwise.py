"""MULTI_PAIRWISE on the device against the host oracle of ``ops/cpu.py``:
weights bitwise, one matching pass exactly (aggregates, count, sizes and
round count), the pass driver in its host form against its device form, the
properties of ``tests/test_multi_pairwise.py`` where no exact yardstick
exists, and whole solves.

Exact comparisons past the first pass run on matrices whose ghost-level sums
are exact (docs/KERNELS.md, "MULTI_PAIRWISE", known limit)."""

import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from amgx_amd import AMGConfig, CSRMatrix, create_solver, ops
from amgx_amd.amg.aggregation import (multi_pairwise_passes,
                                      select_multi_pairwise)
from amgx_amd.problems import poisson_3d
from amgx_amd.resources import Resources
from tests.test_multi_pairwise import (GRAPHS, M777, MERGE, block_matrix,
                                       check_invariants, dyadic_matrix,
                                       matrix_graph, root_vector,
                                       run_matching, scope, signed_matrix,
                                       to_csr)

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev_graph(g):
    return SimpleNamespace(n=g.n, ro=g.ro.to(DEV), ci=g.ci.to(DEV),
                           w=g.w.to(DEV))


def assert_same_result(dev, host):
    assert dev[1] == host[1] and dev[3] == host[3], (dev[1:], host[1:])
    assert dev[0].dtype == torch.int32 and dev[2].dtype == torch.int32
    assert torch.equal(dev[0].cpu(), host[0])
    assert torch.equal(dev[2].cpu(), host[2])


# ====================================================================== weights
WEIGHT_CASES = [(torch.float64, 0), (torch.float64, 1), (torch.float32, 0),
                (torch.float32, 1), (torch.complex128, 0),
                (torch.complex64, 0)]   # formula 1 is real only


@pytest.mark.parametrize("dtype,formula", WEIGHT_CASES,
                         ids=["fp64-f0", "fp64-f1", "fp32-f0", "fp32-f1",
                              "c128-f0", "c64-f0"])
@pytest.mark.parametrize("n", [777, 63, 64, 65, 255, 256, 257])
def test_weights_bitwise(n, dtype, formula):
    m = M777 if n == 777 else signed_matrix(n, seed=n)
    ref = ops.pairwise_weights(to_csr(m, dtype), formula)
    got = ops.pairwise_weights(to_csr(m, dtype, DEV), formula)
    assert got.is_cuda and got.dtype == torch.float64
    assert torch.equal(got.cpu().view(torch.int64), ref.view(torch.int64))


def test_rejections():
    with pytest.raises(NotImplementedError):
        ops.pairwise_weights(to_csr(M777, torch.complex128, DEV), 1)
    Ab = block_matrix().to(DEV)
    with pytest.raises(NotImplementedError):
        ops.pairwise_weights(Ab, 1)
    with pytest.raises(NotImplementedError):
        select_multi_pairwise(to_csr(M777, torch.complex128, DEV),
                              scope(weight_formula=1))
    with pytest.raises(NotImplementedError):
        select_multi_pairwise(Ab, scope(weight_formula=1))


# ===================================================================== matching
_host_results = {}


def host_result(name, merge, cap, **kw):
    key = (name, merge, cap, tuple(sorted(kw.items())))
    if key not in _host_results:
        _host_results[key] = run_matching(GRAPHS[name][0], merge, cap, **kw)
    return _host_results[key]


@MERGE
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_matching_equals_oracle(name, merge):
    g, cap = GRAPHS[name]
    cap = cap if merge == 2 else 0
    dev = run_matching(dev_graph(g), merge, cap)
    assert_same_result(dev, host_result(name, merge, cap))


@MERGE
@pytest.mark.parametrize("kw,rounds", [(dict(max_iterations=15), 15),
                                       (dict(max_unassigned=0.5), 11),
                                       (dict(max_iterations=0), 0)],
                         ids=["iterations", "unassigned", "norounds"])
def test_matching_round_loop_exits(kw, rounds, merge):
    g, cap = GRAPHS["path"]
    cap = cap if merge == 2 else 0
    dev = run_matching(dev_graph(g), merge, cap, **kw)
    host = host_result("path", merge, cap, **kw)
    assert_same_result(dev, host)
    assert host[3] == rounds


@MERGE
@pytest.mark.parametrize("formula", [0, 1])
@pytest.mark.parametrize("kind", ["grid", "random"])
def test_matching_dyadic_with_sizes(kind, formula, merge):
    """Node sizes 1..4 and cap 6, as a later pass sees them."""
    g = matrix_graph(dyadic_matrix(kind), formula)
    sizes = torch.from_numpy(
        np.random.RandomState(2).randint(1, 5, size=g.n).astype(np.int32))
    host = run_matching(g, merge, 6, sizes=sizes, seed=5)
    dev = run_matching(dev_graph(g), merge, 6, sizes=sizes.to(DEV), seed=5)
    assert_same_result(dev, host)


@MERGE
def test_renumbering_equals_torch_unique(merge):
    g, cap = GRAPHS["poisson8"]
    cap = cap if merge == 2 else 0
    d = dev_graph(g)
    agg0 = run_matching(d, 0, cap)[0].cpu().numpy()
    agg, num, _, _ = run_matching(d, merge, cap)
    roots = torch.from_numpy(root_vector(agg0, agg.cpu().numpy())).to(DEV)
    uniq, inv = torch.unique(roots, sorted=True, return_inverse=True)
    assert num == uniq.numel() and torch.equal(inv.to(torch.int32), agg)


DEGREES = [1, 7, 8, 9, 63, 64, 65, 200]


def hub_graph():
    """Hub rows of the degrees that straddle multiples of the lane count, on
    shared leaves, with many tied weights, some aggregated rows and sizes
    that make the cap bind."""
    rng = np.random.RandomState(8)
    n_leaf = 260
    n = n_leaf + len(DEGREES)
    rows = [dict() for _ in range(n)]
    for h, deg in enumerate(DEGREES):
        for j in rng.choice(n_leaf, size=deg, replace=False):
            wt = float(rng.randint(1, 4)) / 8.0
            rows[n_leaf + h][int(j)] = wt
            rows[int(j)][n_leaf + h] = wt
    ro, ci, w = [0], [], []
    for i in range(n):
        for c in sorted(rows[i]):
            ci.append(c)
            w.append(rows[i][c])
        ro.append(len(ci))
    agg = np.where(rng.rand(n) < 0.3, 0, -1).astype(np.int32)
    agg[n_leaf:] = -1
    return SimpleNamespace(
        n=n, ro=torch.tensor(ro, dtype=torch.int32, device=DEV),
        ci=torch.tensor(ci, dtype=torch.int32, device=DEV),
        w=torch.tensor(w, dtype=torch.float64, device=DEV),
        agg=torch.from_numpy(agg).to(DEV),
        sizes=torch.from_numpy(rng.randint(1, 5, size=n).astype(np.int32))
        .to(DEV))


@pytest.mark.parametrize("cap", [0, 6])
@pytest.mark.parametrize("lanes", [8])
def test_lanes_per_row_propose_equals_thread_per_row(lanes, cap):
    from amgx_amd import _core
    g = hub_graph()
    args = (g.ro, g.ci, g.w, g.n, g.agg, g.sizes, cap, 3)
    ref = _core.pairwise_propose(*args, 1)
    got = _core.pairwise_propose(*args, lanes)
    assert torch.equal(got, ref)
    hubs = ref[-len(DEGREES):].cpu().numpy()
    assert (hubs < g.n - len(DEGREES)).sum() >= 6   # hubs do propose


@MERGE
def test_matching_same_for_every_lane_count(merge):
    from amgx_amd.ops import gpu
    g = dev_graph(matrix_graph(dyadic_matrix("grid")))
    sizes = torch.ones(g.n, dtype=torch.int32, device=DEV)
    res = [gpu.pairwise_matching(g.ro, g.ci, g.w, g.n, sizes, 5, merge, 100,
                                 0.0, 1, lanes=L) for L in (1, 8)]
    for r in res[1:]:
        assert_same_result([t.cpu() if torch.is_tensor(t) else t for t in r],
                           [t.cpu() if torch.is_tensor(t) else t
                            for t in res[0]])


# ======================================================================= driver
@pytest.mark.parametrize("formula", [0, 1])
@pytest.mark.parametrize("full_ghost", [0, 1])
@MERGE
@pytest.mark.parametrize("kind", ["grid", "random"])
def test_driver_host_form_equals_device_form(kind, merge, full_ghost, formula):
    A = dyadic_matrix(kind)
    sc = scope(aggregation_passes=3, merge_singletons=merge,
               full_ghost_level=full_ghost, weight_formula=formula)
    agg_h, num_h, lv_h = multi_pairwise_passes(A, sc, return_levels=True)
    agg_d, num_d, lv_d = multi_pairwise_passes(A.to(DEV), sc,
                                               return_levels=True)
    assert len(lv_h) == len(lv_d) == 3
    for h, d in zip(lv_h, lv_d):
        assert_same_result(d, h)
    assert num_d == num_h and torch.equal(agg_d.cpu(), agg_h)
    # the selector on a device matrix is this driver, not the greedy matcher
    agg_s, num_s = select_multi_pairwise(A.to(DEV), sc)
    assert agg_s.is_cuda and num_s == num_h and torch.equal(agg_s.cpu(), agg_h)
    if merge == 2:
        assert lv_d[-1][2].max() <= 10
    # serial_matching = 1 keeps the greedy matcher of the host
    sc_serial = scope(aggregation_passes=3, merge_singletons=merge,
                      serial_matching=1)
    g_d = select_multi_pairwise(A.to(DEV), sc_serial)
    g_h = select_multi_pairwise(A, sc_serial)
    assert g_d[1] == g_h[1] and torch.equal(g_d[0].cpu(), g_h[0].cpu())


def _pass_invariants(A, merge, passes=3):
    """Every pass of the device driver against check_invariants, on the
    graph that pass matched."""
    sc = scope(aggregation_passes=passes, merge_singletons=merge)
    cap = 2 ** passes + passes - passes // 2 if merge == 2 else 0
    agg, num, levels = multi_pairwise_passes(A, sc, return_levels=True)
    g = matrix_graph(A)
    sizes = torch.ones(g.n, dtype=torch.int32, device=DEV)
    for p, (level_agg, lnum, lsizes, rounds) in enumerate(levels):
        kw = dict(sizes=sizes, max_iterations=15, max_unassigned=0.05, seed=p)
        res0 = run_matching(g, 0, cap, **kw)
        again = run_matching(g, merge, cap, **kw)
        assert torch.equal(again[0], level_agg) and again[1] == lnum
        check_invariants(g, merge, cap, again, res0, sizes=sizes,
                         exhausted=False)
        assert lnum < g.n
        if p + 1 < len(levels):
            G = ops.galerkin_aggregation(
                CSRMatrix(g.ro, g.ci, g.w, n_cols=g.n), level_agg, lnum)
            g = SimpleNamespace(n=lnum, ro=G.row_offsets, ci=G.col_indices,
                                w=G.values)
            sizes = lsizes
    assert int(levels[-1][2].sum()) == A.n_rows
    return agg, num


@MERGE
def test_invariants_poisson16(merge):
    _pass_invariants(poisson_3d(16, 16, 16).to(DEV), merge)


@MERGE
def test_invariants_block4(merge):
    _pass_invariants(block_matrix().to(DEV), merge, passes=2)


def test_selector_is_deterministic():
    A = poisson_3d(16, 16, 16).to(DEV)
    sc = scope(aggregation_passes=3, merge_singletons=2)
    a1, n1 = select_multi_pairwise(A, sc)
    A2 = poisson_3d(16, 16, 16).to(DEV)
    a2, n2 = select_multi_pairwise(A2, sc)
    assert n1 == n2 and torch.equal(a1, a2)
    assert torch.bincount(a1.long()).max() <= 10


# =================================================================== end to end
def _solve(cfg_dict, A, vec_dtype):
    dev = str(A.device)
    cfg = AMGConfig.from_dict(cfg_dict)
    s = create_solver(cfg.root_scope(), resources=Resources(dev))
    b = torch.ones(A.n_rows, dtype=vec_dtype, device=A.device)
    x = torch.zeros_like(b)
    s.setup(A)
    st = s.solve(b, x, zero_initial_guess=True)
    rel = float(ops.nrm2(ops.residual(A, x, b)) / ops.nrm2(b))
    return st, rel


def _fgmres_mp(merge):
    return {"config_version": 2, "solver": {
        "solver": "FGMRES", "max_iters": 100, "gmres_n_restart": 20,
        "monitor_residual": 1, "convergence": "RELATIVE_INI",
        "tolerance": 1e-8,
        "preconditioner": {
            "solver": "AMG", "algorithm": "AGGREGATION",
            "selector": "MULTI_PAIRWISE", "aggregation_passes": 2,
            "merge_singletons": merge, "smoother": "MULTICOLOR_DILU",
            "presweeps": 1, "postsweeps": 1, "cycle": "V", "max_iters": 1,
            "min_coarse_rows": 32, "coarse_solver": "DENSE_LU_SOLVER"}}}


def _configs():
    with open(os.path.join(ROOT, "configs",
                           "AGGREGATION_MULTI_PAIRWISE.json")) as f:
        shipped = json.load(f)
    return {"shipped": shipped, "fgmres_merge1": _fgmres_mp(1),
            "fgmres_merge2": _fgmres_mp(2)}


_host_iters = {}


def host_iterations(name):
    """hDDI: the unchanged greedy matcher of the host, solved once."""
    if name not in _host_iters:
        st, rel = _solve(_configs()[name], poisson_3d(16, 16, 16),
                         torch.float64)
        assert st.converged and rel < 1e-6, (st, rel)
        _host_iters[name] = st.iterations
    return _host_iters[name]


@pytest.mark.parametrize("mode", ["dDDI", "dDFI"])
@pytest.mark.parametrize("name", ["shipped", "fgmres_merge1",
                                  "fgmres_merge2"])
def test_solve_poisson16(name, mode):
    """Handshaking is a somewhat weaker matching than the sequential greedy
    one: the device may take up to 1.5x the iterations of hDDI."""
    A = poisson_3d(16, 16, 16)
    if mode == "dDFI":
        A = CSRMatrix(A.row_offsets, A.col_indices,
                      A.values.to(torch.float32), n_cols=A.n_cols)
    st, rel = _solve(_configs()[name], A.to(DEV), torch.float64)
    host = host_iterations(name)
    print(f"{name} {mode}: device {st.iterations} iterations, "
          f"hDDI {host}, rel {rel:.2e}")
    assert st.converged and rel < 1e-5, (st, rel)
    assert st.iterations <= 1.5 * host, (st.iterations, host)


def test_solve_dZZI():
    P = poisson_3d(16, 16, 16)
    va = P.values.to(torch.complex128) * (0.6 + 0.8j)
    A = CSRMatrix(P.row_offsets, P.col_indices, va, n_cols=P.n_cols).to(DEV)
    cfg = _fgmres_mp(2)
    cfg["solver"]["preconditioner"]["weight_formula"] = 0
    st, rel = _solve(cfg, A, torch.complex128)
    print(f"dZZI: {st.iterations} iterations, rel {rel:.2e}")
    assert st.converged and rel < 1e-6, (st, rel)
