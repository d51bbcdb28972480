"""Aggregation-AMG selector registry (reference src/aggregation/selectors/:
size2/size4/size8, multi_pairwise, parallel_greedy, serial_greedy, geo,
dummy; registered src/core.cu:560-690).

Each selector returns (aggregates int32[n_rows], num_aggregates). SIZE_2 is
the gfx950-kernel handshaking matching (ops.size2_matching); SIZE_4/8
compose repeated pairwise passes like the reference. MULTI_PAIRWISE on a
device matrix is the capped handshake matching on a weight graph
(multi_pairwise_passes over ops.pairwise_weights / ops.pairwise_matching);
on a host matrix it is a sequential greedy matcher.
"""

from __future__ import annotations

from typing import Callable, Dict

import numpy as np
import torch

from .. import ops

AGG_SELECTOR_REGISTRY: Dict[str, Callable] = {}


def register_agg_selector(name: str):
    def deco(fn):
        AGG_SELECTOR_REGISTRY[name] = fn
        return fn
    return deco


def _compose_passes(A, scope, passes: int, matcher=None):
    """Repeated pairwise matching: pass k matches the level-k aggregates
    (reference size4 = 'two SIZE_2 passes').
    ``aggregation_passes`` (reference param) overrides the selector's pass
    count when set."""
    override = int(scope.get("aggregation_passes") or 0)
    if override > 0:
        passes = override
    maxit = scope.get("max_matching_iterations")
    match = matcher or (lambda M: ops.size2_matching(M, max_iterations=maxit))
    agg, num = match(A)            # composed fine->current map
    level_agg, work = agg, A       # map/matrix of the CURRENT level
    min_rows = scope.get("min_coarse_rows")
    for _ in range(passes - 1):
        if num <= min_rows:
            break
        work = ops.galerkin_aggregation(
            work, level_agg.to(work.row_offsets.device), num)
        level_agg, num = match(work)
        agg = level_agg.to(agg.device)[agg.long()]
    return agg, num


@register_agg_selector("SIZE_2")
def select_size2(A, scope):
    return _compose_passes(A, scope, 1)


@register_agg_selector("SIZE_4")
def select_size4(A, scope):
    return _compose_passes(A, scope, 2)


@register_agg_selector("SIZE_8")
def select_size8(A, scope):
    return _compose_passes(A, scope, 3)


@register_agg_selector("PARALLEL_GREEDY")
@register_agg_selector("PARALLEL_GREEDY_SELECTOR")
def select_parallel_greedy(A, scope):
    """Handshaking matching run to exhaustion (reference
    parallel_greedy_selector.cu behaves like an aggressive pairwise pass)."""
    return _compose_passes(A, scope, 1)


def _multi_pairwise_pass_count(scope) -> int:
    override = int(scope.get("aggregation_passes") or 0)
    if override > 0:
        return override
    size = int(scope.get("aggregate_size") or 4)
    return max(1, int(np.ceil(np.log2(max(size, 2)))))


def multi_pairwise_passes(A, scope, return_levels: bool = False):
    """The MULTI_PAIRWISE pass loop (reference multi_pairwise.cu
    setAggregates), written against ``ops`` so that it runs on host and
    device matrices alike: edge weights once, then per pass a handshake
    matching (ops.pairwise_matching) on the weight graph, coarsened between
    passes by the aggregation Galerkin product.

    ``full_ghost_level`` = 0: the next graph is the Galerkin product of the
    weight matrix (A's structure, w as values); its off-diagonal values are
    the next weights, its diagonal is ignored. 1: the Galerkin product of A
    itself, weights recomputed from it by the formula.
    ``merge_singletons`` = 2 caps aggregates at 2^passes + passes - passes/2
    rows (3, 5, 10, 18 for 1-4 passes); other modes have no cap.

    Returns (aggregates int32 (n,), num); with ``return_levels`` also the
    list of per-pass (level_agg, num, sizes, rounds)."""
    from ..matrix import CSRMatrix
    passes = _multi_pairwise_pass_count(scope)
    merge = int(scope.get("merge_singletons"))
    formula = int(scope.get("weight_formula"))
    full_ghost = int(scope.get("full_ghost_level"))
    maxit = int(scope.get("max_matching_iterations"))
    max_un = float(scope.get("max_unassigned_percentage"))
    min_rows = int(scope.get("min_coarse_rows"))
    cap = 2 ** passes + passes - passes // 2 if merge == 2 else 0

    n = A.n_rows
    w = ops.pairwise_weights(A, formula)
    dev = w.device
    ro, ci, work = A.row_offsets, A.col_indices, A
    sizes = torch.ones(n, dtype=torch.int32, device=dev)
    agg, num, levels = None, n, []
    for p in range(passes):
        level_agg, num, sizes, rounds = ops.pairwise_matching(
            ro, ci, w, n, sizes, cap, merge, maxit, max_un, p)
        levels.append((level_agg, num, sizes, rounds))
        agg = level_agg if agg is None else level_agg[agg.long()]
        if p == passes - 1 or num <= min_rows or num <= 1 or num == n:
            break
        # ghost level: the graph of the next pass
        if work.n_cols != work.n_rows:
            raise NotImplementedError(
                "MULTI_PAIRWISE ghost levels need a view without halo "
                "columns")
        if full_ghost:
            work = ops.galerkin_aggregation(work, level_agg, num)
            w = ops.pairwise_weights(work, formula)
        else:
            work = ops.galerkin_aggregation(
                CSRMatrix(ro, ci, w, n_cols=n), level_agg, num)
            w = work.values
        ro, ci, n = work.row_offsets, work.col_indices, num
    if return_levels:
        return agg, num, levels
    return agg, num


@register_agg_selector("MULTI_PAIRWISE")
def select_multi_pairwise(A, scope):
    """Notay-style multiple pairwise aggregation (reference
    multi_pairwise.cu). A device matrix runs the parallel handshake matching
    of ``multi_pairwise_passes`` on gfx950 kernels. A host matrix, and a
    device matrix with ``serial_matching`` = 1, runs the sequential greedy
    matcher below: edges sorted by descending scaled strength, composed
    log2(aggregate_size) times (the reference's serial_matching)."""
    if A.is_cuda and not int(scope.get("serial_matching") or 0):
        return multi_pairwise_passes(A, scope)
    size = int(scope.get("aggregate_size") or 4)
    passes = max(1, int(np.ceil(np.log2(max(size, 2)))))

    def greedy_match(M):
        from ..ops.cpu import _strength_weights
        w = _strength_weights(M)
        n = M.n_rows
        coo = w.tocoo()
        mask = coo.row < coo.col
        order = np.argsort(-coo.data[mask], kind="stable")
        er, ec = coo.row[mask][order], coo.col[mask][order]
        agg = np.full(n, -1, dtype=np.int64)
        nid = 0
        for i, j in zip(er, ec):
            if agg[i] < 0 and agg[j] < 0:
                agg[i] = agg[j] = nid
                nid += 1
        for i in np.nonzero(agg < 0)[0]:
            # join the strongest aggregated neighbor, else singleton
            s, e = w.indptr[i], w.indptr[i + 1]
            best, bw = -1, 0.0
            for k in range(s, e):
                jj = w.indices[k]
                if agg[jj] >= 0 and w.data[k] > bw:
                    best, bw = jj, w.data[k]
            if best >= 0:
                agg[i] = agg[best]
            else:
                agg[i] = nid
                nid += 1
        return torch.from_numpy(agg.astype(np.int32)), nid

    return _compose_passes(A, scope, passes, matcher=greedy_match)


@register_agg_selector("SERIAL_GREEDY")
def select_serial_greedy(A, scope):
    """BFS greedy aggregation up to aggregate_size rows per aggregate
    (reference serial_greedy.cu host path)."""
    from ..ops.cpu import _strength_weights
    size = int(scope.get("aggregate_size") or 2)
    w = _strength_weights(A)
    n = A.n_rows
    agg = np.full(n, -1, dtype=np.int64)
    nid = 0
    for s0 in range(n):
        if agg[s0] >= 0:
            continue
        members = [s0]
        agg[s0] = nid
        frontier = [s0]
        while len(members) < size and frontier:
            i = frontier.pop(0)
            s, e = w.indptr[i], w.indptr[i + 1]
            nbrs = [(w.data[k], w.indices[k]) for k in range(s, e)
                    if agg[w.indices[k]] < 0]
            for _, j in sorted(nbrs, reverse=True):
                if len(members) >= size:
                    break
                if agg[j] < 0:
                    agg[j] = nid
                    members.append(j)
                    frontier.append(j)
        nid += 1
    return torch.from_numpy(agg.astype(np.int32)), nid


@register_agg_selector("GEO")
def select_geo(A, scope):
    """Geometric aggregation from attached coordinates (reference
    geo_selector.cu + AMGX_matrix_attach_geometry, include/amgx_c.h): rows
    are binned into cells of ~aggregate_size points."""
    geom = A._cache.get("geometry")
    if geom is None:
        raise ValueError("GEO selector requires attach_geometry(coords)")
    pts = np.asarray(geom, dtype=np.float64)
    n, dim = pts.shape
    size = int(scope.get("aggregate_size") or 2)
    lo, hi = pts.min(0), pts.max(0)
    span = np.where(hi > lo, hi - lo, 1.0)
    cells_per_dim = max(1, int(round((n / size) ** (1.0 / dim))))
    cell = np.minimum((pts - lo) / span * cells_per_dim,
                      cells_per_dim - 1).astype(np.int64)
    key = cell[:, 0]
    for d in range(1, dim):
        key = key * cells_per_dim + cell[:, d]
    uniq, agg = np.unique(key, return_inverse=True)
    return torch.from_numpy(agg.astype(np.int32)), int(uniq.size)


@register_agg_selector("DUMMY")
def select_dummy(A, scope):
    """Consecutive fixed-size blocks (reference dummy.cu: index-order
    aggregates of aggregate_size)."""
    size = max(1, int(scope.get("aggregate_size") or 2))
    n = A.n_rows
    agg = (np.arange(n) // size).astype(np.int32)
    return torch.from_numpy(agg), int((n + size - 1) // size)


@register_agg_selector("ADAPTIVE")
def select_adaptive(A, scope):
    """Adaptive size selection (reference adaptive.cu): pick the pass count
    from average row degree — denser rows get bigger aggregates."""
    avg_deg = A.nnz / max(A.n_rows, 1)
    passes = 1 if avg_deg <= 5 else (2 if avg_deg <= 9 else 3)
    return _compose_passes(A, scope, passes)
