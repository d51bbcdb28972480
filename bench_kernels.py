#!/usr/bin/env python3
"""Per-kernel microbenchmarks on the current device (MI355X when available).

Times the solve-path kernels (csrmv, fused residual, DILU sweeps, color-GS,
reductions, axpy) and the setup kernels (coloring, matching, Galerkin,
SpGEMM, transpose) on a 3D Poisson problem, reporting ms and achieved GB/s
against the analytic bytes-moved model. One JSON line per kernel to stdout;
human table to stderr.

    python bench_kernels.py [--size 192] [--iters 20] [--section multi_pairwise]
    python bench_kernels.py [--size 192] [--iters 20] [--section dilu_lanes]
    python bench_kernels.py --size 64 --iters 50 --section dilu_small
    python bench_kernels.py [--size 192] [--iters 20] [--section dilu_stream]
    python bench_kernels.py [--size 192] [--iters 5] [--section setup]
"""

import argparse
import json
import sys
import time

import torch


def bench(fn, iters, sync):
    fn()                       # warmup
    sync()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    sync()
    return (time.perf_counter() - t0) / iters


def bench_multi_pairwise(A, iters, sync, rec):
    """MULTI_PAIRWISE on the device: the selector at 1, 2 and 3 passes next
    to SIZE_2 / SIZE_4 / SIZE_8 (equal pass counts), and the propose kernel
    in its thread-per-row and 8-lane forms on the graph of each
    pass (g1 = the matrix graph, g3 = the pass-3 ghost graph), on the
    benchmark's 7-point matrix and on a 27-point one."""
    from amgx_amd.amg.aggregation import AGG_SELECTOR_REGISTRY
    from amgx_amd.config import ConfigScope

    it = max(iters // 8, 1)
    for p, sized in ((1, "SIZE_2"), (2, "SIZE_4"), (3, "SIZE_8")):
        sc = ConfigScope(None, {"aggregation_passes": p,
                                "merge_singletons": 2})
        rec(f"multi_pairwise_select_p{p}", bench(
            lambda: AGG_SELECTOR_REGISTRY["MULTI_PAIRWISE"](A, sc), it, sync))
        rec(f"{sized.lower()}_select", bench(
            lambda: AGG_SELECTOR_REGISTRY[sized](A, ConfigScope(None, {})),
            it, sync))
    propose_records(A, "", iters, sync, rec)
    # the wider graphs of a 27-point stencil
    from amgx_amd.problems import poisson_3d_27pt
    side = min(round(A.n_rows ** (1.0 / 3.0)), 128)
    propose_records(poisson_3d_27pt(side, side, side, device=A.device),
                    "27pt_", iters, sync, rec)


def propose_records(A, tag, iters, sync, rec):
    """pairwise_propose with 1 and 8 lanes per row on the graph of each
    of three MULTI_PAIRWISE passes on A, every row unaggregated (the first
    and heaviest round)."""
    from amgx_amd import _core, ops
    from amgx_amd.amg.aggregation import multi_pairwise_passes
    from amgx_amd.config import ConfigScope
    from amgx_amd.matrix import CSRMatrix

    sc = ConfigScope(None, {"aggregation_passes": 3, "merge_singletons": 2})
    _, _, levels = multi_pairwise_passes(A, sc, return_levels=True)
    ro, ci, n = A.row_offsets, A.col_indices, A.n_rows
    w = ops.pairwise_weights(A, 0)
    sizes = torch.ones(n, dtype=torch.int32, device=w.device)
    for p, (level_agg, num, level_sizes, _) in enumerate(levels, 1):
        agg = torch.full((n,), -1, dtype=torch.int32, device=w.device)
        nnz = ci.numel()
        print(f"{tag}pass-{p} graph: {n} rows, {nnz / max(n, 1):.1f} "
              f"entries/row", file=sys.stderr)
        for lanes in (1, 8):
            rec(f"pairwise_propose_{tag}g{p}_l{lanes}", bench(
                lambda: _core.pairwise_propose(ro, ci, w, n, agg, sizes, 10,
                                               p - 1, lanes), iters, sync),
                nnz * 12 + (n + 1) * 4 + n * 12)
        if p < len(levels):
            G = ops.galerkin_aggregation(CSRMatrix(ro, ci, w, n_cols=n),
                                         level_agg, num)
            ro, ci, w, n = G.row_offsets, G.col_indices, G.values, num
            sizes = level_sizes


def bench_dilu_lanes(A, iters, sync, rec):
    """The three scalar per-color DILU sweeps with 1 and 8 lanes per row on
    the 7-point matrix and on its first two Galerkin levels under SIZE_2
    aggregation (about 7, 10 and 12.7 entries per row). A sweep is timed
    through one apply whose other sweep runs over an empty slab; `base` is
    the apply with both slabs empty (launches and row traffic only), to be
    subtracted (dilu_sweep_cases). The whole fused and plain applies
    follow."""
    from amgx_amd import _core, ops
    from amgx_amd.amg.coloring import MatrixColoring
    from amgx_amd.config import ConfigScope
    from amgx_amd.ops import gpu as G

    for level in range(3):
        if level:
            agg, num = ops.size2_matching(A)
            A = ops.galerkin_aggregation(A, agg.to(A.row_offsets.device), num)
        n, nnz = A.n_rows, A.nnz
        if n <= _core.DILU_SMALL_ROWS:
            sys.exit("--section dilu_lanes: level too small for the "
                     "per-color path; raise --size")
        col = MatrixColoring.create(A, ConfigScope(None, {}))
        einv = ops.dilu_setup(A, col)
        b = torch.ones(A.n_cols, dtype=torch.float64, device=A.device)
        x = torch.zeros_like(b)
        w, y = torch.empty_like(b), torch.empty_like(b)
        cases = dilu_sweep_cases(A, col, einv)
        print(f"level {level}: {n} rows, {nnz / n:.2f} entries/row "
              f"(L {cases[2][1][1].numel() / n:.2f}, "
              f"U {cases[3][2][1].numel() / n:.2f}), "
              f"{col.num_colors} colors", file=sys.stderr)
        for name, fwd, bwd, fused, nbytes in cases:
            for lanes in (1, 8):
                sec = bench(lambda: _core.dilu_split(
                    *fwd, *bwd, einv.einv_s, col.rows_sorted, col.bounds, b,
                    w, x, 0.75, fused, lanes, y), iters, sync)
                rec(f"dilu_{name}_g{level}_l{lanes}", sec, nbytes,
                    entries_per_row=nnz / n)
        for lanes in (0, 1, 8):
            rec(f"dilu_smooth_g{level}_l{lanes}", bench(
                lambda: G.dilu_smooth(A, einv, col, b, x, 0.75, lanes=lanes),
                iters, sync), entries_per_row=nnz / n)
            rec(f"dilu_apply_g{level}_l{lanes}", bench(
                lambda: G.dilu_solve(A, einv, col, b, 0.75, x, lanes=lanes),
                iters, sync), entries_per_row=nnz / n)


def eager_graph_cold(run, iters, sync, evict, side):
    """Seconds per eager call of run, and the record fields eager_us,
    graph_us, cold_us and cold_min_us described at bench_dilu_small; evict is
    the 512 MiB buffer streamed before each cold replay, side the capture
    stream."""
    eager = bench(run, iters, sync)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            run()
    torch.cuda.current_stream().wait_stream(side)
    warm = bench(graph.replay, iters, sync)
    cold = []
    for _ in range(max(iters, 5)):
        evict.add_(1.0)
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        graph.replay()
        t1.record()
        sync()
        cold.append(t0.elapsed_time(t1) * 1e-3)
    cold.sort()
    del graph
    return eager, dict(eager_us=eager * 1e6, graph_us=warm * 1e6,
                       cold_us=cold[len(cold) // 2] * 1e6,
                       cold_min_us=cold[0] * 1e6)


def dilu_sweep_cases(A, col, einv):
    """(name, forward slab, backward slab, fused, bytes) of the apply with
    both slabs empty (`base`: launches and row traffic only, to be
    subtracted) and of each sweep alone, its other sweep over an empty slab.
    Bytes: offsets + rows_sorted + Einv per sweep, then the row's own reads
    and writes (bench_kernels.py main, dilu records)."""
    from amgx_amd.ops import gpu as G

    n, nnz = A.n_rows, A.nnz
    st = G._slabs(A, col)
    ro_u, ci_u, _ = G._slab_part(st, True)
    ro_l, ci_l, _ = part_l = G._slab_part(st, False)
    va_l = G._gather_part(einv.va_s, part_l)
    empty = (torch.zeros_like(ro_u), ci_u[:0], einv.va_u[:0])
    full = (st.ro_s, st.ci_s, einv.va_s)
    lower, upper = (ro_l, ci_l, va_l), (ro_u, ci_u, einv.va_u)
    sweep = n * 16 + 4
    return (("base", empty, empty, False, None),
            ("fwd_full", full, empty, True, nnz * 12 + sweep + n * 40),
            ("fwd_lower", lower, empty, False,
             ci_l.numel() * 12 + sweep + n * 24),
            ("bwd_upper", empty, upper, False,
             ci_u.numel() * 12 + sweep + n * 32))


def bench_dilu_stream(A, iters, sync, rec, min_rows=1400):
    """The three scalar per-color DILU sweeps in their stream form next to 1
    and 8 lanes per row, on the matrix and its first two SIZE_2 Galerkin
    levels, timed as in bench_dilu_lanes (`base` to be subtracted; the stream
    form of an empty slab is the lane launch, so `base` has no stream record).
    Then three fused sweeps per form, and routed, on the SIZE_2 chain of a 64^3
    cube down to min_rows rows, where the colors are small: eager, graph
    replay and cold as in bench_dilu_small."""
    from amgx_amd import _core, ops
    from amgx_amd.amg.coloring import MatrixColoring
    from amgx_amd.config import ConfigScope
    from amgx_amd.ops import gpu as G
    from amgx_amd.problems import poisson_3d

    forms = (("l1", 1, 1), ("l8", 8, 1), ("stream", 0, 2))
    for level in range(3):
        if level:
            agg, num = ops.size2_matching(A)
            A = ops.galerkin_aggregation(A, agg.to(A.row_offsets.device), num)
        n, nnz = A.n_rows, A.nnz
        col = MatrixColoring.create(A, ConfigScope(None, {}))
        einv = ops.dilu_setup(A, col)
        b = torch.ones(A.n_cols, dtype=torch.float64, device=A.device)
        x = torch.zeros_like(b)
        w, y = torch.empty_like(b), torch.empty_like(b)
        sizes = [e - s for s, e in zip(col.bounds[:-1], col.bounds[1:])]
        print(f"level {level}: {n} rows, {nnz / n:.2f} entries/row, "
              f"{col.num_colors} colors of {min(sizes)}..{max(sizes)} rows",
              file=sys.stderr)
        for name, fwd, bwd, fused, nbytes in dilu_sweep_cases(A, col, einv):
            for tag, lanes, form in forms:
                if name == "base" and form == 2:
                    continue
                sec = bench(lambda: _core.dilu_split(
                    *fwd, *bwd, einv.einv_s, col.rows_sorted, col.bounds, b,
                    w, x, 0.75, fused, lanes, y, form), iters, sync)
                rec(f"dilu_stream_{name}_g{level}_{tag}", sec, nbytes,
                    rows=n, colors=col.num_colors,
                    entries_per_row=(fwd[1].numel() + bwd[1].numel()) / n)
    chain = (("l1", dict(form="split", lanes=1)),
             ("l8", dict(form="split", lanes=8)),
             ("stream", dict(form="stream")),
             ("routed", dict(form="split")))
    A = poisson_3d(64, 64, 64, device=A.device)
    evict = torch.zeros(512 << 18, dtype=torch.float32, device=A.device)
    side = torch.cuda.Stream()
    while A.n_rows >= min_rows:
        n, nnz = A.n_rows, A.nnz
        col = MatrixColoring.create(A, ConfigScope(None, {}))
        einv = ops.dilu_setup(A, col)
        b = torch.ones(A.n_cols, dtype=torch.float64, device=A.device)
        x = torch.zeros_like(b)
        for name, how in chain:
            def run():
                G.dilu_smooth(A, einv, col, b, x, 0.75, sweeps=3, **how)
            eager, times = eager_graph_cold(run, iters, sync, evict, side)
            # three sweeps: y pass, full slab forward, U backward
            rec(f"dilu_stream_chain_{name}_n{n}", eager,
                3 * (nnz * 18 + n * 120), rows=n, entries_per_row=nnz / n,
                colors=col.num_colors, rows_per_color=n / col.num_colors,
                **times)
        agg, num = ops.size2_matching(A)
        A = ops.galerkin_aggregation(A, agg.to(A.row_offsets.device), num)


def bench_dilu_small(A, iters, sync, rec, max_rows=32768):
    """Three fused DILU sweeps on the levels of at most max_rows rows of the
    SIZE_2 Galerkin chain of A, through the one-launch apply in its earlier
    full-slab form (`full`), the one-launch split-slab apply with 1 and with 8
    lanes per row and routed (`small_l1`, `small_l8`, `small`), and the
    per-color sweeps (`split`). Per form three figures, in microseconds per
    three sweeps: `eager_us` back-to-back calls timed on the host (launch cost
    included), `graph_us` back-to-back replays of the captured calls, and
    `cold_us` one replay after a streaming pass over 512 MiB has evicted the
    level from the caches, timed with events, median of the repetitions: a
    V-cycle meets each level cold, after the fine levels' traffic."""
    from amgx_amd import _core, ops
    from amgx_amd.amg.coloring import MatrixColoring
    from amgx_amd.config import ConfigScope
    from amgx_amd.ops import gpu as G

    forms = (("full", dict(form="small_full")),
             ("small_l1", dict(form="small", lanes=1)),
             ("small_l8", dict(form="small", lanes=8)),
             ("small", dict(form="small")),
             ("split", dict(form="split")))
    evict = torch.zeros(512 << 18, dtype=torch.float32, device=A.device)
    side = torch.cuda.Stream()
    while A.n_rows >= 48:
        n, nnz = A.n_rows, A.nnz
        if n <= max_rows:
            col = MatrixColoring.create(A, ConfigScope(None, {}))
            einv = ops.dilu_setup(A, col)
            b = torch.ones(A.n_cols, dtype=torch.float64, device=A.device)
            x = torch.zeros_like(b)
            nnz_u = G._slab_part(G._slabs(A, col), True)[1].numel()
            print(f"{n} rows, {nnz / n:.2f} entries/row (U {nnz_u / n:.2f}), "
                  f"{col.num_colors} colors, one-launch routing: "
                  f"{n <= _core.DILU_SMALL_ROWS}", file=sys.stderr)
            for name, how in forms:
                def run():
                    G.dilu_smooth(A, einv, col, b, x, 0.75, sweeps=3, **how)
                eager, times = eager_graph_cold(run, iters, sync, evict, side)
                rec(f"dilu_small_{name}_n{n}", eager, rows=n,
                    entries_per_row=nnz / n, colors=col.num_colors, **times)
        agg, num = ops.size2_matching(A)
        A = ops.galerkin_aggregation(A, agg.to(A.row_offsets.device), num)


def bench_setup(A, iters, sync, rec):
    """The setup pieces outside the sparse products, on the 7-point matrix
    and on its first two Galerkin levels under SIZE_2 aggregation: the
    coloring loop, the matching loop with its renumbering, the color order
    (MatrixColoring), the aggregate-membership CSR and the slab structure.
    The two round loops also run cut off after their first round, next to
    the bytes that round has to move; that figure carries the loop's fixed
    cost (two allocations, one fill, one read-back). Where the tree has the
    batch argument, the loops are timed for k = 1, 2, 4, 8 rounds per
    read-back next to the default rule, and the matching with its edge
    weights computed in every round and once per call. A tree without the native entries
    times the torch expressions it runs in their place, so the same section
    compares two trees piece by piece."""
    from amgx_amd import _core, ops
    from amgx_amd.amg.coloring import MatrixColoring
    from amgx_amd.ops import gpu as G

    batched = hasattr(G, "ROUND_BATCH")

    def first_round_color():
        try:
            _core.color_minmax(A.row_offsets, A.col_indices, A.n_rows, 1, 0, 0)
        except RuntimeError:
            pass    # one round does not color the graph: that is the point

    def torch_aggregate_csr(agg, num):
        a64 = agg.to(torch.int64)
        order = torch.argsort(a64, stable=True).to(torch.int32)
        off = torch.zeros(num + 1, dtype=torch.int64, device=agg.device)
        torch.cumsum(torch.bincount(a64, minlength=num), 0, out=off[1:])
        return off.to(torch.int32), order

    def slabs(col):
        A._cache.pop("slabs", None)
        return G._slabs(A, col)

    for level in range(3):
        if level:
            A = ops.galerkin_aggregation(A, agg, num)
        n, nnz = A.n_rows, A.nnz
        tag = f"L{level}"
        print(f"{tag}: {n} rows, {nnz / max(n, 1):.1f} entries/row",
              file=sys.stderr)
        colors, nc = ops.color_matrix(A)
        agg, num = ops.size2_matching(A)
        G._tidx(A)   # cached by the matrix: not part of the matching loop
        rec(f"setup_color_minmax_{tag}",
            bench(lambda: ops.color_matrix(A), iters, sync), rows=n,
            colors=nc)
        rec(f"setup_color_round1_{tag}", bench(first_round_color, iters, sync),
            nnz * 4 + n * 12, rows=n)
        rec(f"setup_size2_match_renumber_{tag}",
            bench(lambda: ops.size2_matching(A), iters, sync), rows=n,
            aggregates=num)
        rec(f"setup_size2_round1_{tag}",
            bench(lambda: ops.size2_matching(A, max_iterations=1), iters,
                  sync),
            # propose (structure, values, transpose index, diagonal, state),
            # match (proposals read and gathered), singleton sweep, renumber
            nnz * 16 + n * 24 + n * 12 + nnz * 16 + n * 20 + n * 16, rows=n)
        if batched:
            for k in (1, 2, 4, 8):
                rec(f"setup_color_minmax_{tag}_k{k}",
                    bench(lambda: G.color_matrix(A, batch=k), iters, sync))
                rec(f"setup_size2_match_renumber_{tag}_k{k}",
                    bench(lambda: G.size2_matching(A, batch=k), iters, sync))
            # propose-kernel A/B: weights computed in every round (w0)
            # against once per call into one double per entry (w1)
            for w in (0, 1):
                rec(f"setup_size2_roots_{tag}_w{w}",
                    bench(lambda: G.size2_roots(A, weights=bool(w)), iters,
                          sync))
        rec(f"setup_color_order_{tag}",
            bench(lambda: MatrixColoring(colors, nc), iters, sync), rows=n)
        build_csr = (lambda: G.aggregate_csr(agg, num)) \
            if hasattr(G, "aggregate_csr") \
            else (lambda: torch_aggregate_csr(agg, num))
        rec(f"setup_aggregate_csr_{tag}", bench(build_csr, iters, sync),
            rows=n)
        col = MatrixColoring(colors, nc)
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        rec(f"setup_slabs_{tag}", bench(lambda: slabs(col), iters, sync),
            rows=n,
            peak_extra_MB=(torch.cuda.max_memory_allocated() - base) / 1e6)
        A._cache.pop("slabs", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=192)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--section", default="all",
                    choices=("all", "multi_pairwise", "dilu_lanes",
                             "dilu_small", "dilu_stream", "setup"),
                    help="multi_pairwise: only the MULTI_PAIRWISE records; "
                         "dilu_lanes: the DILU sweeps by lanes per row; "
                         "dilu_small: the one-launch DILU apply against the "
                         "per-color sweeps on the small Galerkin levels; "
                         "dilu_stream: the stream form of the DILU sweeps "
                         "against the lane forms; setup: the coloring and "
                         "matching loops and the orderings of the setup "
                         "path, per piece")
    args = ap.parse_args()
    sys.path.insert(0, ".")
    from amgx_amd import ops
    from amgx_amd.amg.coloring import MatrixColoring
    from amgx_amd.config import ConfigScope
    from amgx_amd.problems import poisson_3d
    from amgx_amd.solvers.dilu import dilu_setup, dilu_solve

    dev = "cuda:0" if torch.cuda.is_available() else "cpu"
    sync = (lambda: torch.cuda.synchronize()) if dev != "cpu" else (lambda: 0)
    n3 = args.size
    A = poisson_3d(n3, n3, n3, device=dev)
    n, nnz = A.n_rows, A.nnz
    x = torch.rand(n, dtype=torch.float64, device=dev)
    y = torch.zeros_like(x)
    b = torch.ones_like(x)

    rows_bytes = nnz * 12 + (n + 1) * 4            # vals+cols+offsets
    spmv_bytes = rows_bytes + n * 8 * 2            # + x read, y write (approx)

    results = {}

    def rec(name, sec, bytes_moved=None, **extra):
        gbps = bytes_moved / sec / 1e9 if bytes_moved else None
        results[name] = {"ms": sec * 1e3, "GBps": gbps}
        print(json.dumps({"kernel": name, "ms": sec * 1e3, "GBps": gbps,
                          **extra}))

    if args.section == "multi_pairwise":
        if dev == "cpu":
            sys.exit("--section multi_pairwise times device kernels: no GPU")
        bench_multi_pairwise(A, args.iters, sync, rec)
        return
    if args.section == "dilu_lanes":
        if dev == "cpu":
            sys.exit("--section dilu_lanes times device kernels: no GPU")
        bench_dilu_lanes(A, args.iters, sync, rec)
        return
    if args.section == "dilu_stream":
        if dev == "cpu":
            sys.exit("--section dilu_stream times device kernels: no GPU")
        bench_dilu_stream(A, args.iters, sync, rec)
        return
    if args.section == "setup":
        if dev == "cpu":
            sys.exit("--section setup times device kernels: no GPU")
        bench_setup(A, args.iters, sync, rec)
        return
    if args.section == "dilu_small":
        if dev == "cpu":
            sys.exit("--section dilu_small times device kernels: no GPU")
        bench_dilu_small(A, args.iters, sync, rec)
        return

    rec("csrmv", bench(lambda: ops.spmv(A, x, y), args.iters, sync),
        spmv_bytes)
    from amgx_amd.matrix import CSRMatrix
    A32 = CSRMatrix(A.row_offsets, A.col_indices,
                    A.values.to(torch.float32), n_cols=A.n_cols)
    rec("csrmv_mixed_f32A", bench(lambda: ops.spmv(A32, x, y),
                                  args.iters, sync),
        nnz * 8 + (n + 1) * 4 + n * 16)   # fp32 vals: half the value bytes
    # complex128 (dZZI) on the same pattern, same bytes model: 16 B value +
    # 4 B column per nnz (12 B in the real row), x and y counted once
    Az = CSRMatrix(A.row_offsets, A.col_indices,
                   torch.complex(A.values, 0.25 * A.values), n_cols=A.n_cols)
    xz = torch.complex(x, torch.rand_like(x))
    yz = torch.zeros_like(xz)
    rec("csrmv_complex128", bench(lambda: ops.spmv(Az, xz, yz),
                                  args.iters, sync),
        nnz * 20 + (n + 1) * 4 + n * 16 * 2)
    del Az, xz, yz
    r = torch.zeros_like(x)
    rec("residual_fused", bench(lambda: ops.residual(A, x, b, r),
                                args.iters, sync), spmv_bytes + n * 8)
    rec("dot", bench(lambda: ops.dot(x, y), args.iters, sync), n * 16)
    rec("nrm2", bench(lambda: ops.nrm2(x), args.iters, sync), n * 8)
    rec("axpy", bench(lambda: ops.axpy(y, x, 0.5), args.iters, sync), n * 24)

    col = MatrixColoring.create(A, ConfigScope(None, {}))
    dinv = ops.jacobi_dinv(A)
    rec("jacobi_sweep", bench(
        lambda: ops.jacobi_smooth(A, dinv, b, x, y, 0.9), args.iters, sync),
        spmv_bytes + n * 24)
    rec("gs_color_sweep", bench(
        lambda: ops.gs_sweep(A, dinv, b, x.clone(), col, 0.9),
        max(args.iters // 4, 2), sync), spmv_bytes + n * 24)
    einv = dilu_setup(A, col)
    B = ops._backend(A)
    t_apply = bench(lambda: dilu_solve(A, einv, col, r, 0.75, y), args.iters,
                    sync)
    # bytes of one scalar DILU apply, every array counted once per sweep.
    # Both sweeps read offsets + rows_sorted + Einv (n * 16 + 4); the
    # backward sweep reads the U part, reads and writes w and x (n * 32).
    # dilu_apply: forward over the L part, reads r and w, writes w (n * 24).
    # dilu_smooth: the y = x + 0 pass (n * 16), forward over the full slab,
    # reads b, x and the one gathered vector y, writes w and y (n * 40).
    st = A._cache.get("slabs")
    if st is not None and getattr(st, "upper", None) is not None:
        nnz_u = st.upper[1].numel()
        nnz_l = st.lower[1].numel() if st.lower is not None else nnz - n - nnz_u
    else:                       # symmetric pattern: half the off-diagonals
        nnz_u = nnz_l = (nnz - n) // 2
    sweep_bytes = n * 16 + 4
    bwd_bytes = nnz_u * 12 + sweep_bytes + n * 32
    rec("dilu_apply", t_apply, nnz_l * 12 + sweep_bytes + n * 24 + bwd_bytes)
    if getattr(B, "dilu_smooth", None) is not None:
        rec("dilu_smooth", bench(
            lambda: B.dilu_smooth(A, einv, col, b, y, 0.75), args.iters,
            sync), n * 16 + nnz * 12 + sweep_bytes + n * 40 + bwd_bytes)

    # block-4 kernels: MFMA wave path vs the scalar baseline
    from amgx_amd.problems import block_laplacian
    side = max(args.size, 64)          # side^2 block rows
    A4 = block_laplacian(side, side, block_dim=4, seed=3).to(dev)
    n4 = A4.n_rows
    x4 = torch.rand(n4 * 4, dtype=torch.float64, device=dev)
    y4 = torch.zeros_like(x4)
    b4_bytes = A4.nnz * (16 * 8 + 4) + (n4 + 1) * 4 + n4 * 4 * 16
    rec("bsrmv_b4_mfma", bench(lambda: ops.spmv(A4, x4, y4),
                               args.iters, sync), b4_bytes)
    if dev != "cpu":
        from amgx_amd import _core
        rec("bsrmv_b4_scalar_base", bench(
            lambda: _core.bsrmv_generic(A4.row_offsets, A4.col_indices,
                                        A4.values.reshape(-1), 4,
                                        x4, y4, 1.0, 0.0),
            args.iters, sync), b4_bytes)
    col4 = MatrixColoring.create(A4, ConfigScope(None, {}))
    e4 = dilu_setup(A4, col4)
    r4 = torch.rand_like(x4)
    rec("dilu_b4_apply_mfma", bench(
        lambda: dilu_solve(A4, e4, col4, r4, 1.0, y4), args.iters, sync),
        2 * A4.nnz * 16 * 8 + n4 * 4 * 40)
    rec("dilu_b4_setup_mfma", bench(
        lambda: dilu_setup(A4, col4), max(args.iters // 4, 2), sync))

    # setup-path
    rec("coloring_minmax", bench(
        lambda: ops.color_matrix(A), max(args.iters // 4, 2), sync))
    rec("size2_matching", bench(
        lambda: ops.size2_matching(A), max(args.iters // 8, 1), sync))
    agg, num = ops.size2_matching(A)
    agg = agg.to(A.row_offsets.device)
    rec("galerkin_agg", bench(
        lambda: ops.galerkin_aggregation(A, agg, num),
        max(args.iters // 8, 1), sync))
    rec("transpose", bench(lambda: ops.transpose(A),
                           max(args.iters // 8, 1), sync))
    if dev != "cpu":   # the host selector is an interpreted loop
        bench_multi_pairwise(A, args.iters, sync, rec)
    print("kernel              ms         GB/s", file=sys.stderr)
    for k, v in results.items():
        gb = f"{v['GBps']:.0f}" if v["GBps"] else "-"
        print(f"{k:18s} {v['ms']:9.3f}  {gb}", file=sys.stderr)


if __name__ == "__main__":
    main()
