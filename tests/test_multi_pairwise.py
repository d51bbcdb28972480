"""MULTI_PAIRWISE on the host: the per-row oracle (``ops/cpu.py``
``pairwise_weights`` / ``pairwise_matching``) against a dense reference and
against the properties the algorithm of docs/KERNELS.md promises, the pass
driver ``multi_pairwise_passes``, and the unchanged host selector.

``tests/test_gpu_multi_pairwise.py`` imports the matrices and the checkers
from here to test the device kernels against the oracle.

The test graphs carry weights that are small integers over powers of two, so
every weight, every ghost-level sum and every comparison is exact in fp64.
"""

from types import SimpleNamespace

import numpy as np
import pytest
import torch

from amgx_amd import CSRMatrix, ops
from amgx_amd.amg.aggregation import (multi_pairwise_passes,
                                      select_multi_pairwise)
from amgx_amd.config import ConfigScope
from amgx_amd.problems import poisson_3d

MERGE = pytest.mark.parametrize("merge", [0, 1, 2])


# ===================================================================== matrices
def signed_matrix(n, seed=0, n_halo=20):
    """Signed nonsymmetric n-row CSR (sorted unique columns, n + n_halo
    columns) with missing transposes, stored zeros, zero and absent
    diagonals and halo columns. Values are multiples of 1/4 below 8 in
    modulus: exact in fp32, and exact moduli when scaled by 3+4i."""
    rng = np.random.RandomState(seed)
    rows = [dict() for _ in range(n)]
    for i in range(n):
        for d in (1, 5, 37):
            j = i + d
            if j >= n or rng.rand() < 0.2:
                continue
            a, b = rng.randint(-16, 17, size=2) / 4.0   # zeros are stored
            u = rng.rand()
            if u < 0.8 or u >= 0.9:
                rows[i][j] = a
            if u < 0.9:                                  # else: no transpose
                rows[j][i] = b
        u = rng.rand()
        if u < 0.8:
            rows[i][i] = float(rng.choice([1.0, 2.0, 4.0, -2.0, 0.5, 3.0]))
        elif u < 0.9:
            rows[i][i] = 0.0                             # stored zero
        if n_halo and rng.rand() < 0.1:
            rows[i][n + rng.randint(n_halo)] = float(rng.randint(1, 9))
    ro = np.zeros(n + 1, dtype=np.int64)
    ci, va = [], []
    for i in range(n):
        for c in sorted(rows[i]):
            ci.append(c)
            va.append(rows[i][c])
        ro[i + 1] = len(ci)
    return SimpleNamespace(ro=ro, ci=np.asarray(ci, dtype=np.int64),
                           va=np.asarray(va, dtype=np.float64), n=n,
                           ncols=n + n_halo)


def to_csr(m, dtype=torch.float64, device="cpu"):
    """CSRMatrix of a signed_matrix; a complex dtype scales by 3+4i."""
    va = torch.from_numpy(m.va)
    va = (va.to(torch.complex128) * (3 + 4j)).to(dtype) if dtype.is_complex \
        else va.to(dtype)
    A = CSRMatrix(torch.from_numpy(m.ro.astype(np.int32)),
                  torch.from_numpy(m.ci.astype(np.int32)), va,
                  n_cols=m.ncols)
    return A.to(device)


def dense_weights(m, formula, cplx_scale=False):
    """The weight rule on dense lookups, in double."""
    n = m.n
    present = np.zeros((n, m.ncols), dtype=bool)
    val = np.zeros((n, m.ncols), dtype=np.float64)
    for i in range(n):
        for k in range(m.ro[i], m.ro[i + 1]):
            present[i, m.ci[k]] = True
            val[i, m.ci[k]] = m.va[k]

    def mod(v):   # |v (3+4i)| = sqrt((3v)^2 + (4v)^2), exact here
        return float(np.sqrt((3 * v) ** 2 + (4 * v) ** 2)) if cplx_scale \
            else abs(float(v))

    w = np.zeros(m.ci.size, dtype=np.float64)
    for i in range(n):
        for k in range(m.ro[i], m.ro[i + 1]):
            j = m.ci[k]
            if j == i or j >= n or not present[j, i]:
                continue
            dii = val[i, i] if present[i, i] else 0.0
            djj = val[j, j] if present[j, j] else 0.0
            if formula == 0:
                d = max(mod(dii), mod(djj))
                if d > 0.0:
                    w[k] = 0.5 * (mod(val[i, j]) + mod(val[j, i])) / d
            elif dii != 0.0 and djj != 0.0:
                w[k] = -0.5 * (val[i, j] / dii + val[j, i] / djj)
    return w


def graph(n, edges):
    """Weight graph from undirected edges {(i, j): w}: (ro, ci, w) int32 /
    float64 tensors with both directions stored and sorted columns."""
    rows = [dict() for _ in range(n)]
    for (i, j), wt in edges.items():
        rows[i][j] = wt
        rows[j][i] = wt
    ro, ci, w = [0], [], []
    for i in range(n):
        for c in sorted(rows[i]):
            ci.append(c)
            w.append(rows[i][c])
        ro.append(len(ci))
    return SimpleNamespace(
        n=n, ro=torch.tensor(ro, dtype=torch.int32),
        ci=torch.tensor(ci, dtype=torch.int32),
        w=torch.tensor(w, dtype=torch.float64).reshape(-1))


def star(leaves=70, weights=None):
    """Node 0 joined to `leaves` leaves; equal weights unless given."""
    return graph(leaves + 1, {(0, j): (weights[j - 1] if weights else 0.5)
                              for j in range(1, leaves + 1)})


def path(n=40):
    """Edge (i, i+1) weighs (i+1)/64: only the last free edge is ever a
    mutual proposal, so every round forms exactly one pair."""
    return graph(n, {(i, i + 1): (i + 1) / 64.0 for i in range(n - 1)})


def poisson_graph(nx):
    A = poisson_3d(nx, nx, nx)
    return SimpleNamespace(n=A.n_rows, ro=A.row_offsets, ci=A.col_indices,
                           w=ops.pairwise_weights(A, 0))


def dyadic_matrix(kind, seed=3):
    """Symmetric-structure matrices with power-of-two diagonals and small
    integer off-diagonals: every weight of either formula and every
    ghost-level sum is exact. 'grid': 13 x 11 nine-point stencil, 'random':
    150 rows with about 4 random neighbours each."""
    rng = np.random.RandomState(seed)
    if kind == "grid":
        nx, ny = 13, 11
        n = nx * ny
        pairs = set()
        for y in range(ny):
            for x in range(nx):
                for dx, dy in ((1, 0), (0, 1), (1, 1), (1, -1)):
                    if 0 <= x + dx < nx and 0 <= y + dy < ny:
                        pairs.add((y * nx + x, (y + dy) * nx + x + dx))
    else:
        n = 150
        pairs = set()
        for i in range(n):
            for j in rng.randint(n, size=2):
                if i != j:
                    pairs.add((min(i, int(j)), max(i, int(j))))
    rows = [{i: float(2 ** rng.randint(3, 6))} for i in range(n)]
    for i, j in sorted(pairs):
        rows[i][j] = -float(rng.randint(1, 5))
        rows[j][i] = -float(rng.randint(1, 5))
    ro, ci, va = [0], [], []
    for i in range(n):
        for c in sorted(rows[i]):
            ci.append(c)
            va.append(rows[i][c])
        ro.append(len(ci))
    return CSRMatrix(torch.tensor(ro, dtype=torch.int32),
                     torch.tensor(ci, dtype=torch.int32),
                     torch.tensor(va, dtype=torch.float64), n_cols=n)


def matrix_graph(A, formula=0):
    return SimpleNamespace(n=A.n_rows, ro=A.row_offsets, ci=A.col_indices,
                           w=ops.pairwise_weights(A, formula))


# ===================================================================== checkers
def run_matching(g, merge, cap=0, sizes=None, max_iterations=10 ** 6,
                 max_unassigned=0.0, seed=0):
    sizes = torch.ones(g.n, dtype=torch.int32, device=g.w.device) \
        if sizes is None else sizes
    return ops.pairwise_matching(g.ro, g.ci, g.w, g.n, sizes, cap, merge,
                                 max_iterations, max_unassigned, seed)


def _adjacency(g):
    """neighbours over edges with w > 0, as {i: {j: w}} (entry (i, j))."""
    ro, ci, w = g.ro.cpu().numpy(), g.ci.cpu().numpy(), g.w.cpu().numpy()
    return [{int(ci[k]): float(w[k]) for k in range(ro[i], ro[i + 1])
             if ci[k] != i and ci[k] < g.n and w[k] > 0.0}
            for i in range(g.n)]


def root_vector(agg0, agg):
    """Root row of every aggregate of `agg`, given the merge_singletons = 0
    result `agg0` of the same matching: an aggregate holds exactly one
    matched pair (root = its smaller row) or is a single never-matched row."""
    n = len(agg0)
    members0 = {}
    for i in range(n):
        members0.setdefault(int(agg0[i]), []).append(i)
    root = {}
    for i in range(n):
        a = int(agg[i])
        pair = members0[int(agg0[i])]
        if len(pair) == 2:
            assert root.setdefault(a, pair[0]) == pair[0], \
                "two matched pairs in one aggregate"
    out = np.empty(n, dtype=np.int64)
    for i in range(n):
        a = int(agg[i])
        if a not in root:
            assert (np.asarray(agg) == a).sum() == 1, \
                "an aggregate of leftovers only"
            root[a] = i
        out[i] = root[a]
    return out


def check_invariants(g, merge, cap, result, result0, sizes=None,
                     exhausted=True):
    """Properties of one pairwise_matching result; result0 is the
    merge_singletons = 0 result of the same call (same matching phase)."""
    n = g.n
    agg, num, szs, _ = result
    agg = agg.cpu().numpy().astype(np.int64)
    szs = szs.cpu().numpy().astype(np.int64)
    agg0 = result0[0].cpu().numpy().astype(np.int64)
    sizes = np.ones(n, dtype=np.int64) if sizes is None \
        else sizes.cpu().numpy().astype(np.int64)
    adj = _adjacency(g)
    big = cap if cap > 0 else 1 << 60

    # a partition with ids 0..num-1, numbered in ascending root order
    assert agg.shape == (n,) and szs.shape == (num,)
    assert np.array_equal(np.unique(agg), np.arange(num))
    roots = root_vector(agg0, agg)
    uniq, inv = np.unique(roots, return_inverse=True)
    assert np.array_equal(inv, agg)
    # sizes are the member sums
    assert np.array_equal(np.bincount(agg, weights=sizes, minlength=num)
                          .astype(np.int64), szs)
    # every aggregate is connected through w > 0 edges
    members = [[] for _ in range(num)]
    for i in range(n):
        members[agg[i]].append(i)
    for a, mem in enumerate(members):
        seen, todo = {mem[0]}, [mem[0]]
        while todo:
            i = todo.pop()
            for j in adj[i]:
                if agg[j] == a and j not in seen:
                    seen.add(j)
                    todo.append(j)
        assert len(seen) == len(mem), f"aggregate {a} is not connected"
    if merge == 2:
        assert szs.max() <= big

    # the matching phase: pairs and leftovers, read off the mode-0 result
    cnt0 = np.bincount(agg0)
    assert cnt0.max() <= 2
    left = cnt0[agg0] == 1
    if exhausted:   # maximal: no eligible edge between two leftovers
        for i in np.nonzero(left)[0]:
            for j in adj[i]:
                assert not (left[j] and sizes[i] + sizes[j] <= big), (i, j)

    # the leftover phase
    cnt = np.bincount(agg)
    single = cnt[agg] == 1
    if merge == 0:
        assert np.array_equal(agg, agg0)
    elif merge == 1:
        for i in np.nonzero(left)[0]:
            paired = {j: wt for j, wt in adj[i].items() if not left[j]}
            if paired:   # first sweep: the largest edge to an aggregate
                top = max(paired.values())
                assert agg[i] in {agg[j] for j, wt in paired.items()
                                  if wt == top}
            if single[i]:   # nothing aggregated within reach, ever
                assert all(single[j] for j in adj[i])
    else:
        for i in np.nonzero(left & single)[0]:
            for j in adj[i]:   # no neighbouring aggregate had room left
                assert single[j] and left[j] or \
                    szs[agg[j]] + sizes[i] > big, (i, j)


# ====================================================================== weights
M777 = signed_matrix(777, seed=1)


@pytest.mark.parametrize("formula", [0, 1])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32],
                         ids=["fp64", "fp32"])
def test_weights_against_dense_loop(dtype, formula):
    w = ops.pairwise_weights(to_csr(M777, dtype), formula).numpy()
    ref = dense_weights(M777, formula)
    assert w.dtype == np.float64 and np.array_equal(w, ref)
    assert (ref > 0).sum() > 500 and (ref == 0).sum() > 500
    if formula == 1:
        assert (ref < 0).sum() > 100


@pytest.mark.parametrize("dtype", [torch.complex128, torch.complex64],
                         ids=["c128", "c64"])
def test_weights_complex_modulus(dtype):
    w = ops.pairwise_weights(to_csr(M777, dtype), 0).numpy()
    assert np.array_equal(w, dense_weights(M777, 0, cplx_scale=True))
    # |3+4i| = 5 scales every modulus alike and cancels in formula 0
    assert np.array_equal(w, dense_weights(M777, 0))


@pytest.mark.parametrize("formula", [0, 1])
def test_weights_are_bitwise_symmetric(formula):
    m = signed_matrix(300, seed=4, n_halo=0)
    va = m.va * np.random.RandomState(9).rand(m.va.size)   # inexact values
    A = CSRMatrix(torch.from_numpy(m.ro.astype(np.int32)),
                  torch.from_numpy(m.ci.astype(np.int32)),
                  torch.from_numpy(va), n_cols=m.n)
    w = ops.pairwise_weights(A, formula).numpy()
    W = {(i, int(m.ci[k])): w[k] for i in range(m.n)
         for k in range(m.ro[i], m.ro[i + 1])}
    for (i, j), wt in W.items():
        if wt != 0.0:
            assert W[(j, i)] == wt


def test_weights_rejections():
    with pytest.raises(NotImplementedError):
        ops.pairwise_weights(to_csr(M777, torch.complex128), 1)
    Ab = block_matrix()
    with pytest.raises(NotImplementedError):
        ops.pairwise_weights(Ab, 1)
    with pytest.raises(NotImplementedError):
        ops.pairwise_weights(
            CSRMatrix(Ab.row_offsets, Ab.col_indices,
                      Ab.values.to(torch.complex128), n_cols=Ab.n_cols,
                      block_dim=4), 0)


def block_matrix(b=4, seed=6):
    """Real block-b matrix on the structure of dyadic_matrix('grid')."""
    S = dyadic_matrix("grid")
    rng = np.random.RandomState(seed)
    ro, ci = S.row_offsets.numpy(), S.col_indices.numpy()
    vals = rng.randn(ci.size, b, b) * 0.3
    for i in range(S.n_rows):
        for k in range(ro[i], ro[i + 1]):
            if ci[k] == i:
                vals[k] = 4.0 * np.eye(b) + 0.1 * rng.randn(b, b)
    return CSRMatrix(S.row_offsets, S.col_indices, torch.from_numpy(vals),
                     n_cols=S.n_cols, block_dim=b)


def test_block_weights_use_frobenius_norms():
    Ab = block_matrix()
    nrm = np.sqrt((Ab.values.numpy() ** 2).sum(axis=(1, 2)))
    As = CSRMatrix(Ab.row_offsets, Ab.col_indices, torch.from_numpy(nrm),
                   n_cols=Ab.n_cols)
    assert np.array_equal(ops.pairwise_weights(Ab, 0).numpy(),
                          ops.pairwise_weights(As, 0).numpy())


# ===================================================================== matching
def _graphs():
    return {"poisson8": (poisson_graph(8), 5),
            "star": (star(), 5),
            "star_distinct": (star(weights=[(1 + (37 * j) % 70) / 128.0
                                            for j in range(70)]), 5),
            "path": (path(), 3),
            "one_row": (graph(1, {}), 3),
            "one_row_diag": (SimpleNamespace(
                n=1, ro=torch.tensor([0, 1], dtype=torch.int32),
                ci=torch.tensor([0], dtype=torch.int32),
                w=torch.zeros(1, dtype=torch.float64)), 3),
            "one_edge": (graph(2, {(0, 1): 0.25}), 3),
            "dyadic_random": (matrix_graph(dyadic_matrix("random")), 5)}


GRAPHS = _graphs()


@MERGE
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_matching_invariants(name, merge):
    g, cap = GRAPHS[name]
    cap = cap if merge == 2 else 0
    res0 = run_matching(g, 0, cap)
    res = run_matching(g, merge, cap)
    check_invariants(g, merge, cap, res, res0)
    assert res[3] == res0[3] >= (1 if g.n else 0)


@MERGE
def test_matching_with_sizes_respects_the_cap(merge):
    """A later pass: node sizes 1..4 enter the eligibility of an edge."""
    g = GRAPHS["dyadic_random"][0]
    sizes = torch.from_numpy(
        np.random.RandomState(2).randint(1, 5, size=g.n).astype(np.int32))
    res0 = run_matching(g, 0, 6, sizes=sizes)
    res = run_matching(g, merge, 6, sizes=sizes)
    check_invariants(g, merge, 6, res, res0, sizes=sizes)
    if merge != 1:
        assert res[2].max() <= 6


def test_star_accepts_one_leaf_per_round():
    """Equal weights, cap 5: the hash picks the matched leaf, then the root
    takes the smallest remaining leaf in each of three capped rounds."""
    g, cap = GRAPHS["star"]
    agg0 = run_matching(g, 0, cap)[0].numpy()
    matched = int(np.nonzero(agg0 == agg0[0])[0][1])
    agg, num, szs, rounds = run_matching(g, 2, cap)
    others = [j for j in range(1, 71) if j != matched]
    members = set(np.nonzero(agg.numpy() == agg[0].item())[0])
    assert members == {0, matched, *others[:3]}
    assert num == 67 and szs.max() == 5
    # distinct weights: the heaviest leaf is matched, the next three join
    g, cap = GRAPHS["star_distinct"]
    wl = g.w.numpy()[:70]
    agg = run_matching(g, 2, cap)[0].numpy()
    heaviest = 1 + np.argsort(-wl)[:4]
    assert set(np.nonzero(agg == agg[0])[0]) == {0, *heaviest}
    # uncapped sweeps: every leaf joins at once
    assert run_matching(g, 1)[1] == 1


def test_path_round_loop_exits():
    g, _ = GRAPHS["path"]
    # exhaustion: one pair per round; round 20 matches the last two rows
    # and the loop ends on "nothing left"
    assert run_matching(g, 0)[3] == 20
    # max_matching_iterations
    res0 = run_matching(g, 0, 3, max_iterations=15)
    assert res0[3] == 15 and res0[1] == 15 + 10
    for merge in (1, 2):
        res = run_matching(g, merge, 3, max_iterations=15)
        check_invariants(g, merge, 3, res, res0, exhausted=False)
    # mode 1 pulls the whole leftover chain 0..9 into the pair (10, 11);
    # mode 2 (cap 3) only row 9
    assert run_matching(g, 1, max_iterations=15)[2].max() == 12
    a2 = run_matching(g, 2, 3, max_iterations=15)
    assert a2[1] == 15 + 9 and a2[2].max() == 3
    # max_unassigned_percentage: 40 -> 18 < 0.5 * 40 after 11 rounds
    assert run_matching(g, 0, max_unassigned=0.5)[3] == 11
    assert run_matching(g, 0, max_iterations=0)[1] == 40


@pytest.mark.parametrize("nx", [8, 16])
def test_uniform_weights_make_progress(nx):
    """The pair hash breaks the ties of a uniform-weight graph: rounds stay
    below the default max_matching_iterations = 15 when run to exhaustion."""
    g = poisson_graph(nx)
    agg, num, szs, rounds = run_matching(g, 2, 3)
    assert rounds < 15 and num < g.n and szs.max() <= 3


# ======================================================================= driver
def scope(**kw):
    node = {"selector": "MULTI_PAIRWISE", "min_coarse_rows": 2}
    node.update(kw)
    return ConfigScope(None, node)


@pytest.mark.parametrize("full_ghost", [0, 1])
@MERGE
def test_passes_compose(merge, full_ghost):
    A = poisson_3d(8, 8, 8)
    sc = scope(aggregation_passes=3, merge_singletons=merge,
               full_ghost_level=full_ghost)
    agg, num, levels = multi_pairwise_passes(A, sc, return_levels=True)
    assert len(levels) == 3
    composed = levels[0][0].long()
    n = A.n_rows
    for level_agg, lnum, sizes, rounds in levels:
        assert lnum < n and sizes.sum() == A.n_rows
        if merge == 2:
            assert sizes.max() <= 10       # 2^3 + 3 - 3/2
        n = lnum
    for level_agg, *_ in levels[1:]:
        composed = level_agg.long()[composed]
    assert torch.equal(composed.to(torch.int32), agg)
    assert num == levels[-1][1] == int(agg.max()) + 1
    assert torch.equal(torch.bincount(agg.long()).to(torch.int32),
                       levels[-1][2])
    agg2, num2 = multi_pairwise_passes(A, sc)
    assert num2 == num and torch.equal(agg2, agg)


@pytest.mark.parametrize("passes,cap", [(1, 3), (2, 5), (3, 10), (4, 18)])
def test_cap_of_the_pass_count(passes, cap):
    A = poisson_3d(8, 8, 8)
    sc = scope(aggregation_passes=passes, merge_singletons=2)
    _, _, levels = multi_pairwise_passes(A, sc, return_levels=True)
    assert levels[-1][2].max() <= cap
    # the cap binds: without it mode 1 builds larger aggregates
    sc1 = scope(aggregation_passes=passes, merge_singletons=1)
    assert multi_pairwise_passes(A, sc1, return_levels=True)[2][-1][2].max() \
        > cap or passes == 1


def test_pass_count_from_aggregate_size():
    A = poisson_3d(8, 8, 8)
    for size, passes in ((2, 1), (4, 2), (8, 3), (5, 3)):
        levels = multi_pairwise_passes(A, scope(aggregate_size=size),
                                       return_levels=True)[2]
        assert len(levels) == passes


@pytest.mark.parametrize("full_ghost", [0, 1])
def test_early_stops(full_ghost):
    kw = dict(aggregation_passes=3, full_ghost_level=full_ghost)
    A = poisson_3d(8, 8, 8)
    # num <= min_coarse_rows
    lv = multi_pairwise_passes(A, scope(min_coarse_rows=400, **kw),
                               return_levels=True)[2]
    assert len(lv) == 1
    # one aggregate left
    E = CSRMatrix(torch.tensor([0, 2, 4], dtype=torch.int32),
                  torch.tensor([0, 1, 0, 1], dtype=torch.int32),
                  torch.tensor([2.0, -1.0, -1.0, 2.0], dtype=torch.float64))
    agg, num, lv = multi_pairwise_passes(E, scope(min_coarse_rows=0, **kw),
                                         return_levels=True)
    assert len(lv) == 1 and num == 1 and agg.tolist() == [0, 0]
    # a pass that coarsens nothing: no edges at all
    D = CSRMatrix(torch.arange(6, dtype=torch.int32),
                  torch.arange(5, dtype=torch.int32),
                  torch.ones(5, dtype=torch.float64))
    agg, num, lv = multi_pairwise_passes(D, scope(**kw), return_levels=True)
    assert len(lv) == 1 and num == 5 and agg.tolist() == [0, 1, 2, 3, 4]


# ================================================================ host selector
def _greedy_yardstick(M):
    """The sequential greedy matcher of select_multi_pairwise, copied."""
    from amgx_amd.ops.cpu import _strength_weights
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


@pytest.mark.parametrize("kw", [dict(aggregate_size=4),
                                dict(aggregation_passes=1,
                                     merge_singletons=2),
                                dict(aggregate_size=8, serial_matching=1)])
def test_host_selector_is_the_greedy_matcher(kw):
    A = poisson_3d(8, 8, 8)
    passes = kw.get("aggregation_passes") or \
        int(np.ceil(np.log2(kw["aggregate_size"])))
    agg, num = _greedy_yardstick(A)
    work, level = A, agg
    for _ in range(passes - 1):
        work = ops.galerkin_aggregation(work, level, num)
        level, num = _greedy_yardstick(work)
        agg = level[agg.long()]
    got, gnum = select_multi_pairwise(A, scope(**kw))
    assert gnum == num and torch.equal(got, agg)
