"""numpy replays of the device setup rules, and checks of the replays.

The host colouring and matching of ``ops/cpu.py`` use other hashes, so they are
no bitwise oracles of the kernels in ``csrc/kernels_setup.hip``. The replays
below follow the device rules literally, row by row, on frozen snapshots; they
are written for reading. ``tests/test_gpu_setup_paths.py`` compares the
kernels with them exactly. This file checks the replays themselves: the
colouring is a valid distance-1 colouring, the matching is a partition with
aggregates of the expected sizes, and a round added after termination changes
nothing.

Matching replays hold only on graphs whose edge weights are all bit-equal
(symmetric structure, one diagonal value, one off-diagonal value), where the
rounding of ``rsqrt`` cannot enter and ties are decided by the hash alone."""

import numpy as np
import pytest

from amgx_amd.ops.cpu import _hash_u32

_U32 = 0xFFFFFFFF
MATCH_SEED_OFFSET = 0x9E3779B1      # ops.size2_matching adds it to its seed


# ====================================================================== graphs
class Graph:
    """CSR structure of n rows and n_cols >= n columns, columns ascending in
    each row; columns j >= n are halo columns."""

    def __init__(self, n, rows, n_cols=None):
        self.n = n
        self.n_cols = n if n_cols is None else n_cols
        self.rows = [sorted(set(r)) for r in rows]
        assert len(self.rows) == n
        self.ro = np.zeros(n + 1, dtype=np.int32)
        self.ro[1:] = np.cumsum([len(r) for r in self.rows])
        self.ci = np.array([j for r in self.rows for j in r], dtype=np.int32)

    def neighbors(self, i):
        """local columns of row i other than i"""
        return [j for j in self.rows[i] if j != i and j < self.n]


def _symmetric(n, edges, diag=True, n_cols=None, halo=()):
    rows = [[i] if diag else [] for i in range(n)]
    for i, j in edges:
        if i != j:
            rows[i].append(j)
            rows[j].append(i)
    for i, j in halo:
        rows[i].append(j)
    return Graph(n, rows, n_cols)


def chord_graph(n, seed=None):
    """a path 0-1-...-(n-1) plus about n/3 random chords"""
    rng = np.random.default_rng(n if seed is None else seed)
    edges = [(i, i + 1) for i in range(n - 1)]
    if n > 3:
        for _ in range(n // 3):
            i, j = rng.integers(0, n, 2)
            edges.append((int(i), int(j)))
    return _symmetric(n, edges)


def path_graph(n):
    return _symmetric(n, [(i, i + 1) for i in range(n - 1)])


def clique_graph(n):
    return _symmetric(n, [(i, j) for i in range(n) for j in range(i)])


def special_graph(diag_everywhere):
    """Isolated rows (empty, or the diagonal alone), self loops and halo
    columns. With ``diag_everywhere`` every row has its diagonal, which the
    uniform-weight matching needs."""
    n = 70
    edges = [(i, i + 1) for i in range(10, 40)] + [(45, 60), (46, 60),
                                                   (47, 60), (50, 69)]
    g = _symmetric(n, edges, diag=diag_everywhere, n_cols=n + 5,
                   halo=[(12, 70), (12, 74), (45, 71), (3, 72), (69, 73)])
    if not diag_everywhere:
        rows = [list(r) for r in g.rows]
        for i in (0, 1, 15, 16, 60):    # rows 0, 1: the diagonal alone
            rows[i].append(i)
        g = Graph(n, rows, n + 5)
    return g


SIZES = [1, 63, 64, 65, 255, 256, 257, 513]


def coloring_graphs():
    gs = {f"chords-{n}": chord_graph(n) for n in SIZES}
    gs["path-600"] = path_graph(600)
    gs["special"] = special_graph(False)
    gs["clique-64"] = clique_graph(64)
    gs["clique-66"] = clique_graph(66)
    return gs


def matching_graphs():
    gs = {f"chords-{n}": chord_graph(n) for n in SIZES}
    gs["path-600"] = path_graph(600)
    gs["special"] = special_graph(True)
    gs["clique-64"] = clique_graph(64)
    gs["clique-66"] = clique_graph(66)
    return gs


# ==================================================================== colouring
def color_key(i, seed):
    return (_hash_u32(i, seed & _U32) << 32) | i


def color_round(g, colors, r, seed=0):
    """Round r on the frozen snapshot ``colors`` -> (next colours, whether a
    row stays uncoloured)."""
    s = seed + 7919 * r
    nxt = list(colors)
    left = False
    for i in range(g.n):
        if colors[i] >= 0:
            continue
        nb = g.neighbors(i)
        mine = color_key(i, s)
        if any(colors[j] < 0 and color_key(j, s) > mine for j in nb):
            left = True
            continue
        used = {colors[j] for j in nb if colors[j] >= 0}
        c = 0
        while c < 64 and c in used:
            c += 1
        if c == 64:     # past the bitmask: above every colour in use
            c = max(max(used), 63) + 1
        nxt[i] = c
    return nxt, left


def replay_coloring(g, seed=0, extra_rounds=0, max_rounds=4096):
    """-> (colours int32, rounds run up to the one that left no row)"""
    colors = [-1] * g.n
    rounds = 0
    left = g.n > 0
    while left:
        assert rounds < max_rounds
        colors, left = color_round(g, colors, rounds, seed)
        rounds += 1
    for r in range(extra_rounds):
        colors, _ = color_round(g, colors, rounds + r, seed)
    return np.array(colors, dtype=np.int32), rounds


# ===================================================================== matching
def match_round(g, agg, seed):
    """One handshake round in place -> whether a pair was formed. Every
    weight is equal: a row proposes to the unaggregated neighbour with the
    largest (hash_u32(j, seed), j)."""
    s = seed & _U32
    prop = [-1] * g.n
    for i in range(g.n):
        if agg[i] >= 0:
            continue
        cand = [j for j in g.neighbors(i) if agg[j] < 0]
        if cand:
            prop[i] = max(cand, key=lambda j: (_hash_u32(j, s), j))
    changed = False
    for i in range(g.n):
        j = prop[i]
        if j >= 0 and prop[j] == i and i < j:
            agg[i] = agg[j] = i     # the root is the smaller partner
            changed = True
    return changed


def merge_singletons(g, agg):
    """agg_singleton_kernel on a frozen snapshot: a leftover row joins the
    aggregated neighbour with the largest root (equal weights), or stays
    alone."""
    out = list(agg)
    for i in range(g.n):
        if agg[i] >= 0:
            continue
        roots = [agg[j] for j in g.neighbors(i) if agg[j] >= 0]
        out[i] = max(roots) if roots else i
    return out


def replay_matching(g, seed=0, max_iters=15, extra_rounds=0):
    """-> (roots int32, rounds run, whether a round formed no pair, which
    ends the handshake, before max_iters cut it off)"""
    s = seed + MATCH_SEED_OFFSET
    agg = [-1] * g.n
    rounds, ended = 0, False
    while rounds < max_iters and not ended:
        rounds += 1
        ended = not match_round(g, agg, s)
    for _ in range(extra_rounds):
        match_round(g, agg, s)
    return np.array(merge_singletons(g, agg), dtype=np.int32), rounds, ended


def renumber(roots):
    """(agg int32, num): consecutive ids in ascending root order"""
    uniq, inv = np.unique(roots, return_inverse=True)
    return inv.astype(np.int32).reshape(-1), int(uniq.size)


# ======================================================================== tests
COLORING = coloring_graphs()
MATCHING = matching_graphs()


@pytest.mark.parametrize("name", list(COLORING))
def test_coloring_replay_is_valid(name):
    g = COLORING[name]
    colors, rounds = replay_coloring(g)
    assert colors.shape == (g.n,) and (colors >= 0).all()
    for i in range(g.n):
        assert all(colors[j] != colors[i] for j in g.neighbors(i)), i
    # greedy: a row's colour is at most its number of neighbours
    assert all(colors[i] <= len(g.neighbors(i)) for i in range(g.n))
    again, _ = replay_coloring(g, extra_rounds=3)
    assert np.array_equal(again, colors)


def test_coloring_replay_cliques_and_rounds():
    for n in (64, 66):
        colors, rounds = replay_coloring(COLORING[f"clique-{n}"])
        assert sorted(colors.tolist()) == list(range(n)) and rounds == n
    # The cliques take one round per row, so they cross every batch size of
    # the device loop. The path takes few: its rows are re-hashed every round.
    assert replay_coloring(COLORING["path-600"])[1] > 3
    colors, _ = replay_coloring(COLORING["special"])
    assert colors[0] == 0 and colors[5] == 0    # isolated rows


def test_coloring_fallback_past_the_bitmask():
    """A winner whose coloured neighbours hold exactly colours 0..63 takes
    64, not 0."""
    g = clique_graph(65)
    colors = list(range(64)) + [-1]
    nxt, left = color_round(g, colors, 0)
    assert nxt[64] == 64 and not left
    colors = list(range(63)) + [70, -1]     # 0..62 and 70: 63 is free
    assert color_round(g, colors, 0)[0][64] == 63
    g = clique_graph(66)
    colors = list(range(64)) + [70, -1]
    assert color_round(g, colors, 0)[0][65] == 71


@pytest.mark.parametrize("name", list(MATCHING))
def test_matching_replay_is_a_partition(name):
    g = MATCHING[name]
    roots, rounds, ended = replay_matching(g)
    # a clique forms one pair per round: max_iters cuts it off
    assert ended == (not name.startswith("clique")) and rounds <= 15
    agg, num = renumber(roots)
    assert agg.shape == (g.n,)
    assert sorted(set(agg.tolist())) == list(range(num))
    assert all(roots[roots[i]] == roots[i] for i in range(g.n))
    for a in range(num):
        members = np.nonzero(agg == a)[0].tolist()
        root = int(roots[members[0]])
        assert root in members and all(roots[m] == root for m in members)
        if len(members) == 1:
            # alone only without a neighbour
            assert not g.neighbors(root)
            continue
        # the root's partner is its neighbour; every further member is a
        # leftover row next to a member
        assert any(j in g.neighbors(root) for j in members)
        for m in members:
            assert any(q in members for q in g.neighbors(m))
    if ended:
        again = replay_matching(g, extra_rounds=3)[0]
        assert np.array_equal(again, roots)


def test_matching_replay_sizes():
    roots = replay_matching(MATCHING["path-600"])[0]
    sizes = np.bincount(renumber(roots)[0])
    # a pair on a path can take a leftover row at either end
    assert sizes.min() >= 2 and sizes.max() <= 4
    roots = replay_matching(MATCHING["special"])[0]
    sizes = np.bincount(renumber(roots)[0])
    assert (sizes == 1).sum() == sum(
        1 for i in range(70) if not MATCHING["special"].neighbors(i))
    assert replay_matching(Graph(1, [[0]]))[0].tolist() == [0]
