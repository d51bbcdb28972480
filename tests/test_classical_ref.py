"""Per-row references of the classical AMG setup operations, the matrices
that exercise their branches, and the host backend checked against them.

The references are plain float64 loops over the rows, written from the
formulas documented in ``csrc/kernels_classical.hip`` and ``ops/cpu.py``;
they share no code with either. ``tests/test_gpu_classical.py`` imports them
to check the device kernels.

Every matrix entry is a small integer or a dyadic fraction, so row sums,
lumped diagonals and each ``== 0`` decision are exact in fp64 and in fp32;
the only rounding left in an interpolation weight is its final multiply and
divide.
"""

import math
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from amgx_amd import CSRMatrix
from amgx_amd.ops import cpu as cpu_ops
from amgx_amd.problems import poisson_2d, poisson_3d


# ===================================================================== matrices
class Mat(SimpleNamespace):
    """CSR arrays of one test matrix: ro, ci (sorted, unique per row), va
    (float64), n rows, ncols >= n columns (the surplus are halo columns)."""

    def csr(self, dtype=torch.float64, device="cpu"):
        A = CSRMatrix(torch.from_numpy(self.ro.astype(np.int32)),
                      torch.from_numpy(self.ci.astype(np.int32)),
                      torch.from_numpy(self.va).to(dtype), n_cols=self.ncols)
        return A.to(device)


def _from_rows(rows, n, ncols=None):
    ro = np.zeros(n + 1, dtype=np.int64)
    ci, va = [], []
    for i in range(n):
        for c in sorted(rows[i]):
            ci.append(c)
            va.append(float(rows[i][c]))
        ro[i + 1] = len(ci)
    return Mat(ro=ro, ci=np.asarray(ci, dtype=np.int64),
               va=np.asarray(va, dtype=np.float64), n=n,
               ncols=n if ncols is None else ncols)


def from_csr_matrix(A):
    return Mat(ro=A.row_offsets.numpy().astype(np.int64),
               ci=A.col_indices.numpy().astype(np.int64),
               va=A.values.numpy().astype(np.float64), n=A.n_rows,
               ncols=A.n_cols)


# planted rows r (all r % 3 == 1, so under the every-third-row split r is F
# and r - 1 is C). Each has one strong entry -8 to r - 1 and weak positives
# +1, so no positive is ever a strong C connection and the positives are
# lumped: diagonal -3 + 3 = 0 (lumped to zero), stored 0 + 2 (rescued),
# missing + 2 (rescued, no diagonal entry).
LUMPED_ZERO = (7, 67, 127, 187)
RESCUED_ZERO = (22, 82, 142, 202)
RESCUED_MISSING = (37, 97, 157, 217)
THRESHOLD = (52, 112)           # -4, -1, -1: the -1 sit on 0.25 * 4
_PLANTED = LUMPED_ZERO + RESCUED_ZERO + RESCUED_MISSING + THRESHOLD
_HUB_FANS = 8                   # rows r+1..r+8 depend on r-1: a likely C point


def signed_random_rows(n, seed):
    rng = np.random.RandomState(seed)
    vals = np.array([-4, -2, -1, 1, 2, 0])
    prob = np.array([0.25, 0.25, 0.2, 0.1, 0.1, 0.1])
    rows = [dict() for _ in range(n)]
    for i in range(n):
        rows[i][i] = int(rng.choice([-12, -3, 3, 5, 8, 20]))
        if n == 1:
            break
        for t in range(rng.randint(3, 6)):
            if t % 2:
                j = int(rng.randint(n))
            else:
                j = (i + int(rng.randint(-10, 11))) % n
            if j == i:
                continue
            rows[i][j] = int(rng.choice(vals, p=prob))
            if rng.rand() < 0.5 and i not in rows[j]:
                rows[j][i] = int(rng.choice(vals, p=prob))
    planted = [r for r in _PLANTED if r + _HUB_FANS < n]
    guarded = set()
    for r in planted:
        guarded.update(range(r - 1, r + _HUB_FANS + 1))
    free = [i for i in range(n) if i not in guarded and n > 1]
    for t, i in enumerate(free[4::9]):      # every ninth free row, in turn:
        if t % 4 == 0:
            del rows[i][i]                  # missing diagonal
        elif t % 4 == 1:
            rows[i][i] = 0                  # stored zero diagonal
        elif t % 4 == 2:
            rows[i] = {}                    # empty row
        else:
            rows[i] = {i: rows[i][i]}       # diagonal only
    for r in planted:
        if r in LUMPED_ZERO:
            rows[r] = {r - 1: -8, r: -3, r + 1: 1, r + 2: 1, r + 3: 1}
        elif r in RESCUED_ZERO:
            rows[r] = {r - 1: -8, r: 0, r + 1: 1, r + 2: 1}
        elif r in RESCUED_MISSING:
            rows[r] = {r - 1: -8, r + 1: 1, r + 2: 1}
        else:
            rows[r] = {r - 1: -4, r: 6, r + 1: -1, r + 2: -1}
        for d in range(1, _HUB_FANS + 1):
            rows[r + d][r - 1] = -4
    return rows


def signed_random(n, seed):
    return _from_rows(signed_random_rows(n, seed), n)


N_HALO = 9


def with_halo(n, seed):
    """signed_random(n, seed) with N_HALO extra columns, as a rank of the
    distributed path sees its matrix."""
    rows = signed_random_rows(n, seed)
    rng = np.random.RandomState(seed + 1000)
    guarded = {r + d for r in _PLANTED for d in range(-1, 1)}
    for i in range(n):
        if i in guarded or not rows[i] or rng.rand() > 0.3:
            continue
        rows[i][n + int(rng.randint(N_HALO))] = int(rng.choice([-4, -2, 1, 2]))
    return _from_rows(rows, n, n + N_HALO)


def halo_cf(cf_local, nc):
    """cf over all columns: the local split, then 'global' coarse ids on two
    of every three halo columns."""
    halo = np.array([nc + 5 * h + 2 if h % 3 != 2 else -1
                     for h in range(N_HALO)], dtype=np.int64)
    return np.concatenate([np.asarray(cf_local, dtype=np.int64), halo])


def dominant_signed(n, seed):
    """The signed_random pattern and off-diagonals under a diagonal of
    16 + sum|a_ij|: every positive off-diagonal (at most 2) is at most 1/8
    of it and no interpolation denominator comes near zero."""
    rows = signed_random_rows(n, seed)
    for i in range(n):
        off = sum(abs(v) for c, v in rows[i].items() if c != i)
        rows[i][i] = 16 + off
    return _from_rows(rows, n)


def poisson(nx, ny):
    return from_csr_matrix(poisson_2d(nx, ny))


def pmis_hash(i):
    """The integer hash of the PMIS kernels, in uint32 arithmetic."""
    m = 0xFFFFFFFF
    a = np.asarray(i, dtype=np.uint64)
    a = (a ^ np.uint64(61)) ^ (a >> np.uint64(16))
    a = (a * np.uint64(9)) & np.uint64(m)
    a = a ^ (a >> np.uint64(4))
    a = (a * np.uint64(0x27d4eb2d)) & np.uint64(m)
    a = a ^ (a >> np.uint64(15))
    return a.astype(np.uint32)


def hash_tie_pair():
    """First i < j whose hashes agree in the 16 bits the weights use."""
    seen = {}
    j = 0
    while True:
        h = int(pmis_hash(j)) & 0xffff
        if h in seen:
            return seen[h], j
        seen[h] = j
        j += 1


def hash_tie():
    i, j = hash_tie_pair()
    rows = [{r: 2} for r in range(j + 1)]
    rows[i][j] = -1
    rows[j][i] = -1
    return _from_rows(rows, j + 1)


def staircase(K):
    """Path of K nodes; path node k also carries k pendant leaves. All
    off-diagonals -1. lambda grows along the path, so PMIS decides two path
    nodes a round from the far end: K / 2 rounds."""
    n = K + K * (K - 1) // 2
    rows = [dict() for _ in range(n)]
    leaf = K
    for k in range(K):
        if k + 1 < K:
            rows[k][k + 1] = -1
            rows[k + 1][k] = -1
        for _ in range(k):
            rows[k][leaf] = -1
            rows[leaf][k] = -1
            leaf += 1
    for i in range(n):
        rows[i][i] = len(rows[i])
    return _from_rows(rows, n)


_ZOO = {
    "signed1": lambda: signed_random(1, 11),
    "signed255": lambda: signed_random(255, 12),
    "signed256": lambda: signed_random(256, 13),
    "signed257": lambda: signed_random(257, 14),
    "signed777": lambda: signed_random(777, 15),
    "halo257": lambda: with_halo(257, 16),
    "poisson17x19": lambda: poisson(17, 19),
    "hash_tie": hash_tie,
    "staircase100": lambda: staircase(100),
    "staircase140": lambda: staircase(140),
}
ZOO_NAMES = list(_ZOO)
# D2 / MULTIPASS parity matrices, outside the zoo of the per-kernel tests
_ZOO["poisson5x6x4"] = lambda: from_csr_matrix(poisson_3d(5, 6, 4))
_ZOO["dominant257"] = lambda: dominant_signed(257, 14)
D2_NAMES = ["poisson5x6x4", "dominant257"]
# the matrices that carry the planted rows
SIGNED_NAMES = ["signed255", "signed256", "signed257", "signed777", "halo257"]
STRENGTH_PARAMS = [(0.25, 1.1), (0.25, 0.9), (0.5, 0.9)]
_zoo_cache = {}


def zoo(name):
    """Test matrices are built once and never modified."""
    if name not in _zoo_cache:
        _zoo_cache[name] = _ZOO[name]()
    return _zoo_cache[name]


# =================================================================== references
def ref_strength(ro, ci, va, theta, max_row_sum):
    """AHAT: strong iff off-diagonal, max_{k!=i}|a_ik| > 0 and
    |a_ij| >= theta * that max; a row is all weak when max_row_sum < 1 and
    |row sum| > max_row_sum * |a_ii| (|a_ii| = 1 where missing or zero)."""
    n = len(ro) - 1
    strong = np.zeros(len(ci), dtype=bool)
    for i in range(n):
        mx, rs, diag = 0.0, 0.0, None
        for k in range(ro[i], ro[i + 1]):
            a = float(va[k])
            rs += a
            if ci[k] != i:
                mx = max(mx, abs(a))
            elif diag is None:
                diag = a
        weak = False
        if max_row_sum < 1.0:
            d = abs(diag) if diag else 1.0
            weak = abs(rs) > max_row_sum * d
        if weak or mx == 0.0:
            continue
        for k in range(ro[i], ro[i + 1]):
            if ci[k] != i and abs(float(va[k])) >= theta * mx:
                strong[k] = True
    return strong


def ref_trans_index(ro, ci, n):
    """For entry k = (i, j): the index of entry (j, i), or -1 where there is
    none or j >= n."""
    out = np.full(len(ci), -1, dtype=np.int64)
    for i in range(n):
        for k in range(ro[i], ro[i + 1]):
            j = ci[k]
            if j >= n:
                continue
            for t in range(ro[j], ro[j + 1]):
                if ci[t] == i:
                    out[k] = t
                    break
    return out


def ref_d1(ro, ci, va, strong, cf, n):
    """Direct interpolation with pos/neg splitting. For an F row i with
    strong C entries: w_ij = -alpha a_ij / d (a_ij < 0), -beta a_ij / d
    (a_ij >= 0), alpha = sum(neg off-diagonals) / sum(neg strong C), beta
    likewise; where the row has no positive strong C entry its positives are
    lumped into d = a_ii + sum(pos) and beta is unused. A row whose d is zero
    AFTER lumping gets no entries. C rows: one entry 1 at their coarse id.

    Returns (P triplets (rows, cols, vals), the strong-C counts of the count
    pass (1 on C rows), a dict of row classes -> list of F rows)."""
    cf = np.asarray(cf)
    pr, pc, pv = [], [], []
    counts = np.zeros(n, dtype=np.int64)
    cls = {k: [] for k in ("pos_c", "lump", "no_strong_c", "lumped_zero",
                           "rescued", "missing_diag", "strong_halo")}
    for i in range(n):
        if cf[i] >= 0:
            pr.append(i); pc.append(int(cf[i])); pv.append(1.0)
            counts[i] = 1
            continue
        diag, has_diag = 0.0, False
        neg_all = pos_all = neg_c = pos_c = 0.0
        sc = []
        for k in range(ro[i], ro[i + 1]):
            j, a = ci[k], float(va[k])
            if j == i:
                if not has_diag:
                    diag, has_diag = a, True
                continue
            if a < 0:
                neg_all += a
            else:
                pos_all += a
            if strong[k] and j < len(cf) and cf[j] >= 0:
                sc.append(k)
                if a < 0:
                    neg_c += a
                else:
                    pos_c += a
        counts[i] = len(sc)
        if not sc:
            cls["no_strong_c"].append(i)
            continue
        d = diag
        if pos_c == 0.0:
            d = diag + pos_all
            if pos_all > 0.0:
                cls["lump"].append(i)
                if diag != 0.0 and d == 0.0:
                    cls["lumped_zero"].append(i)
        else:
            cls["pos_c"].append(i)
        if diag == 0.0 and d != 0.0:
            cls["rescued"].append(i)
        if not has_diag:
            cls["missing_diag"].append(i)
        if any(ci[k] >= n for k in sc):
            cls["strong_halo"].append(i)
        if d == 0.0:
            continue
        alpha = neg_all / neg_c if neg_c != 0.0 else 0.0
        beta = pos_all / pos_c if pos_c != 0.0 else 0.0
        for k in sc:
            a = float(va[k])
            pr.append(i); pc.append(int(cf[ci[k]]))
            pv.append(-(alpha if a < 0 else beta) * a / d)
    return (np.asarray(pr, dtype=np.int64), np.asarray(pc, dtype=np.int64),
            np.asarray(pv)), counts, cls


def ref_truncate(ro, ci, va, factor, max_elements):
    """Keep |v| >= factor * rowmax; of those at most max_elements (>= 0),
    the first in (|v| descending, position ascending) order; rescale the
    kept entries to the old row sum unless either sum is zero."""
    n = len(ro) - 1
    o_ro, o_ci, o_va = [0], [], []
    for i in range(n):
        ks = list(range(ro[i], ro[i + 1]))
        if ks:
            mx = max(abs(float(va[k])) for k in ks)
            old = 0.0
            for k in ks:
                old += float(va[k])
            keep = [k for k in ks if abs(float(va[k])) >= factor * mx]
            if 0 <= max_elements < len(keep):
                keep = sorted(keep, key=lambda k: (-abs(float(va[k])), k))
                keep = sorted(keep[:max_elements])
            new = 0.0
            for k in keep:
                new += float(va[k])
            scale = old / new if (new != 0.0 and old != 0.0) else 1.0
            for k in keep:
                o_ci.append(int(ci[k]))
                o_va.append(float(va[k]) * scale)
        o_ro.append(len(o_ci))
    return (np.asarray(o_ro, dtype=np.int64),
            np.asarray(o_ci, dtype=np.int64), np.asarray(o_va))


def strong_edges(ro, ci, strong, n):
    """Directed edge list (both directions) of S union S^T among the n
    local points, by a plain loop."""
    nb = [set() for _ in range(n)]
    for i in range(n):
        for k in range(ro[i], ro[i + 1]):
            j = int(ci[k])
            if strong[k] and j != i and j < n:
                nb[i].add(j)
                nb[j].add(i)
    return nb


def emulate_pmis(ro, ci, strong, n):
    """The device PMIS replayed in numpy. Graph: S union S^T among the local
    points. w_i = float32(lambda_i) + float32(hash(i) & 0xffff) / 65536 with
    lambda_i = #{j : (j, i) strong}; isolated points are F; a round decides
    against a frozen snapshot: undecided points that no undecided neighbour
    beats under (w, then larger index) become C, then undecided neighbours of
    C become F; rounds run to completion.

    Returns (cf int32 with coarse ids in row order, nc, rounds, lambda)."""
    nb = strong_edges(ro, ci, strong, n)
    lam = np.zeros(n, dtype=np.int64)
    for i in range(n):
        for k in range(ro[i], ro[i + 1]):
            if strong[k] and ci[k] != i and ci[k] < n:
                lam[ci[k]] += 1
    er = np.asarray([i for i in range(n) for _ in nb[i]], dtype=np.int64)
    ec = np.asarray([j for i in range(n) for j in sorted(nb[i])],
                    dtype=np.int64)
    frac = (pmis_hash(np.arange(n)) & np.uint32(0xffff)).astype(np.float32)
    w = lam.astype(np.float32) + frac / np.float32(65536.0)
    assert w.dtype == np.float32
    state = np.zeros(n, dtype=np.int8)
    deg = np.asarray([len(s) for s in nb], dtype=np.int64)
    state[deg == 0] = -1
    rounds = 0
    while (state == 0).any():
        rounds += 1
        assert rounds <= n + 1
        und = state == 0
        live = und[er] & und[ec]
        beats = (w[ec] > w[er]) | ((w[ec] == w[er]) & (ec > er))
        beaten = np.zeros(n, dtype=bool)
        beaten[er[live & beats]] = True
        state[und & ~beaten] = 1
        hit = (state[er] == 0) & (state[ec] == 1)
        state[er[hit]] = -1
    cf = np.full(n, -1, dtype=np.int32)
    c_rows = np.nonzero(state == 1)[0]
    cf[c_rows] = np.arange(c_rows.size, dtype=np.int32)
    return cf, int(c_rows.size), rounds, lam


def check_pmis_invariants(ro, ci, strong, n, cf):
    """The four properties of a PMIS split, each with its own message."""
    cf = np.asarray(cf)
    assert cf.shape == (n,)
    nb = strong_edges(ro, ci, strong, n)
    for i in range(n):
        if cf[i] >= 0:
            bad = [j for j in nb[i] if cf[j] >= 0]
            assert not bad, f"independence: C points {i} and {bad[0]} adjacent"
        elif nb[i]:
            assert any(cf[j] >= 0 for j in nb[i]), \
                f"maximality: F point {i} has edges but no C neighbour"
        if not nb[i]:
            assert cf[i] < 0, f"isolated point {i} is not F"
    c_rows = np.nonzero(cf >= 0)[0]
    assert (cf[c_rows] == np.arange(c_rows.size)).all(), \
        "coarse ids are not 0..nc-1 in row order"


def every_third(n):
    cf = np.full(n, -1, dtype=np.int64)
    cf[::3] = np.arange(len(cf[::3]))
    return cf, len(cf[::3])


_split_cache = {}


def splits(name):
    """{split name: (S at theta 0.25 / max_row_sum 1.1, cf over all columns,
    number of P columns)} for a zoo matrix; computed once."""
    if name in _split_cache:
        return _split_cache[name]
    m = zoo(name)
    S = ref_strength(m.ro, m.ci, m.va, 0.25, 1.1)
    out = {}
    cf_p, nc_p, _, _ = emulate_pmis(m.ro, m.ci, S, m.n)
    for key, (cf, nc) in (("pmis", (cf_p, nc_p)),
                          ("third", every_third(m.n))):
        if m.ncols > m.n:
            cf = halo_cf(cf, nc)
            nc = int(cf.max()) + 1
        out[key] = (S, np.asarray(cf, dtype=np.int64), nc)
    _split_cache[name] = out
    return out


_d1_cache = {}


def d1_reference(name, split):
    """(S, cf, P columns, canonical reference P, count-pass counts, row
    classes) of ref_d1 for a zoo matrix and split; computed once."""
    key = (name, split)
    if key not in _d1_cache:
        m = zoo(name)
        S, cf, nc = splits(name)[split]
        trip, counts, cls = ref_d1(m.ro, m.ci, m.va, S, cf, m.n)
        _d1_cache[key] = (S, cf, nc, p_matrix(trip, m.n, nc), counts, cls)
    return _d1_cache[key]


def p_matrix(trip, n, ncols):
    """Canonical scipy CSR of P without explicit zeros."""
    r, c, v = trip
    P = sp.csr_matrix((v, (r, c)), shape=(n, ncols))
    P.sum_duplicates()
    P.sort_indices()
    P.eliminate_zeros()
    return P


def csr_matrix_to_p(P):
    """A CSRMatrix (rows may be unsorted and hold explicit zeros) as
    canonical scipy CSR in float64."""
    m = sp.csr_matrix((P.values.cpu().numpy().astype(np.float64).ravel(),
                       P.col_indices.cpu().numpy(),
                       P.row_offsets.cpu().numpy()),
                      shape=(P.n_rows, P.n_cols))
    m.sum_duplicates()
    m.sort_indices()
    m.eliminate_zeros()
    return m


def assert_same_p(P, P_ref, rtol, atol):
    assert P.shape == P_ref.shape
    assert np.isfinite(P.data).all()
    assert np.array_equal(P.indptr, P_ref.indptr)
    assert np.array_equal(P.indices, P_ref.indices)
    np.testing.assert_allclose(P.data, P_ref.data, rtol=rtol, atol=atol)


# a P full of ties for the truncation tests: values from {+-0.25, +-0.5, 1}
TRUNC_PARAMS = [(0.0, 0), (0.0, 1), (0.0, 3), (0.5, -1), (0.5, 2), (0.999, 1)]


def tie_matrix():
    if "ties" in _zoo_cache:
        return _zoo_cache["ties"]
    rng = np.random.RandomState(77)
    n, ncols = 300, 40
    vals = np.array([-0.5, -0.25, 0.25, 0.5, 1.0])
    rows = []
    for i in range(n):
        k = int(rng.randint(0, 9))          # empty rows and rows under a cap
        cols = rng.choice(ncols, size=k, replace=False)
        rows.append({int(c): float(rng.choice(vals)) for c in cols})
    rows[3] = {}
    rows[5] = {1: 0.5, 4: -0.25, 9: -0.25}              # sums to zero
    rows[9] = {0: 0.5, 2: -0.5, 7: 0.25, 8: 0.25}       # kept (cap 2) sum to 0
    rows[11] = {2: 0.5, 3: 0.5, 5: 0.5, 6: 0.5, 30: 0.5}   # all tied
    rows[12] = {1: -1.0, 2: 1.0, 3: 0.5}     # cap 1 picks between -1 and 1
    m = _from_rows(rows, n, ncols)
    _zoo_cache["ties"] = m
    return m


# ======================================================================== tests
@pytest.mark.parametrize("theta,mrs", STRENGTH_PARAMS)
@pytest.mark.parametrize("name", ZOO_NAMES)
def test_host_strength_matches_loops(name, theta, mrs):
    m = zoo(name)
    S = cpu_ops.strength_ahat(m.csr(), theta, mrs)
    assert np.array_equal(S.numpy().astype(bool),
                          ref_strength(m.ro, m.ci, m.va, theta, mrs))


@pytest.mark.parametrize("name", SIGNED_NAMES)
def test_strength_branches_are_exercised(name):
    m = zoo(name)
    on = ref_strength(m.ro, m.ci, m.va, 0.25, 1.1)
    cut = ref_strength(m.ro, m.ci, m.va, 0.25, 0.9)
    rows = np.repeat(np.arange(m.n), np.diff(m.ro))
    has = np.zeros(m.n, dtype=bool)
    has[rows[on]] = True
    has_cut = np.zeros(m.n, dtype=bool)
    has_cut[rows[cut]] = True
    assert (has & ~has_cut).any(), "no row made weak by max_row_sum"
    assert has_cut.any(), "max_row_sum 0.9 made every row weak"
    # an entry exactly on the threshold, strong by >=
    equal = False
    for i in range(m.n):
        off = [abs(m.va[k]) for k in range(m.ro[i], m.ro[i + 1])
               if m.ci[k] != i]
        mx = max(off, default=0.0)
        equal |= any(mx > 0 and a == 0.25 * mx for a in off)
    assert equal, "no entry on the threshold"
    for r in THRESHOLD:
        ks = [k for k in range(m.ro[r], m.ro[r + 1]) if m.va[k] == -1.0]
        assert len(ks) == 2 and on[ks].all()
    assert (m.va == 0.0).any() and not on[m.va == 0.0].any()
    assert (on & (m.ci >= m.n)).any() == (m.ncols > m.n)


@pytest.mark.parametrize("name", SIGNED_NAMES)
def test_signed_random_has_its_row_kinds(name):
    m = zoo(name)
    kinds = {"empty": 0, "diag_only": 0, "no_diag": 0, "zero_diag": 0,
             "neg_diag": 0, "pos_diag": 0}
    for i in range(m.n):
        row = {int(m.ci[k]): m.va[k] for k in range(m.ro[i], m.ro[i + 1])}
        assert len(row) == m.ro[i + 1] - m.ro[i]
        assert list(row) == sorted(row)
        if not row:
            kinds["empty"] += 1
        elif list(row) == [i]:
            kinds["diag_only"] += 1
        elif i not in row:
            kinds["no_diag"] += 1
        elif row[i] == 0.0:
            kinds["zero_diag"] += 1
        kinds["neg_diag"] += row.get(i, 0.0) < 0
        kinds["pos_diag"] += row.get(i, 0.0) > 0
    assert all(kinds.values()), kinds
    off = np.diff(m.ro).sum() / m.n - 1
    assert 4.0 < off < 8.0, off
    assert set(np.unique(m.va)) >= {-4.0, -2.0, -1.0, 0.0, 1.0, 2.0}


@pytest.mark.parametrize("name", ZOO_NAMES)
def test_trans_index_reference(name):
    m = zoo(name)
    t = ref_trans_index(m.ro, m.ci, m.n)
    rows = np.repeat(np.arange(m.n), np.diff(m.ro))
    hit = t >= 0
    assert (m.ci[t[hit]] == rows[hit]).all()
    assert (rows[t[hit]] == m.ci[hit]).all()
    assert (t[t[hit]] == np.nonzero(hit)[0]).all()
    if name in SIGNED_NAMES:
        assert (~hit & (m.ci < m.n)).any(), "pattern is symmetric"
        assert hit.any()
    if m.ncols > m.n:
        assert (m.ci >= m.n).any() and not hit[m.ci >= m.n].any()


@pytest.mark.parametrize("name", ZOO_NAMES)
def test_emulated_pmis_is_a_pmis(name):
    m = zoo(name)
    S = ref_strength(m.ro, m.ci, m.va, 0.25, 1.1)
    cf, nc, rounds, lam = emulate_pmis(m.ro, m.ci, S, m.n)
    assert lam.max(initial=0) < 256     # weights exact in fp32
    check_pmis_invariants(m.ro, m.ci, S, m.n, cf)
    assert nc == (cf >= 0).sum()
    if name in SIGNED_NAMES:
        t = ref_trans_index(m.ro, m.ci, m.n)
        assert (S & (t < 0) & (m.ci < m.n)).any(), "S has no one-way edge"


@pytest.mark.parametrize("name", ZOO_NAMES)
def test_host_pmis_is_a_pmis(name):
    m = zoo(name)
    S = ref_strength(m.ro, m.ci, m.va, 0.25, 1.1)
    cf, nc = cpu_ops.pmis_select(m.csr(), torch.from_numpy(S))
    check_pmis_invariants(m.ro, m.ci, S, m.n, cf.numpy())
    assert nc == int((cf >= 0).sum())


def test_hash_tie_larger_index_wins():
    i, j = hash_tie_pair()
    assert i < j and (int(pmis_hash(i)) ^ int(pmis_hash(j))) & 0xffff == 0
    m = zoo("hash_tie")
    S = ref_strength(m.ro, m.ci, m.va, 0.25, 1.1)
    cf, nc, rounds, lam = emulate_pmis(m.ro, m.ci, S, m.n)
    assert lam[i] == lam[j] == 1
    assert nc == 1 and cf[j] == 0 and cf[i] == -1


@pytest.mark.parametrize("K,rounds", [(100, 50), (140, 70)])
def test_staircase_round_count(K, rounds):
    m = zoo(f"staircase{K}")
    S = ref_strength(m.ro, m.ci, m.va, 0.25, 1.1)
    assert S.sum() == m.ci.size - m.n
    assert emulate_pmis(m.ro, m.ci, S, m.n)[2] == rounds
    # 64 was the device's round cap; the host's guard is far above both
    assert (rounds > 64) == (K == 140)
    assert rounds < 8 * (int(math.log2(m.n + 2)) + 8)


@pytest.mark.parametrize("split", ["pmis", "third"])
@pytest.mark.parametrize("name", ZOO_NAMES)
def test_host_d1_matches_loops(name, split):
    m = zoo(name)
    S, cf, nc, P_ref, counts, cls = d1_reference(name, split)
    P = cpu_ops.interp_d1(m.csr(), torch.from_numpy(S),
                          torch.from_numpy(cf), nc)
    assert_same_p(csr_matrix_to_p(P), P_ref, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("split", ["pmis", "third"])
@pytest.mark.parametrize("name", SIGNED_NAMES)
def test_d1_branches_are_exercised(name, split):
    m = zoo(name)
    S, cf, nc, P_ref, counts, cls = d1_reference(name, split)
    need = ["pos_c", "lump", "no_strong_c", "lumped_zero", "rescued",
            "missing_diag"]
    if m.ncols > m.n:
        need.append("strong_halo")
    for key in need:
        assert cls[key], f"no F row of class {key}"
    assert set(cls["lumped_zero"]) & set(LUMPED_ZERO)
    assert set(cls["rescued"]) & set(RESCUED_ZERO)
    assert set(cls["missing_diag"]) & set(RESCUED_MISSING)
    # degenerate rows keep counted slots but get no entries
    assert all(counts[i] > 0 for i in cls["lumped_zero"])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32],
                         ids=["fp64", "fp32"])
@pytest.mark.parametrize("factor,cap", TRUNC_PARAMS)
def test_host_truncate_matches_loops(factor, cap, dtype):
    m = tie_matrix()
    ro, ci, va = ref_truncate(m.ro, m.ci, m.va, factor, cap)
    T = cpu_ops.truncate_rows(m.csr(dtype), factor, cap)
    assert T.dtype == dtype and T.n_cols == m.ncols
    assert np.array_equal(T.row_offsets.numpy(), ro)
    assert np.array_equal(T.col_indices.numpy(), ci)
    tol = dict(rtol=1e-12, atol=1e-14) if dtype == torch.float64 \
        else dict(rtol=1e-6, atol=0.0)
    np.testing.assert_allclose(T.values.numpy().astype(np.float64), va, **tol)


def test_truncate_branches_are_exercised():
    m = tie_matrix()
    deg = np.diff(m.ro)
    assert (deg == 0).any() and ((deg > 0) & (deg < 3)).any()
    assert (deg > 3).any()
    rows = np.repeat(np.arange(m.n), deg)
    sums = np.bincount(rows, weights=m.va, minlength=m.n)
    assert ((sums == 0.0) & (deg > 0)).any(), "no row sums to zero"
    ro, ci, va = ref_truncate(m.ro, m.ci, m.va, 0.5, 2)
    out_rows = np.repeat(np.arange(m.n), np.diff(ro))
    kept = np.bincount(out_rows, weights=va, minlength=m.n)
    assert ((kept == 0.0) & (np.diff(ro) > 0) & (sums != 0.0)).any(), \
        "no row whose kept entries sum to zero"
    # a cap that cuts through a run of equal magnitudes
    cut = False
    for i in range(m.n):
        a = np.sort(np.abs(m.va[m.ro[i]:m.ro[i + 1]]))[::-1]
        cut |= a.size > 3 and a[2] == a[3]
    assert cut, "no tie across the cap"


@pytest.mark.parametrize("name", D2_NAMES)
def test_d2_multipass_formulations_agree_on_cpu(name):
    """The torch formulations of D2 and MULTIPASS against the scipy ones on
    CPU tensors, signed off-diagonals included (the device run of the same
    comparison is in tests/test_gpu_classical.py)."""
    from amgx_amd.amg.classical import (SELECTOR_REGISTRY, _interp_d2_device,
                                        _interp_d2_host,
                                        _interp_multipass_device,
                                        interp_multipass)
    from amgx_amd.config import ConfigScope
    scope = ConfigScope(None, {"strength_threshold": 0.25})
    m = zoo(name)
    A = m.csr()
    S = torch.from_numpy(ref_strength(m.ro, m.ci, m.va, 0.25, 1.1))
    if name == "dominant257":
        assert (m.va[S.numpy()] > 0).any() and (m.va[S.numpy()] < 0).any()
    cf, nc, _, _ = emulate_pmis(m.ro, m.ci, S.numpy(), m.n)
    cf = torch.from_numpy(cf)
    d = abs(_interp_d2_host(A, S, cf, nc, scope).to_scipy()
            - _interp_d2_device(A, S, cf, nc, scope).to_scipy())
    assert d.nnz == 0 or d.max() < 1e-12
    cf, nc = SELECTOR_REGISTRY["AGGRESSIVE_PMIS"](A, S, scope)
    d = abs(interp_multipass(A, S, cf, nc, scope).to_scipy()
            - _interp_multipass_device(A, S, cf, nc, scope).to_scipy())
    assert d.nnz == 0 or d.max() < 1e-12
