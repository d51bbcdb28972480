"""Shared inputs of tests/test_gpu_sparse_products.py and
tests/test_hash_probe_model.py: exactly representable values, the plain
per-row reference of C = A * B, and the tier-edge matrices whose product rows
sit at and around the table sizes of the LDS hash ladder
(kernels_spgemm.hip: 64 -> 512 -> top cap -> sort fallback).

Values are nonzero integers in [-4, 4] (Gaussian integers for complex) times
2^k, k in {-1, 0, 1}. A triple product of them is a multiple of 1/8 of
modulus at most 8^3 * sqrt(2)^3, and every sum the tests form has fewer than
a thousand terms, so all results stay far below 2^24 units of 1/8: exact in
float32, float64, complex64 and complex128 in any summation order.

The reference pattern is the STRUCTURAL product: column j is stored in row i
as soon as some pair A[i, k], B[k, j] is stored, whatever the values."""

from collections import namedtuple

import numpy as np

Csr = namedtuple("Csr", "ro ci va n_cols")
TierEdge = namedtuple("TierEdge", "A B widths short")
# short rows of the tier-edge matrix the device tests use: enough for the
# average row of the product to send ops.spgemm into the ladder at 64
SHORT_ROWS = 9000


def exact_values(rng, size, cplx=False):
    scale = 2.0 ** rng.randint(-1, 2, size=size)
    nonzero = np.array([-4.0, -3.0, -2.0, -1.0, 1.0, 2.0, 3.0, 4.0])
    if not cplx:
        return rng.choice(nonzero, size=size) * scale
    re = rng.randint(-4, 5, size=size).astype(np.float64)
    im = rng.randint(-4, 5, size=size).astype(np.float64)
    zero = (re == 0) & (im == 0)
    re[zero] = rng.choice(nonzero, size=int(zero.sum()))
    return (re + 1j * im) * scale


def csr_from_rows(cols_per_row, vals_per_row, n_cols, dtype):
    ro = np.zeros(len(cols_per_row) + 1, dtype=np.int64)
    np.cumsum(np.array([len(c) for c in cols_per_row], dtype=np.int64),
              out=ro[1:])
    if ro[-1] == 0:
        return Csr(ro, np.zeros(0, np.int64), np.zeros(0, dtype), n_cols)
    ci = np.concatenate([np.asarray(c, dtype=np.int64)
                         for c in cols_per_row])
    va = np.concatenate([np.asarray(v, dtype=dtype) for v in vals_per_row])
    return Csr(ro, ci, va, n_cols)


def reference_product(A, B):
    """C = A * B row by row in float64 / complex128 on a dense scratch row,
    structural pattern, ascending columns."""
    assert A.n_cols == len(B.ro) - 1
    dtype = np.result_type(A.va.dtype, B.va.dtype, np.float64)
    scratch = np.zeros(B.n_cols, dtype=dtype)
    cols_out, vals_out = [], []
    for i in range(len(A.ro) - 1):
        touched = []
        for k in range(A.ro[i], A.ro[i + 1]):
            s, e = B.ro[A.ci[k]], B.ro[A.ci[k] + 1]
            np.add.at(scratch, B.ci[s:e], A.va[k] * B.va[s:e])
            touched.append(B.ci[s:e])
        cols = (np.unique(np.concatenate(touched)) if touched
                else np.zeros(0, np.int64))
        cols_out.append(cols)
        vals_out.append(scratch[cols])
        scratch[cols] = 0
    return csr_from_rows(cols_out, vals_out, B.n_cols, dtype)


def take_rows(M, rows):
    """The rows `rows` of M, as a new matrix."""
    return csr_from_rows([M.ci[M.ro[i]:M.ro[i + 1]] for i in rows],
                         [M.va[M.ro[i]:M.ro[i + 1]] for i in rows],
                         M.n_cols, M.va.dtype)


def transpose_reference(A):
    """Aᵀ as the stable sort of A's entries by column: ascending rows within
    every output row, values permuted and nothing else."""
    m = len(A.ro) - 1
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(A.ro))
    order = np.argsort(A.ci, kind="stable")
    ro = np.zeros(A.n_cols + 1, dtype=np.int64)
    np.cumsum(np.bincount(A.ci, minlength=A.n_cols), out=ro[1:])
    return Csr(ro, rows[order], A.va[order], m)


def arrival_schedule(A, B, i):
    """Keys of C's row i in the order the mode-0 kernels insert them: one B
    row per entry of A's row i, 64 columns (one per lane) per step."""
    steps = []
    for k in range(A.ro[i], A.ro[i + 1]):
        s, e = B.ro[A.ci[k]], B.ro[A.ci[k] + 1]
        steps += [B.ci[t:min(t + 64, e)] for t in range(s, e, 64)]
    return steps


def overlapping_pieces(rng, cols, t):
    """t subsets of the distinct columns `cols` with union `cols`, each
    overlapping its predecessor by a few columns; each sorted."""
    w = len(cols)
    p = rng.permutation(cols)
    if t == 1:
        return [np.sort(p)]
    cuts = np.sort(rng.choice(np.arange(1, w), size=t - 1, replace=False))
    bounds = [0] + [int(c) for c in cuts] + [w]
    pieces = []
    for q in range(t):
        lo = bounds[q]
        if q > 0:
            lo = max(0, lo - int(rng.randint(1, 6)))
        pieces.append(np.sort(p[lo:bounds[q + 1]]))
    return pieces


def tier_edge_families(top_cap, with_top=True):
    """(row width, number of rows) of the tier-edge matrix."""
    fam = [(w, 64) for w in range(56, 65)] + [(65, 2), (66, 2)]
    fam += [(w, 16) for w in range(505, 512)] + [(512, 400), (513, 2)]
    if with_top:
        fam += [(top_cap - 1, 4), (top_cap, 4)]
    return fam


def tier_edge_case(top_cap, cplx=False, short_rows=0, with_top=True, seed=11):
    """A (m x k) and B (k x top_cap + 64) whose product has rows of the
    widths of tier_edge_families: each such row of A has one, two or three
    entries selecting B rows of random distinct columns whose union has the
    prescribed width (half of the rows 56..64 wide have one entry, so their
    keys arrive in one step). Also: four rows 64 wide with a second entry on
    an empty B row, three rows whose entries hit only empty B rows,
    `short_rows` rows of one or two entries on a pool of B rows 1..3 wide,
    empty rows of A at the start, in the middle and at the end, empty rows
    of B at the start, inside and at the end. Rows are shuffled, so one
    workgroup gets rows of several tiers. `widths` is the intended width of
    every row of C, `short` marks the short rows."""
    rng = np.random.RandomState(seed)
    n_cols = top_cap + 64
    dtype = np.complex128 if cplx else np.float64
    b_rows = [np.zeros(0, np.int64)]          # B row 0 is empty
    empty_b = [0]

    def add_b(cols):
        b_rows.append(cols)
        idx = len(b_rows) - 1
        if len(b_rows) % 97 == 0:             # an empty B row now and then
            empty_b.append(len(b_rows))
            b_rows.append(np.zeros(0, np.int64))
        return idx

    a_rows = []                    # (B row ids, intended width, short?)
    for w, count in tier_edge_families(top_cap, with_top):
        for r in range(count):
            if w <= 64:
                t = 1 if r % 2 == 0 else 2 + (r // 2) % 2
            else:
                t = 1 + r % 3
            cols = rng.choice(n_cols, size=w, replace=False)
            ids = [add_b(p) for p in overlapping_pieces(rng, cols, t)]
            a_rows.append((ids, w, False))
    for r in range(4):
        cols = np.sort(rng.choice(n_cols, size=64, replace=False))
        a_rows.append(([add_b(cols), empty_b[r % len(empty_b)]], 64, False))
    for r in range(3):
        a_rows.append((empty_b[:1 + r], 0, False))   # only empty B rows
    if short_rows:
        pool = [add_b(np.sort(rng.choice(n_cols, size=1 + q % 3,
                                         replace=False)))
                for q in range(32)]
        for r in range(short_rows):
            ids = list(rng.choice(pool, size=1 + r % 2, replace=False))
            width = len(np.unique(np.concatenate([b_rows[q] for q in ids])))
            a_rows.append((ids, width, True))
    b_rows.append(np.zeros(0, np.int64))      # B's last row is empty
    a_rows = [a_rows[q] for q in rng.permutation(len(a_rows))]
    blank = ([], 0, False)
    mid = len(a_rows) // 2
    a_rows = ([blank, blank] + a_rows[:mid] + [blank, blank] + a_rows[mid:]
              + [blank, blank])
    B = csr_from_rows(b_rows,
                      [exact_values(rng, len(c), cplx) for c in b_rows],
                      n_cols, dtype)
    A = csr_from_rows([r[0] for r in a_rows],
                      [exact_values(rng, len(r[0]), cplx) for r in a_rows],
                      len(b_rows), dtype)
    return TierEdge(A, B, np.array([r[1] for r in a_rows], dtype=np.int64),
                    np.array([r[2] for r in a_rows], dtype=bool))
