"""Shared inputs of tests/test_block_ref.py and tests/test_gpu_block.py: a
block-CSR matrix built together with its colouring, whose rows sit at the
edges of the block kernels, and scalar matrices with prescribed row widths
for the SpMV routing.

colored_block_matrix: 126 block rows in 8 colours of COLOR_SIZES rows, the
rows of a colour scattered over the matrix. Couplings join rows of different
colours only, so the colouring is valid by construction. The structure holds
two rows without a diagonal block (one in the first colour, one whose
couplings all lack a transpose entry), an empty row, a row of its diagonal
only, a row of LONG_OFFDIAG off-diagonal blocks, rows of exactly 1, 2, 3, 4,
5 and 8 entries, couplings without a transpose entry (about a quarter of
them), one stored all-zero block and, with halo=True, N_HALO halo columns
with couplings into them. Columns ascend within every row. The accessors
below find each feature again from the arrays alone.

Values, kind="exact": every entry is a nonzero integer in [-4, 4] times 2^-k,
k in 0..2 (vectors: k in 0..1), Gaussian integers for complex; prove_exact
shows by integer arithmetic that a product y = alpha A x + beta y + gamma b
of such data is exact in float32 in any order of summation.
kind="dominant": off-diagonal blocks have entries in [-1, 1] / (blocks of the
row * b), so that the off-diagonal part of every scalar row has an l1 norm of
at most 1; a diagonal block has off-diagonal entries in [-1, 1] / b and
diagonal entries of magnitude 4..6, negative where (row + component) is a
multiple of 3. Every scalar row is so dominant by a factor of at least 2,
which block DILU and block ILU(0) in colour order preserve: no E_i and no
pivot comes near singular. fallback=True (dominant only) rewrites the values
of five rows with two entries or couplings without transposes:
  singular_E  (s0, s1): D_s0 = A_s0s1 = A_s1s0 = I and D_s1 = S + I with the
              exactly singular integer block S = [[1, 2], [2, 4]] (+) I, so
              E_s1 = S exactly;
  nonfinite_E (p, i): D_p = [[1, inf], [1, 1]] (+) I, whose Gauss-Jordan
              inverse is not finite, so E_i is not;
  singular_D  q: D_q = S, no transposes, so E_q = S, and the fallback target
              is singular too.
"""

from types import SimpleNamespace

import numpy as np
import torch

from amgx_amd import CSRMatrix
from amgx_amd.amg.coloring import MatrixColoring

COLOR_SIZES = (16, 1, 65, 3, 17, 4, 15, 5)
N_ROWS = sum(COLOR_SIZES)
N_HALO = 9
LONG_OFFDIAG = 37
# widths every routing matrix holds (scalar_routing_widths)
ROUTING_WIDTHS = (0, 1, 7, 8, 9, 31, 32, 33, 200)

_NONZERO = np.array([-4.0, -3.0, -2.0, -1.0, 1.0, 2.0, 3.0, 4.0])
_TORCH = {np.dtype(np.float32): torch.float32,
          np.dtype(np.float64): torch.float64,
          np.dtype(np.complex64): torch.complex64,
          np.dtype(np.complex128): torch.complex128}


def np_dtype(dtype):
    return np.dtype({torch.float32: np.float32, torch.float64: np.float64,
                     torch.complex64: np.complex64,
                     torch.complex128: np.complex128}.get(dtype, dtype))


# ------------------------------------------------------------------ values
def exact_values(rng, shape, cplx=False, max_shift=2):
    scale = 2.0 ** -rng.randint(0, max_shift + 1, size=shape)
    if not cplx:
        return rng.choice(_NONZERO, size=shape) * scale
    re = rng.randint(-4, 5, size=shape).astype(np.float64)
    im = rng.randint(-4, 5, size=shape).astype(np.float64)
    zero = (re == 0) & (im == 0)
    re[zero] = rng.choice(_NONZERO, size=int(zero.sum()))
    return (re + 1j * im) * scale


def exact_vector(n, dtype, seed):
    """n exact entries (integers in [-4, 4] times 2^-k, k in 0..1)."""
    dt = np_dtype(dtype)
    v = exact_values(np.random.RandomState(seed), n, dt.kind == "c", 1)
    return torch.from_numpy(v.astype(dt))


def _shift(a):
    """Smallest s with a * 2^s integer in every real and imaginary part."""
    parts = np.concatenate([np.real(a).ravel(), np.imag(a).ravel()])
    for s in range(40):
        if np.all(parts * 2.0 ** s == np.round(parts * 2.0 ** s)):
            return s
    raise AssertionError("values are no small dyadic rationals")


def _l1_int(a, s):
    """|re| + |im| of a in units of 2^-s, as Python-exact int64."""
    return (np.round(np.abs(np.real(a)) * 2.0 ** s)
            + np.round(np.abs(np.imag(a)) * 2.0 ** s)).astype(np.int64)


def prove_exact(ro, ci, va, x, y=None, bvec=None, alpha=1.0, beta=0.0,
                gamma=0.0, bits=24):
    """Proof that y' = alpha A x + beta y + gamma bvec is exact in a format
    of `bits` mantissa bits in ANY order of summation, for block values va
    (nnz, b, b) (b = 1 for scalar). Every datum is an integer times a power
    of two, 2^-s with s found by _shift, so every product and every partial
    sum of products is an integer multiple of the finest unit 2^-S involved;
    its magnitude is at most the sum T of the l1 moduli (|re| + |im|, which
    bounds both parts of a complex product) of all terms of its row. If
    T / 2^-S < 2^bits for every row, every intermediate value is an integer
    of fewer than `bits` bits times 2^-S: representable, so no operation
    rounds, fused or not. Computed in int64; returns the largest bit length
    met, and raises AssertionError where the bound fails."""
    va = np.asarray(va)
    b = va.shape[1]
    x = np.asarray(x).reshape(-1, b)
    n = len(ro) - 1
    sa, sx = _shift(va), _shift(x)
    s_al = _shift(np.array([alpha]))
    rows = np.repeat(np.arange(n), np.diff(ro))
    term = np.einsum("krc,kc->kr", _l1_int(va, sa), _l1_int(x[ci], sx))
    total = np.zeros((n, b), dtype=np.int64)
    np.add.at(total, rows, term)
    parts = [(total * int(_l1_int(np.array([alpha]), s_al)[0]),
              sa + sx + s_al)]
    for coef, vec in ((beta, y), (gamma, bvec)):
        if vec is None or coef == 0:
            continue
        vec = np.asarray(vec).reshape(-1, b)[:n]
        sc, sv = _shift(np.array([coef])), _shift(vec)
        parts.append((_l1_int(vec, sv) * int(_l1_int(np.array([coef]),
                                                     sc)[0]), sc + sv))
    S = max(s for _, s in parts)
    bound = sum(p * 2 ** (S - s) for p, s in parts)
    top = int(bound.max()) if bound.size else 0
    assert top < 2 ** bits, (top.bit_length(), bits)
    return top.bit_length()


# --------------------------------------------------------------- structure
def _structure(seed, halo):
    rng = np.random.RandomState(seed)
    n = N_ROWS
    colors = np.repeat(np.arange(len(COLOR_SIZES)), COLOR_SIZES)
    colors = colors[rng.permutation(n)]
    pool = [list(np.nonzero(colors == c)[0]) for c in range(len(COLOR_SIZES))]

    def take(c):
        return int(pool[c].pop())

    sp = SimpleNamespace(
        nodiag_first=take(0), nodiag_notrans=take(6), empty=take(2),
        diag_only=take(2), long=take(4), singular_E=(take(0), take(2)),
        nonfinite_E=(take(0), take(4)), singular_D=take(6),
        four=take(2), five=take(4), eight=take(6))
    frozen = {sp.nodiag_first, sp.nodiag_notrans, sp.empty, sp.diag_only,
              sp.long, *sp.singular_E, *sp.nonfinite_E, sp.singular_D,
              sp.four, sp.five, sp.eight}
    cols = [set() for _ in range(n)]
    general = [i for i in range(n) if i not in frozen]

    def others(i, only_free):
        return [j for j in range(n) if colors[j] != colors[i]
                and not (only_free and j in frozen)]

    for i in general:
        cols[i].add(i)
        for j in rng.choice(others(i, False), size=rng.randint(2, 7),
                            replace=False):
            cols[i].add(int(j))
            # a frozen row keeps its exact width: no transpose into it
            if j not in frozen and rng.rand() < 0.75:
                cols[int(j)].add(i)

    def couple(i, count, transposes):
        cand = [j for j in others(i, True) if i not in cols[j]]
        for j in rng.choice(cand, size=count, replace=False):
            cols[i].add(int(j))
            if transposes and rng.rand() < 0.75:
                cols[int(j)].add(i)

    couple(sp.nodiag_first, 3, True)
    couple(sp.nodiag_notrans, 4, False)
    cols[sp.diag_only].add(sp.diag_only)
    cols[sp.long].add(sp.long)
    couple(sp.long, LONG_OFFDIAG, True)
    for u, v in (sp.singular_E, sp.nonfinite_E):
        cols[u].update((u, v))
        cols[v].update((u, v))
    cols[sp.singular_D].add(sp.singular_D)
    couple(sp.singular_D, 2, False)
    for i, width in ((sp.four, 4), (sp.five, 5), (sp.eight, 8)):
        cols[i].add(i)
        couple(i, width - 1, True)
    # one stored all-zero block: a coupling of a general row that has its
    # transpose entry
    sp.zero_block = next((i, j) for i in general for j in sorted(cols[i])
                         if j != i and i in cols[j])
    n_cols = n
    if halo:
        hrng = np.random.RandomState(seed + 7)
        n_cols = n + N_HALO
        for i in general[::5] + [sp.long]:
            for j in hrng.choice(N_HALO, size=hrng.randint(1, 3),
                                 replace=False):
                cols[i].add(n + int(j))
    ro = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(c) for c in cols], out=ro[1:])
    ci = np.array([j for c in cols for j in sorted(c)], dtype=np.int64)
    return colors, ro, ci, n_cols, sp


def _values(ro, ci, b, kind, seed, sp, fallback):
    rng = np.random.RandomState(seed)
    n = len(ro) - 1
    va = np.zeros((len(ci), b, b))
    pos = {}
    for i in range(n):
        width = ro[i + 1] - ro[i]
        for k in range(ro[i], ro[i + 1]):
            j = int(ci[k])
            pos[(i, j)] = k
            if kind == "exact":
                va[k] = exact_values(rng, (b, b))
            elif j != i:
                va[k] = rng.uniform(-1.0, 1.0, (b, b)) / (width * b)
            else:
                va[k] = rng.uniform(-1.0, 1.0, (b, b)) / b
                comp = np.arange(b)
                sign = np.where((i + comp) % 3 == 0, -1.0, 1.0)
                va[k][comp, comp] = sign * rng.uniform(4.0, 6.0, b)
    va[pos[sp.zero_block]] = 0.0
    if fallback:
        assert kind == "dominant" and b >= 2
        eye = np.eye(b)
        S = eye.copy()
        S[:2, :2] = [[1.0, 2.0], [2.0, 4.0]]
        s0, s1 = sp.singular_E
        va[pos[(s0, s0)]] = va[pos[(s0, s1)]] = va[pos[(s1, s0)]] = eye
        va[pos[(s1, s1)]] = S + eye
        p, _ = sp.nonfinite_E
        va[pos[(p, p)]] = eye
        va[pos[(p, p)]][0, 1] = np.inf
        va[pos[(p, p)]][1, 0] = 1.0
        va[pos[(sp.singular_D, sp.singular_D)]] = S
    return va


def colored_block_matrix(b, dtype, seed=0, kind="dominant", halo=False,
                         fallback=False):
    """The matrix of the module docstring for block size b. Returns a record
    with A (CSRMatrix, values of `dtype`), coloring (MatrixColoring), the
    numpy arrays ro, ci, colors, va (float64 (nnz, b, b): the values after
    rounding to `dtype`, so a reference reads what the kernels read), n_rows,
    n_cols, b and special (the rows the structure was built around)."""
    dt = np_dtype(dtype)
    colors, ro, ci, n_cols, sp = _structure(seed, halo)
    va = _values(ro, ci, b, kind, seed * 1000 + b, sp, fallback)
    with np.errstate(over="ignore"):
        va = va.astype(dt).astype(np.float64)
    A = CSRMatrix.from_bsr(ro, ci, va, n_cols=n_cols, dtype=_TORCH[dt])
    coloring = MatrixColoring(torch.from_numpy(colors.astype(np.int32)),
                              len(COLOR_SIZES))
    return SimpleNamespace(A=A, coloring=coloring, ro=ro, ci=ci, va=va,
                           colors=colors, n_rows=N_ROWS, n_cols=n_cols, b=b,
                           special=sp)


# ---------------------------------------------------------------- accessors
def _has(case, i, j):
    return j in case.ci[case.ro[i]:case.ro[i + 1]]


def empty_rows(case):
    return [i for i in range(case.n_rows) if case.ro[i] == case.ro[i + 1]]


def missing_diag_rows(case):
    """Rows with entries but no diagonal block."""
    return [i for i in range(case.n_rows)
            if case.ro[i] < case.ro[i + 1] and not _has(case, i, i)]


def diag_only_rows(case):
    return rows_of_width(case, 1, with_diag=True)


def rows_of_width(case, width, with_diag=None):
    return [i for i in range(case.n_rows)
            if case.ro[i + 1] - case.ro[i] == width
            and (with_diag is None or _has(case, i, i) == with_diag)]


def long_rows(case, offdiag=LONG_OFFDIAG):
    return [i for i in range(case.n_rows)
            if sum(j != i for j in case.ci[case.ro[i]:case.ro[i + 1]])
            >= offdiag]


def missing_transpose_entries(case):
    """Entries (i, j), j a local column other than i, without an (j, i)."""
    return [k for i in range(case.n_rows)
            for k in range(case.ro[i], case.ro[i + 1])
            if case.ci[k] != i and case.ci[k] < case.n_rows
            and not _has(case, int(case.ci[k]), i)]


def local_offdiag_entries(case):
    return [k for i in range(case.n_rows)
            for k in range(case.ro[i], case.ro[i + 1])
            if case.ci[k] != i and case.ci[k] < case.n_rows]


def zero_blocks(case):
    return [k for k in range(len(case.ci)) if not case.va[k].any()]


def halo_rows(case):
    return [i for i in range(case.n_rows)
            if (case.ci[case.ro[i]:case.ro[i + 1]] >= case.n_rows).any()]


def negative_diag_rows(case):
    """Rows whose diagonal block has a negative diagonal entry."""
    out = []
    for i in range(case.n_rows):
        for k in range(case.ro[i], case.ro[i + 1]):
            if case.ci[k] == i and (np.diag(case.va[k]) < 0).any():
                out.append(i)
    return out


def coloring_is_valid(case):
    rows = np.repeat(np.arange(case.n_rows), np.diff(case.ro))
    loc = (case.ci < case.n_rows) & (case.ci != rows)
    return not (case.colors[rows[loc]] == case.colors[case.ci[loc]]).any()


# ------------------------------------------------------------------- scalar
def scalar_routing_widths(n_rows, nnz):
    """n_rows row widths with sum nnz: ROUTING_WIDTHS once each, the rest
    split evenly, shuffled, so nnz / n_rows is the average degree asked."""
    rest, left = n_rows - len(ROUTING_WIDTHS), nnz - sum(ROUTING_WIDTHS)
    lo, extra = divmod(left, rest)
    w = list(ROUTING_WIDTHS) + [lo + 1] * extra + [lo] * (rest - extra)
    w = np.array(w, dtype=np.int64)
    return w[np.random.RandomState(n_rows + nnz).permutation(n_rows)]


def scalar_matrix(widths, n_cols, dtype, kind="exact", seed=0):
    """Scalar CSR with exactly widths[i] entries in row i, at distinct random
    ascending columns below n_cols. kind="exact": the values of the module
    docstring; kind="dominant": uniform in [-1, 1] (no diagonal is built,
    the name only mirrors colored_block_matrix). Returns the CSRMatrix and
    its numpy arrays ro, ci, va (va in `dtype`)."""
    dt = np_dtype(dtype)
    rng = np.random.RandomState(seed)
    ro = np.zeros(len(widths) + 1, dtype=np.int64)
    np.cumsum(widths, out=ro[1:])
    ci = np.concatenate([np.sort(rng.choice(n_cols, size=int(w),
                                            replace=False))
                         for w in widths] + [np.zeros(0, np.int64)])
    if kind == "exact":
        va = exact_values(rng, len(ci), dt.kind == "c")
    else:
        va = rng.uniform(-1.0, 1.0, len(ci))
    va = va.astype(dt)
    A = CSRMatrix(torch.from_numpy(ro.astype(np.int32)),
                  torch.from_numpy(ci.astype(np.int32)),
                  torch.from_numpy(va), n_cols=n_cols)
    return A, ro, ci.astype(np.int64), va
