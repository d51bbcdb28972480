"""GPU backend: thin wrappers over the in-tree gfx950 extension amgx_amd._core.

Import FAILS LOUDLY if the extension is missing — on a GPU machine there is no
silent eager fallback (the HIP kernels ARE the product). Structural byproducts
(diag index, transpose index, scratch vectors) are cached on the matrix.

Per-kernel reference citations live in the HIP sources (csrc/kernels_*.hip:
reference src/multiply.cu, src/blas.cu, src/norm.cu, src/solvers/*.cu,
src/csr_multiply*.cu, src/matrix_coloring/*.cu, src/aggregation/*,
src/classical/*); this module only routes tensors into them.
"""

from __future__ import annotations

import math

import torch

try:
    from .. import _core
except ImportError as e:  # pragma: no cover
    raise ImportError(
        "amgx_amd._core (gfx950 HIP extension) is not built. Run "
        "`PYTORCH_ROCM_ARCH=gfx950 python setup.py build_ext --inplace` "
        f"at the repo root. Underlying error: {e}") from e


# ---------------------------------------------------------------------- helpers
def _didx(A):
    if A._diag_idx is None:
        A._diag_idx = _core.diag_index(A.row_offsets, A.col_indices, A.n_rows)
    return A._diag_idx


def _tidx(A):
    t = A._cache.get("tidx")
    if t is None:
        t = _core.trans_index(A.row_offsets, A.col_indices, A.n_rows)
        A._cache["tidx"] = t
    return t


def _scratch(A, name, numel, dtype=None):
    dtype = dtype if dtype is not None else A.dtype
    key = ("scratch", name, numel, dtype)
    t = A._cache.get(key)
    if t is None:
        t = torch.empty(numel, dtype=dtype, device=A.device)
        A._cache[key] = t
    return t


MAX_BLOCK_DIM = 16


def _check_block_dim(A, name):
    """The block Jacobi / GS / DILU / ILU(0) kernels keep a block, or one
    vector of block_dim components, in private arrays of MAX_BLOCK_DIM
    (csrc/core_api.h); refuse a larger block size before anything is
    launched. The block SpMV takes any block size."""
    if not 1 <= A.block_dim <= MAX_BLOCK_DIM:
        raise ValueError(
            f"{name}: block_dim {A.block_dim} is outside the supported range "
            f"1..{MAX_BLOCK_DIM} of the block smoother kernels")


# ---------------------------------------------------------------------- structure
def compute_diag_index(A):
    return _didx(A)


def extract_diagonal(A):
    if A.diag is not None:
        return A.diag
    return _core.extract_diag(A.row_offsets, A.col_indices, A.values,
                              _didx(A), A.n_rows, A.block_dim)


# ---------------------------------------------------------------------- SpMV
def spmv(A, x, y=None, alpha=1.0, beta=0.0, row_begin=0, row_end=-1):
    assert A.diag is None, \
        "external DIAG matrices must be folded at upload (capi does this)"
    if row_end < 0:
        row_end = A.n_rows
    if y is None:
        y = torch.zeros(A.n_rows * A.block_dim, dtype=x.dtype, device=x.device)
        beta = 0.0
    _core.csrmv(A.row_offsets, A.col_indices, A.values, A.block_dim,
                x.reshape(-1), y.reshape(-1), None, alpha, beta, 0.0,
                row_begin, row_end)
    return y


def residual(A, x, b, r=None, row_begin=0, row_end=-1):
    if r is None:
        r = torch.empty_like(b)
    if row_end < 0:
        row_end = A.n_rows
    _core.csrmv(A.row_offsets, A.col_indices, A.values, A.block_dim,
                x.reshape(-1), r.reshape(-1), b.reshape(-1), -1.0, 0.0, 1.0,
                row_begin, row_end)
    return r


# ---------------------------------------------------------------------- BLAS-1
def _coef(v, alpha):
    """Coefficient for a kernel on ``v``: complex vectors (dZZI / dCCI / dZCI
    modes) take it as complex, real ones as float exactly as before."""
    return complex(alpha) if v.is_complex() else float(alpha)


# op codes of _core.reduce_op: sum conj(x) y; sum|x|; max|x|; sum|x|^2
# (complex x only)
_RED_DOT, _RED_L1, _RED_LMAX, _RED_ABS2 = range(4)


def dot(x, y):
    r = _core.reduce_op(x.reshape(-1), y.reshape(-1), _RED_DOT).item()
    # complex: conj(x) . y, the convention of ops/cpu.py (torch.vdot)
    return complex(r) if x.is_complex() else float(r)


def nrm2(x):
    if x.is_complex():
        # real accumulation of re^2 + im^2, not Re(vdot(x, x))
        return math.sqrt(float(_core.reduce_op(x.reshape(-1), None,
                                               _RED_ABS2).item()))
    return math.sqrt(max(float(_core.reduce_op(x.reshape(-1), x.reshape(-1),
                                               _RED_DOT).item()), 0.0))


def nrm1(x):
    return float(_core.reduce_op(x.reshape(-1), None, _RED_L1).item())


def nrmmax(x):
    return float(_core.reduce_op(x.reshape(-1), None, _RED_LMAX).item())


def dot_async(x, y):
    """Device-scalar dot (no host sync) for fused/graph paths; real only."""
    if x.is_complex():
        raise TypeError("dot_async is real-only (complex modes use dot)")
    return _core.reduce_op(x.reshape(-1), y.reshape(-1), _RED_DOT)


def axpy_dalpha(y, x, alpha, scale=1.0):
    """y += scale * alpha[0] * x with device-resident alpha (no host
    sync; Krylov MGS projections)."""
    _core.axpy_dalpha(y.reshape(-1), x.reshape(-1), alpha.reshape(-1),
                      float(scale))
    return y


def scal_drsqrt(x, s2):
    """x *= rsqrt(s2[0]) with device-resident s2 (no-op when s2<=0)."""
    _core.scal_drsqrt(x.reshape(-1), s2.reshape(-1))
    return x


def axpy(y, x, alpha):
    _core.axpy(y.reshape(-1), x.reshape(-1), _coef(x, alpha))
    return y


def axpby(y, x, alpha, beta):
    _core.axpby(y.reshape(-1), x.reshape(-1), _coef(x, alpha),
                _coef(x, beta))
    return y


def scal(x, alpha):
    _core.scal(x.reshape(-1), _coef(x, alpha))
    return x


# ---------------------------------------------------------------------- smoothers
def jacobi_dinv(A, l1: bool = False):
    _check_block_dim(A, "jacobi_dinv")
    if l1 and A.values.is_complex():
        raise NotImplementedError(
            "JACOBI_L1 is not available in the complex modes (dZZI / dCCI / "
            "dZCI): the device l1 diagonal is real-only")
    return _core.jacobi_dinv(A.row_offsets, A.col_indices, A.values, _didx(A),
                             A.n_rows, A.block_dim, bool(l1))


def jacobi_smooth(A, dinv, b, x_in, x_out, omega: float):
    _core.jacobi_smooth(A.row_offsets, A.col_indices, A.values, A.block_dim,
                        dinv, b.reshape(-1), x_in.reshape(-1),
                        x_out.reshape(-1), float(omega))
    return x_out


def gs_smooth_color(A, dinv, b, x, color_rows, omega: float):
    _check_block_dim(A, "gs_smooth_color")
    _core.gs_smooth_rows(A.row_offsets, A.col_indices, A.values, A.block_dim,
                         dinv, b.reshape(-1), x.reshape(-1), color_rows,
                         float(omega))
    return x


def gs_sweep(A, dinv, b, x, coloring, omega: float, symmetric: bool = False):
    _check_block_dim(A, "gs_sweep")
    if A.block_dim == 1:
        # color-sorted slab layout (reference reorder-by-color)
        st = _slabs(A, coloring)
        va_s = _slab_copy(st, "gs_va", A.values,
                          lambda v: _gather_nz(v, st.nzmap))
        dinv_s = _slab_copy(st, "gs_dinv", dinv,
                            lambda d: d.reshape(-1)[st.perm])
        _core.gs_sweep_sorted(st.ro_s, st.ci_s, va_s, dinv_s, b.reshape(-1),
                              x.reshape(-1), coloring.rows_sorted,
                              coloring.bounds, coloring.bounds_dev,
                              float(omega), bool(symmetric))
        return x
    _core.gs_sweep(A.row_offsets, A.col_indices, A.values, A.block_dim, dinv,
                   b.reshape(-1), x.reshape(-1), coloring.rows_sorted,
                   coloring.bounds, float(omega), bool(symmetric))
    return x


# ---------------------------------------------------------------------- coloring
# Rounds per read-back of the round flags in the coloring and matching loops
# where the caller names none: 0 = by level size (bindings.cpp round_batch).
# Every value gives the same colors and aggregates; tests set it to compare.
ROUND_BATCH = 0


def color_matrix(A, max_uncolored_frac: float = 0.0, seed: int = 0,
                 multihash_rounds: int = 0, batch: int = 0):
    """Device Jones-Plassmann greedy coloring rounds; multihash_rounds > 0
    prepends MULTI_HASH semantics (color = round id, per-round re-hash).
    batch (tests, bench_kernels.py): rounds per read-back of the round flags,
    0 = by level size; every value gives the same colors."""
    # dense coarse-level graphs (classical RAP) need ~max-clique rounds:
    # each greedy round colors only the local maxima of the uncolored set
    colors, nc = _core.color_minmax(A.row_offsets, A.col_indices, A.n_rows,
                                    4096, int(seed), int(multihash_rounds),
                                    int(batch or ROUND_BATCH))
    return colors, int(nc)


def color_order(colors, num_colors):
    """(rows_sorted int32, bounds_dev int32 (num_colors + 1,)): the rows
    stably sorted by color and the first slot of each color."""
    return _core.key_order(colors.to(torch.int32).contiguous(),
                           int(num_colors))


def aggregate_csr(aggregates, num_aggregates):
    """Aggregate-membership CSR (offsets int32 (num + 1,), fine ids int32
    sorted by aggregate, ascending within one)."""
    fids, off = _core.key_order(aggregates.to(torch.int32).contiguous(),
                                int(num_aggregates))
    return off, fids


# ---------------------------------------------------------------------- DILU
class _Slabs:
    """Structure of the rows_sorted-gathered matrix copy under ONE coloring
    (reference reorder-by-color, include/matrix.h:766): slot-ordered row
    offsets ro_s, gathered columns ci_s, the int32 nz gather map nzmap (for
    value re-gathers after replace_coefficients, through _gather_nz),
    perm = rows_sorted as int64 and its inverse slot_of_row; copies holds the
    gathered value arrays.
    upper / lower: the strict color-split parts of the slab for the scalar
    DILU sweeps, each (offsets, columns, int32 map into the full slab), built
    on first use by _slab_part."""
    __slots__ = ("coloring", "ro_s", "ci_s", "nzmap", "perm", "slot_of_row",
                 "copies", "upper", "lower")


def _slabs(A, coloring):
    """The matrix's slab record; rebuilt (dropping every gathered copy) when
    the matrix is swept under another coloring object."""
    st = A._cache.get("slabs")
    if st is None or st.coloring is not coloring:
        st = _Slabs()
        st.coloring = coloring
        st.copies = {}
        st.upper = st.lower = None
        st.ro_s, st.ci_s, st.nzmap, st.slot_of_row = _core.slab_structure(
            A.row_offsets, A.col_indices, coloring.rows_sorted)
        st.perm = coloring.rows_sorted.to(torch.int64)
        A._cache["slabs"] = st
    return st


def _gather_nz(values, nzmap, b: int = 1):
    """values[nzmap] for b components per entry, flat."""
    src = values.reshape(-1)
    out = torch.empty(nzmap.numel() * b, dtype=src.dtype, device=src.device)
    _core.gather(src.contiguous(), nzmap, b, out)
    return out


def _slab_copy(st, name, src, gather):
    """gather(src) in slab order, redone when src is another tensor or has
    been written in place since the cached copy was taken."""
    key = (src.data_ptr(), src._version)
    hit = st.copies.get(name)
    if hit is None or hit[0] != key:
        hit = (key, gather(src))
        st.copies[name] = hit
    return hit[1]


def _slab_part(st, upper):
    """Structure (ro, ci, map) of the U (upper) or L part of the slab: the
    entries of later- / earlier-color local columns, in slab order."""
    part = st.upper if upper else st.lower
    if part is None:
        part = tuple(_core.slab_split(st.ro_s, st.ci_s,
                                      st.coloring.rows_sorted,
                                      st.coloring.colors, bool(upper)))
        if upper:
            st.upper = part
        else:
            st.lower = part
    return part


def _split_path(A):
    """Scalar levels past the size of the one-launch apply sweep the split
    slabs color by color."""
    return A.block_dim == 1 and A.n_rows > _core.DILU_SMALL_ROWS


class DiluState:
    """Device DILU factor state: Einv in original row order (einv) plus the
    color-sorted matrix/Einv copies the sweeps read contiguously. For scalar
    matrices va_u holds the values of the U part and va_l, gathered on the
    first plain apply, those of the L part."""
    __slots__ = ("einv", "va_s", "einv_s", "va_u", "va_l")

    def __init__(self, einv, va_s, einv_s, va_u=None):
        self.einv = einv
        self.va_s = va_s
        self.einv_s = einv_s
        self.va_u = va_u
        self.va_l = None

    def cpu(self):          # test convenience: compare against host Einv
        return self.einv.cpu()


def _check_dilu_coloring(A, coloring):
    """DILU reads Einv_j and w_j of every coupled row j of an earlier color
    and takes same-color rows as uncoupled; two coupled rows of one color
    would be skipped by the factor and raced on by the sweeps. The complex
    modes check this once per setup; the real modes keep their setup as it
    was and rely on the coloring they are given."""
    n = A.n_rows
    ro = A.row_offsets.to(torch.int64)
    rows = torch.repeat_interleave(
        torch.arange(n, dtype=torch.int64, device=A.device), ro[1:] - ro[:-1])
    cols = A.col_indices.to(torch.int64)
    off = (cols != rows) & (cols < n)
    colors = coloring.colors.to(torch.int64)
    clash = off & (colors[rows] == colors[cols.clamp(max=n - 1)])
    if bool(clash.any()):
        raise RuntimeError(
            "dilu_setup: the coloring is not a valid distance-1 coloring of "
            f"the matrix ({int(clash.sum())} couplings join rows of one "
            "color)")


def dilu_setup(A, coloring):
    _check_block_dim(A, "dilu_setup")
    if A.values.is_complex():
        _check_dilu_coloring(A, coloring)
    einv = _core.dilu_setup(A.row_offsets, A.col_indices, A.values,
                            A.block_dim, _didx(A), _tidx(A), coloring.colors,
                            coloring.rows_sorted, coloring.bounds)
    st = _slabs(A, coloring)
    bb = A.block_dim * A.block_dim
    va_s = _gather_nz(A.values, st.nzmap, bb)
    einv_s = einv.reshape(A.n_rows, bb)[st.perm].reshape(-1).contiguous() \
        if A.block_dim > 1 else einv[st.perm].contiguous()
    # scalar levels of every size sweep the U part backwards
    va_u = _gather_part(va_s, _slab_part(st, True)) if A.block_dim == 1 \
        else None
    return DiluState(einv, va_s, einv_s, va_u)


def _gather_part(va_s, part):
    out = torch.empty(part[2].numel(), dtype=va_s.dtype, device=va_s.device)
    _core.gather(va_s, part[2], 1, out)
    return out


DILU_FORMS = ("split", "small", "small_full", "stream")


def _dilu_sorted(A, Einv, coloring, rhs, x, relaxation, fused, lanes=0,
                 sweeps=1, form=None):
    """`sweeps` applies back to back. Scalar levels take the one-launch apply
    ("small") up to DILU_SMALL_ROWS rows and the per-color sweeps ("split")
    past it; form (tests, bench_kernels.py) names one of DILU_FORMS whatever
    the size, "small_full" being the one-launch apply in its earlier
    full-slab form and "stream" the per-color sweeps in their stream form for
    every color (it goes with lanes=0 only)."""
    _check_block_dim(A, "dilu_solve / dilu_smooth")
    n = A.n_cols * A.block_dim   # ext size: halo tails stay zero in the sweeps
    w = _scratch(A, "dilu_w", n, x.dtype)   # vector precision (dDFI mixed)
    st = _slabs(A, coloring)
    forced = form is not None     # lifts the row bound of the one-launch forms
    if A.block_dim != 1:
        if lanes or forced:
            raise ValueError("lanes and form select among the scalar DILU "
                             "sweeps; a block level does not run them")
        form = "block"
    elif form is None:
        form = "split" if _split_path(A) else "small"
    elif form not in DILU_FORMS:
        raise ValueError(f"form must be one of {DILU_FORMS}")
    if form in ("split", "small", "stream"):
        ro_u, ci_u, _ = _slab_part(st, True)
        y = None
        if fused:
            fwd = (st.ro_s, st.ci_s, Einv.va_s)
            y = _scratch(A, "dilu_y", n, x.dtype)   # x + w, the gathered one
        else:
            ro_l, ci_l, _ = part = _slab_part(st, False)
            if Einv.va_l is None:
                Einv.va_l = _gather_part(Einv.va_s, part)
            fwd = (ro_l, ci_l, Einv.va_l)
        if form == "small":
            _core.dilu_small(*fwd, ro_u, ci_u, Einv.va_u, Einv.einv_s,
                             coloring.rows_sorted, coloring.bounds,
                             coloring.bounds_dev, rhs.reshape(-1), w,
                             x.reshape(-1), float(relaxation), fused,
                             int(lanes), y, int(sweeps), forced)
            return
        for _ in range(sweeps):
            _core.dilu_split(*fwd, ro_u, ci_u, Einv.va_u, Einv.einv_s,
                             coloring.rows_sorted, coloring.bounds,
                             rhs.reshape(-1), w, x.reshape(-1),
                             float(relaxation), fused, int(lanes), y,
                             2 if form == "stream" else 0)
        return
    if lanes:
        raise ValueError("lanes selects the form of the split-slab sweeps; "
                         "the full-slab apply has one")
    z = _scratch(A, "dilu_z", n, x.dtype)
    for _ in range(sweeps):
        _core.dilu_sorted(st.ro_s, st.ci_s, Einv.va_s, A.block_dim,
                          Einv.einv_s, coloring.rows_sorted, coloring.bounds,
                          coloring.bounds_dev, rhs.reshape(-1), w, z,
                          x.reshape(-1), float(relaxation), fused, forced)


def dilu_smooth(A, Einv, coloring, b, x, relaxation, lanes=0, sweeps=1,
                form=None):
    """x += relax * M^{-1}(b - A x) with the residual fused into the
    forward sweep (one matrix read fewer than residual + dilu_solve);
    b=1 scalar and b=4 MFMA paths. Returns False when this block size has
    no fused kernel (caller falls back to residual + dilu_solve).
    sweeps: that many smoothing steps back to back, in one launch where the
    level takes the one-launch apply; the same bits as that many calls.
    lanes (tests, bench_kernels.py): lanes per row of the scalar split-slab
    sweeps, 1 or 8; 0 routes each slab by its entries per row. form: see
    _dilu_sorted."""
    if A.block_dim not in (1, 4):
        return False
    if getattr(A, "manager", None) is not None:
        return False   # distributed path must exchange halos of x first
    _dilu_sorted(A, Einv, coloring, b, x, relaxation, True, lanes, sweeps,
                 form)
    return True


def dilu_solve(A, Einv, coloring, r, relaxation, x, lanes=0, sweeps=1,
               form=None):
    _dilu_sorted(A, Einv, coloring, r, x, relaxation, False, lanes, sweeps,
                 form)
    return x


# ---------------------------------------------------------------------- aggregation
def size2_roots(A, max_iterations: int = 15, seed: int = 0, batch: int = 0,
                weights: bool = False):
    """The handshake matching as root fine-row ids (int32 (n,); roots[r] == r
    exactly at the roots). batch (tests, bench_kernels.py): rounds per
    read-back, 0 = ROUND_BATCH. weights (tests, bench_kernels.py): edge
    weights computed once per call instead of in every round. Every value of
    either gives the same roots."""
    if A.block_dim > 1 and A.values.is_complex():
        raise NotImplementedError(
            "aggregation of a block matrix is not available in the complex "
            "modes (dZZI / dCCI / dZCI)")
    diag = extract_diagonal(A)
    if A.block_dim > 1:
        # Frobenius norms drive the matching for real block matrices
        diag = torch.linalg.vector_norm(diag.reshape(A.n_rows, -1), dim=1)
        va = torch.linalg.vector_norm(
            A.values.reshape(A.nnz, -1).to(torch.float64), dim=1).to(A.dtype)
        diag = diag.to(A.dtype)
    else:
        # scalar, real or complex: the kernel weighs an edge by |a_ij|,
        # the modulus for complex values
        va = A.values
    return _core.size2_match(A.row_offsets, A.col_indices, va, _tidx(A), diag,
                             A.n_rows, max_iterations,
                             int(seed) + 0x9E3779B1,
                             int(batch or ROUND_BATCH), bool(weights))


def size2_matching(A, max_iterations: int = 15, deterministic: bool = True,
                   seed: int = 0, batch: int = 0):
    # the roots are fine-row ids: flag, scan and map number them, no sort
    agg, num = _core.size2_renumber(
        size2_roots(A, max_iterations, seed, batch))
    return agg, int(num)


def pairwise_weights(A, formula: int = 0):
    if A.block_dim > 1 and A.values.is_complex():
        raise NotImplementedError(
            "aggregation of a block matrix is not available in the complex "
            "modes (dZZI / dCCI / dZCI)")
    if formula == 1 and (A.values.is_complex() or A.block_dim > 1):
        raise NotImplementedError(
            "weight_formula 1 is signed: scalar real matrices only")
    if A.block_dim > 1:
        # Frobenius norm of each block, in double; the diagonal "value" is
        # the norm of the diagonal block
        va = torch.linalg.vector_norm(
            A.values.reshape(A.nnz, -1).to(torch.float64), dim=1)
        didx = _didx(A).long()
        diag = torch.where(didx >= 0, va[didx.clamp(min=0)],
                           torch.zeros((), dtype=va.dtype, device=va.device))
    else:
        va, diag = A.values, extract_diagonal(A)
    return _core.pairwise_weights(A.row_offsets, A.col_indices, va, _tidx(A),
                                  diag.contiguous(), A.n_rows, int(formula))


def pairwise_matching(row_offsets, col_indices, w, n, sizes, cap,
                      merge_singletons, max_iterations, max_unassigned, seed,
                      lanes: int = 0):
    """lanes: lanes per row of the propose kernel (1 or 8; 0 = routed by
    average degree). Both give the same result."""
    agg, num, szs, rounds = _core.pairwise_match(
        row_offsets, col_indices, w, int(n), sizes, int(cap or 0),
        int(merge_singletons), int(max_iterations), float(max_unassigned),
        int(seed) & 0x7FFFFFFF, int(lanes))
    return agg, int(num), szs, int(rounds)


def galerkin_aggregation(A, aggregates, num_aggregates, agg_col=None,
                         ncols_mod=None, generator=None, structure=None):
    """structure: the aggregate-membership CSR (offsets, fine ids) of
    aggregate_csr when the caller holds it already; built here otherwise.

    agg_col/ncols_mod: distributed variant — per-column coarse ids (GLOBAL)
    and the global coarse column count; defaults to the single-process case.

    Real and complex values alike (complex: scalar matrices only). A
    row wider than the top hash tier of the value type
    (_core.SPGEMM_HASH_TOP_CAP: 8192 entries, 4096 for complex128) takes the
    one-sort generator.

    Scalar matrices run the LDS-hash LOW_DEG-style generator
    (kernels_spgemm.hip mode 1: wave-per-coarse-row hash accumulation —
    reference src/aggregation/coarseAgenerators/low_deg_…); block matrices,
    hash-capacity overflows, and generator=="THRUST" use the one-sort
    rocPRIM generator (the tiered dispatch is the reference HYBRID role)."""
    from ..matrix import CSRMatrix
    if agg_col is None:
        agg_col = aggregates
    if ncols_mod is None:
        ncols_mod = num_aggregates
    if A.block_dim > 1 and A.values.is_complex():
        raise NotImplementedError(
            "the Galerkin product of a block matrix is not available in the "
            "complex modes (dZZI / dCCI / dZCI)")
    if A.block_dim == 1 and generator != "THRUST":
        # aggregate-membership CSR: coarse row -> fine member rows
        m_ro, fids = structure if structure is not None \
            else aggregate_csr(aggregates, num_aggregates)
        ro, ci, va, big = _core.spgemm_hash(
            m_ro, fids, A.values,   # vaA unused in mode 1
            A.row_offsets, A.col_indices, A.values,
            agg_col, 1, max(A.nnz, 1),
            64 if A.nnz <= 48 * max(num_aggregates, 1) else 512)
        if int(ro[0].item()) != -1:
            if big.numel():
                _sort_unsorted_rows(ro, ci, va, big)
            return CSRMatrix(ro, ci.contiguous(), va.contiguous(),
                             n_cols=int(ncols_mod), block_dim=1)
    ro_c, ci_c, va_c = _core.galerkin_agg(A.row_offsets, A.col_indices,
                                          A.values, aggregates, agg_col,
                                          num_aggregates, int(ncols_mod),
                                          A.block_dim)
    out = CSRMatrix(ro_c, ci_c.contiguous(), va_c.contiguous(),
                    n_cols=int(ncols_mod), block_dim=A.block_dim)
    return out


def restrict_agg(r, aggregates, num_aggregates, block_dim: int = 1,
                 structure=None, out=None):
    """``out``: a vector of at least num_aggregates * block_dim entries whose
    prefix receives the result (no allocation, no copy)."""
    nc = num_aggregates * block_dim
    if out is None or out.dtype != r.dtype:
        rc = torch.empty(nc, dtype=r.dtype, device=r.device)
    else:
        rc = out.reshape(-1)[:nc]
    if structure is not None:
        off, fids = structure
        _core.restrict_csr(r.reshape(-1), off, fids, block_dim, rc)
    else:
        _core.restrict_agg(r.reshape(-1), aggregates, block_dim, rc)
    if out is not None and out.dtype != r.dtype:
        out.reshape(-1)[:nc].copy_(rc)
    return rc


def prolongate_agg(x, xc, aggregates, block_dim: int = 1):
    _core.prolongate_agg(x.reshape(-1), xc.reshape(-1), aggregates, block_dim)
    return x


# ---------------------------------------------------------------------- SpGEMM
def _expansion_bound(A, B):
    degB = (B.row_offsets[1:] - B.row_offsets[:-1]).to(torch.int64)
    return int(degB[A.col_indices.to(torch.int64)].sum().item())


def _sort_unsorted_rows(ro, ci, va, big_rows):
    """Column-sort the (rare) rows the top-tier hash kernel wrote
    unsorted (>512 nnz per row); va is None for a pattern without values."""
    ro64 = ro.to(torch.int64)
    for r in big_rows.tolist():
        s, e = int(ro64[r]), int(ro64[r + 1])
        order = torch.argsort(ci[s:e])
        ci[s:e] = ci[s:e][order]
        if va is not None:
            va[s:e] = va[s:e][order]


def spgemm(A, B):
    """C = A*B — LDS-hash kernels (kernels_spgemm.hip, role of reference
    src/csr_multiply_detail.cu warp-hash family); ESC sort fallback for
    pathological rows past the top hash tier (>8k nnz, >4k for
    complex128)."""
    from ..matrix import CSRMatrix
    cap = max(_expansion_bound(A, B), 1)
    # first hash tier sized to the average output row (AMG rows are tiny)
    cap0 = 64 if cap <= 48 * max(A.n_rows, 1) else 512
    ro, ci, va, big = _core.spgemm_hash(A.row_offsets, A.col_indices,
                                        A.values, B.row_offsets,
                                        B.col_indices, B.values, None, 0,
                                        cap, cap0)
    if int(ro[0].item()) == -1:   # a row exceeded the big hash capacity
        ro, ci, va = _core.spgemm(A.row_offsets, A.col_indices, A.values,
                                  B.row_offsets, B.col_indices, B.values,
                                  B.n_cols, cap)
        return CSRMatrix(ro, ci.contiguous(), va.contiguous(),
                         n_cols=B.n_cols)
    if big.numel():
        _sort_unsorted_rows(ro, ci, va, big)
    return CSRMatrix(ro, ci.contiguous(), va.contiguous(), n_cols=B.n_cols)


def transpose(A):
    from ..matrix import CSRMatrix
    ro, ci, va = _core.transpose(A.row_offsets, A.col_indices, A.values,
                                 A.n_cols)
    return CSRMatrix(ro, ci, va, n_cols=A.n_rows)


def galerkin_rap(R, A, P):
    AP = spgemm(A, P)
    return spgemm(R, AP)


def truncate_rows(P, trunc_factor: float = 0.0, max_elements: int = -1):
    """Drop |p| < factor*rowmax and/or cap rows at the top-max_elements
    entries by |value| (device kernels; reference src/truncate.cu)."""
    if not (0.0 < trunc_factor < 1.0):
        trunc_factor = 0.0
    if trunc_factor <= 0.0 and max_elements < 0:
        return P
    from ..matrix import CSRMatrix
    ro, ci, va = _core.truncate_rows(P.row_offsets, P.col_indices,
                                     P.values, float(trunc_factor),
                                     int(max_elements))
    return CSRMatrix(ro, ci.contiguous(), va.contiguous(), n_cols=P.n_cols)


# ---------------------------------------------------------------------- dense
def dense_solve(Ainv, b, x):
    _core.dense_gemv(Ainv, b.reshape(-1), x.reshape(-1))
    return x


# ---------------------------------------------------------------------- classical
def strength_ahat(A, theta=0.25, max_row_sum=1.1):
    return _core.strength_ahat(A.row_offsets, A.col_indices, A.values,
                               _didx(A), float(theta), float(max_row_sum))


def _pmis_graph(A, S):
    """(row_offsets, col_indices, tidx, strong) the PMIS kernels walk. They
    reach a neighbour j of i only through a stored entry (i, j) and its
    transpose index, which is all of S union S^T as long as every strong
    (j, i) has a stored (i, j). Where one has not (a nonsymmetric pattern),
    the kernels get the pattern of S union S^T itself, an entry flagged
    strong iff it is strong in S, so lambda and the neighbourhoods are those
    of the host."""
    n = A.n_rows
    ci, tidx = A.col_indices, _tidx(A)
    sym = A._cache.get("tidx_complete")
    if sym is None:     # the diagonal's transpose index is itself, never -1
        sym = not bool(((tidx < 0) & (ci < n)).any().item())
        A._cache["tidx_complete"] = sym
    if sym:
        return A.row_offsets, ci, tidx, S
    one_way = (S != 0) & (tidx < 0) & (ci < n)
    if not bool(one_way.any().item()):
        return A.row_offsets, ci, tidx, S
    dev = A.device
    ro64 = A.row_offsets.to(torch.int64)
    rows = torch.repeat_interleave(
        torch.arange(n, dtype=torch.int64, device=dev), ro64[1:] - ro64[:-1])
    ci64 = ci.to(torch.int64)
    sel = (S != 0) & (ci64 != rows) & (ci64 < n)
    r, c = rows[sel], ci64[sel]
    uk, inv = torch.unique(torch.cat([r * n + c, c * n + r]),
                           return_inverse=True)
    flag = torch.zeros(uk.numel(), dtype=torch.uint8, device=dev)
    flag[inv[:r.numel()]] = 1
    g_ro = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    g_ro[1:] = torch.cumsum(torch.bincount(uk // n, minlength=n),
                            0).to(torch.int32)
    g_ci = (uk % n).to(torch.int32).contiguous()
    return g_ro, g_ci, _core.trans_index(g_ro, g_ci, n), flag


def pmis_select(A, S):
    n = A.n_rows
    # the host's round guard: past it the binding raises, it never returns
    # undecided points
    guard = 8 * (int(math.log2(n + 2)) + 8)
    state = _core.pmis_select(*_pmis_graph(A, S), guard)
    cmask = state == 1
    cf = torch.full((n,), -1, dtype=torch.int32, device=A.device)
    csum = torch.cumsum(cmask.to(torch.int64), 0)
    cf[cmask] = (csum[cmask] - 1).to(torch.int32)
    return cf, int(cmask.sum().item())


def interp_d1(A, S, cf_map, num_coarse):
    from ..matrix import CSRMatrix
    counts = _core.interp_d1_count(A.row_offsets, A.col_indices, S, cf_map)
    p_ro = torch.zeros(A.n_rows + 1, dtype=torch.int32, device=A.device)
    p_ro[1:] = torch.cumsum(counts.to(torch.int64), 0).to(torch.int32)
    p_nnz = int(p_ro[-1].item())
    p_ro, p_ci, p_va = _core.interp_d1(A.row_offsets, A.col_indices, A.values,
                                       S, cf_map, _didx(A), p_ro, p_nnz)
    return CSRMatrix(p_ro, p_ci, p_va, n_cols=num_coarse)


# ---------------------------------------------------------------------- ILU(0)
def ilu0_setup(A, coloring):
    _check_block_dim(A, "ilu0_setup")
    pos = _slabs(A, coloring).slot_of_row
    if A.block_dim != 1:
        lu, dinv = _core.ilu0_setup_block(
            A.row_offsets, A.col_indices, A.values.reshape(-1), A.block_dim,
            _didx(A), pos, coloring.rows_sorted, coloring.bounds)
        return (lu, dinv)
    lu = _core.ilu0_setup(A.row_offsets, A.col_indices, A.values, _didx(A),
                          pos, coloring.rows_sorted, coloring.bounds)
    return lu


def ilu1_pattern(A, coloring):
    """Color-aware ILU(1) fill pattern with A's values embedded (see
    ops/cpu.py ilu1_pattern for the rule): LDS-hash count/fill kernels plus
    the embed kernel of kernels_spgemm.hip. A row wider than the top hash
    tier (ILU1_TOP_CAP columns) sends the whole build to the host builder."""
    from ..matrix import CSRMatrix
    colors = coloring.colors.to(torch.int32).contiguous()
    ro, ci, big = _core.ilu1_pattern(A.row_offsets, A.col_indices, colors,
                                     A.n_rows)
    if int(ro[0].item()) == -1:
        from . import cpu
        return cpu.ilu1_pattern(A.to("cpu"), coloring).to(A.device)
    if big.numel():
        _sort_unsorted_rows(ro, ci, None, big)
    bb = A.block_dim * A.block_dim
    va, _ = _core.ilu1_embed(A.row_offsets, A.col_indices,
                             A.values.reshape(-1), bb, ro, ci)
    if A.block_dim != 1:
        va = va.reshape(-1, A.block_dim, A.block_dim)
    return CSRMatrix(ro, ci, va, n_cols=A.n_cols, block_dim=A.block_dim)


def ilu0_solve(A, factors, coloring, r, x, relaxation=1.0):
    _check_block_dim(A, "ilu0_solve")
    n = A.n_cols * A.block_dim
    y = _scratch(A, "ilu_y", n, r.dtype)    # vector precision (dDFI mixed)
    z = _scratch(A, "ilu_z", n, r.dtype)
    st = _slabs(A, coloring)
    if A.block_dim != 1:
        lu, dinv = factors
        _core.ilu0_apply_block(A.row_offsets, A.col_indices, lu, dinv,
                               A.block_dim, st.slot_of_row,
                               coloring.rows_sorted, coloring.bounds,
                               r.reshape(-1), y, z, x.reshape(-1),
                               float(relaxation))
        return x
    # color-sorted slabs (same layout win as the DILU sweeps)
    lu_s, diag_s = _slab_copy(
        st, "ilu", factors, lambda f: (
            _gather_nz(f, st.nzmap),
            f.reshape(-1)[_didx(A).to(torch.int64)][st.perm]))
    _core.ilu0_apply_sorted(st.ro_s, st.ci_s, lu_s, diag_s, st.slot_of_row,
                            coloring.rows_sorted, coloring.bounds,
                            r.reshape(-1), y, z, x.reshape(-1),
                            float(relaxation))
    return x
