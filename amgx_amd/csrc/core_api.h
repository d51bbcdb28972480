// Launcher API of the gfx950 kernel library (implemented in *.hip TUs,
// called from bindings.cpp). Raw pointers + hipStream_t so the bindings TU
// compiles with the host compiler and the kernels with hipcc only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "cplx.h"

// ---- type lists ------------------------------------------------------------
// The one statement of which types the library is built for. The explicit
// instantiations at the end of each .hip file and the dispatch of
// bindings.cpp both expand these lists, so a launcher cannot be dispatched
// for a type it is not instantiated for. X is applied to each entry.
// Pairs are (TA, TV) = (matrix-value type, vector type): the reference's
// value modes dDDI, dFFI, dDFI and, complex, dZZI, dCCI, dZCI.
#define AMGX_REAL_TYPES(X) X(double) X(float)
#define AMGX_VALUE_TYPES(X) AMGX_REAL_TYPES(X) X(cplx<double>) X(cplx<float>)
#define AMGX_REAL_PAIRS(X) X(double, double) X(float, float) X(float, double)
#define AMGX_VALUE_PAIRS(X)                                                   \
    AMGX_REAL_PAIRS(X)                                                        \
    X(cplx<double>, cplx<double>)                                             \
    X(cplx<float>, cplx<float>)                                               \
    X(cplx<float>, cplx<double>)

// explicit instantiation of launcher F for one list entry; the signature is
// taken from the declaration below, so it is written once per .hip file
#define AMGX_INSTANTIATE(F, ...) template decltype(F<__VA_ARGS__>) F<__VA_ARGS__>;

namespace amgx_hip {

// Largest block size of the block smoother kernels (Jacobi, GS, DILU,
// ILU(0)): they keep a block, or one vector of block_dim components, in
// private arrays of this size, and the bindings reject anything larger
// before a launch. The block SpMV alone takes any block size.
constexpr int MAX_BLOCK_DIM = 16;

// ============================================================ kernels_solve.hip
// Launchers marked [value] are instantiated over the value types or value
// pairs (real and complex); all others over the real lists only. A [value]
// launcher with a block size argument runs complex types for b == 1 only
// and throws otherwise: the block kernels are real.

// ---- SpMV family -----------------------------------------------------------
// Mixed precision: TA = matrix-value type, TV = vector type. [value]
// y[i] = alpha * (A x)[i] + beta * y[i] + gamma * b[i]  over rows [r0, r1)
template <typename TA, typename TV>
void csrmv(const int* ro, const int* ci, const TA* va, const TV* x, TV* y,
           const TV* bvec, TV alpha, TV beta, TV gamma, int r0, int r1,
           double avg_deg, hipStream_t s);

// block-CSR variant; values (nnz, b, b) row-major. b == 4 and b in [2,8] run
// the wave kernels of kernels_mfma.hip, larger b bsrmv_generic
template <typename TA, typename TV>
void bsrmv(const int* ro, const int* ci, const TA* va, int b, const TV* x,
           TV* y, const TV* bvec, TV alpha, TV beta, TV gamma, int r0, int r1,
           hipStream_t s);

// baseline thread-per-row-component block SpMV (bench A/B target)
template <typename TA, typename TV>
void bsrmv_generic(const int* ro, const int* ci, const TA* va, int b,
                   const TV* x, TV* y, const TV* bvec, TV alpha, TV beta,
                   TV gamma, int r0, int r1, hipStream_t s);

// ---- BLAS-1 ----------------------------------------------------------------
// Deterministic two-stage reduction over a fixed tree. [value]
// op 0 = sum conj(x) y (the plain dot for real T), 1 = sum|x|, 2 = max|x|,
// 3 = sum|x|^2; any other op throws. out (device scalar) and ws (device
// scratch of >= 2048 elements) are of the partial type: T for op 0,
// real_of<T> for ops 1 to 3. y is read by op 0 only.
template <typename T>
void reduce(const T* x, const T* y, long long n, int op, void* ws, void* out,
            hipStream_t s);

// axpy / axpby / scal: [value]; axpy_dalpha and scal_drsqrt are real-only.
template <typename T>
void axpy(T* y, const T* x, T a, long long n, hipStream_t s);
template <typename T>
void axpy_dalpha(T* y, const T* x, const T* alpha, T scale, long long n,
                 hipStream_t s);
template <typename T>
void scal_drsqrt(T* x, const T* s2, long long n, hipStream_t s);
template <typename T>
void axpby(T* y, const T* x, T a, T b, long long n, hipStream_t s);
template <typename T>
void scal(T* x, T a, long long n, hipStream_t s);

// ---- structure -------------------------------------------------------------
void diag_index(const int* ro, const int* ci, int n, int* out, hipStream_t s);
// [value]
template <typename T>
void extract_diag(const T* va, const int* didx, int n, int b, T* out,
                  hipStream_t s);
void trans_index(const int* ro, const int* ci, int n, int* out, hipStream_t s);

// ---- smoothers -------------------------------------------------------------
// inverse (block) diagonal, d == 0 gives 1; l1 adds the off-diagonal row sum
// of |a_ij| (ro is read only then). [value]: complex T is scalar and plain
// only, b > 1 or l1 throws.
template <typename T>
void jacobi_dinv(const int* ro, const T* va, const int* didx, int n, int b,
                 bool l1, T* dinv, hipStream_t s);
// xo = xi + omega * dinv * (b - A xi)   (block-aware; b=1 scalar fast path).
// [value]
template <typename TA, typename TV>
void jacobi_smooth(const int* ro, const int* ci, const TA* va, const TA* dinv,
                   const TV* bvec, const TV* xi, TV* xo, TV omega, int n,
                   int b, hipStream_t s);
// in-place GS update of rows[count]: x[r] += omega*dinv[r]*(b - A x)[r].
// [value]
template <typename TA, typename TV>
void gs_smooth_rows(const int* ro, const int* ci, const TA* va,
                    const TA* dinv, const TV* bvec, TV* x, const int* rows,
                    int count, TV omega, int n, int b, hipStream_t s);

// ---- color-sorted sweeps (reorder-by-color layout) -------------------------
// Matrix arrays are the rows_sorted-gathered copy, so each color reads one
// contiguous slab. Levels of at most SMALL_LEVEL_ROWS rows (GS) or
// DILU_SMALL_ROWS rows (scalar DILU) run the whole sweep in one
// single-workgroup launch (*_small); larger levels launch once per color
// with ro_s/rows/dinv_s/einv_s pre-offset to the color base.
// All [value]; Einv is held in the matrix type.
constexpr int SMALL_LEVEL_ROWS = 1 << 14;

template <typename TA, typename TV>
void gs_sweep_small(const int* ro_s, const int* ci_s, const TA* va_s,
                    const TA* dinv_s, const TV* bvec, TV* x, const int* rows,
                    const int* bounds, int ncolors, TV omega, bool symmetric,
                    hipStream_t s);
template <typename TA, typename TV>
void gs_rows_sorted(const int* ro_s, const int* ci_s, const TA* va_s,
                    const TA* dinv_s, const TV* bvec, TV* x, const int* rows,
                    int count, TV omega, hipStream_t s);

// DILU: x += relax * M^{-1} rhs.  Fused-residual form: rhs = b and the
// forward sweep folds the residual in, so M^{-1}(b - A x) costs one matrix
// read less; scalar and block-4 only.
// `sweeps` whole applies for a small scalar level in one single-workgroup
// launch, with the row rules (and bits) of the per-color sweeps below: fused
// sweeps the full slab (ro_f, ci_f, va_f), with y = x + 0 over vec_n entries
// written by the kernel at each apply; plain sweeps the L slab (same
// arguments, y unused); backward over U. lanes_f / lanes_u: 1 or 8 lanes per
// row of the forward / backward slab.
// Levels of at most DILU_SMALL_ROWS rows take it; the boundary is the
// measured crossover with the per-color path, whose three sweeps cost about
// the same 0.3 ms of launches from 1400 to 27000 rows while one workgroup's
// time grows with the rows (profiles/NOTES.md, "DILU one-launch apply of
// small levels").
constexpr int DILU_SMALL_ROWS = 1 << 10;
template <typename TA, typename TV>
void dilu_small(const int* ro_f, const int* ci_f, const TA* va_f,
                const int* ro_u, const int* ci_u, const TA* va_u,
                const TA* einv_s, const int* rows, const int* bounds,
                int ncolors, const TV* rhs, TV* w, TV* y, TV* x, TV relax,
                long long vec_n, bool fused, int lanes_f, int lanes_u,
                int sweeps, hipStream_t s);
// the one-launch apply in its earlier form, for tests and bench_kernels.py:
// thread per row over the full slab in both sweeps, w and z zeroed at each
// apply, the relaxed axpy a pass of its own. Same bits as dilu_small.
template <typename TA, typename TV>
void dilu_small_full(const int* ro_s, const int* ci_s, const TA* va_s,
                     const TA* einv_s, const int* rows, const int* bounds,
                     int ncolors, const TV* rhs, TV* w, TV* z, TV* x,
                     TV relax, long long vec_n, bool fused, hipStream_t s);
// block matrices only; xres (block-4) folds the residual in by gathering
// xres + w over a pre-zeroed w
template <typename TA, typename TV>
void dilu_fwd_sorted(const int* ro_s, const int* ci_s, const TA* va_s,
                     const TA* einv_s, const int* rows, int count,
                     const TV* rhs, const TV* xres /* nullptr = plain */,
                     TV* w, int b, hipStream_t s);
template <typename TA, typename TV>
void dilu_bwd_sorted(const int* ro_s, const int* ci_s, const TA* va_s,
                     const TA* einv_s, const int* rows, int count,
                     const TV* wv, TV* z, int b, hipStream_t s);
// Scalar per-color sweeps; ro_* / rows / einv_s pre-offset to the color base.
// Each is one row rule; neither w nor y needs zeroing.
//   dilu_fwd_full, over the full slab: w_i = Einv_i (rhs_i - sum a_ij y_j),
//     y_i = x_i + w_i, after dilu_y_init has written y = x + 0 over the
//     column-extended length once per apply.
//   dilu_fwd_lower, over the strict color-split L slab (slab_split_*):
//     w_i = Einv_i (rhs_i - sum_L a_ij w_j).
//   dilu_bwd_upper, over the U slab, in place: z_i = w_i - Einv_i sum_U
//     a_ij w_j stored to w[i], with x[i] += relax * z_i folded in.
// lanes = 1 or 8 lanes per row; lanes = DILU_STREAM selects the stream form
// (all the same bits): a wave takes DILU_STREAM_ROWS consecutive rows of the
// color, one lane per row, and streams their contiguous entries through a
// wave-private LDS window of DILU_STREAM_WINDOW_BYTES bytes, which holds
// dilu_stream_window_of(bytes of one value and one gathered vector entry)
// entries: 512 in fp64 and with an fp32 matrix, 256 in complex128.
constexpr int DILU_STREAM = 64;
constexpr int DILU_STREAM_ROWS = 64;
constexpr int DILU_STREAM_WINDOW_BYTES = 8192;
constexpr int DILU_STREAM_WINDOW = 512;
constexpr int dilu_stream_window_of(int pair_bytes) {
    int w = DILU_STREAM_WINDOW_BYTES / pair_bytes;
    w -= w % 64;
    return w < DILU_STREAM_WINDOW ? w : DILU_STREAM_WINDOW;
}
template <typename TV>
void dilu_y_init(const TV* x, TV* y, long long n, hipStream_t s);
template <typename TA, typename TV>
void dilu_fwd_full(const int* ro_s, const int* ci_s, const TA* va_s,
                   const TA* einv_s, const int* rows, int count,
                   const TV* rhs, const TV* x, TV* w, TV* y, int lanes,
                   hipStream_t s);
template <typename TA, typename TV>
void dilu_fwd_lower(const int* ro_l, const int* ci_l, const TA* va_l,
                    const TA* einv_s, const int* rows, int count,
                    const TV* rhs, TV* w, int lanes, hipStream_t s);
template <typename TA, typename TV>
void dilu_bwd_upper(const int* ro_u, const int* ci_u, const TA* va_u,
                    const TA* einv_s, const int* rows, int count, TV* w,
                    TV* x, TV relax, int lanes, hipStream_t s);
// Einv of the rows of one color (colors ascending)
template <typename T>
void dilu_setup_color(const int* ro, const int* ci, const T* va,
                      const int* didx, const int* tidx, const int* colors,
                      const int* rows, int count, int color, T* einv, int b,
                      hipStream_t s);

// ---- transfer operators ----------------------------------------------------
// [value]
template <typename T>
void restrict_agg(const T* r, const int* agg, int n, int b, T* rc,
                  hipStream_t s);
// deterministic variant over the aggregate-CSR structure
template <typename T>
void restrict_csr(const int* off, const int* fids, const T* r, int nc, int b,
                  T* rc, hipStream_t s);
template <typename T>
void prolongate_agg(T* x, const T* xc, const int* agg, int n, int b,
                    hipStream_t s);

// ---- dense coarse solve ----------------------------------------------------
// [value]
template <typename TA, typename TV>
void dense_gemv(const TA* Ainv, const TV* b, TV* x, int n, hipStream_t s);

// ---- gather for halo pack and the color-sorted slab copies ------------------
// [value]
template <typename T>
void gather(const T* src, const int* idx, int count, int b, T* dst,
            hipStream_t s);

// ============================================================ kernels_mfma.hip
// MFMA wave-structured block kernels
// v_mfma_f64_4x4x4_4b_f64 path: wave = 4 rows x 16 lanes, coalesced block
// loads; used automatically by the b==4 dispatch of bsrmv/dilu_* above.
void mfma4_probe(const double* a, const double* b, double* c, hipStream_t s);
template <typename TA, typename TV>
void bsrmv_b4(const int* ro, const int* ci, const TA* va, const TV* x, TV* y,
              const TV* bvec, double alpha, double beta, double gamma,
              int row_begin, int row_end, hipStream_t s);
template <typename TA, typename TV>
void bsrmv_bn(const int* ro, const int* ci, const TA* va, int b, const TV* x,
              TV* y, const TV* bvec, double alpha, double beta, double gamma,
              int row_begin, int row_end, hipStream_t s);
template <typename TA, typename TV>
void dilu_fwd_b4_sorted(const int* ro_s, const int* ci_s, const TA* va_s,
                        const TA* einv_s, const int* rows, int count,
                        const TV* r, const TV* xres /* nullptr = plain */,
                        TV* w, hipStream_t s);
template <typename TA, typename TV>
void dilu_bwd_b4_sorted(const int* ro_s, const int* ci_s, const TA* va_s,
                        const TA* einv_s, const int* rows, int count,
                        const TV* w, TV* z, hipStream_t s);
template <typename TA>
void dilu_setup_b4(const int* ro, const int* ci, const TA* va,
                   const int* didx, const int* tidx, const int* colors,
                   const int* rows, int count, int color, TA* einv,
                   hipStream_t s);

// ============================================================ kernels_setup.hip
// ---- coloring --------------------------------------------------------------
// one min-max hash round; *left (zeroed by the caller) becomes 1 when a row
// stays uncolored. A round on a fully colored graph copies the colors.
void color_minmax_round(const int* ro, const int* ci, int n,
                        const int* colors_prev, int* colors_next, int iter,
                        int seed, int mode, int* left, hipStream_t s);
// *out = max(*out, v[0..n))
void int_max(const int* v, int n, int* out, hipStream_t s);

// ---- aggregation -----------------------------------------------------------
// agg_propose / agg_merge_singletons: [value]; the edge weight of a complex
// entry is its modulus, taken in double
// wpre: the weights of agg_edge_weights (one double per entry), or nullptr to
// compute each weight from va, tidx and diag; the same proposals either way
template <typename T>
void agg_propose(const int* ro, const int* ci, const T* va, const int* tidx,
                 const T* diag, const double* wpre, int n, const int* agg,
                 int* prop, int seed, hipStream_t s);
template <typename T>
void agg_edge_weights(const int* ro, const int* ci, const T* va,
                      const int* tidx, const T* diag, int n, double* w,
                      hipStream_t s);
// *changed (zeroed by the caller) becomes 1 when the round forms a pair
void agg_match(const int* prop, int n, int* agg, int* changed, hipStream_t s);
template <typename T>
void agg_merge_singletons(const int* ro, const int* ci, const T* va,
                          const int* tidx, const T* diag, int n,
                          const int* agg_in, int* agg_out, hipStream_t s);

// ---- MULTI_PAIRWISE ----------------------------------------------------------
// Matching on a weight graph w[nnz] over the structure (ro, ci) of n rows;
// entries with w > 0 are edges, compared by (w, hash of the pair, lo, hi).
// State: agg[i] = root row of i's aggregate or -1, sizes[i] = size of a
// root's aggregate or of an unaggregated row. No launcher allocates or
// synchronizes; scratch comes from the caller.
// pairwise_weights: [value]; formula 0 = 0.5(|a_ij|+|a_ji|)/max(|a_ii|,|a_jj|)
// (complex: moduli in double), 1 = -0.5(a_ij/a_ii + a_ji/a_jj) (real only)
template <typename T>
void pairwise_weights(const int* ro, const int* ci, const T* va,
                      const int* tidx, const T* diag, int n, int formula,
                      double* w, hipStream_t s);
// lanes per row: 1 or 8; both write the same prop
void pairwise_propose(const int* ro, const int* ci, const double* w, int n,
                      const int* agg, const int* sizes, int cap, int seed,
                      int lanes, int* prop, hipStream_t s);
void pairwise_match(const int* prop, int n, int* agg, int* sizes,
                    hipStream_t s);
// *count += number of rows with agg < 0
void pairwise_count_unaggregated(const int* agg, int n, int* count,
                                 hipStream_t s);
// merge_singletons = 1: one double-buffered sweep agg_in -> agg_out
void pairwise_join_sweep(const int* ro, const int* ci, const double* w, int n,
                         const int* agg_in, int seed, int* agg_out,
                         hipStream_t s);
// merge_singletons = 2: one capped round (bid, tie-break, accept). bid_root
// (n) is scratch; bid_w (n) must be 0 and bid_i (n) must be n on entry and
// are left so.
void pairwise_join_capped(const int* ro, const int* ci, const double* w, int n,
                          int* agg, int* sizes, int cap, int seed,
                          int* bid_root, unsigned long long* bid_w, int* bid_i,
                          hipStream_t s);
// Roots (agg[i] == i, rows still at -1 included) get consecutive ids in
// ascending order: agg_out[i] = id of i's root, sizes_out[id] (zeroed by the
// caller) = sum of sizes_in over the members. ids: n + 1 ints of scratch,
// ids[n] = number of aggregates afterwards; tmp: pairwise_renumber_tmp_bytes.
size_t pairwise_renumber_tmp_bytes(int n);
void pairwise_renumber(int* agg, int n, const int* sizes_in, int* ids,
                       void* tmp, size_t tmp_bytes, int* agg_out,
                       int* sizes_out, hipStream_t s);

// ============================================================ kernels_order.hip
// Stable order of n rows by an int32 key in [0, nkeys): order (n) = rows
// sorted by key, ascending within a key; off (nkeys + 1) = first position of
// each key, off[nkeys] = n. The values of torch.argsort(stable=True) and of
// bincount + cumsum, from one radix sort over the key bits in use.
void key_order(const int* keys, int n, int nkeys, int* order, int* off,
               hipStream_t s);
// Matching roots (roots[r] == r exactly at the roots) to consecutive ids in
// ascending root order: agg[i] = id of roots[i]. ids: n + 1 ints of scratch,
// ids[n] = number of roots afterwards. No sort.
void root_renumber(const int* roots, int n, int* ids, int* agg,
                   hipStream_t s);
// Structure of the slab whose row t is row rows[t] of (ro, ci).
// slab_offsets: ro_s (n + 1) and slot_of_row (n, inverse of rows); returns
// ro_s[n] (one host sync). slab_fill: nzmap[ro_s[t] + e] = ro[rows[t]] + e
// and ci_s = ci[nzmap], by 1 or 8 lanes per row.
long long slab_offsets(const int* ro, const int* rows, int n, int* ro_s,
                       int* slot_of_row, hipStream_t s);
void slab_fill(const int* ro, const int* ci, const int* rows, int n,
               int lanes, const int* ro_s, int* nzmap, int* ci_s,
               hipStream_t s);

// ============================================================ kernels_setup.hip
// ---- strict color-split of a color-sorted slab -------------------------------
// The U (upper) / L part of slot t keeps, in slab order, the entries with a
// local column j < n of a later / earlier color than the row's; diagonal,
// same-color and halo entries belong to neither. rows = rows_sorted, colors
// per row (n entries).
// count + scan: fills ro_x (n+1) and returns the part's nnz (one host sync)
long long slab_split_count(const int* ro_s, const int* ci_s, const int* rows,
                           const int* colors, int n, bool upper, int* ro_x,
                           hipStream_t s);
// fill: columns ci_x and map_x = position of each kept entry in the full slab
void slab_split_fill(const int* ro_s, const int* ci_s, const int* rows,
                     const int* colors, int n, bool upper, const int* ro_x,
                     int* ci_x, int* map_x, hipStream_t s);

// ---- SpGEMM / Galerkin -----------------------------------------------------
// Aggregation Galerkin: COO keys agg[i]*nc+agg[j] -> radix sort ->
// reduce_by_key -> CSR. Returns nnz_c; fills ro_c (nc+1); ci_c/va_c are
// caller-allocated at worst case nnz (nnz_c <= nnz) and trimmed after.
// bb = block_dim^2 (1 for scalar). Temps allocated internally (setup-time).
// agg = per-ROW local coarse id (n entries); agg_col = per-COLUMN coarse id
// (n_cols entries; equals agg for single-process, GLOBAL coarse ids for the
// distributed path); nc = local coarse rows (ro_c size); ncmod = column-id
// modulus (global coarse columns). [value], complex for bb == 1 only.
template <typename T>
long long galerkin_agg(const int* ro, const int* ci, const T* va, int n,
                       long long nnz, const int* agg, const int* agg_col,
                       int nc, long long ncmod, int* ro_c, int* ci_c, T* va_c,
                       int bb, hipStream_t s);

// General ESC SpGEMM: C = A(m x k) @ B(k x n). Outputs sized by caller at
// the expansion worst case is impractical; instead ci_c/va_c must be sized
// >= nnz(C); pass capacity = expansion bound from Python (sum deg). Returns
// nnz_c. Temps allocated internally. [value]
template <typename T>
long long spgemm_esc(const int* roA, const int* ciA, const T* vaA, int m,
                     long long nnzA, const int* roB, const int* ciB,
                     const T* vaB, int k, int n, int* ro_c, int* ci_c, T* va_c,
                     hipStream_t s);

// CSR transpose via stable radix sort on column ids.
template <typename T>
void transpose_csr(const int* ro, const int* ci, const T* va, int m, int n,
                   long long nnz, int* ro_t, int* ci_t, T* va_t,
                   hipStream_t s);

// ============================================================ kernels_spgemm.hip
// LDS-hash SpGEMM
// mode 0: C = A*B.  mode 1: aggregation Galerkin — A = aggregate-membership
// CSR (coarse row -> fine rows), B = fine matrix, key = aggcol[col].
// Returns nnz(C), or -1 when a row exceeds the top-tier capacity of T (caller
// falls back to the ESC sort path), or -2 when cap_nnz is too small.
// Instantiated over the value types.
// The top tier is one wave per workgroup with one key + one value array in
// LDS: 8192 entries for values of up to 8 bytes (96 KB), 4096 for
// cplx<double> (80 KB; 8192 x 20 B would take all 160 KB of a CU).
template <typename T>
constexpr int spgemm_hash_top_cap() { return sizeof(T) > 8 ? 4096 : 8192; }
// big_rows_out (device, caller frees via free_device_buf) lists rows whose
// entries were written UNSORTED (caller sorts those columns).
template <typename T>
long long spgemm_hash(const int* roA, const int* ciA, const T* vaA, int m,
                      const int* roB, const int* ciB, const T* vaB,
                      const int* aggcol, int mode, int cap0, int* roC_out,
                      int* ciC_cap_buf, T* vaC_cap_buf, long long cap_nnz,
                      int** big_rows_out, int* n_big_out, hipStream_t s);
void free_device_buf(void* p, hipStream_t s);

// ---- color-aware ILU(1) fill pattern ----------------------------------------
// Row i of the pattern = A's row i (halo columns included) + i + every local
// j reached through a local pivot k of A's row i with colors[k] < colors[i],
// (k, j) in A, colors[j] > colors[k] and colors[j] != colors[i]. Same
// 64 -> 512 -> top ladder as spgemm_hash; the top tier holds ILU1_TOP_CAP
// columns (keys only, 32 KB of LDS).
constexpr int ILU1_TOP_CAP = 8192;
// device row lists of the upper tiers, produced by the count pass
struct Ilu1Tiers {
    int* mid_rows = nullptr;   // rows past the 64 tier
    int n_mid = 0;
    int* big_rows = nullptr;   // rows past the 512 tier: written UNSORTED
    int n_big = 0;
};
// count + scan: fills roC_out (n+1) and *tiers, returns the pattern's nnz, or
// -1 (tiers freed) when a row exceeds ILU1_TOP_CAP
long long ilu1_pattern_count(const int* ro, const int* ci, const int* colors,
                             int n, int* roC_out, Ilu1Tiers* tiers,
                             hipStream_t s);
// fill: ciC (nnz of the count pass), rows ascending except tiers.big_rows
void ilu1_pattern_fill(const int* ro, const int* ci, const int* colors, int n,
                       const int* roC, int* ciC, const Ilu1Tiers& tiers,
                       hipStream_t s);
void ilu1_tiers_free(Ilu1Tiers* tiers, hipStream_t s);
// vaL[a_to_lu[k]] = vaA[k] (bb values each) for every entry k of A, where
// a_to_lu[k] is the slot of A's entry in the sorted pattern (roL, ciL); vaL is
// zero-initialised by the caller. Real types.
template <typename T>
void ilu1_embed(const int* roA, const int* ciA, const T* vaA, int n,
                long long nnzA, int bb, const int* roL, const int* ciL,
                T* vaL, int* a_to_lu, hipStream_t s);

// ============================================================ kernels_classical.hip
// ---- classical setup -------------------------------------------------------
template <typename T>
void strength_ahat(const int* ro, const int* ci, const T* va, const int* didx,
                   int n, double theta, double max_row_sum,
                   unsigned char* strong, hipStream_t s);
void pmis_lambda(const int* ro, const int* ci, const int* tidx,
                 const unsigned char* strong, int n, float* w, hipStream_t s);
void pmis_mark_isolated(const int* ro, const int* ci, const int* tidx,
                        const unsigned char* strong, int n, signed char* state,
                        hipStream_t s);
void pmis_one_round(const int* ro, const int* ci, const int* tidx,
                    const unsigned char* strong, int n, const float* w,
                    const signed char* state, signed char* state_mid,
                    signed char* state_out, int* n_undecided, hipStream_t s);
void interp_d1_count(const int* ro, const int* ci, const unsigned char* strong,
                     const int* cf, int n, int ncols, int* counts,
                     hipStream_t s);
template <typename T>
void interp_d1(const int* ro, const int* ci, const T* va,
               const unsigned char* strong, const int* cf, const int* didx,
               const int* p_ro, int n, int ncols, int* p_ci, T* p_va,
               hipStream_t s);

// ---- ILU(0) ----------------------------------------------------------------
template <typename T>
void ilu0_factor_color_launch(const int* ro, const int* ci, const int* pos,
                              const int* didx, const int* rows, int count,
                              T* lu, int n, hipStream_t s);
// color-sorted ILU(0) sweeps (reorder-by-color slabs)
template <typename TA, typename TV>
void ilu0_fwd_sorted(const int* ro_s, const int* ci_s, const TA* lu_s,
                     const int* pos, const int* rows, int count, const TV* r,
                     TV* y, int n, hipStream_t s);
template <typename TA, typename TV>
void ilu0_bwd_sorted(const int* ro_s, const int* ci_s, const TA* lu_s,
                     const TA* diag_s, const int* pos, const int* rows,
                     int count, const TV* y, TV* z, int n, hipStream_t s);
// block ILU(0): L_ik = A_ik U_kk^{-1}, A_ij -= L_ik U_kj; dinv = inverted
// pivot diagonal blocks, refreshed per color via ilu0_invert_diag_block
template <typename T>
void ilu0_factor_color_block_launch(const int* ro, const int* ci,
                                    const int* pos, const int* didx,
                                    const int* rows, int count, T* lu,
                                    const T* dinv, int n, int b,
                                    hipStream_t s);
template <typename T>
void ilu0_invert_diag_block_launch(const int* didx, const int* rows,
                                   int count, const T* lu, T* dinv, int b,
                                   hipStream_t s);
template <typename TA, typename TV>
void ilu0_fwd_block_launch(const int* ro, const int* ci, const int* pos,
                           const TA* lu, const int* rows, int count,
                           const TV* r, TV* y, int n, int b, hipStream_t s);
template <typename TA, typename TV>
void ilu0_bwd_block_launch(const int* ro, const int* ci, const int* pos,
                           const TA* lu, const TA* dinv, const int* rows,
                           int count, const TV* y, TV* z, int n, int b,
                           hipStream_t s);

// ---- truncate --------------------------------------------------------------
template <typename T>
void truncate_rows_gpu(const int* ro, const int* ci, const T* va, int n,
                       double factor, int max_elem, const int* ro_out,
                       int* ci_out, T* va_out, int* counts, hipStream_t s);
template <typename T>
void truncate_fill_gpu(const int* ro, const int* ci, const T* va, int n,
                       double factor, int max_elem, const int* ro_out,
                       int* ci_out, T* va_out, hipStream_t s);
}  // namespace amgx_hip
