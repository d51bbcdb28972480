// Classical Ruge-Stueben setup kernels: AHAT strength, PMIS C/F selection,
// distance-1 (direct) interpolation, and multicolor ILU(0).
//
// Reference behaviors: src/classical/strength/strength_base.cu (AHAT),
// src/classical/selectors/pmis.cu (random-weight independent-set rounds),
// src/classical/interpolators/distance1.cu (direct interpolation with
// pos/neg splitting), src/solvers/multicolor_ilu_solver.cu (color-ordered
// ILU(0) with color-parallel triangular sweeps).

#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "common.h"
#include "core_api.h"

namespace amgx_hip {

// ============================================================ strength (AHAT)
// strong iff |a_ij| >= theta * max_{k!=i}|a_ik|; optional all-weak rows when
// |row sum| > max_row_sum * |a_ii|.
template <typename T>
__global__ __launch_bounds__(AMGX_BLOCK) void strength_kernel(const int* __restrict__ ro,
                                const int* __restrict__ ci,
                                const T* __restrict__ va,
                                const int* __restrict__ didx, int n,
                                double theta, double max_row_sum,
                                unsigned char* __restrict__ strong) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int s = ro[i], e = ro[i + 1];
    double mx = 0.0, rs = 0.0;
    for (int k = s; k < e; ++k) {
        double a = (double)va[k];
        rs += a;
        if (ci[k] != i) mx = fmax(mx, fabs(a));
    }
    bool weak_row = false;
    if (max_row_sum < 1.0) {
        int dk = didx[i];
        double d = dk >= 0 ? fabs((double)va[dk]) : 1.0;
        if (d == 0.0) d = 1.0;
        weak_row = fabs(rs) > max_row_sum * d;
    }
    for (int k = s; k < e; ++k) {
        bool st = !weak_row && ci[k] != i && mx > 0.0 &&
                  fabs((double)va[k]) >= theta * mx;
        strong[k] = st ? 1 : 0;
    }
}

template <typename T>
void strength_ahat(const int* ro, const int* ci, const T* va, const int* didx,
                   int n, double theta, double max_row_sum,
                   unsigned char* strong, hipStream_t s) {
    hipLaunchKernelGGL((strength_kernel<T>), dim3(grid_1d(n)),
                       dim3(AMGX_BLOCK), 0, s, ro, ci, va, didx, n, theta,
                       max_row_sum, strong);
}

// ============================================================ PMIS
// Strong graph = S union S^T via the transpose-entry index: a neighbor j of
// i is seen only through a stored entry (i, j), so the caller passes a
// pattern in which every strong (j, i) has one (ops/gpu.py adds them where
// A's pattern is not symmetric). lambda_i = #strong dependents. One round:
// undecided local maxima of (lambda + hash) become C; undecided strong
// neighbors of new C become F.
__device__ __forceinline__ unsigned int pmis_hash(unsigned int a) {
    a = (a ^ 61u) ^ (a >> 16);
    a *= 9u;
    a ^= a >> 4;
    a *= 0x27d4eb2du;
    a ^= a >> 15;
    return a;
}

__global__ __launch_bounds__(AMGX_BLOCK) void pmis_lambda_kernel(const int* __restrict__ ro,
                                   const int* __restrict__ ci,
                                   const int* __restrict__ tidx,
                                   const unsigned char* __restrict__ strong,
                                   int n, float* __restrict__ w) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int lam = 0;
    for (int k = ro[i]; k < ro[i + 1]; ++k) {
        int tk = tidx[k];
        // j depends strongly on i <=> entry (j,i) is strong
        if (tk >= 0 && strong[tk]) ++lam;
    }
    w[i] = (float)lam + (float)(pmis_hash((unsigned)i) & 0xffff) / 65536.0f;
}

// state: 0 undecided, 1 C, -1 F
__global__ __launch_bounds__(AMGX_BLOCK) void pmis_round1(const int* __restrict__ ro,
                            const int* __restrict__ ci,
                            const int* __restrict__ tidx,
                            const unsigned char* __restrict__ strong, int n,
                            const float* __restrict__ w,
                            const signed char* __restrict__ state,
                            signed char* __restrict__ state_out,
                            int* __restrict__ n_undecided) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    signed char st = state[i];
    if (st != 0) { state_out[i] = st; return; }
    bool ismax = true;
    float wi = w[i];
    for (int k = ro[i]; k < ro[i + 1]; ++k) {
        int j = ci[k];
        if (j == i || j >= n) continue;
        int tk = tidx[k];
        bool edge = strong[k] || (tk >= 0 && strong[tk]);
        if (!edge || state[j] != 0) continue;
        float wj = w[j];
        if (wj > wi || (wj == wi && j > i)) { ismax = false; break; }
    }
    state_out[i] = ismax ? 1 : 0;
    if (!ismax) atomicAdd(n_undecided, 1);
}

__global__ __launch_bounds__(AMGX_BLOCK) void pmis_round2(const int* __restrict__ ro,
                            const int* __restrict__ ci,
                            const int* __restrict__ tidx,
                            const unsigned char* __restrict__ strong, int n,
                            const signed char* __restrict__ state,
                            signed char* __restrict__ state_out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    signed char st = state[i];
    if (st != 0) { state_out[i] = st; return; }
    for (int k = ro[i]; k < ro[i + 1]; ++k) {
        int j = ci[k];
        if (j == i || j >= n) continue;
        int tk = tidx[k];
        bool edge = strong[k] || (tk >= 0 && strong[tk]);
        if (edge && state[j] == 1) { state_out[i] = -1; return; }
    }
    state_out[i] = 0;
}

// isolated rows (no strong edges either way) -> F
__global__ __launch_bounds__(AMGX_BLOCK) void pmis_isolated(const int* __restrict__ ro,
                              const int* __restrict__ ci,
                              const int* __restrict__ tidx,
                              const unsigned char* __restrict__ strong, int n,
                              signed char* __restrict__ state) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int k = ro[i]; k < ro[i + 1]; ++k) {
        int tk = tidx[k];
        if (ci[k] != i && ci[k] < n && (strong[k] || (tk >= 0 && strong[tk])))
            return;
    }
    state[i] = -1;
}

void pmis_lambda(const int* ro, const int* ci, const int* tidx,
                 const unsigned char* strong, int n, float* w, hipStream_t s) {
    hipLaunchKernelGGL(pmis_lambda_kernel, dim3(grid_1d(n)), dim3(AMGX_BLOCK),
                       0, s, ro, ci, tidx, strong, n, w);
}
void pmis_mark_isolated(const int* ro, const int* ci, const int* tidx,
                        const unsigned char* strong, int n, signed char* state,
                        hipStream_t s) {
    hipLaunchKernelGGL(pmis_isolated, dim3(grid_1d(n)), dim3(AMGX_BLOCK), 0, s,
                       ro, ci, tidx, strong, n, state);
}
void pmis_one_round(const int* ro, const int* ci, const int* tidx,
                    const unsigned char* strong, int n, const float* w,
                    const signed char* state, signed char* state_mid,
                    signed char* state_out, int* n_undecided, hipStream_t s) {
    hipLaunchKernelGGL(pmis_round1, dim3(grid_1d(n)), dim3(AMGX_BLOCK), 0, s,
                       ro, ci, tidx, strong, n, w, state, state_mid,
                       n_undecided);
    hipLaunchKernelGGL(pmis_round2, dim3(grid_1d(n)), dim3(AMGX_BLOCK), 0, s,
                       ro, ci, tidx, strong, n, state_mid, state_out);
}

// ============================================================ D1 interpolation
// count pass: C rows -> 1 entry; F rows -> #strong C neighbors
// cf spans ncols entries (= n for single-process, n_local+n_halo with
// GLOBAL coarse ids for the distributed path)
__global__ __launch_bounds__(AMGX_BLOCK) void d1_count(const int* __restrict__ ro,
                         const int* __restrict__ ci,
                         const unsigned char* __restrict__ strong,
                         const int* __restrict__ cf, int n, int ncols,
                         int* __restrict__ counts) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (cf[i] >= 0) { counts[i] = 1; return; }
    int c = 0;
    for (int k = ro[i]; k < ro[i + 1]; ++k)
        if (strong[k] && ci[k] < ncols && cf[ci[k]] >= 0) ++c;
    counts[i] = c;
}

// fill pass: direct interpolation with pos/neg splitting (reference
// src/classical/interpolators/distance1.cu):
//   alpha = sum_neg(all) / sum_neg(strong C), beta likewise for positives;
//   positives lumped into the diagonal when no positive C connection;
//   a row whose diagonal is zero after that lumping gets zero weights.
template <typename T>
__global__ __launch_bounds__(AMGX_BLOCK) void d1_fill(const int* __restrict__ ro, const int* __restrict__ ci,
                        const T* __restrict__ va,
                        const unsigned char* __restrict__ strong,
                        const int* __restrict__ cf, const int* __restrict__ didx,
                        const int* __restrict__ p_ro, int n, int ncols,
                        int* __restrict__ p_ci, T* __restrict__ p_va) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int out = p_ro[i];
    if (cf[i] >= 0) {
        p_ci[out] = cf[i];
        p_va[out] = T(1);
        return;
    }
    int s = ro[i], e = ro[i + 1];
    int dk = didx[i];
    double diag = dk >= 0 ? (double)va[dk] : 0.0;
    double neg_all = 0.0, pos_all = 0.0, neg_c = 0.0, pos_c = 0.0;
    for (int k = s; k < e; ++k) {
        if (ci[k] == i) continue;
        double a = (double)va[k];
        if (a < 0) neg_all += a; else pos_all += a;
        if (strong[k] && ci[k] < ncols && cf[ci[k]] >= 0) {
            if (a < 0) neg_c += a; else pos_c += a;
        }
    }
    if (pos_c == 0.0) { diag += pos_all; pos_all = 0.0; }
    if (diag == 0.0) {
        // degenerate row (zero diagonal after lumping, as on the host):
        // emit zero weights for its counted slots
        for (int k = s; k < e; ++k) {
            if (ci[k] == i || !strong[k] || ci[k] >= ncols || cf[ci[k]] < 0)
                continue;
            p_ci[out] = cf[ci[k]];
            p_va[out] = T(0);
            ++out;
        }
        return;
    }
    double alpha = neg_c != 0.0 ? neg_all / neg_c : 0.0;
    double beta = pos_c != 0.0 ? pos_all / pos_c : 0.0;
    for (int k = s; k < e; ++k) {
        if (ci[k] == i || !strong[k] || ci[k] >= ncols || cf[ci[k]] < 0)
            continue;
        double a = (double)va[k];
        p_ci[out] = cf[ci[k]];
        p_va[out] = (T)(-(a < 0 ? alpha : beta) * a / diag);
        ++out;
    }
}

template <typename T>
void interp_d1(const int* ro, const int* ci, const T* va,
               const unsigned char* strong, const int* cf, const int* didx,
               const int* p_ro, int n, int ncols, int* p_ci, T* p_va,
               hipStream_t s) {
    hipLaunchKernelGGL((d1_fill<T>), dim3(grid_1d(n)), dim3(AMGX_BLOCK), 0, s,
                       ro, ci, va, strong, cf, didx, p_ro, n, ncols, p_ci,
                       p_va);
}

void interp_d1_count(const int* ro, const int* ci, const unsigned char* strong,
                     const int* cf, int n, int ncols, int* counts,
                     hipStream_t s) {
    hipLaunchKernelGGL(d1_count, dim3(grid_1d(n)), dim3(AMGX_BLOCK), 0, s, ro,
                       ci, strong, cf, n, ncols, counts);
}

// ============================================================ ILU(0)
// Color-ordered ILU(0). pos[i] = elimination position of row i (= color-major
// order). Rows of ONE color are eliminated in parallel: their pivots are all
// in earlier colors (same-color rows do not couple under a valid coloring).
// For each row i: for pivots k (pos[k] < pos[i], ascending pos):
//   l_ik = a_ik / u_kk ; for j in row(i) with pos[j] > pos[k] and (k,j) in
//   pattern: a_ij -= l_ik * u_kj.
template <typename T>
__global__ __launch_bounds__(AMGX_BLOCK) void ilu0_factor_color(const int* __restrict__ ro,
                                  const int* __restrict__ ci,
                                  const int* __restrict__ pos,
                                  const int* __restrict__ didx,
                                  const int* __restrict__ rows, int count,
                                  T* __restrict__ lu, int n) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    int i = rows[t];
    int s = ro[i], e = ro[i + 1];
    int pi = pos[i];
    // process pivots in ascending elimination order: simple selection loop
    // over this row's nz (rows are short; O(deg^2) is fine and branch-light)
    for (int step = 0;; ++step) {
        // find the un-processed pivot with the smallest pos < pi
        int kidx = -1, kpos = 0x7fffffff;
        for (int k = s; k < e; ++k) {
            int j = ci[k];
            if (j >= n) continue;
            int pj = pos[j];
            if (pj < pi && pj >= step && pj < kpos) { kpos = pj; kidx = k; }
        }
        if (kidx < 0) break;
        int kcol = ci[kidx];
        int dkk = didx[kcol];
        T ukk = dkk >= 0 ? lu[dkk] : T(1);
        if (ukk == T(0)) ukk = T(1);
        T lik = lu[kidx] / ukk;
        lu[kidx] = lik;
        // subtract lik * U(k, j) for j in row i with pos[j] > kpos
        for (int k2 = ro[kcol]; k2 < ro[kcol + 1]; ++k2) {
            int j = ci[k2];
            if (j >= n || pos[j] <= kpos) continue;
            // find (i, j) in row i (binary search, cols sorted)
            int lo = s, hi = e;
            while (lo < hi) {
                int mid = (lo + hi) >> 1;
                int c = ci[mid];
                if (c == j) { lu[mid] -= lik * lu[k2]; break; }
                if (c < j) lo = mid + 1; else hi = mid;
            }
        }
        // advance past this pivot position
        step = kpos;
    }
}

// ------------------------------------------------------------ block ILU(0)
// Same color-ordered elimination with b x b blocks (reference
// src/solvers/multicolor_ilu_solver.cu block path):
//   L_ik = A_ik * U_kk^{-1};  A_ij -= L_ik * U_kj
// dinv[] holds the inverted pivot diagonal blocks of already-factored
// colors (filled by ilu0_invert_diag_block after each color).
template <typename T, int BMAX>
__global__ __launch_bounds__(AMGX_BLOCK) void ilu0_factor_color_block(
    const int* __restrict__ ro, const int* __restrict__ ci,
    const int* __restrict__ pos, const int* __restrict__ didx,
    const int* __restrict__ rows, int count, T* __restrict__ lu,
    const T* __restrict__ dinv, int n, int b) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    int i = rows[t];
    int s = ro[i], e = ro[i + 1];
    int pi = pos[i];
    int bb = b * b;
    T L[BMAX * BMAX];
    for (int step = 0;; ++step) {
        int kidx = -1, kpos = 0x7fffffff;
        for (int k = s; k < e; ++k) {
            int j = ci[k];
            if (j >= n) continue;
            int pj = pos[j];
            if (pj < pi && pj >= step && pj < kpos) { kpos = pj; kidx = k; }
        }
        if (kidx < 0) break;
        int kcol = ci[kidx];
        // L = lu[kidx] * dinv[kcol]
        const T* Aik = lu + (long long)kidx * bb;
        const T* Ukk_inv = dinv + (long long)kcol * bb;
        for (int r = 0; r < b; ++r)
            for (int c = 0; c < b; ++c) {
                T acc = T(0);
                for (int q = 0; q < b; ++q)
                    acc += Aik[r * b + q] * Ukk_inv[q * b + c];
                L[r * b + c] = acc;
            }
        for (int q = 0; q < bb; ++q) lu[(long long)kidx * bb + q] = L[q];
        // row i -= L * U(kcol, j) over pattern entries with pos[j] > kpos
        for (int k2 = ro[kcol]; k2 < ro[kcol + 1]; ++k2) {
            int j = ci[k2];
            if (j >= n || pos[j] <= kpos) continue;
            int lo = s, hi = e;
            while (lo < hi) {
                int mid = (lo + hi) >> 1;
                int c = ci[mid];
                if (c == j) {
                    const T* Ukj = lu + (long long)k2 * bb;
                    T* Aij = lu + (long long)mid * bb;
                    for (int r = 0; r < b; ++r)
                        for (int cc = 0; cc < b; ++cc) {
                            T acc = T(0);
                            for (int q = 0; q < b; ++q)
                                acc += L[r * b + q] * Ukj[q * b + cc];
                            Aij[r * b + cc] -= acc;
                        }
                    break;
                }
                if (c < j) lo = mid + 1; else hi = mid;
            }
        }
        step = kpos;
    }
}

// invert the (freshly factored) pivot diagonal blocks of one color
template <typename T, int BMAX>
__global__ __launch_bounds__(AMGX_BLOCK) void ilu0_invert_diag_block(
    const int* __restrict__ didx, const int* __restrict__ rows, int count,
    const T* __restrict__ lu, T* __restrict__ dinv, int b) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    int i = rows[t];
    int dk = didx[i];
    int bb = b * b;
    T D[BMAX * BMAX], Inv[BMAX * BMAX];
    double dmax = 0.0;
    for (int q = 0; q < bb; ++q) {
        D[q] = dk >= 0 ? lu[(long long)dk * bb + q] : T(q % (b + 1) == 0);
        dmax = fmax(dmax, fabs((double)D[q]));
    }
    if (dmax == 0.0)                      // fully zero pivot: identity
        for (int q = 0; q < bb; ++q) D[q] = T(q % (b + 1) == 0);
    small_mat_inv(D, Inv, b);
    bool bad = false;
    for (int q = 0; q < bb; ++q)
        if (!isfinite((double)Inv[q]) ||
            fabs((double)Inv[q]) > 1e12 * (1.0 + 1.0 / (dmax + 1e-300)))
            bad = true;
    if (bad) {                            // near-singular: diagonal fallback
        for (int q = 0; q < bb; ++q) Inv[q] = T(0);
        for (int r = 0; r < b; ++r) {
            double d = dk >= 0 ? (double)lu[(long long)dk * bb + r * b + r]
                               : 1.0;
            Inv[r * b + r] = (T)(d != 0.0 ? 1.0 / d : 1.0);
        }
    }
    for (int q = 0; q < bb; ++q) dinv[(long long)i * bb + q] = Inv[q];
}

// fwd: y_i = r_i - sum_{pos[j]<pos[i]} L_ij y_j   (unit diagonal blocks)
template <typename TA, typename TV>
__global__ __launch_bounds__(AMGX_BLOCK) void ilu0_fwd_block(
    const int* __restrict__ ro, const int* __restrict__ ci,
    const int* __restrict__ pos, const TA* __restrict__ lu,
    const int* __restrict__ rows, int count, const TV* __restrict__ r,
    TV* __restrict__ y, int n, int b) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    int i = rows[t];
    int pi = pos[i];
    int bb = b * b;
    TV acc[16];
    for (int c = 0; c < b; ++c) acc[c] = r[(long long)i * b + c];
    for (int k = ro[i]; k < ro[i + 1]; ++k) {
        int j = ci[k];
        if (j >= n || pos[j] >= pi) continue;
        const TA* blk = lu + (long long)k * bb;
        const TV* ys = y + (long long)j * b;
        for (int c = 0; c < b; ++c) {
            TV s = TV(0);
            for (int q = 0; q < b; ++q) s += (TV)blk[c * b + q] * ys[q];
            acc[c] -= s;
        }
    }
    for (int c = 0; c < b; ++c) y[(long long)i * b + c] = acc[c];
}

// bwd: z_i = dinv_i * (y_i - sum_{pos[j]>pos[i]} U_ij z_j)
template <typename TA, typename TV>
__global__ __launch_bounds__(AMGX_BLOCK) void ilu0_bwd_block(
    const int* __restrict__ ro, const int* __restrict__ ci,
    const int* __restrict__ pos, const TA* __restrict__ lu,
    const TA* __restrict__ dinv, const int* __restrict__ rows, int count,
    const TV* __restrict__ y, TV* __restrict__ z, int n, int b) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    int i = rows[t];
    int pi = pos[i];
    int bb = b * b;
    TV acc[16];
    for (int c = 0; c < b; ++c) acc[c] = y[(long long)i * b + c];
    for (int k = ro[i]; k < ro[i + 1]; ++k) {
        int j = ci[k];
        if (j >= n || pos[j] <= pi) continue;
        const TA* blk = lu + (long long)k * bb;
        const TV* zs = z + (long long)j * b;
        for (int c = 0; c < b; ++c) {
            TV s = TV(0);
            for (int q = 0; q < b; ++q) s += (TV)blk[c * b + q] * zs[q];
            acc[c] -= s;
        }
    }
    const TA* Dv = dinv + (long long)i * bb;
    for (int c = 0; c < b; ++c) {
        TV s = TV(0);
        for (int q = 0; q < b; ++q) s += (TV)Dv[c * b + q] * acc[q];
        z[(long long)i * b + c] = s;
    }
}

template <typename T>
void ilu0_factor_color_block_launch(const int* ro, const int* ci,
                                    const int* pos, const int* didx,
                                    const int* rows, int count, T* lu,
                                    const T* dinv, int n, int b,
                                    hipStream_t s) {
    if (count <= 0) return;
    if (b <= 8)
        hipLaunchKernelGGL((ilu0_factor_color_block<T, 8>),
                           dim3(grid_1d(count)), dim3(AMGX_BLOCK), 0, s, ro,
                           ci, pos, didx, rows, count, lu, dinv, n, b);
    else
        hipLaunchKernelGGL((ilu0_factor_color_block<T, 16>),
                           dim3(grid_1d(count)), dim3(AMGX_BLOCK), 0, s, ro,
                           ci, pos, didx, rows, count, lu, dinv, n, b);
}

template <typename T>
void ilu0_invert_diag_block_launch(const int* didx, const int* rows,
                                   int count, const T* lu, T* dinv, int b,
                                   hipStream_t s) {
    if (count <= 0) return;
    if (b <= 8)
        hipLaunchKernelGGL((ilu0_invert_diag_block<T, 8>),
                           dim3(grid_1d(count)), dim3(AMGX_BLOCK), 0, s,
                           didx, rows, count, lu, dinv, b);
    else
        hipLaunchKernelGGL((ilu0_invert_diag_block<T, 16>),
                           dim3(grid_1d(count)), dim3(AMGX_BLOCK), 0, s,
                           didx, rows, count, lu, dinv, b);
}

template <typename TA, typename TV>
void ilu0_fwd_block_launch(const int* ro, const int* ci, const int* pos,
                           const TA* lu, const int* rows, int count,
                           const TV* r, TV* y, int n, int b, hipStream_t s) {
    if (count <= 0) return;
    hipLaunchKernelGGL((ilu0_fwd_block<TA, TV>), dim3(grid_1d(count)),
                       dim3(AMGX_BLOCK), 0, s, ro, ci, pos, lu, rows, count,
                       r, y, n, b);
}

template <typename TA, typename TV>
void ilu0_bwd_block_launch(const int* ro, const int* ci, const int* pos,
                           const TA* lu, const TA* dinv, const int* rows,
                           int count, const TV* y, TV* z, int n, int b,
                           hipStream_t s) {
    if (count <= 0) return;
    hipLaunchKernelGGL((ilu0_bwd_block<TA, TV>), dim3(grid_1d(count)),
                       dim3(AMGX_BLOCK), 0, s, ro, ci, pos, lu, dinv, rows,
                       count, y, z, n, b);
}

// ---------------------------------------------------- color-sorted sweeps
// Same reorder-by-color slab layout as the DILU sweeps (kernels_solve.hip):
// lu_s/ci_s are rows_sorted-gathered copies, diag_s the per-slot pivot.
// forward: y_i = r_i - sum_{pos[j]<pos[i]} l_ij y_j (unit L); per color.
// backward: z_i = (y_i - sum_{pos[j]>pos[i]} u_ij z_j) / u_ii; per color desc.
template <typename TA, typename TV>
__global__ __launch_bounds__(AMGX_BLOCK) void ilu0_fwd_sorted_kernel(
    const int* __restrict__ ro_s, const int* __restrict__ ci_s,
    const TA* __restrict__ lu_s, const int* __restrict__ pos,
    const int* __restrict__ rows, int count, const TV* __restrict__ r,
    TV* __restrict__ y, int n) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    int i = rows[t];
    int pi = pos[i];
    TV sum = r[i];
    for (int k = ro_s[t]; k < ro_s[t + 1]; ++k) {
        int j = ci_s[k];
        if (j < n && pos[j] < pi) sum -= (TV)lu_s[k] * y[j];
    }
    y[i] = sum;
}

template <typename TA, typename TV>
__global__ __launch_bounds__(AMGX_BLOCK) void ilu0_bwd_sorted_kernel(
    const int* __restrict__ ro_s, const int* __restrict__ ci_s,
    const TA* __restrict__ lu_s, const TA* __restrict__ diag_s,
    const int* __restrict__ pos, const int* __restrict__ rows, int count,
    const TV* __restrict__ y, TV* __restrict__ z, int n) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    int i = rows[t];
    int pi = pos[i];
    TV sum = y[i];
    for (int k = ro_s[t]; k < ro_s[t + 1]; ++k) {
        int j = ci_s[k];
        if (j < n && pos[j] > pi) sum -= (TV)lu_s[k] * z[j];
    }
    TV d = (TV)diag_s[t];
    if (d == TV(0)) d = TV(1);
    z[i] = sum / d;
}

template <typename TA, typename TV>
void ilu0_fwd_sorted(const int* ro_s, const int* ci_s, const TA* lu_s,
                     const int* pos, const int* rows, int count, const TV* r,
                     TV* y, int n, hipStream_t s) {
    if (count <= 0) return;
    hipLaunchKernelGGL((ilu0_fwd_sorted_kernel<TA, TV>),
                       dim3(grid_1d(count)), dim3(AMGX_BLOCK), 0, s, ro_s,
                       ci_s, lu_s, pos, rows, count, r, y, n);
}

template <typename TA, typename TV>
void ilu0_bwd_sorted(const int* ro_s, const int* ci_s, const TA* lu_s,
                     const TA* diag_s, const int* pos, const int* rows,
                     int count, const TV* y, TV* z, int n, hipStream_t s) {
    if (count <= 0) return;
    hipLaunchKernelGGL((ilu0_bwd_sorted_kernel<TA, TV>),
                       dim3(grid_1d(count)), dim3(AMGX_BLOCK), 0, s, ro_s,
                       ci_s, lu_s, diag_s, pos, rows, count, y, z, n);
}

template <typename T>
void ilu0_factor_color_launch(const int* ro, const int* ci, const int* pos,
                              const int* didx, const int* rows, int count,
                              T* lu, int n, hipStream_t s) {
    if (count <= 0) return;
    hipLaunchKernelGGL((ilu0_factor_color<T>), dim3(grid_1d(count)),
                       dim3(AMGX_BLOCK), 0, s, ro, ci, pos, didx, rows, count,
                       lu, n);
}

#define INSTANTIATE_CLASSICAL(T)                                               \
    AMGX_INSTANTIATE(strength_ahat, T)                                         \
    AMGX_INSTANTIATE(interp_d1, T)                                             \
    AMGX_INSTANTIATE(ilu0_factor_color_launch, T)                              \
    AMGX_INSTANTIATE(ilu0_factor_color_block_launch, T)                        \
    AMGX_INSTANTIATE(ilu0_invert_diag_block_launch, T)
// ILU(0) applies: the float factor serves double vectors too (dDFI)
#define INSTANTIATE_CLASSICAL_PAIR(TA, TV)                                     \
    AMGX_INSTANTIATE(ilu0_fwd_sorted, TA, TV)                                  \
    AMGX_INSTANTIATE(ilu0_bwd_sorted, TA, TV)                                  \
    AMGX_INSTANTIATE(ilu0_fwd_block_launch, TA, TV)                            \
    AMGX_INSTANTIATE(ilu0_bwd_block_launch, TA, TV)

AMGX_REAL_TYPES(INSTANTIATE_CLASSICAL)
AMGX_REAL_PAIRS(INSTANTIATE_CLASSICAL_PAIR)

// ============================================================ truncate
// Drop |p_ij| < factor * rowmax_i, rescale survivors to preserve the row sum
// (reference src/truncate.cu truncate_kernel:388 + truncateAndScale:506).
// kth-largest key threshold among the factor-filtered entries of a row,
// ordered by (|value| desc, position asc) — a strict total order, so ties
// resolve like the host's stable argsort.  O(m * deg) selection without
// marks: each round finds the max strictly below the previous pick.
template <typename T>
__device__ __forceinline__ void topk_threshold(const T* va, int s, int e,
                                               double factor, double mx,
                                               int m, double* th_v,
                                               int* th_p) {
    double cv = 1.0 / 0.0;   // +inf sentinel: everything is below it
    int cp = -1;
    for (int r = 0; r < m; ++r) {
        double bv = -1.0;
        int bp = -1;
        for (int k = s; k < e; ++k) {
            double a = fabs((double)va[k]);
            if (a < factor * mx) continue;
            // strictly below (cv, cp) in (desc, asc-pos) order
            bool below = a < cv || (a == cv && k > cp);
            if (!below) continue;
            bool better = a > bv || (a == bv && k < bp);
            if (better) { bv = a; bp = k; }
        }
        if (bp < 0) break;      // fewer than m filtered entries
        cv = bv;
        cp = bp;
    }
    *th_v = cv;
    *th_p = cp;
}

template <typename T>
__device__ __forceinline__ bool trunc_keep(const T* va, int k, double factor,
                                           double mx, int m, double th_v,
                                           int th_p) {
    double a = fabs((double)va[k]);
    if (a < factor * mx) return false;
    if (m < 0) return true;
    // keep entries at or above the m-th key in the total order
    return a > th_v || (a == th_v && k <= th_p);
}

template <typename T>
__global__ __launch_bounds__(AMGX_BLOCK) void truncate_count(
    const int* __restrict__ ro, const T* __restrict__ va, int n,
    double factor, int max_elem, int* __restrict__ counts) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int s = ro[i], e = ro[i + 1];
    double mx = 0.0;
    for (int k = s; k < e; ++k) mx = fmax(mx, fabs((double)va[k]));
    int c = 0;
    for (int k = s; k < e; ++k)
        if (fabs((double)va[k]) >= factor * mx) ++c;
    if (max_elem >= 0 && c > max_elem) c = max_elem;
    counts[i] = c;
}

template <typename T>
__global__ __launch_bounds__(AMGX_BLOCK) void truncate_fill(
    const int* __restrict__ ro, const int* __restrict__ ci,
    const T* __restrict__ va, int n, double factor, int max_elem,
    const int* __restrict__ ro_out, int* __restrict__ ci_out,
    T* __restrict__ va_out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int s = ro[i], e = ro[i + 1];
    double mx = 0.0, sum_old = 0.0, sum_new = 0.0;
    for (int k = s; k < e; ++k) {
        double a = (double)va[k];
        sum_old += a;
        mx = fmax(mx, fabs(a));
    }
    double th_v = -1.0;
    int th_p = -1;
    int m = max_elem;
    if (m >= 0) {
        int c = 0;
        for (int k = s; k < e; ++k)
            if (fabs((double)va[k]) >= factor * mx) ++c;
        if (c <= m) m = -1;             // nothing to cap
        else topk_threshold(va, s, e, factor, mx, m, &th_v, &th_p);
    }
    for (int k = s; k < e; ++k)
        if (trunc_keep(va, k, factor, mx, m, th_v, th_p))
            sum_new += (double)va[k];
    double scale = (sum_new != 0.0 && sum_old != 0.0) ? sum_old / sum_new
                                                      : 1.0;
    int out = ro_out[i];
    for (int k = s; k < e; ++k) {
        if (!trunc_keep(va, k, factor, mx, m, th_v, th_p)) continue;
        ci_out[out] = ci[k];
        va_out[out] = (T)((double)va[k] * scale);
        ++out;
    }
}

template <typename T>
void truncate_rows_gpu(const int* ro, const int* ci, const T* va, int n,
                       double factor, int max_elem, const int* ro_out,
                       int* ci_out, T* va_out, int* counts, hipStream_t s) {
    hipLaunchKernelGGL((truncate_count<T>), dim3(grid_1d(n)),
                       dim3(AMGX_BLOCK), 0, s, ro, va, n, factor, max_elem,
                       counts);
}

template <typename T>
void truncate_fill_gpu(const int* ro, const int* ci, const T* va, int n,
                       double factor, int max_elem, const int* ro_out,
                       int* ci_out, T* va_out, hipStream_t s) {
    hipLaunchKernelGGL((truncate_fill<T>), dim3(grid_1d(n)),
                       dim3(AMGX_BLOCK), 0, s, ro, ci, va, n, factor,
                       max_elem, ro_out,
                       ci_out, va_out);
}

#define INSTANTIATE_TRUNC(T)                                                   \
    AMGX_INSTANTIATE(truncate_rows_gpu, T)                                     \
    AMGX_INSTANTIATE(truncate_fill_gpu, T)

AMGX_REAL_TYPES(INSTANTIATE_TRUNC)

}  // namespace amgx_hip
