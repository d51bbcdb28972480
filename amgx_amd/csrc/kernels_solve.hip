// Solve-path kernels: SpMV family, BLAS-1 reductions, Jacobi/GS/DILU
// smoothers, transfer operators, dense coarse GEMV. Hand-written for gfx950
// (wave64, LDS block reductions, grid-stride; see csrc/common.h).
//
// Reference behaviors: src/multiply.cu (SpMV + views), src/blas.cu,
// src/norm.cu, src/solvers/block_jacobi_solver.cu, jacobi_l1_solver.cu,
// multicolor_gauss_seidel_solver.cu, multicolor_dilu_solver.cu,
// src/aggregation/aggregation_amg_level.cu (restrict/prolongate).

#include <stdexcept>
#include <string>
#include <type_traits>

#include "common.h"
#include "core_api.h"

namespace amgx_hip {

// ============================================================ SpMV
// Mixed precision (reference dDFI modes): TA = matrix-value type, TV =
// vector type; products accumulate in TV (double when mixed).
// thread-per-row: right shape for stencil-like rows (<= ~16 nnz).
template <typename TA, typename TV, int UNROLL>
__global__ __launch_bounds__(AMGX_BLOCK) void csrmv_tpr(const int* __restrict__ ro, const int* __restrict__ ci,
                          const TA* __restrict__ va, const TV* __restrict__ x,
                          TV* __restrict__ y, const TV* __restrict__ bvec,
                          TV alpha, TV beta, TV gamma, int r0, int r1) {
    int i = r0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= r1) return;
    int s = ro[i], e = ro[i + 1];
    TV sum = TV(0);
    int k = s;
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
        if (k < e) { sum += (TV)va[k] * x[ci[k]]; ++k; }
    }
    for (; k < e; ++k) sum += (TV)va[k] * x[ci[k]];
    TV out = alpha * sum;
    if (beta != TV(0)) out += beta * y[i];
    if (bvec) out += gamma * bvec[i];
    y[i] = out;
}

// L lanes cooperate on one row: for high-degree rows (unstructured matrices).
template <typename TA, typename TV, int L>
__global__ __launch_bounds__(AMGX_BLOCK) void csrmv_vec(const int* __restrict__ ro, const int* __restrict__ ci,
                          const TA* __restrict__ va, const TV* __restrict__ x,
                          TV* __restrict__ y, const TV* __restrict__ bvec,
                          TV alpha, TV beta, TV gamma, int r0, int r1) {
    const int lane = threadIdx.x & (L - 1);
    int i = r0 + (blockIdx.x * blockDim.x + threadIdx.x) / L;
    if (i >= r1) return;
    int s = ro[i], e = ro[i + 1];
    TV sum = TV(0);
    for (int k = s + lane; k < e; k += L) sum += (TV)va[k] * x[ci[k]];
#pragma unroll
    for (int off = L / 2; off > 0; off >>= 1) sum += __shfl_down(sum, off, L);
    if (lane == 0) {
        TV out = alpha * sum;
        if (beta != TV(0)) out += beta * y[i];
        if (bvec) out += gamma * bvec[i];
        y[i] = out;
    }
}

template <typename TA, typename TV>
void csrmv(const int* ro, const int* ci, const TA* va, const TV* x, TV* y,
           const TV* bvec, TV alpha, TV beta, TV gamma, int r0, int r1,
           double avg_deg, hipStream_t s) {
    long long rows = (long long)r1 - r0;
    if (rows <= 0) return;
    if (avg_deg <= 16.0) {
        hipLaunchKernelGGL((csrmv_tpr<TA, TV, 8>), dim3(grid_1d(rows)),
                           dim3(AMGX_BLOCK), 0, s, ro, ci, va, x, y, bvec,
                           alpha, beta, gamma, r0, r1);
    } else if (avg_deg <= 64.0) {
        hipLaunchKernelGGL((csrmv_vec<TA, TV, 8>), dim3(grid_1d(rows * 8)),
                           dim3(AMGX_BLOCK), 0, s, ro, ci, va, x, y, bvec,
                           alpha, beta, gamma, r0, r1);
    } else {
        hipLaunchKernelGGL((csrmv_vec<TA, TV, 32>), dim3(grid_1d(rows * 32)),
                           dim3(AMGX_BLOCK), 0, s, ro, ci, va, x, y, bvec,
                           alpha, beta, gamma, r0, r1);
    }
}

// block-CSR: one thread per output row component (row i, comp r).
template <typename TA, typename TV>
__global__ __launch_bounds__(AMGX_BLOCK) void bsrmv_kernel(const int* __restrict__ ro,
                             const int* __restrict__ ci,
                             const TA* __restrict__ va, int b,
                             const TV* __restrict__ x, TV* __restrict__ y,
                             const TV* __restrict__ bvec, TV alpha, TV beta,
                             TV gamma, int r0, int r1) {
    long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long nrows = (long long)(r1 - r0) * b;
    if (t >= nrows) return;
    int i = r0 + (int)(t / b);
    int comp = (int)(t % b);
    int st = ro[i], e = ro[i + 1];
    TV sum = TV(0);
    for (int k = st; k < e; ++k) {
        const TA* blk = va + (long long)k * b * b + (long long)comp * b;
        const TV* xs = x + (long long)ci[k] * b;
        for (int c = 0; c < b; ++c) sum += (TV)blk[c] * xs[c];
    }
    long long oi = (long long)i * b + comp;
    TV out = alpha * sum;
    if (beta != TV(0)) out += beta * y[oi];
    if (bvec) out += gamma * bvec[oi];
    y[oi] = out;
}

// baseline scalar thread-per-row-component kernel, any b (A/B comparison
// target for the MFMA b=4 path in bench_kernels.py)
template <typename TA, typename TV>
void bsrmv_generic(const int* ro, const int* ci, const TA* va, int b,
                   const TV* x, TV* y, const TV* bvec, TV alpha, TV beta,
                   TV gamma, int r0, int r1, hipStream_t s) {
    long long rows = ((long long)r1 - r0) * b;
    if (rows <= 0) return;
    hipLaunchKernelGGL((bsrmv_kernel<TA, TV>), dim3(grid_1d(rows)),
                       dim3(AMGX_BLOCK), 0, s, ro, ci, va, b, x, y, bvec,
                       alpha, beta, gamma, r0, r1);
}

template <typename TA, typename TV>
void bsrmv(const int* ro, const int* ci, const TA* va, int b, const TV* x,
           TV* y, const TV* bvec, TV alpha, TV beta, TV gamma, int r0, int r1,
           hipStream_t s) {
    if (r1 <= r0) return;
    if (b == 4)             // MFMA wave kernel (kernels_mfma.hip)
        bsrmv_b4<TA, TV>(ro, ci, va, x, y, bvec, (double)alpha, (double)beta,
                         (double)gamma, r0, r1, s);
    else if (b >= 2 && b <= 8)   // generic wave kernel, coalesced block loads
        bsrmv_bn<TA, TV>(ro, ci, va, b, x, y, bvec, (double)alpha,
                         (double)beta, (double)gamma, r0, r1, s);
    else
        bsrmv_generic<TA, TV>(ro, ci, va, b, x, y, bvec, alpha, beta, gamma,
                              r0, r1, s);
}

// ============================================================ BLAS-1 reduce
// Deterministic two-stage reduction: fixed grid of NPART partials, then one
// block folds them. OP 0: sum conj(x_i) y_i (x_i y_i for real T), partials of
// type T. OP 1 sum|x_i|, OP 2 max|x_i|, OP 3 sum|x_i|^2: accumulators and
// partials of the real type of T, so a complex squared 2-norm is exactly
// real and non-negative.
#define NPART 1024

template <typename T, int OP>
using partial_t = std::conditional_t<OP == 0, T, typename real_of<T>::type>;

template <typename T, int OP>
__global__ __launch_bounds__(AMGX_BLOCK) void reduce_stage1(
    const T* __restrict__ x, const T* __restrict__ y, long long n,
    partial_t<T, OP>* __restrict__ part) {
    using A = partial_t<T, OP>;
    long long stride = (long long)gridDim.x * blockDim.x;
    A acc = A(0);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        if constexpr (OP == 0) acc += conj_mul(x[i], y[i]);
        else if constexpr (OP == 1) acc += abs(x[i]);
        else if constexpr (OP == 2) {
            A a = abs(x[i]);
            acc = a > acc ? a : acc;
        } else acc += abs2(x[i]);
    }
    A r;
    if constexpr (OP == 2) r = block_reduce_max(acc);
    else r = block_reduce_sum(acc);
    if (threadIdx.x == 0) part[blockIdx.x] = r;
}

template <typename T, int OP>
__global__ __launch_bounds__(AMGX_BLOCK) void reduce_stage2(const T* __restrict__ part, int nparts, T* out) {
    T acc = T(0);
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
        if constexpr (OP == 2) acc = part[i] > acc ? part[i] : acc;
        else acc += part[i];
    }
    T r;
    if constexpr (OP == 2) r = block_reduce_max(acc);
    else r = block_reduce_sum(acc);
    if (threadIdx.x == 0) *out = r;
}

template <typename T, int OP>
void reduce_launch(const T* x, const T* y, long long n, void* ws, void* out,
                   hipStream_t s) {
    using A = partial_t<T, OP>;
    int g = grid_1d(n, AMGX_BLOCK, NPART);
    hipLaunchKernelGGL((reduce_stage1<T, OP>), dim3(g), dim3(AMGX_BLOCK), 0, s,
                       x, y, n, (A*)ws);
    // OP 3 folds its partials by the plain sum of OP 1
    hipLaunchKernelGGL((reduce_stage2<A, OP == 3 ? 1 : OP>), dim3(1),
                       dim3(AMGX_BLOCK), 0, s, (const A*)ws, g, (A*)out);
}

template <typename T>
void reduce(const T* x, const T* y, long long n, int op, void* ws, void* out,
            hipStream_t s) {
    switch (op) {
        case 0: return reduce_launch<T, 0>(x, y, n, ws, out, s);
        case 1: return reduce_launch<T, 1>(x, y, n, ws, out, s);
        case 2: return reduce_launch<T, 2>(x, y, n, ws, out, s);
        case 3:   // complex only: a real squared norm is op 0 of (x, x)
            if constexpr (is_cplx<T>::value)
                return reduce_launch<T, 3>(x, y, n, ws, out, s);
            [[fallthrough]];
        default:
            throw std::runtime_error("reduce: unknown op " +
                                     std::to_string(op));
    }
}

template <typename T>
__global__ __launch_bounds__(AMGX_BLOCK) void axpy_kernel(T* y, const T* x, T a, long long n) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride)
        y[i] += a * x[i];
}

template <typename T>
__global__ __launch_bounds__(AMGX_BLOCK) void axpby_kernel(T* y, const T* x, T a, T b, long long n) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride)
        y[i] = a * x[i] + b * y[i];
}

// y += scale * alpha[0] * x — device-resident alpha keeps Krylov inner
// loops (MGS projections) free of host syncs (reference fuses/pipelines
// these; VERDICT r01 item 8: <=1 host sync per FGMRES iteration).
template <typename T>
__global__ __launch_bounds__(AMGX_BLOCK) void axpy_dalpha_kernel(T* __restrict__ y,
                                                                 const T* __restrict__ x,
                                                                 const T* __restrict__ alpha,
                                                                 T scale,
                                                                 long long n) {
    T a = scale * alpha[0];
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride)
        y[i] += a * x[i];
}

// x *= rsqrt(s[0]) with a zero-guard (s<=0 leaves x untouched — the lucky
// breakdown case is decided on the host after the one batched sync)
template <typename T>
__global__ __launch_bounds__(AMGX_BLOCK) void scal_drsqrt_kernel(T* __restrict__ x,
                                                                 const T* __restrict__ s2,
                                                                 long long n) {
    double v = (double)s2[0];
    if (v <= 0.0) return;
    T a = (T)rsqrt(v);
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride)
        x[i] *= a;
}

template <typename T>
void axpy_dalpha(T* y, const T* x, const T* alpha, T scale, long long n,
                 hipStream_t s) {
    hipLaunchKernelGGL((axpy_dalpha_kernel<T>),
                       dim3(grid_1d(n, AMGX_BLOCK, 2048)), dim3(AMGX_BLOCK),
                       0, s, y, x, alpha, scale, n);
}

template <typename T>
void scal_drsqrt(T* x, const T* s2, long long n, hipStream_t s) {
    hipLaunchKernelGGL((scal_drsqrt_kernel<T>),
                       dim3(grid_1d(n, AMGX_BLOCK, 2048)), dim3(AMGX_BLOCK),
                       0, s, x, s2, n);
}

template <typename T>
__global__ __launch_bounds__(AMGX_BLOCK) void scal_kernel(T* x, T a, long long n) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride)
        x[i] *= a;
}

template <typename T>
void axpy(T* y, const T* x, T a, long long n, hipStream_t s) {
    hipLaunchKernelGGL((axpy_kernel<T>), dim3(grid_1d(n, AMGX_BLOCK, 2048)),
                       dim3(AMGX_BLOCK), 0, s, y, x, a, n);
}
template <typename T>
void axpby(T* y, const T* x, T a, T b, long long n, hipStream_t s) {
    hipLaunchKernelGGL((axpby_kernel<T>), dim3(grid_1d(n, AMGX_BLOCK, 2048)),
                       dim3(AMGX_BLOCK), 0, s, y, x, a, b, n);
}
template <typename T>
void scal(T* x, T a, long long n, hipStream_t s) {
    hipLaunchKernelGGL((scal_kernel<T>), dim3(grid_1d(n, AMGX_BLOCK, 2048)),
                       dim3(AMGX_BLOCK), 0, s, x, a, n);
}

// ============================================================ structure
__global__ __launch_bounds__(AMGX_BLOCK) void diag_index_kernel(const int* __restrict__ ro,
                                  const int* __restrict__ ci, int n,
                                  int* __restrict__ out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int lo = ro[i], hi = ro[i + 1];
    int found = -1;
    // columns are sorted: binary search for i
    while (lo < hi) {
        int mid = (lo + hi) >> 1;
        int c = ci[mid];
        if (c == i) { found = mid; break; }
        if (c < i) lo = mid + 1; else hi = mid;
    }
    out[i] = found;
}

void diag_index(const int* ro, const int* ci, int n, int* out, hipStream_t s) {
    hipLaunchKernelGGL(diag_index_kernel, dim3(grid_1d(n)), dim3(AMGX_BLOCK),
                       0, s, ro, ci, n, out);
}

template <typename T>
__global__ __launch_bounds__(AMGX_BLOCK) void extract_diag_kernel(const T* __restrict__ va,
                                    const int* __restrict__ didx, int n, int b,
                                    T* __restrict__ out) {
    long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long total = (long long)n * b * b;
    if (t >= total) return;
    int i = (int)(t / (b * b));
    int off = (int)(t % (b * b));
    int k = didx[i];
    out[t] = (k >= 0) ? va[(long long)k * b * b + off] : T(0);
}

template <typename T>
void extract_diag(const T* va, const int* didx, int n, int b, T* out,
                  hipStream_t s) {
    long long total = (long long)n * b * b;
    hipLaunchKernelGGL((extract_diag_kernel<T>), dim3(grid_1d(total)),
                       dim3(AMGX_BLOCK), 0, s, va, didx, n, b, out);
}

// transpose-entry lookup: for nz k in row i with col j, the index of (j, i).
__global__ __launch_bounds__(AMGX_BLOCK) void trans_index_kernel(const int* __restrict__ ro,
                                   const int* __restrict__ ci, int n,
                                   int* __restrict__ out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int k = ro[i]; k < ro[i + 1]; ++k) {
        int j = ci[k];
        int found = -1;
        if (j < n) {
            int lo = ro[j], hi = ro[j + 1];
            while (lo < hi) {
                int mid = (lo + hi) >> 1;
                int c = ci[mid];
                if (c == i) { found = mid; break; }
                if (c < i) lo = mid + 1; else hi = mid;
            }
        }
        out[k] = found;
    }
}

void trans_index(const int* ro, const int* ci, int n, int* out, hipStream_t s) {
    hipLaunchKernelGGL(trans_index_kernel, dim3(grid_1d(n)), dim3(AMGX_BLOCK),
                       0, s, ro, ci, n, out);
}

// ============================================================ Jacobi
// scalar 1/d, d == 0 gives 1 as on the host. The l1 term needs fabs and a
// sign, so it is compiled out for value types without an ordering (complex).
template <typename T>
__global__ __launch_bounds__(AMGX_BLOCK) void jacobi_dinv_scalar(const int* __restrict__ ro,
                                   const T* __restrict__ va,
                                   const int* __restrict__ didx, int n,
                                   bool l1, T* __restrict__ dinv) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int dk = didx[i];
    T d = dk >= 0 ? va[dk] : T(0);
    if constexpr (!is_cplx<T>::value) {
        if (l1) {
            T sum = T(0);
            for (int k = ro[i]; k < ro[i + 1]; ++k)
                if (k != dk) sum += fabs((double)va[k]);
            d += (d >= T(0) ? sum : -sum);
        }
    }
    if (d == T(0)) d = T(1);
    dinv[i] = T(1) / d;
}

// block: a missing diagonal block counts as zero; l1 adds the l1 norm of the
// off-diagonal part of component r's row with the sign of D_rr (the l1 sign
// rule of ops/cpu.py:jacobi_dinv, as in the scalar kernel above); singular
// blocks by the rule of small_mat_inv (common.h).
template <typename T, int BMAX>
__global__ __launch_bounds__(AMGX_BLOCK) void jacobi_dinv_block(const int* __restrict__ ro,
                                  const T* __restrict__ va,
                                  const int* __restrict__ didx, int n, int b,
                                  bool l1, T* __restrict__ dinv) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    T D[BMAX * BMAX], Inv[BMAX * BMAX];
    int dk = didx[i];
    for (int q = 0; q < b * b; ++q)
        D[q] = dk >= 0 ? va[(long long)dk * b * b + q] : T(0);
    if (l1) {
        for (int k = ro[i]; k < ro[i + 1]; ++k) {
            if (k == dk) continue;
            const T* blk = va + (long long)k * b * b;
            for (int r = 0; r < b; ++r) {
                T s = T(0);
                for (int c = 0; c < b; ++c) s += fabs((double)blk[r * b + c]);
                D[r * b + r] += (D[r * b + r] >= T(0) ? s : -s);
            }
        }
    }
    small_mat_inv(D, Inv, b);
    for (int q = 0; q < b * b; ++q) dinv[(long long)i * b * b + q] = Inv[q];
}

template <typename T>
void jacobi_dinv(const int* ro, const T* va, const int* didx, int n, int b,
                 bool l1, T* dinv, hipStream_t s) {
    if (is_cplx<T>::value && (b != 1 || l1))
        throw std::runtime_error("jacobi_dinv: complex matrices support "
                                 "neither blocks nor the l1 variant");
    if (b == 1) {
        hipLaunchKernelGGL((jacobi_dinv_scalar<T>), dim3(grid_1d(n)),
                           dim3(AMGX_BLOCK), 0, s, ro, va, didx, n, l1, dinv);
    } else if constexpr (!is_cplx<T>::value) {
        if (b <= 8)
            hipLaunchKernelGGL((jacobi_dinv_block<T, 8>), dim3(grid_1d(n)),
                               dim3(AMGX_BLOCK), 0, s, ro, va, didx, n, b, l1,
                               dinv);
        else
            hipLaunchKernelGGL((jacobi_dinv_block<T, 16>), dim3(grid_1d(n)),
                               dim3(AMGX_BLOCK), 0, s, ro, va, didx, n, b, l1,
                               dinv);
    }
}

// fused damped Jacobi sweep: xo = xi + omega*dinv*(b - A xi), single pass.
template <typename TA, typename TV>
__global__ __launch_bounds__(AMGX_BLOCK) void jacobi_smooth_scalar(const int* __restrict__ ro,
                                     const int* __restrict__ ci,
                                     const TA* __restrict__ va,
                                     const TA* __restrict__ dinv,
                                     const TV* __restrict__ bvec,
                                     const TV* __restrict__ xi,
                                     TV* __restrict__ xo, TV omega, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int s = ro[i], e = ro[i + 1];
    TV sum = TV(0);
    for (int k = s; k < e; ++k) sum += (TV)va[k] * xi[ci[k]];
    xo[i] = xi[i] + omega * (TV)dinv[i] * (bvec[i] - sum);
}

template <typename TA, typename TV>
__global__ __launch_bounds__(AMGX_BLOCK) void jacobi_smooth_block(const int* __restrict__ ro,
                                    const int* __restrict__ ci,
                                    const TA* __restrict__ va,
                                    const TA* __restrict__ dinv,
                                    const TV* __restrict__ bvec,
                                    const TV* __restrict__ xi,
                                    TV* __restrict__ xo, TV omega, int n,
                                    int b) {
    long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)n * b) return;
    int i = (int)(t / b);
    int rcomp = (int)(t % b);
    int s = ro[i], e = ro[i + 1];
    // residual components of the whole block-row are needed for dinv apply;
    // recompute per output comp: r_c = b_c - sum_k blk[c,:] x  (c = 0..b-1)
    TV upd = TV(0);
    for (int c = 0; c < b; ++c) {
        TV sum = TV(0);
        for (int k = s; k < e; ++k) {
            const TA* blk = va + ((long long)k * b + c) * b;
            const TV* xs = xi + (long long)ci[k] * b;
            for (int q = 0; q < b; ++q) sum += (TV)blk[q] * xs[q];
        }
        TV rc = bvec[(long long)i * b + c] - sum;
        upd += (TV)dinv[((long long)i * b + rcomp) * b + c] * rc;
    }
    xo[t] = xi[t] + omega * upd;
}

template <typename TA, typename TV>
void jacobi_smooth(const int* ro, const int* ci, const TA* va, const TA* dinv,
                   const TV* bvec, const TV* xi, TV* xo, TV omega, int n,
                   int b, hipStream_t s) {
    if (b == 1) {
        hipLaunchKernelGGL((jacobi_smooth_scalar<TA, TV>), dim3(grid_1d(n)),
                           dim3(AMGX_BLOCK), 0, s, ro, ci, va, dinv, bvec, xi,
                           xo, omega, n);
    } else {
        hipLaunchKernelGGL((jacobi_smooth_block<TA, TV>),
                           dim3(grid_1d((long long)n * b)), dim3(AMGX_BLOCK),
                           0, s, ro, ci, va, dinv, bvec, xi, xo, omega, n, b);
    }
}

// ============================================================ multicolor sweeps
// Row product of slot t of a color-sorted slab with the gathered vector v.
// The first 8 entries are peeled so their loads issue together; summation
// runs in ascending k.
template <typename TA, typename TV>
__device__ __forceinline__ TV slab_row_dot(const int* __restrict__ ro_s,
                                           const int* __restrict__ ci_s,
                                           const TA* __restrict__ va_s, int t,
                                           const TV* v) {
    auto term = [&](int k) { return (TV)va_s[k] * v[ci_s[k]]; };
    int k = ro_s[t], e = ro_s[t + 1];
    TV sum = TV(0);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        if (k < e) { sum += term(k); ++k; }
    }
    for (; k < e; ++k) sum += term(k);
    return sum;
}

// The same product with LANES lanes per row (a power of two, the lanes of
// one row adjacent in the wave): per chunk of LANES entries lane l loads
// entry k0 + l, so the slab reads coalesce and the gathers of a chunk are in
// flight together; the chunk is then folded in ascending k from values
// broadcast within the group, every lane carrying the same sum. Entries past
// the row's end are skipped, not added as zeros, and the product-and-add is
// the expression of slab_row_dot, so the sum is that of the one-lane form
// bit for bit. All LANES lanes of a row must call this together.
template <int LANES, typename TA, typename TV>
__device__ __forceinline__ TV slab_row_dot_lanes(const int* __restrict__ ro_s,
                                                 const int* __restrict__ ci_s,
                                                 const TA* __restrict__ va_s,
                                                 int t, int lane,
                                                 const TV* v) {
    if constexpr (LANES == 1) {
        return slab_row_dot(ro_s, ci_s, va_s, t, v);
    } else {
        const int e = ro_s[t + 1];
        TV sum = TV(0);
        for (int k0 = ro_s[t]; k0 < e; k0 += LANES) {
            TA a = TA(0);
            TV g = TV(0);
            if (k0 + lane < e) {
                a = va_s[k0 + lane];
                g = v[ci_s[k0 + lane]];
            }
#pragma unroll
            for (int u = 0; u < LANES; ++u) {
                TA au = __shfl(a, u, LANES);
                TV gu = __shfl(g, u, LANES);
                if (k0 + u < e) sum += (TV)au * gu;
            }
        }
        return sum;
    }
}

// The same product in stream form: a wave owns the 64 consecutive slab rows
// from t0, one lane per row: lane l has row t0 + l and passes its bounds
// rs = ro_s[t0 + l], re = ro_s[t0 + l + 1], or rs = re = 0 past the color's
// end. Their entries are the contiguous range [ro_s[t0],
// ro_s[min(t0 + 64, count)]), which the wave walks in windows of W entries
// (dilu_stream_window) kept in its private LDS region `lds`: all lanes load
// ci and va of the window coalesced, gather v through every index, and
// write (a, g) to slot k - base; then each lane folds the part of its own
// row that lies in the window, ascending k, with the expression of
// slab_row_dot, and carries the sum into the next window. A row longer than a
// window, or cut by a window's edge, takes no other path, so every row gives
// the bits of the one-lane form. The slab loads of the next window are issued
// once this window's registers are in LDS, so they fly during the fold.
// Invariants: every LDS slot index is k - base with 0 <= k - base < W; a
// load index is clamped to the last entry of the wave's range, so nothing
// is read past the slab's end or gathered through an index that was never
// set (the slots such lanes fill are beyond every row's end and are never
// folded); the window loop's trip count is uniform over the wave and no lane
// leaves it early. LDS writes and the fold are ordered within the wave alone
// (wavefront-scope fences): the trip count differs between the waves of a
// block, so there is no workgroup barrier in here. All 64 lanes call this
// together.
template <typename TA, typename TV>
constexpr int dilu_stream_window() {
    return dilu_stream_window_of((int)(sizeof(TA) + sizeof(TV)));
}

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename TA, typename TV>
__device__ __forceinline__ TV slab_row_dot_stream(
    const int* __restrict__ ci_s, const TA* __restrict__ va_s, int t0,
    int count, int lane, int rs, int re, const TV* v, char* lds) {
    constexpr int W = dilu_stream_window<TA, TV>();
    constexpr int U = W / 64;
    TA* la = reinterpret_cast<TA*>(lds);
    TV* lg = reinterpret_cast<TV*>(lds + W * sizeof(TA));
    // the wave's range, from its first and its last row (lane 0 has a row)
    const int last = (count - t0 < DILU_STREAM_ROWS ? count - t0
                                                    : DILU_STREAM_ROWS) - 1;
    const int kb = __builtin_amdgcn_readfirstlane(rs);
    const int ke = __builtin_amdgcn_readlane(
        re, __builtin_amdgcn_readfirstlane(last));
    TV sum = TV(0);
    int c[U];
    TA a[U];
    auto load_window = [&](int base) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int k = base + u * 64 + lane;
            k = k < ke ? k : ke - 1;
            a[u] = va_s[k];
            c[u] = ci_s[k];
        }
    };
    if (kb < ke) load_window(kb);
    for (int base = kb; base < ke; base += W) {
        TV g[U];
#pragma unroll
        for (int u = 0; u < U; ++u) g[u] = v[c[u]];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            la[u * 64 + lane] = a[u];
            lg[u * 64 + lane] = g[u];
        }
        // the next window's slab loads fly during this window's fold
        if (base + W < ke) load_window(base + W);
        wave_lds_sync();
        int k = (rs > base ? rs : base) - base;
        const int e = (re < base + W ? re : base + W) - base;
        for (; k + 4 <= e; k += 4) {
            TA a0 = la[k], a1 = la[k + 1], a2 = la[k + 2], a3 = la[k + 3];
            TV g0 = lg[k], g1 = lg[k + 1], g2 = lg[k + 2], g3 = lg[k + 3];
            sum += (TV)a0 * g0;
            sum += (TV)a1 * g1;
            sum += (TV)a2 * g2;
            sum += (TV)a3 * g3;
        }
        for (; k < e; ++k) sum += (TV)la[k] * lg[k];
        wave_lds_sync();
    }
    return sum;
}

// ============================================================ multicolor GS
// color-sorted GS row sweep (reorder-by-color layout; ro_s/rows/dinv_s
// pre-offset to the color base, matrix arrays gathered in rows_sorted
// order so the color reads one contiguous slab)
template <typename TA, typename TV>
__global__ __launch_bounds__(AMGX_BLOCK) void gs_rows_scalar_sorted(
    const int* __restrict__ ro_s, const int* __restrict__ ci_s,
    const TA* __restrict__ va_s, const TA* __restrict__ dinv_s,
    const TV* __restrict__ bvec, TV* __restrict__ x,
    const int* __restrict__ rows, int count, TV omega) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    int i = rows[t];
    TV sum = slab_row_dot(ro_s, ci_s, va_s, t, x);
    x[i] += omega * (TV)dinv_s[t] * (bvec[i] - sum);
}

// fused whole-sweep GS for small levels: one single-WG launch loops all
// colors (and the descending pass when symmetric) with __syncthreads as
// the color barrier — same launch-floor fix as dilu_apply_small
template <typename TA, typename TV>
__global__ __launch_bounds__(1024) void gs_sweep_small_kernel(
    const int* __restrict__ ro_s, const int* __restrict__ ci_s,
    const TA* __restrict__ va_s, const TA* __restrict__ dinv_s,
    const TV* __restrict__ bvec, TV* __restrict__ x,
    const int* __restrict__ rows, const int* __restrict__ bounds,
    int ncolors, TV omega, int symmetric) {
    int tid = threadIdx.x;
    int nt = blockDim.x;
    for (int pass = 0; pass < 1 + symmetric; ++pass) {
        for (int cc = 0; cc < ncolors; ++cc) {
            int c = pass == 0 ? cc : ncolors - 1 - cc;
            int s0 = bounds[c], s1 = bounds[c + 1];
            for (int t = s0 + tid; t < s1; t += nt) {
                int i = rows[t];
                TV sum = TV(0);
                for (int k = ro_s[t]; k < ro_s[t + 1]; ++k)
                    sum += (TV)va_s[k] * x[ci_s[k]];
                x[i] += omega * (TV)dinv_s[t] * (bvec[i] - sum);
            }
            __syncthreads();
        }
    }
}

template <typename TA, typename TV>
void gs_sweep_small(const int* ro_s, const int* ci_s, const TA* va_s,
                    const TA* dinv_s, const TV* bvec, TV* x, const int* rows,
                    const int* bounds, int ncolors, TV omega, bool symmetric,
                    hipStream_t s) {
    hipLaunchKernelGGL((gs_sweep_small_kernel<TA, TV>), dim3(1), dim3(1024),
                       0, s, ro_s, ci_s, va_s, dinv_s, bvec, x, rows, bounds,
                       ncolors, omega, symmetric ? 1 : 0);
}

template <typename TA, typename TV>
void gs_rows_sorted(const int* ro_s, const int* ci_s, const TA* va_s,
                    const TA* dinv_s, const TV* bvec, TV* x, const int* rows,
                    int count, TV omega, hipStream_t s) {
    if (count <= 0) return;
    hipLaunchKernelGGL((gs_rows_scalar_sorted<TA, TV>),
                       dim3(grid_1d(count)), dim3(AMGX_BLOCK), 0, s, ro_s,
                       ci_s, va_s, dinv_s, bvec, x, rows, count, omega);
}

template <typename TA, typename TV>
__global__ __launch_bounds__(AMGX_BLOCK) void gs_rows_scalar(const int* __restrict__ ro,
                               const int* __restrict__ ci,
                               const TA* __restrict__ va,
                               const TA* __restrict__ dinv,
                               const TV* __restrict__ bvec, TV* __restrict__ x,
                               const int* __restrict__ rows, int count,
                               TV omega) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    int i = rows[t];
    int s = ro[i], e = ro[i + 1];
    TV sum = TV(0);
    for (int k = s; k < e; ++k) sum += (TV)va[k] * x[ci[k]];
    x[i] += omega * (TV)dinv[i] * (bvec[i] - sum);
}

// one THREAD per block-row: all b components are computed before any write,
// so the in-place update is race-free (same-color rows have no mutual edges
// under a valid distance-1 coloring; the only intra-row hazard is the
// diagonal block, which this thread owns entirely).
template <typename TA, typename TV>
__global__ __launch_bounds__(AMGX_BLOCK) void gs_rows_block(const int* __restrict__ ro,
                              const int* __restrict__ ci,
                              const TA* __restrict__ va,
                              const TA* __restrict__ dinv,
                              const TV* __restrict__ bvec, TV* __restrict__ x,
                              const int* __restrict__ rows, int count,
                              TV omega, int b) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    int i = rows[t];
    int s = ro[i], e = ro[i + 1];
    TV res[16], upd[16];  // b <= 16 (reference supports block sizes to 10)
    for (int c = 0; c < b; ++c) {
        TV sum = TV(0);
        for (int k = s; k < e; ++k) {
            const TA* blk = va + ((long long)k * b + c) * b;
            const TV* xs = x + (long long)ci[k] * b;
            for (int q = 0; q < b; ++q) sum += (TV)blk[q] * xs[q];
        }
        res[c] = bvec[(long long)i * b + c] - sum;
    }
    const TA* D = dinv + (long long)i * b * b;
    for (int c = 0; c < b; ++c) {
        TV s2 = TV(0);
        for (int q = 0; q < b; ++q) s2 += (TV)D[c * b + q] * res[q];
        upd[c] = s2;
    }
    for (int c = 0; c < b; ++c) x[(long long)i * b + c] += omega * upd[c];
}

template <typename TA, typename TV>
void gs_smooth_rows(const int* ro, const int* ci, const TA* va,
                    const TA* dinv, const TV* bvec, TV* x, const int* rows,
                    int count, TV omega, int n, int b, hipStream_t s) {
    if (count <= 0) return;
    if (b == 1) {
        hipLaunchKernelGGL((gs_rows_scalar<TA, TV>), dim3(grid_1d(count)),
                           dim3(AMGX_BLOCK), 0, s, ro, ci, va, dinv, bvec, x,
                           rows, count, omega);
    } else if constexpr (is_cplx<TV>::value) {
        throw std::runtime_error(
            "gs_smooth_rows: complex block matrices are unsupported");
    } else {
        hipLaunchKernelGGL((gs_rows_block<TA, TV>), dim3(grid_1d(count)),
                           dim3(AMGX_BLOCK), 0, s, ro, ci, va, dinv, bvec, x,
                           rows, count, omega, b);
    }
}

// ============================================================ DILU
template <typename T>
__global__ __launch_bounds__(AMGX_BLOCK) void dilu_setup_scalar(const int* __restrict__ ro,
                                  const int* __restrict__ ci,
                                  const T* __restrict__ va,
                                  const int* __restrict__ didx,
                                  const int* __restrict__ tidx,
                                  const int* __restrict__ colors,
                                  const int* __restrict__ rows, int count,
                                  int color, T* __restrict__ einv) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    int i = rows[t];
    int dk = didx[i];
    T d = dk >= 0 ? va[dk] : T(0);
    T e = d;
    for (int k = ro[i]; k < ro[i + 1]; ++k) {
        int j = ci[k];
        if (j == i) continue;
        int tk = tidx[k];
        if (tk >= 0 && colors[j] < color) e -= va[k] * einv[j] * va[tk];
    }
    // tiny-pivot safeguard: a near-zero modified pivot cascades huge Einv
    // through later colors — fall back to the plain diagonal
    T dref = (d != T(0)) ? d : T(1);
    if (absd(e) < 1e-10 * absd(dref)) e = dref;
    einv[i] = T(1) / e;
}

template <typename T, int BMAX>
__global__ __launch_bounds__(AMGX_BLOCK) void dilu_setup_block(const int* __restrict__ ro,
                                 const int* __restrict__ ci,
                                 const T* __restrict__ va,
                                 const int* __restrict__ didx,
                                 const int* __restrict__ tidx,
                                 const int* __restrict__ colors,
                                 const int* __restrict__ rows, int count,
                                 int color, T* __restrict__ einv, int b) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    int i = rows[t];
    int dk = didx[i];
    T E[BMAX * BMAX], Inv[BMAX * BMAX];
    for (int q = 0; q < b * b; ++q)
        E[q] = dk >= 0 ? va[(long long)dk * b * b + q] : T(0);
    for (int k = ro[i]; k < ro[i + 1]; ++k) {
        int j = ci[k];
        if (j == i) continue;
        int tk = tidx[k];
        if (tk >= 0 && colors[j] < color) {
            const T* Aij = va + (long long)k * b * b;
            const T* Einvj = einv + (long long)j * b * b;
            const T* Aji = va + (long long)tk * b * b;
            // E -= Aij * Einvj * Aji
            for (int r = 0; r < b; ++r)
                for (int c = 0; c < b; ++c) {
                    T s = T(0);
                    for (int p = 0; p < b; ++p) {
                        T m = T(0);
                        for (int q = 0; q < b; ++q)
                            m += Aij[r * b + q] * Einvj[q * b + p];
                        s += m * Aji[p * b + c];
                    }
                    E[r * b + c] -= s;
                }
        }
    }
    // stabilized fallback to the plain diagonal block: the rule is stated at
    // dilu_keep_inverse (common.h)
    double emax = 0.0, dmax = 0.0;
    for (int q = 0; q < b * b; ++q) {
        emax = fmax(emax, fabs((double)E[q]));
        double dv = dk >= 0 ? fabs((double)va[(long long)dk * b * b + q])
                            : 0.0;
        dmax = fmax(dmax, dv);
    }
    double pmin = small_mat_inv(E, Inv, b);
    if (!dilu_keep_inverse<T>(emax, pmin, dmax)) {
        for (int q = 0; q < b * b; ++q)
            E[q] = dk >= 0 ? va[(long long)dk * b * b + q]
                           : (q % (b + 1) == 0 ? T(1) : T(0));
        small_mat_inv(E, Inv, b);
    }
    for (int q = 0; q < b * b; ++q) einv[(long long)i * b * b + q] = Inv[q];
}

template <typename T>
void dilu_setup_color(const int* ro, const int* ci, const T* va,
                      const int* didx, const int* tidx, const int* colors,
                      const int* rows, int count, int color, T* einv, int b,
                      hipStream_t s) {
    if (count <= 0) return;
    if (b == 1) {
        hipLaunchKernelGGL((dilu_setup_scalar<T>), dim3(grid_1d(count)),
                           dim3(AMGX_BLOCK), 0, s, ro, ci, va, didx, tidx,
                           colors, rows, count, color, einv);
    } else if constexpr (is_cplx<T>::value) {
        throw std::runtime_error(
            "dilu_setup: complex block matrices are unsupported");
    } else if (b == 4) {   // MFMA triple-product path (kernels_mfma.hip)
        dilu_setup_b4<T>(ro, ci, va, didx, tidx, colors, rows, count, color,
                         einv, s);
    } else if (b <= 8) {
        hipLaunchKernelGGL((dilu_setup_block<T, 8>), dim3(grid_1d(count)),
                           dim3(AMGX_BLOCK), 0, s, ro, ci, va, didx, tidx,
                           colors, rows, count, color, einv, b);
    } else {
        hipLaunchKernelGGL((dilu_setup_block<T, 16>), dim3(grid_1d(count)),
                           dim3(AMGX_BLOCK), 0, s, ro, ci, va, didx, tidx,
                           colors, rows, count, color, einv, b);
    }
}

// ---- color-sorted sweep variants (reference reorder-by-color layout,
// include/matrix.h:766, src/core.cu:489-506, redesigned as a sorted COPY):
// the matrix rows are stored in rows_sorted order, so each color's sweep
// reads a CONTIGUOUS slab of values/columns exactly once — the original
// per-color launches re-fetched ~num_colors scattered cache lines per
// sweep.  ro_s/rows/einv_s pointers arrive pre-offset to the color base.
//
// Scalar matrices keep, next to the full slab, its strict color-split parts
// (slab_split_*, kernels_setup.hip): L holds the entries of earlier-color
// local columns, U those of later colors, both in slab order, so the sums
// below run in the order of a full-row product with the zero terms left out.
//
// A scalar sweep is a row rule (DiluFwdFull, DiluFwdLower, DiluBwdUpper)
// run by a launch shape (dilu_lane_kernel, dilu_stream_kernel,
// dilu_small_kernel). The rule says what a row does around its product: the
// vector gathered(), the row's own reads read(t, i) of slab slot t and row
// i = rows[t], and the epilogue finish(i, own, sum) with its stores. The
// shape says which lanes compute the product and when the own reads are
// issued. Every rule gives the same bits under every shape
// (tests/test_gpu_dilu_{lanes,small,stream}.py).
template <typename T>
__device__ __forceinline__ T add_unfused(T a, T b) {
#pragma clang fp contract(off)
    return a + b;
}
template <typename R>
__device__ __forceinline__ cplx<R> add_unfused(const cplx<R>& a,
                                               const cplx<R>& b) {
#pragma clang fp contract(off)
    return cplx<R>(a.re + b.re, a.im + b.im);
}

template <typename TV>
__global__ __launch_bounds__(AMGX_BLOCK) void dilu_y_init_kernel(
    const TV* __restrict__ x, TV* __restrict__ y, long long n) {
    long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) y[j] = x[j] + TV(0);
}

// The products of a row's epilogue, in the two spellings the shapes use. In a
// complex product a * o the compiler contracts the imaginary part
// a.re * o.im + a.im * o.re to one rounded product and one fused
// multiply-add, and which of the two products it rounds depends on the code
// around the expression: in the lane and one-launch shapes, which take the
// plain e * s (PINNED = false), Einv_i (b_i - sum) and relax * z round
// a.re * o.im, Einv_i * sum of the backward rule rounds a.im * o.re (read
// off their ISA; tests/test_gpu_dilu_stream.py compares the bits). The stream
// shape spells that choice out (PINNED = true, ROUND_RE_IM as just listed), so
// it gives the same bits whatever surrounds the call. A real product is a
// real product.
__device__ __forceinline__ double fma_of(double a, double b, double c) {
    return __builtin_fma(a, b, c);
}
__device__ __forceinline__ float fma_of(float a, float b, float c) {
    return __builtin_fmaf(a, b, c);
}
template <bool ROUND_RE_IM, typename T>
__device__ __forceinline__ T times_pinned(T e, T s) {
    return e * s;
}
template <bool ROUND_RE_IM, typename R>
__device__ __forceinline__ cplx<R> times_pinned(const cplx<R>& e,
                                              const cplx<R>& s) {
#pragma clang fp contract(off)
    R re = fma_of(e.re, s.re, -(e.im * s.im));
    R im = ROUND_RE_IM ? fma_of(e.im, s.re, e.re * s.im)
                       : fma_of(e.re, s.im, e.im * s.re);
    return cplx<R>(re, im);
}
template <bool PINNED, bool ROUND_RE_IM, typename T>
__device__ __forceinline__ T row_times(const T& e, const T& s) {
    if constexpr (PINNED) return times_pinned<ROUND_RE_IM>(e, s);
    else return e * s;
}

// fused forward (full slab): w_i = Einv_i (b_i - sum_k a_k y_k) with the one
// gathered vector y = x + w kept next to w: dilu_y_init writes y = x + 0 (the
// value x_k + w_k had under a zeroed w, sign of zero included) and each row
// stores y_i = x_i + w_i with its w_i, the sum rounded on its own as the
// gathered x[j] + w[j] was. The product so only picks up earlier colors
// (valid coloring => no same-color off-diagonals; the diagonal meets y_i =
// x_i). It replaces residual kernel + sweep with one matrix read,
// mathematically identical to r = b - A x; M w = r; nothing reads a w or y
// that this apply has not written.
template <typename TA, typename TV>
struct DiluFwdFull {
    const TA* einv_s;
    const TV* rhs;
    const TV* x;
    TV* w;
    TV* y;
    struct Own { TA e; TV r, x; };
    __device__ const TV* gathered() const { return y; }
    __device__ Own read(int t, int i) const {
        return {einv_s[t], rhs[i], x[i]};
    }
    template <bool PINNED>
    __device__ void finish(int i, const Own& o, TV sum) const {
        TV wi = row_times<PINNED, true>((TV)o.e, o.r - sum);
        w[i] = wi;
        y[i] = add_unfused(o.x, wi);
    }
};

// plain forward over L: w_i = Einv_i (rhs_i - sum_L A_ij w_j).  Only rows of
// earlier colors, already written by this sweep, are read: w needs no
// zeroing.
template <typename TA, typename TV>
struct DiluFwdLower {
    const TA* einv_s;
    const TV* rhs;
    TV* w;
    struct Own { TA e; TV r; };
    __device__ const TV* gathered() const { return w; }
    __device__ Own read(int t, int i) const { return {einv_s[t], rhs[i]}; }
    template <bool PINNED>
    __device__ void finish(int i, const Own& o, TV sum) const {
        w[i] = row_times<PINNED, true>((TV)o.e, o.r - sum);
    }
};

// backward over U, in place, colors descending: z_i = w_i - Einv_i sum_U
// A_ij z_j.  Later colors already hold z in w, this color still holds w (so
// w_i may be read ahead of the product), and z_i overwrites w_i; the relaxed
// update x_i += relax z_i (the axpy expression) rides along since the sweep
// never reads x.  The last color's U rows are empty: its launch reads ro_u,
// w and x only.
template <typename TA, typename TV>
struct DiluBwdUpper {
    const TA* einv_s;
    TV* w;
    TV* x;
    TV relax;
    struct Own { TA e; TV w, x; };
    __device__ const TV* gathered() const { return w; }
    __device__ Own read(int t, int i) const { return {einv_s[t], w[i], x[i]}; }
    template <bool PINNED>
    __device__ void finish(int i, const Own& o, TV sum) const {
        TV z = o.w - row_times<PINNED, false>((TV)o.e, sum);
        w[i] = z;
        x[i] = o.x + row_times<PINNED, true>(relax, z);
    }
};

// Lane shape: LANES lanes per row (slab_row_dot_lanes), one where rows are
// short, 8 where they are long (the Galerkin levels); lane 0 does the row's
// own reads, after the product, and its stores.
template <int LANES, typename TA, typename TV, typename Rule>
__global__ __launch_bounds__(AMGX_BLOCK) void dilu_lane_kernel(
    const int* __restrict__ ro, const int* __restrict__ ci,
    const TA* __restrict__ va, const int* __restrict__ rows, int count,
    Rule rule) {
    long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g / LANES >= count) return;   // uniform over the lanes of a row
    int t = (int)(g / LANES);
    int lane = threadIdx.x & (LANES - 1);
    TV sum = slab_row_dot_lanes<LANES>(ro, ci, va, t, lane, rule.gathered());
    if (lane != 0) return;
    int i = rows[t];
    rule.template finish<false>(i, rule.read(t, i), sum);
}

// Stream shape (slab_row_dot_stream): a block of DILU_STREAM_WAVES waves, 64
// rows of the color per wave, one LDS region per wave. The row's own reads
// are issued ahead of the windows, so they overlap the slab loads. A wave
// past the color's end leaves as a whole, before any window; in the color's
// last wave a lane without a row reads as the color's last row (tc) and
// stores nothing.
constexpr int DILU_STREAM_WAVES = AMGX_BLOCK / 64;
static inline int dilu_stream_grid(int count) {
    const int per_block = DILU_STREAM_WAVES * DILU_STREAM_ROWS;
    return (count + per_block - 1) / per_block;
}
template <typename TA, typename TV, typename Rule>
__global__ __launch_bounds__(AMGX_BLOCK) void dilu_stream_kernel(
    const int* __restrict__ ro, const int* __restrict__ ci,
    const TA* __restrict__ va, const int* __restrict__ rows, int count,
    Rule rule) {
    __shared__ __attribute__((aligned(16))) char
        lds[DILU_STREAM_WAVES * DILU_STREAM_WINDOW_BYTES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long t0l =
        ((long long)blockIdx.x * DILU_STREAM_WAVES + wave) * DILU_STREAM_ROWS;
    if (t0l >= count) return;
    const int t0 = (int)t0l;
    const bool has_row = t0 + lane < count;
    const int tc = has_row ? t0 + lane : count - 1;
    int rs = ro[tc], re = ro[tc + 1];
    const int i = rows[tc];
    const auto own = rule.read(tc, i);
    if (!has_row) rs = re = 0;
    TV sum = slab_row_dot_stream(ci, va, t0, count, lane, rs, re,
                                 rule.gathered(),
                                 lds + wave * DILU_STREAM_WINDOW_BYTES);
    if (!has_row) return;
    rule.template finish<true>(i, own, sum);
}

// block forward: w_i = Einv_i (rhs_i - sum_{color(j)<c} A_ij w_j); w
// pre-zeroed so the full-row product only picks up earlier colors.
// block backward: z_i = w_i - Einv_i sum_{color(j)>c} A_ij z_j; z pre-zeroed
// and filled color-descending, so a full-row product sees only later colors.
template <typename TA, typename TV>
__global__ __launch_bounds__(AMGX_BLOCK) void dilu_fwd_block_sorted(
    const int* __restrict__ ro_s, const int* __restrict__ ci_s,
    const TA* __restrict__ va_s, const TA* __restrict__ einv_s,
    const int* __restrict__ rows, int count, const TV* __restrict__ r,
    TV* __restrict__ w, int b) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    int i = rows[t];
    TV acc[16];
    for (int c = 0; c < b; ++c) {
        TV sum = TV(0);
        for (int k = ro_s[t]; k < ro_s[t + 1]; ++k) {
            if (ci_s[k] == i) continue;
            const TA* blk = va_s + ((long long)k * b + c) * b;
            const TV* ws = w + (long long)ci_s[k] * b;
            for (int q = 0; q < b; ++q) sum += (TV)blk[q] * ws[q];
        }
        acc[c] = r[(long long)i * b + c] - sum;
    }
    const TA* E = einv_s + (long long)t * b * b;
    for (int c = 0; c < b; ++c) {
        TV s = TV(0);
        for (int q = 0; q < b; ++q) s += (TV)E[c * b + q] * acc[q];
        w[(long long)i * b + c] = s;
    }
}

template <typename TA, typename TV>
__global__ __launch_bounds__(AMGX_BLOCK) void dilu_bwd_block_sorted(
    const int* __restrict__ ro_s, const int* __restrict__ ci_s,
    const TA* __restrict__ va_s, const TA* __restrict__ einv_s,
    const int* __restrict__ rows, int count, const TV* __restrict__ wv,
    TV* __restrict__ z, int b) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    int i = rows[t];
    TV acc[16];
    for (int c = 0; c < b; ++c) {
        TV sum = TV(0);
        for (int k = ro_s[t]; k < ro_s[t + 1]; ++k) {
            if (ci_s[k] == i) continue;
            const TA* blk = va_s + ((long long)k * b + c) * b;
            const TV* zs = z + (long long)ci_s[k] * b;
            for (int q = 0; q < b; ++q) sum += (TV)blk[q] * zs[q];
        }
        acc[c] = sum;
    }
    const TA* E = einv_s + (long long)t * b * b;
    for (int c = 0; c < b; ++c) {
        TV s = TV(0);
        for (int q = 0; q < b; ++q) s += (TV)E[c * b + q] * acc[q];
        z[(long long)i * b + c] = wv[(long long)i * b + c] - s;
    }
}

// One-launch DILU apply for small scalar levels (the deep AMG tail): ONE
// single-workgroup launch runs `sweeps` whole applies back to back, every
// forward and backward color of each, with __syncthreads as the color
// barrier, where the per-color path pays 2 x colors + 1 launches per apply.
// The rows run the rules of the per-color kernels above, so the two paths
// give the same bits: FUSED sweeps the full slab (ro_f, ci_f, va_f) with
// DiluFwdFull, the kernel itself rewriting y = x + 0 at the start of every
// apply; plain sweeps the L slab (same three arguments) with DiluFwdLower;
// the backward sweep runs DiluBwdUpper over the U slab. Neither w nor y is
// read before this launch has written it.
// LF / LU lanes per row of the forward / backward slab (slab_row_dot_lanes).
// A color takes ceil(rows * LANES / blockDim) rounds; blockDim is a multiple
// of LANES, so the lanes of a row share a round, and no thread leaves a
// color before its barrier.
template <int LANES, typename TA, typename TV, typename Rule>
__device__ __forceinline__ void dilu_small_color(
    const int* __restrict__ ro, const int* __restrict__ ci,
    const TA* __restrict__ va, const int* __restrict__ rows, int s0, int s1,
    const Rule& rule) {
    const int lane = threadIdx.x & (LANES - 1);
    const int per_round = blockDim.x / LANES;
    for (int t0 = s0; t0 < s1; t0 += per_round) {
        int t = t0 + threadIdx.x / LANES;
        if (t < s1) {   // uniform over the lanes of a row
            TV sum = slab_row_dot_lanes<LANES>(ro, ci, va, t, lane,
                                               rule.gathered());
            if (lane == 0) {
                int i = rows[t];
                rule.template finish<false>(i, rule.read(t, i), sum);
            }
        }
    }
    __syncthreads();
}

template <int LF, int LU, typename TA, typename TV, bool FUSED>
__global__ __launch_bounds__(1024) void dilu_small_kernel(
    const int* __restrict__ ro_f, const int* __restrict__ ci_f,
    const TA* __restrict__ va_f, const int* __restrict__ ro_u,
    const int* __restrict__ ci_u, const TA* __restrict__ va_u,
    const TA* __restrict__ einv_s, const int* __restrict__ rows,
    const int* __restrict__ bounds, int ncolors, const TV* __restrict__ rhs,
    TV* w, TV* y, TV* x, TV relax, long long vec_n, int sweeps) {
    const auto fwd = [&] {
        if constexpr (FUSED)
            return DiluFwdFull<TA, TV>{einv_s, rhs, x, w, y};
        else
            return DiluFwdLower<TA, TV>{einv_s, rhs, w};
    }();
    const DiluBwdUpper<TA, TV> bwd{einv_s, w, x, relax};
    for (int sw = 0; sw < sweeps; ++sw) {
        if constexpr (FUSED) {
            for (long long j = threadIdx.x; j < vec_n; j += blockDim.x)
                y[j] = x[j] + TV(0);
            __syncthreads();
        }
        for (int c = 0; c < ncolors; ++c)
            dilu_small_color<LF, TA, TV>(ro_f, ci_f, va_f, rows, bounds[c],
                                         bounds[c + 1], fwd);
        for (int c = ncolors - 1; c >= 0; --c)
            dilu_small_color<LU, TA, TV>(ro_u, ci_u, va_u, rows, bounds[c],
                                         bounds[c + 1], bwd);
    }
}

template <typename TA, typename TV>
void dilu_small(const int* ro_f, const int* ci_f, const TA* va_f,
                const int* ro_u, const int* ci_u, const TA* va_u,
                const TA* einv_s, const int* rows, const int* bounds,
                int ncolors, const TV* rhs, TV* w, TV* y, TV* x, TV relax,
                long long vec_n, bool fused, int lanes_f, int lanes_u,
                int sweeps, hipStream_t s) {
    if ((lanes_f != 1 && lanes_f != 8) || (lanes_u != 1 && lanes_u != 8))
        throw std::runtime_error("dilu_small: lanes must be 1 or 8");
    if (sweeps <= 0) return;
#define DILU_SMALL_FORM(LF, LU)                                                \
    (fused ? dilu_small_kernel<LF, LU, TA, TV, true>                           \
           : dilu_small_kernel<LF, LU, TA, TV, false>)
    auto kern = lanes_f == 8
                    ? (lanes_u == 8 ? DILU_SMALL_FORM(8, 8)
                                    : DILU_SMALL_FORM(8, 1))
                    : (lanes_u == 8 ? DILU_SMALL_FORM(1, 8)
                                    : DILU_SMALL_FORM(1, 1));
#undef DILU_SMALL_FORM
    hipLaunchKernelGGL(kern, dim3(1), dim3(1024), 0, s, ro_f, ci_f, va_f,
                       ro_u, ci_u, va_u, einv_s, rows, bounds, ncolors, rhs,
                       w, y, x, relax, vec_n, sweeps);
}

// The one-launch apply as it was before the split slabs reached the small
// levels, kept for tests and bench_kernels.py to compare against: thread per
// row over the full slab in both sweeps, two gathered vectors in the fused
// forward sweep, w and z zeroed at every apply and the relaxed axpy as a
// pass of its own. Same bits as dilu_small: the extra terms are exact zeros.
template <typename TA, typename TV, bool FUSED>
__global__ __launch_bounds__(1024) void dilu_small_full_kernel(
    const int* __restrict__ ro_s, const int* __restrict__ ci_s,
    const TA* __restrict__ va_s, const TA* __restrict__ einv_s,
    const int* __restrict__ rows, const int* __restrict__ bounds,
    int ncolors, const TV* __restrict__ rhs, TV* __restrict__ w,
    TV* __restrict__ z, TV* __restrict__ x, TV relax, long long vec_n) {
    int tid = threadIdx.x;
    int nt = blockDim.x;
    for (long long i = tid; i < vec_n; i += nt) { w[i] = TV(0); z[i] = TV(0); }
    __syncthreads();
    for (int c = 0; c < ncolors; ++c) {
        int s0 = bounds[c], s1 = bounds[c + 1];
        for (int t = s0 + tid; t < s1; t += nt) {
            int i = rows[t];
            TV sum = TV(0);
            for (int k = ro_s[t]; k < ro_s[t + 1]; ++k) {
                int j = ci_s[k];
                sum += (TV)va_s[k] * (FUSED ? x[j] + w[j] : w[j]);
            }
            w[i] = (TV)einv_s[t] * (rhs[i] - sum);
        }
        __syncthreads();
    }
    for (int c = ncolors - 1; c >= 0; --c) {
        int s0 = bounds[c], s1 = bounds[c + 1];
        for (int t = s0 + tid; t < s1; t += nt) {
            int i = rows[t];
            TV sum = TV(0);
            for (int k = ro_s[t]; k < ro_s[t + 1]; ++k)
                sum += (TV)va_s[k] * z[ci_s[k]];
            z[i] = w[i] - (TV)einv_s[t] * sum;
        }
        __syncthreads();
    }
    long long xn = (long long)bounds[ncolors];
    for (long long i = tid; i < xn; i += nt) x[i] += relax * z[i];
}

template <typename TA, typename TV>
void dilu_small_full(const int* ro_s, const int* ci_s, const TA* va_s,
                     const TA* einv_s, const int* rows, const int* bounds,
                     int ncolors, const TV* rhs, TV* w, TV* z, TV* x,
                     TV relax, long long vec_n, bool fused, hipStream_t s) {
    auto kern = fused ? dilu_small_full_kernel<TA, TV, true>
                      : dilu_small_full_kernel<TA, TV, false>;
    hipLaunchKernelGGL(kern, dim3(1), dim3(1024), 0, s, ro_s, ci_s, va_s,
                       einv_s, rows, bounds, ncolors, rhs, w, z, x, relax,
                       vec_n);
}

// block matrices only (xres != nullptr selects the fused-residual sweep of
// block-4, rhs = b and xres = x; there is no fused kernel for generic block
// sizes); the scalar forward sweeps are dilu_fwd_full and dilu_fwd_lower
template <typename TA, typename TV>
void dilu_fwd_sorted(const int* ro_s, const int* ci_s, const TA* va_s,
                     const TA* einv_s, const int* rows, int count,
                     const TV* rhs, const TV* xres, TV* w, int b,
                     hipStream_t s) {
    if (count <= 0) return;
    if (b == 1) {
        throw std::runtime_error(
            "dilu_fwd_sorted: the scalar sweeps are dilu_fwd_full and "
            "dilu_fwd_lower");
    } else if constexpr (is_cplx<TV>::value) {
        throw std::runtime_error(
            "dilu_fwd_sorted: complex block matrices are unsupported");
    } else if (b == 4) {   // MFMA wave kernel (kernels_mfma.hip)
        dilu_fwd_b4_sorted<TA, TV>(ro_s, ci_s, va_s, einv_s, rows, count,
                                   rhs, xres, w, s);
    } else {
        hipLaunchKernelGGL((dilu_fwd_block_sorted<TA, TV>),
                           dim3(grid_1d(count)), dim3(AMGX_BLOCK), 0, s,
                           ro_s, ci_s, va_s, einv_s, rows, count, rhs, w, b);
    }
}

// block matrices only; the scalar backward sweep is dilu_bwd_upper
template <typename TA, typename TV>
void dilu_bwd_sorted(const int* ro_s, const int* ci_s, const TA* va_s,
                     const TA* einv_s, const int* rows, int count,
                     const TV* wv, TV* z, int b, hipStream_t s) {
    if (count <= 0) return;
    if (b == 1) {
        throw std::runtime_error(
            "dilu_bwd_sorted: the scalar sweep is dilu_bwd_upper");
    } else if constexpr (is_cplx<TV>::value) {
        throw std::runtime_error(
            "dilu_bwd_sorted: complex block matrices are unsupported");
    } else if (b == 4) {   // MFMA wave kernel (kernels_mfma.hip)
        dilu_bwd_b4_sorted<TA, TV>(ro_s, ci_s, va_s, einv_s, rows, count,
                                   wv, z, s);
    } else {
        hipLaunchKernelGGL((dilu_bwd_block_sorted<TA, TV>),
                           dim3(grid_1d(count)), dim3(AMGX_BLOCK), 0, s,
                           ro_s, ci_s, va_s, einv_s, rows, count, wv, z, b);
    }
}

// One color of a scalar per-color sweep: 1 or 8 lanes per row, or
// DILU_STREAM for the stream shape
template <typename TA, typename TV, typename Rule>
void dilu_lanes_launch(const char* name, int lanes, const int* ro,
                       const int* ci, const TA* va, const int* rows,
                       int count, Rule rule, hipStream_t s) {
    if (count <= 0) return;
    if (lanes == DILU_STREAM)
        hipLaunchKernelGGL((dilu_stream_kernel<TA, TV, Rule>),
                           dim3(dilu_stream_grid(count)), dim3(AMGX_BLOCK), 0,
                           s, ro, ci, va, rows, count, rule);
    else if (lanes == 8)
        hipLaunchKernelGGL((dilu_lane_kernel<8, TA, TV, Rule>),
                           dim3(grid_1d((long long)count * 8)),
                           dim3(AMGX_BLOCK), 0, s, ro, ci, va, rows, count,
                           rule);
    else if (lanes == 1)
        hipLaunchKernelGGL((dilu_lane_kernel<1, TA, TV, Rule>),
                           dim3(grid_1d(count)), dim3(AMGX_BLOCK), 0, s, ro,
                           ci, va, rows, count, rule);
    else
        throw std::runtime_error(std::string(name) +
                                 ": lanes must be 1, 8 or DILU_STREAM");
}

template <typename TV>
void dilu_y_init(const TV* x, TV* y, long long n, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL((dilu_y_init_kernel<TV>), dim3(grid_1d(n)),
                       dim3(AMGX_BLOCK), 0, s, x, y, n);
}

template <typename TA, typename TV>
void dilu_fwd_full(const int* ro_s, const int* ci_s, const TA* va_s,
                   const TA* einv_s, const int* rows, int count,
                   const TV* rhs, const TV* x, TV* w, TV* y, int lanes,
                   hipStream_t s) {
    dilu_lanes_launch<TA, TV>("dilu_fwd_full", lanes, ro_s, ci_s, va_s, rows,
                              count,
                              DiluFwdFull<TA, TV>{einv_s, rhs, x, w, y}, s);
}

template <typename TA, typename TV>
void dilu_fwd_lower(const int* ro_l, const int* ci_l, const TA* va_l,
                    const TA* einv_s, const int* rows, int count,
                    const TV* rhs, TV* w, int lanes, hipStream_t s) {
    dilu_lanes_launch<TA, TV>("dilu_fwd_lower", lanes, ro_l, ci_l, va_l, rows,
                              count, DiluFwdLower<TA, TV>{einv_s, rhs, w}, s);
}

template <typename TA, typename TV>
void dilu_bwd_upper(const int* ro_u, const int* ci_u, const TA* va_u,
                    const TA* einv_s, const int* rows, int count, TV* w,
                    TV* x, TV relax, int lanes, hipStream_t s) {
    dilu_lanes_launch<TA, TV>("dilu_bwd_upper", lanes, ro_u, ci_u, va_u, rows,
                              count,
                              DiluBwdUpper<TA, TV>{einv_s, w, x, relax}, s);
}

// ============================================================ transfers
template <typename T>
__global__ __launch_bounds__(AMGX_BLOCK) void restrict_kernel(const T* __restrict__ r,
                                const int* __restrict__ agg, long long n,
                                int b, T* __restrict__ rc) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         t < n * b; t += stride) {
        long long i = t / b;
        int c = (int)(t % b);
        atomicAdd(&rc[(long long)agg[i] * b + c], r[t]);
    }
}

template <typename T>
void restrict_agg(const T* r, const int* agg, int n, int b, T* rc,
                  hipStream_t s) {
    hipLaunchKernelGGL((restrict_kernel<T>),
                       dim3(grid_1d((long long)n * b, AMGX_BLOCK, 4096)),
                       dim3(AMGX_BLOCK), 0, s, r, agg, (long long)n, b, rc);
}

// deterministic restriction via the aggregate CSR structure (offsets into
// fine ids sorted by aggregate) — reference fillRowOffsetsAndColIndices R
// storage, src/aggregation/aggregation_amg_level.cu:323.
template <typename T>
__global__ __launch_bounds__(AMGX_BLOCK) void restrict_csr_kernel(const int* __restrict__ off,
                                    const int* __restrict__ fids,
                                    const T* __restrict__ r, long long nc,
                                    int b, T* __restrict__ rc) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         t < nc * b; t += stride) {
        long long I = t / b;
        int c = (int)(t % b);
        T sum = T(0);
        for (int k = off[I]; k < off[I + 1]; ++k)
            sum += r[(long long)fids[k] * b + c];
        rc[t] = sum;
    }
}

template <typename T>
void restrict_csr(const int* off, const int* fids, const T* r, int nc, int b,
                  T* rc, hipStream_t s) {
    hipLaunchKernelGGL((restrict_csr_kernel<T>),
                       dim3(grid_1d((long long)nc * b, AMGX_BLOCK, 4096)),
                       dim3(AMGX_BLOCK), 0, s, off, fids, r, (long long)nc, b,
                       rc);
}

template <typename T>
__global__ __launch_bounds__(AMGX_BLOCK) void prolongate_kernel(T* __restrict__ x, const T* __restrict__ xc,
                                  const int* __restrict__ agg, long long n,
                                  int b) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         t < n * b; t += stride) {
        long long i = t / b;
        int c = (int)(t % b);
        x[t] += xc[(long long)agg[i] * b + c];
    }
}

template <typename T>
void prolongate_agg(T* x, const T* xc, const int* agg, int n, int b,
                    hipStream_t s) {
    hipLaunchKernelGGL((prolongate_kernel<T>),
                       dim3(grid_1d((long long)n * b, AMGX_BLOCK, 4096)),
                       dim3(AMGX_BLOCK), 0, s, x, xc, agg, (long long)n, b);
}

// ============================================================ dense GEMV
// coarse solve x = Ainv b; n <= a few hundred -> wave-per-row.
template <typename TA, typename TV>
__global__ __launch_bounds__(AMGX_BLOCK) void dense_gemv_kernel(const TA* __restrict__ Ainv,
                                  const TV* __restrict__ b,
                                  TV* __restrict__ x, int n) {
    int row = blockIdx.x * (blockDim.x / WAVE_SIZE) + threadIdx.x / WAVE_SIZE;
    int lane = threadIdx.x & (WAVE_SIZE - 1);
    if (row >= n) return;
    TV sum = TV(0);
    const TA* arow = Ainv + (long long)row * n;
    for (int j = lane; j < n; j += WAVE_SIZE) sum += (TV)arow[j] * b[j];
    sum = wave_reduce_sum(sum);
    if (lane == 0) x[row] = sum;
}

template <typename TA, typename TV>
void dense_gemv(const TA* Ainv, const TV* b, TV* x, int n, hipStream_t s) {
    if (n <= 0) return;
    int waves_per_block = AMGX_BLOCK / WAVE_SIZE;
    int g = (n + waves_per_block - 1) / waves_per_block;
    hipLaunchKernelGGL((dense_gemv_kernel<TA, TV>), dim3(g), dim3(AMGX_BLOCK),
                       0, s, Ainv, b, x, n);
}

// ============================================================ gather
template <typename T>
__global__ __launch_bounds__(AMGX_BLOCK) void gather_kernel(const T* __restrict__ src,
                              const int* __restrict__ idx, long long count,
                              int b, T* __restrict__ dst) {
    long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count * b) return;
    long long i = t / b;
    int c = (int)(t % b);
    dst[t] = src[(long long)idx[i] * b + c];
}

template <typename T>
void gather(const T* src, const int* idx, int count, int b, T* dst,
            hipStream_t s) {
    if (count <= 0) return;
    hipLaunchKernelGGL((gather_kernel<T>),
                       dim3(grid_1d((long long)count * b)), dim3(AMGX_BLOCK),
                       0, s, src, idx, (long long)count, b, dst);
}

// ============================================================ instantiation
// over the type lists of core_api.h; complex types get the scalar-CSR
// kernels (Krylov, Jacobi, multicolor GS / DILU, transfers, dense GEMV),
// whose template bodies are the real ones. Block kernels stay real: their
// launchers compile the block branch out for complex types and throw.
#define INSTANTIATE_REAL(T)                                                     \
    AMGX_INSTANTIATE(axpy_dalpha, T)                                            \
    AMGX_INSTANTIATE(scal_drsqrt, T)
#define INSTANTIATE_VALUE(T)                                                    \
    AMGX_INSTANTIATE(reduce, T)                                                 \
    AMGX_INSTANTIATE(axpy, T)                                                   \
    AMGX_INSTANTIATE(axpby, T)                                                  \
    AMGX_INSTANTIATE(scal, T)                                                   \
    AMGX_INSTANTIATE(extract_diag, T)                                           \
    AMGX_INSTANTIATE(jacobi_dinv, T)                                            \
    AMGX_INSTANTIATE(dilu_setup_color, T)                                       \
    AMGX_INSTANTIATE(dilu_y_init, T)                                            \
    AMGX_INSTANTIATE(restrict_agg, T)                                           \
    AMGX_INSTANTIATE(restrict_csr, T)                                           \
    AMGX_INSTANTIATE(prolongate_agg, T)                                         \
    AMGX_INSTANTIATE(gather, T)
#define INSTANTIATE_REAL_PAIR(TA, TV)                                           \
    AMGX_INSTANTIATE(bsrmv, TA, TV)                                             \
    AMGX_INSTANTIATE(bsrmv_generic, TA, TV)
#define INSTANTIATE_VALUE_PAIR(TA, TV)                                          \
    AMGX_INSTANTIATE(csrmv, TA, TV)                                             \
    AMGX_INSTANTIATE(jacobi_smooth, TA, TV)                                     \
    AMGX_INSTANTIATE(dilu_small, TA, TV)                                        \
    AMGX_INSTANTIATE(dilu_small_full, TA, TV)                                   \
    AMGX_INSTANTIATE(dilu_fwd_sorted, TA, TV)                                   \
    AMGX_INSTANTIATE(dilu_bwd_sorted, TA, TV)                                   \
    AMGX_INSTANTIATE(dilu_fwd_full, TA, TV)                                     \
    AMGX_INSTANTIATE(dilu_fwd_lower, TA, TV)                                    \
    AMGX_INSTANTIATE(dilu_bwd_upper, TA, TV)                                    \
    AMGX_INSTANTIATE(gs_sweep_small, TA, TV)                                    \
    AMGX_INSTANTIATE(gs_rows_sorted, TA, TV)                                    \
    AMGX_INSTANTIATE(gs_smooth_rows, TA, TV)                                    \
    AMGX_INSTANTIATE(dense_gemv, TA, TV)

AMGX_REAL_TYPES(INSTANTIATE_REAL)
AMGX_VALUE_TYPES(INSTANTIATE_VALUE)
AMGX_REAL_PAIRS(INSTANTIATE_REAL_PAIR)
AMGX_VALUE_PAIRS(INSTANTIATE_VALUE_PAIR)

}  // namespace amgx_hip
