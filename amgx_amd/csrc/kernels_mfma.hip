// MFMA (matrix-core) block kernels for gfx950 — wave-structured block-4
// DILU and block SpMV (role of the reference's warp-structured NxN dispatch,
// src/solvers/multicolor_dilu_solver.cu:362-2922 and the tuned 4x4 bsrmv,
// src/multiply.cu:952-1143 — redesigned for 64-lane waves + CDNA4 MFMA,
// not translated).
//
// v_mfma_f64_4x4x4f64 fragment layout, decoded ON HARDWARE by the 64x64
// one-hot probe (profiles/mfma_discover.py, gpurun_out/mfma_layout_full.txt)
// — the 4 blocks are interleaved by quads, NOT contiguous 16-lane groups:
//   A[b][m][k] at lane 16k + 4b + m
//   B[b][k][n] at lane 16k + 4b + n
//   C[b][m][n] at lane 16m + 4b + n
// Lane roles used below: b = (lane>>2)&3 (block = row-group / nnz-slot),
// o = lane>>4 (the k index of A/B, the m index of C), q = lane&3 (the m
// index of A, the n index of B/C).
//
// Geometry (b = 4): one wave covers 4 block-rows (one per MFMA block).
// Each row's 16 lanes {16o + 4b + q} load its 4x4 values va[k*16 + o*4+q]
// (element (o,q), a fully coalesced 16-lane 128B segment per nnz); row
// sums reduce over q with two quad shuffles (every lane of the quad ends
// holding the component-o total = exactly the B-fragment layout), and the
// dense 4x4 algebra (Einv apply; the setup's Aij*Einvj*Aji) runs on the
// matrix pipe — one 4-block MFMA per step.

#include "common.h"
#include "core_api.h"

namespace amgx_hip {

namespace {

__device__ __forceinline__ double mfma4x4_4b(double a, double b, double c) {
    return __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c, 0, 0, 0);
}

// full-quad shuffle sum: every lane of a 4-lane quad ends with the total
__device__ __forceinline__ double quad_sum(double v) {
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    return v;
}

}  // namespace

// ---------------------------------------------------------------- probe
// Raw MFMA for the layout-validation GPU test / discovery script.
__global__ void mfma4_probe_kernel(const double* __restrict__ a_frag,
                                   const double* __restrict__ b_frag,
                                   double* __restrict__ c_frag) {
    int l = threadIdx.x;   // one wave
    double c = mfma4x4_4b(a_frag[l], b_frag[l], 0.0);
    c_frag[l] = c;
}

void mfma4_probe(const double* a, const double* b, double* c, hipStream_t s) {
    hipLaunchKernelGGL(mfma4_probe_kernel, dim3(1), dim3(64), 0, s, a, b, c);
}

// ---------------------------------------------------------------- DILU b=4
// Forward sweep, one color: w_i = Einv_i (r_i - sum_{color(j)<c} A_ij w_j).
// w is pre-zeroed outside so the full-row sum only picks up earlier colors.
// Reads the color-sorted matrix copy (ro_s/einv_s indexed by slot, pointers
// pre-offset to the color base; see kernels_solve.hip).
// FUSED folds the residual into the sweep: the gather becomes
// x[j]+w[j] against the FULL row (incl. diagonal; w_i is still zero), so
// w_i = Einv_i (b_i - A_i.x - sum_{earlier} A_ij w_j) in one matrix read.
template <typename TA, typename TV, bool FUSED>
__global__ __launch_bounds__(256) void dilu_fwd_b4_kernel(
    const int* __restrict__ ro, const int* __restrict__ ci,
    const TA* __restrict__ va, const TA* __restrict__ einv,
    const int* __restrict__ rows, int count, const TV* __restrict__ r,
    TV* __restrict__ w, const TV* __restrict__ xv) {
    int lane = threadIdx.x & 63;
    int b = (lane >> 2) & 3;             // MFMA block = row within wave
    int o = lane >> 4;                   // k index of A/B frags
    int q = lane & 3;                    // m of A frag / n of B,C frags
    int slot = blockIdx.x * 16 + (threadIdx.x >> 6) * 4 + b;
    bool valid = slot < count;
    int i = valid ? rows[slot] : 0;
    double acc = 0.0;
    long long ebase = (long long)slot * 16;
    if (valid) {
        int k0 = ro[slot], k1 = ro[slot + 1];
        for (int k = k0; k < k1; ++k) {
            int j = ci[k];
            if (!FUSED && j == i) continue;
            // element (row o, col q) of the 4x4 block — coalesced 16 lanes
            double a = (double)va[(long long)k * 16 + o * 4 + q];
            double x = (double)w[(long long)j * 4 + q];
            if (FUSED) x += (double)xv[(long long)j * 4 + q];
            acc += a * x;
        }
    }
    // component-o row sum lands in every lane of the quad = B frag layout
    acc = quad_sum(acc);
    double bfrag = valid ? ((double)r[(long long)i * 4 + o] - acc) : 0.0;
    // A frag: Einv[m=q][k=o] -> row-major elem q*4 + o
    double afrag = valid ? (double)einv[ebase + q * 4 + o] : 0.0;
    double c = mfma4x4_4b(afrag, bfrag, 0.0);   // C[m=o][n=q] at this lane
    if (valid && q == 0) w[(long long)i * 4 + o] = (TV)c;   // column n=0
}

// Backward sweep, one color: z_i = w_i - Einv_i sum_{color(j)>c} A_ij z_j.
template <typename TA, typename TV>
__global__ __launch_bounds__(256) void dilu_bwd_b4_kernel(
    const int* __restrict__ ro, const int* __restrict__ ci,
    const TA* __restrict__ va, const TA* __restrict__ einv,
    const int* __restrict__ rows, int count, const TV* __restrict__ wv,
    TV* __restrict__ z) {
    int lane = threadIdx.x & 63;
    int b = (lane >> 2) & 3;
    int o = lane >> 4;
    int q = lane & 3;
    int slot = blockIdx.x * 16 + (threadIdx.x >> 6) * 4 + b;
    bool valid = slot < count;
    int i = valid ? rows[slot] : 0;
    double acc = 0.0;
    long long ebase = (long long)slot * 16;
    if (valid) {
        int k0 = ro[slot], k1 = ro[slot + 1];
        for (int k = k0; k < k1; ++k) {
            int j = ci[k];
            if (j == i) continue;
            double a = (double)va[(long long)k * 16 + o * 4 + q];
            double x = (double)z[(long long)j * 4 + q];
            acc += a * x;
        }
    }
    acc = quad_sum(acc);
    double bfrag = valid ? acc : 0.0;
    double afrag = valid ? (double)einv[ebase + q * 4 + o] : 0.0;
    double c = mfma4x4_4b(afrag, bfrag, 0.0);
    if (valid && q == 0)
        z[(long long)i * 4 + o] = wv[(long long)i * 4 + o] - (TV)c;
}

// DILU setup, one color: E_i = D_i - sum_{color(j)<c} A_ij Einv_j A_ji,
// then einv_i = E_i^{-1}.  One wave per row; the wave walks the row 4 nnz
// at a time (one nnz per MFMA block b) and chains two MFMAs per chunk:
// T = Aij x Einvj, contrib = T x Aji (the chain needs one transpose
// shuffle: C layout has (m outer, n inner), the next A operand needs
// (k outer, m inner)).  Cross-block xor-folds (masks 4, 8) sum the 4
// chunks, then lane 0 inverts E through LDS.
template <typename TA>
__global__ __launch_bounds__(256) void dilu_setup_b4_kernel(
    const int* __restrict__ ro, const int* __restrict__ ci,
    const TA* __restrict__ va, const int* __restrict__ didx,
    const int* __restrict__ tidx, const int* __restrict__ colors,
    const int* __restrict__ rows, int count, int color,
    TA* __restrict__ einv) {
    __shared__ double Es[4][16];         // one 4x4 E per wave
    __shared__ double Is[4][16];
    int lane = threadIdx.x & 63;
    int wave = threadIdx.x >> 6;         // 4 waves per WG, one row each
    int slot = blockIdx.x * 4 + wave;
    bool valid = slot < count;
    int i = valid ? rows[slot] : 0;
    int g = (lane >> 2) & 3;             // MFMA block = nnz sub-slot 0..3
    int o = lane >> 4;                   // outer field
    int q = lane & 3;                    // inner field
    int dk = valid ? didx[i] : -1;
    double e_acc = 0.0;
    if (valid) {
        int k0 = ro[i], k1 = ro[i + 1];
        for (int kb = k0; kb < k1; kb += 4) {
            int k = kb + g;
            bool act = k < k1;
            int j = act ? ci[k] : i;
            int tk = act ? tidx[k] : -1;
            bool use = act && j != i && tk >= 0 && colors[j] < color;
            // T = Aij x Einvj: A frag elem (m=q, k=o) -> Aij[q][o];
            //                  B frag elem (k=o, n=q) -> Einvj[o][q]
            double a1 = use ? (double)va[(long long)k * 16 + q * 4 + o]
                            : 0.0;
            double b1 = use ? (double)einv[(long long)j * 16 + o * 4 + q]
                            : 0.0;
            double Tc = mfma4x4_4b(a1, b1, 0.0);  // T[m=o][n=q] here
            // contrib = T x Aji: next A operand needs T[m=q][k=o], which
            // lives at lane 16q + 4g + o -> transpose shuffle
            double a2 = __shfl(Tc, 16 * q + 4 * g + o, 64);
            double b2 = use ? (double)va[(long long)tk * 16 + o * 4 + q]
                            : 0.0;
            e_acc = mfma4x4_4b(a2, b2, e_acc);    // C[m=o][n=q]
        }
    }
    // fold the 4 nnz sub-slots: blocks live in the 4b lane field
    e_acc += __shfl_xor(e_acc, 4, 64);
    e_acc += __shfl_xor(e_acc, 8, 64);
    // E = D - sum; element here is (m=o, n=q) -> row-major o*4 + q
    if (g == 0) {
        // a row without a stored diagonal block has D_i = 0, as in
        // dilu_setup_block and on the host
        double d = (valid && dk >= 0)
                       ? (double)va[(long long)dk * 16 + o * 4 + q]
                       : 0.0;
        Es[wave][o * 4 + q] = d - e_acc;
    }
    __syncthreads();
    // inversion and stabilized fallback (rule at dilu_keep_inverse,
    // common.h): lane 0 of each wave (setup-time)
    if (valid && lane == 0) {
        double emax = 0.0, dmax = 0.0;
        for (int s = 0; s < 16; ++s) {
            emax = fmax(emax, fabs(Es[wave][s]));
            double dv = dk >= 0 ? fabs((double)va[(long long)dk * 16 + s])
                                : 0.0;
            dmax = fmax(dmax, dv);
        }
        double pmin = small_mat_inv(Es[wave], Is[wave], 4);
        if (!dilu_keep_inverse<TA>(emax, pmin, dmax)) {
            for (int s = 0; s < 16; ++s)
                Es[wave][s] = dk >= 0 ? (double)va[(long long)dk * 16 + s]
                                      : (s % 5 == 0 ? 1.0 : 0.0);
            small_mat_inv(Es[wave], Is[wave], 4);
        }
    }
    __syncthreads();
    if (valid && lane < 16)
        einv[(long long)i * 16 + lane] = (TA)Is[wave][lane];
}

// xres != nullptr selects the fused-residual sweep (r = b, xres = x)
template <typename TA, typename TV>
void dilu_fwd_b4_sorted(const int* ro_s, const int* ci_s, const TA* va_s,
                        const TA* einv_s, const int* rows, int count,
                        const TV* r, const TV* xres, TV* w, hipStream_t s) {
    if (count <= 0) return;
    auto kern = xres ? dilu_fwd_b4_kernel<TA, TV, true>
                     : dilu_fwd_b4_kernel<TA, TV, false>;
    hipLaunchKernelGGL(kern, dim3((count + 15) / 16), dim3(256), 0, s, ro_s,
                       ci_s, va_s, einv_s, rows, count, r, w, xres);
}

template <typename TA, typename TV>
void dilu_bwd_b4_sorted(const int* ro_s, const int* ci_s, const TA* va_s,
                        const TA* einv_s, const int* rows, int count,
                        const TV* w, TV* z, hipStream_t s) {
    if (count <= 0) return;
    hipLaunchKernelGGL((dilu_bwd_b4_kernel<TA, TV>),
                       dim3((count + 15) / 16), dim3(256), 0, s, ro_s, ci_s,
                       va_s, einv_s, rows, count, w, z);
}

template <typename TA>
void dilu_setup_b4(const int* ro, const int* ci, const TA* va,
                   const int* didx, const int* tidx, const int* colors,
                   const int* rows, int count, int color, TA* einv,
                   hipStream_t s) {
    if (count <= 0) return;
    hipLaunchKernelGGL((dilu_setup_b4_kernel<TA>), dim3((count + 3) / 4),
                       dim3(256), 0, s, ro, ci, va, didx, tidx, colors, rows,
                       count, color, einv);
}

// ---------------------------------------------------------------- bsrmv b=4
// y = alpha * A x + beta * y (block-4 rows; wave covers 4 rows with the
// same coalesced element-(o,q) block loads; no MFMA needed — the row sums
// are quad reductions and the result is written directly).
template <typename TA, typename TV>
__global__ __launch_bounds__(256) void bsrmv_b4_kernel(
    const int* __restrict__ ro, const int* __restrict__ ci,
    const TA* __restrict__ va, const TV* __restrict__ x,
    TV* __restrict__ y, const TV* __restrict__ bvec, double alpha,
    double beta, double gamma, int row_begin, int row_end) {
    int lane = threadIdx.x & 63;
    int b = (lane >> 2) & 3;
    int o = lane >> 4;
    int q = lane & 3;
    int i = row_begin + blockIdx.x * 16 + (threadIdx.x >> 6) * 4 + b;
    if (i >= row_end) return;
    double acc = 0.0;
    int k0 = ro[i], k1 = ro[i + 1];
    for (int k = k0; k < k1; ++k) {
        double a = (double)va[(long long)k * 16 + o * 4 + q];
        double xv = (double)x[(long long)ci[k] * 4 + q];
        acc += a * xv;
    }
    acc = quad_sum(acc);
    if (q == 0) {
        long long idx = (long long)i * 4 + o;
        double out = alpha * acc;
        if (beta != 0.0) out += beta * (double)y[idx];
        if (gamma != 0.0 && bvec) out += gamma * (double)bvec[idx];
        y[idx] = (TV)out;
    }
}

template <typename TA, typename TV>
void bsrmv_b4(const int* ro, const int* ci, const TA* va, const TV* x,
              TV* y, const TV* bvec, double alpha, double beta, double gamma,
              int row_begin, int row_end, hipStream_t s) {
    int count = row_end - row_begin;
    if (count <= 0) return;
    hipLaunchKernelGGL((bsrmv_b4_kernel<TA, TV>), dim3((count + 15) / 16),
                       dim3(256), 0, s, ro, ci, va, x, y, bvec, alpha, beta,
                       gamma, row_begin, row_end);
}

// generic wave-structured block SpMV for b in 2..8: GROUP lanes per row
// (first B*B active, element (r=t/B, q=t%B)) so va[k*B*B + t] is a
// coalesced contiguous load per nnz; component sums fold with B-1 wave
// shuffles (arbitrary-B segments, so plain __shfl reads instead of xor).
template <typename TA, typename TV, int B, int GROUP>
__global__ __launch_bounds__(256) void bsrmv_bn_kernel(
    const int* __restrict__ ro, const int* __restrict__ ci,
    const TA* __restrict__ va, const TV* __restrict__ x,
    TV* __restrict__ y, const TV* __restrict__ bvec, double alpha,
    double beta, double gamma, int row_begin, int row_end) {
    constexpr int RPW = 64 / GROUP;          // rows per wave
    int lane = threadIdx.x & 63;
    int g = lane / GROUP;
    int t = lane % GROUP;
    int i = row_begin + blockIdx.x * (4 * RPW) + (threadIdx.x >> 6) * RPW
            + g;
    bool active = (t < B * B) && (i < row_end);
    int r = t / B;
    int q = t - r * B;
    double acc = 0.0;
    if (active) {
        int k0 = ro[i], k1 = ro[i + 1];
        for (int k = k0; k < k1; ++k) {
            double a = (double)va[(long long)k * B * B + t];
            double xv = (double)x[(long long)ci[k] * B + q];
            acc += a * xv;
        }
    }
    // fold over q: lanes (laneBase + r*B + 0..B-1); all lanes shuffle
    int base = lane - t;
    double s = acc;
#pragma unroll
    for (int qq = 1; qq < B; ++qq)
        s += __shfl(acc, base + r * B + qq, 64);
    if (active && q == 0) {
        long long idx = (long long)i * B + r;
        double out = alpha * s;
        if (beta != 0.0) out += beta * (double)y[idx];
        if (gamma != 0.0 && bvec) out += gamma * (double)bvec[idx];
        y[idx] = (TV)out;
    }
}

template <typename TA, typename TV>
void bsrmv_bn(const int* ro, const int* ci, const TA* va, int b,
              const TV* x, TV* y, const TV* bvec, double alpha, double beta,
              double gamma, int row_begin, int row_end, hipStream_t s) {
    int count = row_end - row_begin;
    if (count <= 0) return;
    auto launch = [&](auto kern, int rpw) {
        int rows_per_wg = 4 * rpw;
        hipLaunchKernelGGL(kern, dim3((count + rows_per_wg - 1)
                                      / rows_per_wg), dim3(256), 0, s, ro,
                           ci, va, x, y, bvec, alpha, beta, gamma,
                           row_begin, row_end);
    };
    switch (b) {
        case 2: launch(bsrmv_bn_kernel<TA, TV, 2, 4>, 16); break;
        case 3: launch(bsrmv_bn_kernel<TA, TV, 3, 16>, 4); break;
        case 5: launch(bsrmv_bn_kernel<TA, TV, 5, 32>, 2); break;
        case 6: launch(bsrmv_bn_kernel<TA, TV, 6, 64>, 1); break;
        case 7: launch(bsrmv_bn_kernel<TA, TV, 7, 64>, 1); break;
        case 8: launch(bsrmv_bn_kernel<TA, TV, 8, 64>, 1); break;
        default: break;   // caller guards
    }
}

// ------------------------------------------------------------ instantiation
#define INSTANTIATE_MFMA_PAIR(TA, TV)                                         \
    AMGX_INSTANTIATE(dilu_fwd_b4_sorted, TA, TV)                              \
    AMGX_INSTANTIATE(dilu_bwd_b4_sorted, TA, TV)                              \
    AMGX_INSTANTIATE(bsrmv_b4, TA, TV)                                        \
    AMGX_INSTANTIATE(bsrmv_bn, TA, TV)
#define INSTANTIATE_MFMA(TA) AMGX_INSTANTIATE(dilu_setup_b4, TA)

AMGX_REAL_TYPES(INSTANTIATE_MFMA)
AMGX_REAL_PAIRS(INSTANTIATE_MFMA_PAIR)

}  // namespace amgx_hip
