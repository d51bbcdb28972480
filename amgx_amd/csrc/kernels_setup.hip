// Setup-path kernels: MIN_MAX coloring rounds, SIZE_2 pairwise-matching
// aggregation, MULTI_PAIRWISE weights / matching / renumbering, sort-based
// Galerkin products / SpGEMM / transpose.
//
// Reference behaviors: src/matrix_coloring/min_max.cu,
// src/aggregation/selectors/size2_selector.cu,
// src/aggregation/selectors/multi_pairwise.cu,
// src/aggregation/coarseAgenerators/thrust_coarse_A_generator.cu (the
// sort/reduce_by_key Galerkin), src/csr_multiply_detail.cu (SpGEMM; here an
// ESC expand-sort-compress scheme on rocPRIM radix sort — the LDS-hash
// LOW_DEG-style kernel is a planned optimization), src/transpose.cu.
//
// rocPRIM is used only for device sort/scan/reduce primitives (design
// stance: SURVEY.md §7 — math kernels hand-written, rocPRIM for utilities).

#include <climits>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include <stdexcept>
#include <string>

#include "common.h"
#include "core_api.h"

namespace amgx_hip {

// ============================================================ coloring
__device__ __forceinline__ unsigned int hash_u32(unsigned int a,
                                                 unsigned int seed) {
    a ^= seed;
    a = (a ^ 61u) ^ (a >> 16);
    a *= 9u;
    a ^= a >> 4;
    a *= 0x27d4eb2du;
    a ^= a >> 15;
    return a;
}

// One greedy min-max round (reference src/matrix_coloring/
// greedy_min_max_2ring.cu class): an uncolored row whose hash is the strict
// max among uncolored neighbors takes the SMALLEST color not used by its
// already-colored neighbors — greedy-quality color counts (~max degree) with
// Jones-Plassmann parallel rounds. Hash fixed across rounds, tie-break on
// row id => deterministic. Colors >= 64 fall back past the bitmask (rare).
// mode 0: local max takes the smallest color unused by colored neighbors
// (greedy / PARALLEL_GREEDY quality); mode 1: local max takes color = iter
// (MULTI_HASH semantics, reference src/matrix_coloring/multi_hash.cu).
// Reads a FROZEN snapshot (colors_prev) and writes colors_next: same-round
// neighbor decisions must be invisible, or the result depends on wave
// scheduling — valid but nondeterministic (host model's frozen-snapshot
// semantics; determinism_flag discipline, reference src/core.cu:313).
// The round reports "a row is still uncolored" through *left, which the
// caller zeroes: the workgroup votes and one thread stores the constant 1, and
// only while it still reads 0, so the shared word sees a handful of plain
// stores per round instead of one read-modify-write per losing row. Every
// thread reaches the vote: no return stands ahead of it.
__global__ __launch_bounds__(AMGX_BLOCK) void color_round_kernel(const int* __restrict__ ro,
                                   const int* __restrict__ ci, int n,
                                   const int* __restrict__ colors_prev,
                                   int* __restrict__ colors_next, int iter,
                                   int seed, int mode, int* left) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    int lost = 0;
    if (i < n) {
        int out = colors_prev[i];
        if (out < 0) {
            unsigned long long mine =
                ((unsigned long long)hash_u32((unsigned)i, (unsigned)seed) << 32) |
                (unsigned)i;
            bool is_max = true;
            unsigned long long used = 0ull;
            int big_used_max = -1;
            for (int k = ro[i]; k < ro[i + 1]; ++k) {
                int j = ci[k];
                if (j == i || j >= n) continue;
                int cj = colors_prev[j];
                if (cj >= 0) {
                    if (cj < 64) used |= (1ull << cj);
                    else big_used_max = max(big_used_max, cj);
                    continue;
                }
                unsigned long long h =
                    ((unsigned long long)hash_u32((unsigned)j, (unsigned)seed) << 32) |
                    (unsigned)j;
                if (h > mine) { is_max = false; break; }
            }
            if (is_max) {
                if (mode == 1) {
                    out = iter;
                } else {
                    int c = (int)(__builtin_ffsll((long long)~used) - 1);
                    // beyond-bitmask: colors 0..63 are all taken
                    if (c < 0 || c >= 64) c = max(big_used_max, 63) + 1;
                    out = c;
                }
            } else {
                lost = 1;
            }
        }
        colors_next[i] = out;
    }
    if (__syncthreads_or(lost) && threadIdx.x == 0 && *left == 0) *left = 1;
}

void color_minmax_round(const int* ro, const int* ci, int n,
                        const int* colors_prev, int* colors_next, int iter,
                        int seed, int mode, int* left, hipStream_t s) {
    hipLaunchKernelGGL(color_round_kernel, dim3(grid_1d(n)), dim3(AMGX_BLOCK),
                       0, s, ro, ci, n, colors_prev, colors_next, iter, seed,
                       mode, left);
}

// *out = max(*out, max of v[0..n)): one atomic per workgroup of a capped grid
__global__ __launch_bounds__(AMGX_BLOCK) void int_max_kernel(
    const int* __restrict__ v, int n, int* __restrict__ out) {
    int m = INT_MIN;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x)
        m = max(m, v[i]);
    __shared__ int lds[AMGX_BLOCK];
    lds[threadIdx.x] = m;
    __syncthreads();
    for (int w = AMGX_BLOCK / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            lds[threadIdx.x] = max(lds[threadIdx.x], lds[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(out, lds[0]);
}

void int_max(const int* v, int n, int* out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(int_max_kernel, dim3(grid_1d(n, AMGX_BLOCK, 1024)),
                       dim3(AMGX_BLOCK), 0, s, v, n, out);
}

// ============================================================ aggregation
// Edge weight w_ij = (|a_ij| + |a_ji|) / sqrt(|a_ii| |a_jj|): symmetric
// strength used by the pairwise matching (reference size2_selector.cu).
template <typename T>
__device__ __forceinline__ double edge_weight(const T* va, const int* tidx,
                                              const T* diag, int k, int i,
                                              int j) {
    // absd: |.| in double, the modulus for complex values (cplx.h)
    double aij = absd(va[k]);
    double aji = tidx[k] >= 0 ? absd(va[tidx[k]]) : 0.0;
    double di = absd(diag[i]);
    double dj = absd(diag[j]);
    double scale = rsqrt((di > 0 ? di : 1.0) * (dj > 0 ? dj : 1.0));
    return (aij + aji) * scale;
}

// The weight of every entry once per level (0 where the propose kernel never
// asks: diagonal and halo columns), for the PRE form of the propose kernel.
// The expression is edge_weight itself, so both forms compare the same bits.
template <typename T>
__global__ __launch_bounds__(AMGX_BLOCK) void agg_edge_weights_kernel(
    const int* __restrict__ ro, const int* __restrict__ ci,
    const T* __restrict__ va, const int* __restrict__ tidx,
    const T* __restrict__ diag, int n, double* __restrict__ w) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int k = ro[i]; k < ro[i + 1]; ++k) {
        int j = ci[k];
        w[k] = (j == i || j >= n) ? 0.0 : edge_weight(va, tidx, diag, k, i, j);
    }
}

// PRE: read the weight of an entry from wpre (agg_edge_weights_kernel)
// instead of computing it from va, tidx and diag.
template <typename T, bool PRE>
__global__ __launch_bounds__(AMGX_BLOCK) void agg_propose_kernel(const int* __restrict__ ro,
                                   const int* __restrict__ ci,
                                   const T* __restrict__ va,
                                   const int* __restrict__ tidx,
                                   const T* __restrict__ diag,
                                   const double* __restrict__ wpre, int n,
                                   const int* __restrict__ agg,
                                   int* __restrict__ prop, int seed) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (agg[i] >= 0) { prop[i] = -1; return; }
    int best = -1;
    double bw = 0.0;
    unsigned int bt = 0;
    for (int k = ro[i]; k < ro[i + 1]; ++k) {
        int j = ci[k];
        if (j == i || j >= n || agg[j] >= 0) continue;
        double w = PRE ? wpre[k] : edge_weight(va, tidx, diag, k, i, j);
        // Weight ties broken by a seeded per-node hash key (mirrors the host
        // path's random tie[] and the reference's hashed weights,
        // src/aggregation/selectors/size2_selector.cu) — a pure row-id
        // tie-break makes every node on a uniform-weight matrix (Poisson!)
        // propose to its highest-numbered neighbor and handshakes stall.
        // Final fallback on row id keeps the result fully deterministic.
        unsigned int tj = hash_u32((unsigned)j, (unsigned)seed);
        if (w > bw ||
            (w == bw && best >= 0 &&
             (tj > bt || (tj == bt && j > best)))) {
            bw = w; best = j; bt = tj;
        }
    }
    prop[i] = best;
}

// *changed (zeroed by the caller) becomes 1 when the round forms a pair: a
// workgroup vote and one plain store, as color_round_kernel.
__global__ __launch_bounds__(AMGX_BLOCK) void agg_match_kernel(const int* __restrict__ prop, int n,
                                 int* __restrict__ agg, int* changed) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    int made = 0;
    if (i < n) {
        int j = prop[i];
        if (j >= 0 && prop[j] == i && i < j) {
            agg[i] = i;   // root id = smaller partner
            agg[j] = i;
            made = 1;
        }
    }
    if (__syncthreads_or(made) && threadIdx.x == 0 && *changed == 0)
        *changed = 1;
}

template <typename T>
__global__ __launch_bounds__(AMGX_BLOCK) void agg_singleton_kernel(const int* __restrict__ ro,
                                     const int* __restrict__ ci,
                                     const T* __restrict__ va,
                                     const int* __restrict__ tidx,
                                     const T* __restrict__ diag, int n,
                                     const int* __restrict__ agg_in,
                                     int* __restrict__ agg_out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (agg_in[i] >= 0) { agg_out[i] = agg_in[i]; return; }
    int best = -1;
    double bw = -1.0;
    for (int k = ro[i]; k < ro[i + 1]; ++k) {
        int j = ci[k];
        if (j == i || j >= n || agg_in[j] < 0) continue;
        double w = edge_weight(va, tidx, diag, k, i, j);
        if (w > bw || (w == bw && best >= 0 && agg_in[j] > agg_in[best])) {
            bw = w;
            best = j;
        }
    }
    agg_out[i] = best >= 0 ? agg_in[best] : i;
}

template <typename T>
void agg_edge_weights(const int* ro, const int* ci, const T* va,
                      const int* tidx, const T* diag, int n, double* w,
                      hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL((agg_edge_weights_kernel<T>), dim3(grid_1d(n)),
                       dim3(AMGX_BLOCK), 0, s, ro, ci, va, tidx, diag, n, w);
}

template <typename T>
void agg_propose(const int* ro, const int* ci, const T* va, const int* tidx,
                 const T* diag, const double* wpre, int n, const int* agg,
                 int* prop, int seed, hipStream_t s) {
    auto kern = wpre ? agg_propose_kernel<T, true>
                     : agg_propose_kernel<T, false>;
    hipLaunchKernelGGL(kern, dim3(grid_1d(n)), dim3(AMGX_BLOCK), 0, s, ro, ci,
                       va, tidx, diag, wpre, n, agg, prop, seed);
}

void agg_match(const int* prop, int n, int* agg, int* changed, hipStream_t s) {
    hipLaunchKernelGGL(agg_match_kernel, dim3(grid_1d(n)), dim3(AMGX_BLOCK),
                       0, s, prop, n, agg, changed);
}

template <typename T>
void agg_merge_singletons(const int* ro, const int* ci, const T* va,
                          const int* tidx, const T* diag, int n,
                          const int* agg_in, int* agg_out, hipStream_t s) {
    hipLaunchKernelGGL((agg_singleton_kernel<T>), dim3(grid_1d(n)),
                       dim3(AMGX_BLOCK), 0, s, ro, ci, va, tidx, diag, n,
                       agg_in, agg_out);
}

// ============================================================ MULTI_PAIRWISE
// Pairwise handshake matching on a precomputed weight graph w[nnz]
// (reference src/aggregation/selectors/multi_pairwise.cu). The matching
// kernels read w, never matrix values: the graph of a later pass is the
// Galerkin product of the weights and has no matrix behind it. Everything is
// deterministic: candidate edges are compared by the total order
// (w, h(lo, hi), lo, hi) on unordered pairs {lo, hi}, and the only atomics
// are integer max / min / add, whose result does not depend on arrival order.

// w_k for entry k = (i, j); 0 for the diagonal, a halo column, a missing
// transpose entry or a zero divisor. The operand order makes w_ij == w_ji
// bitwise: both sums are commutative. Contraction stays off so the value is
// the one the per-row host oracle computes.
template <typename T>
__device__ __forceinline__ double pairwise_weight(const T* __restrict__ va,
                                                  const int* __restrict__ tidx,
                                                  const T* __restrict__ diag,
                                                  int k, int i, int j, int n,
                                                  int formula) {
#pragma clang fp contract(off)
    if (j == i || j >= n) return 0.0;
    int t = tidx[k];
    if (t < 0) return 0.0;
    if (formula == 0) {
        double di = absd(diag[i]), dj = absd(diag[j]);
        double m = di > dj ? di : dj;
        if (!(m > 0.0)) return 0.0;
        return 0.5 * (absd(va[k]) + absd(va[t])) / m;
    }
    if constexpr (is_cplx<T>::value) {
        return 0.0;   // formula 1 is signed: rejected for complex by the caller
    } else {
        double di = (double)diag[i], dj = (double)diag[j];
        if (di == 0.0 || dj == 0.0) return 0.0;
        return -0.5 * ((double)va[k] / di + (double)va[t] / dj);
    }
}

template <typename T>
__global__ __launch_bounds__(AMGX_BLOCK) void pairwise_weights_kernel(
    const int* __restrict__ ro, const int* __restrict__ ci,
    const T* __restrict__ va, const int* __restrict__ tidx,
    const T* __restrict__ diag, int n, int formula, double* __restrict__ w) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int k = ro[i]; k < ro[i + 1]; ++k)
        w[k] = pairwise_weight(va, tidx, diag, k, i, ci[k], n, formula);
}

// 32-bit hash of the unordered pair {i, j}
__device__ __forceinline__ unsigned int pair_hash(int i, int j,
                                                  unsigned int seed) {
    unsigned int lo = (unsigned)min(i, j), hi = (unsigned)max(i, j);
    return hash_u32(hash_u32(lo, seed) ^ hi, seed);
}

// A row's candidate: the other end j of an edge (-1 = none), its weight and
// pair hash. cand_better(i, a, b): edge {i, a.j} is larger than {i, b.j}.
struct PairCand {
    double w;
    unsigned int h;
    int j;
};

__device__ __forceinline__ bool cand_better(int i, const PairCand& a,
                                            const PairCand& b) {
    if (a.j < 0) return false;
    if (b.j < 0) return true;
    if (a.w != b.w) return a.w > b.w;
    if (a.h != b.h) return a.h > b.h;
    int alo = min(i, a.j), blo = min(i, b.j);
    if (alo != blo) return alo > blo;
    return max(i, a.j) > max(i, b.j);
}

// Entry k of row i as a matching candidate: an edge (w > 0) to another local
// row that is unaggregated and fits under the cap together with i.
__device__ __forceinline__ PairCand match_cand(
    const int* __restrict__ ci, const double* __restrict__ w,
    const int* __restrict__ agg, const int* __restrict__ sizes, int k, int i,
    int n, int si, int cap, unsigned int seed) {
    PairCand c{0.0, 0u, -1};
    int j = ci[k];
    if (j == i || j >= n) return c;
    double wk = w[k];
    if (!(wk > 0.0) || agg[j] >= 0) return c;
    if ((long long)si + sizes[j] > (long long)cap) return c;
    c.w = wk;
    c.h = pair_hash(i, j, seed);
    c.j = j;
    return c;
}

// prop[i] = other end of the largest eligible edge of an unaggregated row,
// i itself if it has none, -1 for an aggregated row. One thread per row.
__global__ __launch_bounds__(AMGX_BLOCK) void pairwise_propose_kernel(
    const int* __restrict__ ro, const int* __restrict__ ci,
    const double* __restrict__ w, int n, const int* __restrict__ agg,
    const int* __restrict__ sizes, int cap, unsigned int seed,
    int* __restrict__ prop) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (agg[i] >= 0) { prop[i] = -1; return; }
    int si = sizes[i];
    PairCand best{0.0, 0u, -1};
    for (int k = ro[i]; k < ro[i + 1]; ++k) {
        PairCand c = match_cand(ci, w, agg, sizes, k, i, n, si, cap, seed);
        if (cand_better(i, c, best)) best = c;
    }
    prop[i] = best.j >= 0 ? best.j : i;
}

// L lanes per row with a shuffle arg-max over the same total order, for the
// wider rows of ghost-level graphs; gives exactly the thread-per-row
// proposal. Built for L = 8: 32 lanes measured slower at every average degree
// from 7 to 27 (profiles/NOTES.md).
template <int L>
__global__ __launch_bounds__(AMGX_BLOCK) void pairwise_propose_vec_kernel(
    const int* __restrict__ ro, const int* __restrict__ ci,
    const double* __restrict__ w, int n, const int* __restrict__ agg,
    const int* __restrict__ sizes, int cap, unsigned int seed,
    int* __restrict__ prop) {
    const int lane = threadIdx.x & (L - 1);
    long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t / L >= n) return;   // uniform over the L lanes of a row
    int i = (int)(t / L);
    if (agg[i] >= 0) {
        if (lane == 0) prop[i] = -1;
        return;
    }
    int si = sizes[i];
    PairCand best{0.0, 0u, -1};
    for (int k = ro[i] + lane; k < ro[i + 1]; k += L) {
        PairCand c = match_cand(ci, w, agg, sizes, k, i, n, si, cap, seed);
        if (cand_better(i, c, best)) best = c;
    }
#pragma unroll
    for (int off = L / 2; off > 0; off >>= 1) {
        PairCand o;
        o.w = __shfl_down(best.w, off, L);
        o.h = __shfl_down(best.h, off, L);
        o.j = __shfl_down(best.j, off, L);
        if (cand_better(i, o, best)) best = o;
    }
    if (lane == 0) prop[i] = best.j >= 0 ? best.j : i;
}

// Mutual proposals merge into the smaller row. Row i alone writes the state
// of i and of its partner, so the kernel has no race and no atomic.
__global__ __launch_bounds__(AMGX_BLOCK) void pairwise_match_kernel(
    const int* __restrict__ prop, int n, int* __restrict__ agg,
    int* __restrict__ sizes) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int j = prop[i];
    if (j > i && prop[j] == i) {
        agg[i] = i;
        agg[j] = i;
        sizes[i] += sizes[j];
    }
}

// *count += rows with agg < 0: block reduction, one atomic per block
__global__ __launch_bounds__(AMGX_BLOCK) void pairwise_count_kernel(
    const int* __restrict__ agg, int n, int* __restrict__ count) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    int c = block_reduce_sum<int>((i < n && agg[i] < 0) ? 1 : 0);
    if (threadIdx.x == 0 && c > 0) atomicAdd(count, c);
}

// Entry k of leftover row i as a join candidate: an edge to an aggregated
// row whose aggregate (root r) still fits i under the cap.
__device__ __forceinline__ PairCand join_cand(
    const int* __restrict__ ci, const double* __restrict__ w,
    const int* __restrict__ agg, const int* __restrict__ sizes, int k, int i,
    int n, int si, int cap, unsigned int seed) {
    PairCand c{0.0, 0u, -1};
    int j = ci[k];
    if (j == i || j >= n) return c;
    double wk = w[k];
    if (!(wk > 0.0)) return c;
    int r = agg[j];
    if (r < 0) return c;
    if (sizes && (long long)si + sizes[r] > (long long)cap) return c;
    c.w = wk;
    c.h = pair_hash(i, j, seed);
    c.j = j;
    return c;
}

// merge_singletons = 1, one double-buffered sweep: a leftover joins the
// aggregate at the other end of its largest edge, as agg_in shows it.
__global__ __launch_bounds__(AMGX_BLOCK) void pairwise_join_sweep_kernel(
    const int* __restrict__ ro, const int* __restrict__ ci,
    const double* __restrict__ w, int n, const int* __restrict__ agg_in,
    unsigned int seed, int* __restrict__ agg_out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int a = agg_in[i];
    if (a < 0) {
        PairCand best{0.0, 0u, -1};
        for (int k = ro[i]; k < ro[i + 1]; ++k) {
            PairCand c = join_cand(ci, w, agg_in, nullptr, k, i, n, 0, 0, seed);
            if (cand_better(i, c, best)) best = c;
        }
        if (best.j >= 0) a = agg_in[best.j];
    }
    agg_out[i] = a;
}

// merge_singletons = 2, one capped round in three steps. Bid: a leftover
// picks the root r of its largest fitting edge and raises bid_w[r] to the
// weight's bit pattern, which orders like the weight for w > 0.
__global__ __launch_bounds__(AMGX_BLOCK) void pairwise_bid_kernel(
    const int* __restrict__ ro, const int* __restrict__ ci,
    const double* __restrict__ w, int n, const int* __restrict__ agg,
    const int* __restrict__ sizes, int cap, unsigned int seed,
    int* __restrict__ bid_root, unsigned long long* __restrict__ bid_w) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int r = -1;
    if (agg[i] < 0) {
        PairCand best{0.0, 0u, -1};
        int si = sizes[i];
        for (int k = ro[i]; k < ro[i + 1]; ++k) {
            PairCand c = join_cand(ci, w, agg, sizes, k, i, n, si, cap, seed);
            if (cand_better(i, c, best)) best = c;
        }
        if (best.j >= 0) {
            r = agg[best.j];
            unsigned long long bits =
                (unsigned long long)__double_as_longlong(best.w);
            bid_w[i] = bits;   // own slot: a leftover is never a root
            atomicMax(&bid_w[r], bits);
        }
    }
    bid_root[i] = r;
}

// Among the bidders that hold a root's largest weight the smallest row wins.
__global__ __launch_bounds__(AMGX_BLOCK) void pairwise_bid_tie_kernel(
    int n, const int* __restrict__ bid_root,
    const unsigned long long* __restrict__ bid_w, int* __restrict__ bid_i) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int r = bid_root[i];
    if (r >= 0 && bid_w[i] == bid_w[r]) atomicMin(&bid_i[r], i);
}

// A root accepts its winner and clears its slots for the next round; the
// root's thread alone writes the root and the winner.
__global__ __launch_bounds__(AMGX_BLOCK) void pairwise_accept_kernel(
    int n, int* __restrict__ agg, int* __restrict__ sizes,
    unsigned long long* __restrict__ bid_w, int* __restrict__ bid_i) {
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    if (agg[r] != r) return;
    int i = bid_i[r];
    if (i < n) {
        agg[i] = r;
        sizes[r] += sizes[i];
        bid_i[r] = n;
    }
    bid_w[r] = 0ull;
}

// Renumbering: flag the roots (agg[i] == i; a row still at -1 becomes its
// own root), exclusive-scan the flags, map every row through its root's id
// and add up the member sizes per aggregate with integer atomics.
__global__ __launch_bounds__(AMGX_BLOCK) void pairwise_root_flag_kernel(
    int* __restrict__ agg, int n, int* __restrict__ ids) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    int f = 0;
    if (i < n) {
        if (agg[i] < 0) agg[i] = i;
        f = agg[i] == i ? 1 : 0;
    }
    ids[i] = f;   // ids[n] = 0 closes the exclusive scan
}

__global__ __launch_bounds__(AMGX_BLOCK) void pairwise_renumber_kernel(
    const int* __restrict__ agg, int n, const int* __restrict__ ids,
    const int* __restrict__ sizes_in, int* __restrict__ agg_out,
    int* __restrict__ sizes_out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int id = ids[agg[i]];
    agg_out[i] = id;
    atomicAdd(&sizes_out[id], sizes_in[i]);
}

template <typename T>
void pairwise_weights(const int* ro, const int* ci, const T* va,
                      const int* tidx, const T* diag, int n, int formula,
                      double* w, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL((pairwise_weights_kernel<T>), dim3(grid_1d(n)),
                       dim3(AMGX_BLOCK), 0, s, ro, ci, va, tidx, diag, n,
                       formula, w);
}

void pairwise_propose(const int* ro, const int* ci, const double* w, int n,
                      const int* agg, const int* sizes, int cap, int seed,
                      int lanes, int* prop, hipStream_t s) {
    if (n <= 0) return;
    if (lanes == 8) {
        hipLaunchKernelGGL((pairwise_propose_vec_kernel<8>),
                           dim3(grid_1d((long long)n * 8)), dim3(AMGX_BLOCK),
                           0, s, ro, ci, w, n, agg, sizes, cap,
                           (unsigned)seed, prop);
    } else if (lanes == 1) {
        hipLaunchKernelGGL(pairwise_propose_kernel, dim3(grid_1d(n)),
                           dim3(AMGX_BLOCK), 0, s, ro, ci, w, n, agg, sizes,
                           cap, (unsigned)seed, prop);
    } else {
        throw std::runtime_error("pairwise_propose: lanes must be 1 or 8");
    }
}

void pairwise_match(const int* prop, int n, int* agg, int* sizes,
                    hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(pairwise_match_kernel, dim3(grid_1d(n)),
                       dim3(AMGX_BLOCK), 0, s, prop, n, agg, sizes);
}

void pairwise_count_unaggregated(const int* agg, int n, int* count,
                                 hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(pairwise_count_kernel, dim3(grid_1d(n)),
                       dim3(AMGX_BLOCK), 0, s, agg, n, count);
}

void pairwise_join_sweep(const int* ro, const int* ci, const double* w, int n,
                         const int* agg_in, int seed, int* agg_out,
                         hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(pairwise_join_sweep_kernel, dim3(grid_1d(n)),
                       dim3(AMGX_BLOCK), 0, s, ro, ci, w, n, agg_in,
                       (unsigned)seed, agg_out);
}

void pairwise_join_capped(const int* ro, const int* ci, const double* w, int n,
                          int* agg, int* sizes, int cap, int seed,
                          int* bid_root, unsigned long long* bid_w, int* bid_i,
                          hipStream_t s) {
    if (n <= 0) return;
    dim3 g(grid_1d(n)), b(AMGX_BLOCK);
    hipLaunchKernelGGL(pairwise_bid_kernel, g, b, 0, s, ro, ci, w, n, agg,
                       sizes, cap, (unsigned)seed, bid_root, bid_w);
    hipLaunchKernelGGL(pairwise_bid_tie_kernel, g, b, 0, s, n, bid_root, bid_w,
                       bid_i);
    hipLaunchKernelGGL(pairwise_accept_kernel, g, b, 0, s, n, agg, sizes,
                       bid_w, bid_i);
}

size_t pairwise_renumber_tmp_bytes(int n) {
    size_t bytes = 0;
    int* p = nullptr;
    (void)rocprim::exclusive_scan(nullptr, bytes, p, p, 0, (size_t)n + 1,
                                  rocprim::plus<int>(), (hipStream_t)0);
    return bytes;
}

void pairwise_renumber(int* agg, int n, const int* sizes_in, int* ids,
                       void* tmp, size_t tmp_bytes, int* agg_out,
                       int* sizes_out, hipStream_t s) {
    hipLaunchKernelGGL(pairwise_root_flag_kernel,
                       dim3(grid_1d((long long)n + 1)), dim3(AMGX_BLOCK), 0,
                       s, agg, n, ids);
    HIP_CHECK(rocprim::exclusive_scan(tmp, tmp_bytes, ids, ids, 0,
                                      (size_t)n + 1, rocprim::plus<int>(),
                                      s));
    if (n <= 0) return;
    hipLaunchKernelGGL(pairwise_renumber_kernel, dim3(grid_1d(n)),
                       dim3(AMGX_BLOCK), 0, s, agg, n, ids, sizes_in, agg_out,
                       sizes_out);
}

// ============================================================ sort helpers
static void* dev_alloc(size_t bytes, hipStream_t s) {
    void* p = nullptr;
    if (bytes == 0) bytes = 16;   // degenerate empty-matrix paths
    HIP_CHECK(hipMallocAsync(&p, bytes, s));
    return p;
}
static void dev_free(void* p, hipStream_t s) { HIP_CHECK(hipFreeAsync(p, s)); }

__global__ __launch_bounds__(AMGX_BLOCK) void fill_row_ids(const int* __restrict__ ro, int n,
                             int* __restrict__ rows) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int k = ro[i]; k < ro[i + 1]; ++k) rows[k] = i;
}

template <typename T>
__global__ __launch_bounds__(AMGX_BLOCK) void make_agg_keys(const int* __restrict__ rows,
                              const int* __restrict__ ci,
                              const T* __restrict__ va,
                              const int* __restrict__ agg_row,
                              const int* __restrict__ agg_col, long long nnz,
                              long long ncmod, unsigned long long* __restrict__ keys,
                              T* __restrict__ vals) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         k < nnz; k += stride) {
        keys[k] = (unsigned long long)agg_row[rows[k]] * ncmod + agg_col[ci[k]];
        vals[k] = va[k];
    }
}

// decompose sorted unique keys -> CSR of the coarse matrix
__global__ __launch_bounds__(AMGX_BLOCK) void keys_to_csr(const unsigned long long* __restrict__ keys,
                            long long nnz_c, long long ncmod, long long nrows,
                            int* __restrict__ ro_c, int* __restrict__ ci_c) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         t < nnz_c; t += stride) {
        unsigned long long key = keys[t];
        int r = (int)(key / ncmod);
        ci_c[t] = (int)(key % ncmod);
        // row start: first t whose row is r
        int rprev = (t == 0) ? -1 : (int)(keys[t - 1] / ncmod);
        if (r != rprev)
            for (int q = rprev + 1; q <= r; ++q) ro_c[q] = (int)t;
        if (t == nnz_c - 1)
            for (long long q = r + 1; q <= nrows; ++q) ro_c[q] = (int)nnz_c;
    }
}

__global__ __launch_bounds__(AMGX_BLOCK) void make_agg_keys_perm(const int* __restrict__ rows,
                                   const int* __restrict__ ci,
                                   const int* __restrict__ agg_row,
                                   const int* __restrict__ agg_col,
                                   long long nnz, long long ncmod,
                                   unsigned long long* __restrict__ keys,
                                   int* __restrict__ perm) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         k < nnz; k += stride) {
        keys[k] = (unsigned long long)agg_row[rows[k]] * ncmod + agg_col[ci[k]];
        perm[k] = (int)k;
    }
}

__global__ __launch_bounds__(AMGX_BLOCK) void find_run_starts(const unsigned long long* __restrict__ keys,
                                long long nnz, int* __restrict__ starts,
                                unsigned int* __restrict__ nruns) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         t < nnz; t += stride) {
        if (t == 0 || keys[t] != keys[t - 1]) {
            unsigned int slot = atomicAdd(nruns, 1u);
            starts[slot] = (int)t;
        }
    }
}

__global__ __launch_bounds__(AMGX_BLOCK) void gather_keys(const unsigned long long* __restrict__ keys,
                            const int* __restrict__ starts, long long n,
                            unsigned long long* __restrict__ out) {
    long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) out[t] = keys[starts[t]];
}

// block variant: payload is the nz INDEX, blocks summed in a second pass
template <typename T>
__global__ __launch_bounds__(AMGX_BLOCK) void sum_blocks_by_run(const int* __restrict__ run_starts,
                                  const int* __restrict__ perm,
                                  const T* __restrict__ va_in, long long nnz_c,
                                  long long nnz, int bb, T* __restrict__ va_out) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         t < nnz_c * bb; t += stride) {
        long long run = t / bb;
        int off = (int)(t % bb);
        long long s = run_starts[run];
        long long e = (run + 1 < nnz_c) ? run_starts[run + 1] : nnz;
        T acc = T(0);
        for (long long q = s; q < e; ++q)
            acc += va_in[(long long)perm[q] * bb + off];
        va_out[t] = acc;
    }
}

// ============================================================ galerkin (agg)
template <typename T>
long long galerkin_agg(const int* ro, const int* ci, const T* va, int n,
                       long long nnz, const int* agg, const int* agg_col,
                       int nc, long long ncmod, int* ro_c,
                       int* ci_c, T* va_c, int bb, hipStream_t s) {
    using K = unsigned long long;
    int* rows = (int*)dev_alloc(nnz * sizeof(int), s);
    hipLaunchKernelGGL(fill_row_ids, dim3(grid_1d(n)), dim3(AMGX_BLOCK), 0, s,
                       ro, n, rows);
    K* keys = (K*)dev_alloc(nnz * sizeof(K) * 2, s);
    K* keys_alt = keys + nnz;
    long long nc_ll = ncmod;

    if (is_cplx<T>::value && bb != 1)
        throw std::runtime_error(
            "galerkin_agg: complex block matrices are unsupported");
    if (bb == 1) {
        T* vals = (T*)dev_alloc(nnz * sizeof(T) * 2, s);
        T* vals_alt = vals + nnz;
        hipLaunchKernelGGL((make_agg_keys<T>), dim3(grid_1d(nnz, AMGX_BLOCK, 4096)),
                           dim3(AMGX_BLOCK), 0, s, rows, ci, va, agg, agg_col,
                           nnz, nc_ll, keys, vals);
        size_t tmp_bytes = 0;
        rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys, keys_alt, vals,
                                  vals_alt, nnz, 0, 64, s);
        void* tmp = dev_alloc(tmp_bytes, s);
        rocprim::radix_sort_pairs(tmp, tmp_bytes, keys, keys_alt, vals,
                                  vals_alt, nnz, 0, 64, s);
        // reduce by key
        K* ukeys = keys;  // reuse
        size_t tmp2 = 0;
        unsigned int* nruns = (unsigned int*)dev_alloc(sizeof(unsigned int), s);
        rocprim::reduce_by_key(nullptr, tmp2, keys_alt, vals_alt, nnz, ukeys,
                               va_c, nruns, rocprim::plus<T>(),
                               rocprim::equal_to<K>(), s);
        void* tmpb = dev_alloc(tmp2, s);
        rocprim::reduce_by_key(tmpb, tmp2, keys_alt, vals_alt, nnz, ukeys,
                               va_c, nruns, rocprim::plus<T>(),
                               rocprim::equal_to<K>(), s);
        unsigned int h_runs = 0;
        HIP_CHECK(hipMemcpyAsync(&h_runs, nruns, sizeof(unsigned int),
                                 hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (h_runs == 0)
            HIP_CHECK(hipMemsetAsync(ro_c, 0, (nc + 1) * sizeof(int), s));
        hipLaunchKernelGGL(keys_to_csr, dim3(grid_1d(h_runs, AMGX_BLOCK, 4096)),
                           dim3(AMGX_BLOCK), 0, s, ukeys, (long long)h_runs,
                           nc_ll, (long long)nc, ro_c, ci_c);
        dev_free(tmp, s); dev_free(tmpb, s); dev_free(vals, s);
        dev_free(nruns, s); dev_free(keys, s); dev_free(rows, s);
        return (long long)h_runs;
    }
    // ---- block path: sort (key, nz-index) then sum blocks per run ----------
    int* perm = (int*)dev_alloc(nnz * sizeof(int) * 2, s);
    int* perm_alt = perm + nnz;
    hipLaunchKernelGGL(make_agg_keys_perm, dim3(grid_1d(nnz, AMGX_BLOCK, 4096)),
                       dim3(AMGX_BLOCK), 0, s, rows, ci, agg, agg_col, nnz,
                       nc_ll, keys, perm);
    size_t tmp_bytes = 0;
    rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys, keys_alt, perm,
                              perm_alt, nnz, 0, 64, s);
    void* tmp = dev_alloc(tmp_bytes, s);
    rocprim::radix_sort_pairs(tmp, tmp_bytes, keys, keys_alt, perm, perm_alt,
                              nnz, 0, 64, s);
    // run starts: t where key changes
    int* run_starts = (int*)dev_alloc((nnz + 1) * sizeof(int), s);
    unsigned int* nruns = (unsigned int*)dev_alloc(sizeof(unsigned int), s);
    HIP_CHECK(hipMemsetAsync(nruns, 0, sizeof(unsigned int), s));
    hipLaunchKernelGGL(find_run_starts, dim3(grid_1d(nnz, AMGX_BLOCK, 4096)),
                       dim3(AMGX_BLOCK), 0, s, keys_alt, nnz, run_starts,
                       nruns);
    unsigned int h_runs = 0;
    HIP_CHECK(hipMemcpyAsync(&h_runs, nruns, sizeof(unsigned int),
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (h_runs == 0) {
        HIP_CHECK(hipMemsetAsync(ro_c, 0, (nc + 1) * sizeof(int), s));
        dev_free(run_starts, s); dev_free(nruns, s); dev_free(perm, s);
        dev_free(tmp, s); dev_free(keys, s); dev_free(rows, s);
        return 0;
    }
    // sort run starts (they were written unordered via atomic)
    size_t tmp3 = 0;
    int* rs_alt = (int*)dev_alloc(h_runs * sizeof(int), s);
    rocprim::radix_sort_keys(nullptr, tmp3, run_starts, rs_alt, h_runs, 0, 32, s);
    void* tmpc = dev_alloc(tmp3, s);
    rocprim::radix_sort_keys(tmpc, tmp3, run_starts, rs_alt, h_runs, 0, 32, s);
    // unique keys at run starts -> csr; then sum blocks
    K* ukeys = keys;  // reuse front half
    hipLaunchKernelGGL(gather_keys, dim3(grid_1d(h_runs, AMGX_BLOCK, 4096)),
                       dim3(AMGX_BLOCK), 0, s, keys_alt, rs_alt,
                       (long long)h_runs, ukeys);
    hipLaunchKernelGGL(keys_to_csr, dim3(grid_1d(h_runs, AMGX_BLOCK, 4096)),
                       dim3(AMGX_BLOCK), 0, s, ukeys, (long long)h_runs, nc_ll,
                       (long long)nc, ro_c, ci_c);
    hipLaunchKernelGGL((sum_blocks_by_run<T>),
                       dim3(grid_1d((long long)h_runs * bb, AMGX_BLOCK, 4096)),
                       dim3(AMGX_BLOCK), 0, s, rs_alt, perm_alt, va, h_runs,
                       nnz, bb, va_c);
    dev_free(tmp, s); dev_free(tmpc, s); dev_free(rs_alt, s);
    dev_free(run_starts, s); dev_free(nruns, s); dev_free(perm, s);
    dev_free(keys, s); dev_free(rows, s);
    return (long long)h_runs;
}

// ============================================================ ESC SpGEMM
__global__ __launch_bounds__(AMGX_BLOCK) void expand_degree(const int* __restrict__ ciA,
                              const int* __restrict__ roB, long long nnzA,
                              unsigned long long* __restrict__ deg) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         k < nnzA; k += stride) {
        int c = ciA[k];
        deg[k] = (unsigned long long)(roB[c + 1] - roB[c]);
    }
}

template <typename T>
__global__ __launch_bounds__(AMGX_BLOCK) void expand_fill(const int* __restrict__ rowsA,
                            const int* __restrict__ ciA,
                            const T* __restrict__ vaA,
                            const int* __restrict__ roB,
                            const int* __restrict__ ciB,
                            const T* __restrict__ vaB, long long nnzA,
                            const unsigned long long* __restrict__ off,
                            long long ncolsB,
                            unsigned long long* __restrict__ keys,
                            T* __restrict__ vals) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         k < nnzA; k += stride) {
        int i = rowsA[k];
        int c = ciA[k];
        T av = vaA[k];
        unsigned long long o = off[k];
        for (int t = roB[c]; t < roB[c + 1]; ++t) {
            keys[o] = (unsigned long long)i * ncolsB + ciB[t];
            vals[o] = av * vaB[t];
            ++o;
        }
    }
}

template <typename T>
long long spgemm_esc(const int* roA, const int* ciA, const T* vaA, int m,
                     long long nnzA, const int* roB, const int* ciB,
                     const T* vaB, int k, int n, int* ro_c, int* ci_c, T* va_c,
                     hipStream_t s) {
    using K = unsigned long long;
    // per-nz expansion degrees + scan
    K* deg = (K*)dev_alloc((nnzA + 1) * sizeof(K), s);
    hipLaunchKernelGGL(expand_degree, dim3(grid_1d(nnzA, AMGX_BLOCK, 4096)),
                       dim3(AMGX_BLOCK), 0, s, ciA, roB, nnzA, deg);
    size_t tmp_bytes = 0;
    rocprim::exclusive_scan(nullptr, tmp_bytes, deg, deg, (K)0, nnzA + 1,
                            rocprim::plus<K>(), s);
    void* tmp = dev_alloc(tmp_bytes, s);
    rocprim::exclusive_scan(tmp, tmp_bytes, deg, deg, (K)0, nnzA + 1,
                            rocprim::plus<K>(), s);
    K total = 0;
    HIP_CHECK(hipMemcpyAsync(&total, deg + nnzA, sizeof(K),
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    dev_free(tmp, s);
    if (total == 0) {
        HIP_CHECK(hipMemsetAsync(ro_c, 0, (m + 1) * sizeof(int), s));
        dev_free(deg, s);
        return 0;
    }
    int* rowsA = (int*)dev_alloc(nnzA * sizeof(int), s);
    hipLaunchKernelGGL(fill_row_ids, dim3(grid_1d(m)), dim3(AMGX_BLOCK), 0, s,
                       roA, m, rowsA);
    K* keys = (K*)dev_alloc(total * sizeof(K) * 2, s);
    K* keys_alt = keys + total;
    T* vals = (T*)dev_alloc(total * sizeof(T) * 2, s);
    T* vals_alt = vals + total;
    hipLaunchKernelGGL((expand_fill<T>), dim3(grid_1d(nnzA, AMGX_BLOCK, 4096)),
                       dim3(AMGX_BLOCK), 0, s, rowsA, ciA, vaA, roB, ciB, vaB,
                       nnzA, deg, (long long)n, keys, vals);
    size_t tmp2 = 0;
    rocprim::radix_sort_pairs(nullptr, tmp2, keys, keys_alt, vals, vals_alt,
                              total, 0, 64, s);
    void* tmpb = dev_alloc(tmp2, s);
    rocprim::radix_sort_pairs(tmpb, tmp2, keys, keys_alt, vals, vals_alt,
                              total, 0, 64, s);
    unsigned int* nruns = (unsigned int*)dev_alloc(sizeof(unsigned int), s);
    size_t tmp3 = 0;
    rocprim::reduce_by_key(nullptr, tmp3, keys_alt, vals_alt, total, keys,
                           va_c, nruns, rocprim::plus<T>(),
                           rocprim::equal_to<K>(), s);
    void* tmpc = dev_alloc(tmp3, s);
    rocprim::reduce_by_key(tmpc, tmp3, keys_alt, vals_alt, total, keys, va_c,
                           nruns, rocprim::plus<T>(), rocprim::equal_to<K>(),
                           s);
    unsigned int h_runs = 0;
    HIP_CHECK(hipMemcpyAsync(&h_runs, nruns, sizeof(unsigned int),
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (h_runs == 0)
        HIP_CHECK(hipMemsetAsync(ro_c, 0, (m + 1) * sizeof(int), s));
    hipLaunchKernelGGL(keys_to_csr, dim3(grid_1d(h_runs, AMGX_BLOCK, 4096)),
                       dim3(AMGX_BLOCK), 0, s, keys, (long long)h_runs,
                       (long long)n, (long long)m, ro_c, ci_c);
    dev_free(tmpb, s); dev_free(tmpc, s); dev_free(nruns, s);
    dev_free(vals, s); dev_free(keys, s); dev_free(rowsA, s); dev_free(deg, s);
    return (long long)h_runs;
}

// ============================================================ transpose
template <typename T>
__global__ __launch_bounds__(AMGX_BLOCK) void gather_vals_rows(const int* __restrict__ perm,
                                 const T* __restrict__ va,
                                 const int* __restrict__ rows, long long nnz,
                                 T* __restrict__ va_t, int* __restrict__ ci_t) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         t < nnz; t += stride) {
        int p = perm[t];
        va_t[t] = va[p];
        ci_t[t] = rows[p];
    }
}

__global__ __launch_bounds__(AMGX_BLOCK) void cols_to_ro(const int* __restrict__ cols_sorted, long long nnz,
                           int n, int* __restrict__ ro_t) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         t < nnz; t += stride) {
        int c = cols_sorted[t];
        int cprev = (t == 0) ? -1 : cols_sorted[t - 1];
        if (c != cprev)
            for (int q = cprev + 1; q <= c; ++q) ro_t[q] = (int)t;
        if (t == nnz - 1)
            for (int q = c + 1; q <= n; ++q) ro_t[q] = (int)nnz;
    }
}

__global__ __launch_bounds__(AMGX_BLOCK) void iota_kernel(int* p, long long n) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n;
         t += stride)
        p[t] = (int)t;
}

template <typename T>
void transpose_csr(const int* ro, const int* ci, const T* va, int m, int n,
                   long long nnz, int* ro_t, int* ci_t, T* va_t,
                   hipStream_t s) {
    if (nnz == 0) {
        HIP_CHECK(hipMemsetAsync(ro_t, 0, (n + 1) * sizeof(int), s));
        return;
    }
    int* rows = (int*)dev_alloc(nnz * sizeof(int), s);
    hipLaunchKernelGGL(fill_row_ids, dim3(grid_1d(m)), dim3(AMGX_BLOCK), 0, s,
                       ro, m, rows);
    int* cols = (int*)dev_alloc(nnz * sizeof(int) * 2, s);
    int* cols_alt = cols + nnz;
    int* perm = (int*)dev_alloc(nnz * sizeof(int) * 2, s);
    int* perm_alt = perm + nnz;
    HIP_CHECK(hipMemcpyAsync(cols, ci, nnz * sizeof(int),
                             hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(iota_kernel, dim3(grid_1d(nnz, AMGX_BLOCK, 4096)),
                       dim3(AMGX_BLOCK), 0, s, perm, nnz);
    size_t tmp_bytes = 0;
    rocprim::radix_sort_pairs(nullptr, tmp_bytes, cols, cols_alt, perm,
                              perm_alt, nnz, 0, 32, s);
    void* tmp = dev_alloc(tmp_bytes, s);
    rocprim::radix_sort_pairs(tmp, tmp_bytes, cols, cols_alt, perm, perm_alt,
                              nnz, 0, 32, s);
    hipLaunchKernelGGL((gather_vals_rows<T>),
                       dim3(grid_1d(nnz, AMGX_BLOCK, 4096)), dim3(AMGX_BLOCK),
                       0, s, perm_alt, va, rows, nnz, va_t, ci_t);
    hipLaunchKernelGGL(cols_to_ro, dim3(grid_1d(nnz, AMGX_BLOCK, 4096)),
                       dim3(AMGX_BLOCK), 0, s, cols_alt, nnz, n, ro_t);
    dev_free(tmp, s); dev_free(perm, s); dev_free(cols, s); dev_free(rows, s);
}

// ============================================================ slab split
// Strict color-split of a color-sorted slab: the U (upper = true) or L part
// of the row at slot t keeps the entries with a local column j < n whose
// color is later (U) / earlier (L) than the row's, in slab order. Diagonal,
// same-color and halo entries belong to neither part (the comparison of
// dilu_setup_scalar).
template <bool UPPER>
__device__ __forceinline__ bool slab_split_keep(int j, int n, int c,
                                                const int* __restrict__ colors) {
    if (j >= n) return false;
    return UPPER ? colors[j] > c : colors[j] < c;
}

template <bool UPPER>
__global__ __launch_bounds__(AMGX_BLOCK) void slab_split_count_kernel(
    const int* __restrict__ ro_s, const int* __restrict__ ci_s,
    const int* __restrict__ rows, const int* __restrict__ colors, int n,
    int* __restrict__ counts) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n) return;
    int cnt = 0;
    if (t < n) {
        int c = colors[rows[t]];
        for (int k = ro_s[t]; k < ro_s[t + 1]; ++k)
            cnt += slab_split_keep<UPPER>(ci_s[k], n, c, colors) ? 1 : 0;
    }
    counts[t] = cnt;   // counts[n] = 0 closes the exclusive scan
}

template <bool UPPER>
__global__ __launch_bounds__(AMGX_BLOCK) void slab_split_fill_kernel(
    const int* __restrict__ ro_s, const int* __restrict__ ci_s,
    const int* __restrict__ rows, const int* __restrict__ colors, int n,
    const int* __restrict__ ro_x, int* __restrict__ ci_x,
    int* __restrict__ map_x) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    int c = colors[rows[t]];
    int o = ro_x[t];
    for (int k = ro_s[t]; k < ro_s[t + 1]; ++k) {
        int j = ci_s[k];
        if (slab_split_keep<UPPER>(j, n, c, colors)) {
            ci_x[o] = j;
            map_x[o] = k;
            ++o;
        }
    }
}

long long slab_split_count(const int* ro_s, const int* ci_s, const int* rows,
                           const int* colors, int n, bool upper, int* ro_x,
                           hipStream_t s) {
    auto kern = upper ? slab_split_count_kernel<true>
                      : slab_split_count_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(grid_1d((long long)n + 1)),
                       dim3(AMGX_BLOCK), 0, s, ro_s, ci_s, rows, colors, n,
                       ro_x);
    size_t tmp_bytes = 0;
    rocprim::exclusive_scan(nullptr, tmp_bytes, ro_x, ro_x, 0, (size_t)n + 1,
                            rocprim::plus<int>(), s);
    void* tmp = dev_alloc(tmp_bytes, s);
    rocprim::exclusive_scan(tmp, tmp_bytes, ro_x, ro_x, 0, (size_t)n + 1,
                            rocprim::plus<int>(), s);
    int total = 0;
    HIP_CHECK(hipMemcpyAsync(&total, ro_x + n, sizeof(int),
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    dev_free(tmp, s);
    return (long long)total;
}

void slab_split_fill(const int* ro_s, const int* ci_s, const int* rows,
                     const int* colors, int n, bool upper, const int* ro_x,
                     int* ci_x, int* map_x, hipStream_t s) {
    if (n <= 0) return;
    auto kern = upper ? slab_split_fill_kernel<true>
                      : slab_split_fill_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(grid_1d(n)), dim3(AMGX_BLOCK), 0, s, ro_s,
                       ci_s, rows, colors, n, ro_x, ci_x, map_x);
}

// ============================================================ instantiation
// aggregation setup (matching, Galerkin, ESC SpGEMM) over the value types;
// the transpose serves classical AMG only and stays real
#define INSTANTIATE_SETUP(T)                                                   \
    AMGX_INSTANTIATE(agg_propose, T)                                           \
    AMGX_INSTANTIATE(agg_edge_weights, T)                                      \
    AMGX_INSTANTIATE(agg_merge_singletons, T)                                  \
    AMGX_INSTANTIATE(pairwise_weights, T)                                      \
    AMGX_INSTANTIATE(galerkin_agg, T)                                         \
    AMGX_INSTANTIATE(spgemm_esc, T)
#define INSTANTIATE_SETUP_REAL(T) AMGX_INSTANTIATE(transpose_csr, T)

AMGX_VALUE_TYPES(INSTANTIATE_SETUP)
AMGX_REAL_TYPES(INSTANTIATE_SETUP_REAL)

}  // namespace amgx_hip
