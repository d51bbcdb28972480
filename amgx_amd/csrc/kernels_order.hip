// Orderings of the setup path, built once per level in int32: the stable
// order of rows by a small key (rows by color, fine rows by aggregate) with
// its offsets, the renumbering of matching roots, and the structure of the
// color-sorted slab. Each replaces a chain of int64 torch sorts, histograms
// and scans and gives the same values.
//
// rocPRIM serves as the sort / scan primitive only, as in kernels_setup.hip.

#include <cstring>

#include <rocprim/rocprim.hpp>

#include <stdexcept>
#include <string>

#include "common.h"
#include "core_api.h"

namespace amgx_hip {

namespace {

void* order_alloc(size_t bytes, hipStream_t s) {
    void* p = nullptr;
    if (bytes == 0) bytes = 16;
    HIP_CHECK(hipMallocAsync(&p, bytes, s));
    return p;
}
void order_free(void* p, hipStream_t s) { HIP_CHECK(hipFreeAsync(p, s)); }

void scan_exclusive(int* v, size_t count, hipStream_t s) {
    size_t tmp_bytes = 0;
    HIP_CHECK(rocprim::exclusive_scan(nullptr, tmp_bytes, v, v, 0, count,
                                      rocprim::plus<int>(), s));
    void* tmp = order_alloc(tmp_bytes, s);
    HIP_CHECK(rocprim::exclusive_scan(tmp, tmp_bytes, v, v, 0, count,
                                      rocprim::plus<int>(), s));
    order_free(tmp, s);
}

}  // namespace

// ============================================================ stable key order
// off[q] = first position of a key >= q in the sorted keys, off[nkeys] = n.
// A key outside [0, nkeys) is clamped, so a bad input cannot write outside
// off.
__global__ __launch_bounds__(AMGX_BLOCK) void keys_to_offsets_kernel(
    const int* __restrict__ sorted, int n, int nkeys, int* __restrict__ off) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    int c = min(max(sorted[t], 0), nkeys - 1);
    int cprev = t == 0 ? -1 : min(max(sorted[t - 1], 0), nkeys - 1);
    for (int q = cprev + 1; q <= c; ++q) off[q] = t;
    if (t == n - 1)
        for (int q = c + 1; q <= nkeys; ++q) off[q] = n;
}

__global__ __launch_bounds__(AMGX_BLOCK) void fill_int_kernel(
    int* __restrict__ p, int count, int v) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < count) p[t] = v;
}

void key_order(const int* keys, int n, int nkeys, int* order, int* off,
               hipStream_t s) {
    if (nkeys < 1) nkeys = 1;
    if (n <= 0) {
        hipLaunchKernelGGL(fill_int_kernel, dim3(grid_1d(nkeys + 1)),
                           dim3(AMGX_BLOCK), 0, s, off, nkeys + 1, 0);
        return;
    }
    // only the bits that the keys use take part: a radix pass per 4-8 bits
    unsigned bits = 1;
    while (bits < 31 && (1ll << bits) < (long long)nkeys) ++bits;
    int* sorted = (int*)order_alloc((size_t)n * sizeof(int), s);
    rocprim::counting_iterator<int> rows(0);
    size_t tmp_bytes = 0;
    HIP_CHECK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys, sorted, rows,
                                        order, (size_t)n, 0u, bits, s));
    void* tmp = order_alloc(tmp_bytes, s);
    // the radix sort is stable: equal keys keep ascending rows
    HIP_CHECK(rocprim::radix_sort_pairs(tmp, tmp_bytes, keys, sorted, rows,
                                        order, (size_t)n, 0u, bits, s));
    hipLaunchKernelGGL(keys_to_offsets_kernel, dim3(grid_1d(n)),
                       dim3(AMGX_BLOCK), 0, s, sorted, n, nkeys, off);
    order_free(tmp, s);
    order_free(sorted, s);
}

// ============================================================ root renumbering
__global__ __launch_bounds__(AMGX_BLOCK) void root_flag_kernel(
    const int* __restrict__ roots, int n, int* __restrict__ ids) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    ids[i] = (i < n && roots[i] == i) ? 1 : 0;   // ids[n] closes the scan
}

__global__ __launch_bounds__(AMGX_BLOCK) void root_map_kernel(
    const int* __restrict__ roots, int n, const int* __restrict__ ids,
    int* __restrict__ agg) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int r = roots[i];
    agg[i] = ids[min(max(r, 0), n - 1)];
}

void root_renumber(const int* roots, int n, int* ids, int* agg,
                   hipStream_t s) {
    hipLaunchKernelGGL(root_flag_kernel, dim3(grid_1d((long long)n + 1)),
                       dim3(AMGX_BLOCK), 0, s, roots, n, ids);
    scan_exclusive(ids, (size_t)n + 1, s);
    if (n <= 0) return;
    hipLaunchKernelGGL(root_map_kernel, dim3(grid_1d(n)), dim3(AMGX_BLOCK), 0,
                       s, roots, n, ids, agg);
}

// ============================================================ slab structure
// lengths of the permuted rows (ro_s[n] = 0 closes the scan) and the inverse
// of the permutation
__global__ __launch_bounds__(AMGX_BLOCK) void slab_lengths_kernel(
    const int* __restrict__ ro, const int* __restrict__ rows, int n,
    int* __restrict__ ro_s, int* __restrict__ slot_of_row) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n) return;
    int len = 0;
    if (t < n) {
        int i = rows[t];
        len = ro[i + 1] - ro[i];
        slot_of_row[i] = t;
    }
    ro_s[t] = len;
}

// LANES lanes walk the entries of slab row t: entry e of the row at slot t is
// entry ro[rows[t]] + e of the matrix
template <int LANES>
__global__ __launch_bounds__(AMGX_BLOCK) void slab_fill_kernel(
    const int* __restrict__ ro, const int* __restrict__ ci,
    const int* __restrict__ rows, int n, const int* __restrict__ ro_s,
    int* __restrict__ nzmap, int* __restrict__ ci_s) {
    long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long t = g / LANES;
    int lane = (int)(g % LANES);
    if (t >= n) return;
    int src = ro[rows[t]];
    int dst = ro_s[t];
    int len = ro_s[t + 1] - dst;
    for (int e = lane; e < len; e += LANES) {
        nzmap[dst + e] = src + e;
        ci_s[dst + e] = ci[src + e];
    }
}

long long slab_offsets(const int* ro, const int* rows, int n, int* ro_s,
                       int* slot_of_row, hipStream_t s) {
    hipLaunchKernelGGL(slab_lengths_kernel, dim3(grid_1d((long long)n + 1)),
                       dim3(AMGX_BLOCK), 0, s, ro, rows, n, ro_s,
                       slot_of_row);
    scan_exclusive(ro_s, (size_t)n + 1, s);
    int total = 0;
    HIP_CHECK(hipMemcpyAsync(&total, ro_s + n, sizeof(int),
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return (long long)total;
}

void slab_fill(const int* ro, const int* ci, const int* rows, int n,
               int lanes, const int* ro_s, int* nzmap, int* ci_s,
               hipStream_t s) {
    if (n <= 0) return;
    if (lanes == 8) {
        hipLaunchKernelGGL((slab_fill_kernel<8>),
                           dim3(grid_1d((long long)n * 8)), dim3(AMGX_BLOCK),
                           0, s, ro, ci, rows, n, ro_s, nzmap, ci_s);
    } else if (lanes == 1) {
        hipLaunchKernelGGL((slab_fill_kernel<1>), dim3(grid_1d(n)),
                           dim3(AMGX_BLOCK), 0, s, ro, ci, rows, n, ro_s,
                           nzmap, ci_s);
    } else {
        throw std::runtime_error("slab_fill: lanes must be 1 or 8");
    }
}

}  // namespace amgx_hip
