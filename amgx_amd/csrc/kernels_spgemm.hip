// LDS-hash SpGEMM + hash aggregation-Galerkin for gfx950 (role of the
// reference's warp-hash csr_multiply family, src/csr_multiply_detail.cu:
// 51-214,945-1500, include/hash_containers_detail.inl, and the LOW_DEG
// coarse-A generator, src/aggregation/coarseAgenerators/
// low_deg_coarse_A_generator.cu — redesigned for 64-lane waves and 160 KB
// LDS, not translated: linear-probe open addressing instead of the
// reference's cuckoo-ish two-table scheme, per-wave in-LDS bitonic sort
// for ordered rows instead of global radix passes).
//
// Scheme (count-then-fill, like the reference):
//   count pass: wave-per-row LDS hash SET of C-column ids -> exact row nnz
//   exclusive scan (rocPRIM) -> C row offsets
//   fill pass:  wave-per-row LDS hash MAP (col -> accumulated value),
//               compacted + bitonic-sorted in LDS, written coalesced
// Rows overflowing the 4-wave/WG capacity run again in a 1-wave/WG kernel
// with a 8-16x larger table (80-96 KB LDS); rows beyond THAT fall back to
// the ESC sort path at the Python dispatch level (rare: >8k nnz per row,
// >4k for complex128 values).
//
// The color-aware ILU(1) fill pattern at the end of the file is a keys-only
// user of the same hash set, ladder and sort.

#include <cstring>

#include <rocprim/rocprim.hpp>

#include <vector>

#include "common.h"
#include "core_api.h"

namespace amgx_hip {

namespace {

constexpr int TINY_CAP = 64;       // per-wave table, 8 waves per WG —
                                   // right-sized for AMG rows (<=64 nnz)
constexpr int SMALL_CAP = 512;     // per-wave table, 4 waves per WG
// top tier, 1 wave per WG: spgemm_hash_top_cap<T>() of core_api.h, 8192
// entries (4096 for cplx<double>)

// LDS bytes of one spgemm_fill_kernel workgroup: keys + values per wave, the
// compaction copy of both in the sorted tiers (one dummy element each
// otherwise) and the per-wave cursor
constexpr int LDS_BYTES = 160 * 1024;       // per CU on gfx950
template <typename T>
constexpr long long fill_lds_bytes(int cap, int waves, bool sorted) {
    long long entry = (long long)(sizeof(int) + sizeof(T));
    return waves * (cap * entry + (sorted ? cap : 1) * entry
                    + (long long)sizeof(int));
}

__device__ __forceinline__ unsigned int hash_col(int c) {
    unsigned int a = (unsigned int)c;
    a = (a ^ 61u) ^ (a >> 16);
    a *= 9u;
    a ^= a >> 4;
    a *= 0x27d4eb2du;
    a ^= a >> 15;
    return a;
}

// hash-SET insert (count pass): returns +1 if newly inserted, 0 if present,
// -1 on table-full overflow.
//
// Probe budget of hset_insert and hmap_add: `visited` counts the slots a key
// has moved past, not loop iterations. A lane that loses the CAS for an empty
// slot to another key looks at the same slot again, finds it occupied and
// moves on; that retry costs no budget. A key therefore gives up only after
// it has seen all cap slots occupied by other keys, so a row whose distinct
// keys fit the table cannot fail, however many lanes insert at once.
__device__ __forceinline__ int hset_insert(int* keys, int cap, int key) {
    unsigned int h = hash_col(key) & (cap - 1);
    for (int visited = 0; visited < cap;) {
        int k0 = keys[h];
        if (k0 == key) return 0;
        if (k0 == -1) {
            int old = atomicCAS(&keys[h], -1, key);
            if (old == -1) return 1;
            if (old == key) return 0;
            continue;      // slot stolen by another key: retry same slot
        }
        h = (h + 1) & (cap - 1);
        ++visited;
    }
    return -1;
}

// hash-MAP accumulate (fill pass). A complex value takes one LDS atomic per
// part (cplx.h); the fill kernel reads a slot only after the wave barrier
// that follows its accumulation loop.
template <typename T>
__device__ __forceinline__ bool hmap_add(int* keys, T* vals, int cap,
                                         int key, T v) {
    unsigned int h = hash_col(key) & (cap - 1);
    for (int visited = 0; visited < cap;) {
        int k0 = keys[h];
        if (k0 == key) { atomicAdd(&vals[h], v); return true; }
        if (k0 == -1) {
            int old = atomicCAS(&keys[h], -1, key);
            if (old == -1 || old == key) {
                atomicAdd(&vals[h], v);
                return true;
            }
            continue;      // slot stolen by another key: retry same slot
        }
        h = (h + 1) & (cap - 1);
        ++visited;
    }
    return false;
}

// wave-cooperative bitonic sort of (key,val) pairs [0,p) in LDS, p = pow2
template <typename T>
__device__ __forceinline__ void wave_bitonic(int* k, T* v, int p, int lane) {
    for (int size = 2; size <= p; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __builtin_amdgcn_s_waitcnt(0);
            __builtin_amdgcn_wave_barrier();
            for (int idx = lane; idx < p / 2; idx += 64) {
                int half = idx / stride;
                int lo = half * 2 * stride + (idx % stride);
                int hi = lo + stride;
                bool up = ((lo & size) == 0);
                int ka = k[lo], kb = k[hi];
                if ((ka > kb) == up) {
                    k[lo] = kb; k[hi] = ka;
                    T t = v[lo]; v[lo] = v[hi]; v[hi] = t;
                }
            }
        }
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
}

// rows with counts[i] == -1 climb the capacity ladder (rare, setup-time: the
// overflow-list compaction runs on host). Returns their number and, when
// non-zero, their device list in *rows_out (caller frees).
int collect_marked_rows(const int* counts, int m, int** rows_out,
                        hipStream_t s) {
    std::vector<int> h_counts(m);
    HIP_CHECK(hipMemcpyAsync(h_counts.data(), counts, m * sizeof(int),
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    std::vector<int> marked;
    for (int i = 0; i < m; ++i)
        if (h_counts[i] == -1) marked.push_back(i);
    int n = (int)marked.size();
    if (n) {
        HIP_CHECK(hipMallocAsync(rows_out, n * sizeof(int), s));
        HIP_CHECK(hipMemcpyAsync(*rows_out, marked.data(), n * sizeof(int),
                                 hipMemcpyHostToDevice, s));
    }
    return n;
}

// exclusive scan of counts[0, m] (counts[m] == 0) -> row offsets ro_out
void exclusive_scan_counts(int* counts, int* ro_out, int m, hipStream_t s) {
    size_t tmp_bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, tmp_bytes, counts, ro_out, 0,
                                  m + 1, rocprim::plus<int>(), s);
    void* tmp = nullptr;
    HIP_CHECK(hipMallocAsync(&tmp, tmp_bytes, s));
    (void)rocprim::exclusive_scan(tmp, tmp_bytes, counts, ro_out, 0, m + 1,
                                  rocprim::plus<int>(), s);
    HIP_CHECK(hipFreeAsync(tmp, s));
}

}  // namespace

// ============================================================ count pass
// mode 0: C = A*B        (walk A row, expand B rows)
// mode 1: Galerkin agg   (walk aggregate members' A rows, key = aggcol[col])
template <int CAP, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void spgemm_count_kernel(
    const int* __restrict__ roA, const int* __restrict__ ciA,
    const int* __restrict__ roB, const int* __restrict__ ciB,
    const int* __restrict__ aggcol, int mode, int m,
    const int* __restrict__ row_list, int n_rows,
    int* __restrict__ counts, int* __restrict__ overflow) {
    __shared__ int keys_s[WAVES][CAP];
    int wave = threadIdx.x / 64;
    int lane = threadIdx.x & 63;
    int slot = blockIdx.x * WAVES + wave;
    if (slot >= n_rows) return;
    int i = row_list ? row_list[slot] : slot;
    int* keys = keys_s[wave];
    for (int t = lane; t < CAP; t += 64) keys[t] = -1;
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    int cnt = 0;
    bool ovf = false;
    for (int k = roA[i]; k < roA[i + 1]; ++k) {
        int c = ciA[k];
        if (mode == 0) {
            for (int t = roB[c] + lane; t < roB[c + 1]; t += 64) {
                int r = hset_insert(keys, CAP, ciB[t]);
                if (r < 0) ovf = true; else cnt += r;
            }
        } else {
            // c is a fine row (aggregate member): expand its A row
            for (int t = roB[c] + lane; t < roB[c + 1]; t += 64) {
                int r = hset_insert(keys, CAP, aggcol[ciB[t]]);
                if (r < 0) ovf = true; else cnt += r;
            }
        }
    }
    // wave-reduce count and overflow
    cnt = (int)wave_reduce_sum(cnt);
    ovf = __any(ovf);
    if (lane == 0) {
        counts[i] = ovf ? -1 : cnt;     // -1 marks the row for a bigger tier
        if (ovf) atomicExch(overflow, 1);
    }
}

// ============================================================ fill pass
// Writes each row's (col, val) entries sorted by column.  SORTED=0 keeps
// the unsorted hash order (the Python caller sorts the rare huge rows).
// hmap_add's return value is not checked: the row guard admits only rows
// whose counted width fits CAP, and under the slots-visited probe budget
// (hset_insert) such a row cannot fail to insert.
template <typename T, int CAP, int WAVES, int SORTED>
__global__ __launch_bounds__(64 * WAVES) void spgemm_fill_kernel(
    const int* __restrict__ roA, const int* __restrict__ ciA,
    const T* __restrict__ vaA, const int* __restrict__ roB,
    const int* __restrict__ ciB, const T* __restrict__ vaB,
    const int* __restrict__ aggcol, int mode, int m,
    const int* __restrict__ row_list, int n_rows,
    const int* __restrict__ roC, int* __restrict__ ciC, T* __restrict__ vaC) {
    static_assert(fill_lds_bytes<T>(CAP, WAVES, SORTED) <= LDS_BYTES,
                  "spgemm_fill_kernel: hash tables exceed the LDS of a CU");
    __shared__ int keys_s[WAVES][CAP];
    __shared__ T vals_s[WAVES][CAP];
    __shared__ int ck_s[WAVES][SORTED ? CAP : 1];
    __shared__ T cv_s[WAVES][SORTED ? CAP : 1];
    __shared__ int cur_s[WAVES];
    int wave = threadIdx.x / 64;
    int lane = threadIdx.x & 63;
    int slot = blockIdx.x * WAVES + wave;
    if (slot >= n_rows) return;
    int i = row_list ? row_list[slot] : slot;
    // rows beyond this kernel's capacity are handled by the big-cap pass
    if ((long long)roC[i + 1] - roC[i] > CAP) return;
    int* keys = keys_s[wave];
    T* vals = vals_s[wave];
    for (int t = lane; t < CAP; t += 64) { keys[t] = -1; vals[t] = T(0); }
    if (lane == 0) cur_s[wave] = 0;
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    for (int k = roA[i]; k < roA[i + 1]; ++k) {
        int c = ciA[k];
        if (mode == 0) {
            T av = vaA[k];
            for (int t = roB[c] + lane; t < roB[c + 1]; t += 64)
                hmap_add(keys, vals, CAP, ciB[t], av * vaB[t]);
        } else {
            for (int t = roB[c] + lane; t < roB[c + 1]; t += 64)
                hmap_add(keys, vals, CAP, aggcol[ciB[t]], vaB[t]);
        }
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    long long base = roC[i];
    int count = (int)((long long)roC[i + 1] - base);
    if (SORTED) {
        int* ck = ck_s[wave];
        T* cv = cv_s[wave];
        // compact live slots (order arbitrary; the sort canonicalizes it)
        for (int t = lane; t < CAP; t += 64) {
            if (keys[t] != -1) {
                int dst = atomicAdd(&cur_s[wave], 1);
                ck[dst] = keys[t];
                cv[dst] = vals[t];
            }
        }
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
        int p = 1;
        while (p < count) p <<= 1;
        for (int t = count + lane; t < p; t += 64) ck[t] = 0x7fffffff;
        wave_bitonic(ck, cv, p, lane);
        for (int t = lane; t < count; t += 64) {
            ciC[base + t] = ck[t];
            vaC[base + t] = cv[t];
        }
    } else {
        for (int t = lane; t < CAP; t += 64) {
            if (keys[t] != -1) {
                int dst = atomicAdd(&cur_s[wave], 1);
                ciC[base + dst] = keys[t];
                vaC[base + dst] = vals[t];
            }
        }
    }
}

// ============================================================ driver
// Returns nnz(C) >= 0 on success, -1 when a row exceeded the top tier (caller
// falls back to the ESC sort path).  counts/roC share the (m+1) buffer.
// cap0 chooses the first tier of the 64 -> 512 -> top capacity ladder
// (64 for AMG-shaped rows; rows past a tier re-run in the next); the top
// tier holds spgemm_hash_top_cap<T>() entries.
template <typename T>
long long spgemm_hash(const int* roA, const int* ciA, const T* vaA, int m,
                      const int* roB, const int* ciB, const T* vaB,
                      const int* aggcol, int mode, int cap0, int* roC_out,
                      int* ciC_cap_buf, T* vaC_cap_buf, long long cap_nnz,
                      int** big_rows_out, int* n_big_out, hipStream_t s) {
    constexpr int BIG_CAP = spgemm_hash_top_cap<T>();
    if (m == 0) {       // no rows: the empty product, no 0-block launches
        HIP_CHECK(hipMemsetAsync(roC_out, 0, sizeof(int), s));
        *big_rows_out = nullptr;
        *n_big_out = 0;
        return 0;
    }
    int* counts = nullptr;
    HIP_CHECK(hipMallocAsync(&counts, (m + 1) * sizeof(int), s));
    int* ovf = nullptr;
    HIP_CHECK(hipMallocAsync(&ovf, sizeof(int), s));
    HIP_CHECK(hipMemsetAsync(ovf, 0, sizeof(int), s));
    HIP_CHECK(hipMemsetAsync(counts, 0, (m + 1) * sizeof(int), s));
    bool tiny_first = cap0 <= TINY_CAP;
    if (tiny_first) {
        int wg = (m + 7) / 8;
        hipLaunchKernelGGL((spgemm_count_kernel<TINY_CAP, 8>), dim3(wg),
                           dim3(64 * 8), 0, s, roA, ciA, roB, ciB, aggcol,
                           mode, m, nullptr, m, counts, ovf);
    } else {
        int wg = (m + 3) / 4;
        hipLaunchKernelGGL((spgemm_count_kernel<SMALL_CAP, 4>), dim3(wg),
                           dim3(64 * 4), 0, s, roA, ciA, roB, ciB, aggcol,
                           mode, m, nullptr, m, counts, ovf);
    }
    int h_ovf = 0;
    HIP_CHECK(hipMemcpyAsync(&h_ovf, ovf, sizeof(int), hipMemcpyDeviceToHost,
                             s));
    HIP_CHECK(hipStreamSynchronize(s));
    auto collect_marked = [&](int** rows_out) -> int {
        return collect_marked_rows(counts, m, rows_out, s);
    };
    int* mid_rows = nullptr;   // rows needing the 512 tier (only if tiny)
    int n_mid = 0;
    int* big_rows = nullptr;   // rows needing the top tier
    int n_big = 0;
    if (h_ovf && tiny_first) {
        n_mid = collect_marked(&mid_rows);
        HIP_CHECK(hipMemsetAsync(ovf, 0, sizeof(int), s));
        hipLaunchKernelGGL((spgemm_count_kernel<SMALL_CAP, 4>),
                           dim3((n_mid + 3) / 4), dim3(64 * 4), 0, s, roA,
                           ciA, roB, ciB, aggcol, mode, m, mid_rows, n_mid,
                           counts, ovf);
        HIP_CHECK(hipMemcpyAsync(&h_ovf, ovf, sizeof(int),
                                 hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    }
    if (h_ovf) {
        n_big = collect_marked(&big_rows);
        HIP_CHECK(hipMemsetAsync(ovf, 0, sizeof(int), s));
        hipLaunchKernelGGL((spgemm_count_kernel<BIG_CAP, 1>), dim3(n_big),
                           dim3(64), 0, s, roA, ciA, roB, ciB, aggcol, mode,
                           m, big_rows, n_big, counts, ovf);
        HIP_CHECK(hipMemcpyAsync(&h_ovf, ovf, sizeof(int),
                                 hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (h_ovf) {     // >BIG_CAP nnz in a row: give up -> ESC fallback
            if (mid_rows) HIP_CHECK(hipFreeAsync(mid_rows, s));
            HIP_CHECK(hipFreeAsync(big_rows, s));
            HIP_CHECK(hipFreeAsync(counts, s));
            HIP_CHECK(hipFreeAsync(ovf, s));
            return -1;
        }
    }
    HIP_CHECK(hipFreeAsync(ovf, s));
    exclusive_scan_counts(counts, roC_out, m, s);
    HIP_CHECK(hipFreeAsync(counts, s));
    int h_nnz = 0;
    HIP_CHECK(hipMemcpyAsync(&h_nnz, roC_out + m, sizeof(int),
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if ((long long)h_nnz > cap_nnz) {
        if (big_rows) HIP_CHECK(hipFreeAsync(big_rows, s));
        return -2;   // caller must re-allocate and retry fill
    }
    // fill tiers mirror the count tiers: each kernel's per-row guard skips
    // rows bigger than its table, and the next tier rewrites them fully
    if (tiny_first) {
        hipLaunchKernelGGL((spgemm_fill_kernel<T, TINY_CAP, 8, 1>),
                           dim3((m + 7) / 8), dim3(64 * 8), 0, s, roA, ciA,
                           vaA, roB, ciB, vaB, aggcol, mode, m, nullptr, m,
                           roC_out, ciC_cap_buf, vaC_cap_buf);
        if (n_mid)
            hipLaunchKernelGGL((spgemm_fill_kernel<T, SMALL_CAP, 4, 1>),
                               dim3((n_mid + 3) / 4), dim3(64 * 4), 0, s,
                               roA, ciA, vaA, roB, ciB, vaB, aggcol, mode,
                               m, mid_rows, n_mid, roC_out, ciC_cap_buf,
                               vaC_cap_buf);
    } else {
        hipLaunchKernelGGL((spgemm_fill_kernel<T, SMALL_CAP, 4, 1>),
                           dim3((m + 3) / 4), dim3(64 * 4), 0, s, roA, ciA,
                           vaA, roB, ciB, vaB, aggcol, mode, m, nullptr, m,
                           roC_out, ciC_cap_buf, vaC_cap_buf);
    }
    if (mid_rows) HIP_CHECK(hipFreeAsync(mid_rows, s));
    if (n_big) {
        hipLaunchKernelGGL((spgemm_fill_kernel<T, BIG_CAP, 1, 0>),
                           dim3(n_big), dim3(64), 0, s, roA, ciA, vaA, roB,
                           ciB, vaB, aggcol, mode, m, big_rows, n_big,
                           roC_out, ciC_cap_buf, vaC_cap_buf);
        *big_rows_out = big_rows;   // caller sorts these rows + frees
        *n_big_out = n_big;
    } else {
        if (big_rows) HIP_CHECK(hipFreeAsync(big_rows, s));
        *big_rows_out = nullptr;
        *n_big_out = 0;
    }
    return (long long)h_nnz;
}

#define INSTANTIATE_SPGEMM_HASH(T) AMGX_INSTANTIATE(spgemm_hash, T)
AMGX_VALUE_TYPES(INSTANTIATE_SPGEMM_HASH)

// ============================================================ ILU(1) pattern
// Color-aware level-1 fill (role of the reference's csr_sparsity_ilu1,
// src/csr_multiply_detail.cu:575-749): the pattern keeps A's own coloring c
// and adds only the fill that color-ordered elimination creates. Row i is
//   A's row i (halo columns >= n included, unchanged)  +  i itself  +
//   every j < n with a local pivot k in A's row i (k < n, c[k] < c[i]) such
//   that (k, j) is in A, c[j] > c[k] and c[j] != c[i].
// Halo columns are never pivots and never expanded. Same scheme as the
// SpGEMM above: wave-per-row hash set, count, scan, fill, tier ladder.
namespace {

// key-only twin of wave_bitonic
__device__ __forceinline__ void wave_bitonic_keys(int* k, int p, int lane) {
    for (int size = 2; size <= p; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __builtin_amdgcn_s_waitcnt(0);
            __builtin_amdgcn_wave_barrier();
            for (int idx = lane; idx < p / 2; idx += 64) {
                int half = idx / stride;
                int lo = half * 2 * stride + (idx % stride);
                int hi = lo + stride;
                bool up = ((lo & size) == 0);
                int ka = k[lo], kb = k[hi];
                if ((ka > kb) == up) { k[lo] = kb; k[hi] = ka; }
            }
        }
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
}

// one wave inserts the pattern of row i into its (cleared) hash set; cnt is
// this lane's number of new keys, ovf is set when the table filled up
template <int CAP>
__device__ __forceinline__ void ilu1_walk_row(
    const int* __restrict__ ro, const int* __restrict__ ci,
    const int* __restrict__ colors, int n, int i, int* keys, int lane,
    int& cnt, bool& ovf) {
    int s = ro[i], e = ro[i + 1];
    int col_i = colors[i];
    for (int k = s + lane; k < e; k += 64) {
        int r = hset_insert(keys, CAP, ci[k]);
        if (r < 0) ovf = true; else cnt += r;
    }
    if (lane == 0) {
        int r = hset_insert(keys, CAP, i);
        if (r < 0) ovf = true; else cnt += r;
    }
    for (int k = s; k < e; ++k) {
        int p = ci[k];                    // wave-uniform
        if (p >= n) continue;             // halo column: not a pivot
        int col_p = colors[p];
        if (col_p >= col_i) continue;
        for (int t = ro[p] + lane; t < ro[p + 1]; t += 64) {
            int j = ci[t];
            if (j >= n) continue;         // halo column: not expanded
            int col_j = colors[j];
            if (col_j > col_p && col_j != col_i) {
                int r = hset_insert(keys, CAP, j);
                if (r < 0) ovf = true; else cnt += r;
            }
        }
    }
}

}  // namespace

template <int CAP, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void ilu1_count_kernel(
    const int* __restrict__ ro, const int* __restrict__ ci,
    const int* __restrict__ colors, int n, const int* __restrict__ row_list,
    int n_rows, int* __restrict__ counts, int* __restrict__ overflow) {
    __shared__ int keys_s[WAVES][CAP];
    int wave = threadIdx.x / 64;
    int lane = threadIdx.x & 63;
    int slot = blockIdx.x * WAVES + wave;
    if (slot >= n_rows) return;
    int i = row_list ? row_list[slot] : slot;
    int* keys = keys_s[wave];
    for (int t = lane; t < CAP; t += 64) keys[t] = -1;
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    int cnt = 0;
    bool ovf = false;
    ilu1_walk_row<CAP>(ro, ci, colors, n, i, keys, lane, cnt, ovf);
    cnt = (int)wave_reduce_sum(cnt);
    ovf = __any(ovf);
    if (lane == 0) {
        counts[i] = ovf ? -1 : cnt;     // -1 marks the row for a bigger tier
        if (ovf) atomicExch(overflow, 1);
    }
}

// Writes each row's columns ascending (the factor kernels binary-search
// them).  SORTED=0 keeps the hash order; the caller sorts those rows.
// ovf is not looked at here: count <= CAP, so every insert finds its slot
// (the probe budget of hset_insert).
template <int CAP, int WAVES, int SORTED>
__global__ __launch_bounds__(64 * WAVES) void ilu1_fill_kernel(
    const int* __restrict__ ro, const int* __restrict__ ci,
    const int* __restrict__ colors, int n, const int* __restrict__ row_list,
    int n_rows, const int* __restrict__ roC, int* __restrict__ ciC) {
    __shared__ int keys_s[WAVES][CAP];
    __shared__ int ck_s[WAVES][SORTED ? CAP : 1];
    __shared__ int cur_s[WAVES];
    int wave = threadIdx.x / 64;
    int lane = threadIdx.x & 63;
    int slot = blockIdx.x * WAVES + wave;
    if (slot >= n_rows) return;
    int i = row_list ? row_list[slot] : slot;
    long long base = roC[i];
    int count = (int)((long long)roC[i + 1] - base);
    // rows beyond this kernel's capacity are handled by the next tier
    if (count > CAP) return;
    int* keys = keys_s[wave];
    for (int t = lane; t < CAP; t += 64) keys[t] = -1;
    if (lane == 0) cur_s[wave] = 0;
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    int cnt = 0;
    bool ovf = false;
    ilu1_walk_row<CAP>(ro, ci, colors, n, i, keys, lane, cnt, ovf);
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    if (SORTED) {
        int* ck = ck_s[wave];
        for (int t = lane; t < CAP; t += 64) {
            if (keys[t] != -1) {
                int dst = atomicAdd(&cur_s[wave], 1);
                ck[dst] = keys[t];
            }
        }
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
        int p = 1;
        while (p < count) p <<= 1;
        for (int t = count + lane; t < p; t += 64) ck[t] = 0x7fffffff;
        wave_bitonic_keys(ck, p, lane);
        for (int t = lane; t < count; t += 64) ciC[base + t] = ck[t];
    } else {
        for (int t = lane; t < CAP; t += 64) {
            if (keys[t] != -1) {
                int dst = atomicAdd(&cur_s[wave], 1);
                ciC[base + dst] = keys[t];
            }
        }
    }
}

long long ilu1_pattern_count(const int* ro, const int* ci, const int* colors,
                             int n, int* roC_out, Ilu1Tiers* tiers,
                             hipStream_t s) {
    *tiers = Ilu1Tiers{};
    int* counts = nullptr;
    HIP_CHECK(hipMallocAsync(&counts, (n + 1) * sizeof(int), s));
    int* ovf = nullptr;
    HIP_CHECK(hipMallocAsync(&ovf, sizeof(int), s));
    HIP_CHECK(hipMemsetAsync(ovf, 0, sizeof(int), s));
    HIP_CHECK(hipMemsetAsync(counts, 0, (n + 1) * sizeof(int), s));
    auto overflowed = [&]() -> bool {
        int h_ovf = 0;
        HIP_CHECK(hipMemcpyAsync(&h_ovf, ovf, sizeof(int),
                                 hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        HIP_CHECK(hipMemsetAsync(ovf, 0, sizeof(int), s));
        return h_ovf != 0;
    };
    if (n > 0)
        hipLaunchKernelGGL((ilu1_count_kernel<TINY_CAP, 8>),
                           dim3((n + 7) / 8), dim3(64 * 8), 0, s, ro, ci,
                           colors, n, nullptr, n, counts, ovf);
    bool too_wide = false;
    if (overflowed()) {
        tiers->n_mid = collect_marked_rows(counts, n, &tiers->mid_rows, s);
        hipLaunchKernelGGL((ilu1_count_kernel<SMALL_CAP, 4>),
                           dim3((tiers->n_mid + 3) / 4), dim3(64 * 4), 0, s,
                           ro, ci, colors, n, tiers->mid_rows, tiers->n_mid,
                           counts, ovf);
        if (overflowed()) {
            tiers->n_big = collect_marked_rows(counts, n, &tiers->big_rows,
                                               s);
            hipLaunchKernelGGL((ilu1_count_kernel<ILU1_TOP_CAP, 1>),
                               dim3(tiers->n_big), dim3(64), 0, s, ro, ci,
                               colors, n, tiers->big_rows, tiers->n_big,
                               counts, ovf);
            too_wide = overflowed();
        }
    }
    HIP_CHECK(hipFreeAsync(ovf, s));
    if (too_wide) {      // a row wider than the top tier: host builder
        HIP_CHECK(hipFreeAsync(counts, s));
        ilu1_tiers_free(tiers, s);
        return -1;
    }
    exclusive_scan_counts(counts, roC_out, n, s);
    HIP_CHECK(hipFreeAsync(counts, s));
    int h_nnz = 0;
    HIP_CHECK(hipMemcpyAsync(&h_nnz, roC_out + n, sizeof(int),
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return (long long)h_nnz;
}

void ilu1_pattern_fill(const int* ro, const int* ci, const int* colors, int n,
                       const int* roC, int* ciC, const Ilu1Tiers& tiers,
                       hipStream_t s) {
    // as in spgemm_hash, each kernel's per-row guard skips rows bigger than
    // its table and the next tier writes them
    if (n > 0)
        hipLaunchKernelGGL((ilu1_fill_kernel<TINY_CAP, 8, 1>),
                           dim3((n + 7) / 8), dim3(64 * 8), 0, s, ro, ci,
                           colors, n, nullptr, n, roC, ciC);
    if (tiers.n_mid)
        hipLaunchKernelGGL((ilu1_fill_kernel<SMALL_CAP, 4, 1>),
                           dim3((tiers.n_mid + 3) / 4), dim3(64 * 4), 0, s,
                           ro, ci, colors, n, tiers.mid_rows, tiers.n_mid,
                           roC, ciC);
    if (tiers.n_big)
        hipLaunchKernelGGL((ilu1_fill_kernel<ILU1_TOP_CAP, 1, 0>),
                           dim3(tiers.n_big), dim3(64), 0, s, ro, ci, colors,
                           n, tiers.big_rows, tiers.n_big, roC, ciC);
}

void ilu1_tiers_free(Ilu1Tiers* tiers, hipStream_t s) {
    if (tiers->mid_rows) HIP_CHECK(hipFreeAsync(tiers->mid_rows, s));
    if (tiers->big_rows) HIP_CHECK(hipFreeAsync(tiers->big_rows, s));
    *tiers = Ilu1Tiers{};
}

// One thread per value element of A: entry k = t / bb finds its row by
// bisection of the row offsets and its column in the sorted LU row, copies
// its element and (element 0) records the slot in a_to_lu.
template <typename T>
__global__ __launch_bounds__(AMGX_BLOCK) void ilu1_embed_kernel(
    const int* __restrict__ roA, const int* __restrict__ ciA,
    const T* __restrict__ vaA, int n, long long total, int bb,
    const int* __restrict__ roL, const int* __restrict__ ciL,
    T* __restrict__ vaL, int* __restrict__ a_to_lu) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         t < total; t += stride) {
        int k = (int)(t / bb);
        int q = (int)(t - (long long)k * bb);
        int lo = 0, hi = n;          // roA[lo] <= k < roA[hi]
        while (hi - lo > 1) {
            int mid = (lo + hi) >> 1;
            if (roA[mid] <= k) lo = mid; else hi = mid;
        }
        int col = ciA[k];
        int slot = -1;
        int a = roL[lo], b = roL[lo + 1];
        while (a < b) {
            int mid = (a + b) >> 1;
            int c = ciL[mid];
            if (c == col) { slot = mid; break; }
            if (c < col) a = mid + 1; else b = mid;
        }
        if (slot >= 0) vaL[(long long)slot * bb + q] = vaA[t];
        if (q == 0) a_to_lu[k] = slot;
    }
}

template <typename T>
void ilu1_embed(const int* roA, const int* ciA, const T* vaA, int n,
                long long nnzA, int bb, const int* roL, const int* ciL,
                T* vaL, int* a_to_lu, hipStream_t s) {
    long long total = nnzA * bb;
    if (total == 0) return;
    hipLaunchKernelGGL((ilu1_embed_kernel<T>),
                       dim3(grid_1d(total, AMGX_BLOCK, 2048)),
                       dim3(AMGX_BLOCK), 0, s, roA, ciA, vaA, n, total, bb,
                       roL, ciL, vaL, a_to_lu);
}

#define INSTANTIATE_ILU1_EMBED(T) AMGX_INSTANTIATE(ilu1_embed, T)
AMGX_REAL_TYPES(INSTANTIATE_ILU1_EMBED)

void free_device_buf(void* p, hipStream_t s) {
    HIP_CHECK(hipFreeAsync(p, s));
}

}  // namespace amgx_hip
