// Python bindings of the gfx950 kernel library (amgx_amd._core).
//
// Besides 1:1 kernel wrappers this TU hosts the C++-side orchestration loops
// whose per-step launches would otherwise pay a Python round trip per color /
// per round: the whole DILU apply, the MIN_MAX coloring loop, the SIZE_2
// matching loop and one MULTI_PAIRWISE pass each run as ONE call from Python.

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <pybind11/complex.h>

#include <algorithm>
#include <array>
#include <climits>
#include <complex>
#include <vector>

#include "core_api.h"

namespace {

using torch::Tensor;

hipStream_t cur_stream() {
    return (hipStream_t)at::cuda::getCurrentCUDAStream().stream();
}

inline void check_dev(const Tensor& t) {
    TORCH_CHECK(t.is_cuda(), "amgx_amd._core requires device tensors");
}

// ---- element types ---------------------------------------------------------
using amgx_hip::cplx;
using amgx_hip::is_cplx;
using cscalar = std::complex<double>;   // coefficient as it arrives from Python

template <typename T> struct tensor_elem { using type = T; };
template <typename R> struct tensor_elem<cplx<R>> { using type = c10::complex<R>; };
static_assert(sizeof(cplx<float>) == sizeof(c10::complex<float>) &&
              sizeof(cplx<double>) == sizeof(c10::complex<double>),
              "cplx must overlay the tensor element");

// typed data pointer; data_ptr<> checks the tensor dtype, so a tensor of
// another dtype raises instead of being reinterpreted
template <typename T>
T* dptr(const Tensor& t) {
    return reinterpret_cast<T*>(t.data_ptr<typename tensor_elem<T>::type>());
}
// the int32 index arrays: row offsets, columns, permutations, colors
inline int* iptr(const Tensor& t) { return dptr<int>(t); }

// coefficient in the kernel's scalar type; a real kernel takes no imaginary part
template <typename T>
T coef(cscalar a, const char* name) {
    if constexpr (is_cplx<T>::value) {
        return T((decltype(T::re))a.real(), (decltype(T::re))a.imag());
    } else {
        TORCH_CHECK(a.imag() == 0.0, name,
                    ": complex coefficient on real tensors");
        return (T)a.real();
    }
}

// ---- dispatch --------------------------------------------------------------
// DISPATCH(LIST, NAME, (tensors), body) calls body, a lambda without
// arguments, for the entry of LIST whose element types are the dtypes of the
// tensors. LIST is a type or pair list of core_api.h, the same one the
// launchers in body are instantiated over. With a type list and (t), body
// sees the entry as scalar_t; with a pair list and (va, x), as scalar_a
// (matrix values) and scalar_v (vectors). Any other dtype or pair raises, so
// an entry over a real list rejects complex tensors.
template <typename... Tn>
std::array<c10::ScalarType, sizeof...(Tn)> dtypes(const Tn&... t) {
    return {t.scalar_type()...};
}
template <typename... Ts>
constexpr std::array<c10::ScalarType, sizeof...(Ts)> dtypes_of() {
    return {c10::CppTypeToScalarType<
        typename tensor_elem<Ts>::type>::value...};
}
template <typename TA, typename TV = TA>
struct list_entry { using a = TA; using v = TV; };

#define DISPATCH_CASE(...)                                                   \
    if (_key == dtypes_of<__VA_ARGS__>())                                    \
        return _body(list_entry<__VA_ARGS__>{});
#define DISPATCH(LIST, NAME, TENSORS, ...)                                   \
    [&] {                                                                    \
        const auto _key = dtypes TENSORS;                                    \
        auto _body = [&](auto _e) {                                          \
            using scalar_t [[maybe_unused]] = typename decltype(_e)::a;      \
            using scalar_a [[maybe_unused]] = typename decltype(_e)::a;      \
            using scalar_v [[maybe_unused]] = typename decltype(_e)::v;      \
            (__VA_ARGS__)();                                                 \
        };                                                                   \
        LIST(DISPATCH_CASE)                                                  \
        TORCH_CHECK(false, NAME, ": unsupported dtype ",                     \
                    c10::Join(" x ", _key));                                 \
    }()

// the block kernels are real: a complex matrix is scalar CSR
inline void check_scalar_if_complex(const Tensor& va, int64_t b,
                                    const char* name) {
    TORCH_CHECK(b == 1 || !va.is_complex(), name,
                ": complex block matrices are unsupported");
}

// the block smoother kernels keep a block or a vector of block_dim components
// in private arrays of MAX_BLOCK_DIM (core_api.h); only the block SpMV takes
// any block size
inline void check_block_dim(int64_t b, const char* name) {
    TORCH_CHECK(b >= 1 && b <= amgx_hip::MAX_BLOCK_DIM, name, ": block_dim ",
                b, " is outside the supported range 1..",
                amgx_hip::MAX_BLOCK_DIM);
}

// f(c, s, e) for every non-empty color c = slots [s, e) of rows_sorted, in
// ascending or descending color order
template <typename F>
void for_each_color(const std::vector<int64_t>& bounds, bool ascending, F f) {
    int nc = (int)bounds.size() - 1;
    for (int k = 0; k < nc; ++k) {
        int c = ascending ? k : nc - 1 - k;
        int64_t s = bounds[c], e = bounds[c + 1];
        if (e > s) f(c, s, e);
    }
}

// ---------------------------------------------------------------- SpMV
template <typename TA, typename TV>
void csrmv_t(const Tensor& ro, const Tensor& ci, const Tensor& va,
             int64_t block_dim, const Tensor& x, const Tensor& y,
             const c10::optional<Tensor>& bvec, cscalar alpha, cscalar beta,
             cscalar gamma, int64_t r0, int64_t r1, double avg) {
    const TV* bp = bvec.has_value() ? dptr<TV>(*bvec) : nullptr;
    TV a = coef<TV>(alpha, "csrmv"), b = coef<TV>(beta, "csrmv"),
       g = coef<TV>(gamma, "csrmv");
    if (block_dim == 1) {
        amgx_hip::csrmv<TA, TV>(iptr(ro), iptr(ci), dptr<TA>(va), dptr<TV>(x),
                                dptr<TV>(y), bp, a, b, g, (int)r0, (int)r1,
                                avg, cur_stream());
    } else if constexpr (is_cplx<TV>::value) {
        TORCH_CHECK(false, "csrmv: complex block matrices are unsupported");
    } else {
        amgx_hip::bsrmv<TA, TV>(iptr(ro), iptr(ci), dptr<TA>(va),
                                (int)block_dim, dptr<TV>(x), dptr<TV>(y), bp,
                                a, b, g, (int)r0, (int)r1, cur_stream());
    }
}

void csrmv(Tensor ro, Tensor ci, Tensor va, int64_t block_dim, Tensor x,
           Tensor y, c10::optional<Tensor> bvec, cscalar alpha, cscalar beta,
           cscalar gamma, int64_t r0, int64_t r1) {
    check_dev(va);
    double avg = ci.numel() / std::max<double>(1.0, ro.numel() - 1);
    DISPATCH(AMGX_VALUE_PAIRS, "csrmv", (va, x), [&] {
        csrmv_t<scalar_a, scalar_v>(ro, ci, va, block_dim, x, y, bvec, alpha,
                                    beta, gamma, r0, r1, avg);
    });
}

// baseline thread-per-row-component block SpMV (A/B target for the MFMA
// b=4 kernel in bench_kernels.py)
void bsrmv_generic(Tensor ro, Tensor ci, Tensor va, int64_t block_dim,
                   Tensor x, Tensor y, double alpha, double beta) {
    check_dev(va);
    int r1 = (int)ro.numel() - 1;
    DISPATCH(AMGX_REAL_PAIRS, "bsrmv_generic", (va, x), [&] {
        amgx_hip::bsrmv_generic<scalar_a, scalar_v>(
            iptr(ro), iptr(ci), dptr<scalar_a>(va), (int)block_dim,
            dptr<scalar_v>(x), dptr<scalar_v>(y), nullptr, (scalar_v)alpha,
            (scalar_v)beta, (scalar_v)0, 0, r1, cur_stream());
    });
}

// ---------------------------------------------------------------- BLAS
// op 0 = sum conj(x) y (y defaults to x) in x's dtype; op 1 / 2 / 3 = sum|x|,
// max|x|, sum|x|^2 in the matching real dtype. Op 3 is complex-only: real
// vectors take their squared norm from op 0. The launcher rejects other ops.
Tensor reduce_op(Tensor x, c10::optional<Tensor> y, int64_t op) {
    check_dev(x);
    TORCH_CHECK(!y.has_value() || y->numel() == x.numel(),
                "reduce: x and y differ in length");
    auto popt = op == 0 ? x.options()
                        : x.options().dtype(
                              c10::toRealValueType(x.scalar_type()));
    auto out = torch::empty({1}, popt);
    auto ws = torch::empty({2048}, popt);
    DISPATCH(AMGX_VALUE_TYPES, "reduce", (x), [&] {
        using real_t = typename amgx_hip::real_of<scalar_t>::type;
        auto partial = [&](const Tensor& t) -> void* {
            if (op == 0) return dptr<scalar_t>(t);
            return dptr<real_t>(t);
        };
        amgx_hip::reduce<scalar_t>(
            dptr<scalar_t>(x), dptr<scalar_t>(y.has_value() ? *y : x),
            x.numel(), (int)op, partial(ws), partial(out), cur_stream());
    });
    return out;
}

void axpy(Tensor y, Tensor x, cscalar a) {
    DISPATCH(AMGX_VALUE_TYPES, "axpy", (x), [&] {
        amgx_hip::axpy<scalar_t>(dptr<scalar_t>(y), dptr<scalar_t>(x),
                                 coef<scalar_t>(a, "axpy"), x.numel(),
                                 cur_stream());
    });
}

// LDS-hash SpGEMM / Galerkin (kernels_spgemm.hip).  Returns
// (roC, ciC, vaC, big_rows): big_rows lists rows written unsorted (the
// Python caller sorts those).  Empty ciC + roC[-1]==-1 signals "fall back
// to the ESC path" (a row exceeded the top hash capacity of its value type,
// SPGEMM_HASH_TOP_CAP).
std::vector<Tensor> spgemm_hash(Tensor roA, Tensor ciA, Tensor vaA,
                                Tensor roB, Tensor ciB, Tensor vaB,
                                c10::optional<Tensor> aggcol, int64_t mode,
                                int64_t cap_nnz, int64_t cap0) {
    int m = (int)roA.numel() - 1;
    auto roC = torch::empty({m + 1}, roA.options());
    auto ciC = torch::empty({cap_nnz}, roA.options());
    auto vaC = torch::empty({cap_nnz}, vaA.options());
    auto big = torch::empty({0}, roA.options());
    hipStream_t st = cur_stream();
    long long nnz = -1;
    DISPATCH(AMGX_VALUE_TYPES, "spgemm_hash", (vaA), [&] {
        int* big_rows = nullptr;
        int n_big = 0;
        nnz = amgx_hip::spgemm_hash<scalar_t>(
            iptr(roA), iptr(ciA), dptr<scalar_t>(vaA), m, iptr(roB), iptr(ciB),
            dptr<scalar_t>(vaB), aggcol ? iptr(*aggcol) : nullptr, (int)mode,
            (int)cap0, iptr(roC), iptr(ciC), dptr<scalar_t>(vaC),
            (long long)cap_nnz, &big_rows, &n_big, st);
        if (n_big > 0) {
            big = torch::empty({n_big}, roA.options());
            TORCH_CHECK(hipMemcpyAsync(iptr(big), big_rows,
                                       n_big * sizeof(int),
                                       hipMemcpyDeviceToDevice,
                                       st) == hipSuccess,
                        "spgemm_hash: big_rows copy failed");
        }
        if (big_rows) amgx_hip::free_device_buf(big_rows, st);
    });
    TORCH_CHECK(nnz != -2, "spgemm_hash: cap_nnz too small (internal)");
    if (nnz < 0) {        // ESC fallback signal
        roC.fill_(-1);
        return {roC, torch::empty({0}, roA.options()),
                torch::empty({0}, vaA.options()), big};
    }
    return {roC, ciC.narrow(0, 0, nnz), vaC.narrow(0, 0, nnz), big};
}

// Color-aware ILU(1) fill pattern of (ro, ci) under the row coloring `colors`
// (kernels_spgemm.hip).  Returns (roL, ciL, big_rows): big_rows lists rows
// written unsorted (the Python caller sorts those).  Empty ciL + roL[-1]==-1
// signals "a row exceeded ILU1_TOP_CAP, build the pattern on the host".
std::vector<Tensor> ilu1_pattern(Tensor ro, Tensor ci, Tensor colors,
                                 int64_t n) {
    check_dev(ro);
    TORCH_CHECK(ro.numel() == n + 1 && colors.numel() == n,
                "ilu1_pattern: ro / colors do not have n rows");
    auto roL = torch::empty({n + 1}, ro.options());
    auto big = torch::empty({0}, ro.options());
    hipStream_t st = cur_stream();
    amgx_hip::Ilu1Tiers tiers;
    long long nnz = amgx_hip::ilu1_pattern_count(
        iptr(ro), iptr(ci), iptr(colors), (int)n, iptr(roL), &tiers, st);
    if (nnz < 0) {
        roL.fill_(-1);
        return {roL, torch::empty({0}, ro.options()), big};
    }
    auto ciL = torch::empty({(int64_t)nnz}, ro.options());
    amgx_hip::ilu1_pattern_fill(iptr(ro), iptr(ci), iptr(colors), (int)n,
                                iptr(roL), iptr(ciL), tiers, st);
    if (tiers.n_big > 0) {
        big = torch::empty({tiers.n_big}, ro.options());
        TORCH_CHECK(hipMemcpyAsync(iptr(big), tiers.big_rows,
                                   tiers.n_big * sizeof(int),
                                   hipMemcpyDeviceToDevice, st) == hipSuccess,
                    "ilu1_pattern: big_rows copy failed");
    }
    amgx_hip::ilu1_tiers_free(&tiers, st);
    return {roL, ciL, big};
}

// A's values at their slots of the sorted pattern (roL, ciL), zeros in the
// fill slots: returns (values (nnzL * bb), a_to_lu (nnzA) int32)
std::vector<Tensor> ilu1_embed(Tensor roA, Tensor ciA, Tensor vaA, int64_t bb,
                               Tensor roL, Tensor ciL) {
    check_dev(vaA);
    int n = (int)roA.numel() - 1;
    int64_t nnzA = ciA.numel();
    TORCH_CHECK(vaA.numel() == nnzA * bb && roL.numel() == roA.numel(),
                "ilu1_embed: shapes of A and the pattern disagree");
    auto vaL = torch::zeros({ciL.numel() * bb}, vaA.options());
    auto a_to_lu = torch::empty({nnzA}, roA.options());
    DISPATCH(AMGX_REAL_TYPES, "ilu1_embed", (vaA), [&] {
        amgx_hip::ilu1_embed<scalar_t>(
            iptr(roA), iptr(ciA), dptr<scalar_t>(vaA), n, (long long)nnzA,
            (int)bb, iptr(roL), iptr(ciL), dptr<scalar_t>(vaL),
            iptr(a_to_lu), cur_stream());
    });
    return {vaL, a_to_lu};
}

Tensor mfma4_probe(Tensor a_frag, Tensor b_frag) {
    auto c = torch::empty_like(a_frag);
    amgx_hip::mfma4_probe(dptr<double>(a_frag), dptr<double>(b_frag),
                          dptr<double>(c), cur_stream());
    return c;
}

void axpy_dalpha(Tensor y, Tensor x, Tensor alpha, double scale) {
    DISPATCH(AMGX_REAL_TYPES, "axpy_dalpha", (x), [&] {
        amgx_hip::axpy_dalpha<scalar_t>(dptr<scalar_t>(y), dptr<scalar_t>(x),
                                        dptr<scalar_t>(alpha), (scalar_t)scale,
                                        x.numel(), cur_stream());
    });
}

void scal_drsqrt(Tensor x, Tensor s2) {
    DISPATCH(AMGX_REAL_TYPES, "scal_drsqrt", (x), [&] {
        amgx_hip::scal_drsqrt<scalar_t>(dptr<scalar_t>(x), dptr<scalar_t>(s2),
                                        x.numel(), cur_stream());
    });
}

void axpby(Tensor y, Tensor x, cscalar a, cscalar b) {
    DISPATCH(AMGX_VALUE_TYPES, "axpby", (x), [&] {
        amgx_hip::axpby<scalar_t>(
            dptr<scalar_t>(y), dptr<scalar_t>(x), coef<scalar_t>(a, "axpby"),
            coef<scalar_t>(b, "axpby"), x.numel(), cur_stream());
    });
}

void scal(Tensor x, cscalar a) {
    DISPATCH(AMGX_VALUE_TYPES, "scal", (x), [&] {
        amgx_hip::scal<scalar_t>(dptr<scalar_t>(x), coef<scalar_t>(a, "scal"),
                                 x.numel(), cur_stream());
    });
}

// ---------------------------------------------------------------- structure
Tensor diag_index(Tensor ro, Tensor ci, int64_t n) {
    auto out = torch::empty({n}, ro.options());
    amgx_hip::diag_index(iptr(ro), iptr(ci), (int)n, iptr(out), cur_stream());
    return out;
}

Tensor extract_diag(Tensor ro, Tensor ci, Tensor va, Tensor didx, int64_t n,
                    int64_t b) {
    auto out = b == 1 ? torch::empty({n}, va.options())
                      : torch::empty({n, b, b}, va.options());
    DISPATCH(AMGX_VALUE_TYPES, "extract_diag", (va), [&] {
        amgx_hip::extract_diag<scalar_t>(dptr<scalar_t>(va), iptr(didx),
                                         (int)n, (int)b, dptr<scalar_t>(out),
                                         cur_stream());
    });
    return out;
}

Tensor trans_index(Tensor ro, Tensor ci, int64_t n) {
    auto out = torch::empty({ci.numel()}, ro.options());
    amgx_hip::trans_index(iptr(ro), iptr(ci), (int)n, iptr(out), cur_stream());
    return out;
}

// ---------------------------------------------------------------- smoothers
Tensor jacobi_dinv(Tensor ro, Tensor ci, Tensor va, Tensor didx, int64_t n,
                   int64_t b, bool l1) {
    check_block_dim(b, "jacobi_dinv");
    auto out = b == 1 ? torch::empty({n}, va.options())
                      : torch::empty({n, b, b}, va.options());
    TORCH_CHECK(!va.is_complex() || (b == 1 && !l1),
                "jacobi_dinv: complex matrices support neither blocks nor "
                "the l1 variant");
    DISPATCH(AMGX_VALUE_TYPES, "jacobi_dinv", (va), [&] {
        amgx_hip::jacobi_dinv<scalar_t>(iptr(ro), dptr<scalar_t>(va),
                                        iptr(didx), (int)n, (int)b, l1,
                                        dptr<scalar_t>(out), cur_stream());
    });
    return out;
}

void jacobi_smooth(Tensor ro, Tensor ci, Tensor va, int64_t b, Tensor dinv,
                   Tensor bvec, Tensor xi, Tensor xo, double omega) {
    int n = (int)(ro.numel() - 1);
    TORCH_CHECK(b == 1 || !va.is_complex(),
                "jacobi_smooth: complex block matrices are unsupported");
    DISPATCH(AMGX_VALUE_PAIRS, "jacobi_smooth", (va, xi), [&] {
        amgx_hip::jacobi_smooth<scalar_a, scalar_v>(
            iptr(ro), iptr(ci), dptr<scalar_a>(va), dptr<scalar_a>(dinv),
            dptr<scalar_v>(bvec), dptr<scalar_v>(xi), dptr<scalar_v>(xo),
            scalar_v(omega), n, (int)b, cur_stream());
    });
}

void gs_smooth_rows(Tensor ro, Tensor ci, Tensor va, int64_t b, Tensor dinv,
                    Tensor bvec, Tensor x, Tensor rows, double omega) {
    check_block_dim(b, "gs_smooth_rows");
    int n = (int)(ro.numel() - 1);
    check_scalar_if_complex(va, b, "gs_smooth_rows");
    DISPATCH(AMGX_VALUE_PAIRS, "gs_smooth_rows", (va, x), [&] {
        amgx_hip::gs_smooth_rows<scalar_a, scalar_v>(
            iptr(ro), iptr(ci), dptr<scalar_a>(va), dptr<scalar_a>(dinv),
            dptr<scalar_v>(bvec), dptr<scalar_v>(x), iptr(rows),
            (int)rows.numel(), (scalar_v)omega, n, (int)b, cur_stream());
    });
}

// multicolor GS full sweep: colors ascending (and descending if symmetric)
void gs_sweep(Tensor ro, Tensor ci, Tensor va, int64_t b, Tensor dinv,
              Tensor bvec, Tensor x, Tensor rows_sorted,
              std::vector<int64_t> bounds, double omega, bool symmetric) {
    check_block_dim(b, "gs_sweep");
    int n = (int)(ro.numel() - 1);
    check_scalar_if_complex(va, b, "gs_sweep");
    DISPATCH(AMGX_VALUE_PAIRS, "gs_sweep", (va, x), [&] {
        auto run = [&](int, int64_t s, int64_t e) {
            amgx_hip::gs_smooth_rows<scalar_a, scalar_v>(
                iptr(ro), iptr(ci), dptr<scalar_a>(va), dptr<scalar_a>(dinv),
                dptr<scalar_v>(bvec), dptr<scalar_v>(x), iptr(rows_sorted) + s,
                (int)(e - s), (scalar_v)omega, n, (int)b, cur_stream());
        };
        for_each_color(bounds, true, run);
        if (symmetric) for_each_color(bounds, false, run);
    });
}

// color-sorted scalar GS sweep (reorder-by-color layout)
void gs_sweep_sorted(Tensor ro_s, Tensor ci_s, Tensor va_s, Tensor dinv_s,
                     Tensor bvec, Tensor x, Tensor rows_sorted,
                     std::vector<int64_t> bounds, Tensor bounds_dev,
                     double omega, bool symmetric) {
    int nc = (int)bounds.size() - 1;
    int64_t n = (int64_t)ro_s.numel() - 1;
    if (n <= amgx_hip::SMALL_LEVEL_ROWS) {
        DISPATCH(AMGX_VALUE_PAIRS, "gs_sweep_small", (va_s, x), [&] {
            amgx_hip::gs_sweep_small<scalar_a, scalar_v>(
                iptr(ro_s), iptr(ci_s), dptr<scalar_a>(va_s),
                dptr<scalar_a>(dinv_s), dptr<scalar_v>(bvec),
                dptr<scalar_v>(x), iptr(rows_sorted), iptr(bounds_dev), nc,
                (scalar_v)omega, symmetric, cur_stream());
        });
        return;
    }
    DISPATCH(AMGX_VALUE_PAIRS, "gs_sweep_sorted", (va_s, x), [&] {
        auto run = [&](int, int64_t s, int64_t e) {
            amgx_hip::gs_rows_sorted<scalar_a, scalar_v>(
                iptr(ro_s) + s, iptr(ci_s), dptr<scalar_a>(va_s),
                dptr<scalar_a>(dinv_s) + s, dptr<scalar_v>(bvec),
                dptr<scalar_v>(x), iptr(rows_sorted) + s, (int)(e - s),
                (scalar_v)omega, cur_stream());
        };
        for_each_color(bounds, true, run);
        if (symmetric) for_each_color(bounds, false, run);
    });
}

// ---------------------------------------------------------------- DILU
Tensor dilu_setup(Tensor ro, Tensor ci, Tensor va, int64_t b, Tensor didx,
                  Tensor tidx, Tensor colors, Tensor rows_sorted,
                  std::vector<int64_t> bounds) {
    check_block_dim(b, "dilu_setup");
    int n = (int)(ro.numel() - 1);
    check_scalar_if_complex(va, b, "dilu_setup");
    auto einv = b == 1 ? torch::zeros({n}, va.options())
                       : torch::zeros({n, b, b}, va.options());
    DISPATCH(AMGX_VALUE_TYPES, "dilu_setup", (va), [&] {
        for_each_color(bounds, true, [&](int c, int64_t s, int64_t e) {
            amgx_hip::dilu_setup_color<scalar_t>(
                iptr(ro), iptr(ci), dptr<scalar_t>(va), iptr(didx), iptr(tidx),
                iptr(colors), iptr(rows_sorted) + s, (int)(e - s), c,
                dptr<scalar_t>(einv), (int)b, cur_stream());
        });
    });
    return einv;
}

// strict color-split of the color-sorted slab (ro_s, ci_s): the U (upper) or
// L part. Returns (ro_x (n+1), ci_x, map_x): offsets in slot order, columns,
// and the full-slab position of every kept entry (the value gather map).
std::vector<Tensor> slab_split(Tensor ro_s, Tensor ci_s, Tensor rows_sorted,
                               Tensor colors, bool upper) {
    check_dev(ro_s);
    int64_t n = (int64_t)ro_s.numel() - 1;
    TORCH_CHECK(rows_sorted.numel() == n && colors.numel() == n,
                "slab_split: rows_sorted / colors do not have n rows");
    hipStream_t st = cur_stream();
    auto ro_x = torch::empty({n + 1}, ro_s.options());
    long long nnz = amgx_hip::slab_split_count(
        iptr(ro_s), iptr(ci_s), iptr(rows_sorted), iptr(colors), (int)n,
        upper, iptr(ro_x), st);
    auto ci_x = torch::empty({(int64_t)nnz}, ro_s.options());
    auto map_x = torch::empty({(int64_t)nnz}, ro_s.options());
    amgx_hip::slab_split_fill(iptr(ro_s), iptr(ci_s), iptr(rows_sorted),
                              iptr(colors), (int)n, upper, iptr(ro_x),
                              iptr(ci_x), iptr(map_x), st);
    return {ro_x, ci_x, map_x};
}

// color-sorted DILU apply x += relax * M^{-1} rhs: matrix arrays in
// rows_sorted order (one contiguous slab per color — reference
// reorder-by-color layout); w, z pre-allocated scratch.
// fused: rhs is b and the residual b - A x is folded into the forward
// sweep (one matrix read fewer per smoother iteration than residual
// kernel + apply); scalar and block-4 only.
// Block matrices. Scalar levels run dilu_small up to DILU_SMALL_ROWS rows
// and dilu_split past it; a scalar call here is the one-launch apply in its
// earlier full-slab form (dilu_small_full), which tests and bench_kernels.py
// compare against, with any_size lifting the row bound for the latter.
void dilu_sorted(Tensor ro_s, Tensor ci_s, Tensor va_s, int64_t b,
                 Tensor einv_s, Tensor rows_sorted,
                 std::vector<int64_t> bounds, Tensor bounds_dev, Tensor rhs,
                 Tensor w, Tensor z, Tensor x, double relax, bool fused,
                 bool any_size) {
    check_block_dim(b, "dilu_sorted");
    TORCH_CHECK(!fused || b == 1 || b == 4,
                "dilu_sorted: no fused-residual kernel for block_dim ", b);
    check_scalar_if_complex(va_s, b, "dilu_sorted");
    int nc = (int)bounds.size() - 1;
    int bb = (int)(b * b);
    int64_t n = (int64_t)ro_s.numel() - 1;
    if (b == 1) {
        TORCH_CHECK(any_size || n <= amgx_hip::DILU_SMALL_ROWS,
                    "dilu_sorted: scalar levels of more than ",
                    amgx_hip::DILU_SMALL_ROWS, " rows run dilu_split");
        TORCH_CHECK(bounds_dev.numel() == nc + 1 && rows_sorted.numel() == n &&
                        w.numel() >= n && z.numel() >= w.numel() &&
                        x.numel() >= n && rhs.numel() >= n &&
                        (!fused || x.numel() >= w.numel()),
                    "dilu_sorted: vectors shorter than the matrix");
        DISPATCH(AMGX_VALUE_PAIRS, "dilu_small_full", (va_s, x), [&] {
            amgx_hip::dilu_small_full<scalar_a, scalar_v>(
                iptr(ro_s), iptr(ci_s), dptr<scalar_a>(va_s),
                dptr<scalar_a>(einv_s), iptr(rows_sorted), iptr(bounds_dev),
                nc, dptr<scalar_v>(rhs), dptr<scalar_v>(w), dptr<scalar_v>(z),
                dptr<scalar_v>(x), (scalar_v)relax, (long long)w.numel(),
                fused, cur_stream());
        });
        return;
    }
    w.zero_();
    z.zero_();
    DISPATCH(AMGX_VALUE_PAIRS, "dilu_sorted", (va_s, x), [&] {
        hipStream_t st = cur_stream();
        const scalar_v* xres = fused ? dptr<scalar_v>(x) : nullptr;
        for_each_color(bounds, true, [&](int, int64_t s, int64_t e) {
            amgx_hip::dilu_fwd_sorted<scalar_a, scalar_v>(
                iptr(ro_s) + s, iptr(ci_s), dptr<scalar_a>(va_s),
                dptr<scalar_a>(einv_s) + s * bb, iptr(rows_sorted) + s,
                (int)(e - s), dptr<scalar_v>(rhs), xres, dptr<scalar_v>(w),
                (int)b, st);
        });
        for_each_color(bounds, false, [&](int, int64_t s, int64_t e) {
            amgx_hip::dilu_bwd_sorted<scalar_a, scalar_v>(
                iptr(ro_s) + s, iptr(ci_s), dptr<scalar_a>(va_s),
                dptr<scalar_a>(einv_s) + s * bb, iptr(rows_sorted) + s,
                (int)(e - s), dptr<scalar_v>(w), dptr<scalar_v>(z), (int)b,
                st);
        });
        amgx_hip::axpy<scalar_v>(dptr<scalar_v>(x), dptr<scalar_v>(z),
                                 (scalar_v)relax, x.numel(), st);
    });
}

// lanes per row of the scalar per-color DILU sweeps, from a slab's average
// entries per row: thread-per-row up to the threshold, 8 lanes above.
// Measured on MI355X (profiles/NOTES.md, "DILU one gathered vector and lane
// forms"): over the split parts L and U one lane wins at 2.98 entries per
// row and 8 lanes from 4.57 upwards. Over the full slab 8 lanes win at every
// figure measured (6.97, 10.14, 12.63); its threshold stays at the 8 of the
// propose kernel, which keeps 7-point matrices on one lane.
constexpr double DILU_LANES_THRESHOLD_FULL = 8.0;
constexpr double DILU_LANES_THRESHOLD_SPLIT = 4.0;
int64_t dilu_lanes(double entries_per_row, bool split) {
    double t = split ? DILU_LANES_THRESHOLD_SPLIT : DILU_LANES_THRESHOLD_FULL;
    return entries_per_row <= t ? 1 : 8;
}

// Stream form of a per-color sweep (amgx_hip::DILU_STREAM) instead of the
// lane form, from the slab's average entries per row and the rows of the
// color. Measured on MI355X (profiles/NOTES.md, "DILU stream form"): on the
// 192^3 matrix and its first two Galerkin levels the stream form is the
// fastest on every slab (full 6.97 / 10.14 / 12.63 entries per row, L and U
// 2.98 / 4.57 / 5.82), 14 to 30 % under the better lane form. Down the
// Galerkin chain of a 64^3 cube it wins at 43.7 k and 13.5 k rows per color,
// ties at 5.7 k and loses 2 to 5 % from 2.5 k down: a small color has too few
// 64-row waves to cover the latency of their windows. The chain is measured
// per level and a level's colors differ widely in size, so the boundary is
// kept on the safe side: colors under 16 k rows keep their lane form,
// whatever the slab.
constexpr int64_t DILU_STREAM_MIN_ROWS_FULL = 1 << 14;
constexpr int64_t DILU_STREAM_MIN_ROWS_SPLIT = 1 << 14;
bool dilu_stream(double entries_per_row, int64_t color_rows, bool split) {
    int64_t least = split ? DILU_STREAM_MIN_ROWS_SPLIT
                          : DILU_STREAM_MIN_ROWS_FULL;
    return entries_per_row > 0.0 && color_rows >= least;
}

// What dilu_split and dilu_small ask of their common arguments (`fn` names
// the caller in the messages), and the lanes of the two slabs: a forced
// `lanes`, or dilu_lanes of the slab's entries per row (the entry counts are
// the tensors' sizes, no read-back; the forward slab of a plain apply and U
// are split parts). y is looked at when fused and present.
struct DiluSlabs {
    double epr_f, epr_u;   // entries per row of the forward / backward slab
    int lanes_f, lanes_u;
};
static DiluSlabs dilu_check_args(const char* fn, const Tensor& ro_f,
                                 const Tensor& ci_f, const Tensor& va_f,
                                 const Tensor& ro_u, const Tensor& ci_u,
                                 const Tensor& va_u, const Tensor& einv_s,
                                 const Tensor& rows_sorted,
                                 const std::vector<int64_t>& bounds,
                                 const Tensor& rhs, const Tensor& w,
                                 const Tensor& x, bool fused, int64_t lanes,
                                 const c10::optional<Tensor>& y_opt) {
    int64_t n = (int64_t)ro_u.numel() - 1;
    TORCH_CHECK(ro_f.numel() == n + 1 && rows_sorted.numel() == n &&
                    einv_s.numel() == n,
                fn, ": slabs, rows_sorted and Einv disagree on n");
    TORCH_CHECK(!bounds.empty() && bounds.front() == 0 && bounds.back() == n,
                fn, ": color bounds do not cover the n rows");
    TORCH_CHECK(va_f.numel() == ci_f.numel() && va_u.numel() == ci_u.numel(),
                fn, ": scalar slabs hold one value per column index");
    TORCH_CHECK(rhs.numel() >= n && x.numel() >= n && w.numel() >= n &&
                    (!fused || w.numel() >= x.numel()),
                fn, ": vectors shorter than the matrix");
    TORCH_CHECK(w.scalar_type() == x.scalar_type() &&
                    rhs.scalar_type() == x.scalar_type() &&
                    va_u.scalar_type() == va_f.scalar_type() &&
                    einv_s.scalar_type() == va_f.scalar_type(),
                fn, ": mixed value types");
    TORCH_CHECK(lanes == 0 || lanes == 1 || lanes == 8,
                fn, ": lanes must be 0 (routed), 1 or 8");
    if (fused && y_opt.has_value()) {
        const Tensor& y = *y_opt;
        TORCH_CHECK(y.is_contiguous() && y.device() == x.device() &&
                        y.scalar_type() == x.scalar_type() &&
                        y.numel() >= x.numel(),
                    fn, ": y must be a vector like w");
    }
    double rows = (double)std::max<int64_t>(n, 1);
    DiluSlabs r;
    r.epr_f = (double)ci_f.numel() / rows;
    r.epr_u = (double)ci_u.numel() / rows;
    r.lanes_f = lanes ? (int)lanes : (int)dilu_lanes(r.epr_f, !fused);
    r.lanes_u = lanes ? (int)lanes : (int)dilu_lanes(r.epr_u, true);
    return r;
}

// per-color scalar DILU apply x += relax * M^{-1} rhs over the strict
// color-split slabs; w is the scratch vector (column-extended).
// fused: rhs is b, the forward sweep reads the full slab (ro_f, ci_f, va_f)
// with the residual b - A x folded in through the second scratch vector
// y = x + w (column-extended like w; taken from the caller so that nothing
// is allocated under graph capture, allocated here when absent). Plain: the
// forward sweep reads the L slab (same three arguments). Neither scratch
// vector needs zeroing. The backward sweep runs in place in w over the U slab
// and updates x as it goes. No host sync: capturable in a hipGraph.
// lanes: 0 routes each slab by its entries per row (dilu_check_args), 1 or 8
// forces that form for both sweeps (tests and bench_kernels.py).
// form: 0 routes each color of each slab between its lane form and the
// stream form (dilu_stream; a forced lanes keeps the lane forms), 1 keeps
// the lane forms, 2 takes the stream form for every color and goes with
// lanes = 0 only. All forms give the same bits.
void dilu_split(Tensor ro_f, Tensor ci_f, Tensor va_f, Tensor ro_u,
                Tensor ci_u, Tensor va_u, Tensor einv_s, Tensor rows_sorted,
                std::vector<int64_t> bounds, Tensor rhs, Tensor w, Tensor x,
                double relax, bool fused, int64_t lanes,
                c10::optional<Tensor> y_opt, int64_t form) {
    TORCH_CHECK(form == 0 || form == 1 || form == 2,
                "dilu_split: form must be 0 (routed), 1 (lane forms) or 2 "
                "(stream form)");
    TORCH_CHECK(form != 2 || lanes == 0,
                "dilu_split: the stream form takes no lanes");
    if (fused && !y_opt.has_value()) y_opt = torch::empty_like(w);
    const DiluSlabs sl =
        dilu_check_args("dilu_split", ro_f, ci_f, va_f, ro_u, ci_u, va_u,
                        einv_s, rows_sorted, bounds, rhs, w, x, fused, lanes,
                        y_opt);
    Tensor y = fused ? *y_opt : Tensor();
    auto pick = [&](int lane_form, double epr, int64_t count, bool split) {
        bool stream = form == 2 || (form == 0 && lanes == 0 &&
                                    dilu_stream(epr, count, split));
        return stream ? amgx_hip::DILU_STREAM : lane_form;
    };
    DISPATCH(AMGX_VALUE_PAIRS, "dilu_split", (va_f, x), [&] {
        hipStream_t st = cur_stream();
        if (fused)
            amgx_hip::dilu_y_init<scalar_v>(dptr<scalar_v>(x),
                                            dptr<scalar_v>(y),
                                            (long long)x.numel(), st);
        for_each_color(bounds, true, [&](int, int64_t s, int64_t e) {
            if (fused)
                amgx_hip::dilu_fwd_full<scalar_a, scalar_v>(
                    iptr(ro_f) + s, iptr(ci_f), dptr<scalar_a>(va_f),
                    dptr<scalar_a>(einv_s) + s, iptr(rows_sorted) + s,
                    (int)(e - s), dptr<scalar_v>(rhs), dptr<scalar_v>(x),
                    dptr<scalar_v>(w), dptr<scalar_v>(y),
                    pick(sl.lanes_f, sl.epr_f, e - s, false), st);
            else
                amgx_hip::dilu_fwd_lower<scalar_a, scalar_v>(
                    iptr(ro_f) + s, iptr(ci_f), dptr<scalar_a>(va_f),
                    dptr<scalar_a>(einv_s) + s, iptr(rows_sorted) + s,
                    (int)(e - s), dptr<scalar_v>(rhs), dptr<scalar_v>(w),
                    pick(sl.lanes_f, sl.epr_f, e - s, true), st);
        });
        for_each_color(bounds, false, [&](int, int64_t s, int64_t e) {
            amgx_hip::dilu_bwd_upper<scalar_a, scalar_v>(
                iptr(ro_u) + s, iptr(ci_u), dptr<scalar_a>(va_u),
                dptr<scalar_a>(einv_s) + s, iptr(rows_sorted) + s,
                (int)(e - s), dptr<scalar_v>(w), dptr<scalar_v>(x),
                (scalar_v)relax, pick(sl.lanes_u, sl.epr_u, e - s, true), st);
        });
    });
}

// one-launch scalar DILU apply for small levels: `sweeps` applies of
// x += relax * M^{-1} rhs back to back in one single-workgroup launch, the
// same arguments and the same bits as `sweeps` calls of dilu_split (bounds
// also as the device copy bounds_dev, which the kernel reads). y is required
// when fused; nothing is allocated, so the call is capturable in a hipGraph.
// Levels of at most DILU_SMALL_ROWS rows; any_size (tests, bench_kernels.py)
// lifts that bound. lanes as in dilu_split.
void dilu_small(Tensor ro_f, Tensor ci_f, Tensor va_f, Tensor ro_u,
                Tensor ci_u, Tensor va_u, Tensor einv_s, Tensor rows_sorted,
                std::vector<int64_t> bounds, Tensor bounds_dev, Tensor rhs,
                Tensor w, Tensor x, double relax, bool fused, int64_t lanes,
                c10::optional<Tensor> y_opt, int64_t sweeps, bool any_size) {
    int64_t n = (int64_t)ro_u.numel() - 1;
    int64_t nc = (int64_t)bounds.size() - 1;
    TORCH_CHECK(any_size || n <= amgx_hip::DILU_SMALL_ROWS,
                "dilu_small: scalar levels of more than ",
                amgx_hip::DILU_SMALL_ROWS, " rows run dilu_split");
    const DiluSlabs sl =
        dilu_check_args("dilu_small", ro_f, ci_f, va_f, ro_u, ci_u, va_u,
                        einv_s, rows_sorted, bounds, rhs, w, x, fused, lanes,
                        y_opt);
    TORCH_CHECK(bounds_dev.numel() == nc + 1 &&
                    bounds_dev.scalar_type() == torch::kInt32,
                "dilu_small: color bounds do not cover the n rows");
    TORCH_CHECK(sweeps >= 1 && sweeps <= (1 << 20),
                "dilu_small: sweeps must be at least 1");
    for (Tensor t : {ro_f, ci_f, va_f, ro_u, ci_u, va_u, einv_s, rows_sorted,
                     bounds_dev, rhs, w, x})
        check_dev(t);
    TORCH_CHECK(!fused || y_opt.has_value(),
                "dilu_small: a fused apply needs y");
    DISPATCH(AMGX_VALUE_PAIRS, "dilu_small", (va_f, x), [&] {
        amgx_hip::dilu_small<scalar_a, scalar_v>(
            iptr(ro_f), iptr(ci_f), dptr<scalar_a>(va_f), iptr(ro_u),
            iptr(ci_u), dptr<scalar_a>(va_u), dptr<scalar_a>(einv_s),
            iptr(rows_sorted), iptr(bounds_dev), (int)nc, dptr<scalar_v>(rhs),
            dptr<scalar_v>(w), fused ? dptr<scalar_v>(*y_opt) : nullptr,
            dptr<scalar_v>(x), (scalar_v)relax, (long long)x.numel(), fused,
            sl.lanes_f, sl.lanes_u, (int)sweeps, cur_stream());
    });
}

// ---------------------------------------------------------------- round loops
// The coloring and matching loops end when a round reports nothing left /
// nothing changed. Each round writes its own int32 slot of an array zeroed
// once per call, and the host reads the slots back once per batch of k
// rounds. That is sound because a round past the end is a no-op: a coloring
// round on a fully colored graph copies the colors, a matching round after
// one that formed no pair sees the same state and forms none. A surplus
// round still streams the level, so k shrinks as the level grows:
// k = 8 up to 2^18 rows, then 4, 2, and 1 from 2^22 rows (profiles/NOTES.md,
// "Setup round loops").
constexpr int64_t ROUND_SLOTS = 512;
int64_t round_batch(int64_t n, int64_t batch) {
    TORCH_CHECK(batch >= 0, "batch must be 0 (by level size) or positive");
    if (batch > 0) return std::min(batch, ROUND_SLOTS);
    if (n >= (int64_t(1) << 22)) return 1;
    if (n >= (int64_t(1) << 20)) return 2;
    if (n >= (int64_t(1) << 18)) return 4;
    return 8;
}

// Runs round(r, slot) for r = 0, 1, ... in batches of k until a round leaves
// its slot at 0 or max_rounds have run; true when a round did. The rounds
// run may exceed the deciding one by up to k - 1.
template <typename Round>
bool run_rounds(int64_t max_rounds, int64_t k, const Tensor& like,
                Round round) {
    auto slots = torch::zeros({ROUND_SLOTS},
                              like.options().dtype(torch::kInt32));
    int64_t rounds = 0, used = 0;
    while (rounds < max_rounds) {
        int64_t kk = std::min(k, max_rounds - rounds);
        if (used + kk > ROUND_SLOTS) {   // the batch before has been read back
            slots.zero_();
            used = 0;
        }
        for (int64_t r = 0; r < kk; ++r, ++rounds)
            round(rounds, iptr(slots) + used + r);
        auto host = slots.narrow(0, used, kk).cpu();
        const int* h = host.data_ptr<int>();
        for (int64_t r = 0; r < kk; ++r)
            if (h[r] == 0) return true;
        used += kk;
    }
    return false;
}

// ---------------------------------------------------------------- coloring
// mode 0: greedy smallest-unused color (MIN_MAX / PARALLEL_GREEDY class);
// mode 1: MULTI_HASH — `mode1_rounds` rounds assigning color = round id
// with per-round re-hash, then greedy cleanup rounds for leftovers.
// batch: rounds per read-back, 0 = by level size (round_batch); the colors
// are the same for every value.
std::tuple<Tensor, int64_t> color_minmax(Tensor ro, Tensor ci, int64_t n,
                                         int64_t max_rounds, int64_t seed,
                                         int64_t mode1_rounds, int64_t batch) {
    check_dev(ro);
    TORCH_CHECK(ro.numel() == n + 1, "color_minmax: ro does not have n rows");
    auto colors = torch::full({n}, -1,
                              ro.options().dtype(torch::kInt32));
    if (n == 0) return {colors, 0};
    auto colors_next = torch::empty_like(colors);
    hipStream_t st = cur_stream();
    bool done = run_rounds(
        max_rounds, round_batch(n, batch), ro, [&](int64_t r, int* left) {
            int mode = r < mode1_rounds ? 1 : 0;
            amgx_hip::color_minmax_round(
                iptr(ro), iptr(ci), (int)n, iptr(colors), iptr(colors_next),
                (int)r, (int)(seed + r * 7919), mode, left, st);
            std::swap(colors, colors_next);
        });
    // a round that left no row uncolored is the convergence check
    TORCH_CHECK(done, "MIN_MAX coloring did not converge in ", max_rounds,
                " rounds");
    auto top = torch::zeros({1}, ro.options().dtype(torch::kInt32));
    amgx_hip::int_max(iptr(colors), (int)n, iptr(top), st);
    int64_t ncolors = top.cpu().item<int>() + 1;
    return {colors, ncolors};
}

// ---------------------------------------------------------------- aggregation
// batch: handshake rounds per read-back, 0 = by level size (round_batch).
// weights: the propose kernel reads edge weights computed once per call
// (one double per entry) instead of computing them from va, tidx and diag in
// every round. The roots are the same for every value of either.
Tensor size2_match(Tensor ro, Tensor ci, Tensor va, Tensor tidx, Tensor diag,
                   int64_t n, int64_t max_iters, int64_t seed,
                   int64_t batch, bool weights) {
    auto agg = torch::full({n}, -1, ro.options().dtype(torch::kInt32));
    if (n == 0) return agg;
    auto prop = torch::empty({n}, ro.options().dtype(torch::kInt32));
    hipStream_t st = cur_stream();
    DISPATCH(AMGX_VALUE_TYPES, "size2_match", (va), [&] {
        Tensor w;
        const double* wpre = nullptr;
        if (weights) {
            w = torch::empty({ci.numel()},
                             ro.options().dtype(torch::kFloat64));
            amgx_hip::agg_edge_weights<scalar_t>(
                iptr(ro), iptr(ci), dptr<scalar_t>(va), iptr(tidx),
                dptr<scalar_t>(diag), (int)n, dptr<double>(w), st);
            wpre = dptr<double>(w);
        }
        run_rounds(max_iters, round_batch(n, batch), ro,
                   [&](int64_t, int* changed) {
            amgx_hip::agg_propose<scalar_t>(
                iptr(ro), iptr(ci), dptr<scalar_t>(va), iptr(tidx),
                dptr<scalar_t>(diag), wpre, (int)n, iptr(agg), iptr(prop),
                (int)seed, st);
            amgx_hip::agg_match(iptr(prop), (int)n, iptr(agg), changed, st);
        });
        auto agg_out = torch::empty_like(agg);
        amgx_hip::agg_merge_singletons<scalar_t>(
            iptr(ro), iptr(ci), dptr<scalar_t>(va), iptr(tidx),
            dptr<scalar_t>(diag), (int)n, iptr(agg), iptr(agg_out), st);
        agg = agg_out;
    });
    return agg;   // root fine-node ids; size2_renumber numbers them
}

// roots of size2_match -> (agg int32[n], num): consecutive ids in ascending
// root order, the values of torch.unique(roots, sorted, return_inverse)
std::tuple<Tensor, int64_t> size2_renumber(Tensor roots) {
    check_dev(roots);
    int64_t n = roots.numel();
    auto agg = torch::empty({n}, roots.options());
    auto ids = torch::empty({n + 1}, roots.options());
    amgx_hip::root_renumber(iptr(roots), (int)n, iptr(ids), iptr(agg),
                            cur_stream());
    int64_t num = ids[n].cpu().item<int>();
    return {agg, num};
}

// Stable order of the rows by an int32 key in [0, nkeys): (order int32[n],
// offsets int32[nkeys + 1]), the values of argsort(stable) and of bincount +
// cumsum. Serves the color order (keys = colors) and the aggregate-membership
// CSR (keys = aggregate ids).
std::tuple<Tensor, Tensor> key_order(Tensor keys, int64_t nkeys) {
    check_dev(keys);
    TORCH_CHECK(nkeys >= 0 && nkeys < INT_MAX && keys.numel() < INT_MAX,
                "key_order: sizes out of the int32 range");
    int64_t n = keys.numel();
    auto order = torch::empty({n}, keys.options());
    auto off = torch::empty({std::max<int64_t>(nkeys, 1) + 1}, keys.options());
    amgx_hip::key_order(iptr(keys), (int)n, (int)nkeys, iptr(order),
                        iptr(off), cur_stream());
    return {order, off.narrow(0, 0, nkeys + 1)};
}

// Slab structure under the row order rows_sorted: (ro_s int32[n + 1],
// ci_s int32[nnz], nzmap int32[nnz], slot_of_row int32[n]). lanes: lanes per
// row of the fill, 0 = by entries per row as the full-slab sweeps.
std::vector<Tensor> slab_structure(Tensor ro, Tensor ci, Tensor rows_sorted,
                                   int64_t lanes) {
    check_dev(ro);
    int64_t n = (int64_t)ro.numel() - 1, nnz = ci.numel();
    TORCH_CHECK(rows_sorted.numel() == n,
                "slab_structure: rows_sorted does not have n rows");
    TORCH_CHECK(lanes == 0 || lanes == 1 || lanes == 8,
                "slab_structure: lanes must be 0 (routed), 1 or 8");
    hipStream_t st = cur_stream();
    auto ro_s = torch::empty({n + 1}, ro.options());
    auto slot = torch::empty({n}, ro.options());
    long long total = amgx_hip::slab_offsets(iptr(ro), iptr(rows_sorted),
                                             (int)n, iptr(ro_s), iptr(slot),
                                             st);
    TORCH_CHECK(total == nnz, "slab_structure: rows_sorted is no permutation "
                "of the rows (", total, " entries of ", nnz, ")");
    auto nzmap = torch::empty({nnz}, ro.options());
    auto ci_s = torch::empty({nnz}, ro.options());
    if (lanes == 0)
        lanes = dilu_lanes((double)nnz / (double)std::max<int64_t>(n, 1),
                           false);
    amgx_hip::slab_fill(iptr(ro), iptr(ci), iptr(rows_sorted), (int)n,
                        (int)lanes, iptr(ro_s), iptr(nzmap), iptr(ci_s), st);
    return {ro_s, ci_s, nzmap, slot};
}

// MULTI_PAIRWISE edge weights, one double per stored entry
Tensor pairwise_weights(Tensor ro, Tensor ci, Tensor va, Tensor tidx,
                        Tensor diag, int64_t n, int64_t formula) {
    check_dev(va);
    TORCH_CHECK(formula == 0 || formula == 1,
                "pairwise_weights: weight_formula must be 0 or 1");
    TORCH_CHECK_NOT_IMPLEMENTED(formula == 0 || !va.is_complex(),
                                "pairwise_weights: weight_formula 1 is "
                                "signed and unavailable for complex values");
    TORCH_CHECK(tidx.numel() == ci.numel() && va.numel() == ci.numel() &&
                    diag.numel() == n && ro.numel() == n + 1,
                "pairwise_weights: array sizes do not match the structure");
    auto w = torch::empty({ci.numel()}, va.options().dtype(torch::kFloat64));
    DISPATCH(AMGX_VALUE_TYPES, "pairwise_weights", (va), [&] {
        amgx_hip::pairwise_weights<scalar_t>(
            iptr(ro), iptr(ci), dptr<scalar_t>(va), iptr(tidx),
            dptr<scalar_t>(diag), (int)n, (int)formula, dptr<double>(w),
            cur_stream());
    });
    return w;
}

// lanes per row of the propose kernel: thread-per-row up to 8 entries per
// row on average, 8 lanes above. Measured on MI355X (profiles/NOTES.md):
// thread-per-row wins at 7.0 entries per row, 8 lanes from 10.2 upwards.
int pairwise_lanes(int64_t nnz, int64_t n) {
    double avg = (double)nnz / (double)std::max<int64_t>(n, 1);
    return avg <= 8.0 ? 1 : 8;
}

// one propose step (tests and bench_kernels.py); lanes = 0 routes by degree
Tensor pairwise_propose(Tensor ro, Tensor ci, Tensor w, int64_t n, Tensor agg,
                        Tensor sizes, int64_t cap, int64_t seed,
                        int64_t lanes) {
    check_dev(w);
    TORCH_CHECK(ro.numel() == n + 1 && w.numel() == ci.numel() &&
                    agg.numel() == n && sizes.numel() == n,
                "pairwise_propose: array sizes do not match the structure");
    auto prop = torch::empty({n}, ro.options().dtype(torch::kInt32));
    int icap = cap <= 0 ? INT_MAX : (int)std::min<int64_t>(cap, INT_MAX);
    if (lanes == 0) lanes = pairwise_lanes(ci.numel(), n);
    amgx_hip::pairwise_propose(iptr(ro), iptr(ci), dptr<double>(w), (int)n,
                               iptr(agg), iptr(sizes), icap, (int)seed,
                               (int)lanes, iptr(prop), cur_stream());
    return prop;
}

// Handshake rounds + leftover phase + renumbering of one MULTI_PAIRWISE pass
// in one call: (agg int32[n], num, sizes int32[num], rounds). One integer
// read-back per round, as size2_match. cap <= 0 = unbounded.
std::tuple<Tensor, int64_t, Tensor, int64_t> pairwise_match(
    Tensor ro, Tensor ci, Tensor w, int64_t n, Tensor sizes_in, int64_t cap,
    int64_t merge_singletons, int64_t max_iters, double max_unassigned,
    int64_t seed, int64_t lanes) {
    check_dev(w);
    TORCH_CHECK(ro.numel() == n + 1 && w.numel() == ci.numel() &&
                    sizes_in.numel() == n,
                "pairwise_match: array sizes do not match the structure");
    TORCH_CHECK(merge_singletons >= 0 && merge_singletons <= 2,
                "pairwise_match: merge_singletons must be 0, 1 or 2");
    auto iopt = ro.options().dtype(torch::kInt32);
    auto agg = torch::full({n}, -1, iopt);
    auto sizes = sizes_in.clone();
    if (n == 0) return {agg, 0, sizes, 0};
    auto prop = torch::empty({n}, iopt);
    auto counter = torch::zeros({1}, iopt);
    hipStream_t st = cur_stream();
    const int* rp = iptr(ro);
    const int* cp = iptr(ci);
    const double* wp = dptr<double>(w);
    int icap = cap <= 0 ? INT_MAX : (int)std::min<int64_t>(cap, INT_MAX);
    if (lanes == 0) lanes = pairwise_lanes(ci.numel(), n);
    auto unaggregated = [&] {
        counter.zero_();
        amgx_hip::pairwise_count_unaggregated(iptr(agg), (int)n,
                                              iptr(counter), st);
        return (int64_t)counter.cpu().item<int>();
    };

    int64_t un = n, rounds = 0;
    while (rounds < max_iters && un > 0 &&
           !((double)un < max_unassigned * (double)n)) {
        amgx_hip::pairwise_propose(rp, cp, wp, (int)n, iptr(agg), iptr(sizes),
                                   icap, (int)seed, (int)lanes, iptr(prop),
                                   st);
        amgx_hip::pairwise_match(iptr(prop), (int)n, iptr(agg), iptr(sizes),
                                 st);
        ++rounds;
        int64_t left = unaggregated();
        if (left == un) break;   // no pair formed
        un = left;
    }

    if (merge_singletons == 1 && un > 0) {
        auto agg_next = torch::empty_like(agg);
        while (un > 0) {
            amgx_hip::pairwise_join_sweep(rp, cp, wp, (int)n, iptr(agg),
                                          (int)seed, iptr(agg_next), st);
            std::swap(agg, agg_next);
            int64_t left = unaggregated();
            if (left == un) break;   // the sweep changed nothing
            un = left;
        }
    } else if (merge_singletons == 2 && un > 0) {
        auto bid_root = torch::empty({n}, iopt);
        auto bid_w = torch::zeros({n}, ro.options().dtype(torch::kInt64));
        auto bid_i = torch::full({n}, n, iopt);
        while (un > 0) {
            amgx_hip::pairwise_join_capped(
                rp, cp, wp, (int)n, iptr(agg), iptr(sizes), icap, (int)seed,
                iptr(bid_root),
                reinterpret_cast<unsigned long long*>(dptr<int64_t>(bid_w)),
                iptr(bid_i), st);
            int64_t left = unaggregated();
            if (left == un) break;   // no proposal was made
            un = left;
        }
    }

    auto ids = torch::empty({n + 1}, iopt);
    size_t tmp_bytes = amgx_hip::pairwise_renumber_tmp_bytes((int)n);
    auto tmp = torch::empty({(int64_t)std::max<size_t>(tmp_bytes, 16)},
                            ro.options().dtype(torch::kUInt8));
    auto agg_out = torch::empty({n}, iopt);
    auto sizes_out = torch::zeros({n}, iopt);
    amgx_hip::pairwise_renumber(iptr(agg), (int)n, iptr(sizes_in), iptr(ids),
                                tmp.data_ptr(), tmp_bytes, iptr(agg_out),
                                iptr(sizes_out), st);
    int64_t num = ids[n].cpu().item<int>();
    return {agg_out, num, sizes_out.narrow(0, 0, num).clone(), rounds};
}

// ---------------------------------------------------------------- transfers
void restrict_agg(Tensor r, Tensor agg, int64_t b, Tensor rc) {
    rc.zero_();
    DISPATCH(AMGX_VALUE_TYPES, "restrict_agg", (r), [&] {
        amgx_hip::restrict_agg<scalar_t>(dptr<scalar_t>(r), iptr(agg),
                                         (int)agg.numel(), (int)b,
                                         dptr<scalar_t>(rc), cur_stream());
    });
}

void restrict_csr(Tensor r, Tensor off, Tensor fids, int64_t b, Tensor rc) {
    DISPATCH(AMGX_VALUE_TYPES, "restrict_csr", (r), [&] {
        amgx_hip::restrict_csr<scalar_t>(
            iptr(off), iptr(fids), dptr<scalar_t>(r), (int)(off.numel() - 1),
            (int)b, dptr<scalar_t>(rc), cur_stream());
    });
}

void prolongate_agg(Tensor x, Tensor xc, Tensor agg, int64_t b) {
    DISPATCH(AMGX_VALUE_TYPES, "prolongate_agg", (x), [&] {
        amgx_hip::prolongate_agg<scalar_t>(
            dptr<scalar_t>(x), dptr<scalar_t>(xc), iptr(agg), (int)agg.numel(),
            (int)b, cur_stream());
    });
}

// ---------------------------------------------------------------- dense
void dense_gemv(Tensor Ainv, Tensor b, Tensor x) {
    DISPATCH(AMGX_VALUE_PAIRS, "dense_gemv", (Ainv, b), [&] {
        amgx_hip::dense_gemv<scalar_a, scalar_v>(
            dptr<scalar_a>(Ainv), dptr<scalar_v>(b), dptr<scalar_v>(x),
            (int)b.numel(), cur_stream());
    });
}

// ---------------------------------------------------------------- pack
void gather(Tensor src, Tensor idx, int64_t b, Tensor dst) {
    DISPATCH(AMGX_VALUE_TYPES, "gather", (src), [&] {
        amgx_hip::gather<scalar_t>(dptr<scalar_t>(src), iptr(idx),
                                   (int)idx.numel(), (int)b,
                                   dptr<scalar_t>(dst), cur_stream());
    });
}

// ---------------------------------------------------------------- SpGEMM
std::tuple<Tensor, Tensor, Tensor> galerkin_agg(Tensor ro, Tensor ci,
                                                Tensor va, Tensor agg,
                                                Tensor agg_col, int64_t nc,
                                                int64_t ncmod,
                                                int64_t block_dim) {
    int n = (int)(ro.numel() - 1);
    long long nnz = ci.numel();
    int bb = (int)(block_dim * block_dim);
    check_scalar_if_complex(va, block_dim, "galerkin_agg");
    auto ro_c = torch::empty({nc + 1}, ro.options());
    auto ci_c = torch::empty({nnz}, ro.options());
    auto va_c = block_dim == 1
                    ? torch::empty({nnz}, va.options())
                    : torch::empty({nnz, block_dim, block_dim}, va.options());
    long long nnz_c = 0;
    DISPATCH(AMGX_VALUE_TYPES, "galerkin_agg", (va), [&] {
        nnz_c = amgx_hip::galerkin_agg<scalar_t>(
            iptr(ro), iptr(ci), dptr<scalar_t>(va), n, nnz, iptr(agg),
            iptr(agg_col), (int)nc, (long long)ncmod, iptr(ro_c), iptr(ci_c),
            dptr<scalar_t>(va_c), bb, cur_stream());
    });
    return {ro_c, ci_c.narrow(0, 0, nnz_c), va_c.narrow(0, 0, nnz_c)};
}

std::tuple<Tensor, Tensor, Tensor> spgemm(Tensor roA, Tensor ciA, Tensor vaA,
                                          Tensor roB, Tensor ciB, Tensor vaB,
                                          int64_t n_cols_B,
                                          int64_t capacity) {
    int m = (int)(roA.numel() - 1);
    int k = (int)(roB.numel() - 1);
    auto ro_c = torch::empty({m + 1}, roA.options());
    auto ci_c = torch::empty({capacity}, roA.options());
    auto va_c = torch::empty({capacity}, vaA.options());
    long long nnz_c = 0;
    DISPATCH(AMGX_VALUE_TYPES, "spgemm", (vaA), [&] {
        nnz_c = amgx_hip::spgemm_esc<scalar_t>(
            iptr(roA), iptr(ciA), dptr<scalar_t>(vaA), m, ciA.numel(),
            iptr(roB), iptr(ciB), dptr<scalar_t>(vaB), k, (int)n_cols_B,
            iptr(ro_c), iptr(ci_c), dptr<scalar_t>(va_c), cur_stream());
    });
    return {ro_c, ci_c.narrow(0, 0, nnz_c), va_c.narrow(0, 0, nnz_c)};
}

std::tuple<Tensor, Tensor, Tensor> transpose(Tensor ro, Tensor ci, Tensor va,
                                             int64_t n_cols) {
    int m = (int)(ro.numel() - 1);
    long long nnz = ci.numel();
    auto ro_t = torch::empty({n_cols + 1}, ro.options());
    auto ci_t = torch::empty({nnz}, ro.options());
    auto va_t = torch::empty({nnz}, va.options());
    DISPATCH(AMGX_REAL_TYPES, "transpose", (va), [&] {
        amgx_hip::transpose_csr<scalar_t>(
            iptr(ro), iptr(ci), dptr<scalar_t>(va), m, (int)n_cols, nnz,
            iptr(ro_t), iptr(ci_t), dptr<scalar_t>(va_t), cur_stream());
    });
    return {ro_t, ci_t, va_t};
}

// ---------------------------------------------------------------- classical
Tensor strength_ahat(Tensor ro, Tensor ci, Tensor va, Tensor didx,
                     double theta, double max_row_sum) {
    int n = (int)(ro.numel() - 1);
    auto strong = torch::empty({ci.numel()}, ro.options().dtype(torch::kUInt8));
    DISPATCH(AMGX_REAL_TYPES, "strength_ahat", (va), [&] {
        amgx_hip::strength_ahat<scalar_t>(
            iptr(ro), iptr(ci), dptr<scalar_t>(va), iptr(didx), n, theta,
            max_row_sum, dptr<unsigned char>(strong), cur_stream());
    });
    return strong;
}

Tensor pmis_select(Tensor ro, Tensor ci, Tensor tidx, Tensor strong,
                   int64_t max_rounds) {
    int n = (int)(ro.numel() - 1);
    auto w = torch::empty({n}, ro.options().dtype(torch::kFloat32));
    auto state = torch::zeros({n}, ro.options().dtype(torch::kChar));
    auto state_mid = torch::zeros_like(state);
    auto state_out = torch::zeros_like(state);
    auto counter = torch::zeros({1}, ro.options().dtype(torch::kInt32));
    hipStream_t st = cur_stream();
    amgx_hip::pmis_lambda(iptr(ro), iptr(ci), iptr(tidx),
                          dptr<unsigned char>(strong), n, dptr<float>(w), st);
    amgx_hip::pmis_mark_isolated(iptr(ro), iptr(ci), iptr(tidx),
                                 dptr<unsigned char>(strong), n,
                                 dptr<signed char>(state), st);
    // Rounds run until no point is left undecided. The counter is taken
    // between the two halves of a round, so it may still count points that
    // the second half turns into F: after max_rounds rounds (the host's
    // guard) the state itself says whether the selection has failed.
    for (int64_t round = 0;; ++round) {
        if (round >= max_rounds) {
            TORCH_CHECK(!state.eq(0).any().item<bool>(),
                        "PMIS failed to converge in ", max_rounds, " rounds");
            break;
        }
        counter.zero_();
        amgx_hip::pmis_one_round(
            iptr(ro), iptr(ci), iptr(tidx), dptr<unsigned char>(strong), n,
            dptr<float>(w), dptr<signed char>(state),
            dptr<signed char>(state_mid), dptr<signed char>(state_out),
            iptr(counter), st);
        std::swap(state, state_out);
        if (counter.cpu().item<int>() == 0) break;
    }
    return state;   // 1 = C, -1 = F; Python builds cf_map via cumsum
}

std::tuple<Tensor, Tensor, Tensor> interp_d1(Tensor ro, Tensor ci, Tensor va,
                                             Tensor strong, Tensor cf,
                                             Tensor didx, Tensor p_ro,
                                             int64_t p_nnz) {
    int n = (int)(ro.numel() - 1);
    auto p_ci = torch::empty({p_nnz}, ro.options());
    auto p_va = torch::empty({p_nnz}, va.options());
    DISPATCH(AMGX_REAL_TYPES, "interp_d1", (va), [&] {
        amgx_hip::interp_d1<scalar_t>(
            iptr(ro), iptr(ci), dptr<scalar_t>(va),
            dptr<unsigned char>(strong), iptr(cf), iptr(didx), iptr(p_ro), n,
            (int)cf.numel(), iptr(p_ci), dptr<scalar_t>(p_va), cur_stream());
    });
    return {p_ro, p_ci, p_va};
}

std::tuple<Tensor, Tensor, Tensor> truncate_rows(Tensor ro, Tensor ci,
                                                 Tensor va, double factor,
                                                 int64_t max_elem) {
    int n = (int)(ro.numel() - 1);
    auto counts = torch::empty({n}, ro.options());
    DISPATCH(AMGX_REAL_TYPES, "truncate_count", (va), [&] {
        amgx_hip::truncate_rows_gpu<scalar_t>(
            iptr(ro), iptr(ci), dptr<scalar_t>(va), n, factor, (int)max_elem,
            nullptr, nullptr, nullptr, iptr(counts), cur_stream());
    });
    auto ro_out = torch::zeros({n + 1}, ro.options());
    ro_out.slice(0, 1, n + 1).copy_(
        torch::cumsum(counts.to(torch::kLong), 0).to(torch::kInt));
    int64_t nnz_out = n > 0 ? ro_out[n].item<int64_t>() : 0;
    auto ci_out = torch::empty({nnz_out}, ro.options());
    auto va_out = torch::empty({nnz_out}, va.options());
    DISPATCH(AMGX_REAL_TYPES, "truncate_fill", (va), [&] {
        amgx_hip::truncate_fill_gpu<scalar_t>(
            iptr(ro), iptr(ci), dptr<scalar_t>(va), n, factor, (int)max_elem,
            iptr(ro_out), iptr(ci_out), dptr<scalar_t>(va_out), cur_stream());
    });
    return {ro_out, ci_out, va_out};
}

Tensor interp_d1_count(Tensor ro, Tensor ci, Tensor strong, Tensor cf) {
    int n = (int)(ro.numel() - 1);
    auto counts = torch::empty({n}, ro.options());
    amgx_hip::interp_d1_count(iptr(ro), iptr(ci), dptr<unsigned char>(strong),
                              iptr(cf), n, (int)cf.numel(), iptr(counts),
                              cur_stream());
    return counts;
}

// ---------------------------------------------------------------- ILU(0)
Tensor ilu0_setup(Tensor ro, Tensor ci, Tensor va, Tensor didx, Tensor pos,
                  Tensor rows_sorted, std::vector<int64_t> bounds) {
    int n = (int)(ro.numel() - 1);
    auto lu = va.clone();
    DISPATCH(AMGX_REAL_TYPES, "ilu0_setup", (va), [&] {
        for_each_color(bounds, true, [&](int, int64_t s, int64_t e) {
            amgx_hip::ilu0_factor_color_launch<scalar_t>(
                iptr(ro), iptr(ci), iptr(pos), iptr(didx),
                iptr(rows_sorted) + s, (int)(e - s), dptr<scalar_t>(lu), n,
                cur_stream());
        });
    });
    return lu;
}

// block ILU(0): returns (lu, dinv) — dinv holds inverted pivot blocks
std::vector<Tensor> ilu0_setup_block(Tensor ro, Tensor ci, Tensor va,
                                     int64_t b, Tensor didx, Tensor pos,
                                     Tensor rows_sorted,
                                     std::vector<int64_t> bounds) {
    check_block_dim(b, "ilu0_setup_block");
    int n = (int)(ro.numel() - 1);
    auto lu = va.clone().reshape({-1});
    auto dinv = torch::zeros({(int64_t)n * b * b}, va.options());
    DISPATCH(AMGX_REAL_TYPES, "ilu0_setup_block", (va), [&] {
        hipStream_t st = cur_stream();
        for_each_color(bounds, true, [&](int, int64_t s, int64_t e) {
            amgx_hip::ilu0_factor_color_block_launch<scalar_t>(
                iptr(ro), iptr(ci), iptr(pos), iptr(didx),
                iptr(rows_sorted) + s, (int)(e - s), dptr<scalar_t>(lu),
                dptr<scalar_t>(dinv), n, (int)b, st);
            amgx_hip::ilu0_invert_diag_block_launch<scalar_t>(
                iptr(didx), iptr(rows_sorted) + s, (int)(e - s),
                dptr<scalar_t>(lu), dptr<scalar_t>(dinv), (int)b, st);
        });
    });
    return {lu, dinv};
}

void ilu0_apply_block(Tensor ro, Tensor ci, Tensor lu, Tensor dinv,
                      int64_t b, Tensor pos, Tensor rows_sorted,
                      std::vector<int64_t> bounds, Tensor r, Tensor y,
                      Tensor z, Tensor x, double relax) {
    check_block_dim(b, "ilu0_apply_block");
    int n = (int)(ro.numel() - 1);
    y.zero_();
    z.zero_();
    DISPATCH(AMGX_REAL_PAIRS, "ilu0_apply_block", (lu, x), [&] {
        hipStream_t st = cur_stream();
        for_each_color(bounds, true, [&](int, int64_t s, int64_t e) {
            amgx_hip::ilu0_fwd_block_launch<scalar_a, scalar_v>(
                iptr(ro), iptr(ci), iptr(pos), dptr<scalar_a>(lu),
                iptr(rows_sorted) + s, (int)(e - s), dptr<scalar_v>(r),
                dptr<scalar_v>(y), n, (int)b, st);
        });
        for_each_color(bounds, false, [&](int, int64_t s, int64_t e) {
            amgx_hip::ilu0_bwd_block_launch<scalar_a, scalar_v>(
                iptr(ro), iptr(ci), iptr(pos), dptr<scalar_a>(lu),
                dptr<scalar_a>(dinv), iptr(rows_sorted) + s, (int)(e - s),
                dptr<scalar_v>(y), dptr<scalar_v>(z), n, (int)b, st);
        });
        amgx_hip::axpy<scalar_v>(dptr<scalar_v>(x), dptr<scalar_v>(z),
                                 (scalar_v)relax, x.numel(), st);
    });
}

// color-sorted ILU(0) apply (reorder-by-color slabs; cf. dilu_sorted)
void ilu0_apply_sorted(Tensor ro_s, Tensor ci_s, Tensor lu_s, Tensor diag_s,
                       Tensor pos, Tensor rows_sorted,
                       std::vector<int64_t> bounds, Tensor r, Tensor y,
                       Tensor z, Tensor x, double relax) {
    int n = (int)(ro_s.numel() - 1);
    y.zero_();
    z.zero_();
    DISPATCH(AMGX_REAL_PAIRS, "ilu0_apply_sorted", (lu_s, x), [&] {
        hipStream_t st = cur_stream();
        for_each_color(bounds, true, [&](int, int64_t s, int64_t e) {
            amgx_hip::ilu0_fwd_sorted<scalar_a, scalar_v>(
                iptr(ro_s) + s, iptr(ci_s), dptr<scalar_a>(lu_s), iptr(pos),
                iptr(rows_sorted) + s, (int)(e - s), dptr<scalar_v>(r),
                dptr<scalar_v>(y), n, st);
        });
        for_each_color(bounds, false, [&](int, int64_t s, int64_t e) {
            amgx_hip::ilu0_bwd_sorted<scalar_a, scalar_v>(
                iptr(ro_s) + s, iptr(ci_s), dptr<scalar_a>(lu_s),
                dptr<scalar_a>(diag_s) + s, iptr(pos), iptr(rows_sorted) + s,
                (int)(e - s), dptr<scalar_v>(y), dptr<scalar_v>(z), n, st);
        });
        amgx_hip::axpy<scalar_v>(dptr<scalar_v>(x), dptr<scalar_v>(z),
                                 (scalar_v)relax, x.numel(), st);
    });
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.attr("SMALL_LEVEL_ROWS") = amgx_hip::SMALL_LEVEL_ROWS;
    // widest row (entries) the LDS-hash SpGEMM / Galerkin takes, by value
    // dtype; spgemm_hash signals the sort fallback for a wider one
    m.attr("SPGEMM_HASH_TOP_CAP") = pybind11::dict(
        pybind11::arg("float64") = amgx_hip::spgemm_hash_top_cap<double>(),
        pybind11::arg("float32") = amgx_hip::spgemm_hash_top_cap<float>(),
        pybind11::arg("complex128") =
            amgx_hip::spgemm_hash_top_cap<cplx<double>>(),
        pybind11::arg("complex64") =
            amgx_hip::spgemm_hash_top_cap<cplx<float>>());
    m.def("csrmv", &csrmv);
    m.def("reduce_op", &reduce_op);
    m.def("axpy", &axpy);
    m.def("axpy_dalpha", &axpy_dalpha);
    m.def("mfma4_probe", &mfma4_probe);
    m.def("spgemm_hash", &spgemm_hash);
    m.attr("ILU1_TOP_CAP") = amgx_hip::ILU1_TOP_CAP;
    m.def("ilu1_pattern", &ilu1_pattern);
    m.def("ilu1_embed", &ilu1_embed);
    m.def("bsrmv_generic", &bsrmv_generic);
    m.def("scal_drsqrt", &scal_drsqrt);
    m.def("axpby", &axpby);
    m.def("scal", &scal);
    m.def("diag_index", &diag_index);
    m.def("extract_diag", &extract_diag);
    m.def("trans_index", &trans_index);
    m.def("jacobi_dinv", &jacobi_dinv);
    m.def("jacobi_smooth", &jacobi_smooth);
    m.def("gs_smooth_rows", &gs_smooth_rows);
    m.def("gs_sweep", &gs_sweep);
    m.def("gs_sweep_sorted", &gs_sweep_sorted);
    m.def("dilu_setup", &dilu_setup);
    // row bound of the one-launch scalar DILU apply (dilu_small)
    m.attr("DILU_SMALL_ROWS") = amgx_hip::DILU_SMALL_ROWS;
    {   // any_size is optional: 14 positional arguments still work
        using pybind11::arg;
        m.def("dilu_sorted", &dilu_sorted, arg("ro_s"), arg("ci_s"),
              arg("va_s"), arg("b"), arg("einv_s"), arg("rows_sorted"),
              arg("bounds"), arg("bounds_dev"), arg("rhs"), arg("w"),
              arg("z"), arg("x"), arg("relax"), arg("fused"),
              arg("any_size") = false);
        m.def("dilu_small", &dilu_small, arg("ro_f"), arg("ci_f"),
              arg("va_f"), arg("ro_u"), arg("ci_u"), arg("va_u"),
              arg("einv_s"), arg("rows_sorted"), arg("bounds"),
              arg("bounds_dev"), arg("rhs"), arg("w"), arg("x"), arg("relax"),
              arg("fused"), arg("lanes") = 0, arg("y") = pybind11::none(),
              arg("sweeps") = 1, arg("any_size") = false);
    }
    {   // trailing lanes / y / form are optional: 14 positional arguments
        // still work
        using pybind11::arg;
        m.def("dilu_split", &dilu_split, arg("ro_f"), arg("ci_f"),
              arg("va_f"), arg("ro_u"), arg("ci_u"), arg("va_u"),
              arg("einv_s"), arg("rows_sorted"), arg("bounds"), arg("rhs"),
              arg("w"), arg("x"), arg("relax"), arg("fused"),
              arg("lanes") = 0, arg("y") = pybind11::none(),
              arg("form") = 0);
    }
    m.def("dilu_lanes", &dilu_lanes, pybind11::arg("entries_per_row"),
          pybind11::arg("split") = false);
    // the stream form of the per-color sweeps: its routing rule and geometry
    m.def("dilu_stream", &dilu_stream, pybind11::arg("entries_per_row"),
          pybind11::arg("color_rows"), pybind11::arg("split") = false);
    m.def("dilu_stream_window", &amgx_hip::dilu_stream_window_of,
          pybind11::arg("pair_bytes") = 16);
    m.attr("DILU_STREAM_ROWS") = amgx_hip::DILU_STREAM_ROWS;
    m.attr("DILU_STREAM_WINDOW") = amgx_hip::DILU_STREAM_WINDOW;
    m.attr("DILU_STREAM_MIN_ROWS_FULL") = DILU_STREAM_MIN_ROWS_FULL;
    m.attr("DILU_STREAM_MIN_ROWS_SPLIT") = DILU_STREAM_MIN_ROWS_SPLIT;
    m.def("slab_split", &slab_split);
    {
        using pybind11::arg;
        m.def("color_minmax", &color_minmax, arg("ro"), arg("ci"), arg("n"),
              arg("max_rounds"), arg("seed"), arg("mode1_rounds"),
              arg("batch") = 0);
        m.def("size2_match", &size2_match, arg("ro"), arg("ci"), arg("va"),
              arg("tidx"), arg("diag"), arg("n"), arg("max_iters"),
              arg("seed"), arg("batch") = 0, arg("weights") = false);
        m.def("slab_structure", &slab_structure, arg("ro"), arg("ci"),
              arg("rows_sorted"), arg("lanes") = 0);
    }
    m.def("size2_renumber", &size2_renumber);
    m.def("key_order", &key_order);
    m.def("pairwise_weights", &pairwise_weights);
    m.def("pairwise_propose", &pairwise_propose);
    m.def("pairwise_match", &pairwise_match);
    m.def("restrict_agg", &restrict_agg);
    m.def("restrict_csr", &restrict_csr);
    m.def("prolongate_agg", &prolongate_agg);
    m.def("dense_gemv", &dense_gemv);
    m.def("gather", &gather);
    m.def("galerkin_agg", &galerkin_agg);
    m.def("spgemm", &spgemm);
    m.def("transpose", &transpose);
    m.def("strength_ahat", &strength_ahat);
    m.def("pmis_select", &pmis_select);
    m.def("interp_d1", &interp_d1);
    m.def("interp_d1_count", &interp_d1_count);
    m.def("truncate_rows", &truncate_rows);
    m.def("ilu0_setup", &ilu0_setup);
    m.def("ilu0_setup_block", &ilu0_setup_block);
    m.def("ilu0_apply_sorted", &ilu0_apply_sorted);
    m.def("ilu0_apply_block", &ilu0_apply_block);
}
