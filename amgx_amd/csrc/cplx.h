// Device complex value type of the dZZI / dCCI / dZCI modes.
//
// cplx<R> is two R laid out as (re, im): the interleaved layout of
// complex64 / complex128 tensors, so bindings reinterpret_cast tensor
// storage to cplx<R>*. alignas(2*sizeof(R)) makes one complex128 element a
// single 16-byte load or store (global_load_dwordx4) and one complex64
// element an 8-byte one.
//
// Usable from device code, from host code of a HIP translation unit and from
// a plain host compiler without HIP (tests/cplx_host_check.cpp); only the
// cross-lane shuffles need hipcc.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AMGX_HD __host__ __device__ __forceinline__
#else
#define AMGX_HD inline
#endif

namespace amgx_hip {

template <typename R>
struct alignas(2 * sizeof(R)) cplx {
    R re, im;

    cplx() = default;
    // from a real (TV(0), T(1) in the kernel templates) or from two parts
    AMGX_HD cplx(R r, R i = R(0)) : re(r), im(i) {}
    // precision change: cplx<float> matrix values x cplx<double> vectors
    template <typename S>
    AMGX_HD explicit cplx(const cplx<S>& o) : re((R)o.re), im((R)o.im) {}

    AMGX_HD cplx& operator+=(const cplx& o) { re += o.re; im += o.im; return *this; }
    AMGX_HD cplx& operator-=(const cplx& o) { re -= o.re; im -= o.im; return *this; }
    AMGX_HD cplx& operator*=(const cplx& o) {
        R r = re * o.re - im * o.im;
        im = re * o.im + im * o.re;
        re = r;
        return *this;
    }
    AMGX_HD cplx& operator*=(R s) { re *= s; im *= s; return *this; }
};

template <typename R>
AMGX_HD cplx<R> operator+(cplx<R> a, const cplx<R>& b) { return a += b; }
template <typename R>
AMGX_HD cplx<R> operator-(cplx<R> a, const cplx<R>& b) { return a -= b; }
template <typename R>
AMGX_HD cplx<R> operator-(const cplx<R>& a) { return cplx<R>(-a.re, -a.im); }
template <typename R>
AMGX_HD cplx<R> operator*(cplx<R> a, const cplx<R>& b) { return a *= b; }
template <typename R>
AMGX_HD cplx<R> operator*(cplx<R> a, R s) { return a *= s; }
template <typename R>
AMGX_HD cplx<R> operator*(R s, cplx<R> a) { return a *= s; }

template <typename R>
AMGX_HD bool operator==(const cplx<R>& a, const cplx<R>& b) {
    return a.re == b.re && a.im == b.im;
}
template <typename R>
AMGX_HD bool operator!=(const cplx<R>& a, const cplx<R>& b) { return !(a == b); }

template <typename R>
AMGX_HD cplx<R> conj(const cplx<R>& a) { return cplx<R>(a.re, -a.im); }
template <typename R>
AMGX_HD R abs2(const cplx<R>& a) { return a.re * a.re + a.im * a.im; }
template <typename R>
AMGX_HD R abs(const cplx<R>& a) { return std::sqrt(abs2(a)); }

// 1/d = conj(d) / |d|^2
template <typename R>
AMGX_HD cplx<R> recip(const cplx<R>& d) {
    R s = R(1) / abs2(d);
    return cplx<R>(d.re * s, -d.im * s);
}
template <typename R>
AMGX_HD cplx<R> operator/(const cplx<R>& a, const cplx<R>& d) { return a * recip(d); }
template <typename R>
AMGX_HD cplx<R> operator/(cplx<R> a, R s) { a.re /= s; a.im /= s; return a; }

// conj(a) * b with every product rounded on its own (no fused
// multiply-add), so conj_mul(x, x).im is exactly zero: the two cross
// products x.re*x.im and x.im*x.re round identically and cancel.
template <typename R>
AMGX_HD cplx<R> conj_mul(const cplx<R>& a, const cplx<R>& b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    R rr = a.re * b.re, ii = a.im * b.im;
    R ri = a.re * b.im, ir = a.im * b.re;
    return cplx<R>(rr + ii, ri - ir);
}

// Real counterparts of conj_mul / abs / abs2, so one kernel template
// (reduce_stage1) serves real and complex T. Plain products with contraction
// left on: a real dot stays one fused multiply-add per element.
AMGX_HD double conj_mul(double a, double b) { return a * b; }
AMGX_HD float conj_mul(float a, float b) { return a * b; }
AMGX_HD double abs(double a) { return std::fabs(a); }
AMGX_HD float abs(float a) { return std::fabs(a); }
AMGX_HD double abs2(double a) { return a * a; }
AMGX_HD float abs2(float a) { return a * a; }

// |a| in double whatever the storage type: the magnitude the setup kernels
// compare (matching edge weights, the DILU pivot guard). Complex: the modulus
// from the two parts widened to double first, so a complex64 entry whose
// modulus is representable compares exactly like its real counterpart.
AMGX_HD double absd(double a) { return std::fabs(a); }
AMGX_HD double absd(float a) { return std::fabs((double)a); }
template <typename R>
AMGX_HD double absd(const cplx<R>& a) {
    double re = (double)a.re, im = (double)a.im;
    return std::sqrt(re * re + im * im);
}

template <typename T> struct is_cplx { static constexpr bool value = false; };
template <typename R> struct is_cplx<cplx<R>> { static constexpr bool value = true; };
// R for cplx<R>, T itself for a real T: the type of |x| and of a norm
template <typename T> struct real_of { using type = T; };
template <typename R> struct real_of<cplx<R>> { using type = R; };

#if defined(__HIPCC__)
// cross-lane moves of the two components (wave_reduce_sum, csrmv_vec); the
// using-declarations keep the built-in real overloads visible to kernels
// inside this namespace
using ::__shfl_down;
using ::__shfl_xor;
using ::__shfl;
template <typename R>
__device__ __forceinline__ cplx<R> __shfl(const cplx<R>& v, int src,
                                          int width = warpSize) {
    return cplx<R>(::__shfl(v.re, src, width), ::__shfl(v.im, src, width));
}
template <typename R>
__device__ __forceinline__ cplx<R> __shfl_down(const cplx<R>& v, unsigned off,
                                               int width = warpSize) {
    return cplx<R>(::__shfl_down(v.re, off, width),
                   ::__shfl_down(v.im, off, width));
}
template <typename R>
__device__ __forceinline__ cplx<R> __shfl_xor(const cplx<R>& v, int mask,
                                              int width = warpSize) {
    return cplx<R>(::__shfl_xor(v.re, mask, width),
                   ::__shfl_xor(v.im, mask, width));
}

// Accumulation into a complex slot is one atomic per part (LDS hash tables,
// the atomic restriction). The two parts of a slot are therefore only
// consistent once every contributor is done: read them after the barrier or
// kernel boundary that ends the accumulation, never in between.
using ::atomicAdd;
template <typename R>
__device__ __forceinline__ void atomicAdd(cplx<R>* p, const cplx<R>& v) {
    ::atomicAdd(&p->re, v.re);
    ::atomicAdd(&p->im, v.im);
}
#endif

static_assert(sizeof(cplx<float>) == 8 && alignof(cplx<float>) == 8,
              "cplx<float> must match interleaved complex64");
static_assert(sizeof(cplx<double>) == 16 && alignof(cplx<double>) == 16,
              "cplx<double> must match interleaved complex128");

}  // namespace amgx_hip
