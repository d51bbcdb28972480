// Stand-alone host check of amgx_amd/csrc/cplx.h (built and run by
// tests/test_cplx_host.py): every operator of cplx<R> against std::complex<R>
// on a fixed table of values, for R = double and float, and the real overloads
// of conj_mul / abs / abs2 against the plain expressions. Exit status 0 = pass.
//
// Bound: each operator is a handful of correctly rounded operations, so a
// result may differ from std::complex by a few ulp of the operand magnitudes
// (std::complex division and abs use scaled algorithms, cplx the textbook
// formulas). The longest chain is a / b = a * (conj(b) / |b|^2): about 6
// roundings on our side and about 4 in std::complex, so 16 eps times the
// natural scale of the result is the tolerance; a wrong sign or a swapped
// component misses it by a factor of 1/eps.

#include <cmath>
#include <complex>
#include <cstdio>
#include <limits>
#include <type_traits>

#include "cplx.h"

using amgx_hip::cplx;

static int failures = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

template <typename R>
static bool close(const cplx<R>& got, const std::complex<R>& want, R scale) {
    const R tol = R(16) * std::numeric_limits<R>::epsilon() * scale;
    return std::abs(got.re - want.real()) <= tol &&
           std::abs(got.im - want.imag()) <= tol;
}

template <typename R>
static void check_type(const char* name) {
    using C = cplx<R>;
    using S = std::complex<R>;
    // zero, pure real, pure imaginary, mixed magnitudes and signs
    const R tab[][2] = {
        {R(0), R(0)},        {R(1), R(0)},        {R(-2.5), R(0)},
        {R(0), R(1)},        {R(0), R(-3.25)},    {R(1.5), R(-0.75)},
        {R(-0.3), R(0.7)},   {R(1e-3), R(2e5)},   {R(-4e4), R(3e-2)},
        {R(1e-6), R(-1e-6)}, {R(123.456), R(-654.321)},
    };
    const int n = (int)(sizeof(tab) / sizeof(tab[0]));
    int before = failures;
    for (int i = 0; i < n; ++i) {
        const C a(tab[i][0], tab[i][1]);
        const S sa(tab[i][0], tab[i][1]);
        const R ma = std::abs(sa);
        CHECK(a.re == tab[i][0] && a.im == tab[i][1]);
        CHECK(close(conj(a), std::conj(sa), ma));
        CHECK(conj(a).re == a.re && conj(a).im == -a.im);
        CHECK(close(-a, -sa, ma));
        CHECK(std::abs(abs2(a) - std::norm(sa)) <=
              R(16) * std::numeric_limits<R>::epsilon() * ma * ma);
        CHECK(std::abs(abs(a) - ma) <=
              R(16) * std::numeric_limits<R>::epsilon() * ma);
        CHECK(abs2(a) >= R(0) && abs(a) >= R(0));
        CHECK(a == a && !(a != a));
        CHECK(close(a * R(3), sa * R(3), ma * 3));
        CHECK(close(R(-0.5) * a, R(-0.5) * sa, ma));
        CHECK(close(a / R(4), sa / R(4), ma));
        { C t = a; t *= R(7); CHECK(close(t, sa * R(7), ma * 7)); }
        // conj(a) * a is real: the imaginary part cancels exactly
        CHECK(conj_mul(a, a).im == R(0));
        CHECK(conj_mul(a, a).re >= R(0));
        if (ma != R(0)) {
            CHECK(close(recip(a), S(1) / sa, R(1) / ma));
            CHECK(close(C(1) / a, S(1) / sa, R(1) / ma));
        }
        for (int j = 0; j < n; ++j) {
            const C b(tab[j][0], tab[j][1]);
            const S sb(tab[j][0], tab[j][1]);
            const R mb = std::abs(sb);
            CHECK(close(a + b, sa + sb, ma + mb));
            CHECK(close(a - b, sa - sb, ma + mb));
            CHECK(close(a * b, sa * sb, ma * mb));
            CHECK(close(conj_mul(a, b), std::conj(sa) * sb, ma * mb));
            { C t = a; t += b; CHECK(close(t, sa + sb, ma + mb)); }
            { C t = a; t -= b; CHECK(close(t, sa - sb, ma + mb)); }
            { C t = a; t *= b; CHECK(close(t, sa * sb, ma * mb)); }
            if (mb != R(0)) CHECK(close(a / b, sa / sb, ma / mb));
            CHECK((a == b) == (sa == sb));
            CHECK((a != b) == (sa != sb));
        }
    }
    // real overloads (one reduction kernel serves real and complex T): one
    // correctly rounded operation each, so they are exact against the plain
    // expression, and they agree with the complex ones on a real argument
    using amgx_hip::abs;
    using amgx_hip::abs2;
    using amgx_hip::conj_mul;
    for (int i = 0; i < n; ++i) {
        const R a = tab[i][0], im = tab[i][1];
        CHECK(abs(a) == std::fabs(a) && abs(-a) == abs(a) && abs(a) >= R(0));
        CHECK(abs2(a) == a * a && abs2(-a) == abs2(a));
        CHECK(abs(C(a)) == abs(a) && abs2(C(a)) == abs2(a));
        CHECK(conj_mul(a, im) == a * im && conj_mul(im, a) == a * im);
        CHECK(conj_mul(C(a), C(im)).re == conj_mul(a, im));
        CHECK(conj_mul(C(a), C(im)).im == R(0));
        CHECK(conj_mul(a, a) == abs2(a));
    }
    static_assert(std::is_same<decltype(abs(R(1))), R>::value &&
                  std::is_same<decltype(abs2(R(1))), R>::value &&
                  std::is_same<decltype(conj_mul(R(1), R(1))), R>::value,
                  "real overloads stay in the argument's precision");
    static_assert(!amgx_hip::is_cplx<R>::value && amgx_hip::is_cplx<C>::value &&
                  std::is_same<typename amgx_hip::real_of<R>::type, R>::value &&
                  std::is_same<typename amgx_hip::real_of<C>::type, R>::value,
                  "type traits of the reduction partials");

    // construction from a real: the kernels' TV(0) and T(1)
    CHECK(C(0).re == R(0) && C(0).im == R(0));
    CHECK(C(1).re == R(1) && C(1).im == R(0));
    CHECK(C(0) == C(R(0), R(0)) && C(1) != C(0));
    std::printf("%s: %s\n", name, failures == before ? "ok" : "FAILED");
}

int main() {
    // layout: interleaved complex64 / complex128, one aligned element
    static_assert(sizeof(cplx<float>) == 8 && alignof(cplx<float>) == 8, "");
    static_assert(sizeof(cplx<double>) == 16 && alignof(cplx<double>) == 16, "");
    CHECK(sizeof(cplx<float>) == sizeof(std::complex<float>));
    CHECK(sizeof(cplx<double>) == sizeof(std::complex<double>));
    {
        cplx<double> arr[2] = {cplx<double>(1, 2), cplx<double>(3, 4)};
        const double* flat = reinterpret_cast<const double*>(arr);
        CHECK(flat[0] == 1 && flat[1] == 2 && flat[2] == 3 && flat[3] == 4);
        cplx<float> arf[2] = {cplx<float>(1, 2), cplx<float>(3, 4)};
        const float* flf = reinterpret_cast<const float*>(arf);
        CHECK(flf[0] == 1 && flf[1] == 2 && flf[2] == 3 && flf[3] == 4);
    }

    check_type<double>("cplx<double>");
    check_type<float>("cplx<float>");

    // float -> double conversion (C matrix x Z vector) is exact
    const float fv[][2] = {{0.f, 0.f}, {1.5f, -0.75f}, {1e-3f, 2e5f},
                           {0.1f, -0.3f}};
    for (const auto& p : fv) {
        cplx<double> d = (cplx<double>)cplx<float>(p[0], p[1]);
        CHECK(d.re == (double)p[0] && d.im == (double)p[1]);
        // mixed product accumulates in double
        cplx<double> x(0.25, -3.0);
        std::complex<double> want =
            std::complex<double>(p[0], p[1]) * std::complex<double>(0.25, -3.0);
        CHECK(close(d * x, want, std::abs(want) + 1e-300));
    }

    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("all cplx checks passed\n");
    return 0;
}
