// The stop rule of the manifold mean on the squared norm (csrc/slk_math.hpp: MEAN_STOP_SQ) against the rule it stands for,
// sqrt(s) > 1e-6 with the correctly rounded square root: the constant is the last double whose root rounds to at most 1e-6, and
// s > MEAN_STOP_SQ equals sqrt(s) > 1e-6 on the doubles on either side of it, on 0, the denormals, infinity and the NaNs.  With
// it the domain tests of the exp series on the upper dword (nonneg_hi_below: x < 0.25, x < 4.0 for x >= +0 or NaN) against the
// comparisons they stand for.  Host code only: the host half of the header; no device is touched.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../slam-localization_amd/csrc/slk_math.hpp"

static double from_bits(uint64_t u)
{
    double d;
    std::memcpy(&d, &u, sizeof d);
    return d;
}

static uint64_t to_bits(double d)
{
    uint64_t u;
    std::memcpy(&u, &d, sizeof u);
    return u;
}

static int failures = 0;

static void check_stop(double sv, const char *what)
{
    const volatile double s = sv;                      // (no folding of the square root at compile time)
    const bool want = std::sqrt(s) > 1e-6;
    const bool got = s > slk::MEAN_STOP_SQ;
    if (got != want) {
        if (failures < 20) std::printf("MISMATCH stop rule, %s: s = %a  sqrt(s) > 1e-6 = %d  s > T = %d\n", what, sv, (int)want, (int)got);
        ++failures;
    }
}

static void check_domain(double xv, const char *what)
{
    const volatile double x = xv;
    const unsigned hi = (unsigned)(to_bits(xv) >> 32);
    const bool q = slk::nonneg_hi_below(hi, slk::HI_QUARTER), f = slk::nonneg_hi_below(hi, slk::HI_FOUR);
    if (q != (x < 0.25) || f != (x < 4.0)) {
        if (failures < 20) std::printf("MISMATCH domain test, %s: x = %a  x < 0.25 = %d / %d  x < 4 = %d / %d\n", what, xv, (int)(x < 0.25),
                                       (int)q, (int)(x < 4.0), (int)f);
        ++failures;
    }
}

int main()
{
    const double T = slk::MEAN_STOP_SQ, inf = std::numeric_limits<double>::infinity();
    // the constant itself: sqrt(T) <= 1e-6 < sqrt(nextafter(T, inf))
    {
        const volatile double t0 = T, t1 = std::nextafter(T, inf);
        if (!(std::sqrt(t0) <= 1e-6) || !(1e-6 < std::sqrt(t1))) {
            std::printf("MISMATCH constant: sqrt(T) = %a, sqrt(next) = %a, 1e-6 = %a\n", std::sqrt(t0), std::sqrt(t1), 1e-6);
            ++failures;
        }
    }
    if ((to_bits(0.25) & 0xffffffffull) != 0 || (to_bits(4.0) & 0xffffffffull) != 0 || (unsigned)(to_bits(0.25) >> 32) != slk::HI_QUARTER ||
        (unsigned)(to_bits(4.0) >> 32) != slk::HI_FOUR) {
        std::printf("MISMATCH bounds of the domain tests\n");
        ++failures;
    }
    // four thousand doubles on either side of T, one by one
    double below = T, above = T;
    check_stop(T, "T");
    for (int i = 0; i < 4000; ++i) {
        below = std::nextafter(below, 0.0);
        above = std::nextafter(above, inf);
        check_stop(below, "below T");
        check_stop(above, "above T");
    }
    const struct { double s; const char *what; } named[] = {
        {0.0, "+0"}, {-0.0, "-0"}, {from_bits(1), "smallest denormal"}, {from_bits(0x000fffffffffffffull), "largest denormal"},
        {DBL_MIN, "DBL_MIN"}, {1e-12, "1e-12"}, {1e-6, "1e-6"}, {1.0, "1"}, {DBL_MAX, "DBL_MAX"}, {inf, "+inf"},
        {std::numeric_limits<double>::quiet_NaN(), "quiet NaN"}, {from_bits(0xfff8000000000000ull), "quiet NaN, sign set"},
        {from_bits(0x7ff0000000000001ull), "signalling NaN"}, {-1.0, "-1 (no sum of squares, for the record)"},
    };
    for (const auto &c : named) check_stop(c.s, c.what);
    // random doubles over all magnitudes (splitmix64, fixed seed), as they are and folded to the neighbourhood of T
    uint64_t st = 0x5eedce0012345ull;
    for (int i = 0; i < 200000; ++i) {
        st += 0x9e3779b97f4a7c15ull;
        uint64_t z = st;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        z ^= z >> 31;
        const double pos = from_bits(z & 0x7fffffffffffffffull);       // +0, positive, +inf or a NaN
        check_stop(pos, "random");
        check_stop(from_bits((to_bits(T) & 0xfff0000000000000ull) | (z & 0x000fffffffffffffull)), "random, binade of T");
        check_domain(pos, "random");
        check_domain(from_bits(z | 0x7ff0000000000000ull), "random NaN / inf of either sign");
        check_domain(from_bits((z & 0x003fffffffffffffull) | 0x3fc0000000000000ull), "random, 0.125 .. 8");
    }
    for (double x : {0.0, 0.25, 4.0, inf}) {
        check_domain(x, "edge");
        check_domain(std::nextafter(x, 0.0), "edge, one below");
        if (x != inf) check_domain(std::nextafter(x, inf), "edge, one above");
    }
    if (failures) {
        std::printf("%d mismatches\n", failures);
        return 1;
    }
    std::printf("mean stop threshold ok\n");
    return 0;
}
