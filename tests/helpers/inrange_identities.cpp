// CPU model of csrc/rtk_device_math.h's sqrt_inrange / rcp_inrange against the full expansions the compiler emits for
// __builtin_sqrt(double) and 1.0 / x on gfx950 (tests/test_inrange_identities.py).  Both short forms and both full
// expansions are restated here with fma(); the scaling and fix-up instructions of the full forms follow the ISA manual's
// pseudo-code (V_DIV_SCALE_F64, V_DIV_FMAS_F64, V_DIV_FIXUP_F64, V_LDEXP_F64, V_CMP_CLASS_F64).  The hardware seed
// (V_RSQ_F64, V_RCP_F64: documented to 2^29 ulp of the f64 result, i.e. 2^-23 relative) is a parameter: the true value
// perturbed by -4 .. 4 units of that precision and by random amounts in between.
//
//   inrange_identities <significands>     prints "identity mismatches: N" and "guard failures: N"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

static uint64_t bits(double x) { uint64_t u; std::memcpy(&u, &x, 8); return u; }
static double from_bits(uint64_t u) { double x; std::memcpy(&x, &u, 8); return x; }
static int exponent_of(double x) { return int((bits(x) >> 52) & 2047u); }  // the biased exponent field, as the ISA manual's exponent()
static bool is_denorm(double x) { return exponent_of(x) == 0 && (bits(x) << 12) != 0; }

// ---- the guard (rtk_device_math.h inrange_f64) ----
static bool inrange_f64(double x) {
    const uint32_t hi = uint32_t(bits(x) >> 32);
    return uint32_t(hi - 0x20100000u) < 0x3FC00000u;
}

// ---- the seeds ----
// the true value rounded to double, moved by `units` x 2^29 ulp plus `fine` ulp
static double perturb(double v, int units, int64_t fine) { return from_bits(bits(v) + uint64_t(int64_t(units) * (int64_t(1) << 29) + fine)); }
static double true_rsq(double x) { return double(1.0L / sqrtl((long double)x)); }
static double true_rcp(double x) { return double(1.0L / (long double)x); }

// ---- square root ----
static double sqrt_short(double x, double y) {  // y = the seed for x
    double g = x * y;
    double h = y * 0.5;
    const double r = std::fma(-h, g, 0.5);
    g = std::fma(g, r, g);
    double d = std::fma(-g, g, x);
    h = std::fma(h, r, h);
    g = std::fma(d, h, g);
    d = std::fma(-g, g, x);
    return std::fma(d, h, g);
}
// the compiler's expansion; *scaled_operand = what the seed instruction sees
static double sqrt_scaled_operand(double x) { return x < 0x1p-767 ? std::ldexp(x, 256) : x; }
static double sqrt_full(double x, double y) {  // y = the seed for sqrt_scaled_operand(x)
    const bool small = x < 0x1p-767;
    const double X = small ? std::ldexp(x, 256) : x;
    double g = X * y;
    double h = y * 0.5;
    const double r = std::fma(-h, g, 0.5);
    g = std::fma(g, r, g);
    double d = std::fma(-g, g, X);
    h = std::fma(h, r, h);
    g = std::fma(d, h, g);
    d = std::fma(-g, g, X);
    g = std::fma(d, h, g);
    g = std::ldexp(g, small ? -128 : 0);
    const bool pass = X == 0.0 || (std::isinf(X) && X > 0);  // v_cmp_class {+-0, +inf}
    return pass ? X : g;
}

// ---- reciprocal ----
static double rcp_short(double x, double y) {  // y = the seed for x
    double e = std::fma(-x, y, 1.0);
    y = std::fma(y, e, y);
    e = std::fma(-x, y, 1.0);
    y = std::fma(y, e, y);
    const double r = std::fma(-x, y, 1.0);
    return std::fma(r, y, y);
}
// V_DIV_SCALE_F64 D, vcc, S0, S1 (denominator), S2 (numerator)
static double div_scale(double s0, double s1, double s2, bool& vcc) {
    vcc = false;
    if (s2 == 0.0 || s1 == 0.0) return NAN;
    if (exponent_of(s2) - exponent_of(s1) >= 768) {
        vcc = true;
        return bits(s0) == bits(s1) ? std::ldexp(s0, 128) : s0;
    }
    if (is_denorm(s1)) return std::ldexp(s0, 128);
    const bool rcp_denorm = is_denorm(1.0 / s1), quot_denorm = is_denorm(s2 / s1);
    if (rcp_denorm && quot_denorm) {
        vcc = true;
        return bits(s0) == bits(s1) ? std::ldexp(s0, 128) : s0;
    }
    if (rcp_denorm) return std::ldexp(s0, -128);
    if (quot_denorm) {
        vcc = true;
        return bits(s0) == bits(s2) ? std::ldexp(s0, 128) : s0;
    }
    if (exponent_of(s2) <= 53) return std::ldexp(s0, 128);
    return s0;
}
static double div_fmas(double a, double b, double c, bool vcc) { return vcc ? std::ldexp(std::fma(a, b, c), 64) : std::fma(a, b, c); }
// V_DIV_FIXUP_F64 S0 (quotient), S1 (denominator), S2 (numerator)
static double div_fixup(double s0, double s1, double s2) {
    const bool neg = std::signbit(s1) != std::signbit(s2);
    if (std::isnan(s2)) return s2;
    if (std::isnan(s1)) return s1;
    if (s1 == 0.0 && s2 == 0.0) return NAN;
    if (std::isinf(s1) && std::isinf(s2)) return NAN;
    if (s1 == 0.0 || std::isinf(s2)) return neg ? -INFINITY : INFINITY;
    if (std::isinf(s1) || s2 == 0.0) return neg ? -0.0 : 0.0;
    if (exponent_of(s2) - exponent_of(s1) < -1075) return neg ? -0.0 : 0.0;
    if (exponent_of(s1) == 2047) return neg ? -INFINITY : INFINITY;
    return neg ? -std::fabs(s0) : std::fabs(s0);
}
static double rcp_scaled_operand(double x) { bool v; return div_scale(x, x, 1.0, v); }
static double rcp_full(double x, double y) {  // y = the seed for rcp_scaled_operand(x)
    bool vcc_d, vcc;
    const double D = div_scale(x, x, 1.0, vcc_d);
    double e = std::fma(-D, y, 1.0);
    y = std::fma(y, e, y);
    e = std::fma(-D, y, 1.0);
    y = std::fma(y, e, y);
    const double N = div_scale(1.0, x, 1.0, vcc);
    double q = N * y;
    const double r = std::fma(-D, q, N);
    q = div_fmas(r, y, q, vcc);
    return div_fixup(q, x, 1.0);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static long mismatches = 0, evaluations = 0;
static void check_operand(double x, int fine_seeds) {
    const double ys = true_rsq(x), yr = true_rcp(x);
    for (int k = -4; k <= 4 + fine_seeds; k++) {
        const int units = k <= 4 ? k : 0;
        const int64_t fine = k <= 4 ? 0 : int64_t(next_u64() % ((uint64_t(8) << 29) + 1)) - (int64_t(4) << 29);
        const double s_seed = perturb(ys, units, fine), r_seed = perturb(yr, units, fine);
        const double a = sqrt_short(x, s_seed), b = sqrt_full(x, s_seed);
        const double c = rcp_short(x, r_seed), d = rcp_full(x, r_seed);
        if (bits(a) != bits(b) || bits(c) != bits(d)) {
            if (mismatches < 10) std::printf("MISMATCH x=%a seed offset %d units %+lld ulp: sqrt %a vs %a, rcp %a vs %a\n", x, units, (long long)fine, a, b, c, d);
            mismatches++;
        }
        evaluations++;
    }
}

int main(int argc, char** argv) {
    const long n_sig = argc > 1 ? std::atol(argv[1]) : (1l << 24);
    // (a) every admitted exponent, with the all-zeros (a power of two), all-ones and a few random significands
    for (int e = 513; e <= 1532; e++) {
        const uint64_t sigs[5] = {0, (uint64_t(1) << 52) - 1, 1, next_u64() >> 12, next_u64() >> 12};
        for (uint64_t s : sigs) {
            const double x = from_bits((uint64_t(e) << 52) | s);
            if (!inrange_f64(x)) { std::printf("GUARD rejects admitted %a\n", x); mismatches++; }
            check_operand(x, 4);
        }
    }
    // (b) random significands (all-ones and powers of two among them), the exponent walking through the admitted range
    for (long i = 0; i < n_sig; i++) {
        uint64_t s = next_u64() >> 12;
        if (i % 4096 == 0) s = (uint64_t(1) << 52) - 1;
        if (i % 4096 == 1) s = 0;
        if (i % 4096 == 2) s = (uint64_t(1) << 52) - 1 - (next_u64() & 7);
        const int e = 513 + int((uint64_t(i) * 7919u) % 1020u);
        check_operand(from_bits((uint64_t(e) << 52) | s), 2);
    }
    // (c) the guard: the last admitted values pass and keep the identity; everything past them, and every special, is refused
    long guard_failures = 0;
    const double lo = 0x1p-510, hi_excl = 0x1p510;
    const double admitted[] = {lo, std::nextafter(lo, 1.0), std::nextafter(hi_excl, 0.0), 1.0, 0x1p-46, 3.0};
    for (double x : admitted) {
        if (!inrange_f64(x)) { std::printf("GUARD rejects %a\n", x); guard_failures++; }
        check_operand(x, 4);
    }
    const double refused[] = {0.0, -0.0, from_bits(1), 0x1p-1074, 0x1p-1023, std::nextafter(0x1p-1022, 0.0), 0x1p-1022, 0x1p-768, 0x1p-767,
                              std::nextafter(lo, 0.0), hi_excl, std::nextafter(hi_excl, INFINITY), 0x1p767, 0x1p1022, 0x1p1023, 1.7976931348623157e308,
                              INFINITY, -INFINITY, NAN, -NAN, from_bits(0x7FF0000000000001ull), -1.0, -0x1p-510, -0x1p509, -3.0, 1e-160 * 1e-160, 1e300};
    for (double x : refused)
        if (inrange_f64(x)) { std::printf("GUARD admits %a\n", x); guard_failures++; }
    // ... and what the guard sends to the full forms is what they exist for: the scaled paths really differ from the plain ones
    long scaled_paths = 0;
    for (double x : {0x1p-800, 0x1p-1030, 0x1p1023})
        scaled_paths += bits(sqrt_scaled_operand(x)) != bits(x) || bits(rcp_scaled_operand(x)) != bits(x);
    std::printf("evaluations: %ld\nidentity mismatches: %ld\nguard failures: %ld\nscaled paths seen: %ld\n", evaluations, mismatches, guard_failures, scaled_paths);
    return (mismatches || guard_failures) ? 1 : 0;
}
