// Host check of the short exact forms of romanimpreprocess_amd/csrc/short_forms.h (the header the device code calls), built and run
// by tests/test_short_forms_host.py with the host compiler and -ffp-contract=off.
//   quotient: rip_div_rcp1(a, b, RN(1/b)) against a / b, bit for bit, for EVERY f32 numerator mantissa at three exponents and a
//             fixed list of divisors (the cases the argument in the header leaves to enumeration are among them);
//   hypot:    rip_hypot_short against (float)sqrt((double)a*a + (double)b*b) on seeded pairs and on pairs whose root lies within
//             a few f64 steps of an f32 rounding midpoint, on both sides, under reciprocal-root estimates of every quality the
//             header admits (the device passes v_rsq_f64; here 1/sqrt(T) with a planted relative error up to 2^-20).
// Prints one line per part and "OK" at the end; exit status 1 on any mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../romanimpreprocess_amd/csrc/short_forms.h"

static inline float u2f(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static inline uint32_t f2u(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
static inline uint64_t d2u(double d) {
    uint64_t u;
    memcpy(&u, &d, 8);
    return u;
}
struct Rng {   // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    double uniform() { return (double)(next() >> 11) * 0x1p-53; }
};

// ---------------------------------------------------------------------------------------------------------------- quotient
static std::vector<float> divisors() {
    std::vector<float> d;
    // 1, the largest and smallest mantissas, all ones and one-off, the middle, 1/3-like patterns, near sqrt(2)
    const uint32_t mant[] = {0x000000, 0x000001, 0x000002, 0x000003, 0x7fffff, 0x7ffffe, 0x7ffffd, 0x7ffffc, 0x400000, 0x400001,
                             0x3fffff, 0x555555, 0x2aaaaa, 0x3504f3, 0x3504f4, 0x7ffff0, 0x7fff00, 0x7f0000, 0x600000, 0x000100};
    for (uint32_t m : mant) d.push_back(u2f(0x3f800000u | m));
    // the edges of the voted ranges, just inside: rcp_safe (1e-18, 1e18), rip_mid_range (1.8e-18, 5.7e17), rip_mid36 (1.5e-11,
    // 6.8e10), and the clip of the gain (1e-4, 1e4); both signs of the widest
    const float lo[] = {1e-18f, 1.8e-18f, 1.5e-11f}, hi[] = {1e18f, 5.7e17f, 6.8e10f};
    for (float x : lo) d.push_back(nextafterf(x, 1.0f)), d.push_back(nextafterf(nextafterf(x, 1.0f), 1.0f));
    for (float x : hi) d.push_back(nextafterf(x, 1.0f)), d.push_back(nextafterf(nextafterf(x, 1.0f), 1.0f));
    d.push_back(1e-4f), d.push_back(1e4f), d.push_back(-nextafterf(1e-18f, 1.0f)), d.push_back(-nextafterf(1e18f, 1.0f));
    // all-ones and one-off mantissas at the ends of the widest range too
    d.push_back(u2f((uint32_t)(127 - 59) << 23 | 0x7fffff)), d.push_back(u2f((uint32_t)(127 + 58) << 23 | 0x7ffffe));
    Rng r{20260101};
    for (int i = 0; i < 700; ++i) d.push_back(u2f(0x3f800000u | (uint32_t)(r.next() & 0x7fffff)));              // any mantissa
    for (int i = 0; i < 200; ++i) d.push_back(u2f(0x3f800000u | (0x7fffffu - (uint32_t)(r.next() & 0xffff))));   // near 2
    for (int i = 0; i < 100; ++i) {                                                                              // any voted exponent
        const uint32_t e = 127 - 59 + (uint32_t)(r.next() % 118);
        d.push_back(u2f((uint32_t)(r.next() & 1) << 31 | e << 23 | (uint32_t)(r.next() & 0x7fffff)));
    }
    return d;
}

__attribute__((noinline)) static long div_mismatches(float b, uint32_t expo, float *first) {
    const float rb = 1.0f / b;   // correctly rounded, as rip_rcp_mid is on the device
    long bad = 0;
    for (uint32_t m = 0; m < (1u << 23); ++m) {   // (nothing but the count in this loop: it vectorises)
        const float a = u2f(expo << 23 | m);
        bad += f2u(rip_div_rcp1(a, b, rb)) != f2u(a / b);
    }
    for (uint32_t m = 0; bad && m < (1u << 23); ++m) {
        const float a = u2f(expo << 23 | m);
        if (f2u(rip_div_rcp1(a, b, rb)) != f2u(a / b)) return *first = a, bad;
    }
    return bad;
}

static long check_quotient(int nthreads) {
    const std::vector<float> div = divisors();
    const uint32_t expos[3] = {127 - 42, 127, 127 + 65};   // the ends of the numerators' range and the middle
    std::vector<long> bad(nthreads, 0);
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t)
        th.emplace_back([&, t] {
            for (size_t i = t; i < div.size() * 3; i += nthreads) {
                float first = 0.0f;
                const long n = div_mismatches(div[i / 3], expos[i % 3], &first);
                if (n) printf("quotient: divisor %a, numerator exponent %d: %ld mismatches, first at a = %a\n", div[i / 3], (int)expos[i % 3] - 127, n, first);
                bad[t] += n;
            }
        });
    for (auto &x : th) x.join();
    long total = 0;
    for (long n : bad) total += n;
    // a zero numerator gives a zero (its sign is +0 where IEEE has -0 / b = -0 for b > 0: so it was with two corrections)
    for (float b : div)
        for (float a : {0.0f, -0.0f})
            if (rip_div_rcp1(a, b, 1.0f / b) != 0.0f) ++total, printf("quotient: %a / %a\n", a, b);
    printf("quotient: %zu divisors x 3 exponents x 2^23 mantissas, %ld mismatches\n", div.size(), total);
    return total;
}

// ---------------------------------------------------------------------------------------------------------------- hypot
static float hypot_ref(float a, float b) { return (float)sqrt((double)a * a + (double)b * b); }

struct HypotCount {
    long n = 0, accepted = 0, bad = 0, below = 0, above = 0, worst = 0;   // below / above: turned away beside a midpoint, by side
};
static void hypot_case(float a, float b, double e0, HypotCount &c) {
    const double T = rip_hypot_radicand(a, b);
    const double root = sqrt(T);
    bool ok;
    const float h = rip_hypot_short(T, (1.0 / root) * (1.0 + e0), ok);
    ++c.n;
    if (!(T >= 0x1p-120 && T < 0x1p120)) {
        if (ok) ++c.bad, printf("hypot: (%a, %a) accepted outside the range\n", a, b);
        return;
    }
    // the written bound: the refined root within 8 steps of the f64 root (re-derive g2 from the same operations)
    const double y = (1.0 / root) * (1.0 + e0), g0 = T * y, h0 = 0.5 * y, r = fma(-h0, g0, 0.5), g1 = fma(g0, r, g0);
    const double g2 = fma(fma(-g1, g1, T), h0, g1);
    const long steps = labs((long)(d2u(g2) - d2u(root)));
    if (steps > c.worst) c.worst = steps;
    if (steps > 8) ++c.bad, printf("hypot: (%a, %a), e0 %g: %ld steps from the f64 root\n", a, b, e0, steps);
    if (ok) {
        ++c.accepted;
        if (f2u(h) != f2u(hypot_ref(a, b))) ++c.bad, printf("hypot: (%a, %a), e0 %g: %a, reference %a\n", a, b, e0, h, hypot_ref(a, b));
    } else {
        const uint32_t lo = (uint32_t)d2u(g2) & 0x1fffffffu;
        if (lo < 0x10000000u) ++c.below; else ++c.above;
        // turned away only inside the guard band
        if (labs((long)lo - 0x10000000L) > (long)RIP_HYPOT_GUARD) ++c.bad, printf("hypot: (%a, %a) turned away outside the band\n", a, b);
    }
}

static long check_hypot() {
    Rng r{77};
    const double e0s[] = {0.0, 0x1p-23, -0x1p-23, 0x1p-20, -0x1p-20};
    HypotCount seeded, near;
    // seeded pairs: any mantissas, exponents over the accepted range and beyond it on both sides, zeros
    for (int i = 0; i < 400000; ++i) {
        const int ea = (int)(r.next() % 150) - 75, eb = (i & 3) ? ea + (int)(r.next() % 30) - 15 : (int)(r.next() % 150) - 75;
        float a = ldexpf(1.0f + (float)(r.next() & 0x7fffff) * 0x1p-23f, ea), b = ldexpf(1.0f + (float)(r.next() & 0x7fffff) * 0x1p-23f, eb);
        if (i % 1000 == 0) a = 0.0f;
        if (i % 1000 == 1) b = -0.0f;
        if (i % 1000 == 2) a = b = 0.0f;
        const double e0 = (i % 7 < 5) ? e0s[i % 7] : (r.uniform() - 0.5) * 0x1p-19;
        hypot_case((i & 8) ? -a : a, b, e0, seeded);
    }
    // roots beside a midpoint: b^2 / (2a) = half a step of a, so that sqrt(a^2 + b^2) = a + half a step + (a few f64 steps); the
    // floats around b move the root by about 2^6 f64 steps each
    for (int i = 0; i < 200000; ++i) {
        const float a = ldexpf(1.0f + (float)(r.next() & 0x7fffff) * 0x1p-23f, (int)(r.next() % 100) - 50);
        const float ulp = nextafterf(a, INFINITY) - a;
        const float b0 = (float)sqrt((double)a * (double)ulp);
        float b = b0;
        for (int k = 0; k < 3; ++k) b = nextafterf(b, 0.0f);
        for (int k = 0; k < 7; ++k, b = nextafterf(b, INFINITY)) hypot_case(a, (i & 1) ? -b : b, e0s[(i + k) % 5], near);
    }
    printf("hypot: seeded %ld pairs, %ld accepted, worst %ld steps; beside a midpoint %ld pairs, %ld accepted, turned away %ld below and %ld "
           "above the midpoint, worst %ld steps; %ld failures\n",
           seeded.n, seeded.accepted, seeded.worst, near.n, near.accepted, near.below, near.above, near.worst, seeded.bad + near.bad);
    long bad = seeded.bad + near.bad;
    if (seeded.accepted < seeded.n / 2 || seeded.accepted == seeded.n) ++bad, printf("hypot: the seeded pairs do not exercise both paths\n");
    if (near.below < 1000 || near.above < 1000 || near.accepted < 1000) ++bad, printf("hypot: the pairs beside a midpoint miss a side\n");
    return bad;
}

int main(int argc, char **argv) {
    const int nthreads = argc > 1 ? atoi(argv[1]) : 4;
    long bad = check_hypot();
    bad += check_quotient(nthreads < 1 ? 1 : nthreads);
    if (bad) return printf("FAILED: %ld\n", bad), 1;
    printf("OK\n");
    return 0;
}
