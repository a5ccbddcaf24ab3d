// Short exact forms of the f32 quotient and of hypotf, stated once for the device (device_rampfit.h, chain_common.h) and for the
// host program that checks them (tests/host/short_forms_check.cpp).  Plain C++: fma / fmaf and integer operations only; the
// hardware estimates (v_rcp_f32, v_rsq_f64) are the callers' arguments.  Compile with -ffp-contract=off, as everything here is.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RIP_SF __host__ __device__ __forceinline__
#else
#define RIP_SF static inline
#endif

// The parts of the second lean pass of the fused chain (profiles/lean2_chain.txt), each separable for an attribution build
// (make EXTRA=-DRIP_LEAN2=<mask>): 1 = one correction per quotient, 2 = the short hypot, 4 = no idle last row step
// (chain2_kernel.h).  Results are the same bits under every mask.
#ifndef RIP_LEAN2
#define RIP_LEAN2 7
#endif

// ------------------------------------------------------------------------------------------------ a / b
// IEEE a/b from the correctly rounded reciprocal rb = RN(1/b) (rip_rcp_mid) by ONE correction with an exact residual:
//     q0 = RN(a rb),   r0 = a - b q0 (fma: exact, see below),   q1 = RN(q0 + r0 rb) = RN(a/b).
// Signs and powers of two carry through every step, so take a, b in [1, 2), b > 1 (b = 1: rb = 1, q0 = a), q = a/b, and
// u = ulp(q): 2^-23 where a >= b, 2^-24 where a < b.  e = rb - 1/b, |e| <= 2^-25 (1/b lies in (1/2, 1)).
//  (1) a rb = q + a e, so |q0 - q| <= a|e| + u/2: at most u where a >= b (|e| <= u/4, a < 2), at most (a + 1) u/2 < 3u/2 where
//      a < b.  The second case does NOT make q0 one of the two neighbours of q, which is what Markstein's division theorem
//      (P. Markstein, "IA-64 and Elementary Functions", ch. 8: rb correctly rounded + q0 faithful => q1 correctly rounded) asks for, so its
//      argument is repeated here with what q0 does satisfy.
//  (2) v = q0 + r0' rb is what the last fma rounds, r0' = RN(a - b q0) = b (q - q0) + rho.  With 1 - b rb = -b e:
//      v - q = (q - q0) b e + rho rb.  r0 is a multiple of ulp(b) ulp(q0) = 2^-23 u and exact (rho = 0) while |q - q0| <= 2u/b;
//      always |rho| <= 2^-23 u.  So |v - q| <= (3u/2) 2 (u/2) + 2^-23 u < 2^-22 u.  (q0 falls into the binade below q only for
//      a = b, q0 = 1 - 2^-24: then r0 = 2^-24 b exactly and v = 1 + 2^-24 b e rounds to 1.)
//  (3) q1 != RN(q) only if a midpoint m of two neighbouring floats has |q - m| <= |v - q|.  b m - a is a non-zero multiple of
//      2^-23 u/2 (q is never a midpoint), so |q - m| >= 2^-24 u / b.  Such a q lies within 2^-22 u of m, and then
//        - q0 is a neighbour of m (|q0 - q| <= u/2 + 2^-22 u) unless a rb passes the NEXT midpoint, m +- u:
//          a|e| >= u - 2^-22 u, which with |e| <= u/2 needs a < b both within three steps of 2 (the cases listed below);
//        - with q0 a neighbour, rho = 0 and |v - q| <= (u/2)(1 + 2^-21) b |e|, so 2^-24 u/b <= |v - q| needs, where a < b
//          (|e| <= u/2, 2^-24 = u), b^2 >= 4 (1 - 2^-21), and where a >= b (|e| <= u/4, 2^-24 = u/2) the same.
//      Both leave only divisors with a mantissa of all ones or one off (b = 2 - 2^-23, 2 - 2^-22).  For these two the host check
//      compares q1 with a/b for every one of the 2^23 numerator mantissas; so it does for the edges of the callers' ranges and
//      some thousand more divisors (0 mismatches; tools/gpu_checks/divcheck.hip: 0 in 1e11 random pairs on the device).
// Range: b and rb normal (the callers' votes rcp_safe, rip_mid_range, rip_mid36 keep |b| inside 2^-59.8 .. 2^59.8); a = 0 or
// |a| in 2^-42 .. 2^66, so that the quotient and r0 (>= 2^-47 |a|) stay finite and normal under every voted b.  The previous form,
// which ran a second pair (r1, q2), carried the same conditions.
RIP_SF float rip_div_rcp1(float a, float b, float rb) {
    const float q0 = a * rb;
    const float r0 = fmaf(-b, q0, a);
    return fmaf(r0, rb, q0);
}

// ------------------------------------------------------------------------------------------------ hypotf
// (float)sqrt((double)a*a + (double)b*b) without the full f64 root.  T = RN(a^2 + b^2) is the reference's radicand (both
// products are exact in f64, the fma rounds once, as the reference's addition does).  rip_hypot_short refines an estimate
// y = (1 + e0) / sqrt(T) of the reciprocal root (v_rsq_f64: |e0| <= 2^-23; anything up to 2^-20 serves) by one coupled
// Goldschmidt step and one residual step:
//     g0 = T y, h0 = y/2, r = 1/2 - h0 g0 = -(e0 + e0^2/2) (+ 2^-53),   g1 = g0 + g0 r = sqrt(T) (1 + e1), |e1| <= 1.5 e0^2 + 2^-51
//     d = T - g1^2 = -T (2 e1 + e1^2) (1 + 2^-53),   g2 = g1 + d h0 = sqrt(T) (1 - e0 e1 + ...) rounded once more:
//     |g2 / sqrt(T) - 1| <= |e0 e1| + e1^2 + 2^-52 e1 + 2^-53 < 2^-52 for |e0| <= 2^-20.  BOUND USED: 2^-50, i.e. at most 8 steps
//     of the f64 g2; the reference's own root is within half a step of sqrt(T) more.
// (float)g2 equals the reference's (float)sqrt(T) when no f32 rounding midpoint lies within those 8.5 steps of g2: the low 29
// bits of g2 are then further than RIP_HYPOT_GUARD = 32 steps from 2^28.  (Beside a power of two both values round to it.)
// ok also wants T in 2^-120 .. 2^120 (root a normal f32; false for T = 0, Inf, NaN).  One lane in 2^23 is turned away.
#define RIP_HYPOT_GUARD 32u
RIP_SF double rip_hypot_radicand(float a, float b) {
    const double da = (double)a, db = (double)b;
    return fma(da, da, db * db);
}
RIP_SF float rip_hypot_short(double T, double y, bool &ok) {
    const double g0 = T * y, h0 = 0.5 * y;
    const double r = fma(-h0, g0, 0.5);
    const double g1 = fma(g0, r, g0);
    const double d = fma(-g1, g1, T);
    const double g2 = fma(d, h0, g1);
    uint64_t tb, gb;
    memcpy(&tb, &T, 8);
    memcpy(&gb, &g2, 8);
    const uint32_t th = (uint32_t)(tb >> 32);
    const uint32_t lo = (uint32_t)gb & 0x1fffffffu;
    const bool range = (th - 0x38700000u) < (0x47700000u - 0x38700000u);   // biased exponent of T in 1023 - 120 .. 1023 + 120
    const bool clear = (lo - (0x10000000u - RIP_HYPOT_GUARD)) > 2u * RIP_HYPOT_GUARD;
    ok = range && clear;
    return (float)g2;
}
