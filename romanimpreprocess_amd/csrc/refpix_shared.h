// The arithmetic the reference-pixel kernels share (refpix.hip, refpix_one.hip): order-preserving keys, the digit layout and the
// scan step of the exact radix selections, the median of a selected pair, the row correction and the channel line.
#pragma once
#include <stdint.h>

__device__ __forceinline__ uint32_t f2key(float f) {
    uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
    uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __uint_as_float(u);
}
// np.median of an even count from the keys of its two middle elements: their f32 mean
__device__ __forceinline__ float key_median(uint32_t lo, uint32_t hi) { return (key2f(lo) + key2f(hi)) * 0.5f; }

// three levels: 11 + 11 + 10 key bits, most significant first
#define SEL_BINS 2048
__device__ __forceinline__ int sel_shift(int level) { return level == 0 ? 21 : (level == 1 ? 10 : 0); }
__device__ __forceinline__ int sel_bits(int level) { return level == 2 ? 10 : 11; }

// One scan of a selection level: which of the SEL_BINS = THREADS x PER bins holds the key of rank `rank`.  Thread t owns bins
// t * PER .. t * PER + PER - 1 (count(k): the count of its bin k); wave prefix sums, the waves' totals through part[THREADS / 64]
// (LDS), then the owner walks its bins.  Returns true in the owner only, with the bin and the rank inside it.  Every thread of
// the workgroup calls; those of a larger workgroup that own no bins pass active = false.  Ends without a barrier.
template <int THREADS, int PER, typename Count>
__device__ __forceinline__ bool sel_find_bin(Count count, uint32_t rank, int t, bool active, uint32_t *part, uint32_t &bin,
                                             uint32_t &left) {
    static_assert(THREADS * PER == SEL_BINS, "one bin range per thread");
    const int lane = t & 63, w = t >> 6;
    uint32_t own = 0, incl = 0;
    if (active) {
#pragma unroll
        for (int k = 0; k < PER; ++k) own += count(k);
        incl = own;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)incl, off, 64);
            if (lane >= off) incl += y;
        }
        if (lane == 63) part[w] = incl;
    }
    __syncthreads();
    for (int k = 0; k < (active ? w : 0); ++k) incl += part[k];
    const uint32_t excl = incl - own;
    if (!active || !((excl <= rank && rank < incl) || (t == THREADS - 1 && rank >= incl))) return false;
    uint32_t cum = excl;
    int b = 0;
#pragma unroll
    for (int k = 0; k < PER - 1; ++k)
        if (b == k && cum + count(k) <= rank) cum += count(b++);
    bin = (uint32_t)(t * PER + b);
    left = rank - cum;
    return true;
}

// row correction of a row median v (reference_subtraction.py:115-123): slope * f64(f32(v - ctr)) for a numpy f64 slope; every
// operation f32 for an f32 slope (row_corr_f32, s32 = f32(slope))
__device__ __forceinline__ double row_corr(double slope, float v, float ctr) { return slope * (double)(v - ctr); }
__device__ __forceinline__ double row_corr_f32(float s32, float v, float ctr) { return (double)(s32 * (v - ctr)); }

// the line through (1.5, b), (ny - 2.5, t) (reference_subtraction.py:57-60), or the caller's (m, c) at ovr (LAPACK's: the
// reference fits it with gelsd, which agrees to ~1e-13 relative but not bit for bit; DESIGN.md "channel line fit")
__device__ __forceinline__ void chan_line(float b, float t, int ny, const double *ovr, double &m, double &c) {
    if (ovr) {
        m = ovr[0];
        c = ovr[1];
    } else {
        m = ((double)t - (double)b) / (double)(ny - 4);
        c = (double)b - 1.5 * m;
    }
}
