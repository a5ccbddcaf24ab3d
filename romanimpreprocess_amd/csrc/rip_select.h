// Order-preserving keys of f32 values and the exact selections built on them, for every kernel that takes a median or a rank
// (refpix.hip, refpix_one.hip, post.hip, stats.hip, darkstack.hip): the key, the three-level digit layout and the scan step of
// the histogram selections, and the per-pixel selection over a column of keys that four waves share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// monotone: key(a) < key(b) <=> a < b, with -0 just below +0; NaNs lie beyond the infinities on the side of their sign.
// (one compare, select and xor each way: key2f sits in the summing loops of darkstack.hip)
__device__ __forceinline__ uint32_t f2key(float f) {
    const uint32_t b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }
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

// ------------------------------------------------------------------------------------------ column selection
// One workgroup of four waves per 64 pixels: wave w holds the planes s = w (mod 4) of the column of n keys of pixel `lane`
// (key(s): from LDS as tile[s*64 + lane], conflict-free, or from memory).  The waves' partial results meet in a double-buffered
// LDS array; every wave leaves with the sum over the four, added in wave order, and so takes the same decisions.
struct ColMeet {
    uint4 (*xch)[4][64];   // __shared__ uint4 [2][4][64]
    int w, lane, buf;
    template <typename Add>
    __device__ __forceinline__ void operator()(uint4 mine, Add &&add) {
        xch[buf][w][lane] = mine;
        __syncthreads();
        for (int q = 0; q < 4; ++q) add(xch[buf][q][lane]);
        buf ^= 1;   // the other buffer is free: every wave has passed the barrier after reading it
    }
};

// Key of 0-based rank `rank` among the keys e of the column with in(e): radix selection, two bits a pass, 16 exchanges.
template <typename Key, typename In>
__device__ __forceinline__ uint32_t col_select(int n, int w, int rank, Key key, In in, ColMeet &meet) {
    int k = rank;
    uint32_t prefix = 0;
    for (int sh = 30; sh >= 0; sh -= 2) {
        const uint32_t hi = sh == 30 ? 0u : (0xFFFFFFFFu << (sh + 2));
        uint32_t c0 = 0, c1 = 0, c2 = 0;
#pragma unroll 8
        for (int s = w; s < n; s += 4) {
            const uint32_t e = key(s);
            const bool m = in(e) && (e & hi) == prefix;
            const uint32_t d = (e >> sh) & 3u;
            c0 += (m && d == 0) ? 1 : 0;
            c1 += (m && d <= 1) ? 1 : 0;
            c2 += (m && d <= 2) ? 1 : 0;
        }
        uint32_t t0 = 0, t1 = 0, t2 = 0;
        meet(make_uint4(c0, c1, c2, 0u), [&](const uint4 &v) {
            t0 += v.x;
            t1 += v.y;
            t2 += v.z;
        });
        uint32_t d;
        if (k < (int)t0) d = 0;
        else if (k < (int)t1) { d = 1; k -= t0; }
        else if (k < (int)t2) { d = 2; k -= t1; }
        else { d = 3; k -= t2; }
        prefix |= d << sh;
    }
    return prefix;
}

// The other middle key of an even count cnt of members, given `mid` = col_select at rank (cnt-1)/2: mid again (ties) or the
// next member above it.  One exchange.
template <typename Key, typename In>
__device__ __forceinline__ uint32_t col_select_upper(int n, int w, int cnt, uint32_t mid, Key key, In in, ColMeet &meet) {
    uint32_t le = 0, nxt = 0xFFFFFFFFu;
#pragma unroll 8
    for (int s = w; s < n; s += 4) {
        const uint32_t e = key(s);
        const bool m = in(e);
        le += (m && e <= mid) ? 1 : 0;
        if (m && e > mid && e < nxt) nxt = e;
    }
    uint32_t lt = 0, nt = 0xFFFFFFFFu;
    meet(make_uint4(le, nxt, 0u, 0u), [&](const uint4 &v) {
        lt += v.x;
        nt = min(nt, v.y);
    });
    return (int)lt >= cnt / 2 + 1 ? mid : nt;
}
