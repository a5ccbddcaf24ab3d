// The growth rule of maskhandling.CombinedMask.build (maskhandling.py:82-117), stated once for mask_build_kernel (post.hip) and
// fpa_bin_kernel (fpaplot.hip): the layer of a dq bit is grown by its kernel -- 1 = copy, 5 = plus, 9 = 3x3, 25 = 5x5, zero
// padded at the frame edge (scipy.signal.convolve mode="same").
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

struct GrowMasks {   // the dq bits of each growth
    uint32_t m1, m5, m9, m25;
};

// What the dq words of one row contribute to a pixel `ady` rows away (0, 1 or 2): w0 is the word in the pixel's own column, w1 the
// OR of the two words one column away, w2 of the two words two columns away (0 for a word outside the frame).  A flagged pixel
// (ay, ax) away reaches this one through the bits grown to 25 always, to 9 where max(ay, ax) <= 1, to 5 where ay + ax <= 1, and
// through every masked bit where it is the pixel itself.  Non-zero: masked.
__device__ __forceinline__ uint32_t grow_row(const GrowMasks &g, int ady, uint32_t w0, uint32_t w1, uint32_t w2) {
    const uint32_t far = g.m25, box = g.m25 | g.m9, plus = g.m25 | g.m9 | g.m5;
    if (ady == 0) return (w0 & (plus | g.m1)) | (w1 & plus) | (w2 & far);
    if (ady == 1) return (w0 & plus) | (w1 & box) | (w2 & far);
    return (w0 | w1 | w2) & far;
}

// grow[32] of the interface into the four bit sets; the offending bit where a growth is not one of 0, 1, 5, 9, 25, else -1
inline int grow_masks(const uint8_t grow[32], GrowMasks *g) {
    *g = GrowMasks{0, 0, 0, 0};
    for (int b = 0; b < 32; ++b) {
        const uint32_t bit = 1u << b;
        switch (grow[b]) {
            case 0: break;
            case 1: g->m1 |= bit; break;
            case 5: g->m5 |= bit; break;
            case 9: g->m9 |= bit; break;
            case 25: g->m25 |= bit; break;
            default: return b;
        }
    }
    return -1;
}
