// What the store-only picture kernels (fpaplot.hip, view.hip) draw over their colour-mapped pixels, stated once: the letters of
// write_text (utils/fpaplot.py:150-182 of the reference) as glyph stamps, and ticks.  A picture kernel has one thread per pixel;
// the thread asks these whether a stamp or a tick covers its pixel (y, x) -- coordinates inside its panel, row 0 at the bottom --
// and stores the last colour it met.  Device code only; the host's checks of a stamp list are rip_stamp_table (rip_host.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RIP_GLYPH_H 12
#define RIP_GLYPH_W 6
#define RIP_STAMP_WORDS 6   // panel, y, x, size, value, character

// does the stamp st cover the pixel?  Glyph rows are stored top first, every glyph cell is size x size pixels, and only the
// cells > 0 are drawn.
__device__ __forceinline__ bool stamp_covers(const uint8_t *__restrict__ glyphs, const int32_t *__restrict__ st, int y, int x) {
    const int size = st[3], yy = y - st[1], xx = x - st[2];
    if (yy < 0 || yy >= RIP_GLYPH_H * size || xx < 0 || xx >= RIP_GLYPH_W * size) return false;
    return glyphs[(st[5] * RIP_GLYPH_H + RIP_GLYPH_H - 1 - yy / size) * RIP_GLYPH_W + xx / size] > 0;
}

// the stamps first .. last-1 in list order: a later one overwrites an earlier one; all three channels take the stamp's value
__device__ __forceinline__ void stamps_over(const uint8_t *__restrict__ glyphs, const int32_t *__restrict__ stamps, int first, int last,
                                            int y, int x, uint8_t &r, uint8_t &g, uint8_t &b) {
    for (int i = first; i < last; ++i) {
        const int32_t *st = stamps + RIP_STAMP_WORDS * i;
        if (stamp_covers(glyphs, st, y, x)) r = g = b = (uint8_t)st[4];
    }
}

// a tick: the black rectangle of h rows and w columns whose first pixel is (ty, tx)
__device__ __forceinline__ void tick_over(int ty, int tx, int h, int w, int y, int x, uint8_t &r, uint8_t &g, uint8_t &b) {
    if (y >= ty && y < ty + h && x >= tx && x < tx + w) r = g = b = 0;
}
