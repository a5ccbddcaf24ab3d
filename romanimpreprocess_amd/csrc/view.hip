// Quick-look pictures of a Level-1 cube (utils/visualize.py and utils/diff.py of the reference): a window of every group and its
// differences against one group, stretched by percentiles of the window.
//   visualize.py:58-59, 83-84, 97   np.percentile of the window (of a difference)        -> rip_view_ranks       (exact)
//   visualize.py:60-111             imshow(cmap, vmin, vmax | PowerNorm) + colour bars    -> rip_view_render      (linear exact)
//   diff.py:17                      data[g2] - data[g1] as float32                         -> rip_view_plane_diff  (exact)
// The cube (u16 or f32) is read where it lies; a sample's value is f32(sample), minus f32(sample of plane `minus`) at the same
// pixel where differencing is asked for -- data.astype(np.float32) - data[minus].  No f32 copy of the window is ever made.
#include <algorithm>
#include <cmath>

#include "rip_host.h"
#include "rip_select.h"
#include "rip_stamp.h"

namespace {

// the window: rows y0 .. y0 + h - 1, columns x0 .. x0 + w - 1 of the planes g0 .. g0 + ngw - 1; n = ngw * h * w samples (< 2^32)
struct VwWin {
    int ny, nx, y0, x0, h, w, g0, ngw, minus;
    uint32_t n;
};

template <typename T>
__device__ __forceinline__ float vw_value(const T *__restrict__ cube, const VwWin &q, int g, int y, int x) {
    const size_t at = (size_t)y * q.nx + x, plane = (size_t)q.ny * q.nx;
    const float v = (float)cube[(size_t)g * plane + at];
    return q.minus >= 0 ? v - (float)cube[(size_t)q.minus * plane + at] : v;
}

// ------------------------------------------------------------------------------------------ selection
// Exact order statistics of the window by three histogram levels over the order-preserving key (rip_select.h): each level
// reads the window once, per-workgroup LDS histograms are merged into HBM by integer atomics, one workgroup scans them
// (sel_find_bin) and extends the prefix of every requested rank.  Level 0 has one histogram (every rank starts with the empty
// prefix); from level 1 on every rank follows its own prefix, and ranks whose prefixes coincide share the histogram of the
// first of them (owner).  Integer counts only: the same bits each call.
#define VW_MAX_RANKS RIP_VIEW_MAX_RANKS
#define VW_PER 8                      // samples per thread and tile
#define VW_TILE (256 * VW_PER)

struct VwSel {
    uint32_t prefix[VW_MAX_RANKS];    // the key bits found so far
    uint32_t left[VW_MAX_RANKS];      // the rank among the samples that share them
    uint32_t owner[VW_MAX_RANKS];     // the first rank with the same prefix: its histogram is this rank's too
    float value[VW_MAX_RANKS];        // after level 2
    uint32_t nan;
};

// dynamic LDS: nslots histograms of SEL_BINS counts (nslots: 1 at level 0, nranks afterwards)
template <typename T>
__global__ __launch_bounds__(256) void view_hist_kernel(const T *__restrict__ cube, VwWin q, int nranks, int level, VwSel *sel,
                                                        uint32_t *__restrict__ ghist) {
    extern __shared__ uint32_t h[];
    const int t = threadIdx.x, nslots = level == 0 ? 1 : nranks;
    for (int i = t; i < nslots * SEL_BINS; i += 256) h[i] = 0;
    uint32_t pre[VW_MAX_RANKS];
    bool counted[VW_MAX_RANKS];
#pragma unroll
    for (int r = 0; r < VW_MAX_RANKS; ++r) {
        pre[r] = r < nranks ? sel->prefix[r] : 0u;
        counted[r] = r < nslots && sel->owner[r] == (uint32_t)r;
    }
    __syncthreads();
    const int shift = sel_shift(level), above = shift + sel_bits(level);
    const uint32_t mask = (1u << sel_bits(level)) - 1u;
    uint32_t nans = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * VW_TILE; base < q.n; base += (uint64_t)gridDim.x * VW_TILE) {
        float v[VW_PER];
#pragma unroll
        for (int k = 0; k < VW_PER; ++k) {   // the loads of a tile are in flight together; past the end: the last sample again
            const uint64_t j = base + (uint64_t)(k * 256 + t);
            const uint32_t i = (uint32_t)(j < q.n ? j : q.n - 1);
            const uint32_t row = i / (uint32_t)q.w, x = i - row * (uint32_t)q.w, g = row / (uint32_t)q.h, y = row - g * (uint32_t)q.h;
            v[k] = vw_value(cube, q, q.g0 + (int)g, q.y0 + (int)y, q.x0 + (int)x);
        }
#pragma unroll
        for (int k = 0; k < VW_PER; ++k) {
            if (base + (uint64_t)(k * 256 + t) >= q.n) continue;
            nans += v[k] != v[k] ? 1u : 0u;
            const uint32_t key = f2key(v[k]), bin = (key >> shift) & mask;
#pragma unroll
            for (int r = 0; r < VW_MAX_RANKS; ++r)
                if (counted[r] && (above >= 32 || ((key ^ pre[r]) >> above) == 0)) atomicAdd(&h[r * SEL_BINS + bin], 1u);
        }
    }
    if (level == 0) {   // the wave's count through one lane
        for (int off = 32; off > 0; off >>= 1) nans += (uint32_t)__shfl_down((int)nans, off, 64);
        if ((t & 63) == 0 && nans) atomicAdd(&sel->nan, nans);
    }
    __syncthreads();
    for (int i = t; i < nslots * SEL_BINS; i += 256)
        if (h[i]) atomicAdd(&ghist[i], h[i]);
}

// one workgroup: for every rank the bin of its histogram that holds it, the prefix extended by that bin, the rank rebased
__global__ __launch_bounds__(256) void view_scan_kernel(VwSel *sel, const uint32_t *__restrict__ ghist, int nranks, int level) {
    __shared__ uint32_t part[4], sp[VW_MAX_RANKS], sl[VW_MAX_RANKS];
    const int t = threadIdx.x;
    for (int r = 0; r < nranks; ++r) {
        const uint32_t *hh = ghist + (size_t)sel->owner[r] * SEL_BINS + t * 8;
        uint32_t c[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) c[k] = hh[k];
        uint32_t bin = 0, left = 0;
        if (sel_find_bin<256, 8>([&](int k) { return c[k]; }, sel->left[r], t, true, part, bin, left)) {
            sp[r] = sel->prefix[r] | (bin << sel_shift(level));
            sl[r] = left;
        }
        __syncthreads();   // part is used again; sp and sl are read below
    }
    if (t < nranks) {
        uint32_t own = (uint32_t)t;
        for (int o = t - 1; o >= 0; --o)
            if (sp[o] == sp[t]) own = (uint32_t)o;
        sel->prefix[t] = sp[t];
        sel->left[t] = sl[t];
        sel->owner[t] = own;
        if (level == 2) sel->value[t] = key2f(sp[t]);
    }
}

// ------------------------------------------------------------------------------------------ plane difference
template <typename T>
__global__ __launch_bounds__(256) void view_diff_kernel(const T *__restrict__ a, const T *__restrict__ b, size_t n, float *__restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = (float)b[i] - (float)a[i];
}

// ------------------------------------------------------------------------------------------ rendering
// A panel is a cell of (ch, cw) picture pixels whose first pixel is (y, x) of its table row; row 0 is the bottom row.  In the cell:
// the window magnified `zoom` times from (0, 0), H x W pixels; the colour bar in the columns bar_x .. bar_x + bar_w - 1 of the rows
// 0 .. H-1; its three ticks (one row high, `tick` columns) right of it at the rows 0, H / 2 and H - 1; the stamps anywhere.
struct VwLayout {
    int npanel, zoom, H, W, bar_x, bar_w, tick, ch, cw, NY, NX;
};
#define VW_PANEL_WORDS 6   // plane, minus, norm kind, y, x, colour bar
#define VW_LIMIT_WORDS 3   // vmin, vmax, gamma

// cmap(t, bytes=True) of a 256-entry table for a value that is not NaN: t * 256 truncated, below 0 -> 0, from 256 on -> 255
template <typename F>
__device__ __forceinline__ int vw_index(F t) {
    const F x = t * (F)256;
    return x < (F)0 ? 0 : (x >= (F)256 ? 255 : (int)x);
}

// One thread per pixel of the picture; every byte is stored once.
template <typename T>
__global__ __launch_bounds__(256) void view_render_kernel(const T *__restrict__ cube, VwWin q, VwLayout L, const int32_t *__restrict__ panels,
                                                          const float *__restrict__ limits, const uint8_t *__restrict__ table,
                                                          const uint8_t *__restrict__ glyphs, const int32_t *__restrict__ stamps,
                                                          const int32_t *__restrict__ stamp_at, uint8_t *__restrict__ out) {
    const int X = blockIdx.x * blockDim.x + threadIdx.x, Y = blockIdx.y;
    if (X >= L.NX) return;
    uint8_t r = 255, gch = 255, b = 255;   // the background is white
    for (int p = 0; p < L.npanel; ++p) {
        const int32_t *pn = panels + VW_PANEL_WORDS * p;
        const int y = Y - pn[3], x = X - pn[4];
        if (y < 0 || y >= L.ch || x < 0 || x >= L.cw) continue;
        int idx = -1;
        if (y < L.H && x < L.W) {
            const float lo = limits[VW_LIMIT_WORDS * p], hi = limits[VW_LIMIT_WORDS * p + 1];
            VwWin one = q;
            one.minus = pn[1];
            const float v = vw_value(cube, one, pn[0], q.y0 + y / L.zoom, q.x0 + x / L.zoom);
            if (lo == hi) {
                idx = 0;   // Normalize: result.fill(0), NaN samples too
            } else {
                float t = v - lo;
                if (pn[2] == 0) {
                    t = (float)((double)t / ((double)hi - (double)lo));   // Normalize: the quotient in f64, rounded once to f32
                } else {
                    t = t / (hi - lo);                                        // PowerNorm: all in f32
                    if (t > 0.0f) t = powf(t, limits[VW_LIMIT_WORDS * p + 2]);
                }
                if (t != t) r = gch = b = 255;   // the bad colour is transparent: the page
                else idx = vw_index(t);
            }
        } else if (pn[5] && y < L.H && x >= L.bar_x && x < L.bar_x + L.bar_w) {
            // np.linspace(0, 1, H): i * (1 / (H - 1)), the last one set to 1; H = 1: [0]
            idx = L.H == 1 ? 0 : (y == L.H - 1 ? 255 : vw_index((double)y * (1.0 / (double)(L.H - 1))));
        }
        if (idx >= 0) {
            r = table[3 * idx];
            gch = table[3 * idx + 1];
            b = table[3 * idx + 2];
        }
        if (pn[5]) {
            const int rows[3] = {0, L.H / 2, L.H - 1};
            for (int j = 0; j < 3; ++j) tick_over(rows[j], L.bar_x + L.bar_w, 1, L.tick, y, x, r, gch, b);
        }
        stamps_over(glyphs, stamps, stamp_at[p], stamp_at[p + 1], y, x, r, gch, b);
    }
    uint8_t *o = out + ((size_t)Y * L.NX + X) * 3;
    o[0] = r;
    o[1] = gch;
    o[2] = b;
}

// the refusals the three entries share: the cube and a window of it (y1, x1 inclusive)
int vw_check_cube(rip_ctx *ctx, const char *who, const void *cube, int dtype, int location, int ng, int ny, int nx) {
    if (!cube) return rip_fail(ctx, RIP_EINVAL, "%s: the cube is NULL", who);
    if (dtype != RIP_U16 && dtype != RIP_F32) return rip_fail(ctx, RIP_EINVAL, "%s: dtype %d is neither RIP_U16 nor RIP_F32", who, dtype);
    if (const int rc = rip_check_location(ctx, who, "cube_location", location)) return rc;
    if (ng < 1 || ny < 1 || nx < 1) return rip_fail(ctx, RIP_EINVAL, "%s: a cube of (%d, %d, %d)", who, ng, ny, nx);
    return RIP_OK;
}
int vw_check_window(rip_ctx *ctx, const char *who, int ny, int nx, int y0, int y1, int x0, int x1) {
    if (y0 < 0 || x0 < 0 || y1 < y0 || x1 < x0 || y1 >= ny || x1 >= nx)
        return rip_fail(ctx, RIP_EINVAL, "%s: the window rows %d..%d, columns %d..%d is empty or leaves the frame of (%d, %d)", who, y0, y1, x0,
                        x1, ny, nx);
    return RIP_OK;
}

}  // namespace

// ============================================================================================ C-ABI

int rip_view_ranks(rip_ctx *ctx, const void *cube, int dtype, int cube_location, int ng, int ny, int nx, int y0, int y1, int x0, int x1,
                   int g0, int g1, int minus, int nranks, const uint32_t *ranks, float *values, uint32_t *nan_count) {
    int rc;
    if ((rc = vw_check_cube(ctx, "view_ranks", cube, dtype, cube_location, ng, ny, nx)) ||
        (rc = vw_check_window(ctx, "view_ranks", ny, nx, y0, y1, x0, x1)))
        return rc;
    if (!ranks || !values || !nan_count) return rip_fail(ctx, RIP_EINVAL, "view_ranks: ranks, values or nan_count is NULL");
    if (g0 < 0 || g1 <= g0 || g1 > ng) return rip_fail(ctx, RIP_EINVAL, "view_ranks: the planes %d..%d are empty or leave the cube of %d", g0, g1, ng);
    if (minus < -1 || minus >= ng) return rip_fail(ctx, RIP_EINVAL, "view_ranks: minus %d is outside the cube of %d planes", minus, ng);
    if (nranks < 1 || nranks > VW_MAX_RANKS) return rip_fail(ctx, RIP_EINVAL, "view_ranks: %d ranks, outside 1..%d", nranks, VW_MAX_RANKS);
    const unsigned long long n = (unsigned long long)(g1 - g0) * (unsigned long long)(y1 - y0 + 1) * (unsigned long long)(x1 - x0 + 1);
    if (n >= (1ull << 32)) return rip_fail(ctx, RIP_EINVAL, "view_ranks: a window of %llu samples, 2^32 or more", n);
    for (int r = 0; r < nranks; ++r)
        if (ranks[r] >= n) return rip_fail(ctx, RIP_EINVAL, "view_ranks: rank %u is not below the %llu samples of the window", ranks[r], n);

    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const VwWin q{ny, nx, y0, x0, y1 - y0 + 1, x1 - x0 + 1, g0, g1 - g0, minus, (uint32_t)n};
    DevArg<char> c;
    DevBuf<VwSel> sel(ctx);
    DevBuf<uint32_t> hist(ctx);   // [level][rank][SEL_BINS]
    VwSel s{};
    for (int r = 0; r < nranks; ++r) s.left[r] = ranks[r];
    const size_t per_level = (size_t)VW_MAX_RANKS * SEL_BINS;
    if ((rc = c.in(ctx, (const char *)cube, (size_t)ng * ny * nx * dsize(dtype), cube_location)) || (rc = sel.upload(&s, 1)) ||
        (rc = hist.alloc(3 * per_level)))
        return rc;
    RIP_HIP(ctx, hipMemsetAsync(hist.p, 0, 3 * per_level * sizeof(uint32_t), ctx->stream));
    const unsigned blocks = (unsigned)std::min<unsigned long long>((n + VW_TILE - 1) / VW_TILE, 2048);
    for (int level = 0; level < 3; ++level) {
        const size_t lds = (size_t)(level == 0 ? 1 : nranks) * SEL_BINS * sizeof(uint32_t);
        uint32_t *gh = hist.p + level * per_level;
        if (dtype == RIP_U16) {
            if ((rc = with_lds(ctx, view_hist_kernel<uint16_t>, lds))) return rc;
            hipLaunchKernelGGL(view_hist_kernel<uint16_t>, dim3(blocks), dim3(256), lds, ctx->stream, (const uint16_t *)c.p, q, nranks, level,
                               sel.p, gh);
        } else {
            if ((rc = with_lds(ctx, view_hist_kernel<float>, lds))) return rc;
            hipLaunchKernelGGL(view_hist_kernel<float>, dim3(blocks), dim3(256), lds, ctx->stream, (const float *)c.p, q, nranks, level, sel.p,
                               gh);
        }
        RIP_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(view_scan_kernel, dim3(1), dim3(256), 0, ctx->stream, sel.p, gh, nranks, level);
        RIP_HIP(ctx, hipGetLastError());
    }
    if ((rc = sel.download(&s, 1)) || (rc = dev_sync(ctx))) return rc;   // s is this call's: read after the wait
    for (int r = 0; r < nranks; ++r) values[r] = s.value[r];
    *nan_count = s.nan;
    return RIP_OK;
}

int rip_view_plane_diff(rip_ctx *ctx, const void *cube, int dtype, int cube_location, int ng, int ny, int nx, int g1, int g2, float *out,
                        int out_location) {
    int rc;
    if ((rc = vw_check_cube(ctx, "view_plane_diff", cube, dtype, cube_location, ng, ny, nx)) ||
        (rc = rip_check_location(ctx, "view_plane_diff", "out_location", out_location)))
        return rc;
    if (!out) return rip_fail(ctx, RIP_EINVAL, "view_plane_diff: out is NULL");
    if (g1 < 0 || g1 >= ng || g2 < 0 || g2 >= ng)
        return rip_fail(ctx, RIP_EINVAL, "view_plane_diff: the planes %d and %d are not both inside the cube of %d", g1, g2, ng);
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)ny * nx, bytes = npix * dsize(dtype);
    DevArg<char> a, b;   // of a host cube only the two planes travel
    DevArg<float> o;
    if ((rc = a.in(ctx, (const char *)cube + (size_t)g1 * bytes, bytes, cube_location)) ||
        (rc = b.in(ctx, (const char *)cube + (size_t)g2 * bytes, bytes, cube_location)) || (rc = o.out(ctx, out, npix, out_location)))
        return rc;
    const unsigned blocks = (unsigned)std::min<size_t>((npix + 255) / 256, 65536);
    if (dtype == RIP_U16)
        hipLaunchKernelGGL(view_diff_kernel<uint16_t>, dim3(blocks), dim3(256), 0, ctx->stream, (const uint16_t *)a.p, (const uint16_t *)b.p, npix,
                           o.p);
    else
        hipLaunchKernelGGL(view_diff_kernel<float>, dim3(blocks), dim3(256), 0, ctx->stream, (const float *)a.p, (const float *)b.p, npix, o.p);
    RIP_HIP(ctx, hipGetLastError());
    if ((rc = o.download())) return rc;
    return dev_sync(ctx);
}

int rip_view_render(rip_ctx *ctx, const void *cube, int dtype, int cube_location, int ng, int ny, int nx, int y0, int y1, int x0, int x1,
                    int npanel, const int32_t *panels, const float *limits, int zoom, int bar_gap, int bar_w, int tick, int cell_h,
                    int cell_w, int pic_ny, int pic_nx, const uint8_t *table, const uint8_t *glyphs, int nstamps, const int32_t *stamps,
                    uint8_t *out, int out_location) {
    int rc;
    if ((rc = vw_check_cube(ctx, "view_render", cube, dtype, cube_location, ng, ny, nx)) ||
        (rc = rip_check_location(ctx, "view_render", "out_location", out_location)) ||
        (rc = vw_check_window(ctx, "view_render", ny, nx, y0, y1, x0, x1)))
        return rc;
    if (!panels || !limits || !table || !out) return rip_fail(ctx, RIP_EINVAL, "view_render: a NULL table or out (only glyphs and stamps may be)");
    if (npanel < 1 || nstamps < 0) return rip_fail(ctx, RIP_EINVAL, "view_render: %d panels, %d stamps", npanel, nstamps);
    if (nstamps > 0 && (!glyphs || !stamps)) return rip_fail(ctx, RIP_EINVAL, "view_render: %d stamps without a glyph table", nstamps);
    if (zoom < 1) return rip_fail(ctx, RIP_EINVAL, "view_render: zoom %d is below 1", zoom);
    const long H = (long)zoom * (y1 - y0 + 1), W = (long)zoom * (x1 - x0 + 1);
    if (pic_ny < 1 || pic_nx < 1 || pic_ny > 65535 || pic_nx > (1 << 24))
        return rip_fail(ctx, RIP_EINVAL, "view_render: a picture of (%d, %d) pixels is empty or too large", pic_ny, pic_nx);
    if (bar_gap < 0 || bar_w < 1 || tick < 0 || cell_h < H || cell_w < W || cell_h > pic_ny || cell_w > pic_nx)
        return rip_fail(ctx, RIP_EINVAL, "view_render: a cell of (%d, %d) with bar gap %d, bar width %d, tick %d does not hold the window of (%ld, %ld) or fit the picture", cell_h,
                        cell_w, bar_gap, bar_w, tick, H, W);
    for (int p = 0; p < npanel; ++p) {
        const int32_t *pn = panels + VW_PANEL_WORDS * p;
        const float lo = limits[VW_LIMIT_WORDS * p], hi = limits[VW_LIMIT_WORDS * p + 1], gamma = limits[VW_LIMIT_WORDS * p + 2];
        if (pn[0] < 0 || pn[0] >= ng || pn[1] < -1 || pn[1] >= ng)
            return rip_fail(ctx, RIP_EINVAL, "view_render: panel %d shows plane %d minus %d of a cube of %d", p, pn[0], pn[1], ng);
        if (pn[2] != 0 && pn[2] != 1) return rip_fail(ctx, RIP_EINVAL, "view_render: panel %d has the norm kind %d", p, pn[2]);
        if (!std::isfinite(lo) || !std::isfinite(hi) || lo > hi || (pn[2] == 1 && !(std::isfinite(gamma) && gamma > 0.0f)))
            return rip_fail(ctx, RIP_EINVAL, "view_render: panel %d has the colour range %g .. %g, gamma %g", p, lo, hi, gamma);
        if (pn[3] < 0 || pn[4] < 0 || (long)pn[3] + cell_h > pic_ny || (long)pn[4] + cell_w > pic_nx)
            return rip_fail(ctx, RIP_EINVAL, "view_render: panel %d at (%d, %d) reaches past the picture of (%d, %d)", p, pn[3], pn[4], pic_ny,
                            pic_nx);
        if (pn[5] && W + bar_gap + bar_w + tick > cell_w)
            return rip_fail(ctx, RIP_EINVAL, "view_render: the colour bar of panel %d does not fit its cell of %d columns", p, cell_w);
    }
    std::vector<int32_t> at, sorted;
    if ((rc = rip_stamp_table(ctx, "view_render", nstamps, stamps, npanel, cell_h, cell_w, at, sorted))) return rc;

    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const VwWin q{ny, nx, y0, x0, y1 - y0 + 1, x1 - x0 + 1, 0, ng, -1, 0u};
    const VwLayout L{npanel, zoom, (int)H, (int)W, (int)W + bar_gap, bar_w, tick, cell_h, cell_w, pic_ny, pic_nx};
    DevArg<char> c;
    DevArg<uint8_t> o;
    DevBuf<int32_t> dpan(ctx), dst(ctx), dat(ctx);
    DevBuf<float> dlim(ctx);
    DevBuf<uint8_t> dtab(ctx), dgl(ctx);
    if ((rc = c.in(ctx, (const char *)cube, (size_t)ng * ny * nx * dsize(dtype), cube_location)) ||
        (rc = dpan.upload(panels, (size_t)npanel * VW_PANEL_WORDS)) || (rc = dlim.upload(limits, (size_t)npanel * VW_LIMIT_WORDS)) ||
        (rc = dtab.upload(table, 768)) || (rc = nstamps ? dst.upload(sorted.data(), sorted.size()) : dst.alloc(1)) ||
        (rc = dat.upload(at.data(), at.size())))
        return rc;
    if (glyphs && (rc = dgl.upload(glyphs, 256 * RIP_GLYPH_H * RIP_GLYPH_W))) return rc;
    if ((rc = o.out(ctx, out, (size_t)pic_ny * pic_nx * 3, out_location))) return rc;
    const dim3 grid((pic_nx + 255) / 256, pic_ny);
    if (dtype == RIP_U16)
        hipLaunchKernelGGL(view_render_kernel<uint16_t>, grid, dim3(256), 0, ctx->stream, (const uint16_t *)c.p, q, L, dpan.p, dlim.p, dtab.p,
                           dgl.p, dst.p, dat.p, o.p);
    else
        hipLaunchKernelGGL(view_render_kernel<float>, grid, dim3(256), 0, ctx->stream, (const float *)c.p, q, L, dpan.p, dlim.p, dtab.p, dgl.p,
                           dst.p, dat.p, o.p);
    RIP_HIP(ctx, hipGetLastError());
    if ((rc = o.download())) return rc;
    return dev_sync(ctx);   // the tables above are host vectors of this call: their copies are done before it returns
}
