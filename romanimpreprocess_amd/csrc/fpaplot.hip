// Focal-plane overview of a calibration set (utils/fpaplot.py of the reference): the quality-assurance picture of the
// calibration-file workflow.
//   fpaplot.py:131-141   pad, grow the mask, masked nanmean over (nside / n1)^2 blocks    -> rip_fpa_bin     (f64 sums; order differs)
//   fpaplot.py:223-275   make_big_image: colour-mapped SCAs, colour bar, ticks, text     -> rip_fpa_render  (exact)
//   fpaplot.py:345-358   multi_image: the panels two abreast                                 (the same launch)
// The reference rebuilds the grown mask for each of its 8 quantities; here one launch reads dq once, grows the mask in LDS and
// bins all planes of the SCA under it.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "rip_grow.h"
#include "rip_host.h"
#include "rip_stamp.h"

namespace {

// ------------------------------------------------------------------------------------------ binning
// One workgroup per tile of FB_TH x FB_TW frame pixels, one wave per 8 of its rows, one lane per column.  The dq words of the tile
// with a 2-pixel halo are staged in LDS (zero outside the frame) and every lane keeps the grown mask of its 8 pixels in a register.
// Per plane: (1) a lane adds its counted pixels from top to bottom until the bin row or its 8 rows end -- a "piece"; (2) the wave
// adds the pieces of the lanes of one bin column in a fixed binary tree over the lanes (fb_segment_sum) and leaves (sum, count) in
// LDS; (3) one thread per bin of the tile adds the pieces of the bin from top to bottom.  A bin that lies inside one tile is
// finished there; otherwise the tile leaves (sum, count) of its part in `part` and fpa_finish_kernel adds the parts in tile order.
// Every sum has one fixed order: no atomics, the same bits each call.  Nothing here assumes a size of the bin: s = 1 makes every
// pixel a piece, s = nside one bin of every tile.
#define FB_TH 32
#define FB_TW 64   // the wave: a lane per column
#define FB_ROWS 8  // rows per wave
#define FB_HALO 2
#define FB_DW (FB_TW + 2 * FB_HALO)
#define FB_DH (FB_TH + 2 * FB_HALO)
static_assert(FB_TH == 4 * FB_ROWS && FB_TW == 64, "four waves of 64 lanes cover the tile");

struct FbPlanes {
    const void *data[RIP_FPA_MAX_PLANES];
    int f64[RIP_FPA_MAX_PLANES];
    int side[RIP_FPA_MAX_PLANES];
};

struct FbPart {
    double sum;
    long long count;
};

// The FB_ROWS values of plane i in column x from row y on, as doubles.  Every load is unconditional, from an address clamped into
// the plane, and selected afterwards, so that the loads of a lane are in flight together; outside the plane the value is 0
// (np.pad).
template <typename T>
__device__ __forceinline__ void fb_rows(const T *__restrict__ base, int m, int pad, int y, int x, double v[FB_ROWS]) {
    const int px = x - pad, cx = min(max(px, 0), m - 1);
    T raw[FB_ROWS];
#pragma unroll
    for (int k = 0; k < FB_ROWS; ++k) raw[k] = base[(size_t)min(max(y + k - pad, 0), m - 1) * m + cx];
#pragma unroll
    for (int k = 0; k < FB_ROWS; ++k) {
        const int py = y + k - pad;
        v[k] = (px >= 0 && px < m && py >= 0 && py < m) ? (double)raw[k] : 0.0;
    }
}

// The lanes a .. b-1 of the wave form one segment (this lane is `rel` lanes from a): afterwards lane a holds the sum of the
// segment, added in the binary tree that pairs lanes 2^k apart -- the same tree whatever the values.  Every lane of the wave
// calls it; `steps` (wave-uniform) bounds the longest segment: 2^steps >= its length.
__device__ __forceinline__ void fb_segment_sum(double &sum, int &cnt, int lane, int rel, int b, int steps) {
    for (int k = 0, d = 1; k < steps; ++k, d <<= 1) {
        const double os = __shfl_down(sum, d);
        const int oc = __shfl_down(cnt, d);
        if ((rel & (2 * d - 1)) == 0 && lane + d < b) {
            sum = sum + os;
            cnt += oc;
        }
    }
}

// direct: every bin lies inside one tile (s divides FB_TH and FB_TW); then part is not used.  fstride: bin columns a tile can touch;
// dynamic LDS: for each of the `group` planes between two barriers FB_TH * fstride sums, then as many counts: one (sum, count) per
// piece and bin column
__global__ __launch_bounds__(256) void fpa_bin_kernel(const uint32_t *__restrict__ dq, GrowMasks g, FbPlanes pl, int nplanes, int nside,
                                                      int n1, int s, int direct, int fmax, int fstride, int steps, int group,
                                                      FbPart *__restrict__ part, double *__restrict__ out) {
    __shared__ uint32_t sdq[FB_DH * FB_DW];
    extern __shared__ double dyn[];
    const int nslot = FB_TH * fstride;
    double *const ssum = dyn;                          // [group][nslot]
    int *const scnt = (int *)(dyn + group * nslot);    // [group][nslot]
    const int t = threadIdx.x, tx = t % FB_TW, r0 = t / FB_TW * FB_ROWS;
    const int x0 = blockIdx.x * FB_TW, y0 = blockIdx.y * FB_TH;
    const int w = min(FB_TW, nside - x0), h = min(FB_TH, nside - y0);   // the tile's part of the frame
    const int x = x0 + tx;

    uint32_t masked = 0;   // bit k: the pixel of row r0 + k is masked
    if (dq) {
        constexpr int NST = (FB_DH * FB_DW + 255) / 256;
        uint32_t word[NST];   // unconditional loads from clamped addresses, selected afterwards: in flight together
#pragma unroll
        for (int j = 0; j < NST; ++j) {
            const int i = min(t + 256 * j, FB_DH * FB_DW - 1), yy = y0 - FB_HALO + i / FB_DW, xx = x0 - FB_HALO + i % FB_DW;
            word[j] = dq[(size_t)min(max(yy, 0), nside - 1) * nside + min(max(xx, 0), nside - 1)];
        }
#pragma unroll
        for (int j = 0; j < NST; ++j) {
            const int i = t + 256 * j, yy = y0 - FB_HALO + i / FB_DW, xx = x0 - FB_HALO + i % FB_DW;
            if (i < FB_DH * FB_DW) sdq[i] = (yy >= 0 && yy < nside && xx >= 0 && xx < nside) ? word[j] : 0u;
        }
        __syncthreads();
        // the 12 staged rows around this lane's 8 pixels, each read once: row j lies j - 2 rows from pixel 0
#pragma unroll
        for (int j = 0; j < FB_ROWS + 2 * FB_HALO; ++j) {
            const uint32_t *row = sdq + (r0 + j) * FB_DW + tx + FB_HALO;
            const uint32_t w0 = row[0], w1 = row[-1] | row[1], w2 = row[-2] | row[2];
#pragma unroll
            for (int ady = 0; ady <= 2; ++ady) {
                const uint32_t m = grow_row(g, ady, w0, w1, w2);
                const int ka = j - FB_HALO - ady, kb = j - FB_HALO + ady;   // the pixels ady rows from row j
                if (ka >= 0 && ka < FB_ROWS) masked |= (m ? 1u : 0u) << ka;
                if (ady && kb >= 0 && kb < FB_ROWS) masked |= (m ? 1u : 0u) << kb;
            }
        }
    }

    const int bx0 = x0 / s, by0 = y0 / s;                                     // the first bin of the tile
    const int nbc = (x0 + w - 1) / s - bx0 + 1, nbr = (y0 + h - 1) / s - by0 + 1;   // bins that the tile touches
    const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    // this lane's segment of the wave: the lanes of its bin column inside the tile
    const int bc = min(x, nside - 1) / s - bx0;
    const int seg_a = max((bx0 + bc) * s, x0) - x0, seg_b = min((bx0 + bc + 1) * s, x0 + w) - x0;
    const int rel = tx - seg_a;
    for (int p0 = 0; p0 < nplanes; p0 += group) {
        const int ng = min(group, nplanes - p0);
        // (1) + (2): the pieces of this wave's rows; every condition on r is the same for the whole wave
        for (int q = 0; q < ng; ++q) {
            double *const bsum = ssum + q * nslot;
            int *const bcnt = scnt + q * nslot;
            double v[FB_ROWS];
            const int m = pl.side[p0 + q], pad = (nside - m) / 2;
            if (pl.f64[p0 + q])
                fb_rows((const double *)pl.data[p0 + q], m, pad, y0 + r0, x, v);
            else
                fb_rows((const float *)pl.data[p0 + q], m, pad, y0 + r0, x, v);
#pragma unroll
            for (int k = 0; k < FB_ROWS; ++k)   // NaN: not counted
                if (tx >= w || r0 + k >= h || ((masked >> k) & 1u)) v[k] = NAN;
            double sum = 0.0;
            int cnt = 0, first = r0, left = s - (y0 + r0) % s;   // left: rows to the end of the bin row
#pragma unroll
            for (int k = 0; k < FB_ROWS; ++k) {
                const int r = r0 + k;
                if (r >= h) break;
                if (v[k] == v[k]) {
                    sum = sum + v[k];
                    ++cnt;
                }
                if (k == FB_ROWS - 1 || r == h - 1 || --left == 0) {   // the piece ends with this row
                    fb_segment_sum(sum, cnt, tx, rel, seg_b, steps);
                    if (rel == 0 && tx < w) {
                        bsum[first * fstride + bc] = sum;
                        bcnt[first * fstride + bc] = cnt;
                    }
                    sum = 0.0;
                    cnt = 0;
                    first = r + 1;
                    left = left ? left : s;
                }
            }
        }
        __syncthreads();
        // (3) the pieces of each bin, top to bottom: a piece starts with the bin row and at every FB_ROWS-th row of the tile
        for (int i = t; i < ng * nbr * nbc; i += 256) {
            const int q = i / (nbr * nbc), j = i - q * (nbr * nbc), br = j / nbc, c = j - br * nbc;
            const int ya = max((by0 + br) * s, y0) - y0, yb = min((by0 + br + 1) * s, y0 + h) - y0;
            double bs = 0.0;
            long long bn = 0;
            for (int r = ya; r < yb; r = (r / FB_ROWS + 1) * FB_ROWS) {
                bs = bs + ssum[q * nslot + r * fstride + c];
                bn += scnt[q * nslot + r * fstride + c];
            }
            if (direct)
                out[((size_t)(p0 + q) * n1 + by0 + br) * n1 + bx0 + c] = bs / (double)bn;   // 0 / 0 = NaN: nothing counted
            else
                part[(tile * fmax + (size_t)br * fstride + c) * nplanes + p0 + q] = FbPart{bs, bn};
        }
        if (p0 + group < nplanes) __syncthreads();   // the next planes overwrite the pieces
    }
}

// One workgroup per (bin, plane): thread t adds the parts of the tiles t, t + 256, ... of the bin in tile order, the 256 sums are
// then added pairwise in a fixed tree.
__global__ __launch_bounds__(256) void fpa_finish_kernel(const FbPart *__restrict__ part, int nplanes, int nside, int n1, int s, int ntx,
                                                         int fmax, int fstride, double *__restrict__ out) {
    __shared__ double rs[256];
    __shared__ long long rc[256];
    const int bin = blockIdx.x, p = blockIdx.y, by = bin / n1, bx = bin % n1;
    const int tx0 = bx * s / FB_TW, tx1 = ((bx + 1) * s - 1) / FB_TW, ty0 = by * s / FB_TH, ty1 = ((by + 1) * s - 1) / FB_TH;
    const int nx = tx1 - tx0 + 1, n = nx * (ty1 - ty0 + 1);
    double sum = 0.0;
    long long cnt = 0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int tyy = ty0 + i / nx, txx = tx0 + i % nx;
        const int br = by - tyy * FB_TH / s, bc = bx - txx * FB_TW / s;
        const FbPart q = part[(((size_t)tyy * ntx + txx) * fmax + (size_t)br * fstride + bc) * nplanes + p];
        sum = sum + q.sum;
        cnt += q.count;
    }
    rs[threadIdx.x] = sum;
    rc[threadIdx.x] = cnt;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) {
            rs[threadIdx.x] = rs[threadIdx.x] + rs[threadIdx.x + k];
            rc[threadIdx.x] += rc[threadIdx.x + k];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[((size_t)p * n1 + by) * n1 + bx] = rs[0] / (double)rc[0];
}

// ------------------------------------------------------------------------------------------ rendering
struct FrLayout {
    int n1, nsca, npanel, nw, gap, ny, nx, sc, nstamps, NY, NX;
};

// cmap(x, bytes=True) of a 256-entry table
__device__ __forceinline__ int fr_index(double x) {
    const int i = (int)(x * 256.0);
    return i > 255 ? 255 : i;
}

// One thread per pixel of the picture; it walks the layers in the reference's order and stores the last colour it met.
// stamp_at[p] .. stamp_at[p + 1]: the stamps of panel p in list order.
__global__ __launch_bounds__(256) void fpa_render_kernel(FrLayout L, const double *__restrict__ maps, const uint8_t *__restrict__ present,
                                                         const int32_t *__restrict__ sca_pos, const double *__restrict__ vmin,
                                                         const double *__restrict__ vmax, const uint8_t *__restrict__ scale,
                                                         const uint8_t *__restrict__ table, const uint8_t *__restrict__ glyphs,
                                                         const int32_t *__restrict__ stamps, const int32_t *__restrict__ stamp_at,
                                                         uint8_t *__restrict__ out) {
    const int X = blockIdx.x * blockDim.x + threadIdx.x, Y = blockIdx.y;
    if (X >= L.NX) return;
    uint8_t r = 255, gch = 255, b = 255;   // the background is white
    const int pc = X / (L.nx + L.gap), pr = Y / (L.ny + L.gap);
    const int x = X - pc * (L.nx + L.gap), y = Y - pr * (L.ny + L.gap);
    const int panel = pr * L.nw + pc;
    if (x < L.nx && y < L.ny && panel < L.npanel) {
        const double lo = vmin[panel], hi = vmax[panel];
        int idx = -1;
        for (int k = 0; k < L.nsca; ++k) {   // the later SCA wins
            const int yy = y - sca_pos[2 * k], xx = x - sca_pos[2 * k + 1];
            if (yy < 0 || yy >= L.n1 || xx < 0 || xx >= L.n1) continue;
            double v = 0.0;
            if (present[panel * L.nsca + k]) v = maps[(((size_t)panel * L.nsca + k) * L.n1 + yy) * L.n1 + xx];
            if (v != v) v = 0.0;   // nan_to_num
            else if (v > DBL_MAX) v = DBL_MAX;
            else if (v < -DBL_MAX) v = -DBL_MAX;
            double q = (v - lo) / (hi - lo);
            q = q < 0.0 ? 0.0 : (q > 1.0 ? 1.0 : q);   // np.clip; never NaN: v is finite and vmax - vmin is not 0
            idx = fr_index(q);
        }
        if (scale[panel]) {
            const int bh = L.n1 / 8, xb = x - (L.nx / 2 - L.n1);
            // np.linspace(0, 1, 2 n1): i * (1 / (2 n1 - 1)), the last one set to 1
            if (y >= L.ny - bh && xb >= 0 && xb < 2 * L.n1)
                idx = xb == 2 * L.n1 - 1 ? 255 : fr_index((double)xb * (1.0 / (double)(2 * L.n1 - 1)));
            if (idx >= 0) {
                r = table[3 * idx];
                gch = table[3 * idx + 1];
                b = table[3 * idx + 2];
            }
            for (int j = 0; j < 3; ++j) tick_over(L.ny - bh - 2 * L.sc, L.nx / 2 - L.n1 + j * L.n1, 2 * L.sc, L.sc, y, x, r, gch, b);
        } else if (idx >= 0) {
            r = table[3 * idx];
            gch = table[3 * idx + 1];
            b = table[3 * idx + 2];
        }
        stamps_over(glyphs, stamps, stamp_at[panel], stamp_at[panel + 1], y, x, r, gch, b);
    }
    uint8_t *o = out + ((size_t)Y * L.NX + X) * 3;
    o[0] = r;
    o[1] = gch;
    o[2] = b;
}

}  // namespace

// ============================================================================================ C-ABI

int rip_fpa_bin(rip_ctx *ctx, const uint32_t *dq, int dq_location, const uint8_t grow[32], int nside, int n1, int nplanes,
                const void **planes, const int *dtypes, const int *sides, const int *locations, double *out, int out_location) {
    if (!grow || !planes || !dtypes || !sides || !locations || !out) return rip_fail(ctx, RIP_EINVAL, "fpa_bin: a NULL table, grow or out");
    if (nside < 1 || n1 < 1 || (n1 & (n1 - 1)) || nside % n1)
        return rip_fail(ctx, RIP_EINVAL, "fpa_bin: n1 %d is not a power of two that divides nside %d", n1, nside);
    if (nplanes < 1 || nplanes > RIP_FPA_MAX_PLANES)
        return rip_fail(ctx, RIP_EINVAL, "fpa_bin: %d planes, outside 1..%d", nplanes, RIP_FPA_MAX_PLANES);
    int rc;
    if ((rc = rip_check_location(ctx, "fpa_bin", "dq_location", dq_location)) ||
        (rc = rip_check_location(ctx, "fpa_bin", "out_location", out_location)))
        return rc;
    for (int i = 0; i < nplanes; ++i) {
        if (!planes[i]) return rip_fail(ctx, RIP_EINVAL, "fpa_bin: plane %d is NULL", i);
        if (dtypes[i] != RIP_F32 && dtypes[i] != RIP_F64)
            return rip_fail(ctx, RIP_EINVAL, "fpa_bin: plane %d has dtype %d, neither RIP_F32 nor RIP_F64", i, dtypes[i]);
        if (!rip_is_location(locations[i])) return rip_fail(ctx, RIP_EINVAL, "fpa_bin: plane %d has the location %d", i, locations[i]);
        const int m = sides[i];
        if (m < 1 || m > nside) return rip_fail(ctx, RIP_EINVAL, "fpa_bin: plane %d of side %d does not fit the frame of side %d", i, m, nside);
        if ((nside - m) % 2)
            return rip_fail(ctx, RIP_EINVAL, "fpa_bin: plane %d of side %d cannot be centred in the frame of side %d (odd difference)", i, m,
                            nside);
    }
    GrowMasks g;
    const int bad = grow_masks(grow, &g);
    if (bad >= 0) return rip_fail(ctx, RIP_EINVAL, "fpa_bin: growth %d of bit %d is not one of 0, 1, 5, 9, 25", grow[bad], bad);

    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const int s = nside / n1;
    const size_t npix = (size_t)nside * nside, nout = (size_t)nplanes * n1 * n1;
    const int ntx = (nside + FB_TW - 1) / FB_TW, nty = (nside + FB_TH - 1) / FB_TH;
    if (nty > 65535) return rip_fail(ctx, RIP_EINVAL, "fpa_bin: a frame of side %d is too large", nside);
    const int direct = (FB_TH % s == 0 && FB_TW % s == 0) ? 1 : 0;
    const int fstride = (FB_TW - 1) / s + 2, fmax = ((FB_TH - 1) / s + 2) * fstride;   // the most bins a tile can touch
    DevArg<uint32_t> q;
    DevArg<char> dpl[RIP_FPA_MAX_PLANES];
    DevBuf<FbPart> part(ctx);
    DevArg<double> o;
    if ((rc = q.in(ctx, dq, npix, dq_location))) return rc;
    FbPlanes pl{};
    for (int i = 0; i < nplanes; ++i) {
        pl.f64[i] = dtypes[i] == RIP_F64;
        pl.side[i] = sides[i];
        if ((rc = dpl[i].in(ctx, (const char *)planes[i], (size_t)pl.side[i] * pl.side[i] * dsize(dtypes[i]), locations[i]))) return rc;
        pl.data[i] = dpl[i].p;
    }
    if (!direct && (rc = part.alloc((size_t)ntx * nty * fmax * nplanes))) return rc;
    if ((rc = o.out(ctx, out, nout, out_location))) return rc;
    int steps = 0;   // 2^steps >= the longest run of lanes in one bin column
    while ((1 << steps) < (s < FB_TW ? s : FB_TW)) ++steps;
    // as many planes between two barriers as 32 KB of LDS hold: all 8 from s = 8 on, one at s = 1
    const size_t per_plane = (size_t)FB_TH * fstride * (sizeof(double) + sizeof(int));
    const int group = (int)std::max<size_t>(1, std::min<size_t>(nplanes, 32768 / per_plane));
    const size_t lds = group * per_plane;
    if ((rc = with_lds(ctx, fpa_bin_kernel, lds))) return rc;
    hipLaunchKernelGGL(fpa_bin_kernel, dim3(ntx, nty), dim3(256), lds, ctx->stream, q.p, g, pl, nplanes, nside, n1, s, direct, fmax, fstride,
                       steps, group, part.p, o.p);
    RIP_HIP(ctx, hipGetLastError());
    if (!direct) {
        hipLaunchKernelGGL(fpa_finish_kernel, dim3(n1 * n1, nplanes), dim3(256), 0, ctx->stream, part.p, nplanes, nside, n1, s, ntx, fmax,
                           fstride, o.p);
        RIP_HIP(ctx, hipGetLastError());
    }
    if ((rc = o.download())) return rc;
    return dev_sync(ctx);
}

int rip_fpa_render(rip_ctx *ctx, int n1, int nsca, int npanel, int nw, int gap, int ny, int nx, const double *maps, int maps_location,
                   const uint8_t *present, const int32_t *sca_pos, const double *vmin, const double *vmax, const uint8_t *scale,
                   const uint8_t *table, const uint8_t *glyphs, int nstamps, const int32_t *stamps, uint8_t *out, int out_location) {
    if (!maps || !present || !sca_pos || !vmin || !vmax || !scale || !table || !out)
        return rip_fail(ctx, RIP_EINVAL, "fpa_render: a NULL argument (only glyphs and stamps may be)");
    const struct {
        int n1, nsca, npanel, nw, gap, ny, nx, sc, nstamps;
    } l{n1, nsca, npanel, nw, gap, ny, nx, (n1 > 64 ? n1 : 64) / 64, nstamps};
    if (l.n1 < 1 || l.nsca < 1 || l.npanel < 1 || l.nw < 1 || l.gap < 0 || l.ny < 1 || l.nx < 1 || l.sc < 1 || l.nstamps < 0)
        return rip_fail(ctx, RIP_EINVAL, "fpa_render: a count or size of the layout is below 1");
    int rc;
    if ((rc = rip_check_location(ctx, "fpa_render", "maps_location", maps_location)) ||
        (rc = rip_check_location(ctx, "fpa_render", "out_location", out_location)))
        return rc;
    if (l.nstamps > 0 && (!glyphs || !stamps)) return rip_fail(ctx, RIP_EINVAL, "fpa_render: %d stamps without a glyph table", l.nstamps);
    for (int k = 0; k < l.nsca; ++k) {
        const int py = sca_pos[2 * k], px = sca_pos[2 * k + 1];
        if (py < 0 || px < 0 || py >= l.ny || px >= l.nx)
            return rip_fail(ctx, RIP_EINVAL, "fpa_render: SCA %d starts outside the image, at (%d, %d) of (%d, %d)", k + 1, py, px, l.ny, l.nx);
        if (py + l.n1 > l.ny || px + l.n1 > l.nx)
            return rip_fail(ctx, RIP_EINVAL, "fpa_render: SCA %d at (%d, %d) reaches past the image of (%d, %d)", k + 1, py, px, l.ny, l.nx);
    }
    for (int p = 0; p < l.npanel; ++p) {
        if (!std::isfinite(vmin[p]) || !std::isfinite(vmax[p]) || vmin[p] == vmax[p])
            return rip_fail(ctx, RIP_EINVAL, "fpa_render: panel %d has the colour range %g .. %g", p, vmin[p], vmax[p]);
        if (!scale[p]) continue;
        if (l.n1 < 8) return rip_fail(ctx, RIP_EINVAL, "fpa_render: a scale needs n1 >= 8, got %d", l.n1);
        if (l.nx / 2 - l.n1 < 0 || l.nx / 2 + l.n1 > l.nx || l.n1 / 8 + 2 * l.sc > l.ny || l.nx / 2 + l.n1 + l.sc > l.nx)
            return rip_fail(ctx, RIP_EINVAL, "fpa_render: the scale of n1 %d does not fit the panel of (%d, %d)", l.n1, l.ny, l.nx);
    }
    std::vector<int32_t> at, sorted;
    if ((rc = rip_stamp_table(ctx, "fpa_render", l.nstamps, stamps, l.npanel, l.ny, l.nx, at, sorted))) return rc;
    const int nh = (l.npanel - 1) / l.nw + 1;
    const long NYl = (long)nh * l.ny + (long)(nh - 1) * l.gap, NXl = (long)l.nw * l.nx + (long)(l.nw - 1) * l.gap;
    if (NYl > 65535 || NXl > (1 << 24)) return rip_fail(ctx, RIP_EINVAL, "fpa_render: a picture of (%ld, %ld) pixels is too large", NYl, NXl);
    const FrLayout L{l.n1, l.nsca, l.npanel, l.nw, l.gap, l.ny, l.nx, l.sc, l.nstamps, (int)NYl, (int)NXl};

    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nmaps = (size_t)l.npanel * l.nsca * l.n1 * l.n1, nout = (size_t)NYl * NXl * 3;
    DevArg<double> m;
    DevArg<uint8_t> o;
    DevBuf<double> dlo(ctx), dhi(ctx);
    DevBuf<uint8_t> dpres(ctx), dscale(ctx), dtab(ctx), dgl(ctx);
    DevBuf<int32_t> dpos(ctx), dst(ctx), dat(ctx);
    if ((rc = m.in(ctx, maps, nmaps, maps_location))) return rc;
    if ((rc = dlo.upload(vmin, l.npanel)) || (rc = dhi.upload(vmax, l.npanel)) || (rc = dpres.upload(present, (size_t)l.npanel * l.nsca)) ||
        (rc = dscale.upload(scale, l.npanel)) || (rc = dtab.upload(table, 768)) || (rc = dpos.upload(sca_pos, (size_t)2 * l.nsca)) ||
        (rc = l.nstamps ? dst.upload(sorted.data(), sorted.size()) : dst.alloc(1)) || (rc = dat.upload(at.data(), at.size())))
        return rc;
    if (glyphs && (rc = dgl.upload(glyphs, 256 * 12 * 6))) return rc;
    if ((rc = o.out(ctx, out, nout, out_location))) return rc;
    hipLaunchKernelGGL(fpa_render_kernel, dim3((L.NX + 255) / 256, L.NY), dim3(256), 0, ctx->stream, L, m.p, dpres.p, dpos.p, dlo.p, dhi.p,
                       dscale.p, dtab.p, dgl.p, dst.p, dat.p, o.p);
    RIP_HIP(ctx, hipGetLastError());
    if ((rc = o.download())) return rc;
    return dev_sync(ctx);   // the tables above are host vectors of this call: their copies are done before it returns
}
