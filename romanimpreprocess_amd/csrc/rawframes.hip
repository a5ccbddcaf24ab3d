// Raw detector frames to exposure cubes and slope images: what the reference's three converters of the test-stand data
// (runs/summer2025run/convert_dark.py, convert_flt.py, convert_loflt.py; the line numbers below are convert_flt.py's) do between
// reading the single-frame files and writing the cube -- the step in front of solid-waffle and of make_dark_file (darkstack.hip).
//   :53-56   cube[0, k] = f[0].data             the stored samples decoded to native u16     \  rip_cal_raw_frame, one call per
//   :59-63   detector frame -> science frame    columns 0..4095 or the rows reversed          /  frame, into plane k of the cube
//   :65-79   two unweighted slope images, f64   sum_k cube[k] * w[k] / de, cast once to f32   -> rip_cal_frame_slopes, one launch
// The cube (1, N, 4096, 4224) u16 stays in HBM: calio.write_fits encodes it from there and DarkStack.add reads it there.
// Both kernels move bytes or do exact arithmetic (every product and partial sum is a multiple of 0.5 far below 2^53), so each
// has two forms that agree bit for bit: W8, one 16-byte load of 8 samples per lane, and one sample (pixel) per lane.
#include "rip_host.h"
#include "rip_samples.h"

namespace {

__device__ __forceinline__ uint32_t rf_swap_halves(uint32_t w) { return (w << 16) | (w >> 16); }

// orient 1: columns 0 .. nflip-1 of every row reversed, the others (the reference output) in place; orient 2: the rows reversed;
// orient 0: a copy.  W8: one lane per chunk of 8 columns, nx and nflip multiples of 8 -- a chunk lies wholly inside the reversed
// columns or wholly outside -- and both bases 16-byte aligned, so that every chunk of every row is (the real row is 8448 bytes).
// A reversed chunk has its 8 samples reversed in registers and goes to the mirrored chunk.  dst does not overlap src.
template <bool W8>
__global__ __launch_bounds__(256) void frame_kernel(const uint16_t *__restrict__ src, int ny, int nx, int orient, int nflip, int stored,
                                                    uint16_t *__restrict__ dst) {
    constexpr int V = W8 ? 8 : 1;
    const int nvec = nx / V;   // (W8: nx is a multiple of 8)
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)ny * nvec) return;
    const int y = (int)(i / nvec), x = (int)(i - (size_t)y * nvec) * V;
    const int yd = orient == 2 ? ny - 1 - y : y;
    const bool rev = orient == 1 && x < nflip;
    const uint16_t *s = src + (size_t)y * nx + x;
    if constexpr (W8) {
        const uint4 q = *reinterpret_cast<const uint4 *>(s);
        uint32_t w[4] = {decode_pair(q.x, stored), decode_pair(q.y, stored), decode_pair(q.z, stored), decode_pair(q.w, stored)};
        uint4 o = make_uint4(w[0], w[1], w[2], w[3]);
        if (rev) o = make_uint4(rf_swap_halves(w[3]), rf_swap_halves(w[2]), rf_swap_halves(w[1]), rf_swap_halves(w[0]));
        const int xd = rev ? nflip - 8 - x : x;
        *reinterpret_cast<uint4 *>(dst + (size_t)yd * nx + xd) = o;
    } else {
        const int xd = rev ? nflip - 1 - x : x;
        dst[(size_t)yd * nx + xd] = (uint16_t)decode_sample(*s, stored);
    }
}

// slp[0][p] = f32(sum_{k=1}^{nc-1} f64(cube[k][p]) * w0[k] / de0), slp[1][p] = f32(sum_{k=1}^{nh-1} f64(cube[k][p]) * w1[k] / de1),
// nh = nc / 2: plane k is read once and feeds the second sum while k < nh.  w (device, 2 nc f64: w0 then w1) and the two
// denominators come from the host, which forms them as the script does.  The sums start at +0.0 and are exact in any order; the
// roundings are the f64 division and the conversion to f32.  de = 0 gives 0 / 0 = NaN (nc 1, 2; the second image up to nc 5).
// W8: one lane per 8 adjacent pixels, npix a multiple of 8 and 16-byte aligned bases (planes are npix samples apart).
template <bool W8>
__global__ __launch_bounds__(256) void slopes_kernel(const uint16_t *__restrict__ cube, size_t npix, int nc, const double *__restrict__ w,
                                                     double de0, double de1, float *__restrict__ slp) {
    constexpr int V = W8 ? 8 : 1;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix / V) return;   // (W8: npix is a multiple of 8)
    const size_t p = i * V;
    const int nh = nc / 2;
    double a0[V], a1[V];
#pragma unroll
    for (int j = 0; j < V; ++j) a0[j] = a1[j] = 0.0;
#pragma unroll 4
    for (int k = 1; k < nc; ++k) {
        const bool second = k < nh;   // (wave-uniform)
        const double w0 = w[k], w1 = second ? w[nc + k] : 0.0;
        uint32_t v[V];
        load_samples<V>(cube + (size_t)k * npix + p, 0, v);   // the cube is native
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const double s = (double)v[j];
            a0[j] = a0[j] + s * w0;
            if (second) a1[j] = a1[j] + s * w1;
        }
    }
    float o0[V], o1[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        o0[j] = (float)(a0[j] / de0);
        o1[j] = (float)(a1[j] / de1);
    }
    store_results(slp + p, o0);
    store_results(slp + npix + p, o1);
}

}   // namespace

// ============================================================================================ C-ABI

int rip_cal_raw_frame(rip_ctx *ctx, const uint16_t *frame, int location, int ny, int nx, int orient, int nflip, int stored,
                      uint16_t *dst) {
    if (!frame || !dst) return rip_fail(ctx, RIP_EINVAL, "cal_raw_frame: a required array is NULL");
    if (const int rc = rip_check_location(ctx, "cal_raw_frame", "location", location)) return rc;
    if (ny < 1 || nx < 1) return rip_fail(ctx, RIP_EINVAL, "cal_raw_frame: a frame of %d x %d samples", ny, nx);
    if (orient < 0 || orient > 2) return rip_fail(ctx, RIP_EINVAL, "cal_raw_frame: orient %d (0 none, 1 columns, 2 rows)", orient);
    if (nflip < 0 || nflip > nx) return rip_fail(ctx, RIP_EINVAL, "cal_raw_frame: nflip %d outside 0..%d", nflip, nx);
    if (stored < 0 || stored > 2)
        return rip_fail(ctx, RIP_EINVAL, "cal_raw_frame: stored %d (0 native, 1 FITS with BZERO 32768, 2 FITS int16)", stored);
    const size_t n = (size_t)ny * nx;
    if (!aligned(dst, 2) || (location == RIP_DEVICE && !aligned(frame, 2)))
        return rip_fail(ctx, RIP_EINVAL, "cal_raw_frame: a device pointer is not aligned to the 2-byte sample");
    if (ranges_meet(frame, n * 2, dst, n * 2)) return rip_fail(ctx, RIP_EINVAL, "cal_raw_frame: dst overlaps frame");
    if ((n + 255) / 256 > 0x7FFFFFFFu) return rip_fail(ctx, RIP_EINVAL, "cal_raw_frame: %zu samples are more than one launch takes", n);
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    DevArg<uint16_t> src;
    if (const int rc = src.in(ctx, frame, n, location)) return rc;
    const bool w8 = nx % 8 == 0 && nflip % 8 == 0 && aligned(src.p, 16) && aligned(dst, 16);
    const dim3 grid((unsigned)(((w8 ? n / 8 : n) + 255) / 256));
    RIP_LAUNCH_W8(frame_kernel, w8, grid, dim3(256), 0, ctx->stream, src.p, ny, nx, orient, nflip, stored, dst);
    RIP_HIP(ctx, hipGetLastError());
    return dev_sync(ctx);
}

int rip_cal_frame_slopes(rip_ctx *ctx, const uint16_t *cube, int n, int nc, size_t npix, const double *w0, double de0, const double *w1,
                         double de1, float *slp, int out_location) {
    if (!cube || !w0 || !w1 || !slp) return rip_fail(ctx, RIP_EINVAL, "cal_frame_slopes: a required array is NULL");
    if (const int rc = rip_check_location(ctx, "cal_frame_slopes", "out_location", out_location)) return rc;
    if (n < 1 || npix < 1 || npix > ((size_t)1 << 38) || (size_t)n > ((size_t)1 << 60) / npix)
        return rip_fail(ctx, RIP_EINVAL, "cal_frame_slopes: a cube of %d planes of %zu pixels", n, npix);
    if (nc < 1 || nc > n) return rip_fail(ctx, RIP_EINVAL, "cal_frame_slopes: nc %d outside 1..%d", nc, n);
    if (!aligned(cube, 2) || (out_location == RIP_DEVICE && !aligned(slp, 4)))
        return rip_fail(ctx, RIP_EINVAL, "cal_frame_slopes: a device pointer is not aligned to its sample");
    if (ranges_meet(cube, (size_t)n * npix * 2, slp, npix * 8)) return rip_fail(ctx, RIP_EINVAL, "cal_frame_slopes: slp overlaps the cube");
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf<double> w(ctx);
    DevArg<float> d;
    int rc;
    if ((rc = w.alloc(2 * (size_t)nc)) || (rc = w.copy_in(w0, (size_t)nc))) return rc;
    RIP_HIP(ctx, hipMemcpyAsync(w.p + nc, w1, (size_t)nc * sizeof(double), hipMemcpyDefault, ctx->stream));
    if ((rc = d.out(ctx, slp, 2 * npix, out_location))) return rc;
    const bool w8 = npix % 8 == 0 && aligned(cube, 16) && aligned(d.p, 16);
    const dim3 grid((unsigned)(((w8 ? npix / 8 : npix) + 255) / 256));
    RIP_LAUNCH_W8(slopes_kernel, w8, grid, dim3(256), 0, ctx->stream, cube, npix, nc, w.p, de0, de1, d.p);
    RIP_HIP(ctx, hipGetLastError());
    if ((rc = d.download())) return rc;
    return dev_sync(ctx);
}
