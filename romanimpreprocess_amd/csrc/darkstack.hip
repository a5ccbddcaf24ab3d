// Dark and read-noise files: what the reference's runs/2026_July/make_dark_file.py computes from a set of dark exposures and a
// noise summary -- the step in front of calfiles.hip (rip_cal_biascorr takes dark_data as input).
//   make_dark_file.py:55-71   group means of one exposure, np.mean(cube[a:b].astype(f32), axis=0)      -> rip_cal_group_means     (exact)
//   make_dark_file.py:72      np.nanmean(sigma_clip(stack, sigma=3, axis=0, masked=False), axis=0)      -> rip_cal_sigma_clip_mean (specified
//                             in include/romanhip.h and DESIGN.md section 7: astropy is not available, its parity is unpinned)
//   make_dark_file.py:79-85   dark_slope, dark_slope_err = where(dark2 > 200, dark1, dark2)              -> rip_cal_dark_planes     (exact)
//   make_dark_file.py:157     read_noise = f32(cds / np.sqrt(2)), a float64 division under numpy >= 2
// The stack (groups x exposures x ny x nx f32, 13 GB for 100 darks of the production table) lives in HBM and never moves: the
// array arguments take a location (RIP_HOST: staged through a scoped device buffer; RIP_DEVICE: used where they are).
#include "rip_host.h"
#include "rip_samples.h"
#include "rip_select.h"

namespace {

#define DS_MAX_PLANES 512   // make_dark_file.py stops at 500 files; 512 keys x 64 pixels x 4 B = 128 KB of the 160 KB of LDS
#define DS_MAX_ITERS 16

struct DsReads {
    int32_t r[2 * RIP_MAX_GROUPS];   // group g holds the reads r[2g] .. r[2g+1]-1
};

// ------------------------------------------------------------------------------------------ group means
// One thread per 8 consecutive columns of one row (W8: one 16-byte load per read; needs nx_file % 8 == 0 and a 16-byte aligned
// cube) or per column.  cube points at row y0 of read 0; reads are `plane` samples apart.  Per group the f32 sum runs in read
// order and is divided once by f32(b - a): np.mean over axis 0 of a float32 array (no pairwise blocking across that axis).
template <bool W8>
__global__ __launch_bounds__(256) void group_means_kernel(const uint16_t *__restrict__ cube, size_t plane, int nx_file, int ny, int nx,
                                                          const DsReads rd, int ng, int be16, float *__restrict__ stack,
                                                          size_t group_stride) {
    constexpr int V = W8 ? 8 : 1;
    const int nvec = (nx + V - 1) / V;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)ny * nvec) return;
    const int y = (int)(i / nvec), x0 = (int)(i - (size_t)y * nvec) * V;
    const uint16_t *src = cube + (size_t)y * nx_file + x0;
    float *dst = stack + (size_t)y * nx + x0;
    const int stored = be16 != 0;
    for (int g = 0; g < ng; ++g) {
        const int a = rd.r[2 * g], b = rd.r[2 * g + 1];
        float acc[V];
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] = 0.0f;
#pragma unroll 4
        for (int r = a; r < b; ++r) {
            uint32_t x[V];
            load_samples<V>(src + (size_t)r * plane, stored, x);
#pragma unroll
            for (int k = 0; k < V; ++k) acc[k] = acc[k] + (float)x[k];
        }
        const float d = (float)(b - a);
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] = acc[k] / d;
        // rows of the stack start on 16 bytes when nx % 4 == 0
        store_results(dst + (size_t)g * group_stride, acc, nx - x0, (nx & 3) == 0);
    }
}

// ------------------------------------------------------------------------------------------ clipped mean over the planes
#define DS_KEY_MIN 0x00800000u   // key(-FLT_MAX): -inf and the NaNs with the sign bit lie below
#define DS_KEY_MAX 0xFF7FFFFFu   // key(+FLT_MAX): +inf and the other NaNs lie above

// Key of the smallest float x with (double)x >= lo, resp. of the largest with (double)x <= hi.  Finite floats are consecutive
// keys, so the neighbour of a float is its key +- 1; the two zeros compare equal and go together.
__device__ __forceinline__ uint32_t ds_lo_key(double lo) {
    const float f = (float)lo;
    uint32_t k = f2key(f);
    if ((double)f < lo) k += 1;
    return key2f(k) == 0.0f ? 0x7FFFFFFFu : k;
}
__device__ __forceinline__ uint32_t ds_hi_key(double hi) {
    const float f = (float)hi;
    uint32_t k = f2key(f);
    if ((double)f > hi) k -= 1;
    return key2f(k) == 0.0f ? 0x80000000u : k;
}

// One workgroup of four waves per 64 pixels, the column layout of rip_select.h: the column of n keys of pixel `lane` sits in
// LDS as tile[s*64 + lane], wave w works on the planes s = w (mod 4) -- keys it stored itself -- and the four partial results
// meet in xch (ColMeet); every wave then takes the same decisions for its 64 pixels.
// The survivors of every round are a contiguous range of the sorted column, so the clip is a pair of KEY bounds [klo, khi]
// (a value is removed when (double)x < lo or (double)x > hi, strictly: ds_lo_key / ds_hi_key); the non-finite values are outside
// the first pair.  Per round: count and f64 sum -> mean m; f64 sum of (x - m)^2 -> s = sqrt(. / count); median c by radix
// selection among the survivors (col_select); new bounds c - slo*s, c + shi*s.  A pixel stops when a round removed nothing
// (its bounds freeze); the workgroup leaves the loop when all 64 have stopped, which every wave finds by itself.  The partial
// sums are added in the order of the waves: a fixed order.  The result is the f64 sum of the survivors in PLANE order (wave 0
// walks the column once), divided by the count and rounded once to f32.  All loops are bounded by n, DS_MAX_ITERS and 32 bits.
__global__ __launch_bounds__(256) void sigma_clip_kernel(const float *__restrict__ stack, int n, size_t plane_stride, size_t npix,
                                                         double slo, double shi, int maxiters, float *__restrict__ mean,
                                                         int32_t *__restrict__ count) {
    extern __shared__ uint32_t tile[];
    __shared__ uint4 xch[2][4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t p = (size_t)blockIdx.x * 64 + lane;
    const bool live = p < npix;
    const size_t pp = live ? p : npix - 1;
    for (int s = w; s < n; s += 4) tile[s * 64 + lane] = f2key(stack[(size_t)s * plane_stride + pp]);
    auto key = [&](int s) -> uint32_t { return tile[s * 64 + lane]; };
    ColMeet meet{xch, w, lane, 0};
    uint32_t klo = DS_KEY_MIN, khi = DS_KEY_MAX;
    int cnt = 0, cnt_prev = -1;
    for (int it = 0; it <= DS_MAX_ITERS; ++it) {
        // survivors: count and sum
        uint32_t c = 0;
        double sum = 0.0;
#pragma unroll 4
        for (int s = w; s < n; s += 4) {
            const uint32_t e = tile[s * 64 + lane];
            if (e >= klo && e <= khi) {
                c += 1;
                sum = sum + (double)key2f(e);
            }
        }
        {
            uint32_t ct = 0;
            double st = 0.0;
            meet(make_uint4(c, (uint32_t)__double2loint(sum), (uint32_t)__double2hiint(sum), 0u), [&](const uint4 &v) {
                ct += v.x;
                st = st + __hiloint2double((int)v.z, (int)v.y);
            });
            cnt = (int)ct;
            sum = st;
        }
        const bool done = cnt == cnt_prev || cnt == 0 || it >= maxiters;
        if (__all(done)) break;   // the four waves hold the same 64 pixels: the same answer in each
        cnt_prev = cnt;
        const double m = sum / (double)cnt;
        // standard deviation about the mean, ddof 0
        double ssq = 0.0;
#pragma unroll 4
        for (int s = w; s < n; s += 4) {
            const uint32_t e = tile[s * 64 + lane];
            if (e >= klo && e <= khi) {
                const double d = (double)key2f(e) - m;
                ssq = ssq + d * d;
            }
        }
        {
            double st = 0.0;
            meet(make_uint4((uint32_t)__double2loint(ssq), (uint32_t)__double2hiint(ssq), 0u, 0u),
                 [&](const uint4 &v) { st = st + __hiloint2double((int)v.y, (int)v.x); });
            ssq = st;
        }
        const double sd = sqrt(ssq / (double)cnt);
        // median of the survivors; for an even count the mean of the two middle values
        auto in = [&](uint32_t e) { return e >= klo && e <= khi; };
        const uint32_t mid = col_select(n, w, (cnt - 1) / 2, key, in, meet);
        const uint32_t upper = col_select_upper(n, w, cnt, mid, key, in, meet);
        double cen = (double)key2f(mid);
        if ((cnt & 1) == 0) cen = 0.5 * (cen + (double)key2f(upper));
        if (!done) {
            klo = max(klo, ds_lo_key(cen - slo * sd));
            khi = min(khi, ds_hi_key(cen + shi * sd));
        }
    }
    if (w != 0) return;   // no barrier follows
    double sum = 0.0;
    for (int s = 0; s < n; ++s) {
        const uint32_t e = tile[s * 64 + lane];
        if (e >= klo && e <= khi) sum = sum + (double)key2f(e);
    }
    if (live) {
        mean[p] = cnt > 0 ? (float)(sum / (double)cnt) : __uint_as_float(0x7FC00000u);
        if (count) count[p] = cnt;
    }
}

// ------------------------------------------------------------------------------------------ dark_slope, dark_slope_err, read_noise
// Inputs are rows of `ld` floats (the [:, :nside] crop of the summary's planes), outputs (ny,nx).
__global__ __launch_bounds__(256) void dark_planes_kernel(const float *__restrict__ dark1, const float *__restrict__ dark2,
                                                          const float *__restrict__ err1, const float *__restrict__ err2,
                                                          const float *__restrict__ cds, size_t ld, int ny, int nx, double root2,
                                                          float *__restrict__ slope, float *__restrict__ slope_err,
                                                          float *__restrict__ read_noise) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)ny * nx) return;
    const size_t y = i / nx, q = y * ld + (i - y * nx);
    const float d2 = dark2[q];
    const bool use1 = d2 > 200.0f;   // above 200 DN/s, switch to dark1 (false on NaN)
    slope[i] = use1 ? dark1[q] : d2;
    slope_err[i] = use1 ? err1[q] : err2[q];
    read_noise[i] = (float)((double)cds[q] / root2);
}

}   // namespace

// ============================================================================================ C-ABI

int rip_cal_group_means(rip_ctx *ctx, const uint16_t *cube, int location, int nreads, int ny_file, int nx_file, int y0, int ny, int nx,
                        const int32_t *reads, int ng, int fits_be16, float *stack, int cap, int j) {
    if (ng < 1 || ng > RIP_MAX_GROUPS) return rip_fail(ctx, RIP_EINVAL, "cal_group_means: %d groups (1..%d supported)", ng, RIP_MAX_GROUPS);
    if (!cube || !reads || !stack) return rip_fail(ctx, RIP_EINVAL, "cal_group_means: a required array is NULL");
    if (const int rc = rip_check_location(ctx, "cal_group_means", "location", location)) return rc;
    if (nreads < 1 || ny_file < 1 || nx_file < 1 || ny < 1 || nx < 1 || y0 < 0 || (int64_t)y0 + ny > ny_file)
        return rip_fail(ctx, RIP_EINVAL, "cal_group_means: rows %d+%d of a (%d,%d,%d) cube", y0, ny, nreads, ny_file, nx_file);
    if (nx > nx_file) return rip_fail(ctx, RIP_EINVAL, "cal_group_means: %d columns wanted of a frame of %d", nx, nx_file);
    if (cap < 1 || j < 0 || j >= cap) return rip_fail(ctx, RIP_EINVAL, "cal_group_means: slot %d outside a stack of %d", j, cap);
    DsReads rd{};
    for (int g = 0; g < ng; ++g) {
        const int64_t a = reads[2 * g], b = reads[2 * g + 1];
        if (b <= a) return rip_fail(ctx, RIP_EINVAL, "cal_group_means: group %d holds no read (READS %ld, %ld)", g, (long)a, (long)b);
        if (a < 0 || b > nreads)
            return rip_fail(ctx, RIP_EINVAL, "cal_group_means: group %d (READS %ld, %ld) lies outside the %d reads of the cube", g, (long)a,
                            (long)b, nreads);
        rd.r[2 * g] = (int32_t)a;
        rd.r[2 * g + 1] = (int32_t)b;
    }
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    CubeBand band(ctx);
    if (const int rc = band.in(cube, location, ny_file, nx_file, 0, nreads, y0, ny)) return rc;
    const size_t npix = (size_t)ny * nx;
    float *out = stack + (size_t)j * npix;
    const size_t group_stride = (size_t)cap * npix;
    const bool w8 = nx_file % 8 == 0 && aligned(band.p, 16) && aligned(stack, 16);
    const size_t threads = (size_t)ny * (w8 ? (nx + 7) / 8 : nx);
    const dim3 grid((unsigned)((threads + 255) / 256));
    RIP_LAUNCH_W8(group_means_kernel, w8, grid, dim3(256), 0, ctx->stream, band.p, band.plane, nx_file, ny, nx, rd, ng, fits_be16, out,
                  group_stride);
    RIP_HIP(ctx, hipGetLastError());
    return dev_sync(ctx);
}

int rip_cal_sigma_clip_mean(rip_ctx *ctx, const float *stack, int location, int n, size_t plane_stride, size_t npix, double sigma_lower,
                            double sigma_upper, int maxiters, float *mean, int32_t *count) {
    if (n < 1 || n > DS_MAX_PLANES) return rip_fail(ctx, RIP_EINVAL, "cal_sigma_clip_mean: %d planes (1..%d supported)", n, DS_MAX_PLANES);
    if (!stack || !mean || npix < 1 || plane_stride < npix || npix > (size_t)0x7FFFFFFF * 64)
        return rip_fail(ctx, RIP_EINVAL, "cal_sigma_clip_mean: bad arguments (%zu pixels, plane stride %zu)", npix, plane_stride);
    if (const int rc = rip_check_location(ctx, "cal_sigma_clip_mean", "location", location)) return rc;
    if (maxiters < 0 || maxiters > DS_MAX_ITERS)
        return rip_fail(ctx, RIP_EINVAL, "cal_sigma_clip_mean: maxiters %d (0..%d supported)", maxiters, DS_MAX_ITERS);
    if (!(sigma_lower >= 0.0 && sigma_lower <= 1.7976931348623157e308 && sigma_upper >= 0.0 && sigma_upper <= 1.7976931348623157e308))
        return rip_fail(ctx, RIP_EINVAL, "cal_sigma_clip_mean: sigma_lower %g, sigma_upper %g (finite, not negative)", sigma_lower, sigma_upper);
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    DevArg<float> s, m;
    DevArg<int32_t> c;
    int rc;
    if ((rc = s.in(ctx, stack, (size_t)(n - 1) * plane_stride + npix, location)) || (rc = m.out(ctx, mean, npix, location)) ||
        (rc = c.out(ctx, count, npix, location)))
        return rc;
    const size_t bytes = (size_t)n * 64 * sizeof(uint32_t);
    if ((rc = with_lds(ctx, sigma_clip_kernel, bytes))) return rc;
    hipLaunchKernelGGL(sigma_clip_kernel, dim3((unsigned)((npix + 63) / 64)), dim3(256), bytes, ctx->stream, s.p, n, plane_stride, npix,
                       sigma_lower, sigma_upper, maxiters, m.p, c.p);
    RIP_HIP(ctx, hipGetLastError());
    if ((rc = m.download()) || (rc = c.download())) return rc;
    return dev_sync(ctx);
}

int rip_cal_dark_planes(rip_ctx *ctx, const float *dark1, const float *dark2, const float *dark1_err, const float *dark2_err,
                        const float *cds, int location, int ny, int nx, size_t row_stride, float *dark_slope, float *dark_slope_err,
                        float *read_noise) {
    if (!dark1 || !dark2 || !dark1_err || !dark2_err || !cds || !dark_slope || !dark_slope_err || !read_noise || ny < 1 || nx < 1 ||
        row_stride < (size_t)nx)
        return rip_fail(ctx, RIP_EINVAL, "cal_dark_planes: bad arguments (%d x %d, row stride %zu)", ny, nx, row_stride);
    if (const int rc = rip_check_location(ctx, "cal_dark_planes", "location", location)) return rc;
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nin = (size_t)(ny - 1) * row_stride + nx, n = (size_t)ny * nx;
    DevArg<float> d1, d2, x1, x2, dc, s, se, rn;
    int rc;
    if ((rc = d1.in(ctx, dark1, nin, location)) || (rc = d2.in(ctx, dark2, nin, location)) || (rc = x1.in(ctx, dark1_err, nin, location)) ||
        (rc = x2.in(ctx, dark2_err, nin, location)) || (rc = dc.in(ctx, cds, nin, location)) || (rc = s.out(ctx, dark_slope, n, location)) ||
        (rc = se.out(ctx, dark_slope_err, n, location)) || (rc = rn.out(ctx, read_noise, n, location)))
        return rc;
    hipLaunchKernelGGL(dark_planes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d1.p, d2.p, x1.p, x2.p, dc.p,
                       row_stride, ny, nx, sqrt(2.0), s.p, se.p, rn.p);
    RIP_HIP(ctx, hipGetLastError());
    if ((rc = s.download()) || (rc = se.download()) || (rc = rn.download())) return rc;
    return dev_sync(ctx);
}
