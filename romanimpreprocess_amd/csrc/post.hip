// Post-path 2-D reductions of the L2 image: what calibrateimage does between the chain's
// outputs and the L2 file.
//   maskhandling.py:82-117   CombinedMask.build (bit-wise grown mask)                    -> rip_stage_build_mask   (exact)
//   sky.py:20-41             binkxk of the masked image                                  -> rip_stage_bin_mean     (f32 sums; order differs)
//   sky.py:44-97             smooth_mode: percentiles + Gaussian-smoothed histogram       -> rip_stage_select_ranks (exact order statistics)
//                                                                                            rip_stage_gauss_hist   (f64 sums; order differs)
//   sky.py:100-191           medfit: block nan-medians, Legendre model, subtraction       -> rip_stage_select_ranks, rip_stage_legendre2d (exact)
//   gen_cal_image.py:697-712 SLICEOUT endslice                                            -> rip_stage_endslice     (exact)
//   coordutils.py:17-82      pixelarea of a FITS zenithal (+SIP) WCS -> AreaFactor plane  -> rip_stage_pixel_area   (f64)
// Arrays in and out are host arrays or device pointers (rip_host.h; these are per-image calls on planes the caller already
// holds, the noise-layer driver in HBM); the area map may also be written to device memory in place.
#include <cmath>

#include "rip_grow.h"
#include "rip_host.h"
#include "rip_select.h"

namespace {

// ------------------------------------------------------------------------------------------ mask
// layer(bit) grown by its kernel: 1 = copy, 5 = plus, 9 = 3x3, 25 = 5x5 (zero padded, scipy.signal.convolve mode="same")
__global__ __launch_bounds__(256) void mask_build_kernel(const uint32_t *__restrict__ dq, uint8_t *__restrict__ out, int ny,
                                                         int nx, GrowMasks g) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= nx) return;
    const auto at = [&](int yy, int xx) -> uint32_t { return (xx < 0 || xx >= nx) ? 0u : dq[(size_t)yy * nx + xx]; };
    uint32_t hit = 0;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= ny) continue;
        hit |= grow_row(g, dy < 0 ? -dy : dy, at(yy, x), at(yy, x - 1) | at(yy, x + 1), at(yy, x - 2) | at(yy, x + 2));
    }
    out[(size_t)y * nx + x] = hit ? 1 : 0;
}

// ------------------------------------------------------------------------------------------ endslice
__global__ __launch_bounds__(256) void endslice_kernel(const uint8_t *__restrict__ rdq, int8_t *__restrict__ out, int G, int ny,
                                                       int nx, int nb) {
    const int xa = blockIdx.x * blockDim.x + threadIdx.x, ya = blockIdx.y;
    const int nxa = nx - 2 * nb;
    if (xa >= nxa) return;
    const size_t npix = (size_t)ny * nx, p = (size_t)(ya + nb) * nx + xa + nb;
    int8_t e = -1;
    uint8_t prev = rdq[p];
    for (int iend = 1; iend < G; ++iend) {
        const uint8_t cur = rdq[(size_t)iend * npix + p];
        if ((cur & ~prev) & DQ_SATURATED) e = (int8_t)(iend - 1);
        prev = cur;
    }
    out[(size_t)ya * nxa + xa] = e;
}

// ------------------------------------------------------------------------------------------ binned mean
// mean over k x k blocks of where(mask, nan, arr): NaN as soon as one pixel of the block is masked or NaN
__global__ __launch_bounds__(256) void bin_mean_kernel(const float *__restrict__ arr, const uint8_t *__restrict__ mask,
                                                       float *__restrict__ out, int nx, int nyo, int nxo, int k) {
    const int xo = blockIdx.x * blockDim.x + threadIdx.x, yo = blockIdx.y;
    if (xo >= nxo) return;
    float s = 0.0f;
    for (int a = 0; a < k; ++a) {
        float t = 0.0f;
        for (int b = 0; b < k; ++b) {
            const size_t p = (size_t)(yo * k + a) * nx + (size_t)xo * k + b;
            const float v = (mask && mask[p]) ? NAN : arr[p];
            t = t + v;
        }
        s = s + t;
    }
    out[(size_t)yo * nxo + xo] = s / (float)(k * k);
}

// ------------------------------------------------------------------------------------------ order statistics
// Blocks: nby x nbx rectangles of ky x kx pixels starting at (y0, x0) of an (ny, nx) f32 image.  NaNs are ignored.
// Three radix levels on the order-preserving key of the float (rip_select.h).
#define PS_MAX_BLOCKS 65535   // grid.y of the histogram launches
struct PsGeom {
    int ny, nx, y0, x0, ky, kx, nby, nbx;
};

// level < 0: count the valid (non-NaN) elements of every block into hist[blk * SEL_BINS]
__global__ __launch_bounds__(256) void ps_hist_kernel(const float *__restrict__ arr, PsGeom g, const uint32_t *__restrict__ prefix,
                                                      uint32_t *__restrict__ hist, int level) {
    __shared__ uint32_t h[SEL_BINS];
    const int blk = blockIdx.y, by = blk / g.nbx, bx = blk % g.nbx;
    for (int i = threadIdx.x; i < SEL_BINS; i += blockDim.x) h[i] = 0;
    __syncthreads();
    const size_t n = (size_t)g.ky * g.kx;
    const int shift = level >= 0 ? sel_shift(level) : 0;
    const uint32_t mask = level >= 0 ? (1u << sel_bits(level)) - 1u : 0u;
    const int above = level >= 0 ? shift + sel_bits(level) : 32;
    const uint32_t pre = (level > 0) ? prefix[blk] : 0u;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int yy = g.y0 + by * g.ky + (int)(i / g.kx), xx = g.x0 + bx * g.kx + (int)(i % g.kx);
        const float v = arr[(size_t)yy * g.nx + xx];
        if (v != v) continue;
        if (level < 0) {
            atomicAdd(&h[0], 1u);
        } else {
            const uint32_t key = f2key(v);
            if (above < 32 && ((key ^ pre) >> above) != 0) continue;
            atomicAdd(&h[(key >> shift) & mask], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SEL_BINS; i += blockDim.x)
        if (h[i]) atomicAdd(&hist[(size_t)blk * SEL_BINS + i], h[i]);
}

// one thread per block: walk the histogram to the bin holding `rank`, extend the key prefix, rebase the rank
__global__ void ps_scan_kernel(uint32_t *__restrict__ hist, uint32_t *__restrict__ prefix, unsigned long long *__restrict__ rank,
                               int nblk, int level) {
    const int blk = blockIdx.x * blockDim.x + threadIdx.x;
    if (blk >= nblk) return;
    uint32_t *h = hist + (size_t)blk * SEL_BINS;
    unsigned long long r = rank[blk], cum = 0;
    const int nb = 1 << sel_bits(level);
    int b = 0;
    for (; b < nb - 1; ++b) {
        if (cum + h[b] > r) break;
        cum += h[b];
    }
    rank[blk] = r - cum;
    prefix[blk] = (level == 0 ? 0u : prefix[blk]) | ((uint32_t)b << sel_shift(level));
    for (int i = 0; i < SEL_BINS; ++i) h[i] = 0;
}

__global__ void ps_finish_kernel(const uint32_t *__restrict__ prefix, float *__restrict__ out, int nblk) {
    const int blk = blockIdx.x * blockDim.x + threadIdx.x;
    if (blk < nblk) out[blk] = key2f(prefix[blk]);
}

// ------------------------------------------------------------------------------------------ smoothed histogram
// out[i] = sum over the non-NaN x of exp(-0.5 ((z[i] - x) / scale)^2), i < nz <= 32, in f64.  Two steps without atomics, so
// that the order of the sum -- and with it every bit of the result -- is the same from run to run: each workgroup leaves
// its partial sums in part[block * nz + i], gauss_hist_finish_kernel adds them in block order.
__global__ __launch_bounds__(256) void gauss_hist_kernel(const float *__restrict__ arr, size_t n, const double *__restrict__ z, int nz,
                                                         double scale, double *__restrict__ part) {
    __shared__ double red[256];
    double acc[32];
    for (int i = 0; i < 32; ++i) acc[i] = 0.0;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
        const float xv = arr[p];
        if (xv != xv) continue;
        const double x = (double)xv;
        for (int i = 0; i < nz; ++i) {
            const double u = (z[i] - x) / scale;
            acc[i] += exp(-0.5 * (u * u));
        }
    }
    for (int i = 0; i < nz; ++i) {
        red[threadIdx.x] = acc[i];
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0) part[(size_t)blockIdx.x * nz + i] = red[0];
        __syncthreads();
    }
}

__global__ void gauss_hist_finish_kernel(const double *__restrict__ part, int nblocks, int nz, double *__restrict__ out) {
    const int i = threadIdx.x;
    if (i >= nz) return;
    double s = 0.0;
    for (int b = 0; b < nblocks; ++b) s += part[(size_t)b * nz + i];
    out[i] = s;
}

// ------------------------------------------------------------------------------------------ Legendre model
// model[y,x] = sum_k coef[k] * (LPY[j_k][y] * LPX[i_k][x]) accumulated in f64 in the order k = 0.. (sky.py:183-189),
// cast to f32; arr -= model when subtract.  (i_k, j_k): i = 0..order, j = 0..order-i.
__global__ __launch_bounds__(256) void legendre2d_kernel(float *__restrict__ arr, float *__restrict__ model_out,
                                                         const double *__restrict__ LPX, const double *__restrict__ LPY,
                                                         const double *__restrict__ coef, int order, int ny, int nx, int subtract) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= nx) return;
    double m = 0.0;
    int k = 0;
    for (int i = 0; i <= order; ++i)
        for (int j = 0; j <= order - i; ++j) {
            const double o = LPY[(size_t)j * ny + y] * LPX[(size_t)i * nx + x];
            m = m + coef[k] * o;
            ++k;
        }
    const float mf = (float)m;
    const size_t p = (size_t)y * nx + x;
    if (model_out) model_out[p] = mf;
    if (subtract) arr[p] = arr[p] - mf;
}

// ------------------------------------------------------------------------------------------ pixel area
// (alpha, delta) in radians of the 0-based pixel coordinate (x, y): SIP, CD, the zenithal projection's native latitude, then
// the spherical rotation of Calabretta & Greisen (2002) eq. 2 with (alpha_p, delta_p) = CRVAL, phi_p = LONPOLE.
__device__ void pa_world(const rip_wcs_desc &w, double x, double y, double &alpha, double &delta) {
    const double deg = M_PI / 180.0;
    double u = x - w.crpix[0], v = y - w.crpix[1];
    if (w.sip_order > 0) {
        double fa = 0.0, fb = 0.0;   // sum over p + q <= order of A_p_q u^p v^q, B likewise (Horner in v, then in u)
        for (int p = w.sip_order; p >= 0; --p) {
            double ra = 0.0, rb = 0.0;
            for (int q = w.sip_order - p; q >= 0; --q) {
                ra = ra * v + w.sip_a[p][q];
                rb = rb * v + w.sip_b[p][q];
            }
            fa = fa * u + ra;
            fb = fb * u + rb;
        }
        u = u + fa;
        v = v + fb;
    }
    const double X = w.cd[0][0] * u + w.cd[0][1] * v, Y = w.cd[1][0] * u + w.cd[1][1] * v;   // degrees
    const double R = hypot(X, Y);
    const double phi = atan2(X, -Y);
    double theta;
    switch (w.projection) {
        case RIP_PROJ_TAN: theta = atan2(180.0 / M_PI, R); break;
        case RIP_PROJ_STG: theta = M_PI / 2.0 - 2.0 * atan(M_PI * R / 360.0); break;
        case RIP_PROJ_ZEA: theta = M_PI / 2.0 - 2.0 * asin(M_PI * R / 360.0); break;
        case RIP_PROJ_ARC: theta = (90.0 - R) * deg; break;
        default: theta = acos(M_PI * R / 180.0); break;   // RIP_PROJ_SIN
    }
    double st, ct, sd, cd, sp, cp;
    sincos(theta, &st, &ct);
    sincos(w.crval[1] * deg, &sd, &cd);
    sincos(phi - w.lonpole * deg, &sp, &cp);
    delta = asin(st * sd + ct * cd * cp);
    alpha = w.crval[0] * deg + atan2(-ct * sp, st * cd - ct * sd * cp);
}

// One workgroup per 32 x 32 output pixels: its threads evaluate the WCS on the tile's grid points plus a one-point halo (34 x 34),
// keep the equal-area coordinates (U, V) in LDS, then form the central-difference Jacobian of each pixel (coordutils.py:57-81).
// Grid point (gx, gy) = pixel coordinate; the grid runs from -1 to nx (ny), so every halo point an output needs exists.
#define PA_T 32
#define PA_H (PA_T + 2)
__global__ __launch_bounds__(256) void pixel_area_kernel(const rip_wcs_desc w, int ny, int nx, double scale, double *__restrict__ out) {
    __shared__ double su[PA_H * PA_H], sv[PA_H * PA_H];
    __shared__ int north;
    const int x0 = blockIdx.x * PA_T, y0 = blockIdx.y * PA_T;
    if (threadIdx.x == 0) {   // the hemisphere of the first grid point picks the pole (coordutils.py:60-62)
        double a, d;
        pa_world(w, -1.0, -1.0, a, d);
        north = d > 0.0 ? 1 : 0;
    }
    __syncthreads();
    const bool n = north != 0;
    for (int i = threadIdx.x; i < PA_H * PA_H; i += blockDim.x) {
        const int gx = x0 - 1 + i % PA_H, gy = y0 - 1 + i / PA_H;
        if (gx > nx || gy > ny) continue;
        double a, d;
        pa_world(w, (double)gx, (double)gy, a, d);
        const double th = n ? M_PI / 2.0 - d : M_PI / 2.0 + d;
        const double rho = 2.0 * sin(th / 2.0);
        double sa, ca;
        sincos(a, &sa, &ca);
        su[i] = rho * ca;
        sv[i] = rho * sa;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < PA_T * PA_T; i += blockDim.x) {
        const int tx = i % PA_T, ty = i / PA_T, x = x0 + tx, y = y0 + ty;
        if (x >= nx || y >= ny) continue;
        const int c = (ty + 1) * PA_H + tx + 1;
        const double J11 = (su[c + 1] - su[c - 1]) / 2.0, J12 = (su[c + PA_H] - su[c - PA_H]) / 2.0;
        const double J21 = (sv[c + 1] - sv[c - 1]) / 2.0, J22 = (sv[c + PA_H] - sv[c - PA_H]) / 2.0;
        out[(size_t)y * nx + x] = fabs(J11 * J22 - J21 * J12) / scale;
    }
}

}  // namespace

// ============================================================================================ C-ABI

int rip_stage_build_mask(rip_ctx *ctx, const uint32_t *dq, int ny, int nx, const uint8_t grow[32], uint8_t *mask) {
    if (!dq || !grow || !mask || ny < 1 || nx < 1) return rip_fail(ctx, RIP_EINVAL, "build_mask: bad arguments");
    GrowMasks g;
    const int bad = grow_masks(grow, &g);
    if (bad >= 0) return rip_fail(ctx, RIP_EINVAL, "build_mask: growth %d of bit %d is not one of 0, 1, 5, 9, 25", grow[bad], bad);
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)ny * nx;
    DevBuf<uint32_t> d(ctx);
    DevBuf<uint8_t> o(ctx);
    int rc;
    if ((rc = d.upload(dq, n)) || (rc = o.alloc(n))) return rc;
    hipLaunchKernelGGL(mask_build_kernel, dim3((nx + 255) / 256, ny), dim3(256), 0, ctx->stream, d.p, o.p, ny, nx, g);
    RIP_HIP(ctx, hipGetLastError());
    if ((rc = o.download(mask, n))) return rc;
    return dev_sync(ctx);
}

int rip_stage_endslice(rip_ctx *ctx, const uint8_t *rdq, int ngrp, int ny, int nx, int nb, int8_t *out) {
    if (!rdq || !out || ngrp < 1 || nb < 0 || ny <= 2 * nb || nx <= 2 * nb) return rip_fail(ctx, RIP_EINVAL, "endslice: bad arguments");
    if (ngrp >= 128) return rip_fail(ctx, RIP_EINVAL, "too many groups");
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)ngrp * ny * nx, na = (size_t)(ny - 2 * nb) * (nx - 2 * nb);
    DevBuf<uint8_t> d(ctx);
    DevBuf<int8_t> o(ctx);
    int rc;
    if ((rc = d.upload(rdq, n)) || (rc = o.alloc(na))) return rc;
    hipLaunchKernelGGL(endslice_kernel, dim3((nx - 2 * nb + 255) / 256, ny - 2 * nb), dim3(256), 0, ctx->stream, d.p, o.p, ngrp, ny, nx,
                       nb);
    RIP_HIP(ctx, hipGetLastError());
    if ((rc = o.download(out, na))) return rc;
    return dev_sync(ctx);
}

int rip_stage_bin_mean(rip_ctx *ctx, const float *arr, const uint8_t *mask, int ny, int nx, int k, float *out) {
    if (!arr || !out || k < 1 || ny < k || nx < k) return rip_fail(ctx, RIP_EINVAL, "bin_mean: bad arguments");
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const int nyo = ny / k, nxo = nx / k;
    const size_t n = (size_t)ny * nx, no = (size_t)nyo * nxo;
    DevBuf<float> d(ctx), o(ctx);
    DevBuf<uint8_t> m(ctx);
    int rc;
    if ((rc = d.upload(arr, n)) || (rc = o.alloc(no))) return rc;
    if (mask && (rc = m.upload(mask, n))) return rc;
    hipLaunchKernelGGL(bin_mean_kernel, dim3((nxo + 255) / 256, nyo), dim3(256), 0, ctx->stream, d.p, mask ? m.p : nullptr, o.p, nx, nyo,
                       nxo, k);
    RIP_HIP(ctx, hipGetLastError());
    if ((rc = o.download(out, no))) return rc;
    return dev_sync(ctx);
}

// counts[blk] = number of non-NaN elements; vals[blk * nranks + r] = element of 0-based rank ranks[blk * nranks + r]
// among them in ascending order (NaN when the rank is out of range).  ranks == NULL: only the counts.
int rip_stage_select_ranks(rip_ctx *ctx, const float *arr, int ny, int nx, int y0, int x0, int ky, int kx, int nby, int nbx,
                           int nranks, const int64_t *ranks, int64_t *counts, float *vals) {
    if (!arr || ky < 1 || kx < 1 || nby < 1 || nbx < 1 || y0 < 0 || x0 < 0 || y0 + (long)nby * ky > ny || x0 + (long)nbx * kx > nx ||
        nranks < 0 || (nranks > 0 && (!ranks || !vals)))
        return rip_fail(ctx, RIP_EINVAL, "select_ranks: bad geometry or arguments");
    // the histogram launches index the block by blockIdx.y: more blocks than grid.y can hold would fail at launch and leave
    // every count 0
    if ((long)nby * nbx > PS_MAX_BLOCKS)
        return rip_fail(ctx, RIP_EINVAL, "select_ranks: %ld blocks (%d x %d) is more than the %d one launch can index", (long)nby * nbx,
                        nby, nbx, PS_MAX_BLOCKS);
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const int nblk = nby * nbx;
    const size_t n = (size_t)ny * nx;
    DevBuf<float> d(ctx), o(ctx);
    DevBuf<uint32_t> hist(ctx), prefix(ctx);
    DevBuf<unsigned long long> rk(ctx);
    int rc;
    if ((rc = d.upload(arr, n)) || (rc = hist.alloc((size_t)nblk * SEL_BINS)) || (rc = prefix.alloc(nblk)) || (rc = rk.alloc(nblk)) ||
        (rc = o.alloc(nblk)))
        return rc;
    const PsGeom g{ny, nx, y0, x0, ky, kx, nby, nbx};
    const size_t per = (size_t)ky * kx;
    unsigned chunks = (unsigned)((per + 256 * 16 - 1) / (256 * 16));
    if (chunks < 1) chunks = 1;
    if (chunks > 1024) chunks = 1024;
    RIP_HIP(ctx, hipMemsetAsync(hist.p, 0, (size_t)nblk * SEL_BINS * 4, ctx->stream));
    hipLaunchKernelGGL(ps_hist_kernel, dim3(chunks, nblk), dim3(256), 0, ctx->stream, d.p, g, prefix.p, hist.p, -1);
    RIP_HIP(ctx, hipGetLastError());
    std::vector<uint32_t> hh((size_t)nblk * SEL_BINS);
    if ((rc = hist.download(hh.data(), hh.size())) || (rc = dev_sync(ctx))) return rc;
    std::vector<int64_t> cnt(nblk);
    for (int b = 0; b < nblk; ++b) cnt[b] = hh[(size_t)b * SEL_BINS];
    if (counts)
        for (int b = 0; b < nblk; ++b) counts[b] = cnt[b];
    std::vector<unsigned long long> r(nblk);
    std::vector<float> v(nblk);
    for (int q = 0; q < nranks; ++q) {
        for (int b = 0; b < nblk; ++b) {
            const int64_t want = ranks[(size_t)b * nranks + q];
            r[b] = (want >= 0 && want < cnt[b]) ? (unsigned long long)want : 0ull;
        }
        if ((rc = rk.copy_in(r.data(), nblk))) return rc;
        RIP_HIP(ctx, hipMemsetAsync(hist.p, 0, (size_t)nblk * SEL_BINS * 4, ctx->stream));
        for (int level = 0; level < 3; ++level) {
            hipLaunchKernelGGL(ps_hist_kernel, dim3(chunks, nblk), dim3(256), 0, ctx->stream, d.p, g, prefix.p, hist.p, level);
            hipLaunchKernelGGL(ps_scan_kernel, dim3((nblk + 63) / 64), dim3(64), 0, ctx->stream, hist.p, prefix.p, rk.p, nblk, level);
        }
        hipLaunchKernelGGL(ps_finish_kernel, dim3((nblk + 63) / 64), dim3(64), 0, ctx->stream, prefix.p, o.p, nblk);
        RIP_HIP(ctx, hipGetLastError());
        if ((rc = o.download(v.data(), nblk)) || (rc = dev_sync(ctx))) return rc;   // the host reads v: one wait per rank
        for (int b = 0; b < nblk; ++b) {
            const int64_t want = ranks[(size_t)b * nranks + q];
            vals[(size_t)b * nranks + q] = (want >= 0 && want < cnt[b]) ? v[b] : NAN;
        }
    }
    return RIP_OK;
}

int rip_stage_gauss_hist(rip_ctx *ctx, const float *arr, int64_t n, const double *z, int nz, double scale, double *out) {
    if (!arr || !z || !out || n < 1 || nz < 1 || nz > 32 || !(scale > 0.0)) return rip_fail(ctx, RIP_EINVAL, "gauss_hist: bad arguments");
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf<float> d(ctx);
    DevBuf<double> dz(ctx), part(ctx), o(ctx);
    unsigned blocks = (unsigned)(((size_t)n + 256 * 8 - 1) / (256 * 8));
    if (blocks > 2048) blocks = 2048;
    int rc;
    if ((rc = d.upload(arr, (size_t)n)) || (rc = dz.upload(z, nz)) || (rc = part.alloc((size_t)blocks * nz)) || (rc = o.alloc(nz)))
        return rc;
    hipLaunchKernelGGL(gauss_hist_kernel, dim3(blocks), dim3(256), 0, ctx->stream, d.p, (size_t)n, dz.p, nz, scale, part.p);
    RIP_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(gauss_hist_finish_kernel, dim3(1), dim3(32), 0, ctx->stream, part.p, (int)blocks, nz, o.p);
    RIP_HIP(ctx, hipGetLastError());
    if ((rc = o.download(out, nz))) return rc;
    return dev_sync(ctx);
}

int rip_stage_legendre2d(rip_ctx *ctx, float *arr, int ny, int nx, int order, const double *LPX, const double *LPY, const double *coef,
                         int subtract, float *model_out) {
    if (!LPX || !LPY || !coef || order < 0 || order > 8 || ny < 1 || nx < 1 || (subtract && !arr) || (!subtract && !model_out))
        return rip_fail(ctx, RIP_EINVAL, "legendre2d: bad arguments");
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)ny * nx;
    const int nc = (order + 1) * (order + 2) / 2;
    DevBuf<float> d(ctx), mo(ctx);
    DevBuf<double> lx(ctx), ly(ctx), c(ctx);
    int rc;
    if ((rc = lx.upload(LPX, (size_t)(order + 1) * nx)) || (rc = ly.upload(LPY, (size_t)(order + 1) * ny)) || (rc = c.upload(coef, nc)))
        return rc;
    if (subtract && (rc = d.upload(arr, n))) return rc;
    if (model_out && (rc = mo.alloc(n))) return rc;
    hipLaunchKernelGGL(legendre2d_kernel, dim3((nx + 255) / 256, ny), dim3(256), 0, ctx->stream, subtract ? d.p : nullptr,
                       model_out ? mo.p : nullptr, lx.p, ly.p, c.p, order, ny, nx, subtract);
    RIP_HIP(ctx, hipGetLastError());
    if (subtract && (rc = d.download(arr, n))) return rc;
    if (model_out && (rc = mo.download(model_out, n))) return rc;
    return dev_sync(ctx);
}

int rip_stage_pixel_area(rip_ctx *ctx, const rip_wcs_desc *wcs, int ny, int nx, double scale, int out_location, double *out) {
    if (!wcs || !out || ny < 1 || nx < 1 || !rip_is_location(out_location))
        return rip_fail(ctx, RIP_EINVAL, "pixel_area: bad arguments (ny %d, nx %d, out_location %d)", ny, nx, out_location);
    if (!(scale > 0.0) || !std::isfinite(scale)) return rip_fail(ctx, RIP_EINVAL, "pixel_area: scale %g is not a positive number", scale);
    if (wcs->projection < RIP_PROJ_TAN || wcs->projection > RIP_PROJ_SIN)
        return rip_fail(ctx, RIP_EINVAL, "pixel_area: projection %d is not one of TAN, STG, ZEA, ARC, SIN", wcs->projection);
    if (wcs->sip_order < 0 || wcs->sip_order > RIP_SIP_MAX_ORDER)
        return rip_fail(ctx, RIP_EINVAL, "pixel_area: SIP order %d outside 0..%d", wcs->sip_order, RIP_SIP_MAX_ORDER);
    const double *scalars = &wcs->crpix[0];   // crpix, cd, crval, lonpole: 9 doubles in a row
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(scalars[i])) return rip_fail(ctx, RIP_EINVAL, "pixel_area: non-finite CRPIX, CD, CRVAL or LONPOLE");
    for (int p = 0; p <= RIP_SIP_MAX_ORDER; ++p)
        for (int q = 0; q <= RIP_SIP_MAX_ORDER; ++q)
            if (!std::isfinite(wcs->sip_a[p][q]) || !std::isfinite(wcs->sip_b[p][q]))
                return rip_fail(ctx, RIP_EINVAL, "pixel_area: non-finite SIP coefficient [%d][%d]", p, q);
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)ny * nx;
    const dim3 grid((nx + PA_T - 1) / PA_T, (ny + PA_T - 1) / PA_T);
    if (grid.y > 65535) return rip_fail(ctx, RIP_EINVAL, "pixel_area: %d rows is too many", ny);
    DevArg<double> o;
    int rc;
    if ((rc = o.out(ctx, out, n, out_location))) return rc;
    hipLaunchKernelGGL(pixel_area_kernel, grid, dim3(256), 0, ctx->stream, *wcs, ny, nx, scale, o.p);
    RIP_HIP(ctx, hipGetLastError());
    if ((rc = o.download())) return rc;
    return out_location == RIP_DEVICE ? RIP_OK : dev_sync(ctx);   // a device map: queued, not waited for
}
