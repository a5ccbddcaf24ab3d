// Calibration-file derivation: what the reference's runs/2026_July/postprocess_calfiles.py and makemask.py compute from a
// linearitylegendre / dark / gain set -- the four remaining CALDIR files.
//   postprocess_calfiles.py:99-140  biascorr: dark cube minus the dark current run forward through   -> rip_cal_biascorr   (exact)
//                                   the inverse linearity, read by read, averaged per group
//   postprocess_calfiles.py:22-40   pflat: / medfit model, * g_ideal / median(gain), flag and clip   -> rip_cal_pflat      (exact)
//   postprocess_calfiles.py:69-97   saturation: clip(Smax, 1, 65535) - 1, dq = !(Smax > Sref)        -> rip_cal_saturation (exact)
//   makemask.py:12-36               mask: border | lin dq | low QE | hot / warm | gain dq            -> rip_cal_mask       (exact)
// The scalar steps around them (the 6 x 6 normal equations of medfit, the two plane medians) stay on the host side
// (romanimpreprocess_amd/calfiles/), on order statistics found by rip_stage_select_ranks.
// Arrays in and out are host arrays or device pointers (rip_host.h); READS, the Legendre tables and coefficients are host arrays.
#include "rip_host.h"
#include "invlin_device.h"

namespace {

#define CAL_MAX_GROUP_READS 65536   // reads of one group: bounds the read loop
#define DQ_HOT (1u << 11)           // makemask.py:32 (roman_datamodels.dqflags.pixel)
#define DQ_WARM (1u << 12)
#define DQ_LOW_QE (1u << 13)        // makemask.py:26

struct CalReads {
    int32_t r[2 * RIP_MAX_GROUPS];   // group j holds the reads r[2j] .. r[2j+1]-1
};

// ------------------------------------------------------------------------------------------ biascorr
// One thread per ACTIVE pixel; the input planes are full frames (ny,nx), the outputs (ngrp, ny-2nb, nx-2nb).
//   dark   = f32(dark_slope * f32(tframe))                                  DN per frame
//   signal = invlinearity(f32(dark * f32(x - xref)))                        f32 bisection, invlin_device.h
//   pred_j = f32(sum over the reads x of group j, in read order) / f32(n_j) ; biascorr_j = dark_data_j - pred_j
// The reads are walked in the order READS gives them.  For one pixel the targets dark * (x - xref) are monotone in x, so
// consecutive reads share the first steps of their bisection paths and rip_invlin_pixel_warm skips those evaluations; it takes
// the same decisions on the same values as the cold rip_invlin_pixel whatever the order of the targets (invlin_device.h), so
// gaps, repeats and unsorted groups only lose the saving.  The coefficients, Smin, Smax and dark_slope are read once.
template <int NP>
__global__ __launch_bounds__(256) void calfiles_biascorr_kernel(const float *__restrict__ dark_slope, const float *__restrict__ dark_data,
                                                                const float *__restrict__ coefs, const float *__restrict__ smin,
                                                                const float *__restrict__ smax, const CalReads rd, int ngrp,
                                                                float tframe, double xref, int ny, int nx, int nb,
                                                                float *__restrict__ biascorr, float *__restrict__ pred) {
    const int nxa = nx - 2 * nb;
    const size_t na = (size_t)(ny - 2 * nb) * nxa, npix = (size_t)ny * nx;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= na) return;
    const int ya = (int)(i / nxa), xa = (int)(i - (size_t)ya * nxa);
    const size_t p = (size_t)(ya + nb) * nx + xa + nb;
    float c[NP];
#pragma unroll
    for (int L = 0; L < NP; ++L) c[L] = coefs[(size_t)L * npix + p];
    const float lo = smin[p], hi = smax[p];
    const float dark = dark_slope[p] * tframe;
    float phi_path[24];
#pragma unroll
    for (int s = 0; s < 24; ++s) phi_path[s] = 0.0f;
    uint32_t path = 0;
    bool have = false;
    for (int j = 0; j < ngrp; ++j) {
        const int fr1 = rd.r[2 * j], fr2 = rd.r[2 * j + 1];
        float acc = 0.0f;
        for (int x = fr1; x < fr2; ++x) {
            const float target = dark * (float)((double)x - xref);
            bool ex;
            acc = acc + rip_invlin_pixel_warm<float, NP>(target, c, c, lo, hi, ex, phi_path, path, have);
        }
        acc = acc / (float)(fr2 - fr1);
        biascorr[(size_t)j * na + i] = dark_data[(size_t)j * npix + p] - acc;
        if (pred) pred[(size_t)j * na + i] = acc;
    }
}

// ------------------------------------------------------------------------------------------ pflat
// p = f32(p / f32(model)); p = f32(p * scale); dq = p < 0.01 || p > 1.99 (f32 compares, false on NaN); p = clip(p, 0.01, 1.99)
// (NaN stays NaN).  model[y,x] = sum_k coef[k] * (LPY[j_k][y] * LPX[i_k][x]) in f64 in rip_stage_legendre2d's order, rounded to
// the array's dtype as sky.medfit returns it (sky.py:191).
__global__ __launch_bounds__(256) void calfiles_pflat_kernel(const float *__restrict__ pflat, const double *__restrict__ LPX,
                                                             const double *__restrict__ LPY, const double *__restrict__ coef, int order,
                                                             int ny, int nx, float scale, float *__restrict__ data,
                                                             uint32_t *__restrict__ dq) {
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
    const size_t q = (size_t)y * nx + x;
    float p = pflat[q] / (float)m;
    p = p * scale;
    const float lo = 0.01f, hi = 1.99f;
    dq[q] = (p < lo || p > hi) ? 1u : 0u;
    data[q] = p < lo ? lo : (p > hi ? hi : p);
}

// ------------------------------------------------------------------------------------------ saturation
__global__ __launch_bounds__(256) void calfiles_saturation_kernel(const float *__restrict__ smax, const float *__restrict__ sref, size_t n,
                                                                  float *__restrict__ data, uint32_t *__restrict__ dq) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float s = smax[i];
    const float cl = s < 1.0f ? 1.0f : (s > 65535.0f ? 65535.0f : s);   // NaN falls through both compares
    data[i] = cl - 1.0f;
    dq[i] = s > sref[i] ? 0u : 1u;
}

// ------------------------------------------------------------------------------------------ mask
__global__ __launch_bounds__(256) void calfiles_mask_kernel(const uint32_t *__restrict__ lin_dq, const float *__restrict__ pflat0, float pmed,
                                                            const float *__restrict__ dark_slope, const uint32_t *__restrict__ gain_dq,
                                                            int ny, int nx, int nb, uint32_t *__restrict__ dq) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= nx) return;
    const size_t q = (size_t)y * nx + x;
    uint32_t m = lin_dq[q] | gain_dq[q];
    if (y < nb || y >= ny - nb || x < nb || x >= nx - nb) m |= DQ_REFERENCE_PIXEL;
    if (pflat0[q] / pmed < 0.5f) m |= DQ_LOW_QE;
    const float d = dark_slope[q];
    if (d > 0.25f) m |= d > 12.5f ? DQ_HOT : DQ_WARM;
    dq[q] = m;
}

template <int NP>
void launch_biascorr(rip_ctx *ctx, size_t na, const float *dark_slope, const float *dark_data, const float *coefs, const float *smin,
                     const float *smax, const CalReads &rd, int ngrp, float tframe, double xref, int ny, int nx, int nb, float *biascorr,
                     float *pred) {
    hipLaunchKernelGGL((calfiles_biascorr_kernel<NP>), dim3((unsigned)((na + 255) / 256)), dim3(256), 0, ctx->stream, dark_slope,
                       dark_data, coefs, smin, smax, rd, ngrp, tframe, xref, ny, nx, nb, biascorr, pred);
}

}   // namespace

// ============================================================================================ C-ABI

int rip_cal_biascorr(rip_ctx *ctx, const float *dark_slope, const float *dark_data, int ngrp_dark, int ny, int nx, int nb, int nplanes,
                     const float *coefs, const float *smin, const float *smax, const int32_t *reads, int ngrp, double tframe, int bframe,
                     float *biascorr, float *pred, double *t0) {
    if (ngrp < 1 || ngrp > RIP_MAX_GROUPS) return rip_fail(ctx, RIP_EINVAL, "cal_biascorr: %d groups (1..%d supported)", ngrp, RIP_MAX_GROUPS);
    if (ngrp != ngrp_dark)
        return rip_fail(ctx, RIP_EINVAL, "cal_biascorr: READS has %d groups, the dark cube %d", ngrp, ngrp_dark);
    if (ny < 1 || nx < 1 || nb < 0 || ny <= 2 * (int64_t)nb || nx <= 2 * (int64_t)nb)
        return rip_fail(ctx, RIP_EINVAL, "cal_biascorr: a border of %d leaves no active pixel on a %d x %d frame", nb, ny, nx);
    if (!dark_slope || !dark_data || !coefs || !smin || !smax || !reads || !biascorr)
        return rip_fail(ctx, RIP_EINVAL, "cal_biascorr: a required array is NULL");
    CalReads rd{};
    for (int j = 0; j < ngrp; ++j) {
        const int64_t fr1 = reads[2 * j], fr2 = reads[2 * j + 1];
        if (fr2 <= fr1) return rip_fail(ctx, RIP_EINVAL, "cal_biascorr: group %d holds no read (READS %ld, %ld)", j, (long)fr1, (long)fr2);
        if (fr2 - fr1 > CAL_MAX_GROUP_READS)
            return rip_fail(ctx, RIP_EINVAL, "cal_biascorr: group %d holds %ld reads (at most %d)", j, (long)(fr2 - fr1), CAL_MAX_GROUP_READS);
        rd.r[2 * j] = (int32_t)fr1;
        rd.r[2 * j + 1] = (int32_t)fr2;
    }
    if (bframe < 0 || bframe >= ngrp) return rip_fail(ctx, RIP_EINVAL, "cal_biascorr: bias group %d outside 0..%d", bframe, ngrp - 1);
    if (nplanes < 2 || nplanes > 17) return rip_fail(ctx, RIP_EINVAL, "cal_biascorr: %d coefficient planes (2..17 supported)", nplanes);
    const double xref = ((double)reads[2 * bframe] + (double)reads[2 * bframe + 1] - 1.0) / 2.0;
    if (t0) *t0 = tframe * xref;
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)ny * nx, na = (size_t)(ny - 2 * nb) * (nx - 2 * nb);
    DevBuf<float> dslope(ctx), ddark(ctx), dc(ctx), dmin(ctx), dmax(ctx), dout(ctx), dpred(ctx);
    int rc;
    if ((rc = dslope.upload(dark_slope, npix)) || (rc = ddark.upload(dark_data, (size_t)ngrp * npix)) ||
        (rc = dc.upload(coefs, (size_t)nplanes * npix)) || (rc = dmin.upload(smin, npix)) || (rc = dmax.upload(smax, npix)) ||
        (rc = dout.alloc((size_t)ngrp * na)) || (pred && (rc = dpred.alloc((size_t)ngrp * na))))
        return rc;
#define CAL_CASE(N)                                                                                                                \
    case N:                                                                                                                        \
        launch_biascorr<N>(ctx, na, dslope.p, ddark.p, dc.p, dmin.p, dmax.p, rd, ngrp, (float)tframe, xref, ny, nx, nb, dout.p,       \
                           pred ? dpred.p : nullptr);                                                                              \
        break;
    switch (nplanes) {
        CAL_CASE(2) CAL_CASE(3) CAL_CASE(4) CAL_CASE(5) CAL_CASE(6) CAL_CASE(7) CAL_CASE(8) CAL_CASE(9) CAL_CASE(10) CAL_CASE(11)
        CAL_CASE(12) CAL_CASE(13) CAL_CASE(14) CAL_CASE(15) CAL_CASE(16) CAL_CASE(17)
    }
#undef CAL_CASE
    RIP_HIP(ctx, hipGetLastError());
    if ((rc = dout.download(biascorr, (size_t)ngrp * na)) || (pred && (rc = dpred.download(pred, (size_t)ngrp * na)))) return rc;
    return dev_sync(ctx);
}

int rip_cal_pflat(rip_ctx *ctx, const float *pflat, int ny, int nx, int order, const double *LPX, const double *LPY, const double *coef,
                  float scale, float *data, uint32_t *dq) {
    if (!pflat || !LPX || !LPY || !coef || !data || !dq || order < 0 || order > 8 || ny < 1 || nx < 1 || ny > 65535)
        return rip_fail(ctx, RIP_EINVAL, "cal_pflat: bad arguments");
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)ny * nx;
    const int nc = (order + 1) * (order + 2) / 2;
    DevBuf<float> d(ctx), o(ctx);
    DevBuf<uint32_t> q(ctx);
    DevBuf<double> lx(ctx), ly(ctx), c(ctx);
    int rc;
    if ((rc = lx.upload(LPX, (size_t)(order + 1) * nx)) || (rc = ly.upload(LPY, (size_t)(order + 1) * ny)) || (rc = c.upload(coef, nc)) ||
        (rc = d.upload(pflat, n)) || (rc = o.alloc(n)) || (rc = q.alloc(n)))
        return rc;
    hipLaunchKernelGGL(calfiles_pflat_kernel, dim3((nx + 255) / 256, ny), dim3(256), 0, ctx->stream, d.p, lx.p, ly.p, c.p, order, ny, nx,
                       scale, o.p, q.p);
    RIP_HIP(ctx, hipGetLastError());
    if ((rc = o.download(data, n)) || (rc = q.download(dq, n))) return rc;
    return dev_sync(ctx);
}

int rip_cal_saturation(rip_ctx *ctx, const float *smax, const float *sref, int ny, int nx, float *data, uint32_t *dq) {
    if (!smax || !sref || !data || !dq || ny < 1 || nx < 1) return rip_fail(ctx, RIP_EINVAL, "cal_saturation: bad arguments");
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)ny * nx;
    DevBuf<float> a(ctx), b(ctx), o(ctx);
    DevBuf<uint32_t> q(ctx);
    int rc;
    if ((rc = a.upload(smax, n)) || (rc = b.upload(sref, n)) || (rc = o.alloc(n)) || (rc = q.alloc(n))) return rc;
    hipLaunchKernelGGL(calfiles_saturation_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, a.p, b.p, n, o.p, q.p);
    RIP_HIP(ctx, hipGetLastError());
    if ((rc = o.download(data, n)) || (rc = q.download(dq, n))) return rc;
    return dev_sync(ctx);
}

int rip_cal_mask(rip_ctx *ctx, int ny, int nx, int nb, const uint32_t *lin_dq, const float *pflat0, float pflat_median,
                 const float *dark_slope, const uint32_t *gain_dq, uint32_t *dq) {
    if (!lin_dq || !pflat0 || !dark_slope || !gain_dq || !dq || ny < 1 || nx < 1 || nb < 0 || ny > 65535)
        return rip_fail(ctx, RIP_EINVAL, "cal_mask: bad arguments");
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)ny * nx;
    DevBuf<uint32_t> l(ctx), g(ctx), o(ctx);
    DevBuf<float> p(ctx), d(ctx);
    int rc;
    if ((rc = l.upload(lin_dq, n)) || (rc = g.upload(gain_dq, n)) || (rc = p.upload(pflat0, n)) || (rc = d.upload(dark_slope, n)) ||
        (rc = o.alloc(n)))
        return rc;
    hipLaunchKernelGGL(calfiles_mask_kernel, dim3((nx + 255) / 256, ny), dim3(256), 0, ctx->stream, l.p, p.p, pflat_median, d.p, g.p, ny,
                       nx, nb, o.p);
    RIP_HIP(ctx, hipGetLastError());
    if ((rc = o.download(dq, n))) return rc;
    return dev_sync(ctx);
}
