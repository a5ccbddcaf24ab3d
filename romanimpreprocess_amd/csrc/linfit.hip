// The linearitylegendre file from flat and dark ramps: the step of the reference's runs/2026_July/make_sca_files_2026Jul.job that
// calls solid-waffle's linearity_run.  solid-waffle's source is not in the reference tree: the rule stated in include/romanhip.h
// and DESIGN.md section 7 IS the specification and parity with solid-waffle is unpinned.  Pinned by the reference are the call
// surface (the JSON of write_linearity_config.pl), the file's schema and what its consumers expect: phi(Sref) = 0,
// dphi/dS(Sref) = 1, pflat[0] the bright flat's rate.
//   rip_cal_frame_sums      one exposure cube added to the per-frame uint32 sums of its ramp set (a stream, exact)
//   rip_cal_linearity_fit   one lane per pixel: range, constrained Legendre least squares, rates and residuals, all in f64
// tests/linfit_ref.py restates both in numpy, operation by operation.
#include "rip_host.h"
#include "rip_samples.h"

namespace {

#define LF_MAX_SETS 8
#define LF_MAX_ORDER 10
#define LF_MAX_EXPOSURES 65536   // 65535 x 65536 still fits in uint32

// ------------------------------------------------------------------------------------------ frame sums
// One thread per 8 consecutive columns of one row of one frame (W8: one 16-byte load of samples; needs nx_file % 8 == 0 and a
// 16-byte aligned cube) or per column.  cube points at row y0 of frame f0; frames are `plane` samples apart.  vec_sums: the rows
// of sums start on 16 bytes (nx % 4 == 0, aligned base), so that a full vector is two 16-byte read-modify-writes.  Every word of
// sums belongs to exactly one thread: no atomics, and integer sums do not depend on any order.
template <bool W8>
__global__ __launch_bounds__(256) void frame_sums_kernel(const uint16_t *__restrict__ cube, size_t plane, int nx_file, int nframes,
                                                         int ny, int nx, int be16, int vec_sums, uint32_t *__restrict__ sums) {
    constexpr int V = W8 ? 8 : 1;
    const int nvec = (nx + V - 1) / V;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)nframes * ny * nvec) return;
    const size_t row = i / nvec;
    const int x0 = (int)(i - row * nvec) * V;
    const size_t f = row / ny, y = row - f * ny;
    uint32_t s[V];
    load_samples<V>(cube + f * plane + y * nx_file + x0, be16 != 0, s);
    add_results(sums + row * nx + x0, s, nx - x0, vec_sums != 0);
}

// ------------------------------------------------------------------------------------------ the fit
struct LfSets {
    const uint32_t *sums[LF_MAX_SETS];   // (nf, ny, nx) each
    int32_t n[LF_MAX_SETS];              // exposures summed
    int32_t i0[LF_MAX_SETS];             // first frame used (TSTART - 1)
    int32_t nf[LF_MAX_SETS];             // frames held
};

// P_l(z), l = 0 .. P, and with D also P_l'(z), by the three-term recurrences
template <int P, bool D>
__device__ __forceinline__ void lf_legendre(double z, double *Pl, double *dPl) {
    Pl[0] = 1.0;
    Pl[1] = z;
    if (D) {
        dPl[0] = 0.0;
        dPl[1] = 1.0;
    }
#pragma unroll
    for (int l = 2; l <= P; ++l) {
        const double t1 = ((double)(2 * l - 1) * z) * Pl[l - 1];
        const double t2 = (double)(l - 1) * Pl[l - 2];
        Pl[l] = (t1 - t2) / (double)l;
        if (D) dPl[l] = dPl[l - 2] + (double)(2 * l - 1) * Pl[l - 1];
    }
}

// One lane per pixel, order P (1..10), M = P - 1 free coefficients q_2 .. q_P.  The samples of a pixel are read four times (count,
// normal equations, regression of phi on [1, u], residuals): lanes of a wave read adjacent words of every frame.  Every operation
// is f64 and stands alone (-ffp-contract=off); tests/linfit_ref.py does the same operations in the same order.
template <int P>
__global__ __launch_bounds__(256) void linfit_kernel(const LfSets st, int nsets, const float *__restrict__ sref, int ny, int nx, int y0, int ny_frame,
                                                     int nb, double tframe, double slopecut, double negativepad, int bright, int dark,
                                                     float *__restrict__ data, float *__restrict__ smin_o, float *__restrict__ smax_o,
                                                     uint32_t *__restrict__ dq, float *__restrict__ pflat, float *__restrict__ dark_o,
                                                     uint16_t *__restrict__ ramperr, int32_t *__restrict__ cut_o) {
    constexpr int M = P - 1, MA = M > 0 ? M : 1;
    const size_t npix = (size_t)ny * nx;
    const size_t px = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (px >= npix) return;
    const int y = (int)(px / nx), x = (int)(px - (size_t)y * nx);
    auto mean = [&](int k, int i) -> double { return (double)st.sums[k][(size_t)i * npix + px] / (double)st.n[k]; };

    // the range: Smin from Sref, the cut and Smax from the bright set
    const double sr = (double)sref[px];
    const bool ok = sr - sr == 0.0;   // finite
    const double t = sr - negativepad;
    const float smin32 = (float)((ok && t > 0.0) ? t : 0.0);
    const int bi0 = st.i0[bright], blast = st.nf[bright] - 1;
    const int n0 = min(4, blast - bi0);
    const double D0 = (mean(bright, bi0 + n0) - mean(bright, bi0)) / (double)n0;
    const double thr = slopecut * D0;
    int cut = blast;
    double Mc;
    {
        double prev = mean(bright, bi0);
        Mc = prev;
        for (int i = bi0; i < blast; ++i) {
            const double next = mean(bright, i + 1);
            if (next - prev < thr) {
                cut = i;
                break;
            }
            prev = next;
            Mc = next;
        }
    }
    const double v = Mc < 65535.0 ? Mc : 65535.0;
    float smax32 = (float)v;
    if ((double)smax32 < v) smax32 = __uint_as_float(__float_as_uint(smax32) + 1u);   // rounded UP: the sample at the cut is in range (v >= 0)
    const double smin = (double)smin32, smax = (double)smax32;
    const double h = (smax - smin) / 2.0;
    const double zref = (sr - smin) / h - 1.0;
    bool bad = !(D0 > 0.0) || !ok || sr >= smax || !(smax > smin);
    const bool border = y + y0 < nb || y + y0 >= ny_frame - nb || x < nb || x >= nx - nb;
    const int nlit = dark >= 0 ? nsets - 1 : nsets;
    smin_o[px] = smin32;
    smax_o[px] = smax32;
    cut_o[px] = cut;

    // a flagged pixel carries the identity phi = S - Sref and zeros
    auto identity = [&](uint32_t flag) {
        data[px] = ok ? (float)((smin + smax) / 2.0 - sr) : __uint_as_float(0x7FC00000u);
        data[npix + px] = (float)h;
        for (int l = 2; l <= P; ++l) data[(size_t)l * npix + px] = 0.0f;
        for (int j = 0; j < nlit; ++j) pflat[(size_t)j * npix + px] = 0.0f;
        for (int k = 0; k < nsets; ++k) ramperr[(size_t)k * npix + px] = 0;
        dark_o[px] = 0.0f;
        dq[px] = flag;
    };
    if (border) return identity(DQ_REFERENCE_PIXEL);
    if (bad) return identity(DQ_NO_LIN_CORR);

    auto used = [&](int k, int i, double Mi) -> bool { return Mi >= smin && Mi <= smax && (k != bright || i <= cut); };
    auto uval = [&](int k, int i) -> double { return (double)(2 * (i - st.i0[k])) / (double)(st.nf[k] - st.i0[k] - 1) - 1.0; };

    // pass 0: the used samples of every set; a set with fewer than two takes no part
    uint32_t part = 0;
    int dof = 0;
    for (int k = 0; k < nsets; ++k) {
        int c = 0;
        for (int i = st.i0[k]; i < st.nf[k]; ++i) c += used(k, i, mean(k, i)) ? 1 : 0;
        if (c >= 2) {
            part |= 1u << k;
            dof += c - 2;
        }
    }
    if (dof < M) return identity(DQ_NO_LIN_CORR);

    double Pr[P + 1], dPr[P + 1];
    lf_legendre<P, true>(zref, Pr, dPr);
    // B_2 .. B_P at a sample: the Legendre polynomials with their value and slope at Sref taken out
    auto basis = [&](double Mi, double *B) {
        const double z = (Mi - smin) / h - 1.0;
        double Pl[P + 1];
        lf_legendre<P, false>(z, Pl, nullptr);
        const double dz = z - zref;
#pragma unroll
        for (int a = 0; a < M; ++a) B[a] = (Pl[a + 2] - Pr[a + 2]) - dPr[a + 2] * dz;
    };

    // pass 1: the normal matrix (lower triangle, row a at a (a + 1) / 2) and right-hand side, [1, u] projected out per set
    double N[MA * (MA + 1) / 2], c[MA];
#pragma unroll
    for (int a = 0; a < MA * (MA + 1) / 2; ++a) N[a] = 0.0;
#pragma unroll
    for (int a = 0; a < MA; ++a) c[a] = 0.0;
    if (M > 0) {
        for (int k = 0; k < nsets; ++k) {
            if (!(part >> k & 1u)) continue;
            double S1 = 0.0, Su = 0.0, Suu = 0.0, Sy = 0.0, Suy = 0.0, s[MA], tt[MA];
#pragma unroll
            for (int a = 0; a < MA; ++a) s[a] = tt[a] = 0.0;
            for (int i = st.i0[k]; i < st.nf[k]; ++i) {
                const double Mi = mean(k, i);
                if (!used(k, i, Mi)) continue;
                const double u = uval(k, i), yy = Mi - sr;
                double B[MA];
                basis(Mi, B);
                S1 = S1 + 1.0;
                Su = Su + u;
                Suu = Suu + u * u;
                Sy = Sy + yy;
                Suy = Suy + u * yy;
#pragma unroll
                for (int a = 0; a < M; ++a) {
                    s[a] = s[a] + B[a];
                    tt[a] = tt[a] + u * B[a];
                    c[a] = c[a] + B[a] * yy;
#pragma unroll
                    for (int b = 0; b <= a; ++b) N[a * (a + 1) / 2 + b] = N[a * (a + 1) / 2 + b] + B[a] * B[b];
                }
            }
            const double det = S1 * Suu - Su * Su;
            const double ay = (Suu * Sy - Su * Suy) / det, by = (S1 * Suy - Su * Sy) / det;
#pragma unroll
            for (int a = 0; a < M; ++a) {
                const double al = (Suu * s[a] - Su * tt[a]) / det, be = (S1 * tt[a] - Su * s[a]) / det;
                c[a] = c[a] - (s[a] * ay + tt[a] * by);
#pragma unroll
                for (int b = a; b < M; ++b) N[b * (b + 1) / 2 + a] = N[b * (b + 1) / 2 + a] - (s[b] * al + tt[b] * be);
            }
        }
    }

    // Cholesky in place, forward and back substitution
    double q[MA];
#pragma unroll
    for (int j = 0; j < M; ++j) {
        double d = N[j * (j + 1) / 2 + j];
#pragma unroll
        for (int r = 0; r < j; ++r) d = d - N[j * (j + 1) / 2 + r] * N[j * (j + 1) / 2 + r];
        if (!(d > 0.0 && d < __builtin_inf())) bad = true;
        const double ljj = sqrt(d);
        N[j * (j + 1) / 2 + j] = ljj;
#pragma unroll
        for (int i = j + 1; i < M; ++i) {
            double e = N[i * (i + 1) / 2 + j];
#pragma unroll
            for (int r = 0; r < j; ++r) e = e - N[i * (i + 1) / 2 + r] * N[j * (j + 1) / 2 + r];
            N[i * (i + 1) / 2 + j] = e / ljj;
        }
    }
    if (bad) return identity(DQ_NO_LIN_CORR);
#pragma unroll
    for (int j = 0; j < M; ++j) {
        double e = 0.0 - c[j];
#pragma unroll
        for (int r = 0; r < j; ++r) e = e - N[j * (j + 1) / 2 + r] * c[r];
        c[j] = e / N[j * (j + 1) / 2 + j];
    }
#pragma unroll
    for (int j = M - 1; j >= 0; --j) {
        double e = c[j];
#pragma unroll
        for (int r = j + 1; r < M; ++r) e = e - N[r * (r + 1) / 2 + j] * q[r];
        q[j] = e / N[j * (j + 1) / 2 + j];
    }

    // the stored coefficients: the series in P_l(z) over [Smin, Smax]
    {
        double sumA = 0.0, sumB = 0.0;
#pragma unroll
        for (int a = 0; a < M; ++a) {
            sumA = sumA + q[a] * dPr[a + 2];
            sumB = sumB + q[a] * (Pr[a + 2] - dPr[a + 2] * zref);
        }
        data[px] = (float)((0.0 - h * zref) - sumB);
        data[npix + px] = (float)(h - sumA);
#pragma unroll
        for (int a = 0; a < M; ++a) data[(size_t)(a + 2) * npix + px] = (float)q[a];
    }

    // passes 2 and 3 per set, the dark one first: a_k, r_k by regression of phi(M) on [1, u], then the largest residual
    double rdark = 0.0;
    for (int j = 0; j < nsets; ++j) {
        const int k = dark < 0 ? j : (j == 0 ? dark : (j - 1 < dark ? j - 1 : j));
        const int slot = k == dark ? -1 : (dark >= 0 && k > dark ? k - 1 : k);
        double rate = 0.0;
        uint16_t err = 0;
        const bool in = (part >> k & 1u) != 0;
        if (in) {
            auto phi = [&](double Mi) -> double {
                double B[MA];
                basis(Mi, B);
                double ph = Mi - sr;
#pragma unroll
                for (int a = 0; a < M; ++a) ph = ph + q[a] * B[a];
                return ph;
            };
            double S1 = 0.0, Su = 0.0, Suu = 0.0, Sw = 0.0, Suw = 0.0;
            for (int i = st.i0[k]; i < st.nf[k]; ++i) {
                const double Mi = mean(k, i);
                if (!used(k, i, Mi)) continue;
                const double u = uval(k, i), ph = phi(Mi);
                S1 = S1 + 1.0;
                Su = Su + u;
                Suu = Suu + u * u;
                Sw = Sw + ph;
                Suw = Suw + u * ph;
            }
            const double det = S1 * Suu - Su * Su;
            const double ak = (Suu * Sw - Su * Suw) / det, rk = (S1 * Suw - Su * Sw) / det;
            double e = 0.0;
            for (int i = st.i0[k]; i < st.nf[k]; ++i) {
                const double Mi = mean(k, i);
                if (!used(k, i, Mi)) continue;
                const double res = fabs(phi(Mi) - (ak + rk * uval(k, i)));
                if (res > e) e = res;
            }
            rate = (rk * 2.0) / ((double)(st.nf[k] - st.i0[k] - 1) * tframe);
            err = (uint16_t)(e < 65535.0 ? ceil(e) : 65535.0);
        }
        ramperr[(size_t)k * npix + px] = err;
        if (slot < 0) {
            rdark = rate;
            dark_o[px] = (float)rate;
        } else {
            pflat[(size_t)slot * npix + px] = in ? (float)(rate - rdark) : 0.0f;
        }
    }
    if (dark < 0) dark_o[px] = 0.0f;
    dq[px] = 0u;
}

template <int P>
void lf_launch(rip_ctx *ctx, size_t npix, const LfSets &st, int nsets, const float *sref, int ny, int nx, int y0, int ny_frame, int nb,
               double tframe,
               double slopecut, double negativepad, int bright, int dark, float *data, float *smin, float *smax, uint32_t *dq, float *pflat,
               float *dark_o, uint16_t *ramperr, int32_t *cut) {
    hipLaunchKernelGGL(linfit_kernel<P>, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, ctx->stream, st, nsets, sref, ny, nx, y0,
                       ny_frame, nb,                       tframe, slopecut, negativepad, bright, dark, data, smin, smax, dq, pflat, dark_o, ramperr, cut);
}

}   // namespace

// ============================================================================================ C-ABI

int rip_cal_frame_sums(rip_ctx *ctx, const uint16_t *cube, int location, int nreads, int ny_file, int nx_file, int y0, int ny, int nx,
                       int f0, int fits_be16, uint32_t *sums, int count) {
    if (!cube || !sums) return rip_fail(ctx, RIP_EINVAL, "cal_frame_sums: a required array is NULL");
    if (const int rc = rip_check_location(ctx, "cal_frame_sums", "location", location)) return rc;
    if (count < 0 || count >= LF_MAX_EXPOSURES)
        return rip_fail(ctx, RIP_EINVAL, "cal_frame_sums: exposure %d of a set (at most %d: the sums are uint32)", count + 1, LF_MAX_EXPOSURES);
    if (nreads < 1 || ny_file < 1 || nx_file < 1 || ny < 1 || nx < 1 || y0 < 0 || (int64_t)y0 + ny > ny_file)
        return rip_fail(ctx, RIP_EINVAL, "cal_frame_sums: rows %d+%d of a (%d,%d,%d) cube", y0, ny, nreads, ny_file, nx_file);
    if (nx > nx_file) return rip_fail(ctx, RIP_EINVAL, "cal_frame_sums: %d columns wanted of a frame of %d", nx, nx_file);
    if (f0 < 0 || f0 >= nreads) return rip_fail(ctx, RIP_EINVAL, "cal_frame_sums: first frame %d outside the %d frames of the cube", f0, nreads);
    const int nframes = nreads - f0;
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    CubeBand band(ctx);
    if (const int rc = band.in(cube, location, ny_file, nx_file, f0, nframes, y0, ny)) return rc;
    const bool w8 = nx_file % 8 == 0 && aligned(band.p, 16);
    const int vec_sums = nx % 4 == 0 && aligned(sums, 16);
    const size_t threads = (size_t)nframes * ny * (w8 ? (nx + 7) / 8 : nx);
    if ((threads + 255) / 256 > 0x7FFFFFFFu) return rip_fail(ctx, RIP_EINVAL, "cal_frame_sums: a (%d,%d,%d) set is too large", nframes, ny, nx);
    const dim3 grid((unsigned)((threads + 255) / 256));
    RIP_LAUNCH_W8(frame_sums_kernel, w8, grid, dim3(256), 0, ctx->stream, band.p, band.plane, nx_file, nframes, ny, nx, fits_be16, vec_sums,
                  sums);
    RIP_HIP(ctx, hipGetLastError());
    return dev_sync(ctx);
}

int rip_cal_linearity_fit(rip_ctx *ctx, int nsets, const uint32_t **sums, const int32_t *counts, const int32_t *first,
                          const int32_t *nframes, const float *sref, int ny, int nx, int y0, int ny_frame, int nb, int p_order, int sign, double tframe,
                          double slopecut, double negativepad, int bright, int dark, float *data, float *smin, float *smax, uint32_t *dq,
                          float *pflat, float *dark_rate, uint16_t *ramperr, int32_t *cut) {
    if (p_order < 1 || p_order > LF_MAX_ORDER)
        return rip_fail(ctx, RIP_EINVAL, "cal_linearity_fit: P_ORDER %d (1..%d supported)", p_order, LF_MAX_ORDER);
    if (sign != 1) return rip_fail(ctx, RIP_EINVAL, "cal_linearity_fit: SIGN %d (only 1, an increasing ramp, is supported)", sign);
    if (!(slopecut > 0.0 && slopecut < 1.0)) return rip_fail(ctx, RIP_EINVAL, "cal_linearity_fit: SLOPECUT %g (must lie in (0, 1))", slopecut);
    if (nsets < 1 || nsets > LF_MAX_SETS) return rip_fail(ctx, RIP_EINVAL, "cal_linearity_fit: RAMPS holds %d sets (1..%d supported)", nsets, LF_MAX_SETS);
    if (dark < -1 || dark >= nsets) return rip_fail(ctx, RIP_EINVAL, "cal_linearity_fit: DARK %d outside the %d sets of RAMPS", dark, nsets);
    if (bright < 0 || bright >= nsets || bright == dark)
        return rip_fail(ctx, RIP_EINVAL, "cal_linearity_fit: bright set %d outside the %d sets of RAMPS (or the dark one)", bright, nsets);
    if (!sums || !counts || !first || !nframes || !sref || !data || !smin || !smax || !dq || !pflat || !dark_rate || !ramperr || !cut)
        return rip_fail(ctx, RIP_EINVAL, "cal_linearity_fit: a required array is NULL");
    if (ny < 1 || nx < 1 || nb < 0 || y0 < 0 || (int64_t)y0 + ny > ny_frame)
        return rip_fail(ctx, RIP_EINVAL, "cal_linearity_fit: rows %d+%d of a %d x %d frame with a border of %d", y0, ny, ny_frame, nx, nb);
    if (!(tframe > 0.0 && tframe < __builtin_inf()) || !(negativepad >= 0.0 && negativepad < __builtin_inf()))
        return rip_fail(ctx, RIP_EINVAL, "cal_linearity_fit: TFRAME %g, NEGATIVEPAD %g (positive; not negative; finite)", tframe, negativepad);
    LfSets st{};
    for (int k = 0; k < nsets; ++k) {
        if (!sums[k]) return rip_fail(ctx, RIP_EINVAL, "cal_linearity_fit: the sums of set %d are NULL", k);
        if (counts[k] < 1 || counts[k] > LF_MAX_EXPOSURES)
            return rip_fail(ctx, RIP_EINVAL, "cal_linearity_fit: NRAMP %d of set %d (1..%d supported)", counts[k], k, LF_MAX_EXPOSURES);
        if (first[k] < 0 || (int64_t)nframes[k] - first[k] < 2)
            return rip_fail(ctx, RIP_EINVAL, "cal_linearity_fit: TSTART %d leaves fewer than 2 of the %d frames of set %d", first[k] + 1,
                            nframes[k], k);
        st.sums[k] = sums[k];
        st.n[k] = counts[k];
        st.i0[k] = first[k];
        st.nf[k] = nframes[k];
    }
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)ny * nx;
#define LF_CASE(P)                                                                                                                  \
    case P:                                                                                                                         \
        lf_launch<P>(ctx, npix, st, nsets, sref, ny, nx, y0, ny_frame, nb, tframe, slopecut, negativepad, bright, dark, data, smin, smax, dq, pflat, \
                     dark_rate, ramperr, cut);                                                                                      \
        break;
    switch (p_order) {
        LF_CASE(1) LF_CASE(2) LF_CASE(3) LF_CASE(4) LF_CASE(5) LF_CASE(6) LF_CASE(7) LF_CASE(8) LF_CASE(9) LF_CASE(10)
    }
#undef LF_CASE
    RIP_HIP(ctx, hipGetLastError());
    return dev_sync(ctx);
}
