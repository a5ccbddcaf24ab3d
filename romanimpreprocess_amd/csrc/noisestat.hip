// Noise summary of a dark set: the step of the reference's runs/2026_July/make_sca_files_2026Jul.job that calls solid-waffle's
// noise_run (line 76) and whose output make_dark_file.py reads (DARK1 .. RESET, ACN, C_PINK, U_PINK, AMP33).  solid-waffle's
// source is not in the reference tree: the rule stated in include/romanhip.h and DESIGN.md section 7 IS the specification and
// parity with solid-waffle is unpinned.  What pins the estimator is the reference's own generator (sim_to_isim.py:306-402): the
// parameters are defined as the inverse of that noise model and tested by round trip.
//   rip_cal_noise_add       one dark exposure, read once: integer per-pixel accumulators and the row sums of its frames
//   rip_cal_noise_rowstats  the row sums of one exposure into f64 moment tables of Haar differences, in exposure order
//   rip_cal_noise_planes    the six per-pixel planes and the reference-output planes, one lane per pixel in f64
// tests/noise_run_ref.py restates all three in numpy, operation by operation.
// Bounds (x <= 65535, n <= 64 frames, N <= 512 exposures): |S| = |sum (2i - (n-1)) x_i| <= 65535 n^2 / 2, so 512 S^2 <= 2^63.1 fits
// in u64; sum d^2 <= 63 * 65535^2 per exposure, 512 of them 2^47; the reference-output sum 512 * 64 * 65535 < 2^31.
#include "rip_host.h"
#include "rip_samples.h"

namespace {

#define NS_MAX_FRAMES 64
#define NS_MAX_EXPOSURES 512
#define NS_MAX_CW 256     // the lanes of a channel sit in one workgroup
#define NS_MIN_ROWS 128
#define NS_MAX_SCALE 6
#define NS_CHUNK 8        // frames between two meetings of the workgroup

struct NsAcc {
    uint32_t *a0;
    uint64_t *a1;
    int32_t *b0;
    uint64_t *b1;
    int64_t *s0;
    uint64_t *s1;
    int32_t *c0;
    uint64_t *c1;
    uint32_t *m33;
};

// A segment is one channel of one row: cw pixels, L = cw / V lanes (V = 8 pixels per lane with W8, one 16-byte load per frame; else
// 1).  Segments are numbered seg = y * nch + c; a workgroup takes CB = 256 / L consecutive ones, so the lanes of a channel never
// straddle two workgroups, and pixel (y, x) of the accumulators (rows of nch * cw words) is word seg * cw + lane * V: the lanes of
// a workgroup read and write consecutive words.  cube points at frame f0; frames are `plane` samples apart.
// Per lane the running x_prev, S and sum d^2 live in registers over the n frames and the accumulators get one read-modify-write.
// Row sums: every lane leaves its (even, odd) column sums of a frame in LDS; every NS_CHUNK frames the workgroup meets and one
// lane per (frame, segment, parity) adds the L words up -- integers, any order -- and stores the sum: no atomics, every word of
// rowsum has one writer.  n is the same for all lanes, so every lane reaches every barrier (dead lanes included).
template <bool W8>
__global__ __launch_bounds__(256) void noise_add_kernel(const uint16_t *__restrict__ cube, size_t plane, int nx_file, int n, int nch, int C,
                                                        int cw, int ref_out, unsigned nseg, int CB, int be16, const NsAcc acc,
                                                        uint32_t *__restrict__ rowsum) {
    constexpr int V = W8 ? 8 : 1;
    __shared__ uint2 part[NS_CHUNK][256];
    const int L = cw / V;
    const int tid = threadIdx.x;
    const int sc = tid / L, lane = tid - sc * L;
    const size_t seg0 = (size_t)blockIdx.x * CB;
    const size_t seg = seg0 + sc;
    const bool live = sc < CB && seg < nseg;
    const size_t y = live ? seg / nch : 0;
    const int c = live ? (int)(seg - y * nch) : 0;
    const uint16_t *src = cube + y * nx_file + (size_t)c * cw + (size_t)lane * V;
    const int stored = be16 != 0;
    const bool odd = (lane & 1) != 0;   // one-pixel form: cw is even, so the column's parity is the lane's

    uint32_t xf[V], xp[V], m[V];
    int32_t d0[V];
    int64_t S[V];
    uint64_t q[V];
#pragma unroll
    for (int k = 0; k < V; ++k) xf[k] = xp[k] = m[k] = 0u, d0[k] = 0, S[k] = 0, q[k] = 0u;

    for (int i = 0; i < n; ++i) {
        uint32_t x[V];
        if (live) {
            load_samples<V>(src + (size_t)i * plane, stored, x);
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) x[k] = 0u;
        }
        uint32_t pe, po;
        if constexpr (W8) {
            pe = (x[0] + x[2]) + (x[4] + x[6]);
            po = (x[1] + x[3]) + (x[5] + x[7]);
        } else {
            pe = odd ? 0u : x[0];
            po = odd ? x[0] : 0u;
        }
        part[i % NS_CHUNK][tid] = make_uint2(pe, po);
        const int64_t wgt = 2 * i - (n - 1);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (i == 0) {
                xf[k] = x[k];
            } else {
                const int32_t d = (int32_t)x[k] - (int32_t)xp[k];
                if (i == 1) d0[k] = d;
                q[k] += (uint64_t)((int64_t)d * d);
            }
            S[k] += wgt * (int64_t)x[k];
            m[k] += x[k];
            xp[k] = x[k];
        }
        if (i % NS_CHUNK == NS_CHUNK - 1 || i == n - 1) {
            __syncthreads();
            const int i0 = i - i % NS_CHUNK, nf = i % NS_CHUNK + 1;
            for (int o = tid; o < nf * CB * 2; o += 256) {
                const int fi = o / (2 * CB), r = o - fi * 2 * CB, s2 = r >> 1, p = r & 1;
                if (seg0 + s2 < nseg) {
                    uint32_t sum = 0u;
                    for (int l = 0; l < L; ++l) {
                        int l2 = l + s2 % L;   // rotated: neighbouring segments start on different LDS banks
                        if (l2 >= L) l2 -= L;
                        const uint2 v = part[fi][s2 * L + l2];
                        sum += p ? v.y : v.x;
                    }
                    rowsum[((size_t)(i0 + fi) * nseg + seg0 + s2) * 2 + p] = sum;
                }
            }
            __syncthreads();
        }
    }
    if (!live) return;

    const size_t px = seg * cw + (size_t)lane * V;
    uint64_t a1[V], b1[V], s1[V];
    int32_t c0[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        a1[k] = (uint64_t)xf[k] * xf[k];
        b1[k] = (uint64_t)((int64_t)d0[k] * d0[k]);
        s1[k] = (uint64_t)(S[k] * S[k]);
        c0[k] = (int32_t)xp[k] - (int32_t)xf[k];
    }
    add_results(acc.a0 + px, xf);
    add_results(acc.a1 + px, a1);
    add_results(acc.b0 + px, d0);
    add_results(acc.b1 + px, b1);
    add_results(acc.s0 + px, S);
    add_results(acc.s1 + px, s1);
    add_results(acc.c0 + px, c0);
    add_results(acc.c1 + px, q);
    if (ref_out && c == C) add_results(acc.m33 + y * cw + (size_t)lane * V, m);
}

// ------------------------------------------------------------------------------------------ moment tables of the row sums
// rs (n, ny, nch, 2) u32.  D_k[y][c] = (rs[k+1][y][c][0] + rs[k+1][y][c][1]) - (rs[k][y][c][0] + rs[k][y][c][1]) as i64.
__device__ __forceinline__ int64_t ns_cds_row(const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi, size_t at) {
    const uint2 a = *reinterpret_cast<const uint2 *>(lo + at), b = *reinterpret_cast<const uint2 *>(hi + at);
    return ((int64_t)b.x + (int64_t)b.y) - ((int64_t)a.x + (int64_t)a.y);
}

// One thread per (k, j, b): the scales j = 0 .. J are laid end to end, nbt = sum_j (ny >> (j+1)) blocks in all.  The thread walks
// the channels; every table word has one writer and is updated once per exposure: the f64 sums run in exposure order.
__global__ __launch_bounds__(256) void rowstats_kernel(const uint32_t *__restrict__ rs, int n, int ny, int nch, int C, int J, int nbt,
                                                       double *__restrict__ h1, double *__restrict__ h2, double *__restrict__ t1,
                                                       double *__restrict__ t2, double *__restrict__ ht) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)(n - 1) * nbt) return;
    const int k = (int)(idx / nbt);
    int b = (int)(idx - (size_t)k * nbt), j = 0;
    while (j < J && b >= (ny >> (j + 1))) {
        b -= ny >> (j + 1);
        ++j;
    }
    const int len = 1 << j, r0 = 2 * b * len;
    const size_t frame = (size_t)ny * nch * 2;
    const uint32_t *lo = rs + (size_t)k * frame, *hi = lo + frame;
    int64_t T = 0, HC = 0;
    for (int c = 0; c < nch; ++c) {
        int64_t H = 0;
        for (int y = 0; y < len; ++y)
            H += ns_cds_row(lo, hi, ((size_t)(r0 + y) * nch + c) * 2) - ns_cds_row(lo, hi, ((size_t)(r0 + len + y) * nch + c) * 2);
        const size_t e = idx * nch + c;
        const double h = (double)H;
        h1[e] = h1[e] + h;
        h2[e] = h2[e] + h * h;
        if (c < C)
            T += H;
        else
            HC = H;
    }
    const double t = (double)T;
    t1[idx] = t1[idx] + t;
    t2[idx] = t2[idx] + t * t;
    if (ht) ht[idx] = ht[idx] + (double)HC * t;
}

// Q[k][c]: the even-column sum minus the odd-column sum of CDS pair k over the whole frame of channel c.  One wave per (k, c);
// the lanes' partial sums are integers and meet by shuffles.
__global__ __launch_bounds__(64) void rowstats_q_kernel(const uint32_t *__restrict__ rs, int ny, int nch, double *__restrict__ q1,
                                                        double *__restrict__ q2) {
    const int k = blockIdx.x / nch, c = blockIdx.x - k * nch;
    const size_t frame = (size_t)ny * nch * 2;
    const uint32_t *lo = rs + (size_t)k * frame, *hi = lo + frame;
    long long Q = 0;
    for (int y = threadIdx.x; y < ny; y += 64) {
        const size_t at = ((size_t)y * nch + c) * 2;
        const uint2 a = *reinterpret_cast<const uint2 *>(lo + at), b = *reinterpret_cast<const uint2 *>(hi + at);
        Q += ((long long)b.x - (long long)a.x) - ((long long)b.y - (long long)a.y);
    }
    for (int off = 32; off > 0; off >>= 1) Q += __shfl_xor(Q, off, 64);
    if (threadIdx.x == 0) {
        const double v = (double)Q;
        q1[blockIdx.x] = q1[blockIdx.x] + v;
        q2[blockIdx.x] = q2[blockIdx.x] + v * v;
    }
}

// ------------------------------------------------------------------------------------------ the planes
__device__ __forceinline__ double ns_var(double q, double s, double m) {
    const double v = (q - s * s / m) / (m - 1.0);
    return v > 0.0 ? v : 0.0;
}

// One lane per pixel of the (ny, nch * cw) accumulators; every operation is f64 and stands alone (-ffp-contract=off), results are
// rounded once to f32.  Science columns go to the six planes (ny, nx); reference-output columns to amp33 (2, ny, cw).
__global__ __launch_bounds__(256) void noise_planes_kernel(const NsAcc acc, int N, int n, int ny, int nx, int cw, int ref_out, double tframe,
                                                           double root2, float *__restrict__ planes, float *__restrict__ amp33) {
    const int nxt = nx + (ref_out ? cw : 0);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)ny * nxt) return;
    const size_t y = i / nxt;
    const int x = (int)(i - y * nxt);
    const double dN = (double)N, ntot = (double)((int64_t)N * (n - 1));
    const float cds = (float)sqrt(ns_var((double)acc.c1[i], (double)acc.c0[i], ntot));
    if (x >= nx) {
        const size_t o = y * cw + (x - nx), np33 = (size_t)ny * cw;
        amp33[o] = (float)((double)acc.m33[o] / (dN * (double)n));
        amp33[np33 + o] = (float)((double)cds / root2);
        return;
    }
    const double nn = (double)((int64_t)n * ((int64_t)n * n - 1));
    const size_t o = y * nx + x, np = (size_t)ny * nx;
    const double b0 = (double)acc.b0[i], s0 = (double)acc.s0[i];
    planes[o] = (float)(b0 / (dN * tframe));
    planes[np + o] = (float)(sqrt(ns_var((double)acc.b1[i], b0, dN) / dN) / tframe);
    planes[2 * np + o] = (float)((6.0 * s0) / ((dN * nn) * tframe));
    planes[3 * np + o] = (float)((6.0 * sqrt(ns_var((double)acc.s1[i], s0, dN) / dN)) / (nn * tframe));
    planes[4 * np + o] = cds;
    planes[5 * np + o] = (float)sqrt(ns_var((double)acc.a1[i], (double)acc.a0[i], dN));
}

int ns_scales(int ny) {   // J = min(6, floor(log2(ny / 64)))
    int J = 0;
    while (J < NS_MAX_SCALE && (ny >> (J + 1)) >= 64) ++J;
    return J;
}

}   // namespace

// ============================================================================================ C-ABI

int rip_cal_noise_add(rip_ctx *ctx, const uint16_t *cube, int location, int nreads, int ny, int nx_file, int C, int cw, int ref_out, int f0,
                      int n, int fits_be16, int count, uint32_t *a0, uint64_t *a1, int32_t *b0, uint64_t *b1, int64_t *s0, uint64_t *s1,
                      int32_t *c0, uint64_t *c1, uint32_t *m33, uint32_t *rowsum) {
    if (!cube || !a0 || !a1 || !b0 || !b1 || !s0 || !s1 || !c0 || !c1 || !rowsum || (ref_out && !m33))
        return rip_fail(ctx, RIP_EINVAL, "cal_noise_add: a required array is NULL");
    if (const int rc = rip_check_location(ctx, "cal_noise_add", "location", location)) return rc;
    if (n < 2 || n > NS_MAX_FRAMES) return rip_fail(ctx, RIP_EINVAL, "cal_noise_add: -tn %d frames (2..%d supported)", n, NS_MAX_FRAMES);
    if (count < 0 || count >= NS_MAX_EXPOSURES)
        return rip_fail(ctx, RIP_EINVAL, "cal_noise_add: exposure %d of a set (at most %d: the sums of squares are uint64)", count + 1,
                        NS_MAX_EXPOSURES);
    if (nreads < 1 || f0 < 0 || (int64_t)f0 + n > nreads)
        return rip_fail(ctx, RIP_EINVAL, "cal_noise_add: -t %d and -tn %d ask for the frames %d..%d of a cube of %d", f0 + 1, n, f0 + 1, f0 + n,
                        nreads);
    if (cw < 2 || cw % 2 != 0 || cw > NS_MAX_CW)
        return rip_fail(ctx, RIP_EINVAL, "cal_noise_add: channel width %d (even, 2..%d)", cw, NS_MAX_CW);
    if (ny < NS_MIN_ROWS) return rip_fail(ctx, RIP_EINVAL, "cal_noise_add: %d rows (at least %d: scale 0 needs 64 blocks)", ny, NS_MIN_ROWS);
    const int64_t nch = (int64_t)C + (ref_out ? 1 : 0), nxt = nch * cw;
    if (C < 1 || nx_file < 1 || nxt > nx_file)
        return rip_fail(ctx, RIP_EINVAL, "cal_noise_add: %d channels of %d columns%s wanted of a frame of %d", C, cw,
                        ref_out ? " and the reference output" : "", nx_file);
    const int64_t nseg = (int64_t)ny * nch;
    if (nseg > 0x7FFFFFFF) return rip_fail(ctx, RIP_EINVAL, "cal_noise_add: a (%d,%ld) frame is too large", ny, (long)nxt);
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    CubeBand band(ctx);   // (the whole rows of the frames that are used)
    if (const int rc = band.in(cube, location, ny, nx_file, f0, n, 0, ny)) return rc;
    const bool w8 = nx_file % 8 == 0 && cw % 8 == 0 && aligned(band.p, 16) && aligned(a0, 16) && aligned(a1, 16) && aligned(b0, 16) &&
                    aligned(b1, 16) && aligned(s0, 16) && aligned(s1, 16) && aligned(c0, 16) && aligned(c1, 16) && aligned(m33, 16);
    const int L = w8 ? cw / 8 : cw, CB = 256 / L;
    const NsAcc acc{a0, a1, b0, b1, s0, s1, c0, c1, m33};
    const dim3 grid((unsigned)((nseg + CB - 1) / CB));
    RIP_LAUNCH_W8(noise_add_kernel, w8, grid, dim3(256), 0, ctx->stream, band.p, band.plane, nx_file, n, (int)nch, C, cw, ref_out,
                  (unsigned)nseg, CB, fits_be16, acc, rowsum);
    RIP_HIP(ctx, hipGetLastError());
    return dev_sync(ctx);
}

int rip_cal_noise_rowstats(rip_ctx *ctx, const uint32_t *rowsum, int n, int ny, int C, int ref_out, double *h1, double *h2, double *t1,
                           double *t2, double *ht, double *q1, double *q2) {
    if (!rowsum || !h1 || !h2 || !t1 || !t2 || !q1 || !q2 || (ref_out && !ht))
        return rip_fail(ctx, RIP_EINVAL, "cal_noise_rowstats: a required array is NULL");
    if (n < 2 || n > NS_MAX_FRAMES) return rip_fail(ctx, RIP_EINVAL, "cal_noise_rowstats: -tn %d frames (2..%d supported)", n, NS_MAX_FRAMES);
    if (ny < NS_MIN_ROWS || C < 1 || (int64_t)ny * ((int64_t)C + 1) > 0x7FFFFFFF)
        return rip_fail(ctx, RIP_EINVAL, "cal_noise_rowstats: %d rows of %d channels (at least %d rows)", ny, C, NS_MIN_ROWS);
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const int nch = C + (ref_out ? 1 : 0), J = ns_scales(ny);
    int nbt = 0;
    for (int j = 0; j <= J; ++j) nbt += ny >> (j + 1);
    const size_t threads = (size_t)(n - 1) * nbt;
    hipLaunchKernelGGL(rowstats_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx->stream, rowsum, n, ny, nch, C, J, nbt, h1,
                       h2, t1, t2, ref_out ? ht : nullptr);
    RIP_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(rowstats_q_kernel, dim3((unsigned)((n - 1) * nch)), dim3(64), 0, ctx->stream, rowsum, ny, nch, q1, q2);
    RIP_HIP(ctx, hipGetLastError());
    return dev_sync(ctx);
}

int rip_cal_noise_planes(rip_ctx *ctx, const uint32_t *a0, const uint64_t *a1, const int32_t *b0, const uint64_t *b1, const int64_t *s0,
                         const uint64_t *s1, const int32_t *c0, const uint64_t *c1, const uint32_t *m33, int nexp, int n, int ny, int C,
                         int cw, int ref_out, double tframe, int location, float *planes, float *amp33) {
    if (!a0 || !a1 || !b0 || !b1 || !s0 || !s1 || !c0 || !c1 || !planes || (ref_out && (!m33 || !amp33)))
        return rip_fail(ctx, RIP_EINVAL, "cal_noise_planes: a required array is NULL");
    if (const int rc = rip_check_location(ctx, "cal_noise_planes", "location", location)) return rc;
    if (nexp < 2 || nexp > NS_MAX_EXPOSURES)
        return rip_fail(ctx, RIP_EINVAL, "cal_noise_planes: -n %d exposures (2..%d: a variance over exposures needs two)", nexp, NS_MAX_EXPOSURES);
    if (n < 2 || n > NS_MAX_FRAMES) return rip_fail(ctx, RIP_EINVAL, "cal_noise_planes: -tn %d frames (2..%d supported)", n, NS_MAX_FRAMES);
    if (!(tframe > 0.0 && tframe < __builtin_inf())) return rip_fail(ctx, RIP_EINVAL, "cal_noise_planes: tframe %g (positive, finite)", tframe);
    const int64_t nx = (int64_t)C * cw, nxt = nx + (ref_out ? cw : 0);
    if (ny < 1 || C < 1 || cw < 1 || nxt > 0x7FFFFFFF || (int64_t)ny * nxt > ((int64_t)0x7FFFFFFF << 8))
        return rip_fail(ctx, RIP_EINVAL, "cal_noise_planes: %d rows of %d channels of %d columns", ny, C, cw);
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)ny * nx, n33 = ref_out ? (size_t)ny * cw : 0;
    DevArg<float> p, r;
    int rc;
    if ((rc = p.out(ctx, planes, 6 * npix, location)) || (rc = r.out(ctx, ref_out ? amp33 : nullptr, 2 * n33, location))) return rc;
    const NsAcc acc{const_cast<uint32_t *>(a0), const_cast<uint64_t *>(a1), const_cast<int32_t *>(b0), const_cast<uint64_t *>(b1),
                    const_cast<int64_t *>(s0), const_cast<uint64_t *>(s1), const_cast<int32_t *>(c0), const_cast<uint64_t *>(c1),
                    const_cast<uint32_t *>(m33)};
    const size_t threads = (size_t)ny * nxt;
    hipLaunchKernelGGL(noise_planes_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx->stream, acc, nexp, n, ny, (int)nx, cw,
                       ref_out, tframe, sqrt(2.0), p.p, r.p);
    RIP_HIP(ctx, hipGetLastError());
    if ((rc = p.download()) || (rc = r.download())) return rc;
    return dev_sync(ctx);
}
