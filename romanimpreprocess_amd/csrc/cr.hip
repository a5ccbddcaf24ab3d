// Cosmic-ray hits of the Level-1 synthesis on the device: the model of romanisim's `cr` module (DESIGN.md 7 restates it; romanisim
// is absent from the reference tree, so parity is unpinned and every constant is a parameter) --
//   rip_synth_cr_tracks    a Poisson number of tracks per read; start, direction, length and energy loss of each by inverse-
//                          transform sampling on tabulated CDFs
//   rip_synth_cr_deposit   every track walked through the pixel grid; a Poisson number of electrons per crossed pixel added to the
//                          electron counts of the hit read and of every later one (reads_e of rip_synth_apportion, in HBM)
// Both asynchronous on the context's stream.  A full exposure has 14 k tracks and 0.7 M atomic adds: nothing here is tuned.  Every
// loop has a static bound.  Deviates under their own Philox tags: an exposure with hits is the hit-free one of its seed plus the hits.
#include <cmath>
#include <cstring>

#include "rip_common.h"

#include "rip_rng.h"

namespace {

constexpr uint32_t TAG_CR_COUNT = 0x20, TAG_CR_TRACK = 0x21, TAG_CR_DEPOSIT = 0x22;
constexpr int MAX_READS = 1024;     // one thread per read in the counting workgroup (rip_synth_apportion has the same limit)
constexpr double SEG_EPS = 1e-10;   // pixels: shorter parts of a track are dropped -- a track through a corner crosses ONE boundary

struct CrDev {   // what the deposit needs of rip_cr_params
    double pixel_size, conversion_factor, depth_ratio;   // depth_ratio = pixel_depth / pixel_size
};
constexpr int DEPOSIT_BLOCKS = 256, DEPOSIT_PASSES = 1 << 15;   // the deposit's grid strides over the rows: 2^31 of them at most

// Poisson deviate of any mean for (a, b, tag): sequential search below 10, transformed rejection above (riprng)
__device__ inline double poisson_any(double lam, uint64_t seed, uint32_t a, uint32_t b, uint32_t tag) {
    if (!(lam > 0.0)) return 0.0;
    if (lam < 10.0) {
        uint32_t c[4] = {a, b, tag, 0x63727069u};
        riprng::philox(c, seed);
        const double u = riprng::u53(c[0], c[1]);
        double p = exp(-lam), cdf = p;
        int k = 0;
        while (u > cdf && k < 200) {
            ++k;
            p *= lam / (double)k;
            cdf += p;
        }
        return (double)k;
    }
    return riprng::poisson_ptrs(riprng::ptrs_plan(lam, sqrt(lam), log(lam)), seed, a, b, tag);
}

// (a): one workgroup, one thread per read -- the number of tracks of every read and where its rows start
__global__ __launch_bounds__(MAX_READS) void cr_counts_kernel(int nreads, double mu, uint64_t seed, const int32_t *__restrict__ counts,
                                                              int capacity, int32_t *__restrict__ offsets) {
    __shared__ uint32_t sh[MAX_READS];
    const int r = threadIdx.x;
    uint32_t mine = 0;
    if (r < nreads) {
        double n = counts ? (double)counts[r] : poisson_any(mu, seed, (uint32_t)r, 0u, TAG_CR_COUNT);
        n = n < 0.0 ? 0.0 : (n > (double)capacity ? (double)capacity : n);   // (the sum of 1024 of them stays below 2^32)
        mine = (uint32_t)n;
    }
    sh[r] = mine;
    __syncthreads();
    for (int d = 1; d < MAX_READS; d <<= 1) {
        const uint32_t add = r >= d ? sh[r - d] : 0u;
        __syncthreads();
        sh[r] += add;
        __syncthreads();
    }
    const uint32_t cap = (uint32_t)capacity;
    if (r < nreads) {
        const uint32_t first = sh[r] - mine;
        offsets[r] = (int32_t)(first < cap ? first : cap);
        if (r == nreads - 1) offsets[nreads] = (int32_t)(sh[r] < cap ? sh[r] : cap);
    }
}

// F^-1(u) on the table (c ascending, x): scipy.interpolate.interp1d(c, x)(u) -- the segment [lo, hi] with c[lo] < u <= c[hi]
// (numpy.searchsorted, left), then slope * (u - c_lo) + x_lo
__device__ inline double inv_cdf(const double *__restrict__ c, const double *__restrict__ x, int n, double u) {
    int lo = 0, hi = n;   // first index in [0, n] whose c >= u
    for (int step = 0; step < 32 && lo < hi; ++step) {   // 14 steps for a grid of 10 000
        const int mid = (lo + hi) >> 1;
        if (c[mid] < u) lo = mid + 1; else hi = mid;
    }
    const int ih = lo < 1 ? 1 : (lo > n - 1 ? n - 1 : lo), il = ih - 1;
    const double slope = (x[ih] - x[il]) / (c[ih] - c[il]);
    return slope * (u - c[il]) + x[il];
}

// (b): one thread per row
__global__ __launch_bounds__(256) void cr_tracks_kernel(int nreads, int nya, int nxa, int grid_size, const double *__restrict__ tab,
                                                        uint64_t seed, const double *__restrict__ uniforms,
                                                        const int32_t *__restrict__ offsets, int capacity, double *__restrict__ tracks) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= capacity || row >= offsets[nreads]) return;
    int lo = 0, hi = nreads;   // the last read whose first row is <= row (reads without tracks share their start with the next)
    for (int step = 0; step < 11 && hi - lo > 1; ++step) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= row) lo = mid; else hi = mid;
    }
    double u[5];
    if (uniforms) {
#pragma unroll
        for (int q = 0; q < 5; ++q) u[q] = uniforms[(size_t)row * 5 + q];
    } else {
        uint32_t w[12];
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            uint32_t c[4] = {(uint32_t)row, (uint32_t)b, TAG_CR_TRACK, 0x6372746bu};
            riprng::philox(c, seed);
#pragma unroll
            for (int q = 0; q < 4; ++q) w[4 * b + q] = c[q];
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) u[q] = riprng::u53(w[2 * q], w[2 * q + 1]);
    }
    double *t = tracks + (size_t)row * 6;
    t[0] = (double)lo;
    t[1] = u[0] * (double)nya;
    t[2] = u[1] * (double)nxa;
    t[3] = 6.283185307179586 * u[2];   // 2 * numpy.pi * u
    t[4] = inv_cdf(tab, tab + grid_size, grid_size, u[3]);
    t[5] = inv_cdf(tab + 2 * (size_t)grid_size, tab + 3 * (size_t)grid_size, grid_size, u[4]);
}

__global__ __launch_bounds__(256) void cr_clear_kernel(size_t npix, int nreads, int32_t *__restrict__ first_read, double *__restrict__ lam) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    first_read[i] = nreads;
    if (lam) lam[i] = 0.0;
}

// (c)-(f): one thread per track.  The segment P0 P1 is P0 + t (P1 - P0); pixel (i, j) is [i - 0.5, i + 0.5) x [j - 0.5, j + 0.5).
// The walk goes from boundary crossing to boundary crossing, t = (k + 0.5 - i0) / (i1 - i0) in i and likewise in j, whichever
// comes first; crossings closer than SEG_EPS pixels are one crossing.
__device__ inline void cr_walk_track(const CrDev &p, int row, int nreads, int nya, int nxa, const double *__restrict__ tracks, int poisson,
                                     uint64_t seed, int32_t *__restrict__ reads_e, int32_t *__restrict__ first_read,
                                     double *__restrict__ lam_out) {
    const double *t = tracks + (size_t)row * 6;
    const double rd = t[0];
    if (!(rd >= 0.0 && rd < (double)nreads)) return;
    const int r = (int)rd;
    const double i0 = t[1], j0 = t[2], phi = t[3];
    if (!(fabs(i0) < 1.0e9 && fabs(j0) < 1.0e9 && fabs(t[4]) < 1.0e15)) return;   // (NaN too) nothing to walk
    const double len_px = t[4] / p.pixel_size;
    const double cpp = t[5] * p.pixel_size / p.conversion_factor;   // electrons per pixel length
    double i1 = i0 + len_px * cos(phi), j1 = j0 + len_px * sin(phi);
    i1 = i1 < -0.5 ? -0.5 : (i1 > (double)nya + 0.5 ? (double)nya + 0.5 : i1);
    j1 = j1 < -0.5 ? -0.5 : (j1 > (double)nxa + 0.5 ? (double)nxa + 0.5 : j1);
    const double di = i1 - i0, dj = j1 - j0, L = sqrt(di * di + dj * dj);
    const size_t npix = (size_t)nya * nxa;
    uint32_t ndep = 0;

    auto deposit = [&](double ci, double cj, double l2) {
        if (!(ci >= 0.0 && ci < (double)nya && cj >= 0.0 && cj < (double)nxa)) return;
        const size_t pix = (size_t)(int)ci * nxa + (size_t)(int)cj;
        const double l3 = sqrt(p.depth_ratio * p.depth_ratio + l2 * l2);
        const double lam = cpp * l3;
        double k = poisson ? poisson_any(lam, seed, (uint32_t)row, ndep, TAG_CR_DEPOSIT) : rint(lam);
        ++ndep;
        k = k > 0.0 ? (k > 2.0e9 ? 2.0e9 : k) : 0.0;   // (the sum with the counts is not saturated: a few 10^5 on counts clipped at 2e9)
        const int ki = (int)k;
        if (ki > 0)
            for (int rr = r; rr < nreads; ++rr) atomicAdd(reads_e + (size_t)rr * npix + pix, ki);
        atomicMin(first_read + pix, r);
        if (lam_out) unsafeAtomicAdd(lam_out + pix, lam);   // the hardware's f64 add: no compare-and-swap loop
    };

    double ci = floor(i0 + 0.5), cj = floor(j0 + 0.5);
    const double si = di > 0.0 ? 1.0 : -1.0, sj = dj > 0.0 ? 1.0 : -1.0;
    double ki = di > 0.0 ? ci : ci - 1.0, kj = dj > 0.0 ? cj : cj - 1.0;   // the next boundary is at k + 0.5
    const double inf = __builtin_inf();
    double t_prev = 0.0;
    bool any = false;
    const int max_steps = nya + nxa + 2;
    for (int step = 0; step < max_steps; ++step) {
        const double ti = di != 0.0 ? (ki + 0.5 - i0) / di : inf;
        const double tj = dj != 0.0 ? (kj + 0.5 - j0) / dj : inf;
        double t_next = ti < tj ? ti : tj;
        t_next = t_next < 1.0 ? t_next : 1.0;
        const double seg = (t_next - t_prev) * L;
        if (seg >= SEG_EPS) {
            deposit(ci, cj, seg);
            any = true;
        }
        if (t_next >= 1.0) break;
        double t_new = t_next;
        if ((ti - t_next) * L < SEG_EPS) {
            ci += si, ki += si;
            t_new = ti > t_new ? ti : t_new;
        }
        if ((tj - t_next) * L < SEG_EPS) {
            cj += sj, kj += sj;
            t_new = tj > t_new ? tj : t_new;
        }
        t_prev = t_new < 1.0 ? t_new : 1.0;
    }
    // a track that stays inside one pixel (no part of SEG_EPS or more): its whole length, which may be zero, in its middle's pixel
    if (!any) deposit(floor((i0 + i1) / 2.0 + 0.5), floor((j0 + j1) / 2.0 + 0.5), L);
}

__global__ __launch_bounds__(256) void cr_deposit_kernel(CrDev p, int nreads, int nya, int nxa, const double *__restrict__ tracks,
                                                         const int32_t *__restrict__ offsets, int poisson, uint64_t seed,
                                                         int32_t *__restrict__ reads_e, int32_t *__restrict__ first_read,
                                                         double *__restrict__ lam_out) {
    const long long first = offsets[0], last = offsets[nreads];
    for (int pass = 0; pass < DEPOSIT_PASSES; ++pass) {
        const long long row = first + ((long long)pass * DEPOSIT_BLOCKS + blockIdx.x) * 256 + threadIdx.x;
        if (row >= last) break;
        cr_walk_track(p, (int)row, nreads, nya, nxa, tracks, poisson, seed, reads_e, first_read, lam_out);
    }
}

int check_params(rip_ctx *ctx, const rip_cr_params *p, const char *who) {
    if (!p) return rip_fail(ctx, RIP_EINVAL, "%s: no parameters", who);
    if (p->grid_size < 2 || p->grid_size > (1 << 24)) return rip_fail(ctx, RIP_EINVAL, "%s: grid_size %d (2..2^24)", who, p->grid_size);
    if (!(p->conversion_factor > 0.0)) return rip_fail(ctx, RIP_EINVAL, "%s: conversion_factor must be positive", who);
    if (!(p->pixel_size > 0.0) || !(p->pixel_depth >= 0.0)) return rip_fail(ctx, RIP_EINVAL, "%s: pixel_size / pixel_depth", who);
    return RIP_OK;
}

// The two inverse-CDF tables, (b) in f64: x = linspace(lo, hi, n), y = pdf(x), c = cumsum(y) - y[0], c /= c.max().
// Layout: c_len | x_len | c_dedx | x_dedx, n doubles each.
void build_tables(const rip_cr_params &p, std::vector<double> &tab) {
    const int n = p.grid_size;
    tab.assign((size_t)4 * n, 0.0);
    auto one = [&](double lo, double hi, double *c, double *x, auto pdf) {
        const double step = (hi - lo) / (double)(n - 1);   // numpy.linspace: arange(n) * step + lo, the last point set to hi
        for (int i = 0; i < n; ++i) x[i] = (double)i * step + lo;
        x[n - 1] = hi;
        double sum = 0.0, y0 = 0.0, cmax = 0.0;
        for (int i = 0; i < n; ++i) {
            const double y = pdf(x[i]);
            if (i == 0) y0 = y;
            sum = i == 0 ? y : sum + y;
            c[i] = sum - y0;
            cmax = c[i] > cmax ? c[i] : cmax;
        }
        for (int i = 0; i < n; ++i) c[i] = c[i] / cmax;
    };
    one(p.min_len, p.max_len, tab.data(), tab.data() + n, [&](double x) { return std::pow(x, p.len_slope); });
    one(p.min_dedx, p.max_dedx, tab.data() + 2 * (size_t)n, tab.data() + 3 * (size_t)n, [&](double x) {
        const double s = (x - p.moyal_location) / p.moyal_scale;
        return std::exp(-(s + std::exp(-s)) / 2.0);
    });
}

}   // namespace

extern "C" int rip_synth_cr_tracks(rip_ctx *ctx, const rip_cr_params *par, int nreads, double read_time, int nya, int nxa, uint64_t seed,
                                   const int32_t *counts, const double *uniforms, int capacity, double *tracks, int32_t *offsets) {
    ctx->stream_dirty = true;
    if (const int rc = check_params(ctx, par, "synth_cr_tracks")) return rc;
    if (!tracks || !offsets || capacity < 1 || nya < 1 || nxa < 1 || nreads < 1 || nreads > MAX_READS)
        return rip_fail(ctx, RIP_EINVAL, "synth_cr_tracks: bad arguments (1..%d reads, capacity >= 1)", MAX_READS);
    const double mu = par->flux * par->area * read_time;
    if (!counts && !(mu >= 0.0 && mu < 1.0e9)) return rip_fail(ctx, RIP_EINVAL, "synth_cr_tracks: %g tracks per read", mu);
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const int n = par->grid_size;
    const void *had = ctx->ws[RIP_WS_CR_TAB];
    double *d_tab = (double *)rip_ws(ctx, RIP_WS_CR_TAB, (size_t)4 * n * sizeof(double));
    if (!d_tab) return RIP_ENOMEM;
    // the device copy of the tables is kept until the parameters that shape them change (the read-share table's rule): exposure
    // after exposure the call stays asynchronous; new tables wait for the kernels still reading the old ones
    rip_cr_params key = *par;
    key.flux = key.area = key.conversion_factor = key.pixel_size = key.pixel_depth = 0.0;   // (do not enter the tables)
    key._pad = 0;
    const bool same = (const void *)d_tab == had && ctx->cr_tab_valid && memcmp(&ctx->cr_tab_key, &key, sizeof key) == 0;
    if (!same) {
        std::vector<double> tab;
        build_tables(*par, tab);
        if (!(tab[n - 1] > 0.0) || !(tab[3 * (size_t)n - 1] > 0.0) || tab[n - 1] != tab[n - 1] || tab[3 * (size_t)n - 1] != tab[3 * (size_t)n - 1])
            return rip_fail(ctx, RIP_EINVAL, "synth_cr_tracks: a probability density sums to nothing on its grid");
        RIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ctx->cr_tab_valid = false;
        RIP_HIP(ctx, hipMemcpy(d_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
        ctx->cr_tab_key = key;
        ctx->cr_tab_valid = true;
    }
    hipLaunchKernelGGL(cr_counts_kernel, dim3(1), dim3(MAX_READS), 0, ctx->stream, nreads, mu, seed, counts, capacity, offsets);
    hipLaunchKernelGGL(cr_tracks_kernel, dim3((unsigned)((capacity + 255) / 256)), dim3(256), 0, ctx->stream, nreads, nya, nxa, n,
                       (const double *)d_tab, seed, uniforms, (const int32_t *)offsets, capacity, tracks);
    RIP_HIP(ctx, hipGetLastError());
    return RIP_OK;
}

extern "C" int rip_synth_cr_deposit(rip_ctx *ctx, const rip_cr_params *par, int nreads, int nya, int nxa, const double *tracks,
                                    const int32_t *offsets, int poisson, uint64_t seed, int32_t *reads_e, int32_t *first_read,
                                    double *lam) {
    ctx->stream_dirty = true;
    if (const int rc = check_params(ctx, par, "synth_cr_deposit")) return rc;
    if (!tracks || !offsets || !reads_e || !first_read || nya < 1 || nxa < 1 || nreads < 1 || nreads > MAX_READS ||
        (long long)nya + nxa > 0x7ffffff0ll)
        return rip_fail(ctx, RIP_EINVAL, "synth_cr_deposit: bad arguments (1..%d reads)", MAX_READS);
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)nya * nxa;
    CrDev p;
    p.pixel_size = par->pixel_size;
    p.conversion_factor = par->conversion_factor;
    p.depth_ratio = par->pixel_depth / par->pixel_size;
    hipLaunchKernelGGL(cr_clear_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, ctx->stream, npix, nreads, first_read, lam);
    hipLaunchKernelGGL(cr_deposit_kernel, dim3(DEPOSIT_BLOCKS), dim3(256), 0, ctx->stream, p, nreads, nya, nxa, tracks,
                       offsets, poisson, seed, reads_e, first_read, lam);
    RIP_HIP(ctx, hipGetLastError());
    return RIP_OK;
}
