// Reference-pixel correction tables (exact medians) -- a small pre-pass in front of the cube kernel.
//
// Replaces (reference file:line):
//   L1_to_L2/gen_cal_image.py:536-539        amp33 block = amp33 - med, minus its own np.median
//   utils/reference_subtraction.py:104-123   ref_subtraction_row  (row medians of the reference output,
//                                            their median `ctr`, per-row correction slope*(med-ctr))
//   utils/reference_subtraction.py:50-60     ref_subtraction_channel (medians of the bottom/top 4 reference
//                                            rows of every 128-column channel, line through them)
// Only the tables are produced here: rowcorr[g][r] (f64) and lines[g][ch] = (m, c) (f64).  The
// per-pixel application is fused into the cube kernel (linearity.hip).  What makes this possible:
//   * with `slope` given (always, when read.amp33 exists) the science-row medians and the polyfit
//     of reference_subtraction.py:107,114 are dead code;
//   * x -> f32(x - M) is monotone, so the rank-63/64 elements of a row of (v - M) are the
//     rank-63/64 elements of v, minus M: row medians and the global median M come from one pass;
//   * the channel step only needs rows 0:4 and ny-4:ny of the row-corrected image.
// All medians are exact selections (np.median: mean of the two middle elements in f32).
// Arithmetic recipe: oracle/refpix.py.
//
// Keys, the selection levels' scan step and the median of a selected pair come from rip_select.h, the row correction and the
// channel line from refpix_shared.h (shared with refpix_one.hip).
#include "rip_host.h"
#include "refpix_shared.h"

// np.median of vals[0..n) in LDS by an in-place bitonic sort; the buffer must hold npow2 >= n floats
// (entries n.. are overwritten with +inf).  All threads of the block must call it.  The median of the image drop-ins; the
// pre-pass's rowcorr_kernel takes block_median_select, whose key order can pick the other of two tied -0 / +0.
// As np.median forms it: NaN where any of the n values is NaN (the network's `x > y` would sort past one); the middle element
// of an odd count as it is (not (v + v) / 2, which overflows above FLT_MAX / 2); the mean of the two middle elements of an even
// count; and never -0 -- numpy's mean adds to +0, so a median of -0 comes out +0 (the `+ 0.0f`, kept by -ffp-contract=off
// without fast-math).
__device__ float block_median_sorted(float *vals, int n, int npow2) {
    for (int i = n + threadIdx.x; i < npow2; i += blockDim.x) vals[i] = INFINITY;
    __syncthreads();
    int nan = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) nan |= vals[i] != vals[i];
    nan = __syncthreads_or(nan);
    for (int k = 2; k <= npow2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < npow2; i += blockDim.x) {
                const int p = i ^ j;
                if (p > i) {
                    const float x = vals[i], y = vals[p];
                    const bool up = (i & k) == 0;
                    if ((x > y) == up) {
                        vals[i] = y;
                        vals[p] = x;
                    }
                }
            }
            __syncthreads();
        }
    const int k_hi = n / 2;
    const float mid = (n & 1) ? vals[k_hi] : (vals[k_hi - 1] + vals[k_hi]) * 0.5f;
    return nan ? NAN : mid + 0.0f;
}

// ---- 1. per (group,row): rank-63 / rank-64 elements of v = f32(amp33) - med -----------------------
// one wave per row: the 128 values live two per lane (elements lane and lane+64) and are sorted by a
// bitonic network of cross-lane exchanges; rank 63 ends in (lane 63, slot 0), rank 64 in (lane 0, slot 1)
__global__ __launch_bounds__(256) void amp33_rows_kernel(const uint16_t *__restrict__ amp33,
                                                         const float *__restrict__ med, float *__restrict__ lohi,
                                                         int ny, int row_first, int nrows_total) {
    const int lane = threadIdx.x & 63;
    const int row_id = row_first + blockIdx.x * 4 + (threadIdx.x >> 6);  // flattened (g, r), from the first group whose tables are made
    if (row_id >= nrows_total) return;
    const int r = row_id % ny;
    const uint16_t *a = amp33 + (size_t)row_id * RIP_CW;
    const float *m = med + (size_t)r * RIP_CW;
    float v0 = (float)a[lane] - m[lane];
    float v1 = (float)a[lane + 64] - m[lane + 64];
#pragma unroll
    for (int k = 2; k <= 128; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (j == 64) {  // partner = the other slot of this lane; k = 128: ascending everywhere
                const float lo = fminf(v0, v1), hi = fmaxf(v0, v1);
                v0 = lo;
                v1 = hi;
            } else {
                const float p0 = __shfl_xor(v0, j, 64), p1 = __shfl_xor(v1, j, 64);
                const bool lower = (lane & j) == 0;
                const bool up0 = (lane & k) == 0, up1 = ((lane + 64) & k) == 0;
                v0 = (lower == up0) ? fminf(v0, p0) : fmaxf(v0, p0);
                v1 = (lower == up1) ? fminf(v1, p1) : fmaxf(v1, p1);
            }
        }
    }
    float *o = lohi + (size_t)row_id * 2;
    if (lane == 63) o[0] = v0;
    if (lane == 0) o[1] = v1;
}

// ---- 2. exact selection of two ranks among the ny*128 values of each group (3-level radix) -------
struct SelState {
    uint32_t prefix[2];
    uint32_t rank[2];
};

__global__ __launch_bounds__(256) void sel_hist_kernel(const uint16_t *__restrict__ amp33, const float *__restrict__ med,
                                                       const SelState *__restrict__ st, uint32_t *__restrict__ ghist,
                                                       int ny, int level, int chunk, int g0) {
    __shared__ uint32_t h[2][SEL_BINS];
    const int g = g0 + blockIdx.y;
    for (int i = threadIdx.x; i < 2 * SEL_BINS; i += blockDim.x) (&h[0][0])[i] = 0;
    __syncthreads();
    const size_t n = (size_t)ny * RIP_CW;
    const size_t lo = (size_t)blockIdx.x * chunk;
    const size_t hi = (lo + chunk < n) ? lo + chunk : n;
    const int shift = sel_shift(level);
    const uint32_t mask = (1u << sel_bits(level)) - 1u;
    const int above = shift + sel_bits(level);  // bits above this level's field
    const uint32_t p0 = level ? st[g].prefix[0] : 0u, p1 = level ? st[g].prefix[1] : 0u;   // level 0: no prefix yet (st not read)
    for (size_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        const uint32_t key = f2key((float)amp33[(size_t)g * n + i] - med[i]);
        const uint32_t bin = (key >> shift) & mask;
        const bool m0 = (above >= 32) || (((key ^ p0) >> above) == 0);
        const bool m1 = (above >= 32) || (((key ^ p1) >> above) == 0);
        if (m0) atomicAdd(&h[0][bin], 1u);
        if (m1) atomicAdd(&h[1][bin], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * SEL_BINS; i += blockDim.x) {
        const uint32_t c = (&h[0][0])[i];
        if (c) atomicAdd(&ghist[(size_t)g * 2 * SEL_BINS + i], c);
    }
}

__global__ __launch_bounds__(256) void sel_scan_kernel(SelState *__restrict__ st, uint32_t *__restrict__ ghist, int level, uint32_t n,
                                                       int g0) {
    // bin holding the wanted rank: 8 bins per thread
    __shared__ uint32_t part[4];
    const int g = g0 + blockIdx.x, t = blockIdx.y;
    uint32_t *h = ghist + ((size_t)g * 2 + t) * SEL_BINS;
    const int per = SEL_BINS / 256;
    const int tid = threadIdx.x;
    // level 0 starts the selection: the two middle elements of n values, empty prefix (no separate initialisation launch)
    const uint32_t rank = level ? st[g].rank[t] : (t ? n / 2 : n / 2 - 1);
    const uint32_t before = level ? st[g].prefix[t] : 0u;
    uint32_t bin, left;
    if (sel_find_bin<256, per>([&](int k) { return h[tid * per + k]; }, rank, tid, true, part, bin, left)) {
        st[g].prefix[t] = before | (bin << sel_shift(level));
        st[g].rank[t] = left;
    }
    __syncthreads();
    for (int k = 0; k < per; ++k) h[tid * per + k] = 0;  // ready for the next level
}

// np.median of vals[0..n) in LDS by a three-level radix selection inside one block (11 + 11 + 10 key bits, two LDS histograms:
// one per middle element): 3 x (count, scan) instead of the 78 compare-exchange passes of a bitonic sort of 4096 values.
// The median of an even count is the f32 mean of the two middle elements, as np.median forms it.  All threads of the block
// call it; h: 2 x SEL_BINS words, tmp: 8 words of LDS.
__device__ float block_median_select(const float *vals, int n, uint32_t (*h)[SEL_BINS], uint32_t *tmp) {
    uint32_t prefix[2] = {0u, 0u};
    uint32_t rank[2] = {(uint32_t)((n & 1) ? n / 2 : n / 2 - 1), (uint32_t)(n / 2)};
    const int t = threadIdx.x;
    for (int lv = 0; lv < 3; ++lv) {
        for (int i = t; i < 2 * SEL_BINS; i += blockDim.x) (&h[0][0])[i] = 0;
        __syncthreads();
        const int shift = sel_shift(lv), above = shift + sel_bits(lv);
        const uint32_t mask = (1u << sel_bits(lv)) - 1u;
        for (int i = t; i < n; i += blockDim.x) {
            const uint32_t key = f2key(vals[i]);
            const uint32_t bin = (key >> shift) & mask;
            if (above >= 32 || ((key ^ prefix[0]) >> above) == 0) atomicAdd(&h[0][bin], 1u);
            if (above >= 32 || ((key ^ prefix[1]) >> above) == 0) atomicAdd(&h[1][bin], 1u);
        }
        __syncthreads();
        for (int q = 0; q < 2; ++q) {
            // the 2048 bins: 8 per thread for the first 256 threads; the owner writes {bin, rank inside it} to tmp[4..5]
            const int per = SEL_BINS / 256;
            const uint32_t *own = h[q] + t * per;
            sel_find_bin<256, per>([=](int k) { return own[k]; }, rank[q], t, t < 256, tmp, tmp[4], tmp[5]);
            __syncthreads();
            prefix[q] |= tmp[4] << shift;
            rank[q] = tmp[5];
            __syncthreads();
        }
    }
    return key_median(prefix[0], prefix[1]);
}

// ---- 3. per group: global median M, row medians, ctr, rowcorr ------------------------------------
__global__ __launch_bounds__(1024) void rowcorr_kernel(const SelState *__restrict__ st, const float *__restrict__ lohi,
                                                       double slope, double *__restrict__ rowcorr,
                                                       double *__restrict__ rowcorr_t, int ny, int G, int g0) {
    extern __shared__ float rm[];  // [ny] row medians
    const int g = g0 + blockIdx.x;
    const float M = key_median(st[g].prefix[0], st[g].prefix[1]);  // np.median of the block
    auto refmed = [&](int r) {
        const float a = lohi[((size_t)g * ny + r) * 2] - M;
        const float b = lohi[((size_t)g * ny + r) * 2 + 1] - M;
        return (a + b) * 0.5f;
    };
    __shared__ uint32_t hsel[2][SEL_BINS];
    __shared__ uint32_t tmp[8];
    for (int r = threadIdx.x; r < ny; r += blockDim.x) rm[r] = refmed(r);
    __syncthreads();
    const float ctr = block_median_select(rm, ny, hsel, tmp);
    for (int r = threadIdx.x; r < ny; r += blockDim.x) {
        const double v = row_corr(slope, refmed(r), ctr);
        rowcorr[(size_t)g * ny + r] = v;
        if (rowcorr_t) rowcorr_t[(size_t)r * G + g] = v;  // [row][group]: one scalar load per row
    }
}

// ---- 4. per (group, channel): bottom/top medians of the row-corrected image, line fit ---------
template <typename DT>
__global__ __launch_bounds__(1024) void chan_kernel(const DT *__restrict__ data, const float *__restrict__ dark,
                                                    const double *__restrict__ rowcorr,
                                                    const double *__restrict__ lines_override,
                                                    double *__restrict__ lines, int ny, int nx, int g0) {
    __shared__ float v[1024];
    const int ch = blockIdx.x, g = g0 + blockIdx.y, nch = gridDim.x;
    const int e = threadIdx.x & 511, half = threadIdx.x >> 9;
    const int row = (half ? ny - 4 : 0) + e / RIP_CW;
    const size_t idx = ((size_t)g * ny + row) * nx + (size_t)ch * RIP_CW + e % RIP_CW;
    float val = (float)data[idx] - dark[idx];
    val = (float)((double)val - rowcorr[(size_t)g * ny + row]);
    v[threadIdx.x] = val;
    __syncthreads();
    // both halves at once: the bitonic network over the 1024 values stopped at runs of 512 leaves the bottom rows' values
    // ascending in v[0:512] and the top rows' descending in v[512:1024]; the two middle elements sit at 255, 256 either way
    // (45 compare-exchange steps per thread instead of 512 rank comparisons: a third of the kernel's time)
    for (int k = 2; k <= 512; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int i = threadIdx.x, p = i ^ j;
            if (p > i) {
                const float x = v[i], y = v[p];
                const bool up = (i & k) == 0;
                if ((x > y) == up) {
                    v[i] = y;
                    v[p] = x;
                }
            }
            __syncthreads();
        }
    if (threadIdx.x == 0) {
        const size_t o = ((size_t)g * nch + ch) * 2;
        double m, c;
        chan_line((v[255] + v[256]) * 0.5f, (v[512 + 255] + v[512 + 256]) * 0.5f, ny, lines_override ? lines_override + o : nullptr,
                  m, c);
        lines[o] = m;
        lines[o + 1] = c;
    }
}

// which pre-pass makes the tables: 1 the single launch of refpix_one.hip, 0 the launches below.  option (rip_ctx::prepass_form,
// or the form a stage call asks for): -1 by situation -- the single launch in front of its own ramp, the small launches beside
// the previous ramp's fused kernel (a.background) --, 1 the single launch wherever it covers the frame, 0 never
int rip_refpix_form(int option, const RefpixArgs &a) {
    return (option == 1 || (option < 0 && !a.background)) && rip_refpix_one_supported(a) ? 1 : 0;
}

int rip_launch_refpix_prepass(rip_ctx *ctx, const RefpixArgs &a, int form) {
    if (a.nx % RIP_CW) return rip_fail(ctx, RIP_EINVAL, "refpix: nx=%d is not a multiple of 128", a.nx);
    if (a.ny < 8) return rip_fail(ctx, RIP_EINVAL, "refpix: ny=%d too small", a.ny);
    const int G = a.ngrp, ny = a.ny, nch = a.nx / RIP_CW;
    // tables of groups g0 .. G-1 only (g0 = 1 in front of a fused kernel that skips group 0): every kernel below works group by
    // group, so the launches simply cover G - g0 groups from g0 on; the entries of the groups before g0 stay unwritten
    const int g0 = a.g0;
    if (g0 < 0 || g0 >= G) return rip_fail(ctx, RIP_EINVAL, "refpix: first group %d of %d", g0, G);
    hipStream_t strm = a.stream ? a.stream : ctx->stream;   // (the overlapped pre-pass: the context's second stream)
    if (form == 1) return rip_launch_refpix_one(ctx, a);
    if (a.amp33) {
        // scratch: lohi (G,ny,2) f32 | SelState[G]
        const size_t lohi_b = (size_t)G * ny * 2 * sizeof(float);
        const size_t st_b = ((size_t)G * sizeof(SelState) + 255) / 256 * 256;
        char *ws = (char *)rip_ws(ctx, RIP_WS_REFPIX, lohi_b + st_b);
        if (!ws) return RIP_ENOMEM;
        float *lohi = (float *)ws;
        SelState *st = (SelState *)(ws + lohi_b);
        // the selection histograms have a workspace slot of their own, of a fixed size: every level's scan leaves them zero, so
        // they are cleared only when the slot is first allocated (no initialisation launch per call)
        const size_t gh_b = (size_t)RIP_MAX_GROUPS * 2 * SEL_BINS * sizeof(uint32_t);
        const void *had = ctx->ws[RIP_WS_SEL_HIST];
        uint32_t *ghist = (uint32_t *)rip_ws(ctx, RIP_WS_SEL_HIST, gh_b);
        if (!ghist) return RIP_ENOMEM;
        if ((const void *)ghist != had) RIP_HIP(ctx, hipMemsetAsync(ghist, 0, gh_b, strm));
        const uint32_t n = (uint32_t)ny * RIP_CW;
        hipLaunchKernelGGL(amp33_rows_kernel, dim3((unsigned)(((G - g0) * ny + 3) / 4)), dim3(256), 0, strm, a.amp33,
                           a.amp33_med, lohi, ny, g0 * ny, G * ny);
        const int chunk = 8192;
        const unsigned nblk = (unsigned)((n + chunk - 1) / chunk);
        for (int level = 0; level < 3; ++level) {
            hipLaunchKernelGGL(sel_hist_kernel, dim3(nblk, G - g0), dim3(256), 0, strm, a.amp33, a.amp33_med, st,
                               ghist, ny, level, chunk, g0);
            hipLaunchKernelGGL(sel_scan_kernel, dim3(G - g0, 2), dim3(256), 0, strm, st, ghist, level, n, g0);
        }
        const size_t lds = (size_t)ny * sizeof(float);
        int rc;
        if ((rc = with_lds(ctx, rowcorr_kernel, lds))) return rc;
        hipLaunchKernelGGL(rowcorr_kernel, dim3(G - g0), dim3(1024), lds, strm, st, lohi, a.slope, a.rowcorr, a.rowcorr_t, ny, G, g0);
    } else {
        // no reference output in the read file: the row step is the identity
        RIP_HIP(ctx, hipMemsetAsync(a.rowcorr, 0, (size_t)G * ny * sizeof(double), strm));
        if (a.rowcorr_t) RIP_HIP(ctx, hipMemsetAsync(a.rowcorr_t, 0, (size_t)G * ny * sizeof(double), strm));
    }
    if (a.data_dtype == RIP_U16)
        hipLaunchKernelGGL(chan_kernel<uint16_t>, dim3(nch, G - g0), dim3(1024), 0, strm, (const uint16_t *)a.data,
                           a.dark_data, a.rowcorr, a.lines_override, a.lines, ny, a.nx, g0);
    else
        hipLaunchKernelGGL(chan_kernel<float>, dim3(nch, G - g0), dim3(1024), 0, strm, (const float *)a.data,
                           a.dark_data, a.rowcorr, a.lines_override, a.lines, ny, a.nx, g0);
    RIP_HIP(ctx, hipGetLastError());
    return RIP_OK;
}

// ------------------------------------------------------------------ image-level drop-ins
// reference_subtraction.py with ANY of its arguments, on one f32 image resident on the device (rip_stage_refpix_image, the
// configuration of calibrateimage, is the two of them in a row):
//   ref_subtraction_row(image, use_ref_channel=False, slope=None)      :77-125  row medians of the 4+4 border pixels or of
//       the reference output, of the science pixels (for the np.polyfit of slope=None, done by the host mirror), update
//       in the dtype numpy's promotion gives: f64 for a numpy f64 slope, f32 for a Python float / numpy f32 slope
//   ref_subtraction_channel(image, channel_start, channel_end, use_ref_channel) :16-74  windows [start+128k, end+128k),
//       one after the other as the reference's loop runs them (windows wider than 128 columns overlap)

// median of the values of `nr` rows x (cols [c0, c0+n0) u [c1, c1+n1)) per block: block (b, k) starts at row row0 + b * rstep,
// its columns are shifted by 128 k (window k); out[k * gridDim.x + b].  Dynamic LDS: npow2 floats.
__global__ __launch_bounds__(1024) void img_window_median_kernel(const float *__restrict__ image, int w, int row0, int rstep,
                                                                 int nr, int c0, int n0, int c1, int n1,
                                                                 float *__restrict__ out, int npow2) {
    extern __shared__ float mv[];
    const int per = n0 + n1, n = nr * per;
    const int rbase = row0 + (int)blockIdx.x * rstep, cs = (int)blockIdx.y * RIP_CW;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int rr = i / per, cc = i % per;
        const int col = cs + (cc < n0 ? c0 + cc : c1 + (cc - n0));
        mv[i] = image[(size_t)(rbase + rr) * w + col];
    }
    __syncthreads();
    const float m = block_median_sorted(mv, n, npow2);
    if (threadIdx.x == 0) out[blockIdx.y * gridDim.x + blockIdx.x] = m;
}

// ctr = median of the row medians; rowcorr[r] = the row correction of ref_med[r], f64 or f32 form
__global__ __launch_bounds__(1024) void img_ctr2_kernel(const float *__restrict__ ref_med, double slope, int f32_form,
                                                        double *__restrict__ rowcorr, float *__restrict__ ctr_out, int ny,
                                                        int npow2) {
    extern __shared__ float rm[];
    for (int r = threadIdx.x; r < ny; r += blockDim.x) rm[r] = ref_med[r];
    const float ctr = block_median_sorted(rm, ny, npow2);
    const float s32 = (float)slope;
    for (int r = threadIdx.x; r < ny; r += blockDim.x)
        rowcorr[r] = f32_form ? row_corr_f32(s32, ref_med[r], ctr) : row_corr(slope, ref_med[r], ctr);
    if (threadIdx.x == 0 && ctr_out) *ctr_out = ctr;
}

__global__ void img_rowapply_kernel(float *__restrict__ image, const double *__restrict__ rowcorr, int ny, int w) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)ny * w) return;
    image[i] = (float)((double)image[i] - rowcorr[i / w]);
}

__global__ void img_rowapply_f32_kernel(float *__restrict__ image, const double *__restrict__ rowcorr, int ny, int w) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)ny * w) return;
    image[i] = image[i] - (float)rowcorr[i / w];
}

// the lines of nwin windows from their bottom / top medians bt[k] (or the caller's, line_override[k])
__global__ void img_lines_kernel(const float *__restrict__ bt, const double *__restrict__ line_override, double *__restrict__ line,
                                 float *__restrict__ bt_out, int ny, int nwin) {
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= nwin) return;
    const float b = bt[2 * k], t = bt[2 * k + 1];
    chan_line(b, t, ny, line_override ? line_override + 2 * k : nullptr, line[2 * k], line[2 * k + 1]);
    if (bt_out) {
        bt_out[2 * k] = b;
        bt_out[2 * k + 1] = t;
    }
}

// the update of the ncols columns of window k = blockIdx.y, from column c0 + 128 k, by its line
__global__ void img_winapply_kernel(float *__restrict__ image, const double *__restrict__ line, int ny, int w, int c0,
                                    int ncols) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)ny * ncols) return;
    const int k = (int)blockIdx.y;
    const int r = (int)(i / ncols), c = c0 + k * RIP_CW + (int)(i % ncols);
    const double iel = line[2 * k] * (double)r + line[2 * k + 1];
    float *p = image + (size_t)r * w + c;
    *p = (float)((double)*p - iel);
}

static int pow2_at_least(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

int rip_refpix_row_general(rip_ctx *ctx, float *d_image, int ny, int width, int nside, int use_ref_channel, int mode,
                           double slope, float *d_ref_med, float *d_sci_med, float *d_ctr) {
    if (nside < 16 || nside > width || (use_ref_channel && nside + RIP_CW > width))
        return rip_fail(ctx, RIP_EINVAL, "refpix row: nside=%d does not fit an image %d wide", nside, width);
    if (nside - 8 > 32768 || ny > 32768) return rip_fail(ctx, RIP_EINVAL, "refpix row: frame too large (%d x %d)", ny, nside);
    char *ws = (char *)rip_ws(ctx, RIP_WS_REFPIX, (size_t)ny * (sizeof(double) + 2 * sizeof(float)) + 256);
    if (!ws) return RIP_ENOMEM;
    double *rowcorr = (double *)ws;
    float *refmed = (float *)(rowcorr + ny), *scimed = refmed + ny;
    int rc;
    {   // reference medians: the reference output, or the 4 + 4 border pixels of the row (reference_subtraction.py:108-111)
        const int n = use_ref_channel ? RIP_CW : 8, np2 = pow2_at_least(n);
        if ((rc = with_lds(ctx, img_window_median_kernel, (size_t)np2 * 4))) return rc;
        if (use_ref_channel)
            hipLaunchKernelGGL(img_window_median_kernel, dim3(ny), dim3(1024), (size_t)np2 * 4, ctx->stream, d_image, width, 0, 1, 1,
                               nside, RIP_CW, 0, 0, refmed, np2);
        else
            hipLaunchKernelGGL(img_window_median_kernel, dim3(ny), dim3(1024), (size_t)np2 * 4, ctx->stream, d_image, width, 0, 1, 1,
                               0, 4, nside - 4, 4, refmed, np2);
    }
    if (d_sci_med) {   // science medians (:107), only needed for the polyfit of slope=None
        const int n = nside - 8, np2 = pow2_at_least(n);
        if ((rc = with_lds(ctx, img_window_median_kernel, (size_t)np2 * 4))) return rc;
        hipLaunchKernelGGL(img_window_median_kernel, dim3(ny), dim3(1024), (size_t)np2 * 4, ctx->stream, d_image, width, 0, 1, 1, 4,
                           n, 0, 0, scimed, np2);
        RIP_HIP(ctx, hipMemcpyAsync(d_sci_med, scimed, (size_t)ny * 4, hipMemcpyDeviceToDevice, ctx->stream));
    }
    {
        const int np2 = pow2_at_least(ny);
        if ((rc = with_lds(ctx, img_ctr2_kernel, (size_t)np2 * 4))) return rc;
        hipLaunchKernelGGL(img_ctr2_kernel, dim3(1), dim3(1024), (size_t)np2 * 4, ctx->stream, refmed, slope, mode == 2 ? 1 : 0,
                           rowcorr, d_ctr, ny, np2);
    }
    if (d_ref_med) RIP_HIP(ctx, hipMemcpyAsync(d_ref_med, refmed, (size_t)ny * 4, hipMemcpyDeviceToDevice, ctx->stream));
    const size_t n = (size_t)ny * width;
    if (mode == 1)
        hipLaunchKernelGGL(img_rowapply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_image, rowcorr, ny,
                           width);
    else if (mode == 2)
        hipLaunchKernelGGL(img_rowapply_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_image, rowcorr,
                           ny, width);
    RIP_HIP(ctx, hipGetLastError());
    return RIP_OK;
}

int rip_refpix_channel_general(rip_ctx *ctx, float *d_image, int ny, int width, int channel_start, int channel_end, int nchan,
                               const double *d_lines, float *d_bottom_top) {
    const int cw = channel_end - channel_start;
    if (ny < 8 || cw < 1 || channel_start < 0 || nchan < 1 || channel_end + (nchan - 1) * RIP_CW > width)
        return rip_fail(ctx, RIP_EINVAL, "refpix channel: windows [%d,%d) + 128 k, k < %d do not fit an image %d wide", channel_start,
                        channel_end, nchan, width);
    if (4 * cw > 32768) return rip_fail(ctx, RIP_EINVAL, "refpix channel: window of %d columns is too wide", cw);
    // The reference's loop takes the windows one after the other, and a window sees the updates of the windows before it.
    // Windows no wider than a channel are disjoint column ranges: then all of them at once (medians, lines, update) give the
    // same result; wider ones, which overlap, go one at a time.
    const int batch = cw <= RIP_CW ? nchan : 1;
    char *ws = (char *)rip_ws(ctx, RIP_WS_REFPIX, (size_t)batch * 2 * (sizeof(double) + sizeof(float)));
    if (!ws) return RIP_ENOMEM;
    double *line = (double *)ws;
    float *bt = (float *)(line + 2 * batch);
    const int np2 = pow2_at_least(4 * cw);
    int rc;
    if ((rc = with_lds(ctx, img_window_median_kernel, (size_t)np2 * 4))) return rc;
    const size_t n = (size_t)ny * cw;
    for (int k = 0; k < nchan; k += batch) {
        const int c0 = channel_start + k * RIP_CW;
        // per window two blocks: rows 0:4 and ny-4:ny
        hipLaunchKernelGGL(img_window_median_kernel, dim3(2, batch), dim3(1024), (size_t)np2 * 4, ctx->stream, d_image, width, 0,
                           ny - 4, 4, c0, cw, 0, 0, bt, np2);
        hipLaunchKernelGGL(img_lines_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, ctx->stream, bt,
                           d_lines ? d_lines + 2 * k : nullptr, line, d_bottom_top ? d_bottom_top + 2 * k : nullptr, ny, batch);
        hipLaunchKernelGGL(img_winapply_kernel, dim3((unsigned)((n + 255) / 256), batch), dim3(256), 0, ctx->stream, d_image, line,
                           ny, width, c0, cw);
    }
    RIP_HIP(ctx, hipGetLastError());
    return RIP_OK;
}
