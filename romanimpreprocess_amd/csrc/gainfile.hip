// Gain and ipc4d files: what the reference's runs/2026_July/make_gain_file.py (the same script in runs/summer2025run) expands
// from solid-waffle's superpixel summaries -- the two CALDIR files every other derivation reads.
//   make_gain_file.py:59-68, 88, 104   gain = f32(unpack(mean_g)), dq = 0 / 2**19 from unpack(good)          -> rip_cal_gain_ipc4d (exact)
//   make_gain_file.py:130-175, 195     ipc4d (3,3,ny-2nb,nx-2nb): fill, clip at the edges, symmetrise, centre    (one entry, exact)
// The tables (nanmean over files and over superpixels, make_gain_file.py:39-54) are numpy's on the host side
// (romanimpreprocess_amd/calfiles/): their bits are numpy's summation order.  The device only expands them, so both kernels are
// pure store kernels: the table slice a workgroup needs sits in LDS, every lane writes 16 bytes per store where the row allows
// it, with non-temporal policy (nothing reads the planes back in this launch, and 1.2 GB does not fit any cache).
//
// Closed form per active pixel p = (ya,xa), with sp(Y,X) = (Y / ry, X / rx) on full-frame coordinates and
// a_t(p) = f64(f32(mean_t[sp(p + nb)])):
//   K[1+dy][1+dx][p] = (a_t(p) + a_t(p + o)) / 2.0 for o = (dy,dx) != (0,0) with p + o inside the active region, else 0.0;
//                      t = aV for (+-1,0), aH for (0,+-1), aD for the diagonals
//   K[1][1][p]       = 1.0 - S, S the f64 sum of the nine planes in row-major order with the centre taken as 0.0
// (the script's "+ 0.0" for the centre is kept: it turns a sum of -0.0 into +0.0, as numpy's np.sum does).
// The script fills the planes with a_t(p), zeroes the rows and columns whose neighbour lies outside, then replaces each pair
// K[1+dy][1+dx][p], K[1-dy][1-dx][p+o] by its mean: the mean of a_t(p) and a_t(p+o), which is the form above.
#include <climits>
#include <vector>

#include "rip_host.h"

namespace {

#define GF_THREADS 256
#define GF_DQ_NO_GAIN (1u << 19)   // make_gain_file.py:104

__device__ __forceinline__ int gf_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// V adjacent values of one plane row, in one store of V * sizeof(T) bytes (16 for double x 2 and float x 4)
template <typename T, int V>
__device__ __forceinline__ void gf_store(T *dst, const double (&v)[V]) {
    if constexpr (V == 1) {
        __builtin_nontemporal_store((T)v[0], dst);
    } else {
        typedef T vec_t __attribute__((ext_vector_type(V)));
        vec_t q;
#pragma unroll
        for (int j = 0; j < V; ++j) q[j] = (T)v[j];   // the one rounding of the float32 file
        __builtin_nontemporal_store(q, reinterpret_cast<vec_t *>(dst));
    }
}

// ------------------------------------------------------------------------------------------ ipc4d
// One workgroup per GF_THREADS * V consecutive columns of one active row; a lane writes V adjacent pixels of all nine planes.
// V divides the active width (the host picks it), so a lane is inside the row with all its pixels or with none, and every
// store is aligned to its width.  The lane's pixels may straddle a superpixel seam or touch the frame edge: it looks up the
// V + 2 columns xa0-1 .. xa0+V of the three rows ya-1, ya, ya+1 one by one.
// tab holds the slice of the f32 tables those columns fall into: [0] aV, [1] aD of the row above, [2] aH, [3] aV, [4] aD of
// the row itself, [5] aV, [6] aD of the row below.  Rows and columns outside the frame are clamped to its first or last
// superpixel: their values are never used (the planes are 0.0 there), the indices stay inside the tables.
template <typename T, int V>
__global__ __launch_bounds__(GF_THREADS) void gainfile_ipc4d_kernel(const float *__restrict__ aH, const float *__restrict__ aV,
                                                                    const float *__restrict__ aD, int nsy, int nsx, int ry, int rx,
                                                                    int nb, int nya, int nxa, int nbx, T *__restrict__ K) {
    constexpr int SPAN = GF_THREADS * V + 2;
    __shared__ float tab[7][SPAN];
    const int ya = (int)(blockIdx.x / (unsigned)nbx), bx = (int)(blockIdx.x - (unsigned)ya * (unsigned)nbx);
    const int xb = bx * (GF_THREADS * V);
    const int sx0 = gf_clamp((xb - 1 + nb) / rx, nsx - 1), sx1 = gf_clamp((xb + GF_THREADS * V + nb) / rx, nsx - 1);
    const int span = sx1 - sx0 + 1;   // <= SPAN: the columns xb-1 .. xb + GF_THREADS * V
    const int sym = gf_clamp((ya + nb - 1) / ry, nsy - 1), syc = gf_clamp((ya + nb) / ry, nsy - 1), syp = gf_clamp((ya + nb + 1) / ry, nsy - 1);
    for (int c = threadIdx.x; c < span; c += GF_THREADS) {
        const size_t m = (size_t)sym * nsx + sx0 + c, z = (size_t)syc * nsx + sx0 + c, p = (size_t)syp * nsx + sx0 + c;
        tab[0][c] = aV[m];
        tab[1][c] = aD[m];
        tab[2][c] = aH[z];
        tab[3][c] = aV[z];
        tab[4][c] = aD[z];
        tab[5][c] = aV[p];
        tab[6][c] = aD[p];
    }
    __syncthreads();
    const int xa0 = xb + (int)threadIdx.x * V;
    if (xa0 >= nxa) return;

    // the table column of the full-frame columns xa0 - 1 + nb + j, j = 0 .. V+1, by one division and V + 1 steps
    double vm[V + 2], dm[V + 2], h0[V + 2], v0[V + 2], d0[V + 2], vp[V + 2], dp[V + 2];
    {
        const int X0 = xa0 - 1 + nb;   // >= -1
        int q = X0 >= 0 ? X0 / rx : -1, rem = X0 >= 0 ? X0 - q * rx : rx - 1;
#pragma unroll
        for (int j = 0; j < V + 2; ++j) {
            const int c = gf_clamp(q, nsx - 1) - sx0;
            vm[j] = (double)tab[0][c];
            dm[j] = (double)tab[1][c];
            h0[j] = (double)tab[2][c];
            v0[j] = (double)tab[3][c];
            d0[j] = (double)tab[4][c];
            vp[j] = (double)tab[5][c];
            dp[j] = (double)tab[6][c];
            if (++rem == rx) {
                rem = 0;
                ++q;
            }
        }
    }
    const bool up = ya > 0, dn = ya < nya - 1;
    double k[9][V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int xa = xa0 + j, c = j + 1;
        const bool lf = xa > 0, rt = xa < nxa - 1;
        k[0][j] = (up && lf) ? (d0[c] + dm[c - 1]) / 2.0 : 0.0;
        k[1][j] = up ? (v0[c] + vm[c]) / 2.0 : 0.0;
        k[2][j] = (up && rt) ? (d0[c] + dm[c + 1]) / 2.0 : 0.0;
        k[3][j] = lf ? (h0[c] + h0[c - 1]) / 2.0 : 0.0;
        k[5][j] = rt ? (h0[c] + h0[c + 1]) / 2.0 : 0.0;
        k[6][j] = (dn && lf) ? (d0[c] + dp[c - 1]) / 2.0 : 0.0;
        k[7][j] = dn ? (v0[c] + vp[c]) / 2.0 : 0.0;
        k[8][j] = (dn && rt) ? (d0[c] + dp[c + 1]) / 2.0 : 0.0;
        double s = k[0][j];
        s = s + k[1][j];
        s = s + k[2][j];
        s = s + k[3][j];
        s = s + 0.0;   // the centre plane, zero while the script sums: -0.0 becomes +0.0 here
        s = s + k[5][j];
        s = s + k[6][j];
        s = s + k[7][j];
        s = s + k[8][j];
        k[4][j] = 1.0 - s;
    }
    const size_t na = (size_t)nya * nxa, at = (size_t)ya * nxa + xa0;
#pragma unroll
    for (int pl = 0; pl < 9; ++pl) gf_store<T, V>(K + (size_t)pl * na + at, k[pl]);
}

// ------------------------------------------------------------------------------------------ gain and its flags
// One workgroup per GF_THREADS * V consecutive columns of one full-frame row, V dividing nx.  gain = f32(mean_g) of the pixel's
// superpixel, 0.0 on the nb border rows and columns; dq = 0 where the superpixel is good and the pixel is off the border, else
// 2**19.  Either plane may be null.
template <int V>
__global__ __launch_bounds__(GF_THREADS) void gainfile_gain_kernel(const float *__restrict__ g, const uint8_t *__restrict__ good, int nsx,
                                                                   int ry, int rx, int nb, int ny, int nx, int nbx,
                                                                   float *__restrict__ gain, uint32_t *__restrict__ dq) {
    constexpr int SPAN = GF_THREADS * V;
    __shared__ float tg[SPAN];
    __shared__ uint32_t tq[SPAN];
    const int Y = (int)(blockIdx.x / (unsigned)nbx), bx = (int)(blockIdx.x - (unsigned)Y * (unsigned)nbx);
    const int xb = bx * SPAN, sy = Y / ry;   // Y < ny = nsy * ry
    const int sx0 = xb / rx, sx1 = gf_clamp((xb + SPAN - 1) / rx, nsx - 1);
    for (int c = threadIdx.x; c <= sx1 - sx0; c += GF_THREADS) {
        tg[c] = g[(size_t)sy * nsx + sx0 + c];
        tq[c] = good[(size_t)sy * nsx + sx0 + c] ? 0u : GF_DQ_NO_GAIN;
    }
    __syncthreads();
    const int x0 = xb + (int)threadIdx.x * V;
    if (x0 >= nx) return;
    const bool yborder = Y < nb || Y >= ny - nb;
    int q = x0 / rx, rem = x0 - q * rx;
    float gv[V];
    uint32_t qv[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int X = x0 + j, c = q - sx0;
        const bool border = yborder || X < nb || X >= nx - nb;
        gv[j] = border ? 0.0f : tg[c];
        qv[j] = border ? GF_DQ_NO_GAIN : tq[c];
        if (++rem == rx) {
            rem = 0;
            ++q;
        }
    }
    const size_t at = (size_t)Y * nx + x0;
    if constexpr (V == 1) {
        if (gain) __builtin_nontemporal_store(gv[0], gain + at);
        if (dq) __builtin_nontemporal_store(qv[0], dq + at);
    } else {
        typedef float f4 __attribute__((ext_vector_type(4)));
        typedef uint32_t u4 __attribute__((ext_vector_type(4)));
        static_assert(V == 4, "the wide form stores 16 bytes");
        if (gain) __builtin_nontemporal_store((f4){gv[0], gv[1], gv[2], gv[3]}, reinterpret_cast<f4 *>(gain + at));
        if (dq) __builtin_nontemporal_store((u4){qv[0], qv[1], qv[2], qv[3]}, reinterpret_cast<u4 *>(dq + at));
    }
}

template <typename T, int V>
void launch_ipc4d(rip_ctx *ctx, const float *t, size_t ntab, int nsy, int nsx, int ry, int rx, int nb, int nya, int nxa, void *K) {
    const int nbx = (nxa / V + GF_THREADS - 1) / GF_THREADS;
    hipLaunchKernelGGL((gainfile_ipc4d_kernel<T, V>), dim3((unsigned)nbx * (unsigned)nya), dim3(GF_THREADS), 0, ctx->stream, t + ntab,
                       t + 2 * ntab, t + 3 * ntab, nsy, nsx, ry, rx, nb, nya, nxa, nbx, (T *)K);
}

// the widest store of n-element rows of `size`-byte values that starts every row (and plane) of `base` on its own boundary:
// 16 bytes, 8 bytes, or the single value
int store_width(const void *base, int n, size_t size) {
    for (int v = (int)(16 / size); v > 1; v /= 2)
        if (n % v == 0 && (uintptr_t)base % (v * size) == 0) return v;
    return 1;
}

}   // namespace

// ============================================================================================ C-ABI

int rip_cal_gain_ipc4d(rip_ctx *ctx, const double *means, const uint8_t *good, int nsy, int nsx, int ny, int nx, int nb, int location,
                       float *gain, uint32_t *gain_dq, void *kernel, int kernel_dtype, uint32_t *kernel_dq) {
    if (nsy < 1 || nsx < 1) return rip_fail(ctx, RIP_EINVAL, "cal_gain_ipc4d: a table of %d x %d superpixels", nsy, nsx);
    if (ny < 1 || nx < 1 || (int64_t)(ny / nsy) * nsy != ny || (int64_t)(nx / nsx) * nsx != nx)
        return rip_fail(ctx, RIP_EINVAL, "cal_gain_ipc4d: %d x %d superpixels do not tile a %d x %d frame", nsy, nsx, ny, nx);
    if (nb < 0 || ny <= 2 * (int64_t)nb || nx <= 2 * (int64_t)nb)
        return rip_fail(ctx, RIP_EINVAL, "cal_gain_ipc4d: a border of %d leaves no active pixel on a %d x %d frame", nb, ny, nx);
    if (kernel_dtype != RIP_F32 && kernel_dtype != RIP_F64)
        return rip_fail(ctx, RIP_EINVAL, "cal_gain_ipc4d: kernel dtype code %d is neither RIP_F32 nor RIP_F64", kernel_dtype);
    if (!gain && !gain_dq && !kernel && !kernel_dq) return rip_fail(ctx, RIP_EINVAL, "cal_gain_ipc4d: every output is NULL");
    if (!means || !good) return rip_fail(ctx, RIP_EINVAL, "cal_gain_ipc4d: a table is NULL");
    if (const int rc = rip_check_location(ctx, "cal_gain_ipc4d", "location", location)) return rc;
    const int ry = ny / nsy, rx = nx / nsx, nya = ny - 2 * nb, nxa = nx - 2 * nb;
    const size_t ntab = (size_t)nsy * nsx, npix = (size_t)ny * nx, na = (size_t)nya * nxa, ksize = dsize(kernel_dtype);
    if (npix / GF_THREADS + (size_t)ny > (size_t)INT_MAX / 2)   // one workgroup per row segment, counted in 32 bits
        return rip_fail(ctx, RIP_EINVAL, "cal_gain_ipc4d: a %d x %d frame is beyond the launch grid", ny, nx);
    RIP_HIP(ctx, hipSetDevice(ctx->device));

    // the tables as the script's .astype(np.float32) leaves them: g, aH, aV, aD
    std::vector<float> t32(4 * ntab);
    for (size_t i = 0; i < 4 * ntab; ++i) t32[i] = (float)means[i];
    DevBuf<float> dt(ctx);
    DevBuf<uint8_t> dgood(ctx);
    DevArg<float> pg;
    DevArg<uint32_t> pgq, pkq;
    DevArg<char> pk;
    int rc;
    if ((rc = dt.upload(t32.data(), 4 * ntab)) || (rc = dgood.upload(good, ntab))) return rc;
    if ((rc = pg.out(ctx, gain, npix, location)) || (rc = pgq.out(ctx, gain_dq, npix, location)) ||
        (rc = pk.out(ctx, (char *)kernel, 9 * na * ksize, location)) || (rc = pkq.out(ctx, kernel_dq, na, location)))
        return rc;

    if (pk.p) {
        const int v = store_width(pk.p, nxa, ksize);
        if (kernel_dtype == RIP_F64) {
            if (v == 2) launch_ipc4d<double, 2>(ctx, dt.p, ntab, nsy, nsx, ry, rx, nb, nya, nxa, pk.p);
            else launch_ipc4d<double, 1>(ctx, dt.p, ntab, nsy, nsx, ry, rx, nb, nya, nxa, pk.p);
        } else {
            if (v == 4) launch_ipc4d<float, 4>(ctx, dt.p, ntab, nsy, nsx, ry, rx, nb, nya, nxa, pk.p);
            else if (v == 2) launch_ipc4d<float, 2>(ctx, dt.p, ntab, nsy, nsx, ry, rx, nb, nya, nxa, pk.p);
            else launch_ipc4d<float, 1>(ctx, dt.p, ntab, nsy, nsx, ry, rx, nb, nya, nxa, pk.p);
        }
        RIP_HIP(ctx, hipGetLastError());
    }
    if (pg.p || pgq.p) {
        const bool wide = nx % 4 == 0 && aligned(pg.p, 16) && aligned(pgq.p, 16);   // a null plane does not count
        const int V = wide ? 4 : 1, nbx = (nx / V + GF_THREADS - 1) / GF_THREADS;
        if (wide)
            hipLaunchKernelGGL(gainfile_gain_kernel<4>, dim3((unsigned)nbx * (unsigned)ny), dim3(GF_THREADS), 0, ctx->stream, dt.p, dgood.p,
                               nsx, ry, rx, nb, ny, nx, nbx, pg.p, pgq.p);
        else
            hipLaunchKernelGGL(gainfile_gain_kernel<1>, dim3((unsigned)nbx * (unsigned)ny), dim3(GF_THREADS), 0, ctx->stream, dt.p, dgood.p,
                               nsx, ry, rx, nb, ny, nx, nbx, pg.p, pgq.p);
        RIP_HIP(ctx, hipGetLastError());
    }
    // the ipc4d flags: the script convolves its bad-pixel map with an all-zero 3 x 3 kernel, so every pixel comes out good
    if (pkq.p) RIP_HIP(ctx, hipMemsetAsync(pkq.p, 0, na * sizeof(uint32_t), ctx->stream));
    if ((rc = pg.download()) || (rc = pgq.download()) || (rc = pk.download()) || (rc = pkq.download())) return rc;
    return dev_sync(ctx);
}
