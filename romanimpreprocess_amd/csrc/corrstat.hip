// Pair statistics of two flat (or dark) exposures per superpixel: the device half of the drop-in for solid-waffle's
// correlation_run (lines 48-64 of the reference's runs/2026_July/make_sca_files_2026Jul.job), whose summaries make_gain_file.py
// expands into the gain and ipc4d files.  solid-waffle's source is not in the reference tree: the rule stated in
// include/romanhip.h and DESIGN.md section 7 IS the specification and parity with solid-waffle is unpinned.  What pins the
// estimator is the package's own generator (L1Synth): calfiles/corrstack.py: solve_summary inverts it, tested by round trip.
//   rip_cal_corr_pair   the 25 integer sums of every superpixel of one pair of exposures
// tests/corr_ref.py restates them in numpy.  Everything here is an integer: no order of threads changes a bit.
// Bounds (samples <= 65535, a superpixel of at most 16384 pixels): |e| <= 131070 (18 bits with its sign), e^2 and e_p e_q
// <= 1.72e10, their sums < 2^48; the CDS sums < 2^32; all slots are int64.
#include "rip_host.h"
#include "rip_samples.h"
#include "rip_select.h"

namespace {

#define CR_THREADS 256
#define CR_MAX_PIX 16384        // 128 x 128 (NBIN 32 32 on 4096): 64 KiB of int32 in LDS
#define CR_SLOTS 25
#define CR_NSUM 22              // slots 0 .. 21 are sums over the lanes; 22 .. 24 the three ranks
#define CR_OFF 131072           // e + CR_OFF in [2, 262142]: the 18-bit key, 11 bits in the first level, 7 in the second
#define CR_LOW 7
#define CR_BORDER INT32_MIN     // the tile word of a pixel in the frame's border: never counted, never kept

struct CrFrames {
    const uint16_t *p[2][4];    // the first sample of the frames a, b, c, d of the two exposures; rows are nx_file samples
};

// the three CDS sums of one pixel from its eight samples v[exposure][frame a, b, c, d]
struct CrCds {
    int e, ab, cd, ad;
};
__device__ __forceinline__ CrCds cr_cds(const int (&v)[2][4]) {
    const int ad1 = v[0][3] - v[0][0], ad2 = v[1][3] - v[1][0];
    return {ad1 - ad2, (v[0][1] - v[0][0]) + (v[1][1] - v[1][0]), (v[0][3] - v[0][2]) + (v[1][3] - v[1][2]), ad1 + ad2};
}

// a lane meets at most CR_MAX_PIX / CR_THREADS pixels in a pass (twice that for the CDS sums, added in one pass and taken off in
// another): its sums of e and of the CDS sums fit in 32 bits, and so do a wave's
static_assert(2ll * (CR_MAX_PIX / CR_THREADS) * 64 * 131070 < 0x7FFFFFFFll, "32-bit lane and wave sums");

// One workgroup per superpixel (blockIdx.y, blockIdx.x) of sy x sx pixels.
//   1  the eight samples of every pixel are read once (W8: a lane takes 8 adjacent pixels of a row, one 16-byte load per frame;
//      else one pixel): e goes to the LDS tile (CR_BORDER for a border pixel), the first-level histogram of its key is counted,
//      and the lane sums the three CDS sums of ALL its n0 pixels
//   2  the three ranks by a two-level histogram selection in LDS (sel_find_bin): 2048 bins of the top 11 key bits, shared by
//      the ranks, then 128 bins of the low 7 bits per rank
//   3  one pass over the tile, the neighbours read from LDS.  |e - q50| * 1349 <= 5000 (q75 - q25) is, for integers, |e - q50|
//      <= T with T = 5000 (q75 - q25) / 1349 rounded down (formed in 64 bits): two comparisons with q50 -+ T, which CR_BORDER
//      fails.  A pixel that is not kept is rare: its samples are read again and its CDS sums taken off the lane's totals
//      (integers: exact).  Only the sums of products are 64-bit in the lane
//   4  the 22 sums meet by wave shuffles and LDS; lane k of the workgroup owns slot k and stores it
// n0 depends on the geometry only: every lane takes the same path to every barrier.
template <bool W8>
__global__ __launch_bounds__(CR_THREADS) void corr_pair_kernel(const CrFrames src, int nx_file, int ny, int nx, int nb, int sy, int sx,
                                                               int be16, int64_t *__restrict__ out) {
    extern __shared__ __align__(16) int32_t tile[];   // sy * sx
    __shared__ uint32_t hist[SEL_BINS];
    __shared__ uint32_t part[CR_THREADS / 64];
    __shared__ uint32_t sel[3][2];
    __shared__ int32_t qs[3];
    __shared__ long long red[CR_THREADS / 64][CR_NSUM];

    const int tid = threadIdx.x;
    const int y0 = blockIdx.y * sy, x0 = blockIdx.x * sx, npix = sy * sx;
    int64_t *o = out + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * CR_SLOTS;
    const int ylo = max(y0, nb), yhi = min(y0 + sy, ny - nb), xlo = max(x0, nb), xhi = min(x0 + sx, nx - nb);
    const int n0 = (yhi > ylo && xhi > xlo) ? (yhi - ylo) * (xhi - xlo) : 0;
    if (n0 == 0) {   // a superpixel inside the border
        if (tid < CR_SLOTS) o[tid] = 0;
        return;
    }
    const int stored = be16 != 0;
    // the eight samples of the pixel at sample `at` of every frame
    auto samples = [&](size_t at, int(&v)[2][4]) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                uint32_t x[1];
                load_samples<1>(src.p[s][f] + at, stored, x);
                v[s][f] = (int)x[0];
            }
    };
    for (int k = tid; k < SEL_BINS; k += CR_THREADS) hist[k] = 0u;
    __syncthreads();

    // ---- 1
    int tab = 0, tcd = 0, tad = 0;
    auto pixel = [&](const int(&v)[2][4], int r, int c) {
        const int y = y0 + r, x = x0 + c;
        int word = CR_BORDER;
        if (y >= ylo && y < yhi && x >= xlo && x < xhi) {
            const CrCds s = cr_cds(v);
            word = s.e;
            tab += s.ab, tcd += s.cd, tad += s.ad;
            atomicAdd(&hist[(uint32_t)(s.e + CR_OFF) >> CR_LOW], 1u);
        }
        return word;
    };
    if constexpr (W8) {
        const int cpr = sx >> 3;
        for (int ch = tid; ch < sy * cpr; ch += CR_THREADS) {
            const int r = ch / cpr, c = (ch - r * cpr) << 3;
            const size_t at = (size_t)(y0 + r) * nx_file + x0 + c;
            uint32_t x[2][4][8];
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int f = 0; f < 4; ++f) load_samples<8>(src.p[s][f] + at, stored, x[s][f]);
            int32_t words[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                int v[2][4];
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int f = 0; f < 4; ++f) v[s][f] = (int)x[s][f][k];
                words[k] = pixel(v, r, c + k);
            }
            int4 *dst = reinterpret_cast<int4 *>(tile + r * sx + c);   // sx % 8 == 0: 32-byte aligned
            dst[0] = make_int4(words[0], words[1], words[2], words[3]);
            dst[1] = make_int4(words[4], words[5], words[6], words[7]);
        }
    } else {
        for (int i = tid; i < npix; i += CR_THREADS) {
            const int r = i / sx, c = i - r * sx;
            int v[2][4];
            samples((size_t)(y0 + r) * nx_file + x0 + c, v);
            tile[i] = pixel(v, r, c);
        }
    }
    __syncthreads();

    // ---- 2
    const uint32_t rank[3] = {(uint32_t)(n0 - 1) / 4u, (uint32_t)(n0 - 1) / 2u, 3u * (uint32_t)(n0 - 1) / 4u};
    for (int j = 0; j < 3; ++j) {
        uint32_t bin, left;
        if (sel_find_bin<CR_THREADS, SEL_BINS / CR_THREADS>([&](int k) { return hist[tid * (SEL_BINS / CR_THREADS) + k]; }, rank[j], tid, true,
                                                            part, bin, left))
            sel[j][0] = bin, sel[j][1] = left;
        __syncthreads();
    }
    const uint32_t top[3] = {sel[0][0], sel[1][0], sel[2][0]}, left2[3] = {sel[0][1], sel[1][1], sel[2][1]};
    for (int k = tid; k < (3 << CR_LOW); k += CR_THREADS) hist[k] = 0u;   // every lane has read its first-level bins: barrier above
    __syncthreads();
    for (int i = tid; i < npix; i += CR_THREADS) {
        const int e = tile[i];
        if (e == CR_BORDER) continue;
        const uint32_t key = (uint32_t)(e + CR_OFF), hi = key >> CR_LOW, lo = key & ((1u << CR_LOW) - 1u);
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (hi == top[j]) atomicAdd(&hist[(j << CR_LOW) + lo], 1u);
    }
    __syncthreads();
    for (int j = 0; j < 3; ++j) {
        uint32_t bin, left;
        const uint32_t *h = hist + (j << CR_LOW);
        if (sel_find_bin<CR_THREADS, SEL_BINS / CR_THREADS>(
                [&](int k) {
                    const int b = tid * (SEL_BINS / CR_THREADS) + k;
                    return b < (1 << CR_LOW) ? h[b] : 0u;
                },
                left2[j], tid, true, part, bin, left))
            qs[j] = (int32_t)((top[j] << CR_LOW) | bin) - CR_OFF;
        __syncthreads();
    }
    const int q50 = qs[1];
    const int T = (int)(5000ll * ((long long)qs[2] - qs[0]) / 1349ll);   // at most 971608
    const int klo = q50 - T, khi = q50 + T;
    auto kept = [&](int e) { return e >= klo && e <= khi; };

    // ---- 3
    int cnt = 0, se = 0, m[4] = {0, 0, 0, 0}, sp[4] = {0, 0, 0, 0}, sq[4] = {0, 0, 0, 0};
    long long see = 0, spq[4] = {0, 0, 0, 0};
    const int dr = CR_THREADS / sx, dc = CR_THREADS - dr * sx;   // the lane's next pixel, without a division
    int r = tid / sx, c = tid - r * sx;
    const int off[4] = {1, sx, sx + 1, sx - 1};
    for (int i = tid; i < npix; i += CR_THREADS) {
        const int e = tile[i];
        if (kept(e)) {
            cnt += 1, se += e, see += (long long)e * e;
            const bool down = r + 1 < sy;
            // the shifts (dy, dx) = (0,1), (1,0), (1,1), (1,-1); a partner outside the superpixel does not count
            const bool in[4] = {c + 1 < sx, down, down && c + 1 < sx, down && c >= 1};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int q = in[s] ? tile[i + off[s]] : CR_BORDER;
                if (kept(q)) m[s] += 1, sp[s] += e, sq[s] += q, spq[s] += (long long)e * q;
            }
        } else if (e != CR_BORDER) {
            int v[2][4];
            samples((size_t)(y0 + r) * nx_file + x0 + c, v);
            const CrCds s = cr_cds(v);
            tab -= s.ab, tcd -= s.cd, tad -= s.ad;
        }
        r += dr, c += dc;
        if (c >= sx) c -= sx, r += 1;
    }

    // ---- 4: the slots in their order; 32-bit sums stay 32-bit through the wave
    const int narrow[17] = {cnt, se, m[0], sp[0], sq[0], m[1], sp[1], sq[1], m[2], sp[2], sq[2], m[3], sp[3], sq[3], tab, tcd, tad};
    const int narrow_slot[17] = {0, 1, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15, 16, 17, 19, 20, 21};
    const long long wide[5] = {see, spq[0], spq[1], spq[2], spq[3]};
    const int wide_slot[5] = {2, 6, 10, 14, 18};
#pragma unroll
    for (int k = 0; k < 17; ++k) {
        int v = narrow[k];
        for (int sh = 32; sh > 0; sh >>= 1) v += __shfl_xor(v, sh, 64);
        if ((tid & 63) == 0) red[tid >> 6][narrow_slot[k]] = v;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        long long v = wide[k];
        for (int sh = 32; sh > 0; sh >>= 1) v += __shfl_xor(v, sh, 64);
        if ((tid & 63) == 0) red[tid >> 6][wide_slot[k]] = v;
    }
    __syncthreads();
    if (tid < CR_NSUM) {
        long long v = 0;
        for (int w = 0; w < CR_THREADS / 64; ++w) v += red[w][tid];
        o[tid] = v;
    } else if (tid < CR_SLOTS) {
        o[tid] = qs[tid - CR_NSUM];
    }
}

}   // namespace

// ============================================================================================ C-ABI

int rip_cal_corr_pair(rip_ctx *ctx, const uint16_t *cube1, int location1, const uint16_t *cube2, int location2, int nreads, int ny_file,
                      int nx_file, int fits_be16, int fa, int fb, int fc, int fd, int ny, int nx, int nb, int sy, int sx, int64_t *table,
                      int table_location) {
    if (!cube1 || !cube2 || !table) return rip_fail(ctx, RIP_EINVAL, "cal_corr_pair: a required array is NULL");
    int rc;
    if ((rc = rip_check_location(ctx, "cal_corr_pair", "location1", location1)) ||
        (rc = rip_check_location(ctx, "cal_corr_pair", "location2", location2)) ||
        (rc = rip_check_location(ctx, "cal_corr_pair", "table_location", table_location)))
        return rc;
    if (nreads < 1 || ny_file < 1 || nx_file < 1) return rip_fail(ctx, RIP_EINVAL, "cal_corr_pair: a (%d,%d,%d) cube", nreads, ny_file, nx_file);
    if (fa < 0 || fb < 0 || fc < 0 || fd < 0 || fa >= nreads || fb >= nreads || fc >= nreads || fd >= nreads)
        return rip_fail(ctx, RIP_EINVAL, "cal_corr_pair: TIME %d %d %d %d asks for frames outside a cube of %d", fa + 1, fb + 1, fc + 1, fd + 1,
                        nreads);
    if (!(fa < fb && fc < fd && fa < fd))
        return rip_fail(ctx, RIP_EINVAL, "cal_corr_pair: TIME %d %d %d %d (a < b, c < d and a < d are needed)", fa + 1, fb + 1, fc + 1, fd + 1);
    if (ny < 1 || nx < 1 || ny > ny_file || nx > nx_file || nb < 0)
        return rip_fail(ctx, RIP_EINVAL, "cal_corr_pair: a frame of (%d,%d) with a border of %d in a file of (%d,%d)", ny, nx, nb, ny_file, nx_file);
    if (sy < 1 || sx < 1 || ny % sy != 0 || nx % sx != 0)
        return rip_fail(ctx, RIP_EINVAL, "cal_corr_pair: NBIN: superpixels of (%d,%d) do not divide the frame of (%d,%d)", sy, sx, ny, nx);
    if ((int64_t)sy * sx > CR_MAX_PIX)
        return rip_fail(ctx, RIP_EINVAL, "cal_corr_pair: NBIN: a superpixel of (%d,%d) has %ld pixels (at most %d: it is held in LDS)", sy, sx,
                        (long)((int64_t)sy * sx), CR_MAX_PIX);
    const int nby = ny / sy, nbx = nx / sx;
    if (nby > 65535) return rip_fail(ctx, RIP_EINVAL, "cal_corr_pair: NBIN: %d rows of superpixels (at most 65535)", nby);
    RIP_HIP(ctx, hipSetDevice(ctx->device));

    const int frames[4] = {fa, fb, fc, fd};
    const uint16_t *cubes[2] = {cube1, cube2};
    const int locations[2] = {location1, location2};
    const size_t plane = (size_t)ny * nx_file;
    DevBuf<uint16_t> rows[2] = {DevBuf<uint16_t>(ctx), DevBuf<uint16_t>(ctx)};   // of a host cube only the rows of the four frames travel
    CrFrames src;
    bool w8 = sx % 8 == 0 && nx_file % 8 == 0;
    for (int s = 0; s < 2; ++s) {
        if (locations[s] == RIP_HOST && (rc = rows[s].alloc(4 * plane))) return rc;
        for (int f = 0; f < 4; ++f) {
            CubeBand band(ctx);   // one frame
            uint16_t *into = rows[s].p ? rows[s].p + f * plane : nullptr;
            if ((rc = band.in(cubes[s], locations[s], ny_file, nx_file, frames[f], 1, 0, ny, into))) return rc;
            src.p[s][f] = band.p;
            w8 = w8 && aligned(src.p[s][f], 16);
        }
    }
    DevArg<int64_t> t;
    if ((rc = t.out(ctx, table, (size_t)nby * nbx * CR_SLOTS, table_location))) return rc;
    const size_t lds = (size_t)sy * sx * 4;
    const dim3 grid((unsigned)nbx, (unsigned)nby);
    if ((rc = with_lds(ctx, RIP_W8_KERNEL(corr_pair_kernel, w8), lds))) return rc;
    RIP_LAUNCH_W8(corr_pair_kernel, w8, grid, dim3(CR_THREADS), lds, ctx->stream, src, nx_file, ny, nx, nb, sy, sx, fits_be16, t.p);
    RIP_HIP(ctx, hipGetLastError());
    if ((rc = t.download())) return rc;
    return dev_sync(ctx);
}
