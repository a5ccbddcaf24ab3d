// FITS data units made on the device: native samples -> FITS storage order (the bytes of each sample reversed), with the BZERO
// convention of the unsigned / signed-byte types (most significant bit inverted) and, for float32, the substitution of a fill
// value under a byte mask -- the inverse of what DarkStack.add(..., fits_be16=True) undoes on the way in (darkstack.hip).
// The reference writes these arrays through astropy (gen_cal_image.py:725-736, gen_noise_image.py:387-391, maskhandling.py:
// 145-149, the _asdf_data.fits dumps of the calibration-file scripts); here the arrays are in HBM already and the writer
// (calio.write_fits) takes the encoded bytes chunk by chunk.  DESIGN.md section 7.
//   rip_stage_fits_encode   host arrays or device pointers, source and destination independently (include/romanhip.h)
// One kernel per sample width.  Samples [head, head + nvec * V) -- V = 16 / W samples, both addresses 16-byte aligned there --
// go as one 16-byte load and one 16-byte store per lane and iteration; the samples before and behind them, and every sample
// of a pointer pair whose alignments differ (nvec = 0), go one per lane.  dst may be src: a lane stores only what it has loaded
// itself, in the same iteration.  Capped grid, grid-stride loops, 64-bit indices.  Exact (bytes are moved, never computed on).
#include <cstring>

#include "rip_host.h"

// The vector body's stores are non-temporal where dst is not src: the destination is written once and read by a copy engine,
// and in one process the kernel then takes 0.96 of its time with plain stores (f32, f64, i16 and the masked form alike); in
// place the hint costs 1.6 %, so that form keeps plain stores (profiles/fits_out.txt).  -DRIP_FITS_PLAIN_STORES=1 builds the
// library without the hint: the variant tools/gpu_checks/fits_encode_timing.py --variant times against this one.
#ifndef RIP_FITS_PLAIN_STORES
#define RIP_FITS_PLAIN_STORES 0
#endif

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr unsigned FITS_BLOCK = 256, FITS_MAX_BLOCKS = 2048;   // 8 blocks for each of the 256 compute units

// one dword of samples of W bytes: `fx` inverts their most significant bits (0: no BZERO), then the bytes of each are reversed.
// (W = 8: the caller also swaps the two dwords of a sample.)
template <int W>
__device__ __forceinline__ uint32_t enc_dword(uint32_t x, uint32_t fx) {
    x ^= fx;
    if (W == 2) return ((uint32_t)__builtin_bswap16((uint16_t)(x >> 16)) << 16) | __builtin_bswap16((uint16_t)x);
    if (W >= 4) return __builtin_bswap32(x);
    return x;
}

template <int W>
__device__ __forceinline__ void enc_sample(const unsigned char *src, unsigned char *dst, size_t i, uint32_t fx) {
    if (W == 1) dst[i] = (unsigned char)(src[i] ^ (unsigned char)fx);
    if (W == 2) {
        const uint16_t v = reinterpret_cast<const uint16_t *>(src)[i];
        reinterpret_cast<uint16_t *>(dst)[i] = __builtin_bswap16((uint16_t)(v ^ (uint16_t)fx));
    }
    if (W == 4) {
        const uint32_t v = reinterpret_cast<const uint32_t *>(src)[i];
        reinterpret_cast<uint32_t *>(dst)[i] = __builtin_bswap32(v ^ fx);
    }
    if (W == 8) {
        const uint64_t v = reinterpret_cast<const uint64_t *>(src)[i];
        reinterpret_cast<uint64_t *>(dst)[i] = __builtin_bswap64(v);
    }
}

// MASK (W = 4 only): sample i becomes `fill` where (mask[i] != 0) == sense, before the reversal.  mask_dword: mask + head is
// 4-byte aligned, so the four mask bytes of a vector are one dword load.  NT: non-temporal stores in the vector body.
template <int W, bool MASK, bool NT>
__global__ __launch_bounds__(FITS_BLOCK) void fits_encode_kernel(const unsigned char *src, unsigned char *dst,
                                                                 const uint8_t *__restrict__ mask, bool sense, uint32_t fill, uint32_t fx,
                                                                 size_t head, size_t nvec, size_t n, bool mask_dword) {
    static_assert(!MASK || W == 4, "the masked form is float32's");
    constexpr size_t V = 16 / W;
    const size_t gid = (size_t)blockIdx.x * FITS_BLOCK + threadIdx.x, stride = (size_t)gridDim.x * FITS_BLOCK;
    const u32x4 *vs = reinterpret_cast<const u32x4 *>(src + head * W);
    u32x4 *vd = reinterpret_cast<u32x4 *>(dst + head * W);
    for (size_t v = gid; v < nvec; v += stride) {
        u32x4 q = vs[v];
        if (MASK) {
            const uint8_t *m = mask + head + v * 4;
            const uint32_t mm = mask_dword ? *reinterpret_cast<const uint32_t *>(m)
                                           : ((uint32_t)m[0] | ((uint32_t)m[1] << 8) | ((uint32_t)m[2] << 16) | ((uint32_t)m[3] << 24));
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((((mm >> (8 * j)) & 0xFFu) != 0) == sense) q[j] = fill;
        }
        u32x4 o;
        if (W == 8) {
            o[0] = enc_dword<W>(q[1], 0), o[1] = enc_dword<W>(q[0], 0), o[2] = enc_dword<W>(q[3], 0), o[3] = enc_dword<W>(q[2], 0);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = enc_dword<W>(q[j], fx);
        }
        if (NT)
            __builtin_nontemporal_store(o, vd + v);
        else
            vd[v] = o;
    }
    // the samples in front of the vector body and behind it (all of them where there is no body)
    const size_t tail0 = head + nvec * V, nscalar = head + (n - tail0);
    for (size_t s = gid; s < nscalar; s += stride) {
        const size_t i = s < head ? s : tail0 + (s - head);
        if (MASK) {
            const uint32_t v = ((mask[i] != 0) == sense) ? fill : reinterpret_cast<const uint32_t *>(src)[i];
            reinterpret_cast<uint32_t *>(dst)[i] = __builtin_bswap32(v);
        } else {
            enc_sample<W>(src, dst, i, fx);
        }
    }
}

// device pointers; w = |bitpix| / 8
int launch_fits_encode(rip_ctx *ctx, const void *src, int w, bool flip, size_t n, const uint8_t *mask, bool sense, float fill, void *dst) {
    const uintptr_t sa = (uintptr_t)src, da = (uintptr_t)dst;
    size_t head = n, nvec = 0;
    if ((sa & 15) == (da & 15)) {   // (both multiples of w: checked by the entry)
        head = ((16 - (sa & 15)) & 15) / (size_t)w;
        if (head > n) head = n;
        nvec = (n - head) / (size_t)(16 / w);
    }
    const size_t nscalar = n - nvec * (size_t)(16 / w), items = nvec > nscalar ? nvec : nscalar;
    size_t blocks = (items + FITS_BLOCK - 1) / FITS_BLOCK;
    if (blocks > FITS_MAX_BLOCKS) blocks = FITS_MAX_BLOCKS;
    const uint32_t fx = !flip ? 0u : (w == 1 ? 0x80808080u : (w == 2 ? 0x80008000u : 0x80000000u));
    uint32_t fillbits;
    memcpy(&fillbits, &fill, 4);
    const bool mdw = mask && (((uintptr_t)mask + head) & 3) == 0;
    const unsigned char *s = (const unsigned char *)src;
    unsigned char *d = (unsigned char *)dst;
    const dim3 grid((unsigned)blocks), block(FITS_BLOCK);
    const bool nt = !RIP_FITS_PLAIN_STORES && src != dst;
#define RIP_FITS_LAUNCH(W, M)                                                                                                             \
    do {                                                                                                                                  \
        if (nt)                                                                                                                           \
            hipLaunchKernelGGL((fits_encode_kernel<W, M, true>), grid, block, 0, ctx->stream, s, d, mask, sense, fillbits, fx, head, nvec, \
                               n, mdw);                                                                                                   \
        else                                                                                                                              \
            hipLaunchKernelGGL((fits_encode_kernel<W, M, false>), grid, block, 0, ctx->stream, s, d, mask, sense, fillbits, fx, head,      \
                               nvec, n, mdw);                                                                                             \
    } while (0)
    if (mask) RIP_FITS_LAUNCH(4, true);
    else if (w == 1) RIP_FITS_LAUNCH(1, false);
    else if (w == 2) RIP_FITS_LAUNCH(2, false);
    else if (w == 4) RIP_FITS_LAUNCH(4, false);
    else RIP_FITS_LAUNCH(8, false);
#undef RIP_FITS_LAUNCH
    RIP_HIP(ctx, hipGetLastError());
    return RIP_OK;
}

}   // namespace

extern "C" int rip_stage_fits_encode(rip_ctx *ctx, const void *src, int bitpix, int flip_sign, size_t n, int src_location,
                                     const uint8_t *mask, int mask_sense, float fill, void *dst, int dst_location) {
    if (bitpix != 8 && bitpix != 16 && bitpix != 32 && bitpix != -32 && bitpix != -64)
        return rip_fail(ctx, RIP_EINVAL, "fits_encode: bitpix %d is not one of 8, 16, 32, -32, -64", bitpix);
    if (flip_sign && bitpix < 0) return rip_fail(ctx, RIP_EINVAL, "fits_encode: flip_sign with the float bitpix %d", bitpix);
    if (mask && bitpix != -32) return rip_fail(ctx, RIP_EINVAL, "fits_encode: mask with bitpix %d (float32 samples only)", bitpix);
    if (n == 0) return rip_fail(ctx, RIP_EINVAL, "fits_encode: n is 0");
    if (!src) return rip_fail(ctx, RIP_EINVAL, "fits_encode: src is NULL");
    if (!dst) return rip_fail(ctx, RIP_EINVAL, "fits_encode: dst is NULL");
    int rc;
    if ((rc = rip_check_location(ctx, "fits_encode", "src_location", src_location)) ||
        (rc = rip_check_location(ctx, "fits_encode", "dst_location", dst_location)))
        return rc;
    const int w = (bitpix < 0 ? -bitpix : bitpix) / 8;
    if (n > ((size_t)1 << 60)) return rip_fail(ctx, RIP_EINVAL, "fits_encode: n = %zu samples", n);
    const size_t bytes = n * (size_t)w;
    if (src_location == dst_location && src != dst && ranges_meet(src, bytes, dst, bytes))
        return rip_fail(ctx, RIP_EINVAL, "fits_encode: dst overlaps src without being equal to it");
    if (mask && src_location == dst_location && ranges_meet(mask, n, dst, bytes))
        return rip_fail(ctx, RIP_EINVAL, "fits_encode: dst overlaps mask");
    // device memory is used where it is: the kernel's loads and stores are sample-wide at least
    if (src_location == RIP_DEVICE && !aligned(src, w))
        return rip_fail(ctx, RIP_EINVAL, "fits_encode: the device pointer src is not aligned to the %d-byte sample", w);
    if (dst_location == RIP_DEVICE && !aligned(dst, w))
        return rip_fail(ctx, RIP_EINVAL, "fits_encode: the device pointer dst is not aligned to the %d-byte sample", w);
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const bool sense = mask_sense != 0;
    const bool queued = src_location == RIP_DEVICE && dst_location == RIP_DEVICE;   // device to device: not waited for
    if (queued) ctx->stream_dirty = true;   // (the next overlapped rip_calibrate orders its pre-pass behind this work)
    // a host source is encoded in place in dst's device memory (dst itself, or the scoped buffer of a host dst); the call
    // returns when the bytes have arrived
    DevArg<unsigned char> d;
    DevArg<uint8_t> m;
    if ((rc = d.out(ctx, (unsigned char *)dst, bytes, dst_location))) return rc;
    const void *s = src;
    if (src_location == RIP_HOST) {
        RIP_HIP(ctx, hipMemcpyAsync(d.p, src, bytes, hipMemcpyDefault, ctx->stream));
        s = d.p;
    }
    if ((rc = m.in(ctx, mask, n, src_location)) || (rc = launch_fits_encode(ctx, s, w, flip_sign != 0, n, m.p, sense, fill, d.p)) ||
        (rc = d.download()))
        return rc;
    return queued ? RIP_OK : dev_sync(ctx);
}
