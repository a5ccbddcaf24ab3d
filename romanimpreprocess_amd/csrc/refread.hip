// Level-1 exposures stored with the reference read subtracted: the inverse of the EXTRACT_REF block (sim_to_isim.py:711-730,
// rip_synth_extract_ref in synth.hip).  The encoder keeps resultant 0 as reference_read and stores, for every other resultant,
// clip(i32(data[k]) - (i32(data[0]) - offset), 0, 65535); the decoder gives back v = i32(enc) + i32(reference_read) - offset.
// In the reference the decoding is romancal's (dq-init, gen_cal_image.py:117-118), whose source is not in the reference tree:
// what pins the semantics is the encoder itself, the two places that expect a cube one group shorter than the CALDIR arrays
// (gen_cal_image.py:561-562, gen_noise_image.py:104-111) and the workflow test that compares the L2 image of an encoded run with
// the plain one (tests/romanimpreprocess/test_workflow.py:871-874).  DESIGN.md section 7.
//   rip_stage_decode_reference_read   host arrays or device pointers (include/romanhip.h)
//   rip_launch_decode_reference_read  what rip_upload_host_ramp (calibrate.hip) queues behind the upload of such a ramp
// For everything the encoder made of u16 data v lies in 0..65535 (not clipped: the original sample; clipped at 0: reference -
// offset >= the original; clipped at 65535: below the original), so the decoded cube is a u16 cube and takes the fused kernel's
// u16 ingest.  A v outside means that the pieces do not belong together: the sample is clamped and COUNTED, and the caller refuses.
#include "rip_host.h"

namespace {

__device__ __forceinline__ uint32_t rr_decode(uint32_t enc, int shift, unsigned long long &bad) {
    const int v = (int)enc + shift;   // |shift| <= 65535 + 2^30: no overflow
    const int c = v < 0 ? 0 : (v > 65535 ? 65535 : v);
    bad += (c != v) ? 1ull : 0ull;
    return (uint32_t)c;
}

// W8: one thread per eight adjacent pixels -- the reference samples are loaded once as 16 bytes and kept as reference - offset,
// then one 16-byte load and one 16-byte store per group: the reference plane is read once, not ngrp times.  Needs n % 8 == 0
// (plane k starts at element k * n) and 16-byte aligned base pointers.  Otherwise one thread per pixel.  out may be data: a thread
// stores only what it has loaded itself.  The count goes wave by wave: one 64-bit vector atomic from a wave that has something
// to add, none from the others.  Every thread of the block reaches the shuffles.
template <bool W8>
__global__ __launch_bounds__(256) void decode_ref_kernel(const uint16_t *data, int ngrp, size_t n, const uint16_t *__restrict__ ref,
                                                         int offset, uint16_t *out, unsigned long long *count) {
    constexpr int V = W8 ? 8 : 1;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n / V;   // (W8: n is a multiple of 8)
    unsigned long long bad = 0;
    if (live) {
        const size_t p = i * V;
        if (W8) {
            const uint4 r = *reinterpret_cast<const uint4 *>(ref + p);
            const uint32_t rw[4] = {r.x, r.y, r.z, r.w};
            int shift[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                shift[2 * j] = (int)(rw[j] & 0xFFFFu) - offset;
                shift[2 * j + 1] = (int)(rw[j] >> 16) - offset;
            }
            for (int k = 0; k < ngrp; ++k) {
                const size_t at = (size_t)k * n + p;
                const uint4 q = *reinterpret_cast<const uint4 *>(data + at);
                const uint32_t w[4] = {q.x, q.y, q.z, q.w};
                uint32_t o[4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    o[j] = rr_decode(w[j] & 0xFFFFu, shift[2 * j], bad) | (rr_decode(w[j] >> 16, shift[2 * j + 1], bad) << 16);
                *reinterpret_cast<uint4 *>(out + at) = make_uint4(o[0], o[1], o[2], o[3]);
            }
        } else {
            const int shift = (int)ref[p] - offset;
            for (int k = 0; k < ngrp; ++k) {
                const size_t at = (size_t)k * n + p;
                out[at] = (uint16_t)rr_decode(data[at], shift, bad);
            }
        }
    }
    if (!__any(bad != 0)) return;   // wave-uniform
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) bad += __shfl_xor(bad, d, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(count, bad);
}

}   // namespace

int rip_launch_decode_reference_read(rip_ctx *ctx, const uint16_t *data, int ngrp, size_t n, const uint16_t *ref, int offset,
                                     uint16_t *out, unsigned long long *count, hipStream_t stream) {
    hipStream_t st = stream ? stream : ctx->stream;
    const bool w8 = n % 8 == 0 && aligned(data, 16) && aligned(ref, 16) && aligned(out, 16);
    const size_t threads = w8 ? n / 8 : n;
    const size_t blocks = (threads + 255) / 256;
    if (blocks > 0x7FFFFFFFu) return rip_fail(ctx, RIP_EINVAL, "decode_reference_read: %zu pixels a plane are more than one launch takes", n);
    if (w8)
        hipLaunchKernelGGL(decode_ref_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, data, ngrp, n, ref, offset, out, count);
    else
        hipLaunchKernelGGL(decode_ref_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, data, ngrp, n, ref, offset, out, count);
    RIP_HIP(ctx, hipGetLastError());
    return RIP_OK;
}

int rip_refread_words(rip_ctx *ctx, int n) {
    if (n <= ctx->refread_cap) return RIP_OK;
    if (ctx->refread_dev) (void)hipFree(ctx->refread_dev);
    if (ctx->refread_host) (void)hipHostFree(ctx->refread_host);
    ctx->refread_dev = ctx->refread_host = nullptr;
    ctx->refread_cap = 0;
    const int cap = n < 16 ? 16 : n;
    hipError_t e = hipMalloc((void **)&ctx->refread_dev, (size_t)cap * 8);
    if (e == hipSuccess) e = hipHostMalloc((void **)&ctx->refread_host, (size_t)cap * 8, hipHostMallocDefault);
    if (e != hipSuccess) {
        if (ctx->refread_dev) (void)hipFree(ctx->refread_dev);
        ctx->refread_dev = nullptr;
        return rip_fail(ctx, RIP_ENOMEM, "decode_reference_read: counting words: %s", hipGetErrorString(e));
    }
    ctx->refread_cap = cap;
    return RIP_OK;
}

extern "C" int rip_stage_decode_reference_read(rip_ctx *ctx, const uint16_t *data, int ngrp, size_t n, const uint16_t *reference_read,
                                               int offset, int location, uint16_t *out, uint64_t *n_out_of_range) {
    if (!data || !reference_read || !out || !n_out_of_range)
        return rip_fail(ctx, RIP_EINVAL, "decode_reference_read: a required array is NULL");
    if (ngrp < 1 || n < 1) return rip_fail(ctx, RIP_EINVAL, "decode_reference_read: %d groups of %zu pixels", ngrp, n);
    if (offset > (1 << 30) || offset < -(1 << 30))
        return rip_fail(ctx, RIP_EINVAL, "decode_reference_read: data_encoding_offset %d (|offset| <= 2^30 supported)", offset);
    if (const int rc = rip_check_location(ctx, "decode_reference_read", "location", location)) return rc;
    const size_t total = (size_t)ngrp * n;
    if (total / n != (size_t)ngrp || total > ((size_t)1 << 62))
        return rip_fail(ctx, RIP_EINVAL, "decode_reference_read: %d groups of %zu pixels", ngrp, n);
    if (out != data && (uintptr_t)out < (uintptr_t)(data + total) && (uintptr_t)data < (uintptr_t)(out + total))
        return rip_fail(ctx, RIP_EINVAL, "decode_reference_read: out overlaps data without being equal to it");
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    // (the next overlapped rip_calibrate orders its pre-pass behind this work: these may be its inputs)
    if (location == RIP_DEVICE) ctx->stream_dirty = true;
    DevArg<uint16_t> o, ref;
    DevArg<unsigned long long> cnt;
    int rc;
    if ((rc = o.out(ctx, out, total, location))) return rc;
    const uint16_t *d = data;
    if (location == RIP_HOST) {   // a host cube is decoded in place, in the buffer of the result
        if ((rc = o.buf.copy_in(data, total))) return rc;
        d = o.p;
    }
    if ((rc = ref.in(ctx, reference_read, n, location)) || (rc = cnt.out(ctx, (unsigned long long *)n_out_of_range, 1, location)))
        return rc;
    RIP_HIP(ctx, hipMemsetAsync(cnt.p, 0, 8, ctx->stream));
    if ((rc = rip_launch_decode_reference_read(ctx, d, ngrp, n, ref.p, offset, o.p, cnt.p)) || (rc = o.download()) || (rc = cnt.download()))
        return rc;
    return location == RIP_DEVICE ? RIP_OK : dev_sync(ctx);   // device pointers: queued, not waited for
}
