// A batch of ramps handed over in HOST memory, pipelined over PCIe: while ramp i runs through the chain, ramp i+1 is
// uploaded and the results of ramp i-1 are downloaded (three streams, two sets of device buffers).  The reference's driver
// calls calibrateimage file by file (runs/summer2025run/OpenUniverse_to_L1L2.py:123-137: 18 SCAs x filters per exposure);
// this entry is what a batch driver hands its arrays to.  Each ramp goes through rip_calibrate's device path unchanged, so
// results are those of single calls.  With page-locked host arrays (rip_host_alloc) the copies run at PCIe rate in both
// directions at once (measured: 10.6 ms per 4096 x 4096 x 8 ramp with all outputs, 17.6 ms for single calls); pageable
// arrays work but serialise.  Streams map onto a few hardware queues (four by default), which is why the entry makes none of
// its own: with two extra streams the copies did not overlap at all.
#include "rip_host.h"   // the staging of a host ramp that rip_calibrate's host branch (calibrate.hip) uses as well

namespace {

struct BatchSet {
    char *in = nullptr, *out = nullptr;
    hipEvent_t ev_in = nullptr, ev_done = nullptr, ev_out = nullptr;
    bool used = false;
};

}   // namespace

extern "C" int rip_calibrate_batch(rip_ctx *ctx, int slot, int plan_id, unsigned stages, int n, const rip_ramp_desc *in,
                                   const rip_outputs *out) {
    if (n < 0 || (n > 0 && (!in || !out))) return rip_fail(ctx, RIP_EINVAL, "calibrate_batch: bad arguments");
    if (n == 0) return RIP_OK;
    if (!(stages & RIP_STAGE_RAMPFIT)) return rip_fail(ctx, RIP_EINVAL, "calibrate_batch: the stage mask must include the ramp fit");
    if (slot < 0 || slot >= (int)ctx->cals.size() || !ctx->cals[slot].valid)
        return rip_fail(ctx, RIP_EINVAL, "calibrate_batch: caldir slot %d is empty", slot);
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const RipCal &c = ctx->cals[slot];
    const int ny = c.ny, nx = c.nx, G = in[0].ngrp;
    const size_t npix = (size_t)ny * nx;
    bool encoded = false;
    for (int i = 0; i < n; ++i) {
        if (in[i].location != RIP_HOST || out[i].location != RIP_HOST)
            return rip_fail(ctx, RIP_EINVAL, "calibrate_batch: ramp %d is not in host memory (use rip_calibrate for device pointers)", i);
        if (in[i].ngrp != G || in[i].data_dtype != in[0].data_dtype)
            return rip_fail(ctx, RIP_EINVAL, "calibrate_batch: ramp %d differs in group count or dtype from ramp 0", i);
        if (!in[i].data || !in[i].pixeldq || !out[i].slope || !out[i].err_read || !out[i].err_poisson || !out[i].pixeldq)
            return rip_fail(ctx, RIP_EINVAL, "calibrate_batch: ramp %d lacks a required array", i);
        if (out[i].cube) return rip_fail(ctx, RIP_EINVAL, "calibrate_batch: the corrected cube is not returned by this entry");
        if (const int rc_ref = rip_check_reference_read(ctx, in[i], "calibrate_batch")) return rc_ref;
        encoded = encoded || rip_ramp_is_encoded(in[i]);
    }
    // ramps stored with their reference read subtracted are decoded behind their uploads (rip_upload_host_ramp); ramp i counts its
    // out-of-range samples in word i, and the words come down with the last synchronisation (cleanup)
    if (encoded)
        if (const int rc_ref = rip_refread_words(ctx, n)) return rc_ref;
    if (G < 1 || G > RIP_MAX_GROUPS) return rip_fail(ctx, RIP_EINVAL, "calibrate_batch: %d groups unsupported", G);
    const size_t in_bytes = rip_host_ramp_bytes(in[0], ny, nx), out_bytes = rip_result_bytes(G, npix, true);

    // Streams map onto a few hardware queues (four by default), so no stream is made here: the uploads ride on the context's
    // second stream, in front of the reference-pixel pre-pass of the same ramp; the downloads have the context's third one.
    if (!ctx->stream2 || !ctx->stream3) return rip_fail(ctx, RIP_EHIP, "calibrate_batch: the context has no copy streams");
    hipStream_t s_in = ctx->stream2, s_out = ctx->stream3;
    BatchSet set[2];
    int rc = RIP_OK;
    ctx->batch_completed = 0;  // ramps whose results have been queued for download in full (valid after an error return too)
    ctx->in_batch = true;   // the second stream carries the uploads: no pre-pass gate on it (calibrate.hip)
    int uploaded = 0;   // ramps whose upload (and decoding) has been queued
    int bad_ramp = -1;   // after cleanup: the first ramp whose decoded samples left 0..65535
    unsigned long long bad_count = 0;
    auto cleanup = [&]() {   // waits for every stream; the device buffers stay with the context
        ctx->in_batch = false;
        const bool counts = encoded && uploaded > 0 &&
                            hipMemcpyAsync(ctx->refread_host, ctx->refread_dev, (size_t)uploaded * 8, hipMemcpyDeviceToHost, s_in) == hipSuccess;
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipStreamSynchronize(s_in);
        (void)hipStreamSynchronize(s_out);
        for (auto &b : set)
            for (hipEvent_t e : {b.ev_in, b.ev_done, b.ev_out})
                if (e) (void)hipEventDestroy(e);
        for (int i = 0; counts && i < uploaded && bad_ramp < 0; ++i)
            if (rip_ramp_is_encoded(in[i]) && ctx->refread_host[i] != 0) {
                bad_ramp = i;
                bad_count = ctx->refread_host[i];
            }
        if (bad_ramp >= 0 && ctx->batch_completed > bad_ramp) ctx->batch_completed = bad_ramp;
    };
    // the error of a ramp whose pieces do not belong together takes precedence: it is the first ramp that is not good
    auto verdict = [&](int rc_other) {
        if (bad_ramp < 0) return rc_other;
        return rip_fail(ctx, RIP_EINVAL, "calibrate_batch: ramp %d: %llu samples of the decoded ramp lie outside 0..65535: reference_read, data "
                        "and data_encoding_offset %d do not belong together (%d ramps before it are good)", bad_ramp, bad_count,
                        (int)in[bad_ramp].data_encoding_offset, bad_ramp);
    };
#define BATCH_HIP(call)                                                                         \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            rc = rip_fail(ctx, RIP_EHIP, "%s: %s", #call, hipGetErrorString(e_));               \
            cleanup();                                                                          \
            return verdict(rc);                                                                 \
        }                                                                                       \
    } while (0)
    for (int k = 0; k < 2; ++k) {
        BatchSet &b = set[k];
        for (int io = 0; io < 2; ++io) {
            const int s = 2 * k + io;
            const size_t need = io ? out_bytes : in_bytes;
            if (ctx->batch_bytes[s] < need) {
                if (ctx->batch_buf[s]) (void)hipFree(ctx->batch_buf[s]);
                ctx->batch_buf[s] = nullptr;
                ctx->batch_bytes[s] = 0;
                BATCH_HIP(hipMalloc(&ctx->batch_buf[s], need));
                ctx->batch_bytes[s] = need;
            }
        }
        b.in = (char *)ctx->batch_buf[2 * k];
        b.out = (char *)ctx->batch_buf[2 * k + 1];
        BATCH_HIP(hipEventCreateWithFlags(&b.ev_in, hipEventDisableTiming));
        BATCH_HIP(hipEventCreateWithFlags(&b.ev_done, hipEventDisableTiming));
        BATCH_HIP(hipEventCreateWithFlags(&b.ev_out, hipEventDisableTiming));
    }
    for (int i = 0; i < n; ++i) {
        BatchSet &b = set[i & 1];
        const rip_ramp_desc &ri = in[i];
        const rip_outputs &ro = out[i];
        // upload: the input buffers of this set are free once the chain of ramp i-2 has run
        if (b.used) BATCH_HIP(hipStreamWaitEvent(s_in, b.ev_done, 0));
        rip_ramp_desc rd;
        if (rip_upload_host_ramp(ctx, ri, ny, nx, b.in, s_in, &rd, encoded ? ctx->refread_dev + i : nullptr) != RIP_OK) {
            rc = rip_fail(ctx, RIP_EHIP, "calibrate_batch: upload of ramp %d failed", i);
            cleanup();
            return verdict(rc);
        }
        uploaded = i + 1;
        BATCH_HIP(hipEventRecord(b.ev_in, s_in));
        // chain: after its inputs have landed and the previous results of this set have left
        rd.ready_event = b.ev_in;   // the pre-pass stream and the main stream wait for the upload inside rip_calibrate
        if (b.used) BATCH_HIP(hipStreamWaitEvent(ctx->stream, b.ev_out, 0));
        const rip_outputs od = rip_result_planes(b.out, ro, npix);
        if ((rc = rip_calibrate(ctx, slot, plan_id, stages, &rd, &od)) != RIP_OK) {
            cleanup();
            return verdict(rc);
        }
        BATCH_HIP(hipEventRecord(b.ev_done, ctx->stream));
        // download
        BATCH_HIP(hipStreamWaitEvent(s_out, b.ev_done, 0));
        if ((rc = rip_download_results(ctx, od, ro, G, npix, s_out)) != RIP_OK) {
            cleanup();
            return verdict(rc);
        }
        BATCH_HIP(hipEventRecord(b.ev_out, s_out));
        b.used = true;
        ctx->batch_completed = i + 1;
    }
#undef BATCH_HIP
    cleanup();   // waits for every stream
    return verdict(RIP_OK);
}

extern "C" int rip_calibrate_batch_completed(rip_ctx *ctx) { return ctx ? ctx->batch_completed : RIP_EINVAL; }
