// The chain driver (include/romanhip.h: rip_calibrate) and the staging of a ramp handed over in host memory.  Host code only.
#include <string.h>

#include <cmath>

#include "rip_host.h"

// bytes that take a ramp's inputs: data, amp33, groupdq, pixeldq, area factor, channel lines, reference read, reference amp33,
// each in a 256-byte aligned slot (every array counted, present or not)
size_t rip_host_ramp_bytes(const rip_ramp_desc &in, int ny, int nx) {
    const size_t G = in.ngrp, npix = (size_t)ny * nx;
    return al256(G * npix * (in.data_dtype == RIP_U16 ? 2 : 4)) + al256(G * ny * RIP_CW * 2) + al256(G * npix) + al256(npix * 4) +
           al256(npix * 8) + al256(G * (nx / RIP_CW) * 16) + al256(npix * 2) + al256((size_t)ny * RIP_CW * 2);
}

// what a ramp stored with its reference read subtracted must satisfy (include/romanhip.h, rip_ramp_desc::reference_read)
int rip_check_reference_read(rip_ctx *ctx, const rip_ramp_desc &in, const char *who) {
    if (!rip_ramp_is_encoded(in)) return RIP_OK;
    if (in.location == RIP_DEVICE)
        return rip_fail(ctx, RIP_EINVAL, "%s: reference_read / reference_amp33 come with host ramps only (a device caller decodes its arrays with "
                        "rip_stage_decode_reference_read and calibrates them as usual)", who);
    if (in.reference_read && in.data_dtype != RIP_U16) return rip_fail(ctx, RIP_EINVAL, "%s: reference_read needs u16 data", who);
    if (in.reference_amp33 && !in.amp33) return rip_fail(ctx, RIP_EINVAL, "%s: reference_amp33 without amp33", who);
    if (in.data_encoding_offset > (1 << 30) || in.data_encoding_offset < -(1 << 30))
        return rip_fail(ctx, RIP_EINVAL, "%s: data_encoding_offset %d (|offset| <= 2^30 supported)", who, (int)in.data_encoding_offset);
    return RIP_OK;
}

// queues the copies of the host arrays of `in` into `w` on `st`, in the order above (an absent array takes no slot), and sets
// DO_NOT_USE on the copy of the first group with or_first_group; `dev` = `in` with the device copies in place of the host arrays.
// A ramp stored with its reference read subtracted (checked by the caller: rip_check_reference_read) is decoded in place on the
// device copies of data and amp33, on `st` behind the copies and before anything reads them: `dev` then describes a plain u16
// ramp, and *count (zeroed here, on `st`) receives the samples that left 0..65535.
int rip_upload_host_ramp(rip_ctx *ctx, const rip_ramp_desc &in, int ny, int nx, char *w, hipStream_t st, rip_ramp_desc *dev,
                         unsigned long long *count) {
    const size_t G = in.ngrp, npix = (size_t)ny * nx;
    hipError_t e = hipSuccess;
    auto put = [&](const void *src, size_t bytes) -> void * {
        if (!src) return nullptr;
        void *dst = w;
        w += al256(bytes);
        // (pageable arrays too: the runtime's own staging runs at the page-locked rate -- 16.7 against 16.5 ms per 4096 x 4096 x 8
        // ramp; a ring of page-locked slots fed by copy threads was measured SLOWER, 18.0 ms: profiles/r04_summary.md)
        if (e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
        return dst;
    };
    *dev = in;
    dev->location = RIP_DEVICE;
    dev->or_first_group = 0;
    dev->data = put(in.data, G * npix * (in.data_dtype == RIP_U16 ? 2 : 4));
    dev->amp33 = (const uint16_t *)put(in.amp33, G * ny * RIP_CW * 2);
    dev->groupdq = (const uint8_t *)put(in.groupdq, G * npix);
    dev->pixeldq = (const uint32_t *)put(in.pixeldq, npix * 4);
    dev->area_factor = (const double *)put(in.area_factor, npix * 8);
    dev->channel_lines = (const double *)put(in.channel_lines, G * (nx / RIP_CW) * 16);
    const uint16_t *ref = (const uint16_t *)put(in.reference_read, npix * 2);
    const uint16_t *ref33 = (const uint16_t *)put(in.reference_amp33, (size_t)ny * RIP_CW * 2);
    dev->reference_read = dev->reference_amp33 = nullptr;   // (decoded below: the chain sees a plain ramp)
    dev->data_encoding_offset = 0;
    if (e != hipSuccess) return rip_fail(ctx, RIP_EHIP, "calibrate: upload of the ramp failed: %s", hipGetErrorString(e));
    if (ref || ref33) {
        if (!count) return rip_fail(ctx, RIP_ESTATE, "calibrate: a ramp with a reference read and no counting word");
        RIP_HIP(ctx, hipMemsetAsync(count, 0, 8, st));
        int rc;
        if (ref && (rc = rip_launch_decode_reference_read(ctx, (const uint16_t *)dev->data, (int)G, npix, ref, in.data_encoding_offset,
                                                          (uint16_t *)dev->data, count, st)))
            return rc;
        if (ref33 && (rc = rip_launch_decode_reference_read(ctx, dev->amp33, (int)G, (size_t)ny * RIP_CW, ref33, in.data_encoding_offset,
                                                            (uint16_t *)dev->amp33, count, st)))
            return rc;
    }
    // gen_cal_image.py:142-143 (rdq[0] |= DO_NOT_USE with EXCLUDE_FIRST) on the device copy, so that the host need not copy a
    // 134 MB array to set one plane's bit
    if (in.or_first_group && dev->groupdq) return rip_launch_or_bytes(ctx, (uint8_t *)dev->groupdq, npix, (uint8_t)DQ_DO_NOT_USE, st);
    return RIP_OK;
}

// result planes in one buffer: slope, err_read, err_poisson, pixeldq, then groupdq
size_t rip_result_bytes(int G, size_t npix, bool groupdq) {
    return 4 * al256(npix * 4) + (groupdq ? al256((size_t)G * npix) : 0);
}

// the device planes in `w` for the caller's HOST outputs (groupdq where the caller wants it; never the cube)
rip_outputs rip_result_planes(char *w, const rip_outputs &host, size_t npix) {
    const size_t pl = al256(npix * 4);
    rip_outputs o{};
    o.location = RIP_DEVICE;
    o.slope = (float *)w;
    o.err_read = (float *)(w + pl);
    o.err_poisson = (float *)(w + 2 * pl);
    o.pixeldq = (uint32_t *)(w + 3 * pl);
    o.groupdq = host.groupdq ? (uint8_t *)(w + 4 * pl) : nullptr;
    return o;
}

// queues the copies of the result planes `dev` into the caller's `host` arrays on `st`
int rip_download_results(rip_ctx *ctx, const rip_outputs &dev, const rip_outputs &host, int G, size_t npix, hipStream_t st) {
    RIP_HIP(ctx, hipMemcpyAsync(host.slope, dev.slope, npix * 4, hipMemcpyDeviceToHost, st));
    RIP_HIP(ctx, hipMemcpyAsync(host.err_read, dev.err_read, npix * 4, hipMemcpyDeviceToHost, st));
    RIP_HIP(ctx, hipMemcpyAsync(host.err_poisson, dev.err_poisson, npix * 4, hipMemcpyDeviceToHost, st));
    RIP_HIP(ctx, hipMemcpyAsync(host.pixeldq, dev.pixeldq, npix * 4, hipMemcpyDeviceToHost, st));
    if (host.groupdq) RIP_HIP(ctx, hipMemcpyAsync(host.groupdq, dev.groupdq, (size_t)G * npix, hipMemcpyDeviceToHost, st));
    return RIP_OK;
}

namespace {

// profiling (rip_profile_enable): an event on `st`; every call records six, which rip_profile_read pairs up
void mark(rip_ctx *ctx, hipStream_t st) {
    if (!ctx->prof) return;
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return;
    (void)hipEventRecord(e, st);
    ctx->prof_events.push_back(e);
}

// one rip_calibrate call; each step returns RIP_OK or the error it has recorded
struct Calibration {
    rip_ctx *ctx;
    const RipCal &c;
    unsigned stages;
    const rip_ramp_desc *in;
    const rip_outputs *out;
    RipPlan *plan = nullptr;
    int G = 0, ny = 0, nx = 0, nch = 0;
    size_t npix = 0;
    bool host = false, do_fit = false, do_ref = false, do_bias = false, do_lin = false, do_ipc = false, do_sat = false;
    rip_ramp_desc d{};   // the inputs on the device: the caller's arrays or (host) their copies; the flag pass replaces the dq arrays
    rip_outputs o{};     // the result planes on the device: the caller's or (host) workspace 7
    // reference-pixel tables (rowcorr, its transpose, lines) in workspace 3, double-buffered by call parity
    size_t tab_bytes = 0;
    char *ws3 = nullptr;
    double *rowcorr = nullptr, *rowcorr_t = nullptr, *lines = nullptr;
    int par = 0;
    bool overlap = false;
    hipStream_t pre = nullptr;   // where the pre-pass and the saturation pass of THIS call are launched
    const float *flat = nullptr;        // the plane the slope is divided by
    const float *cur = nullptr;         // the corrected cube
    const uint32_t *pdq_mid = nullptr;  // pixeldq after the cube stage
    bool ran_fused = false;
    bool skip0 = false;   // the fused kernel of this call skips group 0, and the pre-pass leaves its tables out
    bool decoded = false;   // a host ramp stored with its reference read subtracted: decoded on the device behind its upload

    // ---- May this call's fused kernel skip group 0 (option "skip_first")?  Decided before the pre-pass.  Group 0 must be dead in
    // the fit (rip_chain_may_skip_first: the plan, and that the fused kernel WILL run) and known to be finite without being
    // computed: a u16 cube on a CALDIR set that passed the screen at upload (caldir.hip: the chain of bounds), no corrected cube
    // to write, and channel lines that are either the pre-pass's own or a HOST array whose group-0 entries are within the
    // bounds that chain assumes of them (|m| <= 2^32, |c| <= 2^35; lines on the device cannot be looked at here).
    // A bias correction is not required: without one (no biascorr in the set, an all +0 one dropped at upload, or a stage mask
    // without RIP_STAGE_BIAS) the chain of bounds holds with biascorr = 0.
    void choose_skip() {
        skip0 = false;
        if (!(do_ref && do_lin && do_ipc && do_fit && in->data_dtype == RIP_U16 && !out->cube && c.first_group_safe)) return;
        const bool with_flat = (stages & RIP_STAGE_FLAT) && c.has_flat;
        const int merged = c.merged_plane[(with_flat ? 1 : 0) | ((stages & RIP_STAGE_DARK) ? 2 : 0)];   // as fused_chain sets it
        if (!rip_chain_may_skip_first(ctx, plan, c.lin_nplanes, G, c.ipc_dtype, c.gain_dtype, merged, c.nb)) return;
        if (in->channel_lines) {
            if (!host) return;
            for (int ch = 0; ch < nch; ++ch)
                if (!(std::fabs(in->channel_lines[2 * ch]) <= 4294967296.0 && std::fabs(in->channel_lines[2 * ch + 1]) <= 34359738368.0)) return;
        }
        skip0 = true;
    }

    int validate(int slot, int plan_id) {
        if (in->location != out->location) return rip_fail(ctx, RIP_EINVAL, "calibrate: inputs and outputs must share a location");
        if (const int rc = rip_check_reference_read(ctx, *in, "calibrate")) return rc;
        RIP_HIP(ctx, hipSetDevice(ctx->device));
        G = in->ngrp, ny = c.ny, nx = c.nx, nch = nx / RIP_CW;
        npix = (size_t)ny * nx;
        if (G < 1 || G > RIP_MAX_GROUPS) return rip_fail(ctx, RIP_EINVAL, "calibrate: %d groups unsupported", G);
        if (!in->data || (in->data_dtype != RIP_U16 && in->data_dtype != RIP_F32))
            return rip_fail(ctx, RIP_EINVAL, "calibrate: data must be u16 or f32");
        do_fit = stages & RIP_STAGE_RAMPFIT;
        if (do_fit || (stages & RIP_STAGE_LIN)) {
            plan = get_plan(ctx, plan_id);
            if (!plan) return RIP_EINVAL;
            if (plan->h.ngrp != G) return rip_fail(ctx, RIP_EINVAL, "calibrate: ramp has %d groups, plan %d", G, plan->h.ngrp);
        }
        do_ref = stages & RIP_STAGE_REFPIX, do_bias = (stages & RIP_STAGE_BIAS) && c.has_bias;
        do_lin = stages & RIP_STAGE_LIN, do_ipc = (stages & RIP_STAGE_IPC) && c.has_ipc;
        if (do_ref && (!c.dark_data || c.ngrp_dark < G)) return rip_fail(ctx, RIP_EINVAL, "calibrate: dark.data has %d groups, ramp %d", c.ngrp_dark, G);
        // (a biascorr that was all +0 and dropped at upload subtracts nothing, but one with too few planes fails like any other)
        if ((do_bias || ((stages & RIP_STAGE_BIAS) && c.bias_dropped)) && c.ngrp_bias < G)
            return rip_fail(ctx, RIP_EINVAL, "calibrate: biascorr has %d groups, ramp %d", c.ngrp_bias, G);
        if (do_lin && !c.lin_coefs) return rip_fail(ctx, RIP_EINVAL, "calibrate: no linearity arrays in caldir slot %d", slot);
        do_sat = in->flag_saturation != 0;
        if (do_sat && !c.sat_thr) return rip_fail(ctx, RIP_EINVAL, "calibrate: flag_saturation needs the saturation array in caldir slot %d", slot);
        if ((do_fit || do_lin) && ((!in->groupdq && !do_sat) || !in->pixeldq))
            return rip_fail(ctx, RIP_EINVAL, "calibrate: groupdq/pixeldq required");
        if (do_fit && (!out->slope || !out->err_read || !out->err_poisson || !out->pixeldq))
            return rip_fail(ctx, RIP_EINVAL, "calibrate: output planes required");
        if ((stages & RIP_STAGE_DARK) && !c.dark_rate) return rip_fail(ctx, RIP_EINVAL, "calibrate: no dark_slope in caldir");
        host = in->location == RIP_HOST;
        d = *in;
        o = *out;
        return RIP_OK;
    }

    // host arrays: the inputs into workspace 2, the result planes into workspace 7 (a cube is read back from the workspace
    // the chain writes it to)
    int stage_host() {
        if (!host) return RIP_OK;
        char *w = (char *)rip_ws(ctx, RIP_WS_STAGING, rip_host_ramp_bytes(*in, ny, nx));
        if (!w) return RIP_ENOMEM;
        // (a ramp stored with its reference read subtracted: decoded behind the upload, counting word 0; read_back looks at it)
        decoded = rip_ramp_is_encoded(*in);
        if (decoded)
            if (const int rc = rip_refread_words(ctx, 1)) return rc;
        if (const int rc = rip_upload_host_ramp(ctx, *in, ny, nx, w, ctx->stream, &d, decoded ? ctx->refread_dev : nullptr)) return rc;
        RIP_HIP(ctx, hipGetLastError());
        w = (char *)rip_ws(ctx, RIP_WS_RESULTS, rip_result_bytes(G, npix, out->groupdq != nullptr));
        if (!w) return RIP_ENOMEM;
        o = rip_result_planes(w, *out, npix);
        return RIP_OK;
    }

    // ---- reference-pixel tables and the saturation pass, then the chain's first mark on the main stream.  With device-resident
    // inputs the pre-pass runs on a second stream so that it overlaps the previous ramp's main kernel; the tables are
    // double-buffered by call parity:
    //   stream2: wait(main kernels of call n-2 done) -> gate -> pre-pass -> ev_tab[p]
    //   stream : wait(ev_tab[p]) -> main kernels -> ev_done[p]
    // (the gate: prepass_gate below)
    int prepass() {
        // inputs guarded by a caller's event: the kernels on the main stream read them as well
        if (!host && in->ready_event) RIP_HIP(ctx, hipStreamWaitEvent(ctx->stream, (hipEvent_t)in->ready_event, 0));
        tab_bytes = ((size_t)2 * G * ny * 8 + (size_t)G * nch * 16 + 255) / 256 * 256;
        ws3 = (do_ref || (do_fit && (stages & RIP_STAGE_FLAT) && c.has_flat && d.area_factor))
                  ? (char *)rip_ws(ctx, RIP_WS_TABLES, 2 * tab_bytes + npix * 4 + 512)
                  : nullptr;
        par = ctx->parity;
        ctx->last_gate = 0;
        choose_skip();
        // (by situation: where the fused kernel fills the LDS the pre-pass of the next ramp finds no room beside it, runs when it
        // drains, and the single-launch form in front of the own ramp is the shorter way: 1.121 against 1.140 ms per ramp at f64
        // ipc4d x 8 groups, profiles/r04_summary.md)
        const bool lds_full = rip_chain_fills_lds(G, c.ipc_dtype) && ctx->use_fused && in->data_dtype == RIP_U16;
        overlap = do_ref && !host && ctx->can_overlap && ctx->overlap_mode != 0 && (ctx->overlap_mode == 1 || !lds_full);
        pre = overlap ? ctx->stream2 : ctx->stream;
        int rc;
        if (do_ref) {
            if ((rc = refpix_tables())) return rc;
        } else {
            mark(ctx, pre);
            if (do_sat && ((rc = pre_order()) || (rc = sat_pass()) || (rc = pre_done()))) return rc;
            mark(ctx, pre);
        }
        mark(ctx, ctx->stream);
        return RIP_OK;
    }

    // ---- The gate in front of an overlapped pre-pass (option "prepass_gate").  What releases pre-pass n on the second stream is
    // the end of the main kernels of call n-2, and that is the instant at which the fused kernel of call n-1 starts to dispatch:
    // the pre-pass's small workgroups then take pieces of CUs that the fused workgroups cannot use until they leave, and the fused
    // kernel ends as late as its last-started workgroup.  An event fires only at a kernel boundary, so the release comes from
    // inside the running kernel: every fused workgroup counts itself in (ChainArgs::wg_counter), and one wave on the second stream
    // waits until the count has reached the host's running total after the launch of call n-1.
    // The gate orders nothing that correctness needs (the event waits in front of it stay as they are), so its wait is bounded
    // and falling through is always correct.  Queued only where the PREVIOUS call on this context queued a fused launch with the
    // counter: not on the first call, not after a call that took the stage kernels, not inside rip_calibrate_batch (whose second
    // stream carries the uploads).
    // No cycle: fused n-1 waits only for ev_tab of pre-pass n-1 (and the main stream before it), which was recorded on the second
    // stream BEFORE gate n is queued; gate n waits for fused n-1 to have started; fused n waits for pre-pass n.  Should the
    // runtime map both streams onto one hardware queue, gate n sits in front of fused n-1 there, and the bound ends the wait: it
    // is there for that case.
    int prepass_gate() {
        if (!(overlap && pre != ctx->stream && ctx->prepass_gate > 0 && ctx->gate_words && ctx->gate_armed && !ctx->in_batch)) return RIP_OK;
        ctx->last_gate = 1;
        return rip_launch_prepass_gate(ctx, ctx->gate_words, ctx->gate_total, ctx->prepass_gate, pre);
    }

    int refpix_tables() {
        if (nx % RIP_CW) return rip_fail(ctx, RIP_EINVAL, "calibrate: nx=%d is not a multiple of 128", nx);
        if (!ws3) return RIP_ENOMEM;
        if (c.has_amp33 && !d.amp33) return rip_fail(ctx, RIP_EINVAL, "calibrate: the read file has amp33 but the ramp has none");
        rowcorr = (double *)(ws3 + (size_t)par * tab_bytes);
        rowcorr_t = rowcorr + (size_t)G * ny;
        lines = rowcorr_t + (size_t)G * ny;
        RefpixArgs ra{d.data, in->data_dtype, c.dark_data, c.has_amp33 ? d.amp33 : nullptr, c.amp33_med, c.refout_slope,
                      d.channel_lines, rowcorr, rowcorr_t, lines, ny, nx, G, overlap ? 1 : 0, pre};
        ra.g0 = skip0 ? 1 : 0;   // (both forms work group by group: the tables of a skipped group 0 are neither made nor read)
        if (overlap) {
            if (ctx->ev_done_valid[par]) RIP_HIP(ctx, hipStreamWaitEvent(ctx->stream2, ctx->ev_done[par], 0));
            // what the pre-pass stream waits for before it reads the inputs (rip_ramp_desc::inputs_ready / ready_event): the
            // caller's event, and -- unless the caller vouches for complete inputs -- everything queued on the main stream so far
            // (work of the caller's own, or of this library's device-pointer entry points: stream_dirty, which an event that
            // guards only some of the inputs does not cover)
            if (in->ready_event) RIP_HIP(ctx, hipStreamWaitEvent(ctx->stream2, (hipEvent_t)in->ready_event, 0));
            if ((!in->ready_event && in->inputs_ready != RIP_INPUTS_COMPLETE) || ctx->stream_dirty) {
                if (!ctx->ev_in) RIP_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_in, hipEventDisableTiming));
                RIP_HIP(ctx, hipEventRecord(ctx->ev_in, ctx->stream));
                RIP_HIP(ctx, hipStreamWaitEvent(ctx->stream2, ctx->ev_in, 0));
            }
        }
        int rc;
        if ((rc = prepass_gate())) return rc;
        mark(ctx, pre);
        if ((rc = pre_order()) || (rc = rip_launch_refpix_prepass(ctx, ra, rip_refpix_form(ctx->prepass_form, ra)))) return rc;
        if (do_sat && (rc = sat_pass())) return rc;  // same stream as the pre-pass: overlaps the previous ramp's main kernel
        if ((rc = pre_done())) return rc;
        mark(ctx, pre);
        if (overlap) {
            RIP_HIP(ctx, hipEventRecord(ctx->ev_tab[par], ctx->stream2));
            RIP_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_tab[par], 0));
        }
        return RIP_OK;
    }

    // dq-init + saturation flagging into workspace copies of the flag arrays (the caller's inputs stay untouched), double
    // buffered by call parity like the reference-pixel tables because the pass may run ahead on the second stream
    int sat_pass() {
        const size_t b_gdq = al256((size_t)G * npix), one = b_gdq + al256(npix * 4);
        char *w = (char *)rip_ws(ctx, RIP_WS_SATFLAG, 2 * one);
        if (!w) return RIP_ENOMEM;
        uint8_t *g2 = (uint8_t *)(w + (size_t)par * one);
        uint32_t *p2 = (uint32_t *)(w + (size_t)par * one + b_gdq);
        const int dnu_first = (plan && plan->h.start == 1) ? 1 : 0;  // the plan excludes the first group
        const int rc = rip_launch_satflag(ctx, d.data, in->data_dtype, c.sat_thr, c.sat_dq, d.groupdq, d.pixeldq, g2, p2, G, ny, nx,
                                          in->sat_backup, in->sat_skip_firstn, dnu_first, in->sat_dilution, pre);
        d.groupdq = g2;
        d.pixeldq = p2;
        return rc;
    }

    // pre-passes of consecutive calls share workspaces: one that runs on another stream than its predecessor waits for it
    int pre_order() {
        if (ctx->ev_pre_valid && ctx->pre_stream != pre) RIP_HIP(ctx, hipStreamWaitEvent(pre, ctx->ev_pre, 0));
        return RIP_OK;
    }
    int pre_done() {
        if (!ctx->ev_pre) RIP_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_pre, hipEventDisableTiming));
        RIP_HIP(ctx, hipEventRecord(ctx->ev_pre, pre));
        ctx->pre_stream = pre;
        ctx->ev_pre_valid = true;
        return RIP_OK;
    }

    // flat plane the slope is divided by: f32(flat_dn / AreaFactor)  (gen_cal_image.py:622)
    int flat_plane() {
        if (!(do_fit && (stages & RIP_STAGE_FLAT) && c.has_flat)) return RIP_OK;
        flat = c.flat_dn;
        if (d.area_factor) {
            if (!ws3) return RIP_ENOMEM;
            float *fl = (float *)(ws3 + 2 * tab_bytes);
            if (const int rc = rip_launch_flat_area(ctx, c.flat_dn, d.area_factor, fl, npix)) return rc;
            flat = fl;
        }
        return RIP_OK;
    }

    // ---- one kernel: refpix apply + bias + linearity + IPC + ramp fit + finish (chain.hip).  It covers the complete chain on a
    // Level-1 (u16) cube, with or without the bias step (no biascorr in the set, an all +0 one dropped at upload, a stage mask
    // without RIP_STAGE_BIAS: the launch then carries no bias stream, ChainArgs::bias_records); other sub-chains and f32 cubes
    // take the stage-by-stage kernels
    int fused_chain() {
        ctx->last_form = 0;
        ctx->last_first_group = 0;
        ctx->last_bias_stream = 0;
        memset(ctx->last_geo, 0, sizeof ctx->last_geo);
        ctx->gate_armed = false;   // (the launcher sets it: the next call's gate waits for a launch that carries the counter)
        if (!(ctx->use_fused && !c.has_inf && do_ref && do_lin && do_ipc && do_fit && in->data_dtype == RIP_U16 &&
              rip_chain_supported(ctx, c.lin_nplanes, G, c.ipc_dtype, c.gain_dtype))) {
            // (a call planned without group 0 must reach the fused kernel: the stage kernels would read unwritten tables)
            if (skip0) return rip_fail(ctx, RIP_ESTATE, "calibrate: a call planned without group 0 does not take the fused kernel");
            return RIP_OK;
        }
        ChainArgs ca;
        memset(&ca, 0, sizeof ca);
        ca.data = d.data;
        ca.data_u16 = in->data_dtype == RIP_U16;
        ca.gdq = d.groupdq;
        ca.pdq = d.pixeldq;
        ca.dark_data = c.dark_data;
        ca.rowcorr = rowcorr;
        ca.rowcorr_t = rowcorr_t;
        ca.lines = lines;
        if (do_bias) {
            ca.bias = c.bias + (size_t)(c.ngrp_bias - G) * npix;   // biascorr[de:], gen_cal_image.py:561-562
            ca.bias_records = -1;
        } else {
            // no bias stream: a descriptor of zero records (every load dropped) on a base that is valid all the same, with at
            // least G planes behind it (validate)
            ca.bias = c.dark_data;
            ca.bias_records = 0;
        }
        ca.planes = c.slab;
        ca.do_not_flag_first = plan->h.do_not_flag_first;
        ca.kern = c.ipc;
        ca.finish = (stages & (RIP_STAGE_DARK | RIP_STAGE_FLAT)) ? 1 : 0;
        if (stages & RIP_STAGE_DARK) {
            ca.dark_rate = 1;
            ca.dark_dq = c.has_dark_dq ? c.dark_dq : nullptr;
        }
        ca.flat = flat;
        ca.slope = o.slope;
        ca.err_read = o.err_read;
        ca.err_poisson = o.err_poisson;
        ca.pdq_out = o.pixeldq;
        ca.gdq_out = o.groupdq;
        float *cube = nullptr;
        if (out->cube) {
            cube = host ? (float *)rip_ws(ctx, RIP_WS_CUBE_B, (size_t)G * npix * 4) : out->cube;
            if (!cube) return RIP_ENOMEM;
            ca.cube_out = cube;
        }
        ca.ny = ny;
        ca.nx = nx;
        ca.nb = c.nb;
        ca.ngrp = G;
        ca.dense = plan->d_dense;
        // the flag word that holds what this call's finish step ORs into pixeldq (flat flags with the flat stage, dark dq with
        // the dark stage): -1 = not mergeable for this CALDIR set, the wave-specialised kernel is then not taken
        ca.merged_dq = c.merged_plane[((flat ? 1 : 0) | ((stages & RIP_STAGE_DARK) ? 2 : 0))];
        ca.dbg = ctx->chain_dbg;
        ca.dbg_buf = ctx->chain_dbg_buf;
        ca.wg_counter = ctx->prepass_gate > 0 ? ctx->gate_words : nullptr;
        const int rc = rip_launch_chain(ctx, plan, ca, c.lin_nplanes, c.ipc_dtype, skip0);
        // (choose_skip has asked the launcher's own questions: the stage kernels would find group 0's tables unwritten)
        if (rc == 1 && skip0) return rip_fail(ctx, RIP_ESTATE, "calibrate: the fused kernel declined a launch planned without group 0");
        // 1: no fused kernel for this plan / CALDIR set (flag words not mergeable, unusual difference mask): stage kernels
        if (rc == 1) return RIP_OK;
        if (rc) return rc;
        ran_fused = true;
        cur = cube;
        for (int i = 0; i < 3; ++i) mark(ctx, ctx->stream);
        return RIP_OK;
    }

    int stage_kernels() {
        int rc;
        pdq_mid = d.pixeldq;
        // ---- cube stage: refpix apply + bias + linearity (or a plain conversion to f32)
        if (do_ref || do_bias || do_lin || in->data_dtype != RIP_F32) {
            float *cubeA = (float *)rip_ws(ctx, RIP_WS_CUBE_A, (size_t)G * npix * 4 + npix * 4);
            if (!cubeA) return RIP_ENOMEM;
            uint32_t *pdq_ws = (uint32_t *)(cubeA + (size_t)G * npix);
            LinArgs la;
            memset(&la, 0, sizeof la);
            la.data = d.data;
            la.data_dtype = in->data_dtype;
            la.phi = cubeA;
            la.gdq = d.groupdq;
            la.gdq_is_attempt = 0;
            la.pdq_in = d.pixeldq;
            la.pdq_out = do_lin ? pdq_ws : nullptr;
            if (do_ref) {
                la.dark_data = c.dark_data;
                la.rowcorr = rowcorr;
                la.lines = lines;
            }
            if (do_bias) la.bias = c.bias + (size_t)(c.ngrp_bias - G) * npix;  // biascorr[de:], gen_cal_image.py:561-562
            if (do_lin) {
                la.coefs = c.lin_coefs;
                la.smin = c.lin_smin;
                la.smax = c.lin_smax;
                la.sref = c.lin_sref;
                la.lin_dq = c.lin_dq;
                la.nplanes = c.lin_nplanes;
                la.do_not_flag_first = plan->h.do_not_flag_first;
            }
            la.ny = ny;
            la.nx = nx;
            la.nb = c.nb;
            la.ngrp = G;
            if ((rc = rip_launch_lin(ctx, la))) return rc;
            cur = cubeA;
            if (do_lin) pdq_mid = pdq_ws;
        } else {
            cur = (const float *)d.data;
        }
        mark(ctx, ctx->stream);
        // ---- IPC
        if (do_ipc) {
            float *cubeB = (float *)rip_ws(ctx, RIP_WS_CUBE_B, (size_t)G * npix * 4);
            if (!cubeB) return RIP_ENOMEM;
            IpcArgs ia{cur, cubeB, c.ipc, c.gain, c.ipc_dtype, c.gain_dtype, ny, nx, c.nb, G};
            if ((rc = rip_launch_ipc_cube(ctx, ia))) return rc;
            cur = cubeB;
        }
        mark(ctx, ctx->stream);
        // ---- ramp fit + finish
        if (do_fit) {
            RampFitArgs fa;
            memset(&fa, 0, sizeof fa);
            fa.cube = cur;
            fa.gdq_in = d.groupdq;
            fa.gdq_out = o.groupdq;
            fa.pdq_in = pdq_mid;
            fa.pdq_out = o.pixeldq;
            fa.gain = c.gain;
            fa.read_noise = c.read_noise;
            fa.slope = o.slope;
            fa.err_read = o.err_read;
            fa.err_poisson = o.err_poisson;
            fa.finish = (stages & (RIP_STAGE_DARK | RIP_STAGE_FLAT)) ? 1 : 0;
            if (stages & RIP_STAGE_DARK) {
                fa.dark_rate = c.dark_rate;
                fa.dark_dq = c.has_dark_dq ? c.dark_dq : nullptr;
            }
            fa.flat = flat;
            fa.flat_flags = flat ? c.flat_flags : nullptr;
            fa.ny = ny;
            fa.nx = nx;
            fa.nb = c.nb;
            fa.ngrp = G;
            if ((rc = rip_launch_rampfit(ctx, plan, fa, c.gain_dtype))) return rc;
        }
        mark(ctx, ctx->stream);
        return RIP_OK;
    }

    // the main-stream kernels of this call are the last readers of the tables / flag copies of parity `par`: the
    // pre-pass of call n+2 (same parity, second stream) waits for this event before it overwrites them
    // EVERY call takes a parity and leaves its event, overlapped or not: a call whose pre-pass / flag pass ran on the main stream
    // has used the buffers of `par` too, and the next overlapped call must neither reuse them (it takes the other parity)
    // nor, two calls on, overwrite them before this call's main-stream kernels are done
    int parity_event() {
        ctx->stream_dirty = false;
        if (ctx->ev_done[par]) {
            RIP_HIP(ctx, hipEventRecord(ctx->ev_done[par], ctx->stream));
            ctx->ev_done_valid[par] = true;
        }
        ctx->parity ^= 1;
        return RIP_OK;
    }

    // ---- results back: host arrays from the device planes (waits for them); device outputs the chain did not write in place
    int read_back() {
        if (!host) {
            if (!do_fit && out->pixeldq && out->pixeldq != pdq_mid)
                RIP_HIP(ctx, hipMemcpyAsync(out->pixeldq, pdq_mid, npix * 4, hipMemcpyDeviceToDevice, ctx->stream));
            if (out->cube && out->cube != cur)
                RIP_HIP(ctx, hipMemcpyAsync(out->cube, cur, (size_t)G * npix * 4, hipMemcpyDeviceToDevice, ctx->stream));
            return RIP_OK;
        }
        if (do_fit) {
            if (const int rc = rip_download_results(ctx, o, *out, G, npix, ctx->stream)) return rc;
        } else if (out->pixeldq) {
            RIP_HIP(ctx, hipMemcpyAsync(out->pixeldq, pdq_mid, npix * 4, hipMemcpyDeviceToHost, ctx->stream));
        }
        if (out->cube) RIP_HIP(ctx, hipMemcpyAsync(out->cube, cur, (size_t)G * npix * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (decoded) RIP_HIP(ctx, hipMemcpyAsync(ctx->refread_host, ctx->refread_dev, 8, hipMemcpyDeviceToHost, ctx->stream));
        RIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (decoded && ctx->refread_host[0] != 0) {
            // the pieces do not belong together: what was computed from the clamped samples is not a result.  The word is cleared
            // so that the next call starts clean whatever it does.
            const unsigned long long bad = ctx->refread_host[0];
            ctx->refread_host[0] = 0;
            RIP_HIP(ctx, hipMemsetAsync(ctx->refread_dev, 0, 8, ctx->stream));
            return rip_fail(ctx, RIP_EINVAL, "calibrate: %llu samples of the decoded ramp lie outside 0..65535: reference_read, data and "
                            "data_encoding_offset %d do not belong together (the outputs are invalid)", bad, (int)in->data_encoding_offset);
        }
        return RIP_OK;
    }
};

}  // namespace

extern "C" {

int rip_calibrate(rip_ctx *ctx, int slot, int plan_id, unsigned stages, const rip_ramp_desc *in, const rip_outputs *out) {
    if (!in || !out) return rip_fail(ctx, RIP_EINVAL, "calibrate: NULL argument");
    if (slot < 0 || slot >= (int)ctx->cals.size() || !ctx->cals[slot].valid)
        return rip_fail(ctx, RIP_EINVAL, "calibrate: caldir slot %d is empty", slot);
    Calibration k{ctx, ctx->cals[slot], stages, in, out};
    int rc;
    if ((rc = k.validate(slot, plan_id)) || (rc = k.stage_host()) || (rc = k.prepass()) || (rc = k.flat_plane()) ||
        (rc = k.fused_chain()) || (!k.ran_fused && (rc = k.stage_kernels())) || (rc = k.parity_event()))
        return rc;
    return k.read_back();
}

}  // extern "C"
