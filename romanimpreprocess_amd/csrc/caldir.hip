// The device-resident CALDIR of one SCA (include/romanhip.h: rip_caldir_upload, rip_caldir_drop).  Host code only.
#include <cmath>

#include "rip_host.h"

namespace {

int dev_copy_in(rip_ctx *ctx, void **dst, const void *src, size_t bytes) {
    *dst = nullptr;
    if (!src) return RIP_OK;
    hipError_t e = hipMalloc(dst, bytes);
    if (e != hipSuccess) return rip_fail(ctx, RIP_ENOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    RIP_HIP(ctx, hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return RIP_OK;
}

// ---- The screen behind RipCal::first_group_safe.
// With an excluded first group the fit gives d[0] (group 0 after reference pixels, bias, linearity, IPC and the division by the
// gain) the weight +-0 and tests no difference on it: d[0] reaches the results only as 0 * d[0] and d[0] - d[1], i.e. only when
// it is not finite -- or so large that d[0] - d[1] overflows for a finite d[1] (|d[0]| < 2^103 rules that out: half an ulp of the
// largest f32).  The fused kernel may therefore leave group 0 out (chain2_form.h, "SKIPPED FIRST GROUP") wherever |d[0]| < 2^103
// is known WITHOUT computing it.  It is, for every u16 ramp, when the arrays of the set that reach group 0 pass these bounds:
//     V = 2^20 >= |dark.data|, |biascorr| (every plane: which one is "group 0" depends on the ramp), |Legendre planes|,
//                 |Smin|, |Smax|, |Sref|, |amp33.med|
//     2^-10 <= |gain| <= 2^10 (f32),   |ipc4d| <= 2^4,   |slope_ref| <= 2^10,   f32(Smax - Smin) != 0,   ny <= 2^16
// (the values of real and synthetic sets are below 2^17, gains near 1.5, IPC coefficients within [0, 1], the slope of order 1).
// The chain of bounds, each line one rounded operation of the kernels (rounding adds at most one part in 2^23: every bound below
// is rounded up generously), S a u16 sample < 2^16:
//   reference output   amp33 - med                          < 2^21   its medians (mean of two middle elements)      < 2^21
//                      minus the block's median, row medians < 2^22   minus their median ctr                         < 2^23
//   row correction     rc = slope_ref * (med - ctr), f64     < 2^33   (0 without a reference output)
//   v1 = S - dark      < 2^21                                         v2 = f32(f64(v1) - rc)                          < 2^34
//   channel line       medians b, t of v2 over the reference rows < 2^34;  m = (t - b) / (ny - 4), ny - 4 >= 12      < 2^32
//                      c = b - 1.5 m < 2^35;  iel = m * y + c, y < 2^16                                             < 2^49
//                      (a caller's line is checked per call against |m| <= 2^32, |c| <= 2^35: calibrate.hip)
//   v3 = f32(f64(v2) - iel) < 2^50    S' = v3 + dark - biascorr < 2^52    t = 2 (S' - Smin)                          < 2^54
//   z = t / span - 1   span is finite and non-zero, t finite: the quotient is finite or +-inf, never NaN (0/0 and non-finite
//                      operands are the only sources of NaN); through the shared reciprocal (taken when 1e-18 < |span| < 1e18)
//                      |t * (1/span)| < 2^114 and every fma of the correction steps stays finite.  Group 0 of a plan with
//                      do_not_flag_first is then CLIPPED to [-1, 1] (inf clips), so |z| <= 1 and no extrapolation branch
//   Legendre series    p_0 = 1, p_1 = z, p_{L+1} = (c1 z) p_L - c2 p_{L-1} with c1 < 2, c2 < 1: |p_{L+1}| < 2 |p_L| + |p_{L-1}|,
//                      so |p_L| < 3^L <= 3^10 < 2^16 for the at most 11 planes;  phi = sum of 11 terms cf_L p_L               < 2^40
//   flagged pixels     S' - Sref < 2^53 in place of phi
//   x = gain * phi (border pixels: phi)                      < 2^63
//   first iterate      f = sum of nine k x < 9 * 2^4 * 2^63 < 2^71;   O1 = 2 x - f                                    < 2^72
//   second iterate     f' = sum of nine k O1 < 2^80;                   O2 = (O1 + x) - f'                              < 2^81
//   d[0] = O2 / gain   |gain| >= 2^-10                                                                               < 2^91
// (f64 ipc4d: the iterates and the division are f64 with the same bounds, rounded to f32 at the end.)  So |d[0]| < 2^91: twelve
// binades below the 2^103 the argument needs, 36 below overflow.  A set that fails takes the full kernel form, call by call
// (RipCal::has_inf: one with an INFINITE value among these arrays takes the stage kernels).
// A set WITHOUT a bias correction -- no biascorr given, or one whose every word was +0 and that was dropped at upload
// (rip_caldir_upload) -- is screened like any other: the chain holds with biascorr = 0 (S' = v3 + dark < 2^51, and every later
// line only needs S' < 2^52), and so does a call whose stage mask leaves the bias step out.
constexpr double SCREEN_V = 1048576.0, SCREEN_GAIN = 1024.0, SCREEN_K = 16.0, SCREEN_SLOPE = 1024.0;

int screen_first_group(rip_ctx *ctx, RipCal &c, const rip_caldir_desc *d) {
    c.first_group_safe = c.has_inf = false;
    // what the fused chain needs anyway
    if (!c.dark_data || !c.lin_coefs || !c.has_ipc || c.gain_dtype != RIP_F32) return RIP_OK;
    const size_t npix = (size_t)c.ny * c.nx;
    DevBuf<uint32_t> bad(ctx);
    int rc;
    if ((rc = bad.alloc(1))) return rc;
    RIP_HIP(ctx, hipMemsetAsync(bad.p, 0, 4, ctx->stream));
    if ((rc = rip_launch_screen(ctx, c.dark_data, RIP_F32, npix * c.ngrp_dark, 0.0, SCREEN_V, bad.p)) ||
        (rc = rip_launch_screen(ctx, c.bias, RIP_F32, npix * c.ngrp_bias, 0.0, SCREEN_V, bad.p)) ||   // (none, or dropped: null, nothing to screen)
        // Legendre planes, Smin, Smax, Sref: planes [0, NP + 3) of the slab
        (rc = rip_launch_screen(ctx, c.slab, RIP_F32, npix * (size_t)(c.lin_nplanes + 3), 0.0, SCREEN_V, bad.p)) ||
        (rc = rip_launch_screen_span(ctx, c.lin_smin, c.lin_smax, npix, bad.p)) ||
        (rc = rip_launch_screen(ctx, c.gain, RIP_F32, npix, 1.0 / SCREEN_GAIN, SCREEN_GAIN, bad.p)) ||
        (rc = rip_launch_screen(ctx, c.ipc, c.ipc_dtype, 9 * npix, 0.0, SCREEN_K, bad.p)) ||
        (rc = rip_launch_screen(ctx, c.amp33_med, RIP_F32, (size_t)c.ny * RIP_CW, 0.0, SCREEN_V, bad.p)))
        return rc;
    uint32_t h_bad = 1;
    RIP_HIP(ctx, hipMemcpyAsync(&h_bad, bad.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    RIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const bool scalars_ok = c.ny <= 65536 && (!d->amp33_med || std::fabs(d->refout_slope) <= SCREEN_SLOPE);
    c.first_group_safe = h_bad == 0 && scalars_ok;
    c.has_inf = (h_bad & 2u) != 0 || (d->amp33_med && std::isinf(d->refout_slope));
    return RIP_OK;
}

}  // namespace

void free_cal(RipCal &c) {
    // everything else (linearity planes, gain if f32, read noise, dark rate, flat planes) lives in the slab
    void *ptrs[] = {c.dark_data, c.dark_slope, c.dark_dq, c.amp33_med, c.ipc, c.bias, c.slab, c.sat_thr, c.sat_dq,
                    c.gain_dtype == RIP_F64 ? c.gain : nullptr};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    c = RipCal();
}

extern "C" {

int rip_caldir_drop(rip_ctx *ctx, int slot) {
    if (slot < 0 || slot >= (int)ctx->cals.size() || !ctx->cals[slot].valid)
        return rip_fail(ctx, RIP_EINVAL, "caldir slot %d is empty", slot);
    RIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    free_cal(ctx->cals[slot]);
    return RIP_OK;
}

int rip_caldir_upload(rip_ctx *ctx, int slot, const rip_caldir_desc *d) {
    if (!d || slot < 0 || slot > 255) return rip_fail(ctx, RIP_EINVAL, "caldir upload: bad arguments");
    if (d->ny < 16 || d->nx < 16 || d->nborder < 0 || 2 * d->nborder + 3 > d->ny || 2 * d->nborder + 3 > d->nx)
        return rip_fail(ctx, RIP_EINVAL, "caldir upload: bad geometry %dx%d border %d", d->ny, d->nx, d->nborder);
    if (!d->gain || !d->read_noise) return rip_fail(ctx, RIP_EINVAL, "caldir upload: gain and read noise are required");
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    if ((int)ctx->cals.size() <= slot) ctx->cals.resize(slot + 1);
    if (ctx->cals[slot].valid) {
        RIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        free_cal(ctx->cals[slot]);
    }
    RipCal c;
    struct Guard {   // frees the partial set on every exit but the last
        RipCal &c;
        bool done = false;
        ~Guard() {
            if (!done) free_cal(c);
        }
    } guard{c};
    c.ny = d->ny;
    c.nx = d->nx;
    c.nb = d->nborder;
    const size_t npix = (size_t)c.ny * c.nx;
    const int nya = c.ny - 2 * c.nb, nxa = c.nx - 2 * c.nb;
    c.gain_dtype = d->gain_dtype;
    c.ipc_dtype = d->ipc_dtype;
    c.refout_slope = d->refout_slope;
    int rc;
#define UP(dst, src, bytes) \
    if ((rc = dev_copy_in(ctx, (void **)&(dst), (src), (bytes)))) return rc
    if (d->lin_coefs && (!d->lin_smin || !d->lin_smax || !d->lin_sref || !d->lin_dq || d->lin_nplanes < 1))
        return rip_fail(ctx, RIP_EINVAL, "caldir upload: incomplete linearity arrays");
    const int NPl = d->lin_coefs ? d->lin_nplanes : 0;
    if (hipMalloc((void **)&c.slab, (size_t)(NPl + 12) * npix * 4) != hipSuccess)
        return rip_fail(ctx, RIP_ENOMEM, "caldir upload: %zu bytes for the per-pixel planes", (size_t)(NPl + 12) * npix * 4);
    RIP_HIP(ctx, hipMemsetAsync(c.slab, 0, (size_t)(NPl + 12) * npix * 4, ctx->stream));
    float *pl = c.slab;
    auto plane = [&](int k) { return pl + (size_t)(NPl + k) * npix; };
#define UPS(dst, src, bytes)                                                                                        \
    do {                                                                                                            \
        hipError_t e_ = (src) ? hipMemcpyAsync((void *)(dst), (src), (bytes), hipMemcpyHostToDevice, ctx->stream) : hipSuccess; \
        if (e_ != hipSuccess) return rip_fail(ctx, RIP_EHIP, "caldir upload: %s", hipGetErrorString(e_));          \
    } while (0)
    if (d->dark_data) {
        c.ngrp_dark = d->ngrp_dark;
        UP(c.dark_data, d->dark_data, npix * 4 * (size_t)d->ngrp_dark);
    }
    UP(c.dark_slope, d->dark_slope, npix * 4);
    UP(c.dark_dq, d->dark_dq, npix * 4);
    UP(c.sat_thr, d->saturation, npix * 4);
    UP(c.sat_dq, d->saturation_dq, npix * 4);
    c.read_noise = plane(5);
    UPS(c.read_noise, d->read_noise, npix * 4);
    UP(c.amp33_med, d->amp33_med, (size_t)c.ny * RIP_CW * 4);
    c.has_amp33 = d->amp33_med != nullptr;
    if (d->gain_dtype == RIP_F64) {
        UP(c.gain, d->gain, npix * 8);
    } else {
        c.gain = plane(4);
        UPS(c.gain, d->gain, npix * 4);
    }
    if (d->lin_coefs) {
        c.lin_nplanes = d->lin_nplanes;
        c.lin_coefs = pl;
        c.lin_smin = plane(0);
        c.lin_smax = plane(1);
        c.lin_sref = plane(2);
        c.lin_dq = (uint32_t *)plane(3);
        UPS(c.lin_coefs, d->lin_coefs, npix * 4 * (size_t)d->lin_nplanes);
        UPS(c.lin_smin, d->lin_smin, npix * 4);
        UPS(c.lin_smax, d->lin_smax, npix * 4);
        UPS(c.lin_sref, d->lin_sref, npix * 4);
        UPS(c.lin_dq, d->lin_dq, npix * 4);
    }
    // dark dq: only kept if any bit is set (every dark file the reference writes has dq == 0)
    if (d->dark_dq) {
        bool any = false;
        for (size_t i = 0; i < npix && !any; ++i) any = d->dark_dq[i] != 0;
        c.has_dark_dq = any;
    }
    // ipc4d (3,3,nya,nxa) -> (9,ny,nx), biascorr (g,nya,nxa) -> (g,ny,nx): zero border, aligned rows
    if (d->ipc4d) {
        const size_t es = dsize(d->ipc_dtype);
        void *tmp = rip_ws(ctx, RIP_WS_STAGING, (size_t)9 * nya * nxa * es);
        hipError_t e = tmp ? hipMalloc(&c.ipc, 9 * npix * es) : hipErrorOutOfMemory;
        if (e != hipSuccess) return rip_fail(ctx, RIP_ENOMEM, "caldir upload: ipc4d allocation failed");
        RIP_HIP(ctx, hipMemcpyAsync(tmp, d->ipc4d, (size_t)9 * nya * nxa * es, hipMemcpyHostToDevice, ctx->stream));
        if ((rc = rip_launch_embed(ctx, tmp, c.ipc, 9, c.ny, c.nx, c.nb, (int)es))) return rc;
        c.has_ipc = true;
    }
    if (d->biascorr) {
        c.ngrp_bias = d->ngrp_bias;
        const size_t nb_in = (size_t)d->ngrp_bias * nya * nxa * 4;
        void *tmp = rip_ws(ctx, RIP_WS_STAGING, nb_in);
        hipError_t e = tmp ? hipMalloc((void **)&c.bias, (size_t)d->ngrp_bias * npix * 4) : hipErrorOutOfMemory;
        if (e != hipSuccess) return rip_fail(ctx, RIP_ENOMEM, "caldir upload: biascorr allocation failed");
        RIP_HIP(ctx, hipStreamSynchronize(ctx->stream));  // tmp may still feed the ipc embed
        RIP_HIP(ctx, hipMemcpyAsync(tmp, d->biascorr, nb_in, hipMemcpyHostToDevice, ctx->stream));
        if ((rc = rip_launch_embed(ctx, tmp, c.bias, d->ngrp_bias, c.ny, c.nx, c.nb, 4))) return rc;
        c.has_bias = true;
        // A bias correction of +0 everywhere corrects nothing: S - (+0.0f) is S for every f32 (-0, infinities, NaN included).  The
        // test is on BITS and over EVERY plane (which planes a ramp uses depends on its group count): a single -0.0 keeps the
        // array, because S - (-0.0f) turns an S of -0 into +0.  Such a set keeps no device copy (RipCal::bias_dropped) and its
        // calls run without the bias stream, like those of a set that never had a biascorr.
        DevBuf<uint32_t> nz(ctx);
        if ((rc = nz.alloc(1))) return rc;
        uint32_t h_nz = 1;
        RIP_HIP(ctx, hipMemsetAsync(nz.p, 0, 4, ctx->stream));
        if ((rc = rip_launch_screen_zero_words(ctx, (const uint32_t *)c.bias, (size_t)d->ngrp_bias * npix, nz.p))) return rc;
        RIP_HIP(ctx, hipMemcpyAsync(&h_nz, nz.p, 4, hipMemcpyDeviceToHost, ctx->stream));
        RIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (h_nz == 0) {
            (void)hipFree(c.bias);
            c.bias = nullptr;
            c.has_bias = false;
            c.bias_dropped = true;
        }
    }
    // IPC-deconvolved dark rate (gen_cal_image.py:217-221)
    if (c.dark_slope) {
        c.dark_rate = plane(6);
        if (c.has_ipc) {
            IpcArgs ia{c.dark_slope, c.dark_rate, c.ipc, c.gain, c.ipc_dtype, c.gain_dtype, c.ny, c.nx, c.nb, 1};
            if ((rc = rip_launch_ipc_cube(ctx, ia))) return rc;
        } else {
            RIP_HIP(ctx, hipMemcpyAsync(c.dark_rate, c.dark_slope, npix * 4, hipMemcpyDeviceToDevice, ctx->stream));
        }
    }
    // flat in DN units (flatutils.get_flat with pdq given) + the flags it would OR into pdq
    if (d->flat) {
        DevBuf<float> raw(ctx), padded(ctx);
        DevBuf<> gclip(ctx);
        if ((rc = raw.upload(d->flat, npix)) || (rc = padded.alloc(npix)) || (rc = gclip.alloc(npix * dsize(c.gain_dtype)))) return rc;
        c.flat_dn = plane(7);
        c.flat_flags = (uint32_t *)plane(8);
        rc = rip_launch_flat_prepare(ctx, raw.p, c.gain, c.gain_dtype, c.ny, c.nx, c.nb, padded.p, gclip.p, c.flat_flags,
                                     c.has_ipc ? 1 : 0);
        if (!rc) {
            if (c.has_ipc) {
                IpcArgs ia{padded.p, c.flat_dn, c.ipc, gclip.p, c.ipc_dtype, c.gain_dtype, c.ny, c.nx, c.nb, 1};
                rc = rip_launch_ipc_cube(ctx, ia);
            } else {
                hipError_t e = hipMemcpyAsync(c.flat_dn, padded.p, npix * 4, hipMemcpyDeviceToDevice, ctx->stream);
                if (e != hipSuccess) rc = rip_fail(ctx, RIP_EHIP, "flat copy: %s", hipGetErrorString(e));
            }
        }
        hipError_t e = hipStreamSynchronize(ctx->stream);
        if (!rc && e != hipSuccess) rc = rip_fail(ctx, RIP_EHIP, "caldir upload: %s", hipGetErrorString(e));
        if (rc) return rc;
        c.has_flat = true;
    }
    // the flag words of the wave-specialised fused kernel: linearity dq merged with the flat flags and / or the dark dq
    if (c.lin_dq) {
        DevBuf<uint32_t> clash(ctx);
        if ((rc = clash.alloc(4))) return rc;
        uint32_t h_clash[3] = {0, 0, 0};
        RIP_HIP(ctx, hipMemsetAsync(clash.p, 0, 16, ctx->stream));
        for (int combo = 1; combo < 4 && !rc; ++combo) {
            const bool ff = (combo & 1) && c.has_flat, dd = (combo & 2) && c.has_dark_dq;
            if (((combo & 1) && !c.has_flat) || ((combo & 2) && !c.has_dark_dq)) continue;   // nothing to add: see below
            rc = rip_launch_merge_dq(ctx, c.lin_dq, ff ? c.flat_flags : nullptr, dd ? c.dark_dq : nullptr, (uint32_t *)plane(8 + combo),
                                     c.ny, c.nx, c.nb, clash.p + (combo - 1));
        }
        if (!rc) {
            hipError_t em = hipMemcpyAsync(h_clash, clash.p, 12, hipMemcpyDeviceToHost, ctx->stream);
            if (em == hipSuccess) em = hipStreamSynchronize(ctx->stream);
            if (em != hipSuccess) rc = rip_fail(ctx, RIP_EHIP, "caldir upload: %s", hipGetErrorString(em));
        }
        if (rc) return rc;
        for (int combo = 1; combo < 4; ++combo) {
            const int eff = (c.has_flat ? (combo & 1) : 0) | (c.has_dark_dq ? (combo & 2) : 0);   // what this set can add at all
            c.merged_plane[combo] = eff == 0 ? 3 : (h_clash[eff - 1] ? -1 : 8 + eff);
        }
    }
#undef UP
#undef UPS
    if ((rc = screen_first_group(ctx, c, d))) return rc;
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return rip_fail(ctx, RIP_EHIP, "caldir upload: %s", hipGetErrorString(e));
    c.valid = true;
    ctx->cals[slot] = c;
    guard.done = true;
    return RIP_OK;
}

}  // extern "C"
