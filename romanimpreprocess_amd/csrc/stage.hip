// Stage-level entry points (include/romanhip.h: function-level drop-ins and parity tests): each copies the caller's HOST arrays
// into scoped device buffers, launches the stage's kernels, queues the copies back and waits once.  Host code only.
#include <string.h>

#include "rip_host.h"

extern "C" {

int rip_stage_refpix_image(rip_ctx *ctx, float *image, int ny, int nx, double slope, int do_row, int do_channel,
                           const double *lines, float *ref_med, float *ctr, float *bottom_top) {
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    if (nx % RIP_CW) return rip_fail(ctx, RIP_EINVAL, "refpix: nx=%d is not a multiple of 128", nx);
    const int w = nx + RIP_CW, nch = w / RIP_CW;
    const size_t n = (size_t)ny * w;
    DevBuf<float> img(ctx), rm(ctx), ct(ctx), bt(ctx);
    DevBuf<double> ln(ctx);
    int rc;
    if ((rc = img.upload(image, n))) return rc;
    if (lines && (rc = ln.upload(lines, (size_t)nch * 2))) return rc;
    if ((rc = rm.alloc(ny)) || (rc = ct.alloc(1)) || (rc = bt.alloc((size_t)nch * 2))) return rc;
    // the row step on the reference output (nside = nx, f64 slope), then the channel step on the nch 128-column channels
    if (do_row && (rc = rip_refpix_row_general(ctx, img.p, ny, w, nx, 1, RIP_ROW_SLOPE_F64, slope, rm.p, nullptr, ct.p))) return rc;
    if (do_channel && (rc = rip_refpix_channel_general(ctx, img.p, ny, w, 0, RIP_CW, nch, lines ? ln.p : nullptr, bt.p))) return rc;
    if ((rc = img.download(image, n))) return rc;
    if (ref_med && do_row && (rc = rm.download(ref_med, ny))) return rc;
    if (ctr && do_row && (rc = ct.download(ctr, 1))) return rc;
    if (bottom_top && do_channel && (rc = bt.download(bottom_top, (size_t)nch * 2))) return rc;
    return dev_sync(ctx);
}

int rip_stage_refpix_row(rip_ctx *ctx, float *image, int ny, int width, int nside, int use_ref_channel, int mode, double slope,
                         float *ref_med, float *sci_med, float *ctr) {
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    if (!image || ny < 1 || width < 1) return rip_fail(ctx, RIP_EINVAL, "refpix row: image required");
    if (mode < RIP_ROW_MEDIANS_ONLY || mode > RIP_ROW_SLOPE_F32) return rip_fail(ctx, RIP_EINVAL, "refpix row: mode %d", mode);
    const size_t n = (size_t)ny * width;
    DevBuf<float> img(ctx), rm(ctx), sm(ctx), ct(ctx);
    int rc;
    if ((rc = img.upload(image, n)) || (rc = rm.alloc(ny)) || (rc = ct.alloc(1))) return rc;
    if (sci_med && (rc = sm.alloc(ny))) return rc;
    if ((rc = rip_refpix_row_general(ctx, img.p, ny, width, nside, use_ref_channel, mode, slope, rm.p, sci_med ? sm.p : nullptr, ct.p)))
        return rc;
    if (mode != RIP_ROW_MEDIANS_ONLY && (rc = img.download(image, n))) return rc;
    if (ref_med && (rc = rm.download(ref_med, ny))) return rc;
    if (sci_med && (rc = sm.download(sci_med, ny))) return rc;
    if (ctr && (rc = ct.download(ctr, 1))) return rc;
    return dev_sync(ctx);
}

int rip_stage_refpix_channel(rip_ctx *ctx, float *image, int ny, int width, int channel_start, int channel_end, int nchan,
                             const double *lines, float *bottom_top) {
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    if (!image || ny < 1 || width < 1 || nchan < 1) return rip_fail(ctx, RIP_EINVAL, "refpix channel: image required");
    const size_t n = (size_t)ny * width;
    DevBuf<float> img(ctx), bt(ctx);
    DevBuf<double> ln(ctx);
    int rc;
    if ((rc = img.upload(image, n))) return rc;
    if (lines && (rc = ln.upload(lines, (size_t)nchan * 2))) return rc;
    if ((rc = bt.alloc((size_t)nchan * 2))) return rc;
    if ((rc = rip_refpix_channel_general(ctx, img.p, ny, width, channel_start, channel_end, nchan, lines ? ln.p : nullptr, bt.p)))
        return rc;
    if ((rc = img.download(image, n))) return rc;
    if (bottom_top && (rc = bt.download(bottom_top, (size_t)nchan * 2))) return rc;
    return dev_sync(ctx);
}

int rip_stage_refpix_tables(rip_ctx *ctx, const void *data, int data_dtype, const float *dark, const uint16_t *amp33,
                            const float *amp33_med, double slope, int ngrp, int ny, int nx, int form, double *rowcorr,
                            double *lines, int *status) {
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    if (!data || !dark || !amp33 || !amp33_med || !rowcorr || !lines || ngrp < 1 || ngrp > RIP_MAX_GROUPS || ny < 8 || nx < RIP_CW ||
        nx % RIP_CW || (data_dtype != RIP_U16 && data_dtype != RIP_F32))
        return rip_fail(ctx, RIP_EINVAL, "refpix tables: bad argument");
    const size_t npix = (size_t)ny * nx, nch = (size_t)nx / RIP_CW;
    DevBuf<> d_data(ctx);
    DevBuf<float> d_dark(ctx), d_med(ctx);
    DevBuf<uint16_t> d_a33(ctx);
    DevBuf<double> d_rc(ctx), d_rt(ctx), d_ln(ctx);
    int rc;
    if ((rc = d_data.upload(data, (size_t)ngrp * npix * dsize(data_dtype))) || (rc = d_dark.upload(dark, (size_t)ngrp * npix)) ||
        (rc = d_a33.upload(amp33, (size_t)ngrp * ny * RIP_CW)) || (rc = d_med.upload(amp33_med, (size_t)ny * RIP_CW)) ||
        (rc = d_rc.alloc((size_t)ngrp * ny)) || (rc = d_rt.alloc((size_t)ngrp * ny)) || (rc = d_ln.alloc((size_t)ngrp * nch * 2)))
        return rc;
    RefpixArgs ra{d_data.p, data_dtype, d_dark.p, d_a33.p, d_med.p, slope, nullptr, d_rc.p, d_rt.p, d_ln.p, ny, nx, ngrp};
    if (form < -1 || form > 1) return rip_fail(ctx, RIP_EINVAL, "refpix tables: form %d", form);
    if (form == 1 && !rip_refpix_one_supported(ra))
        return rip_fail(ctx, RIP_EINVAL, "refpix tables: the single-launch kernel does not cover a %d x %d frame of %d groups", ny, nx, ngrp);
    if ((rc = rip_launch_refpix_prepass(ctx, ra, rip_refpix_form(form < 0 ? ctx->prepass_form : form, ra)))) return rc;
    if ((rc = d_rc.download(rowcorr, (size_t)ngrp * ny)) || (rc = d_ln.download(lines, (size_t)ngrp * nch * 2)) || (rc = dev_sync(ctx)))
        return rc;
    if (status) return rip_refpix_one_status(ctx, status);
    return RIP_OK;
}

int rip_stage_multilin(rip_ctx *ctx, const float *S, int ngrp, int ny, int nx, int nplanes, const float *coefs,
                       const float *smin, const float *smax, const float *sref, const uint32_t *lin_dq,
                       int do_not_flag_first, const uint8_t *attempt_corr, float *phi, uint32_t *dq) {
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)ny * nx;
    DevBuf<float> dS(ctx), dC(ctx), dmin(ctx), dmax(ctx), dref(ctx), dphi(ctx);
    DevBuf<uint32_t> ddq(ctx), dout(ctx);
    DevBuf<uint8_t> dac(ctx);
    int rc;
    if ((rc = dS.upload(S, (size_t)ngrp * npix)) || (rc = dC.upload(coefs, (size_t)nplanes * npix)) || (rc = dmin.upload(smin, npix)) ||
        (rc = dmax.upload(smax, npix)) || (rc = dref.upload(sref, npix)) || (rc = ddq.upload(lin_dq, npix)) ||
        (rc = dphi.alloc((size_t)ngrp * npix)) || (rc = dout.alloc(npix)))
        return rc;
    if (attempt_corr && (rc = dac.upload(attempt_corr, (size_t)ngrp * npix))) return rc;
    LinArgs la;
    memset(&la, 0, sizeof la);
    la.data = dS.p;
    la.data_dtype = RIP_F32;
    la.phi = dphi.p;
    la.gdq = attempt_corr ? dac.p : nullptr;
    la.gdq_is_attempt = 1;
    la.pdq_out = dout.p;
    la.coefs = dC.p;
    la.smin = dmin.p;
    la.smax = dmax.p;
    la.sref = dref.p;
    la.lin_dq = ddq.p;
    la.nplanes = nplanes;
    la.do_not_flag_first = do_not_flag_first;
    la.ny = ny;
    la.nx = nx;
    la.nb = 0;
    la.ngrp = ngrp;
    if ((rc = rip_launch_lin(ctx, la))) return rc;
    if ((rc = dphi.download(phi, (size_t)ngrp * npix)) || (rc = dout.download(dq, npix))) return rc;
    return dev_sync(ctx);
}

int rip_stage_ipc_image(rip_ctx *ctx, int reverse, int order, const void *image, int img_dtype, int ny, int nx,
                        const void *kernel, int k_dtype, const void *gain, int g_dtype, void *outp) {
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)ny * nx;
    const bool t64 = img_dtype == RIP_F64 || k_dtype == RIP_F64 || (gain && g_dtype == RIP_F64);
    DevBuf<> di(ctx), dk(ctx), dg(ctx), dout(ctx);   // bytes: the element types are the call's dtypes
    int rc;
    if ((rc = di.upload(image, npix * dsize(img_dtype))) || (rc = dk.upload(kernel, 9 * npix * dsize(k_dtype))) ||
        (rc = dout.alloc(npix * (t64 ? 8 : 4))))
        return rc;
    if (gain && (rc = dg.upload(gain, npix * dsize(g_dtype)))) return rc;
    if ((rc = rip_launch_ipc_image(ctx, reverse, order, di.p, img_dtype, ny, nx, dk.p, k_dtype, gain ? dg.p : nullptr, g_dtype, dout.p)))
        return rc;
    if ((rc = dout.download(outp, npix * (t64 ? 8 : 4)))) return rc;
    return dev_sync(ctx);
}

int rip_stage_correct_cube(rip_ctx *ctx, float *data, int ngrp, int ny, int nx, int nb, const void *kernel, int k_dtype,
                           const void *gain, int g_dtype) {
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)ny * nx;
    const int nya = ny - 2 * nb, nxa = nx - 2 * nb;
    const size_t es = dsize(k_dtype);
    DevBuf<float> din(ctx), dout(ctx);
    DevBuf<> kraw(ctx), kemb(ctx), dg(ctx);
    int rc;
    if ((rc = din.upload(data, (size_t)ngrp * npix)) || (rc = dout.alloc((size_t)ngrp * npix)) ||
        (rc = kraw.upload(kernel, (size_t)9 * nya * nxa * es)) || (rc = kemb.alloc(9 * npix * es)))
        return rc;
    if (gain && (rc = dg.upload(gain, npix * dsize(g_dtype)))) return rc;
    if ((rc = rip_launch_embed(ctx, kraw.p, kemb.p, 9, ny, nx, nb, (int)es))) return rc;
    IpcArgs ia{din.p, dout.p, kemb.p, gain ? dg.p : nullptr, k_dtype, g_dtype, ny, nx, nb, ngrp};
    if ((rc = rip_launch_ipc_cube(ctx, ia))) return rc;
    if ((rc = dout.download(data, (size_t)ngrp * npix))) return rc;
    return dev_sync(ctx);
}

int rip_stage_ramp_fit(rip_ctx *ctx, int plan_id, const float *data, uint8_t *rdq, uint32_t *pdq, int ny, int nx, int nb,
                       const void *gain, int g_dtype, const float *read_noise, float *slope, float *err_read,
                       float *err_poisson) {
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    RipPlan *plan = get_plan(ctx, plan_id);
    if (!plan) return RIP_EINVAL;
    const int G = plan->h.ngrp;
    const size_t npix = (size_t)ny * nx;
    DevBuf<float> dd(ctx), dn(ctx), ds(ctx), de(ctx), dq2(ctx);
    DevBuf<uint8_t> dr(ctx), dr2(ctx);
    DevBuf<uint32_t> dp(ctx), dp2(ctx);
    DevBuf<> dg(ctx);
    int rc;
    if ((rc = dd.upload(data, (size_t)G * npix)) || (rc = dr.upload(rdq, (size_t)G * npix)) || (rc = dp.upload(pdq, npix)) ||
        (rc = dg.upload(gain, npix * dsize(g_dtype))) || (rc = dn.upload(read_noise, npix)) || (rc = ds.alloc(npix)) ||
        (rc = de.alloc(npix)) || (rc = dq2.alloc(npix)) || (rc = dr2.alloc((size_t)G * npix)) || (rc = dp2.alloc(npix)))
        return rc;
    RampFitArgs fa;
    memset(&fa, 0, sizeof fa);
    fa.cube = dd.p;
    fa.gdq_in = dr.p;
    fa.gdq_out = dr2.p;
    fa.pdq_in = dp.p;
    fa.pdq_out = dp2.p;
    fa.gain = dg.p;
    fa.read_noise = dn.p;
    fa.slope = ds.p;
    fa.err_read = de.p;
    fa.err_poisson = dq2.p;
    fa.finish = 0;
    fa.ny = ny;
    fa.nx = nx;
    fa.nb = nb;
    fa.ngrp = G;
    if ((rc = rip_launch_rampfit(ctx, plan, fa, g_dtype))) return rc;
    if ((rc = ds.download(slope, npix)) || (rc = de.download(err_read, npix)) || (rc = dq2.download(err_poisson, npix)) ||
        (rc = dr2.download(rdq, (size_t)G * npix)) || (rc = dp2.download(pdq, npix)))
        return rc;
    return dev_sync(ctx);
}

int rip_stage_jump_detect(rip_ctx *ctx, int plan_id, const float *data, uint8_t *rdq, int ny, int nx, int nb, const void *gain,
                          int g_dtype, const float *read_noise, float *slope, float *err_read, float *err_poisson, float *smap) {
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    RipPlan *plan = get_plan(ctx, plan_id);
    if (!plan) return RIP_EINVAL;
    if (!data || !rdq || !gain || !read_noise || !slope || !err_read || !err_poisson || !smap)
        return rip_fail(ctx, RIP_EINVAL, "jump_detect: NULL array");
    const int G = plan->h.ngrp, nd = plan->variants[0].ndiff;
    if (G < 2 || nd <= 0) return rip_fail(ctx, RIP_EINVAL, "jump_detect: a plan of %d groups has no difference to test", G);
    const size_t npix = (size_t)ny * nx;
    DevBuf<float> dd(ctx), dn(ctx), ds(ctx), de(ctx), dp(ctx), dm(ctx);
    DevBuf<uint8_t> dr(ctx);
    DevBuf<> dg(ctx);
    int rc;
    if ((rc = dd.upload(data, (size_t)G * npix)) || (rc = dr.upload(rdq, (size_t)G * npix)) ||
        (rc = dg.upload(gain, npix * dsize(g_dtype))) || (rc = dn.upload(read_noise, npix)) || (rc = ds.alloc(npix)) ||
        (rc = de.alloc(npix)) || (rc = dp.alloc(npix)) || (rc = dm.alloc((size_t)nd * npix)))
        return rc;
    if ((rc = rip_launch_jumpdetect(ctx, plan, dd.p, dr.p, dg.p, g_dtype, dn.p, ds.p, de.p, dp.p, dm.p, ny, nx, nb))) return rc;
    if ((rc = ds.download(slope, npix)) || (rc = de.download(err_read, npix)) || (rc = dp.download(err_poisson, npix)) ||
        (rc = dr.download(rdq, (size_t)G * npix)) || (rc = dm.download(smap, (size_t)nd * npix)))
        return rc;
    return dev_sync(ctx);
}

int rip_stage_get_flat(rip_ctx *ctx, const float *flat, int ny, int nx, int nb, const void *gain, int g_dtype,
                       const void *kernel, int k_dtype, int ipc_deconvolve, uint32_t *pdq, float *outp) {
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)ny * nx;
    const int nya = ny - 2 * nb, nxa = nx - 2 * nb;
    const size_t es = dsize(k_dtype);
    DevBuf<float> raw(ctx), padded(ctx), dout(ctx);
    DevBuf<uint32_t> flags(ctx);
    DevBuf<> dg(ctx), gclip(ctx), kraw(ctx), kemb(ctx);
    int rc;
    if ((rc = raw.upload(flat, npix)) || (rc = padded.alloc(npix)) || (rc = flags.alloc(npix)) || (rc = dout.alloc(npix))) return rc;
    int with_gain = 0;
    if (ipc_deconvolve) {
        if (!gain || !kernel) return rip_fail(ctx, RIP_EINVAL, "get_flat: gain and ipc4d needed for deconvolution");
        with_gain = pdq ? 1 : 2;
        if ((rc = dg.upload(gain, npix * dsize(g_dtype))) || (rc = gclip.alloc(npix * dsize(g_dtype))) ||
            (rc = kraw.upload(kernel, (size_t)9 * nya * nxa * es)) || (rc = kemb.alloc(9 * npix * es)))
            return rc;
        if ((rc = rip_launch_embed(ctx, kraw.p, kemb.p, 9, ny, nx, nb, (int)es))) return rc;
    }
    if ((rc = rip_launch_flat_prepare(ctx, raw.p, dg.p, g_dtype, ny, nx, nb, padded.p, gclip.p, flags.p, with_gain))) return rc;
    const DevBuf<float> *res = &padded;
    if (ipc_deconvolve) {
        IpcArgs ia{padded.p, dout.p, kemb.p, gclip.p, k_dtype, g_dtype, ny, nx, nb, 1};
        if ((rc = rip_launch_ipc_cube(ctx, ia))) return rc;
        res = &dout;
    }
    if ((rc = res->download(outp, npix))) return rc;
    if (!pdq) return dev_sync(ctx);
    std::vector<uint32_t> fl(npix);
    if ((rc = flags.download(fl.data(), npix)) || (rc = dev_sync(ctx))) return rc;
    for (size_t i = 0; i < npix; ++i) pdq[i] |= fl[i];
    return RIP_OK;
}

}  // extern "C"
