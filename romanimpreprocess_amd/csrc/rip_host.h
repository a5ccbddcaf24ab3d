// Host-only helpers of libromanhip, defined once: the scoped device buffer of the stage-level entry points and the
// declarations the host translation units share.  Included by host code in .hip files only -- never by rip_common.h or by a
// header that holds device code.
//
// Pointer kinds of the ARRAY arguments of the stage-level entry points (include/romanhip.h says the same at each):
//   host arrays OR device pointers   rip_stage_noise_inject (in-place calls, out == cube, included), rip_stage_poisson_resample,
//                                    rip_stage_pearson, and the post-path entries of post.hip (rip_stage_build_mask, _endslice,
//                                    _bin_mean, _select_ranks, _gauss_hist, _legendre2d; rip_stage_pixel_area by out_location),
//                                    and the calibration-file entries of calfiles.hip (rip_cal_biascorr, _pflat, _saturation,
//                                    _mask).  The noise-layer driver (L1_to_L2/gen_noise_image.py) hands them planes that live in HBM.
//   host arrays OR device pointers,  the dark-file entries of darkstack.hip (rip_cal_group_means, _sigma_clip_mean, _dark_planes):
//   told by a `location` argument    RIP_DEVICE arrays are used where they are -- the stack of group means is too large to copy;
//                                    the OUTPUTS of rip_cal_gain_ipc4d (gainfile.hip), whose inputs are small host tables;
//                                    rip_stage_fits_encode (fitsout.hip): one location for src and mask, another for dst;
//                                    rip_stage_l2_planes, rip_stage_l2_refpix_strips (l2out.hip): one location for every pointer;
//                                    rip_cal_raw_frame (rawframes.hip): the frame by its location, the cube plane always in HBM;
//                                    rip_cal_frame_slopes: the cube always in HBM, the slopes by out_location;
//                                    rip_fpa_bin (fpaplot.hip): dq, every plane and out each by a location of its own;
//                                    rip_fpa_render: the maps and the picture by theirs, its small tables host arrays
//                                    rip_cal_frame_sums (linfit.hip): the cube by its location, the sums always in HBM
//   device pointers                  rip_cal_linearity_fit: the sums of every set, Sref and all result planes (its tables are host arrays)
//   host arrays                      the wrappers of stage.hip, rip_stage_invlinearity, rip_stage_noise_1f
// Small tables (nreads, group tables, weights, ranks, counts) are host arrays everywhere.
// DevBuf copies with hipMemcpyDefault in both directions: under unified addressing that IS the host-to-device (device-to-host)
// copy for a host array, so the one helper serves both rows.  A copy direction "tidied" to an explicit kind breaks the first.
#pragma once

#include "rip_common.h"

#define RIP_SHARED __attribute__((visibility("hidden")))   // shared between translation units, not part of the interface

inline size_t dsize(int dtype) { return dtype == RIP_F64 ? 8 : ((dtype == RIP_U16 || dtype == RIP_F16) ? 2 : 4); }
inline size_t al256(size_t x) { return (x + 255) / 256 * 256; }

// Scoped device allocation of n elements of T for one call of an entry point (`who`: its name, for the error text).
// upload / download queue their copies on `stream` (null: the context's main stream) and do not wait: an entry point that
// reads back several arrays pays one dev_sync at its end.
template <typename T = char>
struct DevBuf {
    rip_ctx *ctx;
    const char *who;
    T *p = nullptr;
    explicit DevBuf(rip_ctx *c, const char *who_ = __builtin_FUNCTION()) : ctx(c), who(who_) {}
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    int alloc(size_t n) {   // n = 0 yields a valid buffer too
        const size_t bytes = n * sizeof(T);
        const hipError_t e = hipMalloc((void **)&p, bytes ? bytes : 1);
        if (e != hipSuccess) return rip_fail(ctx, RIP_ENOMEM, "%s: hipMalloc(%zu bytes): %s", who, bytes, hipGetErrorString(e));
        return RIP_OK;
    }
    int copy_in(const void *src, size_t n, hipStream_t stream = nullptr) {   // into the buffer as it stands
        RIP_HIP(ctx, hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyDefault, stream ? stream : ctx->stream));
        return RIP_OK;
    }
    int upload(const void *src, size_t n, hipStream_t stream = nullptr) {
        if (const int rc = alloc(n)) return rc;
        return copy_in(src, n, stream);
    }
    int download(void *dst, size_t n, hipStream_t stream = nullptr) const {
        RIP_HIP(ctx, hipMemcpyAsync(dst, p, n * sizeof(T), hipMemcpyDefault, stream ? stream : ctx->stream));
        return RIP_OK;
    }
};

// waits for what an entry point has queued (its downloads among it)
inline int dev_sync(rip_ctx *ctx, hipStream_t stream = nullptr) {
    RIP_HIP(ctx, hipStreamSynchronize(stream ? stream : ctx->stream));
    return RIP_OK;
}

// before a launch with `lds` bytes of dynamic LDS: above the 48 KB a kernel may take by default, its limit has to be raised
template <typename K>
inline int with_lds(rip_ctx *ctx, K kernel, size_t lds) {
    if (lds > 48 * 1024)
        RIP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return RIP_OK;
}

// caldir.hip
RIP_SHARED void free_cal(RipCal &c);
// plan.hip
struct PlanFree {   // a plan and its device image
    void operator()(RipPlan *p) const {
        if (p->dev) (void)hipFree(p->dev);
        delete p;
    }
};
RIP_SHARED RipPlan *get_plan(rip_ctx *ctx, int id);   // nullptr (error recorded) where the plan does not exist

// calibrate.hip: a ramp in HOST memory is staged into device buffers, its results laid out there and copied back, by
// rip_calibrate and by rip_calibrate_batch (batch.hip)
RIP_SHARED size_t rip_host_ramp_bytes(const rip_ramp_desc &in, int ny, int nx);
// (count: the device word that receives the out-of-range samples of a ramp stored with its reference read subtracted, zeroed and
// added to on `st`; not looked at for a ramp without reference planes)
RIP_SHARED int rip_upload_host_ramp(rip_ctx *ctx, const rip_ramp_desc &in, int ny, int nx, char *w, hipStream_t st, rip_ramp_desc *dev,
                                    unsigned long long *count = nullptr);
// the refusals of rip_ramp_desc::reference_read / reference_amp33 (`who`: the entry's name, for the error text)
RIP_SHARED int rip_check_reference_read(rip_ctx *ctx, const rip_ramp_desc &in, const char *who);
inline bool rip_ramp_is_encoded(const rip_ramp_desc &in) { return in.reference_read || in.reference_amp33; }
RIP_SHARED size_t rip_result_bytes(int G, size_t npix, bool groupdq);
RIP_SHARED rip_outputs rip_result_planes(char *w, const rip_outputs &host, size_t npix);
RIP_SHARED int rip_download_results(rip_ctx *ctx, const rip_outputs &dev, const rip_outputs &host, int G, size_t npix, hipStream_t st);
