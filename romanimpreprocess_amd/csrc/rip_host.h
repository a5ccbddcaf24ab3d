// Host-only helpers of libromanhip, defined once: the scoped device buffer of the stage-level entry points and the
// declarations the host translation units share.  Included by host code in .hip files only -- never by rip_common.h or by a
// header that holds device code.
//
// Pointer kinds of the ARRAY arguments of the stage-level entry points (include/romanhip.h says the same at each).
// THE RULE: an entry that takes a `location` (RIP_HOST or RIP_DEVICE) for an array declares that array as a DevArg below: a
// RIP_DEVICE pointer is used where it is, a RIP_HOST array goes through a scoped device buffer, a NULL optional array stays NULL,
// and the end of the entry reads the same for every location.  Which arrays a location covers is said by the entry's in() / out()
// lines; whether it waits before it returns, by its last line.  Under the rule:
// rip_cal_group_means, _sigma_clip_mean, _dark_planes, rip_cal_gain_ipc4d, rip_cal_raw_frame, rip_cal_frame_slopes,
// rip_cal_frame_sums, rip_stage_l2_planes, rip_stage_l2_refpix_strips, rip_fpa_bin, rip_fpa_render, rip_stage_fits_encode,
// rip_stage_decode_reference_read, rip_stage_pixel_area, rip_cal_noise_add, rip_cal_noise_planes, rip_view_ranks,
// rip_view_plane_diff, rip_view_render, rip_cal_corr_pair.  The exceptions:
//   partial copies                   the raw-sample cubes of rip_cal_group_means, rip_cal_frame_sums, rip_cal_noise_add and
//                                    rip_cal_corr_pair are CubeBands below: of a host cube only the frames and rows that are
//                                    read travel (corr_pair: one band per frame, into one buffer per cube).
//                                    rip_view_plane_diff copies only its two planes; rip_stage_fits_encode and
//                                    rip_stage_decode_reference_read turn a host source into the result in place, in the
//                                    output's buffer
//   always device pointers           the cube plane of rip_cal_raw_frame, the cube of rip_cal_frame_slopes, the sums of
//                                    rip_cal_frame_sums, every plane of rip_cal_linearity_fit, the accumulators and row sums
//                                    of rip_cal_noise_add and every array of rip_cal_noise_rowstats
//   always host arrays               the wrappers of stage.hip, rip_stage_invlinearity, rip_stage_noise_1f; the tables of
//                                    rip_cal_gain_ipc4d, rip_fpa_render and rip_view_render; small tables (nreads, group tables, weights, ranks,
//                                    counts) everywhere
//   host arrays OR device pointers,  rip_stage_noise_inject (in place, out == cube, included), rip_stage_poisson_resample,
//   not told apart                   rip_stage_pearson, the post-path entries of post.hip but rip_stage_pixel_area, and the entries
//                                    of calfiles.hip (rip_cal_biascorr, _pflat, _saturation, _mask): they copy through DevBuf
//                                    either way (the noise-layer driver hands them planes that live in HBM)
// DevBuf copies with hipMemcpyDefault in both directions: under unified addressing that IS the host-to-device (device-to-host)
// copy for a host array, so the one helper serves both.  A copy direction "tidied" to an explicit kind breaks the last row.
#pragma once

#include <algorithm>

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

// ---- array arguments that come with a `location`
inline bool rip_is_location(int location) { return location == RIP_HOST || location == RIP_DEVICE; }
inline int rip_check_location(rip_ctx *ctx, const char *who, const char *name, int location) {
    return rip_is_location(location) ? RIP_OK : rip_fail(ctx, RIP_EINVAL, "%s: %s %d", who, name, location);
}
// (NULL or empty ranges meet nothing)
inline bool ranges_meet(const void *a, size_t na, const void *b, size_t nb) {
    return a && b && na && nb && (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
}
inline bool aligned(const void *p, uintptr_t to) { return ((uintptr_t)p % to) == 0; }

// One array argument of n elements at a checked `location`, resolved to the device pointer `p` that the kernels get: the
// caller's own pointer for RIP_DEVICE (nothing owned) and for a NULL optional array (NULL), a scoped buffer for RIP_HOST.
// in() queues the upload of a host input; out() remembers a host output, and download() queues its way back (and does nothing
// in the other cases).  Nothing here waits.  An entry that fills a host output's buffer itself copies into `buf`.
template <typename T = char>
struct DevArg {
    T *p = nullptr;
    DevBuf<T> buf{nullptr};
    int out(rip_ctx *ctx, T *dst, size_t n, int location, const char *who = __builtin_FUNCTION()) {
        p = dst;
        if (!dst || location == RIP_DEVICE) return RIP_OK;
        buf.ctx = ctx, buf.who = who;
        host = dst, count = n;
        const int rc = buf.alloc(n);
        p = buf.p;
        return rc;
    }
    int in(rip_ctx *ctx, const T *src, size_t n, int location, const char *who = __builtin_FUNCTION()) {   // p: read only
        const int rc = out(ctx, const_cast<T *>(src), n, location, who);
        if (rc || !host) return rc;
        host = nullptr;
        return buf.copy_in(src, n);
    }
    int download() const { return host && count ? buf.download(host, count) : RIP_OK; }

private:
    T *host = nullptr;   // where a host output goes back to
    size_t count = 0;
};

// The part of a (., ny_file, nx_file) cube of 16-bit samples at a checked `location` that an entry reads: the rows y0 .. y0 + ny - 1
// of the frames f0 .. f0 + nframes - 1.  p: the device pointer of the first sample used; plane: the frame stride in samples.  A
// RIP_DEVICE cube is read where it is; of a RIP_HOST cube only those frames and rows travel, into a scoped buffer (one copy where
// the rows are whole, a 2-D copy otherwise) -- or into `into`, room for nframes * ny * nx_file samples that the caller holds
// (rip_cal_corr_pair: one allocation for the four separate frames of a cube).  Nothing here waits.
struct CubeBand {
    const uint16_t *p = nullptr;
    size_t plane = 0;
    DevBuf<uint16_t> buf;
    explicit CubeBand(rip_ctx *c, const char *who = __builtin_FUNCTION()) : buf(c, who) {}
    int in(const uint16_t *cube, int location, int ny_file, int nx_file, int f0, int nframes, int y0, int ny, uint16_t *into = nullptr) {
        rip_ctx *ctx = buf.ctx;
        const size_t plane_file = (size_t)ny_file * nx_file;
        p = cube + (size_t)f0 * plane_file + (size_t)y0 * nx_file;
        plane = plane_file;
        if (location == RIP_DEVICE) return RIP_OK;
        plane = (size_t)ny * nx_file;
        if (!into) {
            if (const int rc = buf.alloc((size_t)nframes * plane)) return rc;
            into = buf.p;
        }
        if (ny == ny_file)
            RIP_HIP(ctx, hipMemcpyAsync(into, p, (size_t)nframes * plane * 2, hipMemcpyHostToDevice, ctx->stream));
        else
            RIP_HIP(ctx, hipMemcpy2DAsync(into, plane * 2, p, plane_file * 2, plane * 2, (size_t)nframes, hipMemcpyHostToDevice,
                                          ctx->stream));
        p = into;
        return RIP_OK;
    }
};

// The launch of a kernel template <bool W8> (rip_samples.h: 8 samples or one per lane), stated once: kernel<true> where w8 holds,
// else kernel<false>.  The entry decides w8 and sizes the grid for it.
#define RIP_W8_KERNEL(kernel, w8) ((w8) ? kernel<true> : kernel<false>)
#define RIP_LAUNCH_W8(kernel, w8, grid, block, lds, stream, ...) \
    hipLaunchKernelGGL(RIP_W8_KERNEL(kernel, w8), grid, block, lds, stream, __VA_ARGS__)

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

// The stamp list of a picture entry (rip_fpa_render, rip_view_render; rip_stamp.h draws it): nstamps rows of [panel, y, x, size,
// value, character], positions inside a panel of (ny, nx) pixels.  Refuses (RIP_EINVAL, `who`: the entry's name) a stamp of a
// panel that does not exist, of size < 1, of a value or character outside 0..255, one that does not start inside its panel or
// reaches past it; otherwise leaves the stamps by panel in `sorted`, list order kept within each, and in at[p] .. at[p + 1] the
// range of panel p.
inline int rip_stamp_table(rip_ctx *ctx, const char *who, int nstamps, const int32_t *stamps, int npanel, int ny, int nx,
                           std::vector<int32_t> &at, std::vector<int32_t> &sorted) {
    at.assign(npanel + 1, 0);
    sorted.resize((size_t)nstamps * 6);
    for (int i = 0; i < nstamps; ++i) {
        const int32_t *st = stamps + 6 * i;
        if (st[0] < 0 || st[0] >= npanel) return rip_fail(ctx, RIP_EINVAL, "%s: stamp %d is of panel %d of %d", who, i, st[0], npanel);
        if (st[3] < 1 || st[4] < 0 || st[4] > 255 || st[5] < 0 || st[5] > 255)
            return rip_fail(ctx, RIP_EINVAL, "%s: stamp %d has size %d, value %d, character %d", who, i, st[3], st[4], st[5]);
        if (st[1] < 0 || st[2] < 0 || st[1] >= ny || st[2] >= nx)
            return rip_fail(ctx, RIP_EINVAL, "%s: stamp %d starts outside the image, at (%d, %d) of (%d, %d)", who, i, st[1], st[2], ny, nx);
        if (st[1] + 12 * (long)st[3] > ny || st[2] + 6 * (long)st[3] > nx)
            return rip_fail(ctx, RIP_EINVAL, "%s: stamp %d at (%d, %d) of size %d reaches past the image of (%d, %d)", who, i, st[1], st[2],
                            st[3], ny, nx);
        ++at[st[0] + 1];
    }
    for (int p = 0; p < npanel; ++p) at[p + 1] += at[p];
    std::vector<int32_t> next(at.begin(), at.end() - 1);
    for (int i = 0; i < nstamps; ++i) {
        const int32_t *st = stamps + 6 * i;
        std::copy(st, st + 6, sorted.begin() + (size_t)6 * next[st[0]]++);
    }
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
