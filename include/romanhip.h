/*
 * romanhip.h -- C-ABI of libromanhip.so: the MI355X (gfx950) implementation of the per-pixel
 * L1->L2 detector-calibration path of romanimpreprocess.
 *
 * The reference has no FFI layer; its seam is the Python-function level of
 *   src/romanimpreprocess/utils/reference_subtraction.py:16,77   (ref_subtraction_channel/_row)
 *   src/romanimpreprocess/utils/ipc_linearity.py:37,102,145,276  (ipc_fwd, ipc_rev, correct_cube, multilin)
 *   src/romanimpreprocess/utils/fitting.py:89,258                (jump_detect, ramp_fit)
 *   src/romanimpreprocess/utils/flatutils.py:20                  (get_flat)
 *   src/romanimpreprocess/L1_to_L2/gen_cal_image.py:531-629      (the in-line per-pixel arithmetic of calibrateimage)
 * Each entry point below names the reference callable it replaces.  The Python binding a
 * reference maintainer would add is shown in INTEGRATION.md (ctypes).
 *
 * Conventions
 *   - plain C types only; all arrays are C-order, dense.
 *   - a frame has `ny` rows and `nx` science columns (4096 x 4096 in flight); the reference
 *     pixel border is `nborder` (4); the active region is (ny-2nb) x (nx-2nb); the reference
 *     output ("amp33") has `ny` rows x 128 columns.  nx must be a multiple of 128 when the
 *     reference-pixel stage is used.
 *   - the caller owns every buffer it passes; the library copies CALDIR arrays to the device at
 *     rip_caldir_upload and owns those copies.
 *   - `location` says where ramp/output buffers live: RIP_HOST (the library stages them through
 *     HBM) or RIP_DEVICE (pointers into this process's HIP address space, e.g. torch tensors).
 *   - every function returns 0 on success, a negative rip_status otherwise; rip_last_error()
 *     gives the message.  No exceptions or longjmp cross this boundary.
 *   - one rip_ctx per GPU; a ctx is not thread-safe (one calling thread at a time).
 */
#ifndef ROMANHIP_H
#define ROMANHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RIP_VERSION 100 /* 0.1.0 */
/* rip_version() of a library compiled with -DRIP_TIMING_BUILD (timing experiments whose kernels may skip phases: results
   invalid by construction) = RIP_VERSION + RIP_TIMING_BUILD_FLAG; the Python binding refuses such a library unless
   ROMANHIP_ALLOW_TIMING_BUILD=1 */
#define RIP_TIMING_BUILD_FLAG 1000000
#define RIP_MAX_GROUPS 64
#define RIP_CHANNEL_WIDTH 128

typedef struct rip_ctx rip_ctx;

typedef enum { RIP_OK = 0, RIP_EINVAL = -1, RIP_ENOMEM = -2, RIP_EHIP = -3, RIP_ESTATE = -4 } rip_status;
typedef enum { RIP_F32 = 0, RIP_F64 = 1, RIP_U16 = 2, RIP_F16 = 3 } rip_dtype;
typedef enum { RIP_HOST = 0, RIP_DEVICE = 1 } rip_location;
/* rip_ramp_desc::inputs_ready: what the library may assume about DEVICE-resident inputs when rip_calibrate is called */
typedef enum { RIP_INPUTS_STREAM_ORDERED = 0, RIP_INPUTS_COMPLETE = 1 } rip_inputs_ready;

/* stages of the chain (bit mask), in the order of calibrateimage (gen_cal_image.py:531-629) */
enum {
    RIP_STAGE_REFPIX = 1 << 0,  /* :531-556  reference-pixel row/channel correction              */
    RIP_STAGE_BIAS = 1 << 1,    /* :559-565  data[act] -= biascorr                                  */
    RIP_STAGE_LIN = 1 << 2,     /* :580-588  multilin + pdq |= dq_lin                               */
    RIP_STAGE_IPC = 1 << 3,     /* :594-597  correct_cube                                           */
    RIP_STAGE_RAMPFIT = 1 << 4, /* :600      ramp_fit (slope, errors, jump flags, flag propagation) */
    RIP_STAGE_DARK = 1 << 5,    /* :603      slope[act] -= IPC-deconvolved dark rate                 */
    RIP_STAGE_FLAT = 1 << 6,    /* :616-629  get_flat flags + divide by flat/AreaFactor              */
    RIP_STAGE_ALL = 0x7f
};

/* ---- CALDIR arrays of one SCA (host pointers) ------------------------- */
typedef struct {
    int32_t ny, nx, nborder;
    /* dark file: data (ngrp_dark,ny,nx) f32, dark_slope (ny,nx) f32, dq (ny,nx) u32 or NULL */
    int32_t ngrp_dark;
    const float *dark_data;
    const float *dark_slope;
    const uint32_t *dark_dq;
    /* read file: data (ny,nx) f32; amp33.med (ny,128) f32 or NULL; refout_slope = the scalar of
       gen_cal_image.py:542-553 (computed by the host from M_PINK, RU_PINK, C_PINK, median(std)) */
    const float *read_noise;
    const float *amp33_med;
    double refout_slope;
    /* gain file: data (ny,nx), f32 or f64 */
    const void *gain;
    int32_t gain_dtype;
    /* linearitylegendre file: data (lin_nplanes,ny,nx) f32; Smin,Smax,Sref (ny,nx) f32; dq u32 */
    int32_t lin_nplanes;
    const float *lin_coefs;
    const float *lin_smin, *lin_smax, *lin_sref;
    const uint32_t *lin_dq;
    /* ipc4d file: data (3,3,ny-2nb,nx-2nb), f32 or f64; NULL = no IPC correction */
    const void *ipc4d;
    int32_t ipc_dtype;
    /* flat (pflat) file: data (ny,nx) f32; NULL = no flat division */
    const float *flat;
    /* biascorr file: data (ngrp_bias,ny-2nb,nx-2nb) f32; NULL = skip */
    int32_t ngrp_bias;
    const float *biascorr;
    /* saturation file: data (ny,nx) f32 threshold in DN, dq (ny,nx) u32 (NO_SAT_CHECK honoured) or NULL.
       Only needed for rip_ramp_desc::flag_saturation; NULL = not available. */
    const float *saturation;
    const uint32_t *saturation_dq;
} rip_caldir_desc;

/* ---- ramp-fit plan: MA table, weights, thresholds (host scalars) --- */
typedef struct {
    int32_t ngrp;
    int32_t exclude_first;     /* config EXCLUDE_FIRST (gen_cal_image.py:142, fitting.py:159-161)     */
    int32_t do_not_flag_first; /* read_pattern[0] == [0] (gen_cal_image.py:583-584)                   */
    float tbar[RIP_MAX_GROUPS]; /* meta["tbar"], f32 (gen_cal_image.py:137)                           */
    float tau[RIP_MAX_GROUPS];  /* meta["tau"],  f32 (:138)                                            */
    int16_t nreads[RIP_MAX_GROUPS]; /* meta["N"], int16 (:135)                                          */
    float K[RIP_MAX_GROUPS];    /* fitting.construct_weights(...) cast f32 (fitting.py:86)             */
    /* per fit variant v: v = 0 is the full ramp; v = 1.. are ramps truncated to [0, g_v) for
       g_v = ngrp-1 ... 3+start (fitting.py:326).  coef = Poisson coefficient (fitting.py:196-200),
       rfac = sqrt(sum K^2/N) (fitting.py:209); both f32 scalars computed by the host exactly as the
       reference computes them. */
    int32_t nvariants;
    int32_t variant_g[RIP_MAX_GROUPS];
    float variant_coef[RIP_MAX_GROUPS];
    float variant_rfac[RIP_MAX_GROUPS];
    /* jump thresholds (fitting.py:172-184) */
    double sthresh_a, sthresh_b, ithresh_a, ithresh_b;
} rip_plan_desc;

/* ---- one ramp in, one calibrated image out ---------------------------------------------- */
typedef struct {
    int32_t location;      /* rip_location of every pointer in this struct                             */
    int32_t ngrp;
    const void *data;      /* (ngrp,ny,nx) u16 (Level-1) or f32 (after dq-init)                        */
    int32_t data_dtype;    /* RIP_U16 or RIP_F32                                                       */
    const uint16_t *amp33; /* (ngrp,ny,128) or NULL                                                    */
    const uint8_t *groupdq;  /* (ngrp,ny,nx) after dq-init + saturation flagging                       */
    const uint32_t *pixeldq; /* (ny,nx)                                                                */
    const double *area_factor; /* (ny,nx) f64 pixel-area ratio (gen_cal_image.py:618-622) or NULL = 1  */
    /* optional override of the channel-step line fit: (ngrp,nx/128,2) f64 (m,c) computed by the
       host with LAPACK exactly as reference_subtraction.py:57-60; NULL = fitted on the device */
    const double *channel_lines;
    /* dq-init + saturation flagging on the device before the chain (gen_cal_image.py:148-185: romancal's dq_init and
       saturation steps with n_pix_grow_sat = 1; stcal's source is not in the reference tree, so this follows the
       documented behaviour restated in romanimpreprocess_amd/L1_to_L2/gen_cal_image.py:flag_saturation -- PARITY
       UNPINNED).  flag_saturation != 0: group g >= sat_skip_firstn is SATURATED where data >= threshold in the 3x3
       neighbourhood, sticky for later groups and set on the sat_backup preceding groups; pixeldq |= SATURATED where any
       group is flagged; DO_NOT_USE is set on group 0 when the plan excludes the first group.  groupdq may then be NULL
       (= zeros); pixeldq is the mask dq.  A pixel is checked where its threshold is finite (up to FLT_MAX, as np.isfinite
       has it) and its saturation dq lacks NO_SAT_CHECK; a pixel that is not checked raises no flag whatever its samples
       (an infinite one included) and still receives its neighbours'. */
    int32_t flag_saturation;
    int32_t sat_backup;      /* config SATURATION_BACKUP (gen_cal_image.py:172), default 1.  Any non-negative value is valid; it is
                                clamped to the group count, from which on larger values mean the same */
    int32_t sat_skip_firstn; /* 1 in the reference's call */
    /* groups that average several reads: a pixel whose LAST reads saturate holds a group value below the threshold, so
       the group is compared with threshold * sat_dilution[g], sat_dilution[g] = mean(read_pattern[g]) / read_pattern[g][-1]
       (stcal's read_pattern rule, "checks for groups with some reads saturated", docs/L1_to_L2_README.rst:139-141; the
       reference hands the read pattern over at gen_cal_image.py:172-185).  Host pointer to ngrp doubles (also for device
       ramps), or NULL = 1 for every group.  A NaN entry (0/0 for a group holding only read 0) never flags. */
    const double *sat_dilution;
    /* When the DEVICE-resident inputs of this call (data, amp33, groupdq, pixeldq, area_factor, channel_lines) are valid.
       The reference-pixel pre-pass of a call reads data / amp33 on a SECOND stream so that it can run beside the previous
       call's main kernel; these two fields say what that stream has to wait for.  Ignored for location == RIP_HOST.
         inputs_ready == RIP_INPUTS_STREAM_ORDERED (0, the default): the inputs are complete, or are written by work the
             caller has ALREADY queued on rip_stream().  Every kernel of the call, the pre-pass included, is ordered behind
             everything queued on rip_stream() at the time of the call (so the pre-pass cannot overlap the previous call's
             main kernel: correct for every caller that uses one stream, ~0.03-0.06 ms per 4096^2 x 8 ramp slower).
         inputs_ready == RIP_INPUTS_COMPLETE: the caller guarantees that the inputs are complete NOW (a ramp resident since
             the last synchronisation, ...): the pre-pass starts at once.
         ready_event != NULL (a hipEvent_t as void*, recorded by the caller behind the work that writes the inputs, on any
             stream): the pre-pass and the main kernels wait for exactly that event; inputs_ready is not looked at.  This is
             the form for inputs produced on another stream (a torch side stream, a copy engine) without giving up the
             overlap.  The event must stay alive until the call returns (the wait is queued before that). */
    int32_t inputs_ready;
    void *ready_event;
    /* location == RIP_HOST only: OR DO_NOT_USE into groupdq[0] on the library's device copy (gen_cal_image.py:142-143 does it to
       the array itself when the first group is excluded; a host caller that wants its own array untouched would otherwise copy
       134 MB to set one plane's bit).  The groupdq returned carries the bit, as the reference's does. */
    int32_t or_first_group;
    /* location == RIP_HOST only: a Level-1 exposure stored with the reference read subtracted (the EXTRACT_REF block of
       sim_to_isim.py:711-730, rip_synth_extract_ref: data[k] = clip(i32(resultant k+1) - (i32(resultant 0) - offset), 0, 65535),
       reference_read = resultant 0, the read pattern without its first group).  The library decodes its device copies of data
       and amp33 in place behind the upload -- v = i32(enc) + i32(reference) - offset, rip_stage_decode_reference_read -- before
       anything reads them; the chain then sees a u16 cube of ngrp groups, one fewer than the exposure had (the CALDIR arrays may
       hold that one group more: biascorr[de:], gen_cal_image.py:561-562).  A v outside 0..65535 means that the three pieces do
       not belong together: the samples are counted, and the call (in a batch: that ramp) fails with RIP_EINVAL once the results
       are down; its outputs are invalid.  RIP_EINVAL at once: reference_read with data_dtype != RIP_U16, reference_amp33 without
       amp33, either with location == RIP_DEVICE (a device caller decodes its own arrays with the stage entry on the context's
       stream and then calibrates as usual).  All zero = the data are not encoded: nothing changes. */
    const uint16_t *reference_read;    /* (ny,nx) or NULL = data is not encoded */
    const uint16_t *reference_amp33;   /* (ny,128) or NULL = amp33 is used as stored */
    int32_t data_encoding_offset;
} rip_ramp_desc;

typedef struct {
    int32_t location;
    float *slope;        /* (ny,nx) DN/s                                  */
    float *err_read;     /* (ny,nx)                                       */
    float *err_poisson;  /* (ny,nx)                                       */
    uint32_t *pixeldq;   /* (ny,nx)                                       */
    uint8_t *groupdq;    /* (ngrp,ny,nx) or NULL                          */
    float *cube;         /* (ngrp,ny,nx) corrected cube (after the last cube stage run) or NULL */
} rip_outputs;

/* ---- life cycle ------------------------------------------------------------------------- */
int rip_version(void);
int rip_ctx_create(int device_id, rip_ctx **out);
void rip_ctx_destroy(rip_ctx *ctx);
const char *rip_last_error(const rip_ctx *ctx); /* ctx may be NULL: message of the last failed create */
int rip_synchronize(rip_ctx *ctx);
/* the HIP stream all work of this ctx is enqueued on (hipStream_t as void*) */
void *rip_stream(rip_ctx *ctx);
/* page-locked host memory for arrays handed to the library with location RIP_HOST (the reference's numpy arrays are
   pageable; buffers from here are copied at PCIe rate).  NULL on failure (rip_last_error). */
void *rip_host_alloc(rip_ctx *ctx, size_t bytes);
void rip_host_free(rip_ctx *ctx, void *p);

/* CALDIR: replaces the per-call asdf.open(caldir[...]) of the reference with device-resident
   copies (plus the per-SCA constants derived from them: IPC-deconvolved dark rate
   gen_cal_image.py:217-221 and the flat of flatutils.get_flat) */
int rip_caldir_upload(rip_ctx *ctx, int sca_slot, const rip_caldir_desc *desc);
int rip_caldir_drop(rip_ctx *ctx, int sca_slot);
/* 1: the set in sca_slot passed the screen rip_caldir_upload runs over its device copies -- every plane of dark.data and of
   biascorr, the Legendre planes, Smin, Smax, Sref, amp33.med finite and within 2^20, Smax - Smin (f32) non-zero, the (f32)
   gain within 2^-10 .. 2^10 in magnitude, ipc4d within 2^4, slope_ref within 2^10 -- so that group 0 of ANY u16 ramp comes
   out of the chain finite (the chain of bounds: csrc/caldir.hip) and the fused kernel may skip an excluded first group
   (option "skip_first").  0: it did not (one NaN anywhere is enough; such a set runs the full kernel form, same results).
   RIP_EINVAL for an empty slot. */
int rip_caldir_first_group_safe(rip_ctx *ctx, int sca_slot);
/* Has the set in sca_slot a bias correction to make?
     RIP_BIAS_ABSENT   no biascorr was given
     RIP_BIAS_PRESENT  one was given and is subtracted by every call with RIP_STAGE_BIAS
     RIP_BIAS_DROPPED  one was given and EVERY 32-bit word of it, over all its planes, was 0x00000000 (+0.0f): S - (+0.0f) is S
                       for every f32, so rip_caldir_upload keeps no device copy of it and calls subtract nothing.  The test is on
                       bits: one -0.0 (S - (-0.0f) turns an S of -0 into +0) or one non-zero sample anywhere keeps the array.
                       A ramp with more groups than the array had planes still fails with RIP_EINVAL, as on any biascorr.
   A set that is ABSENT or DROPPED is screened for rip_caldir_first_group_safe like any other and takes the fused kernel without
   its biascorr stream (rip_last_chain_bias_stream), as does a call whose stage mask leaves RIP_STAGE_BIAS out.
   RIP_EINVAL for an empty slot. */
enum { RIP_BIAS_ABSENT = 0, RIP_BIAS_PRESENT = 1, RIP_BIAS_DROPPED = 2 };
int rip_caldir_bias_state(rip_ctx *ctx, int sca_slot);

/* plan: replaces meta{ngrp,N,tbar,tau,K,jump_detect_pars} of gen_cal_image.py:123-145,439-444 */
int rip_plan_create(rip_ctx *ctx, const rip_plan_desc *desc, int *plan_id);
int rip_plan_destroy(rip_ctx *ctx, int plan_id);
/* 1: a plan made from desc excludes the first group and gives group 0 the weight zero in the full-ramp weights and in the
   weights of every truncated variant (what skipping group 0 in the fused kernel rests on; rip_plan_create checks the same of
   the weights it uploads); 0 otherwise.  Host arithmetic: needs no context and no GPU. */
int rip_plan_desc_first_weight_zero(const rip_plan_desc *desc);

/* the chain: replaces gen_cal_image.py:531-629 (stages selects a sub-chain).  Asynchronous with
   respect to the host when location == RIP_DEVICE (use rip_synchronize / the stream).
   Device-resident INPUTS: by default the call is ordered behind everything already queued on rip_stream() (inputs written
   by a kernel the caller queued there are safe without a synchronisation); rip_ramp_desc::inputs_ready / ready_event let a
   caller whose inputs are complete, or guarded by an event of another stream, keep the overlap of the reference-pixel
   pre-pass (second stream) with the previous call's main kernel.  Outputs are ordered on rip_stream() either way; with
   "overlap" off every kernel of a call runs on rip_stream(). */
int rip_calibrate(rip_ctx *ctx, int sca_slot, int plan_id, unsigned stages, const rip_ramp_desc *in,
                  const rip_outputs *out);

/* A batch of n ramps in HOST memory through the same chain, pipelined over PCIe: upload of ramp i+1, chain of ramp i and
   download of ramp i-1 overlap (three streams, two sets of device buffers); results equal those of n single calls.  What a
   batch driver (runs/summer2025run/OpenUniverse_to_L1L2.py:123-137: every SCA of an exposure) hands its arrays to.  All
   ramps share the CALDIR slot, the plan, the group count and the data dtype; location must be RIP_HOST in every
   descriptor; the stage mask must include the ramp fit; outputs::cube is not available here.  Page-locked arrays
   (rip_host_alloc) make the copies run at PCIe rate in both directions at once.  Returns when everything has arrived. */
int rip_calibrate_batch(rip_ctx *ctx, int sca_slot, int plan_id, unsigned stages, int n, const rip_ramp_desc *in,
                        const rip_outputs *out);
/* after rip_calibrate_batch: the number of ramps (from the front of the batch) whose outputs are complete.  n on success;
   after an error return every stream has been drained, outputs [0, this) are valid and the rest are not. */
int rip_calibrate_batch_completed(rip_ctx *ctx);

/* ---- stage-level entry points (for function-level drop-in and parity tests) ------------------
   Array arguments of this section are HOST arrays.  (Which stage-level entry points also take device pointers is stated at
   each; the list is at the top of romanimpreprocess_amd/csrc/rip_host.h.) */

/* reference_subtraction.ref_subtraction_row(image, use_ref_channel=True, slope) followed by
   ref_subtraction_channel(image, use_ref_channel=True) on one (ny, nx+128) f32 image, in place: rip_stage_refpix_row
   (nside = nx, RIP_ROW_SLOPE_F64) then rip_stage_refpix_channel (windows [0, 128) + 128 k, nx/128+1 of them).
   do_row / do_channel select the steps; medians out (optional): ref_med (ny) f32, ctr (1) f32,
   bottom_top (nx/128+1, 2) f32; lines in (optional, (nx/128+1,2) f64 (m,c)) override the fit. */
int rip_stage_refpix_image(rip_ctx *ctx, float *image, int ny, int nx, double slope, int do_row, int do_channel,
                           const double *lines, float *ref_med, float *ctr, float *bottom_top);

/* reference_subtraction.ref_subtraction_row with ANY of its arguments (reference_subtraction.py:77-125) on one (ny, width) f32
   image, in place.  nside = science columns (the reference hard-codes 4096): border pixels 0:4 and nside-4:nside, science
   pixels 4:nside-4, reference output nside:nside+128.  use_ref_channel: the row medians are those of the reference output
   (width >= nside+128), else of the 4+4 border pixels (:108-111).  mode:
     RIP_ROW_MEDIANS_ONLY  no update: ref_med / sci_med / ctr out -- what the host needs for the np.polyfit of slope=None (:114)
     RIP_ROW_SLOPE_F64     image = f32(f64(image) - slope * f64(f32(ref_med - ctr)))   (slope a numpy f64 scalar, :123)
     RIP_ROW_SLOPE_F32     image = image - f32(slope) * (ref_med - ctr), every operation f32 (slope a Python float or a numpy
                           f32 scalar, as np.polyfit returns it for f32 medians: numpy's promotion rules)
   ref_med, sci_med (ny) f32 and ctr (1) f32 out, each may be NULL (sci_med costs a 4088-value selection per row).
   Every median is np.median's: NaN where a value is NaN (one NaN in a reference pixel makes ctr, and so the image, NaN), never
   -0.  Limits (RIP_EINVAL beyond them): 16 <= nside <= 32776 and 1 <= ny <= 32768 -- a median is one sort of at most 32768
   values in 128 KiB of LDS, which gfx950 grants a workgroup. */
enum { RIP_ROW_MEDIANS_ONLY = 0, RIP_ROW_SLOPE_F64 = 1, RIP_ROW_SLOPE_F32 = 2 };
int rip_stage_refpix_row(rip_ctx *ctx, float *image, int ny, int width, int nside, int use_ref_channel, int mode, double slope,
                         float *ref_med, float *sci_med, float *ctr);

/* reference_subtraction.ref_subtraction_channel with ANY of its arguments (:16-74): nchan windows of columns
   [channel_start + 128 k, channel_end + 128 k), k = 0 .. nchan-1 (32, or 33 with use_ref_channel), handled one after the
   other as the reference's loop does (windows wider than 128 columns overlap and see each other's updates); per window
   the medians of rows 0:4 and ny-4:ny, the line through (1.5, b), (ny-2.5, t) -- or lines (nchan,2) f64 (m,c) from the
   caller's LAPACK -- subtracted from every row.  bottom_top (nchan,2) f32 out or NULL.  Medians as above (a NaN in a bottom
   or top reference row makes its window NaN).  Limits (RIP_EINVAL beyond them): ny >= 8, 1 <= channel_end - channel_start
   <= 8192 (4 x 8192 values a median), every window inside the image. */
int rip_stage_refpix_channel(rip_ctx *ctx, float *image, int ny, int width, int channel_start, int channel_end, int nchan,
                             const double *lines, float *bottom_top);

/* The reference-pixel TABLES the chain applies to a ramp (gen_cal_image.py:531-556 through reference_subtraction.py:16-125,
   with the reference output: use_ref_channel=True, slope given), from host arrays: data (ngrp,ny,nx) u16|f32, dark (>= ngrp,ny,nx)
   f32, amp33 (ngrp,ny,128) u16, amp33_med (ny,128) f32 -> rowcorr (ngrp,ny) f64 = slope * f64(f32(row median - ctr)) and
   lines (ngrp,nx/128,2) f64 = (m, c) of the science channels.  form: 1 = the single-launch kernel (refpix_one.hip; frames up to
   4096 rows), 0 = the multi-launch kernels (refpix.hip), -1 = what rip_calibrate takes for a pre-pass in front of its own ramp
   (option "prepass_form").  Both forms give identical bits.  status out (may be NULL): != 0 when a group barrier of the single-launch kernel
   timed out since the last status read; the read clears the word, so a timeout is reported once. */
int rip_stage_refpix_tables(rip_ctx *ctx, const void *data, int data_dtype, const float *dark, const uint16_t *amp33,
                            const float *amp33_med, double slope, int ngrp, int ny, int nx, int form, double *rowcorr,
                            double *lines, int *status);

/* ipc_linearity.multilin: S (ngrp,ny,nx) f32 -> phi (ngrp,ny,nx) f32, dq (ny,nx) u32.
   attempt_corr (ngrp,ny,nx) u8 nonzero = flag when extrapolated, or NULL = all. */
int rip_stage_multilin(rip_ctx *ctx, const float *S, int ngrp, int ny, int nx, int nplanes, const float *coefs,
                       const float *smin, const float *smax, const float *sref, const uint32_t *lin_dq,
                       int do_not_flag_first, const uint8_t *attempt_corr, float *phi, uint32_t *dq);

/* ipc_linearity.ipc_fwd / ipc_rev on one (ny,nx) image with kernel (3,3,ny,nx); gain NULL or (ny,nx).
   image/out dtype = img_dtype (f32|f64); kernel k_dtype; gain g_dtype; out dtype = promote(all). */
int rip_stage_ipc_image(rip_ctx *ctx, int reverse, int order, const void *image, int img_dtype, int ny, int nx,
                        const void *kernel, int k_dtype, const void *gain, int g_dtype, void *out);

/* ipc_linearity.correct_cube: data (ngrp,ny,nx) f32 in place; kernel (3,3,ny-2nb,nx-2nb); gain (ny,nx) or NULL */
int rip_stage_correct_cube(rip_ctx *ctx, float *data, int ngrp, int ny, int nx, int nb, const void *kernel,
                           int k_dtype, const void *gain, int g_dtype);

/* fitting.ramp_fit: data (ngrp,ny,nx) f32; rdq u8 and pdq u32 updated in place; outputs (ny,nx) f32 */
int rip_stage_ramp_fit(rip_ctx *ctx, int plan_id, const float *data, uint8_t *rdq, uint32_t *pdq, int ny, int nx,
                       int nb, const void *gain, int g_dtype, const float *read_noise, float *slope,
                       float *err_read, float *err_poisson);

/* fitting.jump_detect (fitting.py:89-255): ONE pass of slope fit + jump flagging over all ngrp groups of the plan with the
   plan's weights K.  data (ngrp,ny,nx) f32; rdq (ngrp,ny,nx) u8 updated in place (JUMP_DET OR-ed into group i of a flagged
   difference, active region only: the reference ORs into whatever flag cube it is handed); slope / err_read / err_poisson
   (ny,nx) f32 out; smap (2*(ngrp-start)-3, ny, nx) f32 out: the significance of every tested difference, every pixel, in
   the reference's exact operation order.  truncate_ramp = t of the reference is this call under a plan of t groups holding
   the two-point weights of fitting.py:162-167 (the Python mirror builds it). */
int rip_stage_jump_detect(rip_ctx *ctx, int plan_id, const float *data, uint8_t *rdq, int ny, int nx, int nb, const void *gain,
                          int g_dtype, const float *read_noise, float *slope, float *err_read, float *err_poisson, float *smap);

/* flatutils.get_flat: flat (ny,nx) f32, gain, kernel; pdq updated in place (may be NULL) */
int rip_stage_get_flat(rip_ctx *ctx, const float *flat, int ny, int nx, int nb, const void *gain, int g_dtype,
                       const void *kernel, int k_dtype, int ipc_deconvolve, uint32_t *pdq, float *out);

/* ---- post-path 2-D reductions: between the chain's outputs and the L2 file -------------------
   Array arguments of this section, of the noise-layer section (rip_stage_noise_inject, rip_stage_poisson_resample) and of
   rip_stage_pearson may be host arrays OR device pointers (each is copied with hipMemcpyDefault): a driver that keeps its
   planes in HBM (the noise-layer loop, romanimpreprocess_amd/L1_to_L2/gen_noise_image.py) hands them over without a PCIe
   round trip.  The calls stay synchronous: they return when the result is complete.  Small tables (ranks, counts, Legendre
   tables, coefficients, weights) are host arrays. */

/* maskhandling.CombinedMask.build (maskhandling.py:82-117): grow[bit] in {0, 1, 5, 9, 25} = how the layer of that dq bit
   is grown (copy, plus, 3x3, 5x5; zero padded); mask (ny,nx) u8 = 1 where masked.  Exact. */
int rip_stage_build_mask(rip_ctx *ctx, const uint32_t *dq, int ny, int nx, const uint8_t grow[32], uint8_t *mask);

/* SLICEOUT endslice (gen_cal_image.py:697-712): (ny-2nb, nx-2nb) i8, iend-1 of the last group that first saturates, -1 if
   none.  Exact. */
int rip_stage_endslice(rip_ctx *ctx, const uint8_t *rdq, int ngrp, int ny, int nx, int nb, int8_t *out);

/* sky.binkxk(np.where(mask, nan, arr), k) (sky.py:20-41): (ny/k, nx/k) f32 block means, NaN where the block holds a
   masked or NaN pixel; mask may be NULL.  f32 sums in row-then-column order (numpy's order differs: ~1e-7 relative). */
int rip_stage_bin_mean(rip_ctx *ctx, const float *arr, const uint8_t *mask, int ny, int nx, int k, float *out);

/* Order statistics ignoring NaN, per block of ky x kx pixels (nby x nbx blocks from (y0,x0)) of an (ny,nx) f32 image:
   the building block of np.nanpercentile (sky.py:72-74) and of the block nan-medians of medfit (sky.py:152).
   counts[blk] = non-NaN elements; vals[blk*nranks + r] = element of 0-based ascending rank ranks[blk*nranks + r] (NaN
   when out of range).  ranks may be NULL with nranks = 0 (counts only).  Exact.  At most 65535 blocks (nby * nbx) a call:
   more is RIP_EINVAL. */
int rip_stage_select_ranks(rip_ctx *ctx, const float *arr, int ny, int nx, int y0, int x0, int ky, int kx, int nby, int nbx,
                           int nranks, const int64_t *ranks, int64_t *counts, float *vals);

/* smoothed histogram of smooth_mode (sky.py:80-84): out[i] = sum over non-NaN x of exp(-0.5 ((z[i]-x)/scale)^2), nz <= 32,
   f64 (summation order differs from numpy: ~1e-13 relative; it is fixed, so a call is reproducible to the bit). */
int rip_stage_gauss_hist(rip_ctx *ctx, const float *arr, int64_t n, const double *z, int nz, double scale, double *out);

/* Legendre model of medfit (sky.py:183-191): model = f32(sum_k coef[k] * outer(LPY[j_k], LPX[i_k])) accumulated in f64 in
   the order k = 0.. with (i, j): i = 0..order, j = 0..order-i; LPX (order+1, nx), LPY (order+1, ny) f64 from the host.
   subtract != 0: arr -= model in place; model_out (ny,nx) f32 optional.  Exact. */
int rip_stage_legendre2d(rip_ctx *ctx, float *arr, int ny, int nx, int order, const double *LPX, const double *LPY,
                         const double *coef, int subtract, float *model_out);

/* A FITS celestial WCS of a zenithal projection (Calabretta & Greisen 2002, sect. 5.1), optionally with SIP distortion: what
   the exposure's FITSWCS header (gen_cal_image.py:64-87) holds, parsed and validated by the host
   (romanimpreprocess_amd/utils/coordutils.py:FitsWCS).  Pixel coordinates are 0-based and crpix is a 0-based pixel
   coordinate (the header's CRPIX minus 1, the convention sim_to_isim.py:501-503 writes the header in).  Angles in degrees. */
typedef enum { RIP_PROJ_TAN = 0, RIP_PROJ_STG = 1, RIP_PROJ_ZEA = 2, RIP_PROJ_ARC = 3, RIP_PROJ_SIN = 4 } rip_projection;
#define RIP_SIP_MAX_ORDER 9
typedef struct {
    int32_t projection;  /* rip_projection                                                                              */
    int32_t sip_order;   /* 0 = no SIP; else max(A_ORDER, B_ORDER) <= RIP_SIP_MAX_ORDER                                  */
    double crpix[2];     /* 0-based reference pixel (x, y)                                                              */
    double cd[2][2];     /* CDi_j, or CDELTi * PCi_j                                                                    */
    double crval[2];     /* (alpha0, delta0) of the reference point                                                     */
    double lonpole;      /* LONPOLE, 180 by default                                                                    */
    double sip_a[RIP_SIP_MAX_ORDER + 1][RIP_SIP_MAX_ORDER + 1]; /* A_p_q at [p][q], zero where absent                     */
    double sip_b[RIP_SIP_MAX_ORDER + 1][RIP_SIP_MAX_ORDER + 1]; /* B_p_q at [p][q], zero where absent                     */
} rip_wcs_desc;

/* coordutils.pixelarea (coordutils.py:17-82) on an (ny,nx) frame: the solid angle of every pixel from the WCS evaluated on the
   pixel grid x = -1..nx, y = -1..ny, re-projected to Lambert equal-area coordinates about the pole of the hemisphere of grid
   point (-1,-1), and central differences of those; out (ny,nx) f64 = area / scale (scale = 1: steradians; Omega_ideal: the
   AreaFactor of gen_cal_image.py:618-621, which rip_ramp_desc::area_factor takes).  f64 throughout.
   out_location RIP_HOST: out is a host array, the call returns when it is filled; RIP_DEVICE: out is device memory, written
   in place, ordered on rip_stream().  RIP_EINVAL for an unknown projection, sip_order outside 0..9, ny or nx < 1, scale <= 0
   or a non-finite descriptor. */
int rip_stage_pixel_area(rip_ctx *ctx, const rip_wcs_desc *wcs, int ny, int nx, double scale, int out_location, double *out);

/* ---- simulation side ------------------------------------------------- */
/* ipc_linearity.invlinearity (ipc_linearity.py:347-394): 24 bisection steps on z in (-1, 1) of the Legendre series evaluated
   as ipc_linearity._lin does without the extrapolation branch, then S = Smin + (Smax - Smin)/2 * (1 + z).  slin (ny,nx) f32 or
   f64 (dtype); coefs (nplanes,ny,nx), smin, smax f32 already cut to the block; S has slin's dtype; exflag (ny,nx) u8 or NULL
   (|z| > 1 at the last evaluation: the reference's second return value).  Host arrays (no device pointers).  Exact. */
int rip_stage_invlinearity(rip_ctx *ctx, const void *slin, int dtype, int ny, int nx, int nplanes, const float *coefs,
                           const float *smin, const float *smax, void *S, uint8_t *exflag);

/* ---- noise layers ---------------------------------------------------- */
/* gen_noise_image.make_noise_cube, read-noise injection (gen_noise_image.py:120-134): per group k and active pixel
   data' = u16(rint(clip(f32(data) + f32(f64(normal) * (f64(read) / sqrt(f64(N_k)))), 0, 65535))); border pixels unchanged.
   cube, out (ngrp,ny,nx) u16; read_noise (ny,nx) f32; nreads[ngrp]; normals (ngrp,ny-2nb,nx-2nb) f32 standard normal
   deviates from the caller, or NULL: drawn on the device from a counter-based generator keyed by (seed, layer, group,
   pixel).  cube, read_noise, normals and out are host arrays or device pointers; out may be cube (in place).  Exact given the
   normals. */
int rip_stage_noise_inject(rip_ctx *ctx, const uint16_t *cube, int ngrp, int ny, int nx, int nb, const float *read_noise,
                           const int32_t *nreads, const float *normals, uint64_t seed, uint32_t layer, uint16_t *out);

/* sim_to_isim.noise_1f_frame (sim_to_isim.py:265-303): nframes frames of rows x width samples of 1/f noise (unit variance per
   logarithmic frequency range), the generator behind the correlated part of a read-noise layer (:376-399).  For each frame
   L = 2*rows*width complex samples (n_k + i n_{L+k}) |k|^-1/2 are Fourier transformed in f64 (hipFFT), the real part of the
   first L/2 outputs / sqrt(2) minus its mean is the frame, cast to f32.  normals (nframes, 2L) f64 standard normal deviates
   from the caller, or NULL: drawn on the device (seed, stream_id).  out (nframes, rows, width) f32.  Host arrays (no device
   pointers: rip_synth_noise_1f leaves the frames on the device).  Agrees
   with the reference's numpy FFT to rounding (~1e-12 relative before the cast), not bit for bit. */
int rip_stage_noise_1f(rip_ctx *ctx, int rows, int width, int nframes, const double *normals, uint64_t seed,
                       uint32_t stream_id, float *out);

/* gen_noise_image.make_noise_cube, resampled Poisson layer 'P..r' (gen_noise_image.py:262-331) on n pixels: electrons per frame
   e = clip(skylevel * gain * frame_time, 0); for each read a Poisson deviate of mean e, re-centred, in DN, accumulated into the
   change of every resultant (group j = reads group_first[j] .. + group_count[j] - 1), then diff += sum_j w[endslice][j] *
   delta[j] with the weight vector of the ramp's end slice (weights (ngrp,ngrp) f32 row-major, has_weights[es] = 0 where the
   reference has no vector; endslice (n) i8 already mapped as the reference does, <= 0 -> ngrp - 1).  samples (nsamp,n) f64
   Poisson deviates from the caller, or NULL: drawn on the device (inversion / PTRS on Philox uniforms keyed by seed, layer,
   read, pixel).  gain (n) f32 or f64, already clipped to [1e-4, 1e4].  Up to 16 groups.  skylevel, gain, endslice, samples and
   diff (in/out) are host arrays or device pointers; the group tables and weights are host arrays.
   Exact given the deviates. */
int rip_stage_poisson_resample(rip_ctx *ctx, const float *skylevel, const void *gain, int gain_dtype, size_t n,
                               double frame_time, int ngrp, const int32_t *group_first, const int32_t *group_count,
                               const float *weights, const uint8_t *has_weights, const int8_t *endslice,
                               const double *samples, int nsamp, uint64_t seed, uint32_t layer, float *diff);

/* ---- statistics over many noise realisations of one ramp -- DEVICE pointers, asynchronous ------- */
/* Replaces the per-pixel arithmetic of validation_tests/many_realizations.py:57-106 on stacks (nseeds, rows, nx) that stay
   in HBM (256 realisations of a 4096 x 4096 SCA: 56 GB).  All results are exact (f32 operations in the reference's order,
   medians by selection). */

/* :69-72  out (ny,nx) f32 = f32(cube[ga]) - f32(cube[gb]) of a Level-1 cube (ngrp,ny,nx) u16 (the reference: ga = last
   group, gb = 1). */
int rip_stats_l1_diff(rip_ctx *ctx, const uint16_t *cube, int ngrp, int ny, int nx, int ga, int gb, float *out);

/* :74-77  one realisation's L2 planes into the stacks: image = slope and err = sqrt(err_read^2 + err_poisson^2) inside a
   zero border of nb pixels; good = 1 where the pixel passes the grown mask (grow[bit] as rip_stage_build_mask, host array)
   of the dq plane trimmed by nb (maskhandling.PixelMask1.build on the L2 file's dq), 0 elsewhere and in the border. */
int rip_stats_l2_pack(rip_ctx *ctx, const float *slope, const float *err_read, const float *err_poisson,
                      const uint32_t *pixeldq, int ny, int nx, int nb, const uint8_t grow[32], float *image, float *err,
                      uint8_t *good);

/* :78-101  the eight output planes for rows [y0, y0+nrows) of the (ny,nx) frame from stacks (nseeds,nrows,nx) holding every
   realisation in order; out (8,nrows,nx) f32 = ideal, median(diffs), median(images), N, mean, std, mean - ideal,
   median(err); N = mean = std = 0 in the border, mean = std = -1000 where N = 0 (:87).  alias_err != 0 reproduces the
   reference as written: its `images` and `err` stacks are memory maps of the same file (:58-59), so plane 2 equals
   plane 7.  ideal (nrows,nx) f32. */
int rip_stats_reduce(rip_ctx *ctx, int nseeds, const float *diffs, const float *images, const float *errs, const uint8_t *good,
                     const float *ideal, int y0, int nrows, int ny, int nx, int nb, int alias_err, float *out);

/* ---- measurement -------------------------------------------------------------------------- */
/* When enabled, rip_calibrate brackets each kernel group with HIP events on the ctx stream.
   rip_profile_read synchronises and returns the summed device time (ms) since the last read:
   out_ms[0] reference-pixel pre-pass, [1] cube stage (refpix apply + bias + linearity),
   [2] IPC, [3] ramp fit + finish; *ncalls = number of rip_calibrate calls summed. */
int rip_profile_enable(rip_ctx *ctx, int on);
int rip_profile_read(rip_ctx *ctx, double out_ms[4], int *ncalls);

/* ---- options of a context ---------------------------------------------------------------------
   One table in the library (csrc/api.hip) holds every option's name, default and accepted range; the calls below all read it.
   Results are identical whatever the integer options hold (chain_dbg excepted): they exist for A/B timing and tests.
   A value outside [lo, hi], or an unknown name, is RIP_EINVAL and changes nothing.  "any" = every int is taken, 0 = off.
     name            default  range         meaning
     "fused"            1     any           the chain as one fused kernel where the configuration allows it (complete chain on a u16 cube; f32 gain; 4, 9 or 11 Legendre planes; 5 to 16 groups; mergeable flag words); 0 = the stage-by-stage kernels
     "chain2"           1     any           the fused kernel (chain2_kernel.h: f32 or f64 ipc4d, 5 to 16 groups); 0 = the stage kernels where it would run
     "chain_quad"       1     any           a last strip of at most 64 live columns goes to workgroups whose 64-column wave columns take a row range each (4096 x 4096: 504 workgroups of 139 steps, not 510 of 143; timing-neutral, profiles/r04_summary.md)
     "skip_first"       1     any           the fused kernel neither loads nor evaluates group 0 where the result cannot depend on it (an excluded first group that is the single read 0, weight zero in every fit variant, a u16 cube, no corrected cube asked for, no caller's channel lines on the device, a set that passed rip_caldir_first_group_safe; the pre-pass then makes the tables of groups 1 .. G-1 only); rip_last_chain_first_group tells which form ran
     "chain_reserve"    8     0 .. INT_MAX  workgroup slots the 256-column fused kernel's grid leaves free; a negative value is stored as 0
     "prepass_form"    -1     -1 .. 1       how the reference-pixel tables are made: -1 by situation (a pre-pass that overlaps the previous ramp's fused kernel as the nine small launches of refpix.hip, which slip into that kernel's tail; one in front of its own ramp on the same stream as the single launch of refpix_one.hip, 0.068 against 0.094 ms, where it covers the frame: up to 4096 rows, a reference output); 0 = refpix.hip always; 1 = refpix_one.hip wherever it covers the frame
     "prepass_gate"     0     0 .. 1000000  N > 0: an overlapped pre-pass whose predecessor call ran the fused kernel starts behind a one-wave gate that waits, for at most N microseconds, until every workgroup of that launch has started (they count themselves in); 0 = no gate, no counting (measured without a gain, profiles/prepass_gate.txt); rip_last_prepass_gate tells what the last gate did
     "pink_form"       -1     any           the complex-to-real transform of the 1/f frames: the library's own two-pass transform for power-of-two lengths (2^8 .. 2^21 points; csrc/pink_fft.h) and hipFFT otherwise; 0 = hipFFT for every length
     "overlap"         -1     -1 .. 1       the reference-pixel pre-pass of a ramp on a second stream beside the previous ramp's fused kernel: -1 by situation (wherever that kernel leaves room on the CUs: every form except the f64-ipc4d one of 5 to 8 groups, whose partial coefficient ring fills the LDS), 0 never, 1 always; a context without a second stream never overlaps
     "chain_dbg"        0     any           timing builds only: the fused kernel skips phases, results invalid
     "guard_band"    1e-5     0 .. INFINITY (f64: the _f64 calls, and only they, take it) relative half-width of the band around the jump threshold inside which the significance is re-evaluated in the reference's exact operation order; INFINITY = always exact.  It is the stage kernels' band (the fused kernel derives its own and takes only INFINITY from here).  The default 1e-5 is tested, not proven: the flags are the reference's on every ramp tried, those made to sit at the threshold included (tests/test_gpu_jump_band.py), but the bound plan.hip derives per difference (RipDiff::relerr) reaches 2.7e-5, and at 1e-6 an emulation of the stage kernel's f32 path gives wrong flags on such ramps of 16 and more groups (profiles/jump_band.txt) */
int rip_set_option(rip_ctx *ctx, const char *name, int value);
int rip_set_option_f64(rip_ctx *ctx, const char *name, double value);
/* the value as it was set (what rip_set_option stored: "overlap" reads -1, 0 or 1 whatever the context can do) */
int rip_get_option(rip_ctx *ctx, const char *name, int *value);
int rip_get_option_f64(rip_ctx *ctx, const char *name, double *value);
/* every option, the f64 one included, back to its default: the state of a new context */
int rip_reset_options(rip_ctx *ctx);
/* row `index` of the table: 1 for an integer option, 2 for the f64 one (def / lo / hi then hold its values cut to int: the
   default reads 0), 0 past the last row.  Any of the four pointers may be NULL.  Needs no context and no GPU. */
int rip_option_info(int index, const char **name, int *def, int *lo, int *hi);

/* how the last rip_calibrate ran: 0 = stage kernels, 2 = the fused kernel (1 and 3 were the general and the wave-private fused
   kernels of rounds 1-2) */
int rip_last_chain_form(rip_ctx *ctx);
/* 1: the fused launch of the last rip_calibrate skipped group 0 (option "skip_first"); 0: it did not, or the stage kernels ran */
int rip_last_chain_first_group(rip_ctx *ctx);
/* 1: the fused launch of the last rip_calibrate streamed the biascorr planes; 0: it ran without that stream (the set has no bias
   correction to make -- rip_caldir_bias_state -- or the stage mask left RIP_STAGE_BIAS out), or the stage kernels ran */
int rip_last_chain_bias_stream(rip_ctx *ctx);
/* the gate in front of the overlapped pre-pass of the last rip_calibrate (option "prepass_gate"): 0 = none was queued, 1 = the
   counter released it, 2 = it gave up at its bound; *giveups (may be NULL) receives the give-ups of all gates of this context so
   far.  Waits for the context's streams.  Negative: an error code. */
int rip_last_prepass_gate(rip_ctx *ctx, int *giveups);

/* Is a fused-kernel form compiled for a complete chain with this many Legendre planes, groups and these ipc4d / gain dtypes
   (RIP_F32 / RIP_F64)?  2 = yes (the value rip_last_chain_form reports), 0 = such a ramp takes the stage kernels.  Needs no
   context and no GPU.  What it does not know: the plan (a difference mask other than the full one takes the stage kernels), the
   CALDIR set (flag words that cannot be merged do too), the call (a sub-chain, an f32 cube, "fused" / "chain2" switched off). */
int rip_chain_form_for(int lin_nplanes, int ngroups, int ipc_dtype, int gain_dtype);

/* The launch geometry the fused kernel takes for such a ramp on a frame of ny rows and nx columns, on a device of ncu compute
   units, with the options "chain_reserve" = reserve and "chain_quad" = quad_ok -- computed by the launcher's own code, on the
   host: needs no context and no GPU.  Returns 0 where rip_chain_form_for does (or for a frame the chain does not take: ny < 16,
   nx not a multiple of 128), else 2 and
     out[0] columns of a workgroup's window (256 or 384)     out[1] column strips (pitch out[0] - 4)
     out[2] columns of the last strip's window inside the frame (nx - (out[1] - 1) * (out[0] - 4))
     out[3] row ranges of every full-width strip             out[4] rows of such a range
     out[5] quad workgroups covering the last strip, 0 = uniform grid (the last strip like every other: out[3] ranges)
     out[6] rows of the range of ONE 64-column wave column of a quad workgroup (out[0] / 64 of them each), 0 = uniform grid
     out[7] grid size: out[3] * (out[1] - 1) + out[5] in quad mode, out[3] * out[1] in the uniform grid.
   Row range i starts at row i * rows; ranges that start at or beyond ny are empty, the last non-empty one may be short.
   The result depends on the group count and the ipc4d dtype only through the form (5-8 / 9-16 groups, f32 / f64). */
int rip_chain_geometry_for(int lin_nplanes, int ngroups, int ipc_dtype, int gain_dtype, int ny, int nx, int ncu, int reserve,
                           int quad_ok, int out[8]);
/* the geometry (as above) of the fused launch of the last rip_calibrate on this context; zeros when it ran the stage kernels */
int rip_last_chain_geometry(rip_ctx *ctx, int out[8]);

/* pseudo-Poisson noise layers ("O" directives, gen_noise_image.py:173-240): per element of I (n doubles) the
   member of the Pearson family with the moments tilnu_21 I, tilnu_31 I, 3 tilnu_21^2 I^2 + tilnu_41 I, replacing
   L1_to_L2/GalPoisson/draw_with_tilnus.py:draw_from_Pearson (:12-135) and the solvers / samplers it calls.
   types  (n int32, or NULL): 0 = outside the admissible region (deviate 0), 1, 3, 4, 5, 6 = Pearson type;
   params (4 n doubles, or NULL): type 1: a, b, mean, c; 3: shape, scale, shift, sign; 4: m, nu, a, lambda; 5: a, b, mu, sign;
          6: alpha, beta, scale, shift -- the reference's formulas in f64 (pinned by goldens);
   draws  (n doubles, or NULL): one deviate each from a counter-based generator keyed by (seed, stream, element); the
          reference's scipy / numpy streams cannot be reproduced: parity of the random part unpinned (moments tested).
   I, draws, types and params are host arrays or device pointers. */
int rip_stage_pearson(rip_ctx *ctx, size_t n, const double *I, double tilnu21, double tilnu31, double tilnu41, uint64_t seed,
                      uint32_t stream, double *draws, int32_t *types, double *params);

/* ---- Level-1 synthesis -- DEVICE pointers, asynchronous on the context's stream ------------------ */
/* The per-pixel work of from_sim/sim_to_isim.py that turns an electron-count image into a raw exposure: make_l1_fullcal
   (:163-262, with the loop of romanisim.l1.apportion_counts_to_resultants it calls), fill_in_refdata_and_1f (:306-403) and the
   EXTRACT_REF block (:711-730).  Calibration arrays as the CALDIR files hold them, resident in HBM: */
typedef struct rip_synth_cal {
    int32_t ny, nx, nb;        /* full frame and its reference-pixel border; active region (ny-2nb, nx-2nb)             */
    int32_t channelwidth;      /* columns per readout channel (nx / channelwidth channels: 32 of 128 on a full frame);   */
                               /* the reference output has one channel's width                                           */
    int32_t nplanes;           /* Legendre planes of the linearity file, 2..17                                          */
    int32_t gain_dtype;        /* RIP_F32 or RIP_F64                                                                     */
    int32_t ipc_dtype;         /* RIP_F32 or RIP_F64                                                                     */
    int32_t amp33_valid;       /* read file has a valid amp33 block (med, std, M_PINK, RU_PINK)                          */
    const void *gain;          /* (ny,nx)                                                                               */
    const float *read_noise;   /* read file "data" (ny,nx)                                                              */
    const float *resetnoise;   /* read file "resetnoise" (ny,nx)                                                        */
    const float *dark_slope;   /* dark file "dark_slope" (ny,nx)                                                        */
    const float *dark;         /* the LAST ngrp planes of the dark file's "data": (ngrp,ny,nx)                          */
    const float *lin_coefs;    /* (nplanes,ny,nx)                                                                       */
    const float *smin, *smax;  /* (ny,nx)                                                                               */
    const void *ipc4d;         /* (3,3,ny-2nb,nx-2nb), or NULL: no IPC (IL(..., ipc_file=None))                          */
    const float *biascorr;     /* the last ngrp planes of the biascorr file's "data": (ngrp,ny-2nb,nx-2nb), or NULL      */
    double tbias;              /* biascorr "t0" (used only with biascorr)                                               */
    const float *amp33_med, *amp33_std;   /* (ny,channelwidth), or NULL                                                 */
    double m_pink, ru_pink;    /* amp33 "M_PINK", "RU_PINK"                                                             */
    double u_pink, c_pink;     /* read file anc "U_PINK", "C_PINK"                                                      */
} rip_synth_cal;

/* romanisim.l1.apportion_counts_to_resultants, the sampling part (dependency absent from the reference tree: published
   algorithm restated, oracle/l1sim.py): read r takes Binomial(counts - collected so far, (t_r - t_{r-1}) / (t_last - t_{r-1}))
   electrons; reads_e (nreads,nya,nxa) i32 = electrons collected up to each read, so reads_e[nreads-1] == counts.  counts
   (nya,nxa) f32 holds integers, or -- poisson != 0 -- the MEAN, of which a Poisson deviate is drawn first (what
   Image2D.simulate :660-662 adds before it calls make_l1_fullcal).  t_reads: nreads times, HOST array, ascending.
   Deviates from the device generator (Philox; inversion / BTRS binomial, inversion / PTRS Poisson) keyed by (seed, read,
   pixel).  The distribution is what is reproduced, not romanisim's numpy stream.  Poisson means below 10 per read are inverted
   in f32 against a 23-bit uniform: the count lies within 64 * 2^-24 in probability of the f64 quantile, and at the largest
   uniforms, where the f32 sum of the probabilities saturates, the search ends at the count whose term no longer moves the sum
   (tests/test_gpu_synth_deviates.py: never beyond the quantile of 1 - 2^-32 at 160 means of 0.05 .. 9.99).  Asynchronous like the other rip_synth_*
   entries when t_reads equals those of the previous call (the device copy of the share table is kept); a NEW table first
   waits for the work queued on the stream. */
int rip_synth_apportion(rip_ctx *ctx, const float *counts, int nya, int nxa, int poisson, int nreads, const double *t_reads,
                        uint64_t seed, int32_t *reads_e);

/* make_l1_fullcal :203-260 after the sampling: reset noise in electrons (normal * resetnoise * gain - t0 * dark_slope / gain),
   per read IL.apply(electrons + reset, electrons=True) (ipc_linearity.py:461-513: i32 + f32 -> f64, ipc_fwd, / gain, 24
   bisection steps of invlinearity in f64), resultant = f32 mean of its reads, + normal * read_noise / sqrt(reads), + biascorr,
   rounded half to even.  group_count: HOST array, reads per resultant (sum = the number of planes of reads_e).
   normals_reset (nya,nxa) f32 and normals_read (ngrp,nya,nxa) f32 standard normal deviates, or NULL: device generator (seed).
   Outputs, each optional: start_e (nya,nxa) f32 the reset-noise image; resultants (ngrp,nya,nxa) f32; cube (ngrp,ny,nx) u16 --
   the resultants clipped to 0..65535 inside a zero border (what romanisim.l1.make_asdf builds around them).
   Exact given the deviates (goldens from the reference's function). */
int rip_synth_resultants(rip_ctx *ctx, const rip_synth_cal *cal, int ngrp, const int32_t *group_count, const int32_t *reads_e,
                         const float *normals_reset, const float *normals_read, uint64_t seed, float *start_e,
                         float *resultants, uint16_t *cube);

/* fill_in_refdata_and_1f :306-403, in place on cube (ngrp,ny,nx) u16 and amp33 (ngrp,ny,channelwidth) u16 (or NULL: no
   reference output): reference pixels = normal * read / sqrt(reads) + normal * resetnoise + dark, active pixels kept, every
   pixel + (1/f frame of its channel * U_PINK + common frame * C_PINK) / sqrt(reads) with odd channels mirrored, rounded and
   clipped to u16; amp33 = med + (normal * std + RU_PINK * frame + M_PINK * common) / sqrt(reads), cast.  banding == 0 skips
   the correlated noise (fill_in_banding=False; amp33 is then left untouched, as in the reference).
   normals (ngrp+1,ny,nx) f32, frames (ngrp,nch+2,ny,channelwidth) f32 in the reference's draw order per group (common, channels
   0..nch-1, reference output; nch = nx / channelwidth) and white33 (ngrp,ny,channelwidth) f32, or NULL each: device generators (seed; frames as
   rip_stage_noise_1f makes them).  Exact given the deviates (goldens from the reference's function). */
int rip_synth_fill(rip_ctx *ctx, const rip_synth_cal *cal, int ngrp, const int32_t *group_count, int banding, const float *normals,
                   const float *frames, const float *white33, uint64_t seed, uint16_t *cube, uint16_t *amp33);

/* rip_stage_noise_1f with the frames left on the device: out (nframes,rows,width) f32 DEVICE memory. */
int rip_synth_noise_1f(rip_ctx *ctx, int rows, int width, int nframes, uint64_t seed, uint32_t stream_id, float *out);
/* The 1/f frames of the NEXT rip_synth_fill(frames = NULL, banding != 0, the same seed and geometry: rows = ny, width =
   channelwidth, nframes = ngrp * (nx / channelwidth + 2)) made AHEAD on the context's second stream, so that the Fourier
   transforms (HBM-bound) run beside the inverse-linearity kernel (arithmetic-bound) queued on rip_stream() between this call
   and the fill: same frames, same bits.  They start behind whatever rip_stream() holds at the time of the call -- call it AFTER
   rip_synth_apportion (HBM-bound too) and before rip_synth_resultants.  The fill waits for them; a fill with another seed or
   geometry, or any other 1/f call, waits too and makes its own.  No-op without a second stream. */
int rip_synth_frames_ahead(rip_ctx *ctx, int rows, int width, int nframes, uint64_t seed);

/* EXTRACT_REF (:711-730) on n-element planes: reference_read = data[0]; data[k] = clip(i32(data[k]) - (i32(data[0]) -
   offset), 0, 65535) for k = 1..ngrp-1, in place (the caller drops plane 0).  Used for the cube and for amp33.  Exact. */
int rip_synth_extract_ref(rip_ctx *ctx, uint16_t *data, int ngrp, size_t n, int offset, uint16_t *reference_read);

/* The inverse of EXTRACT_REF, what romancal's dq-init does to such an exposure before calibrateimage sees it (gen_cal_image.py:
   117-118; its source is not in the reference tree: PARITY UNPINNED): per pixel and stored resultant
   v = i32(data[k]) + i32(reference_read) - offset, out[k] = clip(v, 0, 65535), k = 0..ngrp-1; *n_out_of_range = the number of
   samples the clip changed (0 for everything the encoder made of u16 data: where it did not clip v is the original sample,
   where it clipped v stays inside 0..65535).  data, out (ngrp,n) u16, reference_read (n) u16; out may equal data (in place).
   Used for the cube (n = ny * nx) and for amp33 (n = ny * 128, reference_amp33).  `location` holds for all four pointers:
   RIP_HOST: staged through HBM, complete on return; RIP_DEVICE: asynchronous on the context's stream, n_out_of_range is one
   device word that the entry zeroes first.
   RIP_EINVAL, before anything is copied or launched: a NULL pointer, ngrp < 1, n < 1, |offset| > 2^30, an unknown location,
   out overlapping data without being equal to it.  Exact. */
int rip_stage_decode_reference_read(rip_ctx *ctx, const uint16_t *data, int ngrp, size_t n, const uint16_t *reference_read,
                                    int offset, int location, uint16_t *out, uint64_t *n_out_of_range);

/* A FITS data unit from native samples (what astropy's writeto does to the arrays of gen_cal_image.py:725-736, gen_noise_image.py:
   387-391, maskhandling.py:145-149): src holds n little-endian samples of |bitpix| / 8 bytes, bitpix one of 8, 16, 32, -32, -64;
   dst receives n * |bitpix| / 8 bytes in FITS storage order, the bytes of each sample reversed.  flip_sign != 0 (bitpix 8, 16, 32
   only) also inverts the most significant bit of each sample: the BZERO convention of uint16 (BZERO 32768), uint32 (2147483648)
   and int8 (-128).  mask (NULL, or with bitpix -32 one byte per sample, living where src lives): sample i is replaced by `fill`
   where (mask[i] != 0) == (mask_sense != 0), before the reversal -- where(mask, fill, data) with sense 1, where(good, data, fill)
   with sense 0.  src_location and dst_location are independent (RIP_HOST / RIP_DEVICE): a host side goes through a scoped
   device buffer and the call is complete on return; with both on the device it is asynchronous on rip_stream().  dst may equal
   src (in place, same location).
   RIP_EINVAL, before anything is copied or launched: an unknown bitpix, flip_sign with a float bitpix, mask with a bitpix other
   than -32, n == 0, NULL src or dst, an unknown location, dst overlapping src without being equal to it, dst overlapping mask,
   a DEVICE pointer that is not aligned to the sample (device memory is used where it is).  Exact. */
int rip_stage_fits_encode(rip_ctx *ctx, const void *src, int bitpix, int flip_sign, size_t n, int src_location,
                          const uint8_t *mask, int mask_sense, float fill, void *dst, int dst_location);

/* The planes of the L2 tree from the chain's results (gen_cal_image.py:653-662 with romanisim's make_asdf, oututils.py:52-55,
   typefix.py:38-56): slope, err_read, err_poisson f32 and pixeldq u32 are (ny,nx) frames; over the active region (ny-2nb,
   nx-2nb)   data = slope,  dq = pixeldq,  var_rnoise = err_read * err_read,  var_poisson = err_poisson * err_poisson (f32
   products),  err = sqrt(var_rnoise + var_poisson) (f32 sum, correctly rounded f32 square root).  var_dtype RIP_F32: the three
   are stored as computed; RIP_F16: each f32 value is then rounded to nearest-even float16 (numpy's astype(float16): overflow to
   infinity, float16 subnormals kept, NaN stays NaN).  The flag strips are full rows and columns of pixeldq, corners in both:
   dq_left (ny,nb) = pixeldq[:, :nb], dq_right (ny,nb) = pixeldq[:, nx-nb:], dq_top (nb,nx) = pixeldq[ny-nb:, :], dq_bottom (nb,nx)
   = pixeldq[:nb, :] (empty with nb = 0).  Any output may be NULL and is then not made.  `location` holds for every pointer:
   RIP_HOST: through scoped device buffers, complete on return; RIP_DEVICE: asynchronous on rip_stream().
   RIP_EINVAL, before anything is copied or launched: a NULL input, ny or nx < 1, nb < 0, 2 nb >= ny or 2 nb >= nx, a var_dtype
   other than RIP_F32 / RIP_F16, an unknown location, a DEVICE pointer that is not aligned to its element, an output overlapping
   an input.  Exact. */
int rip_stage_l2_planes(rip_ctx *ctx, const float *slope, const float *err_read, const float *err_poisson, const uint32_t *pixeldq,
                        int ny, int nx, int nb, int var_dtype, int location, float *data, uint32_t *dq, void *var_rnoise,
                        void *var_poisson, void *err, uint32_t *dq_left, uint32_t *dq_right, uint32_t *dq_top, uint32_t *dq_bottom);

/* The reference-pixel strips of a Level-1 cube (oututils.py:46-49): cube (ngrp,ny,nx) of cube_dtype RIP_U16 or RIP_F32; as f32
   left (ngrp,ny,nb) = cube[:, :, :nb], right (ngrp,ny,nb) = cube[:, :, nx-nb:], top (ngrp,nb,nx) = cube[:, ny-nb:, :], bottom
   (ngrp,nb,nx) = cube[:, :nb, :] (empty with nb = 0; f32 samples are moved as bits).  Any output may be NULL.  `location` as for
   rip_stage_l2_planes.
   RIP_EINVAL, before anything is copied or launched: a NULL cube, ngrp, ny or nx < 1, nb < 0, nb > ny or nb > nx, a cube_dtype
   other than RIP_U16 / RIP_F32, an unknown location, a DEVICE pointer that is not aligned to its element, an output overlapping
   the cube.  Exact. */
int rip_stage_l2_refpix_strips(rip_ctx *ctx, const void *cube, int cube_dtype, int ngrp, int ny, int nx, int nb, int location,
                               float *left, float *right, float *top, float *bottom);

/* Cosmic-ray hits (the model of romanisim's cr module, restated in DESIGN.md 7: romanisim is absent from the reference tree, so
   parity is unpinned and every constant is a parameter).  Defaults in brackets. */
typedef struct rip_cr_params {
    double flux, area;               /* tracks per cm^2 and second [8], detector area in cm^2 [16.8]                         */
    double conversion_factor;        /* eV per electron as romanisim names it [0.5]: electrons per pixel length =            */
                                     /* dEdx * pixel_size / conversion_factor                                                */
    double pixel_size, pixel_depth;  /* micrometres [10, 5]                                                                  */
    double min_dedx, max_dedx;       /* range of the energy loss in eV per micrometre [10, 10000]                            */
    double moyal_location, moyal_scale;   /* its Moyal density exp(-(s + exp(-s)) / 2), s = (x - location) / scale [120, 50] */
    double min_len, max_len;         /* range of the track length in micrometres [10, 2000]                                  */
    double len_slope;                /* its density x ** slope [-4.33]                                                       */
    int32_t grid_size, _pad;         /* points of the two tabulated CDFs [10000]                                             */
} rip_cr_params;

/* The tracks of an exposure.  Read r of nreads has Poisson(flux * area * read_time) of them; each starts at (u1 nya, u2 nxa) in
   (row, column) pixel coordinates, points along phi = 2 pi u3 and has length F_len^-1(u4) and energy loss F_dEdx^-1(u5), F^-1
   the linear interpolation scipy.interpolate.interp1d(c, x) evaluates on x = linspace(lo, hi, grid_size), c = cumsum(pdf(x)) -
   pdf(x[0]), c /= max(c): the tables are made on the host in f64 and kept in the context until a parameter that shapes them
   changes (new tables first wait for the work queued on the stream).
   tracks (capacity,6) f64 rows = read index, i0, j0, phi, length, dEdx; offsets (nreads+1) i32 = first row of each read,
   offsets[nreads] = number of rows, clamped to capacity (rows past it are lost: size it for the mean plus ten sigma).
   counts (nreads) i32 or NULL: device Poisson deviates; uniforms (capacity,5) f64 in [0,1) or NULL: device generator (Philox
   under tags of its own).  Exact given counts and uniforms up to the host's exp / pow in the tables. */
int rip_synth_cr_tracks(rip_ctx *ctx, const rip_cr_params *params, int nreads, double read_time, int nya, int nxa, uint64_t seed,
                        const int32_t *counts, const double *uniforms, int capacity, double *tracks, int32_t *offsets);

/* The deposits of the rows offsets[0] .. offsets[nreads]-1 of tracks, in place on reads_e (nreads,nya,nxa) i32 (the output of
   the apportioning).  A track ends at (clip(i0 + l cos phi, -0.5, nya + 0.5), clip(j0 + l sin phi, -0.5, nxa + 0.5)), l = length /
   pixel_size; pixel (i,j) is the square [i-0.5,i+0.5) x [j-0.5,j+0.5).  Every pixel of the image that holds a part of the track
   of length l2 (parts shorter than 1e-10 pixels do not count; a track without such a part deposits once, with its whole length,
   in the pixel of its middle) receives k ~ Poisson(lambda) electrons, lambda = dEdx * pixel_size / conversion_factor *
   sqrt((pixel_depth / pixel_size)^2 + l2^2), in the read of its row and every later one (poisson == 0: k = rint(lambda)).
   first_read (nya,nxa) i32 is WRITTEN by the call: the first read in which a track crossed the pixel, nreads where none did.
   lam (nya,nxa) f64 or NULL: the sum of lambda per pixel.  Integer adds commute: the same tracks and seed give the same
   reads_e on every run.  The walk of a track stops after nya + nxa + 2 boundary crossings. */
int rip_synth_cr_deposit(rip_ctx *ctx, const rip_cr_params *params, int nreads, int nya, int nxa, const double *tracks,
                         const int32_t *offsets, int poisson, uint64_t seed, int32_t *reads_e, int32_t *first_read, double *lam);

/* ---- calibration-file derivation ----------------------------------------------------------- */
/* What runs/2026_July/postprocess_calfiles.py and makemask.py of the reference compute from a linearitylegendre / dark / gain
   set.  The array arguments of these four entries are host arrays or device pointers; READS, LPX, LPY and coef are host arrays.
   Every input plane is a full (ny,nx) frame.  Exact: the reference's numpy operations in its order and dtypes (numpy >= 2). */

/* biascorr (postprocess_calfiles.py:103-140).  reads[2 ngrp]: group j holds the reads reads[2j] .. reads[2j+1]-1 (groups need be
   neither contiguous nor sorted).  xref = (reads[2 bframe] + reads[2 bframe + 1] - 1) / 2; dark = f32(dark_slope * f32(tframe));
   per active pixel and group, pred_j = f32(sum over the group's reads x, in read order, of invlinearity(f32(dark * f32(x - xref))))
   / f32(number of reads), the inverse linearity in f32 as rip_stage_invlinearity evaluates it on coefs (nplanes,ny,nx), smin,
   smax at the pixel; biascorr_j = dark_data_j - pred_j.  dark_data (ngrp_dark,ny,nx); biascorr and pred (NULL: not wanted) are
   (ngrp, ny-2nb, nx-2nb) f32; t0 (NULL: not wanted) receives tframe * xref.
   RIP_EINVAL, before anything is launched: ngrp outside 1..RIP_MAX_GROUPS, a group with reads[2j+1] <= reads[2j] (or more than
   65536 reads), bframe outside [0, ngrp), ngrp != ngrp_dark, a border that leaves no active pixel, nplanes outside 2..17. */
int rip_cal_biascorr(rip_ctx *ctx, const float *dark_slope, const float *dark_data, int ngrp_dark, int ny, int nx, int nb, int nplanes,
                     const float *coefs, const float *smin, const float *smax, const int32_t *reads, int ngrp, double tframe, int bframe,
                     float *biascorr, float *pred, double *t0);

/* pflat (postprocess_calfiles.py:22-40) from the raw p-flat plane: p = f32(p / f32(model)), the medfit model evaluated as
   rip_stage_legendre2d does from LPX (order+1,nx), LPY (order+1,ny), coef (sky.medfit rounds it to the plane's dtype, :191);
   p = f32(p * scale), scale = f32(g_ideal / median(gain)) from the caller; dq = 1 where p < 0.01 or p > 1.99 (f32 compares);
   data = clip(p, 0.01, 1.99) (NaN stays).  data f32, dq u32, (ny,nx). */
int rip_cal_pflat(rip_ctx *ctx, const float *pflat, int ny, int nx, int order, const double *LPX, const double *LPY, const double *coef,
                  float scale, float *data, uint32_t *dq);

/* saturation (postprocess_calfiles.py:69-97): data = f32(clip(Smax, 1, 65535)) - 1, dq = 0 where Smax > Sref, else 1. */
int rip_cal_saturation(rip_ctx *ctx, const float *smax, const float *sref, int ny, int nx, float *data, uint32_t *dq);

/* mask (makemask.py:12-36): REFERENCE_PIXEL on the nb border rows and columns | lin_dq | LOW_QE where pflat0 / pflat_median
   < 0.5 (f32; pflat_median = np.median of the plane, from the caller) | HOT where dark_slope > 12.5, else WARM where > 0.25
   | gain_dq. */
int rip_cal_mask(rip_ctx *ctx, int ny, int nx, int nb, const uint32_t *lin_dq, const float *pflat0, float pflat_median,
                 const float *dark_slope, const uint32_t *gain_dq, uint32_t *dq);

/* ---- dark and read-noise files ------------------------------------------------------------- */
/* What runs/2026_July/make_dark_file.py of the reference computes from a set of dark exposures and a noise summary.  The ARRAY
   arguments of these three entries live where `location` says: RIP_HOST (staged through HBM by the call) or RIP_DEVICE (used
   where they are); READS is a host array.  The calls return when their kernels are done. */

/* Group means of one dark exposure (make_dark_file.py:55-71) into slot j of a stack of such means.  cube (nreads,ny_file,nx_file)
   u16; the rows y0 .. y0+ny-1 and the columns 0 .. nx-1 of it are used.  reads[2 ng] as for rip_cal_biascorr.  stack
   (ng,cap,ny,nx) f32, ALWAYS a device pointer: stack[g][j] = np.mean(cube[a:b].astype(f32), axis=0), i.e. the f32 sum of the
   reads a .. b-1 in read order, divided once in f32 by f32(b - a).  fits_be16 != 0: the samples are FITS storage (big-endian
   int16, BZERO = 32768), un-swapped and offset by the kernel.  The cube is read once for all groups.
   RIP_EINVAL, before anything is launched or copied: ng outside 1..RIP_MAX_GROUPS, a group with reads[2g+1] <= reads[2g], a
   group that starts below 0 or ends beyond nreads, j outside [0, cap), nx > nx_file, rows outside the frame. */
int rip_cal_group_means(rip_ctx *ctx, const uint16_t *cube, int location, int nreads, int ny_file, int nx_file, int y0, int ny, int nx,
                        const int32_t *reads, int ng, int fits_be16, float *stack, int cap, int j);

/* mean[p] = np.nanmean(sigma_clip(stack[:, p], sigma, maxiters, cenfunc='median', stdfunc='std', masked=False)) over the n planes
   stack[s * plane_stride + p] (f32; plane_stride >= npix, in elements), count[p] (i32, NULL: not wanted) the number of values
   kept.  astropy is not available to this project: the rule below IS the specification, parity with astropy is unpinned.
   Per pixel: non-finite values are excluded from the start.  Up to maxiters times, over the survivors: c = median (0.5 * (a + b)
   of the two middle values for an even count), m = mean, s = sqrt(sum((x - m)^2) / count), all three in f64; lo = c -
   sigma_lower * s, hi = c + sigma_upper * s; a value is removed when (double)x < lo or (double)x > hi (strict: a constant column
   keeps everything); stop when nothing was removed.  Result: the f64 sum of the survivors in plane order, divided by their
   count in f64, rounded once to f32; NaN and count 0 where nothing survives.  The f64 sums behind m and s are taken in a
   fixed order (not plane order): the result is the same on every run.
   RIP_EINVAL: n outside 1..512, maxiters outside 0..16, a sigma that is negative or not finite, plane_stride < npix. */
int rip_cal_sigma_clip_mean(rip_ctx *ctx, const float *stack, int location, int n, size_t plane_stride, size_t npix, double sigma_lower,
                            double sigma_upper, int maxiters, float *mean, int32_t *count);

/* dark_slope = where(dark2 > 200, dark1, dark2), dark_slope_err likewise from the error planes (make_dark_file.py:79-85), and
   read_noise = f32(f64(cds) / sqrt(2)) (:157; numpy >= 2 divides a float32 array by the float64 scalar np.sqrt(2) in float64).
   The five inputs are f32 planes of ny rows of row_stride floats (the [:, :nside] crop of wider frames), the outputs (ny,nx). */
int rip_cal_dark_planes(rip_ctx *ctx, const float *dark1, const float *dark2, const float *dark1_err, const float *dark2_err,
                        const float *cds, int location, int ny, int nx, size_t row_stride, float *dark_slope, float *dark_slope_err,
                        float *read_noise);

/* ---- gain and ipc4d files ------------------------------------------------------------------ */
/* What runs/2026_July/make_gain_file.py of the reference (the same script in runs/summer2025run) expands from solid-waffle's
   superpixel tables.  means[4][nsy*nsx] (g, aH, aV, aD: the script's meanvals, bad superpixels already filled with the array
   mean) and good[nsy*nsx] (non-zero: at least one summary file has N > 0 there) are HOST arrays; the frame is ny = nsy * ry rows
   of nx = nsx * rx pixels, pixel (Y,X) belongs to superpixel (Y / ry, X / rx).  The four outputs live where `location` says
   (RIP_HOST: filled through a scoped device buffer; RIP_DEVICE: written where they are); each may be NULL (not wanted).
     gain      f32 (ny,nx)   f32(mean_g) of the superpixel, 0.0 on the nb border rows and columns            (:59-68, 88)
     gain_dq   u32 (ny,nx)   0 where the superpixel is good and the pixel is off the border, else 2**19      (:104)
     kernel    (3,3,ny-2nb,nx-2nb) of kernel_dtype.  With a_t(p) = f64(f32(mean_t)) of the superpixel of active pixel p:
               kernel[1+dy][1+dx][p] = (a_t(p) + a_t(p+o)) / 2.0 in f64 for o = (dy,dx) != (0,0) where p+o is an active pixel,
               0.0 where it is not; t = aV for (+-1,0), aH for (0,+-1), aD for the diagonals.  kernel[1][1][p] = 1.0 - S, S the
               f64 sum of the nine planes in row-major order, the centre taken as 0.0.  RIP_F64 is what the script writes
               (:130-175); RIP_F32 is each of those values rounded once.
     kernel_dq u32 (ny-2nb,nx-2nb)   all zero: the script convolves its bad-pixel map with an all-zero kernel (:130, 195)
   All nine kernel planes of a pixel are written by one launch.  The call returns when its kernels and copies are done.
   RIP_EINVAL, before anything is launched or copied: nsy or nsx below 1; superpixels that do not tile the frame (nsy * ry != ny
   or nsx * rx != nx); nb negative or leaving no active pixel; kernel_dtype neither RIP_F32 nor RIP_F64; every output NULL. */
int rip_cal_gain_ipc4d(rip_ctx *ctx, const double *means, const uint8_t *good, int nsy, int nsx, int ny, int nx, int nb, int location,
                       float *gain, uint32_t *gain_dq, void *kernel, int kernel_dtype, uint32_t *kernel_dq);

/* ---- raw detector frames to exposure cubes ------------------------------------------------- */
/* What runs/summer2025run/convert_dark.py, convert_flt.py and convert_loflt.py of the reference do between reading the
   single-frame files of an exposure and writing its cube (line numbers: convert_flt.py).  Both entries return when their kernels
   and copies are done.  Exact: bytes are moved, and the slope arithmetic has no rounding but the script's own two. */

/* One frame into its plane of the cube (:53-63).  frame (ny,nx) 16-bit samples as `stored` says -- 0: native u16; 1: FITS
   storage, big-endian int16 with BZERO 32768 (the unsigned sample: bytes swapped, top bit inverted); 2: FITS storage, big-endian
   int16 without BZERO, its bits kept (numpy's cast to uint16 wraps) -- living where `location` says: RIP_HOST (it goes through a
   scoped device buffer) or RIP_DEVICE (read where it is).  dst: ny * nx u16, ALWAYS a device pointer (plane k of a cube in HBM),
   receives the decoded frame in the science frame: orient 0 as it is; 1 (sca % 3 == 0, :61) the columns 0 .. nflip-1 of every
   row reversed, the columns nflip .. nx-1 (the reference output) in place; 2 (:63) the rows reversed, whole rows moving.
   nflip is looked at with orient 1 only, and checked always.  With nx and nflip multiples of 8 and both pointers 16-byte aligned
   a lane moves 8 samples; otherwise one.  The two forms give the same bytes.
   RIP_EINVAL, before anything is launched or copied: ny or nx < 1, nflip outside 0..nx, an unknown orient, stored or location, a
   NULL pointer, a device pointer that is not aligned to the 2-byte sample, dst overlapping frame. */
int rip_cal_raw_frame(rip_ctx *ctx, const uint16_t *frame, int location, int ny, int nx, int orient, int nflip, int stored,
                      uint16_t *dst);

/* The two unweighted slope images of a cube (:65-79; convert_dark.py:65-76 with nc = n).  cube (n,npix) u16, a DEVICE pointer;
   the planes 1 .. nc-1 are read, each once.  w0[nc], w1[nc] HOST arrays of f64 weights and de0, de1 their denominators, formed by
   the caller as the script forms them (w0[k] = k - nc / 2.0 for k = 1 .. nc-1, w1[k] = k - (nc / 2) / 2.0 for k = 1 .. nc/2 - 1,
   de the running sum of their squares in k order); w0[0] and w1[k] outside 1 .. nc/2 - 1 are not read.  slp (2,npix) f32, where
   out_location says (RIP_HOST: through a scoped device buffer):
     slp[0][p] = f32((sum over k = 1 .. nc-1   of f64(cube[k][p]) * w0[k]) / de0)
     slp[1][p] = f32((sum over k = 1 .. nc/2-1 of f64(cube[k][p]) * w1[k]) / de1)
   Every product and partial sum is a multiple of 0.5 far below 2^53: the numerators are exact in any order and start at +0.0;
   the only roundings are the f64 division and the conversion to f32, so the result is numpy's in every bit.  A denominator of
   zero meets a numerator of zero (nc 1, 2: both images; nc 3, 4, 5: the second): 0 / 0 = NaN, never an infinity.
   RIP_EINVAL, before anything is launched or copied: n or npix < 1, nc outside 1..n, a NULL pointer, an unknown out_location, a
   device pointer that is not aligned to its sample, slp overlapping the cube. */
int rip_cal_frame_slopes(rip_ctx *ctx, const uint16_t *cube, int n, int nc, size_t npix, const double *w0, double de0, const double *w1,
                         double de1, float *slp, int out_location);

/* ---- the linearitylegendre file -------------------------------------------------------------- */
/* The step of the reference's runs/2026_July/make_sca_files_2026Jul.job that calls solid-waffle's linearity_run on the JSON of
   write_linearity_config.pl.  solid-waffle's source is not in the reference tree: the rule below IS the specification, parity
   with solid-waffle is unpinned.  Pinned by the reference are the JSON, the file's schema and what its consumers expect of the
   result: phi(Sref) = 0, dphi/dS(Sref) = 1, pflat[0] the bright flat's rate.  Both calls return when their kernels are done. */

/* One exposure cube added to the per-frame sums of its ramp set.  cube (nreads,ny_file,nx_file) u16 where `location` says
   (RIP_HOST: the frames and rows used are staged through a scoped device buffer); fits_be16 as for rip_cal_group_means.  sums
   (nreads - f0, ny, nx) u32, ALWAYS a device pointer, zeroed by the caller before the first exposure:
     sums[f - f0][y - y0][x] += cube[f][y][x]   for f = f0 .. nreads-1, y = y0 .. y0+ny-1, x = 0 .. nx-1
   count: the number of exposures added so far.  The sums are integers: the result depends on no order and is the same on every
   run.  With nx_file % 8 == 0 and a 16-byte aligned first sample a lane takes 8 pixels (and two 16-byte read-modify-writes of
   sums where nx % 4 == 0 and sums is 16-byte aligned); otherwise one.  The forms give the same words.
   RIP_EINVAL, before anything is launched or copied: count outside 0..65535 (65536 exposures of 65535 still fit in u32), nx >
   nx_file, rows outside the frame, f0 outside [0, nreads), a NULL pointer, an unknown location. */
int rip_cal_frame_sums(rip_ctx *ctx, const uint16_t *cube, int location, int nreads, int ny_file, int nx_file, int y0, int ny, int nx,
                       int f0, int fits_be16, uint32_t *sums, int count);

/* The fit, one lane per pixel.  HOST tables of nsets (1..8) entries: sums[k] the DEVICE pointer of set k's u32 (nframes[k],ny,nx)
   sums, counts[k] its exposures, first[k] the first frame used (TSTART - 1).  sref (ny,nx) f32 and every output are DEVICE
   pointers; the planes hold the rows y0 .. y0+ny-1 of a frame of ny_frame rows (a row band; the whole frame: 0, ny), which only the
   border looks at.  bright: the set that defines the range; dark: the dark set, or -1.  All arithmetic is f64, one rounding per
   operation (no contraction; / and sqrt correctly rounded), in the order of tests/linfit_ref.py; results are rounded once.
   Per pixel, with M_k[i] = sums_k[i] / counts[k] and F_k = nframes[k] - first[k]:
     range    Smin = f32(max(Sref - negativepad, 0)).  On the bright set, i0 = first: D0 = (M[i0+n0] - M[i0]) / n0 with n0 =
              min(4, F-1); the cut c is the first i >= i0 with M[i+1] - M[i] < slopecut * D0, the last frame where there is none;
              Smax = min(M[c], 65535) rounded UP to f32 (the sample at the cut stays in range).  The fit works on these two f32
              values, so that the stored planes are the ones its basis was built on.
     samples  frames first[k] .. of every set with Smin <= M <= Smax, on the bright set only i <= c; a set with fewer than two
              takes no part.
     model    phi(M_k[i]) = a_k + r_k u_i, u_i = 2 (i - first[k]) / (F_k - 1) - 1;  h = (Smax - Smin) / 2, z = (S - Smin) / h - 1,
              phi(S) = (S - Sref) + sum over l = 2..p of q_l B_l(z), B_l(z) = P_l(z) - P_l(z_ref) - P_l'(z_ref) (z - z_ref): the
              two constraints hold by construction.  Unweighted least squares for q, a_k, r_k: [1, u] is projected out per set,
              the (p-1) x (p-1) normal equations are solved by Cholesky, a_k and r_k follow by regression of phi(M) on [1, u].
     data     (p+1,ny,nx) f32, the series in P_l(z): c_l = q_l (l >= 2), c_1 = h - sum q_l P_l'(z_ref),
              c_0 = -h z_ref - sum q_l (P_l(z_ref) - P_l'(z_ref) z_ref)
     smin, smax (ny,nx) f32;  cut (ny,nx) i32: c, a frame index of the bright set's sums
     pflat    (sets but the dark one, in their order; ny,nx) f32: rate_k - rate_dark in DN_lin/s, rate_k = 2 r_k / ((F_k - 1)
              tframe); no subtraction without a dark set or where it took no part; 0 for a set that took no part
     dark_rate (ny,nx) f32: rate_dark (0 without one);  ramperr (nsets,ny,nx) u16: the largest |phi(M) - a_k - r_k u| of the
              set's used samples, rounded up, at most 65535
     dq       (ny,nx) u32: REFERENCE_PIXEL (2^31) on the nb border rows and columns; elsewhere NO_LIN_CORR (2^20) where D0 <= 0,
              Sref is not finite, Sref >= Smax, Smax <= Smin, the degrees of freedom sum (used_k - 2) are below p - 1, or a
              Cholesky pivot is not positive and finite; else 0.  A flagged pixel carries the identity phi = S - Sref -- c_0 =
              (Smin + Smax) / 2 - Sref (the quiet NaN 0x7FC00000 where Sref is not finite, Smin then 0), c_1 = h, the rest 0 --
              and zeros in pflat, dark_rate and ramperr.
   RIP_EINVAL, before anything is launched, naming the key of the JSON: P_ORDER outside 1..10, SIGN other than 1, SLOPECUT
   outside (0, 1), more than 8 sets in RAMPS, DARK or the bright set outside the sets (or the same set), a TSTART that leaves
   fewer than 2 frames, NRAMP outside 1..65536, TFRAME not positive, NEGATIVEPAD negative, rows outside the frame, a NULL pointer. */
int rip_cal_linearity_fit(rip_ctx *ctx, int nsets, const uint32_t **sums, const int32_t *counts, const int32_t *first,
                          const int32_t *nframes, const float *sref, int ny, int nx, int y0, int ny_frame, int nb, int p_order, int sign, double tframe,
                          double slopecut, double negativepad, int bright, int dark, float *data, float *smin, float *smax, uint32_t *dq,
                          float *pflat, float *dark_rate, uint16_t *ramperr, int32_t *cut);

/* ---- the noise summary of a dark set --------------------------------------------------------- */
/* The step of the reference's runs/2026_July/make_sca_files_2026Jul.job (line 76) that calls solid-waffle's noise_run, whose
   output make_dark_file.py reads.  solid-waffle's source is not in the reference tree: the rule below IS the specification,
   parity with solid-waffle is unpinned.  The noise parameters are defined as the inverse of the reference's own generator
   (from_sim/sim_to_isim.py:306-402) and tested by round trip (calfiles/noisestack.py: noise_params).  The three calls return when
   their kernels are done.
   Geometry: C science channels of cw columns (cw even, at most 256; production 32 x 128), nch = C + 1 channels with ref_out != 0:
   the reference output is the cw columns after the science ones.  Frames used: f0 .. f0+n-1 (-t = f0 + 1, -tn = n). */

/* One dark exposure, read once.  cube (nreads,ny,nx_file) u16 where `location` says (RIP_HOST: the n frames used are staged
   through a scoped device buffer); fits_be16 as for rip_cal_group_means; the columns 0 .. nch*cw-1 are used.  count: the number
   of exposures added so far.  With x_i the sample of frame f0+i, d_i = x_(i+1) - x_i and S = sum_i (2i - (n-1)) x_i, the
   per-pixel accumulators (ny, nch*cw), ALWAYS device pointers, zeroed by the caller before the first exposure, get
     a0 u32 += x_0      a1 u64 += x_0^2     b0 i32 += d_0            b1 u64 += d_0^2
     s0 i64 += S        s1 u64 += S^2       c0 i32 += x_(n-1) - x_0  c1 u64 += sum_i d_i^2
   and m33 (ny,cw) u32 (ref_out only, else NULL) += sum_i x_i of the reference-output columns.  All are integers: the result
   depends on no order.  Nothing wraps for n <= 64 and 512 exposures: |S| <= 65535 n^2 / 2, so 512 S^2 < 2^64.
   rowsum (n,ny,nch,2) u32, a device pointer, is WRITTEN: rowsum[i][y][c][p] = the sum of frame f0+i over the columns of channel c
   (C: the reference output) in row y whose index has parity p.  The lanes of a channel meet in LDS; no atomics.
   A lane takes 8 adjacent pixels (16-byte loads and stores) when nx_file % 8 == 0, cw % 8 == 0 and the first sample and the
   accumulators are 16-byte aligned; otherwise one.  Both forms give the same words.
   RIP_EINVAL, before anything is launched or copied: n outside 2..64, count outside 0..511, f0 + n > nreads (the message names
   -tn), cw odd or above 256, ny < 128, nch * cw > nx_file, a NULL pointer, an unknown location. */
int rip_cal_noise_add(rip_ctx *ctx, const uint16_t *cube, int location, int nreads, int ny, int nx_file, int C, int cw, int ref_out, int f0,
                      int n, int fits_be16, int count, uint32_t *a0, uint64_t *a1, int32_t *b0, uint64_t *b1, int64_t *s0, uint64_t *s1,
                      int32_t *c0, uint64_t *c1, uint32_t *m33, uint32_t *rowsum);

/* The rowsum of one exposure into the f64 moment tables, all DEVICE pointers, zeroed by the caller before the first exposure.
   Scales j = 0 .. J, J = min(6, floor(log2(ny / 64))); scale j has ny >> (j+1) blocks b, and the (j, b) of all scales are laid end
   to end: nbt = sum_j (ny >> (j+1)).  For the CDS pair k = 0 .. n-2: D_k[y][c] = rowsum[k+1][y][c][0] + rowsum[k+1][y][c][1] -
   rowsum[k][y][c][0] - rowsum[k][y][c][1] (i64); H[k][j][b][c] = the sum of D_k over the rows [2b 2^j, (2b+1) 2^j) minus the sum
   over the next 2^j rows (trailing rows are unused); T[k][j][b] = sum over c < C of H; Q[k][c] = the sum over all rows of
   (rowsum[k+1][y][c][0] - rowsum[k][y][c][0]) - (rowsum[k+1][y][c][1] - rowsum[k][y][c][1]).
     h1, h2 (n-1,nbt,nch) += H, H^2     t1, t2 (n-1,nbt) += T, T^2     ht (n-1,nbt) += H[..][C] * T (ref_out only, else NULL)
     q1, q2 (n-1,nch) += Q, Q^2
   Every term is f64(int) * f64(int), one rounding, added with one rounding; every word has one writer and calls come in exposure
   order, so a numpy loop over the exposures gives the same bits.  No atomics.
   RIP_EINVAL: n outside 2..64, ny < 128, C < 1, a NULL pointer. */
int rip_cal_noise_rowstats(rip_ctx *ctx, const uint32_t *rowsum, int n, int ny, int C, int ref_out, double *h1, double *h2, double *t1,
                           double *t2, double *ht, double *q1, double *q2);

/* The per-pixel planes from the accumulators of nexp exposures (device pointers), one lane per pixel in f64, one rounding per
   operation (no contraction; / and sqrt correctly rounded), each result rounded once to f32.  With N = nexp, n_tot = N (n-1),
   var(q, s, m) = (q - s*s/m) / (m - 1) where that is positive, else 0, and nn = n (n^2 - 1):
     planes (6,ny,C*cw) f32:  0 DARK1 = b0 / (N tframe)              1 DARK1ERR = sqrt(var(b1, b0, N) / N) / tframe
                              2 DARK2 = (6 s0) / ((N nn) tframe)      3 DARK2ERR = (6 sqrt(var(s1, s0, N) / N)) / (nn tframe)
                              4 CDS = sqrt(var(c1, c0, n_tot))        5 RESET = sqrt(var(a1, a0, N))
     amp33 (2,ny,cw) f32 (ref_out only, else NULL), from the reference-output columns:  0 = m33 / (N n), the mean sample;
                              1 = f32(f64(CDS) / sqrt(2)), as rip_cal_dark_planes makes read_noise
   DARK1 is the short-baseline rate in DN/s, DARK2 the unweighted least-squares slope of the n frames.  planes and amp33 live where
   `location` says (RIP_HOST: filled through a scoped device buffer).
   RIP_EINVAL: nexp outside 2..512 (a variance over exposures needs two), n outside 2..64, tframe not positive, a NULL pointer, an
   unknown location. */
int rip_cal_noise_planes(rip_ctx *ctx, const uint32_t *a0, const uint64_t *a1, const int32_t *b0, const uint64_t *b1, const int64_t *s0,
                         const uint64_t *s1, const int32_t *c0, const uint64_t *c1, const uint32_t *m33, int nexp, int n, int ny, int C,
                         int cw, int ref_out, double tframe, int location, float *planes, float *amp33);

/* ---- gain and IPC summaries of a flat set --------------------------------------------------- */
/* The device half of the step of the reference's runs/2026_July/make_sca_files_2026Jul.job (lines 48-64) that calls
   solid-waffle's correlation_run (run_ir_all), whose _summary.txt files make_gain_file.py reads.  solid-waffle's source is not
   in the reference tree: the rule below IS the specification, parity with solid-waffle is unpinned.  The host half
   (calfiles/corrstack.py: solve_summary) turns these sums into gain, IPC couplings and non-linearity as the inverse of the
   package's own generator (L1Synth), tested by round trip.

   One pair of exposures.  cube1, cube2 (nreads,ny_file,nx_file) u16, each where its location says (RIP_HOST: only the first ny
   rows of the four frames used are staged through a scoped device buffer); fits_be16 (both cubes) as for rip_cal_group_means.
   fa, fb, fc, fd: 0-based frames (TIME a b c d minus one), fa < fb, fc < fd, fa < fd.  The frame is the first (ny,nx) samples of
   the file's (ny_file,nx_file), nb its border, a superpixel (sy,sx) pixels with ny % sy == 0 and nx % sx == 0, at most 16384
   pixels (128 x 128, NBIN 32 32 on 4096: its differences are held in LDS).
   table int64 [ny/sy][nx/sx][25] where table_location says.  Per superpixel, with S1, S2 the two exposures, cds_i(p,q) = S_i[q] -
   S_i[p] as int32 and e = cds_1(a,d) - cds_2(a,d) on the n0 pixels of the superpixel outside the nb border of the frame:
     q25, q50, q75   the order statistics of those n0 values of e at the 0-based ranks (n0-1)/4, (n0-1)/2, 3(n0-1)/4 (integer
                     division)
     kept            a pixel with |e - q50| * 1349 <= 5000 * (q75 - q25) in 64-bit integers: five robust sigmas
     slot 0, 1, 2    n (kept), sum e, sum e^2 over the kept pixels
     slots 3 .. 18   for the shifts (dy,dx) = (0,1), (1,0), (1,1), (1,-1) in this order four slots each: the count m of pixels p
                     with p and q = p + shift both kept and both inside this superpixel, sum e_p, sum e_q, sum e_p e_q
     slot 19, 20, 21 sum of cds_1(a,b) + cds_2(a,b) over the kept pixels; the same for (c,d); the same for (a,d)
     slots 22 .. 24  q25, q50, q75
   n0 = 0 (a superpixel inside the border) gives 25 zeros.  Integers only: no order of threads changes a bit, and
   tests/corr_ref.py restates every slot with np.sort.
   One workgroup per superpixel: the samples are read once (a lane takes 8 adjacent pixels with 16-byte loads when sx % 8 == 0,
   nx_file % 8 == 0 and every frame used starts on 16 bytes; otherwise one pixel; both forms give the same words; the samples of a
   pixel that is not kept are read a second time), the ranks come from a two-level histogram selection in LDS, the neighbours from
   LDS; the sums meet by wave shuffles and LDS, every slot has one writer, no atomics on the sums.  Returns when its kernel and
   copies are done.
   RIP_EINVAL, before anything is launched or copied: a NULL pointer, an unknown location, a frame of TIME outside the cube or an
   order other than the above (the message names TIME), a frame outside the file, nb negative, sy or sx that do not divide the
   frame or a superpixel above 16384 pixels (the message names NBIN). */
int rip_cal_corr_pair(rip_ctx *ctx, const uint16_t *cube1, int location1, const uint16_t *cube2, int location2, int nreads, int ny_file,
                      int nx_file, int fits_be16, int fa, int fb, int fc, int fd, int ny, int nx, int nb, int sy, int sx, int64_t *table,
                      int table_location);

/* ---- focal-plane overview of a calibration set (utils/fpaplot.py of the reference) ---------- */
#define RIP_FPA_MAX_PLANES 8

/* fpaplot.read_sca_image (:131-141) for up to 8 quantities of one SCA in one launch over the frame: the masked block means.
   dq (nside,nside) u32 where dq_location says, NULL: nothing is masked; grow[32] as rip_stage_build_mask (host array).  The mask
   is grown on the fly from dq (zero padded at the frame edge, the rule of rip_stage_build_mask) and never written to memory; dq
   is read once plus a 2-pixel halo, each plane once.  n1 is a power of two that divides nside; a bin is s x s pixels, s =
   nside / n1, any s from 1 to nside.  The planes come as four HOST tables of nplanes entries: plane i is (sides[i], sides[i])
   elements of dtypes[i] (RIP_F32 or RIP_F64) at planes[i], living where locations[i] says (RIP_HOST: through a scoped device
   buffer; RIP_DEVICE: read where it is).  A plane of side m < nside sits centred in the frame, zeros around it (np.pad(obj,
   (nside - m) // 2)).  out (nplanes,n1,n1) f64 where out_location says:
     out[i][by][bx] = sum / count over the pixels of the bin where the grown mask is 0 and the value is not NaN (padded zeros
     count); NaN where count is 0; +-inf propagate as in numpy (inf + -inf = NaN).
   Sums are f64 in a fixed order without floating-point atomics: two calls give the same bits.  The call returns when its kernels
   and copies are done.
   RIP_EINVAL, before anything is launched or copied: nside < 1; n1 not a power of two or not dividing nside; nplanes outside
   1..8; a NULL plane or out; a dtype that is neither RIP_F32 nor RIP_F64; a plane with side < 1, side > nside or nside - side
   odd; a growth that is not one of 0, 1, 5, 9, 25; an unknown location. */
int rip_fpa_bin(rip_ctx *ctx, const uint32_t *dq, int dq_location, const uint8_t grow[32], int nside, int n1, int nplanes,
                const void **planes, const int *dtypes, const int *sides, const int *locations, double *out, int out_location);

/* fpaplot.make_big_image (:223-275) and multi_image (:345-358): the finished RGB picture in one store-only launch, every byte
   written once by the thread that owns the pixel.  The picture is npanel panels of (ny,nx) pixels, nw abreast with `gap` pixels
   between them; every panel shows the nsca SCAs as n1 x n1 maps.  All positions are the host's, computed with the reference's
   integer arithmetic; the ticks are sc = max(n1, 64) / 64 pixels wide and 2 sc high.
     maps     (npanel,nsca,n1,n1) f64, where maps_location says: the means of rip_fpa_bin
   HOST tables:
     present  (npanel,nsca) u8    0: the SCA's file is absent and it draws as an all-zero map (:114-117)
     sca_pos  (nsca,2) i32        (posy, posx) of the SCA's first pixel in its panel; a later SCA overwrites an earlier one
     vmin, vmax (npanel) f64;  scale (npanel) u8: non-zero draws the colour bar and its three ticks
     table    (256,3) u8          the colour table;  glyphs (256,12,6) u8 or NULL (then nstamps must be 0)
     stamps   (nstamps,6) i32     panel, y, x, size, value, character: one letter of write_text (:150-182), drawn in list order --
              glyph rows reversed, every cell size x size pixels, only where the glyph is > 0, all three channels = value
   Per SCA pixel: v = nan_to_num(mean) (NaN 0, +-inf +-DBL_MAX), x = clip((v - vmin) / (vmax - vmin), 0, 1) in f64, index =
   min(int(x * 256), 255), colour = table[index].  The background is white; over the SCAs comes the bar -- rows ny - n1/8 .. ny-1,
   columns nx/2 - n1 .. nx/2 + n1 - 1, linspace(0, 1, 2 n1) through the same index rule -- then the ticks, then the stamps.
   out (nh * ny + (nh-1) * gap, nw * nx + (nw-1) * gap, 3) u8 where out_location says, nh = (npanel - 1) / nw + 1.
   RIP_EINVAL, before anything is launched or copied: a NULL table; a count below 1 (nstamps below 0); a scale with n1 < 8 (there
   the reference's arr[-(n1 // 8):] is the whole image) or with a bar or tick outside the panel; an SCA or a stamp that does not
   start inside its panel, or reaches past it (the reference result there is numpy's negative-index slicing or an exception); a
   stamp of a panel that does not exist, of size < 1, of a value or character outside 0..255; stamps without glyphs; a vmin or
   vmax that is not finite, or vmax == vmin; an unknown location. */
int rip_fpa_render(rip_ctx *ctx, int n1, int nsca, int npanel, int nw, int gap, int ny, int nx, const double *maps, int maps_location,
                   const uint8_t *present, const int32_t *sca_pos, const double *vmin, const double *vmax, const uint8_t *scale,
                   const uint8_t *table, const uint8_t *glyphs, int nstamps, const int32_t *stamps, uint8_t *out, int out_location);

/* ---- quick-look pictures of a Level-1 cube (utils/visualize.py, utils/diff.py of the reference) ---------- */
#define RIP_VIEW_MAX_RANKS 8

/* The three entries read a cube (ng,ny,nx) of dtype RIP_U16 or RIP_F32 where cube_location says (RIP_HOST: through a scoped
   device buffer; RIP_DEVICE: read where it is) and are ordered on rip_stream(); each returns when its kernels and copies are
   done.  The value of a sample of plane g is f32(sample), minus f32(sample of plane `minus` at the same pixel) where minus >= 0
   (minus = -1: no differencing): data.astype(np.float32) - data[minus], exact for u16.  No f32 copy of the cube is made.

   np.percentile's raw material (visualize.py:58-59, 83-84, 97): exact order statistics of the window rows y0..y1, columns
   x0..x1 (both INCLUSIVE, as the reference's slice) of the planes g0 .. g1-1.  values[r] (HOST, f32) is the element of 0-based
   rank ranks[r] (HOST) of the n = (g1-g0)(y1-y0+1)(x1-x0+1) values in ascending order; nan_count (HOST, one word) the number
   of NaNs among them.  The order is that of the key of rip_select.h: -0 just below +0, NaNs beyond the infinities on the side of
   their sign (np.sort puts every NaN last: with nan_count > 0 a caller that mirrors numpy answers NaN).  Three histogram levels
   of 11 + 11 + 10 key bits, each one pass over the window; integer atomics only: two calls give the same bits.
   RIP_EINVAL, before anything is launched or copied: a NULL pointer; an unknown dtype or location; an empty or out-of-frame
   window or plane range; minus outside -1..ng-1; nranks outside 1..8; a rank >= n; n >= 2^32. */
int rip_view_ranks(rip_ctx *ctx, const void *cube, int dtype, int cube_location, int ng, int ny, int nx, int y0, int y1, int x0, int x1,
                   int g0, int g1, int minus, int nranks, const uint32_t *ranks, float *values, uint32_t *nan_count);

/* diff.py:17: out (ny,nx) f32 = f32(cube[g2]) - f32(cube[g1]) over the whole frame; out where out_location says.  Of a host
   cube only the two planes travel.  RIP_EINVAL: a NULL pointer, an unknown dtype or location, a plane outside the cube. */
int rip_view_plane_diff(rip_ctx *ctx, const void *cube, int dtype, int cube_location, int ng, int ny, int nx, int g1, int g2, float *out,
                        int out_location);

/* visualize.py:60-111: the finished RGB picture in one store-only launch, every byte written once by the thread that owns the
   pixel.  out (pic_ny,pic_nx,3) u8 where out_location says; row 0 is the BOTTOM row of the picture (as rip_fpa_render's).  The
   background is white.  Every panel is a cell of (cell_h,cell_w) pixels and shows the window rows y0..y1, columns x0..x1
   (inclusive) of one plane, every sample as zoom x zoom pixels (nearest neighbour), window row y0 at the bottom
   (origin="lower"), from the cell's first pixel on: H = zoom (y1-y0+1) rows, W = zoom (x1-x0+1) columns.
   HOST tables:
     panels  (npanel,6) i32   plane g, minus (or -1), norm kind (0 linear, 1 power), (y, x) of the cell's first pixel in the
                              picture, colour bar (0 / 1)
     limits  (npanel,3) f32   vmin, vmax, gamma (read for the power norm only)
     table   (256,3) u8       the colour table;  glyphs (256,12,6) u8 or NULL (then nstamps must be 0)
     stamps  (nstamps,6) i32  as rip_fpa_render's, (y, x) inside the cell
   Per pixel the arithmetic is matplotlib's (3.10, numpy 2) for float32 input, cmap(norm(v), bytes=True)[..., :3]:
     d = v - vmin in f32;  linear (Normalize):  t = f32(f64(d) / (f64(vmax) - f64(vmin)))
                           power (PowerNorm):   t = d / (vmax - vmin) in f32, then t = powf(t, gamma) where t > 0
     index = int(t * 256), below 0 -> 0, from 256 on -> 255 (t == 1 gives 255);  NaN -> white (the map's bad colour is
     transparent);  vmin == vmax -> index 0 for every sample, NaN included (Normalize fills with 0).  / is correctly rounded.
   The colour bar of a panel: the columns W + bar_gap .. W + bar_gap + bar_w - 1 of the rows 0 .. H-1, np.linspace(0, 1, H) from
   the bottom through the same index rule in f64; then its ticks, black, one row high and `tick` columns long, right of the bar at
   the rows 0, H / 2 and H - 1; then the stamps.  A later panel draws over an earlier one.
   RIP_EINVAL, before anything is launched or copied: a NULL cube, table or out; an unknown dtype or location; an empty or
   out-of-frame window; npanel < 1; a plane or minus outside the cube; an unknown norm kind; vmin > vmax or a bound that is not
   finite (matplotlib raises there too); a power norm whose gamma is not finite and positive; zoom < 1; bar_gap or tick < 0,
   bar_w < 1; a cell smaller than H x W, or than W + bar_gap + bar_w + tick columns where the panel has a bar; a cell that
   reaches past the picture; a picture of more than 65535 rows; stamps without glyphs; a stamp of a panel that does not exist,
   outside its cell, of size < 1, of a value or character outside 0..255. */
int rip_view_render(rip_ctx *ctx, const void *cube, int dtype, int cube_location, int ng, int ny, int nx, int y0, int y1, int x0, int x1,
                    int npanel, const int32_t *panels, const float *limits, int zoom, int bar_gap, int bar_w, int tick, int cell_h,
                    int cell_w, int pic_ny, int pic_nx, const uint8_t *table, const uint8_t *glyphs, int nstamps, const int32_t *stamps,
                    uint8_t *out, int out_location);

#ifdef __cplusplus
}
#endif
#endif /* ROMANHIP_H */
