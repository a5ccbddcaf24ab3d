// The arithmetic the reference-pixel kernels share (refpix.hip, refpix_one.hip) beyond the keys and selections of rip_select.h:
// the row correction and the channel line.
#pragma once
#include "rip_select.h"

// row correction of a row median v (reference_subtraction.py:115-123): slope * f64(f32(v - ctr)) for a numpy f64 slope; every
// operation f32 for an f32 slope (row_corr_f32, s32 = f32(slope))
__device__ __forceinline__ double row_corr(double slope, float v, float ctr) { return slope * (double)(v - ctr); }
__device__ __forceinline__ double row_corr_f32(float s32, float v, float ctr) { return (double)(s32 * (v - ctr)); }

// the line through (1.5, b), (ny - 2.5, t) (reference_subtraction.py:57-60), or the caller's (m, c) at ovr (LAPACK's: the
// reference fits it with gelsd, which agrees to ~1e-13 relative but not bit for bit; DESIGN.md "channel line fit")
__device__ __forceinline__ void chan_line(float b, float t, int ny, const double *ovr, double &m, double &c) {
    if (ovr) {
        m = ovr[0];
        c = ovr[1];
    } else {
        m = ((double)t - (double)b) / (double)(ny - 4);
        c = (double)b - 1.5 * m;
    }
}
