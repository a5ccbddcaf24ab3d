"""Independent numpy restatement of the dark-file arithmetic (the reference's runs/2026_July/make_dark_file.py; device code:
csrc/darkstack.hip).  Group means are the script's own np.mean expression.  The clipped mean is a masked loop over np.nanmedian /
np.nanmean / np.nanstd by the rule written down for rip_cal_sigma_clip_mean (include/romanhip.h) -- astropy
is not available, so that rule is the specification.  tests/test_host_darkstack_ref.py checks this file by closed forms.

numpy sums f64 pairwise, the device in another fixed order, so `s` may differ in its last bits between the two.  sigma_clip_mean
therefore also reports the pixels where that could matter: those with a value within 1e-9 * (|c| + sigma * s) of a bound, but
not ON it, in any round ("borderline").  The GPU tests compare ALL pixels, and may, because every input of theirs has none.  A
value exactly on a bound is not borderline: the tests put values there only where m and s are exact in any order of summation
(a constant column: every deviation is zero; two dyadic values: the deviations and their squares are exact)."""

import warnings

import numpy as np


def group_means(cube, reads, nx=None):
    """(ng, ny, nx) float32: make_dark_file.py:66-69 per group, on the first nx columns"""
    cube = np.asarray(cube)
    nx = cube.shape[2] if nx is None else nx
    return np.stack([np.mean(cube[reads[2 * g]:reads[2 * g + 1], :, :nx].astype(np.float32), axis=0) for g in range(len(reads) // 2)])


def group_means_sequential(cube, reads, nx=None):
    """the same by the rule stated for the kernel: the f32 sum read after read, divided once by f32(number of reads)"""
    cube = np.asarray(cube)
    nx = cube.shape[2] if nx is None else nx
    out = []
    for g in range(len(reads) // 2):
        a, b = reads[2 * g], reads[2 * g + 1]
        acc = np.zeros(cube.shape[1:2] + (nx,), np.float32)
        for r in range(a, b):
            acc = acc + cube[r, :, :nx].astype(np.float32)
        out.append(acc / np.float32(b - a))
    return np.stack(out)


def from_fits_be16(raw):
    """the unsigned samples of FITS storage (big-endian int16, BZERO = 32768)"""
    return (np.asarray(raw).astype(np.int32) + 32768).astype(np.uint16)


def to_fits_be16(cube):
    return (np.asarray(cube).astype(np.int32) - 32768).astype(">i2")


def sigma_clip_mean(stack, sigma=3.0, maxiters=5, sigma_lower=None, sigma_upper=None):
    """(mean f32, count i32, borderline bool), each of shape stack.shape[1:]; see the module docstring"""
    stack = np.asarray(stack)
    assert stack.dtype == np.float32
    sl = float(sigma if sigma_lower is None else sigma_lower)
    su = float(sigma if sigma_upper is None else sigma_upper)
    data = stack.astype(np.float64)
    data[~np.isfinite(data)] = np.nan
    borderline = np.zeros(stack.shape[1:], bool)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for _ in range(int(maxiters)):
            c = np.nanmedian(data, axis=0)
            m = np.nanmean(data, axis=0)
            s = np.nanstd(data, axis=0)   # about the MEAN, ddof 0
            lo, hi = c - sl * s, c + su * s
            fin = ~np.isnan(data)
            dlo, dhi = np.abs(data - lo), np.abs(data - hi)
            near = ((dlo > 0) & (dlo <= 1e-9 * (np.abs(c) + sl * s))) | ((dhi > 0) & (dhi <= 1e-9 * (np.abs(c) + su * s)))
            borderline |= np.any(fin & near, axis=0)
            remove = fin & ((data < lo) | (data > hi))
            if not remove.any():   # a pixel that lost nothing keeps c, m and s: going on for the others does not change it
                break
            data[remove] = np.nan
        fin = ~np.isnan(data)
        count = np.count_nonzero(fin, axis=0).astype(np.int32)
        total = np.zeros(stack.shape[1:], np.float64)
        for plane, keep in zip(data, fin):   # plane order, what np.nanmean does along axis 0 (test_host_darkstack_ref.py)
            total = total + np.where(keep, plane, 0.0)
        mean = (total / count).astype(np.float32)
    return mean, count, borderline


def dark_planes(dark1, dark2, dark1_err, dark2_err, cds, nside):
    """make_dark_file.py:79-85, 157 as written there"""
    use1 = dark2[:, :nside] > 200
    dark_slope = np.where(use1, dark1[:, :nside], dark2[:, :nside]).astype(np.float32)
    dark_slope_err = np.where(use1, dark1_err[:, :nside], dark2_err[:, :nside]).astype(np.float32)
    read_noise = (cds[:, :nside] / np.sqrt(2)).astype(np.float32)
    return dark_slope, dark_slope_err, read_noise
