"""Case table and input generators of the reference-pixel image drop-ins at small and odd frames
(test_host_refpix_dropin_cases.py proves the table is what it claims, test_gpu_refpix_dropins.py runs it on the device).

Every median of the drop-ins is taken by one in-LDS sort of `count` values padded to a power of two
(block_median_sorted, csrc/refpix.hip), in blocks of 1024 threads:
  row step      ref_med[r]: 8 border pixels or the 128 values of the reference output; sci_med[r]: nside - 8 science pixels
                (only for slope=None and for row_medians); ctr: the ny row medians
  channel step  bottom / top: 4 * (channel_end - channel_start) values per window
The tables below choose ny, nside and the windows so that these counts are odd, no power of two, below, at and just over the
block size.  Inputs are seeded by the case's name: no fixtures on disk.
"""

import collections
import warnings
import zlib

import numpy as np

from oracle import refpix as orp

BLOCK = 1024   # threads per block of the median kernels

# ---------------------------------------------------------------------------------------------------------------- row step
ROW_NYS = (1, 2, 5, 37, 1024, 1025, 2049)
ROW_NSIDES = (16, 24, 136, 1037)
ROW_WIDTHS = ((False, 0), (False, 3), (True, 0), (True, 5))   # (use_ref_channel, columns beyond the narrowest width)
ROW_FORMS = ("f64", "pyfloat", "f32", "fit", "medians")
ROW_SLOPES = {"f64": np.float64(0.3371), "pyfloat": 0.7, "f32": np.float32(0.83), "fit": None, "medians": None}
FIT_MIN_NY = 16   # np.polyfit of slope=None wants a well-conditioned fit

RowCase = collections.namedtuple("RowCase", "name ny nside use_ref extra form family")


def row_width(c):
    return c.nside + (128 if c.use_ref else 0) + c.extra


def _row_case(ny, nside, use_ref, extra, form, family="noise"):
    name = f"{family}-ny{ny}-ns{nside}-{'refout' if use_ref else 'border'}+{extra}-{form}"
    return RowCase(name, ny, nside, use_ref, extra, form, family)


def _row_geometry_cases():
    # not the cross product: per update form every ny, and nside and width rotated against it so that every value of every
    # parameter meets every form (test_host_refpix_dropin_cases.py checks exactly that)
    out = []
    for f, form in enumerate(ROW_FORMS):
        nys = [ny for ny in ROW_NYS if form != "fit" or ny >= FIT_MIN_NY]
        for i, ny in enumerate(nys):
            use_ref, extra = ROW_WIDTHS[(i + i // 4 + 2 * f) % 4]
            out.append(_row_case(ny, ROW_NSIDES[(i + f) % 4], use_ref, extra, form))
    return out


# the value families, each on a border-pixel geometry (8 values a row) and a reference-output geometry (128 values a row);
# NaN only with a given slope (np.polyfit on NaN is not the subject); `huge`: an odd count of values above FLT_MAX / 2, which
# only the science medians of an odd nside can hold (a mean of two finite floats never exceeds FLT_MAX / 2)
_A = (37, 24, False, 3)
_B = (37, 136, True, 0)
ROW_FAMILY_CASES = [
    _row_case(*_A, "f64", "ties"), _row_case(*_B, "f32", "ties"), _row_case(*_B, "medians", "ties"),
    _row_case(*_A, "pyfloat", "const"), _row_case(*_B, "f64", "const"),
    _row_case(*_A, "f64", "zeros"), _row_case(*_B, "pyfloat", "zeros"), _row_case(*_A, "medians", "zeros"),
    _row_case(*_B, "medians", "zeros"),
    _row_case(*_A, "f64", "inf"), _row_case(*_B, "f32", "inf"), _row_case(*_B, "medians", "inf"),
    _row_case(*_A, "f64", "nan"), _row_case(*_B, "pyfloat", "nan"), _row_case(*_A, "medians", "nan"),
    _row_case(*_B, "f32", "nan"),
    _row_case(5, 1037, False, 0, "medians", "huge"),
]
ROW_CASES = _row_geometry_cases() + ROW_FAMILY_CASES
ROW_BY_NAME = {c.name: c for c in ROW_CASES}


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def row_ref_columns(c):
    """the columns whose values make ref_med[r] (reference_subtraction.py:108-111)"""
    if c.use_ref:
        return np.arange(c.nside, c.nside + 128)
    return np.concatenate((np.arange(0, 4), np.arange(c.nside - 4, c.nside)))


def _minus_zero_window(rng, n):
    """n values whose two middle elements (n even) are both -0, between runs of -1 and +1, shuffled"""
    k = max(2, n // 12)
    lo = (n - k) // 2
    v = np.concatenate((np.full(lo, -1.0), np.full(k, -0.0), np.full(n - k - lo, 1.0))).astype(np.float32)
    return rng.permutation(v)


def row_image(c):
    """the float32 image of a row case, (ny, row_width)"""
    rng = _rng(c.name)
    ny, w = c.ny, row_width(c)
    cols = row_ref_columns(c)
    n = cols.size
    # science and reference pixels share a per-row drift, so the fit of slope=None has something to find
    img = (rng.normal(0, 30, size=(ny, w)) + rng.normal(0, 25, size=ny)[:, None]).astype(np.float32)
    if c.family == "ties":
        img = rng.choice(np.array([-1.5, 0.25, 2.0], np.float32), size=(ny, w))
    elif c.family == "const":
        img = np.full((ny, w), 7.25, np.float32)
    elif c.family == "zeros":
        u = rng.random(size=(ny, w))
        img[u < 0.2] = -0.0
        img[(u >= 0.2) & (u < 0.4)] = 0.0
        for r in range(ny):
            if r % 3 == 0:
                img[r, cols] = _minus_zero_window(rng, n)
            elif r % 3 == 1:
                img[r, cols] = -0.0
    elif c.family == "inf":
        many = n // 2 + 1
        img[1, cols[rng.permutation(n)[:many]]] = np.inf       # more than half the window +inf
        img[2, cols[rng.permutation(n)[:many]]] = -np.inf      # more than half -inf
        one = rng.permutation(n)[:2]
        img[3, cols[one[0]]] = np.inf                          # one of each
        img[3, cols[one[1]]] = -np.inf
        img[5, 6] = np.inf                                     # and a science pixel
    elif c.family == "nan":
        img[7, cols[rng.integers(n)]] = np.nan                 # one NaN, inside the reference window of row 7
    elif c.family == "huge":
        img[:, 4:c.nside - 4] = rng.uniform(2.0e38, 3.3e38, size=(ny, c.nside - 8)).astype(np.float32)
    return np.ascontiguousarray(img, dtype=np.float32)


def row_oracle(c, image):
    """oracle.refpix.row_step on a copy of `image`: (image out, ref_med, sci_med, ctr, the slope applied or None).  A medians-only
    case returns the image as it was."""
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        sci = np.median(image[:, 4:c.nside - 4], axis=1)
        if c.form == "medians":
            _, ref, ctr = orp.row_step(image.copy(), c.nside, c.use_ref, 0.0)
            return image.copy(), ref, sci, ctr, None
        slope = ROW_SLOPES[c.form]
        if slope is None:
            ref = orp.row_step(image.copy(), c.nside, c.use_ref, 0.0)[1]
            slope = orp._polyfit_slope(ref, sci)
        out, ref, ctr = orp.row_step(image.copy(), c.nside, c.use_ref, slope)
    return out, ref, sci, ctr, slope


def row_median_counts(c):
    """the counts of the medians a row case takes on the device"""
    counts = [128 if c.use_ref else 8, c.ny]
    if c.form in ("fit", "medians"):
        counts.append(c.nside - 8)
    return counts


# ------------------------------------------------------------------------------------------------------------ channel step
CHAN_NYS = (8, 9, 13, 300)
CHAN_WINDOWS = ((0, 128), (4, 124), (0, 1), (5, 8), (0, 129), (0, 192), (0, 257))
CHAN_COUNTS = ((1, False), (2, True), (5, False), (1, True), (2, False), (5, True))   # (n_channels, use_ref_channel)
CHAN_EXTRAS = (0, 3)   # columns beyond the narrowest width that fits

ChanCase = collections.namedtuple("ChanCase", "name ny start end n_channels use_ref extra family")


def chan_windows(c):
    return c.n_channels + (1 if c.use_ref else 0)


def chan_width(c):
    return c.end + (chan_windows(c) - 1) * 128 + c.extra


def _chan_case(ny, win, n_channels, use_ref, extra, family="noise"):
    name = f"{family}-ny{ny}-w{win[0]}_{win[1]}-n{n_channels}{'+ref' if use_ref else ''}+{extra}"
    return ChanCase(name, ny, win[0], win[1], n_channels, use_ref, extra, family)


def _chan_geometry_cases():
    out = []
    for q in range(2 * len(CHAN_WINDOWS)):
        n, ref = CHAN_COUNTS[q % 6]
        out.append(_chan_case(CHAN_NYS[q % 4], CHAN_WINDOWS[q % 7], n, ref, CHAN_EXTRAS[(q + q // 7) % 2]))
    # every overlapping width with several windows (a window sees the updates of those before it), at adjacent bottom and top rows
    out.append(_chan_case(8, (0, 257), 5, False, 0))
    out.append(_chan_case(8, (0, 129), 5, True, 3))
    return out


_C = (13, (0, 128), 2, True, 3)     # three disjoint windows: the batched path
_D = (9, (0, 192), 2, False, 0)     # two overlapping windows: the sequential path
CHAN_FAMILY_CASES = [_chan_case(*g, family=f) for f in ("ties", "const", "zeros", "inf", "nan") for g in (_C, _D)]
CHAN_CASES = _chan_geometry_cases() + CHAN_FAMILY_CASES
CHAN_BY_NAME = {c.name: c for c in CHAN_CASES}


def chan_image(c):
    """the float32 image of a channel case, (ny, chan_width)"""
    rng = _rng(c.name)
    ny, w, cw = c.ny, chan_width(c), c.end - c.start
    img = (rng.normal(0, 30, size=(ny, w)) + 0.7 * np.arange(ny)[:, None] + rng.normal(0, 20, size=w)[None, :]).astype(np.float32)
    win = [slice(c.start + 128 * k, c.end + 128 * k) for k in range(chan_windows(c))]
    bottom, top = slice(0, 4), slice(ny - 4, ny)
    if c.family == "ties":
        img = rng.choice(np.array([-1.5, 0.25, 2.0], np.float32), size=(ny, w))
    elif c.family == "const":
        img = np.full((ny, w), 7.25, np.float32)
    elif c.family == "zeros":
        u = rng.random(size=(ny, w))
        img[u < 0.2] = -0.0
        img[(u >= 0.2) & (u < 0.4)] = 0.0
        img[bottom, win[0]] = _minus_zero_window(rng, 4 * cw).reshape(4, cw)
        img[top, win[0]] = -0.0
    elif c.family == "inf":
        def put(rows, k, values):
            # into the first 128 columns of window k: the next window, where windows overlap, starts after them
            own = slice(win[k].start, win[k].start + min(cw, 128))
            flat = img[rows, own].reshape(-1)
            flat[rng.permutation(flat.size)[:len(values)]] = values
            img[rows, own] = flat.reshape(4, -1)
        put(bottom, 0, [np.inf] * (2 * cw + 1))      # more than half the window +inf
        put(top, 1, [-np.inf] * (2 * cw + 1))        # more than half -inf
        put(top, 0, [np.inf, -np.inf])               # one of each
    elif c.family == "nan":
        img[rng.integers(4), win[1].start + rng.integers(cw)] = np.nan   # one NaN in a bottom reference row of window 1
    return np.ascontiguousarray(img, dtype=np.float32)


def chan_oracle(c, image):
    """oracle.refpix.channel_step on a copy: (image out, table) with table[k] = (bottom, top, m, c), LAPACK lines"""
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return orp.channel_step(image.copy(), c.n_channels * 128, c.use_ref, c.start, c.end, n_channels=c.n_channels)


def channel_step_two_point(image, start, end, nwin):
    """the channel step with the device's line restated in float64 (channel line fit): m = (t - b) / (ny - 4),
    c = b - 1.5 m from the float32 medians, taken as the loop goes.  In place; returns (image, table) like the oracle."""
    ny = image.shape[0]
    rows = np.arange(ny, dtype=np.float64)
    table = np.zeros((nwin, 4), dtype=np.float64)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for k in range(nwin):
            sl = slice(start + 128 * k, end + 128 * k)
            b, t = np.median(image[0:4, sl]), np.median(image[ny - 4:ny, sl])
            assert b.dtype == np.float32 and t.dtype == np.float32
            m = (np.float64(t) - np.float64(b)) / np.float64(ny - 4)
            cc = np.float64(b) - 1.5 * m
            line = m * rows + cc
            image[:, sl] = (image[:, sl].astype(np.float64) - line[:, None]).astype(np.float32)
            table[k] = (b, t, m, cc)
    return image, table


def chan_median_count(c):
    return 4 * (c.end - c.start)


# ------------------------------------------------------------------------------------------------- rip_stage_refpix_image
IMAGE_CASES = [(ny, nx, do_row, do_chan) for ny in (8, 37) for nx in (128, 384)
               for do_row, do_chan in ((1, 0), (0, 1), (1, 1))]
IMAGE_SLOPE = np.float64(0.3371)


def image_case_image(ny, nx):
    rng = np.random.default_rng(1000 * ny + nx)
    img = (rng.normal(0, 30, size=(ny, nx + 128)) + rng.normal(0, 25, size=ny)[:, None] + 0.7 * np.arange(ny)[:, None])
    return np.ascontiguousarray(img, dtype=np.float32)


# ------------------------------------------------------------------------------------------------ limits the code accepts
MAX_SORT = 32768              # the largest count block_median_sorted is asked for: 128 KiB of dynamic LDS
LIMIT_ROW_NY = dict(ny=32768, nside=16)          # ctr over 32768 row medians
LIMIT_ROW_NSIDE = dict(ny=8, nside=32776)        # science medians over 32768 pixels
LIMIT_CHAN_WINDOW = dict(ny=8, start=0, end=8192)   # 4 x 8192 values


def limit_image(ny, w, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.normal(0, 30, size=(ny, w)) + rng.normal(0, 25, size=ny)[:, None], dtype=np.float32)
