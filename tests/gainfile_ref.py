"""numpy restatement of the gain / ipc4d derivation (romanimpreprocess_amd/calfiles: summary_means, derive_gain_ipc4d), with
every dtype written out.  The expansion is written from the closed form per pixel, not from the slicing
of the reference's make_gain_file.py: tests/test_host_gainfile_ref.py holds it against the fixtures that script produced, and
the GPU tests use it where no fixture exists -- non-square frames, and chosen rows of the full frame (`rows`).

With sp(Y, X) = (Y // ry, X // rx) on full-frame coordinates and a_t(p) = f64(f32(mean_t[sp(p + nb)])) for active pixel p:
  K[1+dy, 1+dx][p] = (a_t(p) + a_t(p + o)) / 2.0 where p + o is an active pixel, else 0.0     (o = (dy, dx) != (0, 0))
                     t = aV for (+-1, 0), aH for (0, +-1), aD for the diagonals
  K[1, 1][p]       = 1.0 - S, S the float64 sum of the nine planes taken one after the other in row-major order, centre 0.0
"""

import warnings

import numpy as np

COLS = {"X": 0, "Y": 1, "N": 2, "g": 5, "aH": 6, "aV": 7, "aD": 10}
NAMES = ("g", "aH", "aV", "aD")
TYPE_OF = {(-1, 0): "aV", (1, 0): "aV", (0, -1): "aH", (0, 1): "aH", (-1, -1): "aD", (-1, 1): "aD", (1, -1): "aD", (1, 1): "aD"}


def summary_means(tables):
    """(means dict of float64 (nsy,nsx), good bool (nsy,nsx), tmean dict): numpy's nanmean IS the definition of these bits"""
    t = np.asarray(tables, dtype=np.float64)
    n = t[:, :, COLS["N"]]
    good = np.count_nonzero(n, axis=0) > 0
    nsx, nsy = 1 + int(np.amax(t[0, :, COLS["X"]])), 1 + int(np.amax(t[0, :, COLS["Y"]]))
    means, tmean = {}, {}
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for e in NAMES:
            m = np.nanmean(np.where(n > 0, t[:, :, COLS[e]], np.nan), axis=0)
            tmean[e] = np.nanmean(m)
            means[e] = np.where(good, m, tmean[e]).reshape(nsy, nsx)
    return means, good.reshape(nsy, nsx), tmean


def tiling(means, shape):
    nsy, nsx = np.shape(means["g"])
    ny, nx = shape
    ry, rx = ny // nsy, nx // nsx
    assert nsy * ry == ny and nsx * rx == nx, "the superpixels must tile the frame"
    return nsy, nsx, ry, rx


def gain_planes(means, good, shape, nb=4):
    """(gain float32, dq uint32), full frames"""
    nsy, nsx, ry, rx = tiling(means, shape)
    ny, nx = shape
    Y, X = np.arange(ny)[:, None], np.arange(nx)[None, :]
    border = (Y < nb) | (Y >= ny - nb) | (X < nb) | (X >= nx - nb)
    g32 = np.asarray(means["g"], np.float64).astype(np.float32)
    gain = np.where(border, np.float32(0.0), g32[Y // ry, X // rx]).astype(np.float32)
    dq = np.where(border | ~np.asarray(good, bool)[Y // ry, X // rx], np.uint32(2**19), np.uint32(0)).astype(np.uint32)
    return gain, dq


def ipc4d(means, shape, nb=4, ipc_dtype=np.float64, rows=None):
    """The kernel (3, 3, len(rows), nx - 2 nb) for the active rows `rows` (None: all of them, in order)."""
    nsy, nsx, ry, rx = tiling(means, shape)
    ny, nx = shape
    nya, nxa = ny - 2 * nb, nx - 2 * nb
    ya = (np.arange(nya) if rows is None else np.asarray(rows, dtype=np.int64))[:, None]
    xa = np.arange(nxa)[None, :]
    t32 = {e: np.asarray(means[e], np.float64).astype(np.float32) for e in ("aH", "aV", "aD")}

    def alpha(e, y, x):   # neighbours outside the active region are looked up at the nearest pixel inside: never used
        y, x = np.clip(y, 0, nya - 1), np.clip(x, 0, nxa - 1)
        return t32[e][(y + nb) // ry, (x + nb) // rx].astype(np.float64)

    K = np.zeros((3, 3, ya.shape[0], nxa), np.float64)
    for (dy, dx), e in TYPE_OF.items():
        inside = (ya + dy >= 0) & (ya + dy < nya) & (xa + dx >= 0) & (xa + dx < nxa)
        K[1 + dy, 1 + dx] = np.where(inside, (alpha(e, ya, xa) + alpha(e, ya + dy, xa + dx)) / np.float64(2.0), np.float64(0.0))
    s = K[0, 0].copy()
    for j in range(1, 9):
        s = s + K[j // 3, j % 3]   # j = 4 adds the centre's 0.0
    K[1, 1] = np.float64(1.0) - s
    return K if np.dtype(ipc_dtype) == np.float64 else K.astype(ipc_dtype)


def derive(means, good, shape, nb=4, ipc_dtype=np.float64):
    """(gain, gain_dq, kernel, kernel_dq) as calfiles.derive_gain_ipc4d returns them"""
    gain, dq = gain_planes(means, good, shape, nb)
    return gain, dq, ipc4d(means, shape, nb, ipc_dtype), np.zeros((shape[0] - 2 * nb, shape[1] - 2 * nb), np.uint32)
