"""The four CALDIR files the reference derives from a ``linearitylegendre`` / ``dark`` / ``gain`` set -- ``pflat``,
``saturation``, ``biascorr`` (``runs/2026_July/postprocess_calfiles.py``) and ``mask`` (``runs/2026_July/makemask.py``) -- on the
GPU (``csrc/calfiles.hip``).  The array-level functions below take numpy arrays or ``DevArray`` planes (results then stay in
HBM as ``DevArray`` too) and reproduce the scripts' numpy arithmetic bit for bit (numpy >= 2 promotion rules, float32 planes);
``postprocess_calfiles.run`` and ``makemask.run`` are the scripts' file-level drop-ins.  The step in front of them, the ``dark`` and
``read`` files of ``make_dark_file.py``, is ``darkstack.py`` (``DarkStack``, ``sigma_clip_mean``, ``derive_dark_planes``) and the
drop-in ``make_dark_file.run``; in front of that, the exposure cubes and slope images that the three converters of
``runs/summer2025run`` make of the raw test-stand frames are ``convert_frames.py`` (``frames_to_cube``, ``cube_slopes``, ``convert``,
``csrc/rawframes.hip``) with the drop-ins ``convert_dark``, ``convert_flt`` and ``convert_loflt``.  The ``gain`` and ``ipc4d`` files that all of them read come from ``summary_means`` (numpy, on
the host: the tables are a few KB) and ``derive_gain_ipc4d`` (``csrc/gainfile.hip``), with the drop-in ``make_gain_file.run``.  The
``linearitylegendre`` file itself -- the per-frame sums of the flat and dark ramps and the constrained Legendre fit to them -- is
``linfit.py`` (``RampStack``, ``derive_linearity``, ``csrc/linfit.hip``) with the drop-in ``linearity_run.run``.  The noise summary
that ``make_dark_file`` reads -- the ``DARK1`` .. ``RESET`` planes, ``AMP33`` and the parameters of the correlated noise -- is
``noisestack.py`` (``NoiseStack``, ``noise_params``, ``csrc/noisestat.hip``) with the drop-in ``noise_run.run``.  The superpixel
summaries that ``make_gain_file`` reads -- gain and inter-pixel capacitance from pairs of flats and darks -- are ``corrstack.py``
(``CorrStack``, ``solve_summary``, ``csrc/corrstat.hip``) with the drop-in ``correlation_run.run_ir_all`` and, for the job's whole
gain step, ``correlation_run.gain_from_flats``.
"""

import warnings

import numpy as np

from .. import _native, pars
from ..devarray import DevArray, is_dev
from ..utils import sky

TFRAME = 3.04   # postprocess_calfiles.py:106
BFRAME = 1      # :109
NBORDER = 4     # :119


def _plane(a, dtype, what):
    """C-contiguous array of ``dtype``: a DevArray as it is, anything else through numpy.  The scripts' arithmetic is pinned for
    float32 planes and uint32 flags (what the reference's files hold); another float width is refused, not converted."""
    if is_dev(a):
        if a.dtype != np.dtype(dtype):
            raise TypeError(f"{what}: device arrays must be {np.dtype(dtype).name}, not {a.dtype.name}")
        return a
    a = np.asarray(a)
    if np.dtype(dtype).kind == "f" and a.dtype != np.dtype(dtype):
        raise TypeError(f"{what} must be {np.dtype(dtype).name} (the reference's arithmetic follows the file's dtype), not {a.dtype.name}")
    return np.ascontiguousarray(a, dtype=dtype)


def _empty(shape, dtype, on_device, ctx):
    if not on_device:
        return np.empty(shape, dtype)
    import torch

    tdt = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.uint32): torch.int32}[np.dtype(dtype)]
    return DevArray(torch.empty(shape, dtype=tdt, device=f"cuda:{ctx.device}"), dtype)


def _sync(*arrays):
    for a in arrays:
        if is_dev(a):
            a.sync()
            return


def parse_reads(reads, bframe=BFRAME):
    """``READS`` of a ``settings_<name>.yaml`` -> (int32 array of 2 ngrp read numbers, ngrp, xref): group ``j`` holds the reads
    ``READS[2j] .. READS[2j+1]-1`` and ``xref`` is the mean read number of the bias group (``postprocess_calfiles.py:115-127``)."""
    r = [int(v) for v in reads]
    ngrp = len(r) // 2
    if not 0 <= int(bframe) < ngrp:
        raise ValueError(f"bias group {bframe} outside the {ngrp} groups of READS")
    xref = (r[2 * int(bframe)] + r[2 * int(bframe) + 1] - 1) / 2.0
    return np.array(r[:2 * ngrp], dtype=np.int32), ngrp, xref


def reads_of_pattern(read_pattern):
    """The flat ``READS`` list of a read pattern given as a list of groups of consecutive read numbers."""
    out = []
    for g in read_pattern:
        out += [int(g[0]), int(g[-1]) + 1]
    return out


def derive_biascorr(dark_slope, dark_data, lin_data, smin, smax, reads, tframe=TFRAME, bframe=BFRAME, nb=NBORDER, want_pred=False,
                    ctx=None):
    """``postprocess_calfiles.py:103-140``.  ``dark_slope`` (ny,nx), ``dark_data`` (ngrp,ny,nx), the linearity planes ``lin_data``
    (nplanes,ny,nx), ``smin``, ``smax`` (ny,nx), all float32 full frames; ``reads`` the flat ``READS`` list.
    Returns ``(biascorr, t0)``, with ``want_pred`` ``(biascorr, t0, pred)``: (ngrp, ny-2nb, nx-2nb) float32 planes, ``pred`` the
    script's ``Sdark_predicted``, and ``t0 = tframe * xref`` in seconds."""
    ctx = ctx or _native.default_context()
    ds, dd = _plane(dark_slope, np.float32, "dark_slope"), _plane(dark_data, np.float32, "dark data")
    co, lo, hi = _plane(lin_data, np.float32, "linearity data"), _plane(smin, np.float32, "Smin"), _plane(smax, np.float32, "Smax")
    r = np.ascontiguousarray([int(v) for v in reads], dtype=np.int32)
    ngrp = r.size // 2
    if ds.ndim != 2 or dd.ndim != 3 or co.ndim != 3 or dd.shape[1:] != ds.shape or co.shape[1:] != ds.shape or lo.shape != ds.shape \
            or hi.shape != ds.shape:
        raise ValueError("dark_slope, dark data and the linearity planes must be full frames of one shape")
    ny, nx = ds.shape
    nb = int(nb)
    shape = (max(ngrp, 0), max(ny - 2 * nb, 0), max(nx - 2 * nb, 0))
    dev = any(is_dev(a) for a in (ds, dd, co, lo, hi))
    _sync(ds, dd, co, lo, hi)
    out = _empty(shape, np.float32, dev, ctx)
    pred = _empty(shape, np.float32, dev, ctx) if want_pred else None
    t0 = _native.C.c_double(0.0)
    ctx.call("rip_cal_biascorr", ds, dd, dd.shape[0], ny, nx, nb, co.shape[0], co, lo, hi, r, ngrp, tframe, bframe, out, pred,
             _native.C.byref(t0))
    return (out, t0.value, pred) if want_pred else (out, t0.value)


def derive_pflat(pflat0, gain, N=6, order=2, g_ideal=pars.g_ideal, ctx=None):
    """``postprocess_calfiles.py:22-40``: the raw p-flat plane ``lin["pflat"][0]`` divided by its ``medfit`` model, scaled by
    ``g_ideal / np.median(gain)``, flagged outside [0.01, 1.99] and clipped.  Returns ``(data f32, dq u32, coefs)``.  The median is
    over the whole gain plane and NaN as soon as it holds one NaN, as numpy's."""
    ctx = ctx or _native.default_context()
    p, g = _plane(pflat0, np.float32, "pflat"), _plane(gain, np.float32, "gain")
    if p.ndim != 2:
        raise ValueError("pflat must be one (ny,nx) plane")
    _sync(p, g)
    ny, nx = p.shape
    coef, LPX, LPY = sky.medfit_tables(p, int(N), int(order), ctx)
    c = np.ascontiguousarray(coef, dtype=np.float64)
    with np.errstate(all="ignore"):
        scale = np.float32(g_ideal) / sky.median(g, ctx=ctx)   # Python float / np.float32: a float32 division under numpy >= 2 (:34)
    dev = is_dev(p)
    data, dq = _empty((ny, nx), np.float32, dev, ctx), _empty((ny, nx), np.uint32, dev, ctx)
    ctx.call("rip_cal_pflat", p, ny, nx, order, LPX, LPY, c, scale, data, dq)
    return data, dq, coef


def derive_saturation(smax, sref, ctx=None):
    """``postprocess_calfiles.py:69-97``: ``(data, dq)`` = (float32(clip(Smax, 1, 65535)) - 1, 0 where Smax > Sref else 1)."""
    ctx = ctx or _native.default_context()
    a, b = _plane(smax, np.float32, "Smax"), _plane(sref, np.float32, "Sref")
    if a.ndim != 2 or a.shape != b.shape:
        raise ValueError("Smax and Sref must be (ny,nx) planes of one shape")
    _sync(a, b)
    dev = is_dev(a) or is_dev(b)
    data, dq = _empty(a.shape, np.float32, dev, ctx), _empty(a.shape, np.uint32, dev, ctx)
    ctx.call("rip_cal_saturation", a, b, a.shape[0], a.shape[1], data, dq)
    return data, dq


def derive_mask(lin_dq, pflat0, dark_slope, gain_dq, nb=NBORDER, ctx=None):
    """``makemask.py:12-36``: REFERENCE_PIXEL on the ``nb`` border rows and columns | ``lin_dq`` | LOW_QE where
    ``pflat0 / np.median(pflat0) < 0.5`` | HOT (``dark_slope`` > 12.5) or WARM (> 0.25) | ``gain_dq``.  Returns the uint32 plane."""
    ctx = ctx or _native.default_context()
    l, g = _plane(lin_dq, np.uint32, "linearity dq"), _plane(gain_dq, np.uint32, "gain dq")
    p, d = _plane(pflat0, np.float32, "pflat"), _plane(dark_slope, np.float32, "dark_slope")
    if p.ndim != 2 or any(a.shape != p.shape for a in (l, g, d)):
        raise ValueError("the four planes must be (ny,nx) frames of one shape")
    _sync(l, g, p, d)
    ny, nx = p.shape
    med = sky.median(p, ctx=ctx)
    dq = _empty((ny, nx), np.uint32, any(is_dev(a) for a in (l, g, p, d)), ctx)
    ctx.call("rip_cal_mask", ny, nx, nb, l, p, med, d, g, dq)
    return dq

SUMMARY_COLS = {"X": 0, "Y": 1, "N": 2, "g": 5, "aH": 6, "aV": 7, "aD": 10}   # solid-waffle output columns (make_gain_file.py:21)
GAIN_OUTPUTS = ("gain", "gain_dq", "kernel", "kernel_dq")


def summary_means(tables):
    """``make_gain_file.py:39-56``: the superpixel tables of solid-waffle summary files.  ``tables`` is (N_in, nrow, ncol), one
    ``np.loadtxt`` array per file.  Returns ``(means, good, tmean)``: ``means`` the float64 (nsy,nsx) tables of ``g``, ``aH``,
    ``aV``, ``aD`` -- the ``nanmean`` over the files that have ``N > 0`` in a superpixel, the ``nanmean`` of that over the array
    (``tmean[e]``) where no file has; ``good`` the bool (nsy,nsx) table of superpixels with ``N > 0`` in at least one file;
    ``nsx = 1 + max X`` and ``nsy = 1 + max Y`` of the first file.  numpy's own sums, so that the bits are the script's."""
    alldata = np.zeros(np.shape(tables))   # float64, as the script's np.zeros((N_in, nrow, ncol))
    alldata[...] = tables
    if alldata.ndim != 3 or alldata.shape[0] < 1 or alldata.shape[2] <= max(SUMMARY_COLS.values()):
        raise ValueError(f"summary tables must be (N_in, nrow, >= {max(SUMMARY_COLS.values()) + 1} columns), not {alldata.shape}")
    cols = SUMMARY_COLS
    good = np.count_nonzero(alldata[:, :, cols["N"]], axis=0) > 0
    nsx = 1 + int(np.amax(alldata[0, :, cols["X"]]))
    nsy = 1 + int(np.amax(alldata[0, :, cols["Y"]]))
    if nsy * nsx != alldata.shape[1]:
        raise ValueError(f"{alldata.shape[1]} table rows are not {nsy} x {nsx} superpixels")
    means, tmean = {}, {}
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")   # "Mean of empty slice" where no file covers a superpixel
        for e in ("g", "aH", "aV", "aD"):
            m = np.nanmean(np.where(alldata[:, :, cols["N"]] > 0, alldata[:, :, cols[e]], np.nan), axis=0)
            tmean[e] = np.nanmean(m)
            means[e] = np.where(good, m, tmean[e]).reshape((nsy, nsx))
    return means, good.reshape((nsy, nsx)), tmean


def derive_gain_ipc4d(means, good, shape=(pars.nside, pars.nside), nb=NBORDER, ipc_dtype=np.float64, on_device=False, ctx=None,
                      outputs=GAIN_OUTPUTS):
    """``make_gain_file.py:59-68, 88, 104, 130-175, 195``: the tables of ``summary_means`` expanded to a frame of ``shape``, each
    superpixel ``shape[0] // nsy`` rows by ``shape[1] // nsx`` columns (a frame they do not tile exactly is refused).  Returns
    ``(gain, gain_dq, kernel, kernel_dq)``: gain f32 and its flags u32 (ny,nx), zero and ``2**19`` on the ``nb`` border; the ipc4d
    kernel (3,3,ny-2nb,nx-2nb) and its all-zero flags u32 (ny-2nb,nx-2nb), as the script leaves them.  ``ipc_dtype`` float64 is
    what the script writes; float32 is each of those values rounded once (the fused chain's faster form reads it).  numpy arrays,
    or ``DevArray`` with ``on_device`` (the inputs are small host tables, so residency cannot follow them).  ``outputs`` names
    the results wanted; the others are not computed and come back as None."""
    ctx = ctx or _native.default_context()
    t = np.ascontiguousarray([np.asarray(means[e], dtype=np.float64) for e in ("g", "aH", "aV", "aD")])
    if t.ndim != 3:
        raise ValueError("the four mean tables must be (nsy,nsx) arrays of one shape")
    gd = np.ascontiguousarray(np.asarray(good) != 0, dtype=np.uint8)
    if gd.shape != t.shape[1:]:
        raise ValueError(f"good is {gd.shape}, the mean tables {t.shape[1:]}")
    unknown = [o for o in outputs if o not in GAIN_OUTPUTS]
    if unknown:
        raise ValueError(f"unknown outputs {unknown}; known: {GAIN_OUTPUTS}")
    nsy, nsx = t.shape[1:]
    ny, nx, nb = int(shape[0]), int(shape[1]), int(nb)
    code = {np.dtype(np.float32): _native.RIP_F32, np.dtype(np.float64): _native.RIP_F64}.get(np.dtype(ipc_dtype), -1)
    active = (max(ny - 2 * nb, 0), max(nx - 2 * nb, 0))
    specs = {"gain": ((ny, nx), np.float32), "gain_dq": ((ny, nx), np.uint32), "kernel": ((3, 3) + active, ipc_dtype),
             "kernel_dq": (active, np.uint32)}
    # a dtype the library has no code for is refused there, by name, like the other arguments: nothing is allocated for it
    out = {o: _empty(*specs[o], on_device, ctx) if o in outputs and code >= 0 and min(ny, nx) > 0 else None for o in GAIN_OUTPUTS}
    ctx.call("rip_cal_gain_ipc4d", t, gd, nsy, nsx, ny, nx, nb, _native.RIP_DEVICE if on_device else _native.RIP_HOST,
             out["gain"], out["gain_dq"], out["kernel"], code, out["kernel_dq"])
    return tuple(out[o] for o in GAIN_OUTPUTS)


from .darkstack import DarkStack, derive_dark_planes, sigma_clip_mean  # noqa: E402, F401
from .convert_frames import convert, cube_slopes, find_frames, frames_to_cube  # noqa: E402, F401
from .linfit import RampStack, derive_linearity  # noqa: E402, F401
from .noisestack import NoiseStack, NoiseSummary, noise_params  # noqa: E402, F401
from .corrstack import CorrStack, solve_summary  # noqa: E402, F401
