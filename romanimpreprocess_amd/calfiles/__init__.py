"""The four CALDIR files the reference derives from a ``linearitylegendre`` / ``dark`` / ``gain`` set -- ``pflat``,
``saturation``, ``biascorr`` (``runs/2026_July/postprocess_calfiles.py``) and ``mask`` (``runs/2026_July/makemask.py``) -- on the
GPU (``csrc/calfiles.hip``).  The array-level functions below take numpy arrays or ``DevArray`` planes (results then stay in
HBM as ``DevArray`` too) and reproduce the scripts' numpy arithmetic bit for bit (numpy >= 2 promotion rules, float32 planes);
``postprocess_calfiles.run`` and ``makemask.run`` are the scripts' file-level drop-ins.  The step in front of them, the ``dark`` and
``read`` files of ``make_dark_file.py``, is ``darkstack.py`` (``DarkStack``, ``sigma_clip_mean``, ``derive_dark_planes``) and the
drop-in ``make_dark_file.run``.
"""

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

    tdt = {np.dtype(np.float32): torch.float32, np.dtype(np.uint32): torch.int32}[np.dtype(dtype)]
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
    ctx.check(ctx.lib.rip_cal_biascorr(ctx.h, ds.ctypes.data, dd.ctypes.data, dd.shape[0], ny, nx, nb, co.shape[0], co.ctypes.data,
                                       lo.ctypes.data, hi.ctypes.data, r.ctypes.data, ngrp, float(tframe), int(bframe),
                                       out.ctypes.data, None if pred is None else pred.ctypes.data, _native.C.byref(t0)))
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
    ctx.check(ctx.lib.rip_cal_pflat(ctx.h, p.ctypes.data, ny, nx, int(order), LPX.ctypes.data, LPY.ctypes.data, c.ctypes.data,
                                    float(scale), data.ctypes.data, dq.ctypes.data))
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
    ctx.check(ctx.lib.rip_cal_saturation(ctx.h, a.ctypes.data, b.ctypes.data, a.shape[0], a.shape[1], data.ctypes.data, dq.ctypes.data))
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
    ctx.check(ctx.lib.rip_cal_mask(ctx.h, ny, nx, int(nb), l.ctypes.data, p.ctypes.data, float(med), d.ctypes.data, g.ctypes.data,
                                   dq.ctypes.data))
    return dq


from .darkstack import DarkStack, derive_dark_planes, sigma_clip_mean  # noqa: E402, F401
