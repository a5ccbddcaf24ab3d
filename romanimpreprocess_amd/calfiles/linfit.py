"""The arrays of a ``linearitylegendre`` file on the GPU (``csrc/linfit.hip``): the per-frame sums of every ramp set, kept in HBM
(``RampStack``), and the constrained Legendre fit of the linearity curve to their mean ramps (``derive_linearity``).  Device in,
device out: the planes feed ``derive_pflat``, ``derive_saturation``, ``derive_biascorr`` and ``derive_mask`` where they are.

The reference runs solid-waffle's ``linearity_run`` for this step and solid-waffle's source is not part of it: the rule is
specified in ``include/romanhip.h`` (``rip_cal_linearity_fit``) and DESIGN.md section 7, and parity with solid-waffle is unpinned.
"""

import ctypes as C

import numpy as np

from .. import _native
from ..devarray import DevArray, is_dev, to_device
from ._cubes import raw_cube

MAX_SETS = 8        # linfit.hip: LF_MAX_SETS
MAX_ORDER = 10      # LF_MAX_ORDER
MAX_EXPOSURES = 65536
KEYS = ("data", "dq", "Smin", "Smax", "Sref", "dark", "pflat", "ramperr")   # the planes of the file


def _dev_empty(shape, dtype, ctx, zero=False):
    import torch

    dtype = np.dtype(dtype)
    tdt = {"float32": torch.float32, "int32": torch.int32, "uint32": torch.int32, "uint16": torch.int16}[dtype.name]
    make = torch.zeros if zero else torch.empty
    return DevArray(make(shape, dtype=tdt, device=f"cuda:{ctx.device}"), dtype).sync()


class RampStack:
    """The uint32 (nframes, rows, nx) per-frame sums of one ramp set in HBM.  ``ny``, ``nx``: the frame of the result (``nx`` may
    crop the exposures' columns, as the ``[:4096]`` of the 4224-wide cubes); ``rows = (y0, y1)``: hold only that band of rows --
    for a set that does not fit in memory at once.  ``count`` is the number of exposures added, ``sums`` the ``DevArray``."""

    def __init__(self, nframes, ny, nx, ctx=None, rows=None):
        self.ctx = ctx or _native.default_context()
        self.nframes, self.ny, self.nx = int(nframes), int(ny), int(nx)
        self.y0, self.y1 = (0, self.ny) if rows is None else (int(rows[0]), int(rows[1]))
        if self.nframes < 1 or self.ny < 1 or self.nx < 1 or not 0 <= self.y0 < self.y1 <= self.ny:
            raise ValueError(f"rows {self.y0}..{self.y1} of {self.nframes} frames of {self.ny} x {self.nx}")
        self.sums = _dev_empty((self.nframes, self.y1 - self.y0, self.nx), np.uint32, self.ctx, zero=True)
        self.count = 0

    def add(self, cube, fits_be16=False):
        """One exposure, a (nframes, ny, width >= nx) or (1, nframes, ny, width) cube of 16-bit samples (numpy array, memory map or
        ``DevArray``, as ``frames_to_cube`` makes them).  ``fits_be16``: the samples are FITS storage (big-endian int16 with ``BZERO
        = 32768``), as ``calio.read_fits_image`` maps them; otherwise they are native uint16."""
        cube = raw_cube(cube, fits_be16, True)
        if cube.ndim != 3 or cube.shape[0] != self.nframes or cube.shape[1] != self.ny:
            raise ValueError(f"a ({self.nframes}, {self.ny}, width) cube is needed, not {tuple(cube.shape)}")
        self.ctx.call("rip_cal_frame_sums", cube, _native.location_of(cube), self.nframes, self.ny, cube.shape[2],
                      self.y0, self.y1 - self.y0, self.nx, 0, bool(fits_be16), self.sums, self.count)
        self.count += 1


def _set_index(i, n, key):
    """a Python-style index into the ``n`` sets"""
    i = int(i)
    if not -n <= i < n:
        raise ValueError(f"{key} {i} outside the {n} sets of RAMPS")
    return i % n


def derive_linearity(stacks, sref, *, p_order=8, tframe=3.04, slopecut=0.5, negativepad=500, tstart=1, dark=-1, bright=0, nb=4,
                     sign=1, rows=None, ctx=None):
    """The planes of the ``linearitylegendre`` file as a dict of ``DevArray``: ``data`` (p_order+1, ny, nx) f32, ``dq`` u32, ``Smin``,
    ``Smax``, ``Sref`` f32, ``dark`` f32, ``pflat`` (sets but the dark one, ny, nx) f32, ``ramperr`` (sets, ny, nx) u16 -- and
    ``cut`` i32, the frame of the bright set where its ramp was cut (a diagnostic, not part of the file).
    ``stacks``: the ramp sets in the order of ``RAMPS``, each a ``RampStack`` or a ``(sums, count)`` pair with ``sums`` uint32
    (frames, ny, nx), numpy or ``DevArray``.  ``sref``: (ny, nx) float32, numpy or ``DevArray``.  ``tstart``: the first frame to
    use, counted from 1 (``TSTART``), one number or one per set.  ``dark``, ``bright``: Python-style indices into ``stacks``;
    ``dark=None``: no dark set.  ``rows = (y0, ny_frame)``: the planes are the band of rows from ``y0`` of a frame of ``ny_frame`` rows
    (the stacks were made with ``rows``), which only the ``nb`` border looks at.  The rule is that of ``rip_cal_linearity_fit``."""
    ctx = ctx or _native.default_context()
    n = len(stacks)
    if not 1 <= n <= MAX_SETS:
        raise ValueError(f"RAMPS holds {n} sets (1..{MAX_SETS} supported)")
    dark = -1 if dark is None else _set_index(dark, n, "DARK")
    bright = _set_index(bright, n, "bright set")
    tstart = [int(tstart)] * n if np.ndim(tstart) == 0 else [int(t) for t in tstart]
    if len(tstart) != n:
        raise ValueError(f"{len(tstart)} TSTART values for {n} sets")
    sums, counts = [], []
    for s in stacks:
        a, c = (s.sums, s.count) if isinstance(s, RampStack) else s
        if not is_dev(a):
            a = np.asarray(a)
            if a.dtype != np.uint32:
                raise TypeError(f"sums must be uint32, not {a.dtype.name}")
            a = to_device(a, ctx.device)
        if a.dtype != np.dtype(np.uint32) or a.ndim != 3:
            raise TypeError(f"sums must be uint32 (frames, ny, nx), not {a.dtype.name} {tuple(a.shape)}")
        sums.append(a.sync())
        counts.append(int(c))
    ny, nx = sums[0].shape[1:]
    if any(a.shape[1:] != (ny, nx) for a in sums):
        raise ValueError("the sums of all sets must be frames of one shape")
    if not is_dev(sref):
        sref = np.asarray(sref)
        if sref.dtype != np.float32:
            raise TypeError(f"Sref must be float32, not {sref.dtype.name}")
        sref = to_device(sref, ctx.device)
    if sref.dtype != np.dtype(np.float32) or tuple(sref.shape) != (ny, nx):
        raise ValueError(f"Sref must be float32 ({ny}, {nx}), not {sref.dtype.name} {tuple(sref.shape)}")
    sref.sync()
    p = int(p_order)
    ok = 1 <= p <= MAX_ORDER   # refused by the library, by name: nothing is sized by it here
    out = {"data": _dev_empty((p + 1 if ok else 1, ny, nx), np.float32, ctx), "dq": _dev_empty((ny, nx), np.uint32, ctx),
           "Smin": _dev_empty((ny, nx), np.float32, ctx), "Smax": _dev_empty((ny, nx), np.float32, ctx), "Sref": sref,
           "dark": _dev_empty((ny, nx), np.float32, ctx), "pflat": _dev_empty((n - (dark >= 0) or 1, ny, nx), np.float32, ctx),
           "ramperr": _dev_empty((n, ny, nx), np.uint16, ctx), "cut": _dev_empty((ny, nx), np.int32, ctx)}
    ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in sums])
    ctx.call("rip_cal_linearity_fit", n, ptrs, np.array(counts, np.int32), np.array([t - 1 for t in tstart], np.int32),
             np.array([a.shape[0] for a in sums], np.int32), sref, ny, nx,
             *((0, ny) if rows is None else (int(rows[0]), int(rows[1]))), int(nb), p, int(sign), float(tframe), float(slopecut),
             float(negativepad), bright, dark, out["data"], out["Smin"], out["Smax"], out["dq"], out["pflat"], out["dark"],
             out["ramperr"], out["cut"])
    return out
