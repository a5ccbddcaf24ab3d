"""The arrays of the reference's ``runs/2026_July/make_dark_file.py`` on the GPU (``csrc/darkstack.hip``): the group means of every
dark exposure, stacked in HBM (``DarkStack.add``), their sigma-clipped mean over the exposures (``sigma_clip_mean``,
``DarkStack.finish``) -- the ``dark_data`` that ``derive_biascorr`` takes -- and the ``dark_slope`` / ``dark_slope_err`` /
``read_noise`` planes (``derive_dark_planes``).  Device in, device out, as the other ``derive_*`` functions.

The clip is specified in ``include/romanhip.h`` (``rip_cal_sigma_clip_mean``) and DESIGN.md section 7 after astropy's documented
defaults; astropy itself is not a dependency and parity with it is unpinned.
"""

import numpy as np

from .. import _native
from ..devarray import DevArray, is_dev
from ._cubes import raw_cube

MAX_PLANES = 512   # darkstack.hip: DS_MAX_PLANES


def _dev_empty(shape, dtype, ctx):
    import torch

    tdt = {np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32}[np.dtype(dtype)]
    return DevArray(torch.empty(shape, dtype=tdt, device=f"cuda:{ctx.device}"), dtype)


def _f32(a, what):
    if is_dev(a):
        if a.dtype != np.dtype(np.float32):
            raise TypeError(f"{what}: device arrays must be float32, not {a.dtype.name}")
        return a
    a = np.asarray(a)
    if a.dtype != np.dtype(np.float32):   # '>f4' included: the arithmetic is pinned for native float32 planes
        raise TypeError(f"{what} must be float32 (the reference's arithmetic follows the file's dtype), not {a.dtype.str}")
    return a


def sigma_clip_mean(stack, sigma=3, maxiters=5, want_count=False, *, sigma_lower=None, sigma_upper=None, n=None, ctx=None):
    """``np.nanmean(sigma_clip(stack[:n], sigma, maxiters=maxiters, axis=0, masked=False), axis=0)`` by the rule of
    ``rip_cal_sigma_clip_mean``.  ``stack``: float32 (planes, ...) numpy array or ``DevArray``, of which the first ``n`` planes
    (default: all, at most 512) take part.  Returns the float32 mean of shape ``stack.shape[1:]`` -- a ``DevArray`` for a
    ``DevArray`` -- and with ``want_count`` also the int32 number of values kept per pixel."""
    ctx = ctx or _native.default_context()
    s = _f32(stack, "stack")
    if s.ndim < 2:
        raise ValueError("stack must be (planes, ...)")
    n = s.shape[0] if n is None else int(n)
    if not 1 <= n <= s.shape[0]:
        raise ValueError(f"{n} planes wanted of a stack of {s.shape[0]}")
    shape = tuple(s.shape[1:])
    npix = int(np.prod(shape, dtype=np.int64))
    lo = float(sigma if sigma_lower is None else sigma_lower)
    hi = float(sigma if sigma_upper is None else sigma_upper)
    dev = is_dev(s)
    if dev:
        s.sync()
        mean = _dev_empty(shape, np.float32, ctx)
        count = _dev_empty(shape, np.int32, ctx) if want_count else None
    else:
        s = np.ascontiguousarray(s)
        mean = np.empty(shape, np.float32)
        count = np.empty(shape, np.int32) if want_count else None
    ctx.call("rip_cal_sigma_clip_mean", s, _native.location_of(s), n, npix, npix, lo, hi, maxiters, mean,
             count)
    return (mean, count) if want_count else mean


def derive_dark_planes(dark1, dark2, dark1_err, dark2_err, cds, nside=None, ctx=None):
    """``make_dark_file.py:79-85, 157`` on five float32 (ny, width) planes of a noise summary, cropped to their first ``nside``
    columns (default: all): ``(dark_slope, dark_slope_err, read_noise)`` = (``where(dark2 > 200, dark1, dark2)``, the same choice
    between the error planes, ``float32(cds / np.sqrt(2))`` -- a float64 division under numpy >= 2), float32 (ny, nside)."""
    ctx = ctx or _native.default_context()
    planes = [_f32(a, w) for a, w in zip((dark1, dark2, dark1_err, dark2_err, cds), ("dark1", "dark2", "dark1_err", "dark2_err", "cds"))]
    if planes[0].ndim != 2 or any(a.shape != planes[0].shape for a in planes):
        raise ValueError("the five planes must be (ny, width) frames of one shape")
    dev = [is_dev(a) for a in planes]
    if any(dev) and not all(dev):
        raise TypeError("the five planes must be all numpy arrays or all DevArrays")
    ny, width = planes[0].shape
    nx = width if nside is None else min(int(nside), width)
    if nx < 1:
        raise ValueError(f"nside {nside} leaves no column")
    if dev[0]:
        planes[0].sync()
        out = [_dev_empty((ny, nx), np.float32, ctx) for _ in range(3)]
    else:
        planes = [np.ascontiguousarray(a) for a in planes]
        out = [np.empty((ny, nx), np.float32) for _ in range(3)]
    ctx.call("rip_cal_dark_planes", *planes, _native.location_of(planes[0]), ny, nx, width, *out)
    return tuple(out)


class DarkStack:
    """The (groups, capacity, rows, nx) float32 stack of group means in HBM.  ``reads``: the flat ``READS`` list; ``ny``, ``nx``: the
    frame of the result (``nx`` may crop the exposures' columns, as the script's ``[:, :, :nside]``); ``capacity``: the number of
    exposures it can take; ``rows = (y0, y1)``: hold only that band of rows -- for a set that does not fit in memory at once."""

    def __init__(self, reads, ny, nx, capacity, ctx=None, rows=None):
        import torch

        self.ctx = ctx or _native.default_context()
        self.reads = np.ascontiguousarray([int(v) for v in reads][:2 * (len(reads) // 2)], dtype=np.int32)
        self.ng = self.reads.size // 2
        self.ny, self.nx, self.capacity = int(ny), int(nx), int(capacity)
        self.y0, self.y1 = (0, self.ny) if rows is None else (int(rows[0]), int(rows[1]))
        if not 1 <= self.ng <= _native.RIP_MAX_GROUPS:
            raise ValueError(f"READS holds {self.ng} groups (1..{_native.RIP_MAX_GROUPS} supported)")
        if self.ny < 1 or self.nx < 1 or not 0 <= self.y0 < self.y1 <= self.ny:
            raise ValueError(f"rows {self.y0}..{self.y1} of a {self.ny} x {self.nx} frame")
        if not 1 <= self.capacity <= MAX_PLANES:
            raise ValueError(f"a capacity of {self.capacity} exposures (1..{MAX_PLANES} supported)")
        shape = (self.ng, self.capacity, self.y1 - self.y0, self.nx)
        need = 4 * int(np.prod(shape, dtype=np.int64))
        free = int(torch.cuda.mem_get_info(self.ctx.device)[0])
        if need > free:
            raise MemoryError(f"the stack of group means needs {need} bytes and {free} bytes of device memory are free: "
                              "work in row bands (rows=(y0, y1))")
        self.stack = DevArray(torch.empty(shape, dtype=torch.float32, device=f"cuda:{self.ctx.device}"))
        self.n = 0
        self._dev = False

    def add(self, cube, fits_be16=False):
        """One dark exposure, a (nreads, ny, width >= nx) cube of 16-bit samples (numpy array, memory map or ``DevArray``), into
        the next slot.  ``fits_be16``: the samples are FITS storage (big-endian int16 with ``BZERO = 32768``), as
        ``calio.read_fits_image`` maps them; otherwise they are native uint16.  A host array is uploaded on the library's stream
        (only the rows of the band)."""
        if self.n >= self.capacity:
            raise ValueError(f"the stack holds {self.capacity} exposures already")
        cube = raw_cube(cube, fits_be16, False)
        if cube.ndim != 3 or cube.shape[1] != self.ny:
            raise ValueError(f"a (nreads, {self.ny}, width) cube is needed, not {tuple(cube.shape)}")
        self._dev = self._dev or is_dev(cube)
        nreads, _, width = cube.shape
        self.ctx.call("rip_cal_group_means", cube, _native.location_of(cube), nreads, self.ny, width, self.y0,
                      self.y1 - self.y0, self.nx, self.reads, self.ng, bool(fits_be16), self.stack, self.capacity, self.n)
        self.n += 1

    def finish(self, sigma=3, maxiters=5, want_count=False, *, sigma_lower=None, sigma_upper=None):
        """``dark_data``: per group the clipped mean over the exposures added, float32 (ng, rows, nx) -- a ``DevArray`` when an
        exposure came as one, else a numpy array -- and with ``want_count`` the int32 counts of the same shape."""
        if self.n < 1:
            raise ValueError("no exposure was added")
        ctx = self.ctx
        shape = (self.ng,) + self.stack.shape[2:]
        npix = shape[1] * shape[2]
        mean = _dev_empty(shape, np.float32, ctx)
        count = _dev_empty(shape, np.int32, ctx) if want_count else None
        lo = float(sigma if sigma_lower is None else sigma_lower)
        hi = float(sigma if sigma_upper is None else sigma_upper)
        for g in range(self.ng):
            ctx.call("rip_cal_sigma_clip_mean", self.stack.t[g], _native.RIP_DEVICE, self.n, npix, npix, lo, hi, maxiters, mean.t[g],
                     None if count is None else count.t[g])
        if not self._dev:
            mean, count = mean.numpy(), None if count is None else count.numpy()
        return (mean, count) if want_count else mean
