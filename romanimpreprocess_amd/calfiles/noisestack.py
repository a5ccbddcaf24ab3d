"""The noise summary of a dark set on the GPU (``csrc/noisestat.hip``): what the reference's job obtains from solid-waffle's
``noise_run`` and ``make_dark_file.py`` reads -- the planes ``DARK1``, ``DARK1ERR``, ``DARK2``, ``DARK2ERR``, ``CDS``, ``RESET``, the
reference output's ``AMP33`` planes and the parameters ``ACN``, ``C_PINK``, ``U_PINK``, ``M_PINK``, ``RU_PINK`` of the correlated
noise.  ``NoiseStack.add`` streams every exposure through the device once (integer per-pixel accumulators and f64 moment tables of
row-sum differences, all in HBM), ``NoiseStack.finish`` makes the planes there and the parameters on the host (``noise_params``: a
few hundred KB of tables, numpy, no GPU).

solid-waffle's source is not part of the reference: the estimator is specified in ``include/romanhip.h`` and DESIGN.md section 7,
and parity with solid-waffle is unpinned.  The parameters are defined as the inverse of the reference's own generator
(``from_sim/sim_to_isim.py`` :306-402, restated by ``L1Synth.fill``) and tested by round trip.
"""

import numpy as np

from .. import _native
from ..devarray import DevArray
from ._cubes import raw_cube

MAX_FRAMES = 64       # noisestat.hip: NS_MAX_FRAMES
MAX_EXPOSURES = 512   # NS_MAX_EXPOSURES
MAX_CW = 256          # NS_MAX_CW
MIN_ROWS = 128        # NS_MIN_ROWS
MAX_SCALE = 6         # NS_MAX_SCALE
G = 8.0 * np.log(2.0)   # variance of the difference of two adjacent block means of a CDS of 1/f noise with S(f) = 1/f
PLANES = ("DARK1", "DARK1ERR", "DARK2", "DARK2ERR", "CDS", "RESET")   # the order of rip_cal_noise_planes
_ACC = (("a0", np.uint32), ("a1", np.uint64), ("b0", np.int32), ("b1", np.uint64), ("s0", np.int64), ("s1", np.uint64),
        ("c0", np.int32), ("c1", np.uint64))
TABLES = ("h1", "h2", "t1", "t2", "ht", "q1", "q2")


def _dev(shape, dtype, ctx, zero=True):
    import torch

    dtype = np.dtype(dtype)
    tdt = {"float32": torch.float32, "float64": torch.float64, "int32": torch.int32, "uint32": torch.int32, "int64": torch.int64,
           "uint64": torch.int64}[dtype.name]
    return DevArray((torch.zeros if zero else torch.empty)(shape, dtype=tdt, device=f"cuda:{ctx.device}"), dtype).sync()


def scales(ny):
    """the largest scale J = min(6, floor(log2(ny / 64))): scale j compares blocks of 2^j rows and has ``ny >> (j+1)`` pairs"""
    return min(MAX_SCALE, (int(ny) // 64).bit_length() - 1)


def check_geometry(ny, nx_file, C, cw, f0, n, ref_out):
    """the refusals of ``rip_cal_noise_add`` that size an array, by the names of the command line; ValueError"""
    if not 2 <= n <= MAX_FRAMES:
        raise ValueError(f"-tn {n} frames (2..{MAX_FRAMES} supported)")
    if f0 < 0:
        raise ValueError(f"-t {f0 + 1}: frames are counted from 1")
    if cw < 2 or cw % 2 or cw > MAX_CW:
        raise ValueError(f"channel width {cw} (even, 2..{MAX_CW})")
    if ny < MIN_ROWS:
        raise ValueError(f"{ny} rows (at least {MIN_ROWS})")
    if C < 1 or (C + bool(ref_out)) * cw > nx_file:
        raise ValueError(f"{C} channels of {cw} columns{' and the reference output' if ref_out else ''} wanted of a frame of {nx_file}")


def _line_intercept(y):
    """``a`` of the unweighted least-squares line ``y_j = a + w 2^-j``"""
    x = 0.5 ** np.arange(y.size)
    dx = x - x.mean()
    return float(y.mean() - (dx * (y - y.mean())).sum() / (dx * dx).sum() * x.mean())


def noise_params(tables, N, n, ny, C, cw, vbar):
    """The parameters of the correlated noise from the moment tables of ``rip_cal_noise_rowstats`` (a dict of numpy arrays ``h1``,
    ``h2`` (n-1, nbt, nch), ``t1``, ``t2``, ``ht`` (n-1, nbt; ``ht`` None without reference output), ``q1``, ``q2`` (n-1, nch)) of
    ``N`` exposures; ``vbar``: the mean of ``CDS**2`` over the science columns.  Returns a dict with ``ACN``, ``C_PINK``, ``U_PINK``
    and, with a reference output, ``M_PINK`` and ``RU_PINK``.  numpy on the host, no GPU.

    With h = H / (cw 2^j) (the difference of the means of two adjacent blocks of 2^j rows of one channel of a CDS) and all
    covariances taken over the exposures, which removes the fixed pattern: ``V_j`` the mean variance of a science channel's h,
    ``X_j`` the mean covariance of two different science channels' h (from the variance of their sum T), ``V33_j`` and ``E_j`` the
    variance of the reference output's h and its covariance with T / C.  1/f noise of unit amplitude gives h the variance ``G = 8 ln 2``
    at every scale, white noise one that falls as 2^-j: ``C_PINK^2 = mean_j X_j / G``, ``U_PINK^2 = a / G`` with ``V_j - X_j = a + w
    2^-j``, ``M_PINK = mean_j E_j / mean_j X_j``, ``RU_PINK^2 = a33 / G - M_PINK^2 C_PINK^2`` with ``V33_j = a33 + w33 2^-j``.  ``ACN``:
    q = 2 Q / (ny cw) is the mean of a channel-frame's even columns minus that of its odd ones in a CDS; alternating column noise
    of amplitude A gives it the variance 8 A^2 on top of the 4 vbar / (ny cw) of the pixels' own noise.  Negative squares give 0."""
    N, C, cw, ny = int(N), int(C), int(cw), int(ny)
    if N < 2:
        raise ValueError(f"-n {N} exposures: a variance over exposures needs two")
    J = scales(ny)
    nb = [ny >> (j + 1) for j in range(J + 1)]
    scale_of = np.repeat(np.arange(J + 1), nb)                    # (nbt,)
    inv2 = 1.0 / (cw * 2.0 ** scale_of) ** 2
    h1, h2, t1, t2 = (np.asarray(tables[k], np.float64) for k in ("h1", "h2", "t1", "t2"))
    ref_out = tables.get("ht") is not None

    def per_scale(a):   # mean over the pairs and blocks of each scale
        a = a.reshape(a.shape[0], a.shape[1], -1).mean(axis=2)
        return np.array([a[:, scale_of == j].mean() for j in range(J + 1)])

    var_h = (h2 - h1 * h1 / N) / (N - 1) * inv2[None, :, None]
    var_t = (t2 - t1 * t1 / N) / (N - 1) * inv2[None, :]
    V = per_scale(var_h[:, :, :C])
    X = per_scale((var_t - var_h[:, :, :C].sum(axis=2)) / (C * (C - 1))) if C > 1 else np.zeros(J + 1)
    xm = float(X.mean())
    out = {"C_PINK": float(np.sqrt(max(xm, 0.0) / G)), "U_PINK": float(np.sqrt(max(_line_intercept(V - X) / G, 0.0)))}
    if ref_out:
        ht = np.asarray(tables["ht"], np.float64)
        E = per_scale((ht - h1[:, :, C] * t1 / N) / (N - 1) * inv2[None, :] / C)
        m = float(E.mean() / xm) if xm > 0.0 else 0.0
        a33 = _line_intercept(per_scale(var_h[:, :, C]))
        out["M_PINK"] = m
        out["RU_PINK"] = float(np.sqrt(max(a33 / G - m * m * out["C_PINK"] ** 2, 0.0)))
    q1, q2 = (np.asarray(tables[k], np.float64)[:, :C] for k in ("q1", "q2"))
    area = float(ny) * cw
    var_q = (q2 - q1 * q1 / N) / (N - 1) * (4.0 / (area * area))
    out["ACN"] = float(np.sqrt(max((var_q.mean() - 4.0 * float(vbar) / area) / 8.0, 0.0)))
    return out


class NoiseSummary:
    """What ``NoiseStack.finish`` returns: ``planes`` (6, ny, C*cw) float32 in the order ``PLANES`` and ``amp33`` (2, ny, cw)
    float32 (None without reference output) as ``DevArray``; ``params`` (``noise_params``); ``tables`` (numpy); and the scalars
    ``N``, ``n``, ``f0``, ``tframe``.  ``plane(name)`` is one plane, a ``DevArray`` view."""

    def __init__(self, planes, amp33, params, tables, N, n, f0, tframe):
        self.planes, self.amp33, self.params, self.tables = planes, amp33, params, tables
        self.N, self.n, self.f0, self.tframe = int(N), int(n), int(f0), float(tframe)

    def plane(self, name):
        return DevArray(self.planes.t[PLANES.index(name)], np.float32)

    def hdus(self, cards=()):
        """the summary as the list ``calio.write_fits`` takes: an empty primary HDU, the cube with the cards that
        ``make_dark_file`` reads (the plane indices ``DARK1`` .. ``RESET``, ``ACN``, ``C_PINK``, ``U_PINK``, ``NDARK``, ``TSTART``,
        ``NFRAME``, ``TFRAME``, then ``cards``) and, with a reference output, the ``AMP33`` extension with ``M_PINK``, ``RU_PINK``"""
        p = self.params
        head = [(k, i) for i, k in enumerate(PLANES)] + [(k, float(p[k])) for k in ("ACN", "C_PINK", "U_PINK")]
        head += [("NDARK", self.N), ("TSTART", self.f0 + 1), ("NFRAME", self.n), ("TFRAME", self.tframe)] + list(cards)
        out = [None, {"data": self.planes, "cards": head}]
        if self.amp33 is not None:
            out.append({"data": self.amp33, "extname": "AMP33", "cards": [("M_PINK", float(p["M_PINK"])), ("RU_PINK", float(p["RU_PINK"]))]})
        return out


class NoiseStack:
    """The accumulators of a noise summary in HBM.  Exposures are (nreads, ``ny``, ``nx_file``) cubes of which the frames ``f0`` ..
    ``f0 + n - 1`` (``-t`` = f0 + 1, ``-tn`` = n) and the first ``C * cw`` columns take part, with ``ref_out`` also the ``cw`` columns
    of the reference output behind them.  52 bytes per pixel (56 in the reference output), about 1 GB for 4096 x 4224: no row bands.
    ``count`` is the number of exposures added; ``acc`` (per-pixel integer sums), ``tables`` (f64 moment tables) and ``rowsum``
    (the last exposure's row sums) are dicts of ``DevArray`` / a ``DevArray``, as ``rip_cal_noise_add`` and ``_rowstats`` lay them out."""

    def __init__(self, ny, nx_file, C, cw, f0, n, ref_out, ctx=None):
        self.ctx = ctx or _native.default_context()
        self.ny, self.nx_file, self.C, self.cw, self.f0, self.n = int(ny), int(nx_file), int(C), int(cw), int(f0), int(n)
        self.ref_out = bool(ref_out)
        check_geometry(self.ny, self.nx_file, self.C, self.cw, self.f0, self.n, self.ref_out)
        self.nch = self.C + self.ref_out
        self.nx = self.C * self.cw
        ctx = self.ctx
        self.acc = {k: _dev((self.ny, self.nch * self.cw), t, ctx) for k, t in _ACC}
        self.acc["m33"] = _dev((self.ny, self.cw), np.uint32, ctx) if self.ref_out else None
        self.rowsum = _dev((self.n, self.ny, self.nch, 2), np.uint32, ctx)
        K, nbt = self.n - 1, sum(self.ny >> (j + 1) for j in range(scales(self.ny) + 1))
        shapes = {"h1": (K, nbt, self.nch), "h2": (K, nbt, self.nch), "t1": (K, nbt), "t2": (K, nbt), "ht": (K, nbt),
                  "q1": (K, self.nch), "q2": (K, self.nch)}
        self.tables = {k: _dev(s, np.float64, ctx) if (k != "ht" or self.ref_out) else None for k, s in shapes.items()}
        self.count = 0

    def add(self, cube, fits_be16=False):
        """One dark exposure, a (nreads, ny, nx_file) or (1, nreads, ny, nx_file) cube of 16-bit samples: numpy array, memory map
        or ``DevArray`` (as ``frames_to_cube`` makes them).  ``fits_be16``: the samples are FITS storage (big-endian int16 with
        ``BZERO = 32768``), as ``calio.read_fits_image`` maps them; otherwise native uint16.  Of a host array only the frames used
        travel."""
        cube = raw_cube(cube, fits_be16, True)
        if cube.ndim != 3 or cube.shape[1] != self.ny or cube.shape[2] != self.nx_file:
            raise ValueError(f"a (nreads, {self.ny}, {self.nx_file}) cube is needed, not {tuple(cube.shape)}")
        a, t = self.acc, self.tables
        self.ctx.call("rip_cal_noise_add", cube, _native.location_of(cube), cube.shape[0], self.ny, self.nx_file, self.C, self.cw,
                      self.ref_out, self.f0, self.n, bool(fits_be16), self.count, a["a0"], a["a1"], a["b0"], a["b1"], a["s0"], a["s1"],
                      a["c0"], a["c1"], a["m33"], self.rowsum)
        self.ctx.call("rip_cal_noise_rowstats", self.rowsum, self.n, self.ny, self.C, self.ref_out, t["h1"], t["h2"], t["t1"], t["t2"],
                      t["ht"], t["q1"], t["q2"])
        self.count += 1

    def finish(self, tframe=3.04):
        """The ``NoiseSummary`` of the exposures added (two at least): the planes by ``rip_cal_noise_planes``, the parameters by
        ``noise_params`` from the downloaded tables and the ``CDS`` plane."""
        a = self.acc
        planes = _dev((6, self.ny, self.nx), np.float32, self.ctx, zero=False)
        amp33 = _dev((2, self.ny, self.cw), np.float32, self.ctx, zero=False) if self.ref_out else None
        self.ctx.call("rip_cal_noise_planes", a["a0"], a["a1"], a["b0"], a["b1"], a["s0"], a["s1"], a["c0"], a["c1"], a["m33"],
                      self.count, self.n, self.ny, self.C, self.cw, self.ref_out, float(tframe), _native.RIP_DEVICE, planes, amp33)
        tables = {k: None if v is None else v.numpy() for k, v in self.tables.items()}
        cds = planes.t[PLANES.index("CDS")].cpu().numpy().astype(np.float64)
        params = noise_params(tables, self.count, self.n, self.ny, self.C, self.cw, float(np.mean(cds * cds)))
        return NoiseSummary(planes, amp33, params, tables, self.count, self.n, self.f0, tframe)
