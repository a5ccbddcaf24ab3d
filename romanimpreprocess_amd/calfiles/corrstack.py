"""Gain and inter-pixel capacitance of a flat set per superpixel: what the reference's job obtains from solid-waffle's
``correlation_run.run_ir_all`` (``runs/2026_July/make_sca_files_2026Jul.job`` lines 48-64) and ``make_gain_file.py`` reads.
``CorrStack.add_pair`` sends one pair of exposures through the device once (``csrc/corrstat.hip``, ``rip_cal_corr_pair``): 25
integer sums per superpixel.  ``solve_summary`` (numpy float64 on the host: the tables are a few hundred KB) turns the sums of a
light and a dark set into the summary table.

solid-waffle's source is not part of the reference: the estimator is specified in ``include/romanhip.h`` and DESIGN.md section 7,
and parity with solid-waffle is unpinned.  It is the inverse of the package's own forward model (``L1Synth``: ``ipc_fwd`` with
the ``ipc4d`` kernel, ``1 / gain``, the inverse linearity, read noise, rounding) and tested by round trip.
"""

import numpy as np

from .. import _native
from ._cubes import raw_cube

SLOTS = 25            # corrstat.hip: CR_SLOTS
MAX_SUPERPIXEL = 16384   # CR_MAX_PIX: a superpixel's differences are held in LDS
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))   # (dy, dx) of the slots 3 .. 18, four slots each
NCOL = 11             # columns of the summary table
IPC_STEPS = 32


def check_frames(frames, nreads=None):
    """the four 0-based frames ``(fa, fb, fc, fd)`` as ints; ValueError naming ``TIME`` (1-based, as the configuration has it)"""
    try:
        fa, fb, fc, fd = (int(f) for f in frames)
    except (TypeError, ValueError):
        raise ValueError(f"TIME needs four frames, got {frames!r}") from None
    time = f"TIME {fa + 1} {fb + 1} {fc + 1} {fd + 1}"
    if min(fa, fb, fc, fd) < 0 or (nreads is not None and max(fa, fb, fc, fd) >= nreads):
        raise ValueError(f"{time} asks for frames outside a cube of {nreads if nreads is not None else 'any number of'} frames (counted from 1)")
    if not (fa < fb and fc < fd and fa < fd):
        raise ValueError(f"{time} (a < b, c < d and a < d are needed)")
    return fa, fb, fc, fd


def check_geometry(ny, nx, nbin, nb):
    """``(sy, sx)`` of ``nbin = (nbx, nby)`` superpixels (the order of ``NBIN``) on a (ny, nx) frame; ValueError naming ``NBIN``"""
    nbx, nby = int(nbin[0]), int(nbin[1])
    if nbx < 1 or nby < 1 or ny % nby or nx % nbx:
        raise ValueError(f"NBIN {nbx} {nby}: the superpixels do not divide the frame of ({ny},{nx})")
    sy, sx = ny // nby, nx // nbx
    if sy * sx > MAX_SUPERPIXEL:
        raise ValueError(f"NBIN {nbx} {nby}: a superpixel of ({sy},{sx}) has {sy * sx} pixels (at most {MAX_SUPERPIXEL})")
    if nb < 0:
        raise ValueError(f"a border of {nb}")
    return sy, sx


def _cube(cube, fits_be16):
    """a cube as ``rip_cal_corr_pair`` takes it: (nreads, ny_file, nx_file) 16-bit words, contiguous, viewed as uint16"""
    cube = raw_cube(cube, fits_be16, True)
    if cube.ndim != 3:
        raise ValueError(f"a (nreads, ny, nx) cube is needed, not {tuple(cube.shape)}")
    return cube


class CorrStack:
    """The pair statistics of one set of exposures (the flats, or the darks).  ``frames``: the four 0-based frames ``(fa, fb, fc,
    fd)`` (``TIME`` minus one); the frame is the first ``(ny, nx)`` samples of every file frame (the ``[:4096]`` crop of 4224-wide
    cubes); ``nbin = (nbx, nby)`` superpixels as ``NBIN`` gives them; ``nb`` the border.  ``count`` pairs have been added."""

    def __init__(self, frames, ny, nx, nbin, nb=4, ctx=None):
        self.ctx = ctx or _native.default_context()
        self.frames = check_frames(frames)
        self.ny, self.nx, self.nb = int(ny), int(nx), int(nb)
        self.nbx, self.nby = int(nbin[0]), int(nbin[1])
        self.sy, self.sx = check_geometry(self.ny, self.nx, nbin, self.nb)
        self.tables = []

    @property
    def count(self):
        return len(self.tables)

    def add_pair(self, cube1, cube2, fits_be16=False):
        """One pair of exposures of one shape (nreads, ny_file, nx_file) or (1, nreads, ny_file, nx_file): numpy arrays, memory
        maps or ``DevArray`` cubes (as ``frames_to_cube`` makes them), either one in host memory or in HBM.  ``fits_be16``: the
        samples of both are FITS storage (big-endian int16 with ``BZERO = 32768``), as ``calio.read_fits_image`` maps them;
        otherwise native uint16.  Of a host cube only the rows of the four frames travel.  Returns the pair's int64 table."""
        a, b = _cube(cube1, fits_be16), _cube(cube2, fits_be16)
        if a.shape != b.shape:
            raise ValueError(f"the two exposures of a pair are {tuple(a.shape)} and {tuple(b.shape)}")
        nreads, ny_file, nx_file = a.shape
        check_frames(self.frames, nreads)
        out = np.empty((self.nby, self.nbx, SLOTS), np.int64)
        fa, fb, fc, fd = self.frames
        self.ctx.call("rip_cal_corr_pair", a, _native.location_of(a), b, _native.location_of(b), nreads, ny_file, nx_file, bool(fits_be16),
                      fa, fb, fc, fd, self.ny, self.nx, self.nb, self.sy, self.sx, out, _native.RIP_HOST)
        self.tables.append(out)
        return out

    def table(self):
        """int64 (npairs, nby, nbx, 25): the sums of every pair added, in the order they were added"""
        return np.stack(self.tables) if self.tables else np.empty((0, self.nby, self.nbx, SLOTS), np.int64)


def frame_times(frames, timeref):
    """``t_k = (k + 1) - TIMEREF`` in frames for the four 0-based frames"""
    return tuple(float(k + 1) - float(timeref) for k in frames)


def _moments(tab):
    """The pooled second moments and rates of one set, per superpixel: ``tab`` (npairs, nby, nbx, 25).  Returns ``(V, C, U, nmin,
    ok)``: V (nby, nbx), C (4, nby, nbx) in the order ``SHIFTS``, U (3, nby, nbx) the mean CDS of (a,b), (c,d), (a,d) per exposure
    (not yet divided by the time), nmin the smallest kept count over the pairs, ok where at least one pair has n >= 2.  A pair takes
    part in V and U with weight n where n >= 2, in C_s with weight m where m >= 1; every pair's moments are taken about its own
    means (a pair's two exposures differ by their own lamp level)."""
    t = np.asarray(tab, np.float64)
    if t.ndim != 4 or t.shape[3] != SLOTS:
        raise ValueError(f"a table of (npairs, nby, nbx, {SLOTS}) sums is needed, not {t.shape}")
    with np.errstate(all="ignore"):
        n = t[..., 0]
        use = n >= 2
        w = np.where(use, n, 0.0)
        wsum = w.sum(axis=0)
        var = 0.5 * (t[..., 2] / n - (t[..., 1] / n) ** 2)
        V = np.where(use, w * var, 0.0).sum(axis=0) / wsum
        C = []
        for s in range(len(SHIFTS)):
            m, sp, sq, spq = (t[..., 3 + 4 * s + k] for k in range(4))
            mu = use & (m >= 1)
            mw = np.where(mu, m, 0.0)
            cov = 0.5 * (spq / m - (sp / m) * (sq / m))
            C.append(np.where(mu, mw * cov, 0.0).sum(axis=0) / mw.sum(axis=0))
        U = [np.where(use, t[..., 19 + k], 0.0).sum(axis=0) / (2.0 * wsum) for k in range(3)]
        nmin = n.min(axis=0) if t.shape[0] else np.zeros(t.shape[1:3])
    return V, np.stack(C), np.stack(U), nmin, wsum > 0


def solve_summary(light, dark, frames, timeref):
    """The summary table of one configuration, float64 (nby * nbx, 11), row ``iy * nbx + ix``: columns 0 X = ix, 1 Y = iy, 2 N (the
    smallest kept count over the light pairs), 3 the raw gain ``u_ad t_ad / V``, 4 ``g`` with ``F = 1``, 5 ``g``, 6 alphaH, 7
    alphaV, 8 beta, 9 I, 10 alphaD.  ``light``, ``dark``: (npairs, nby, nbx, 25) tables of ``CorrStack.table()`` (or their numpy
    restatement; any numeric dtype); ``frames`` the four 0-based frames, ``timeref`` ``TIMEREF``.

    Model: ``S = (Q' - beta Q'^2) / g`` with ``Q' = K * Q``, ``Q`` Poisson of rate ``I`` per frame, ``K`` 3 x 3 with alphaH beside,
    alphaV above and below, alphaD on the diagonals and ``k0 = 1 - 2 alphaH - 2 alphaV - 4 alphaD`` in the centre.  Per set: ``V
    = (sum e^2 / n - (sum e / n)^2) / 2``, ``C_s`` likewise from the pair sums, ``u_pq = sum cds(p,q) / (2n) / (t_q - t_p)``; light
    minus dark of each removes read noise, correlated noise and dark current.  With ``s1 = t_a + t_b``, ``s2 = t_c + t_d``: ``r =
    (u_ab s2 - u_cd s1) / (s2 - s1)`` is the rate at zero signal and ``b = (u_ab - u_cd) / ((s2 - s1) r)`` the curvature ``beta
    I``.  The couplings follow from ``rho_H = C_H / V``, ``rho_V = C_V / V``, ``rho_D = (C_D1 + C_D2) / (2V)`` by 32 steps from zero
    of ``S2 = k0^2 + 2 aH^2 + 2 aV^2 + 4 aD^2``, ``aH = (rho_H S2 - 4 aV aD) / (2 k0)``, ``aV = (rho_V S2 - 4 aH aD) / (2 k0)``,
    ``aD = (rho_D S2 - 2 aH aV) / (2 k0)`` (the autocorrelation of K at the four shifts).  ``F = (1 - 2 b t_d)^2 + 4 b^2 t_ad
    t_a`` is the variance of a non-linear CDS over that of a linear one; ``g = r t_ad S2 F / V``, ``I = r g``, ``beta = b / I``.
    A superpixel where V, r, g or k0 is not positive and finite, or where no light or no dark pair has n >= 2, has N = 0 and
    zeros in the columns 3 .. 10; ``make_gain_file`` fills it with the array mean."""
    fa, fb, fc, fd = check_frames(frames)
    ta, tb, tc, td = frame_times((fa, fb, fc, fd), timeref)
    s1, s2 = ta + tb, tc + td
    if s1 == s2:
        raise ValueError(f"TIME {fa + 1} {fb + 1} {fc + 1} {fd + 1}: a + b = c + d leaves the curvature undetermined")
    VL, CL, UL, nmin, okL = _moments(light)
    VD, CD, UD, _, okD = _moments(dark)
    if VL.shape != VD.shape:
        raise ValueError(f"light and dark tables have {VL.shape} and {VD.shape} superpixels")
    nby, nbx = VL.shape
    tad = td - ta
    with np.errstate(all="ignore"):
        V, C, U = VL - VD, CL - CD, UL - UD
        uab, ucd, uad = U[0] / (tb - ta), U[1] / (td - tc), U[2] / tad
        r = (uab * s2 - ucd * s1) / (s2 - s1)
        b = (uab - ucd) / ((s2 - s1) * r)
        rho = (C[0] / V, C[1] / V, (C[2] + C[3]) / (2.0 * V))
        aH, aV, aD = np.zeros_like(V), np.zeros_like(V), np.zeros_like(V)
        for _ in range(IPC_STEPS):
            k0 = 1.0 - 2.0 * aH - 2.0 * aV - 4.0 * aD
            S2 = k0 * k0 + 2.0 * aH * aH + 2.0 * aV * aV + 4.0 * aD * aD
            aH, aV, aD = ((rho[0] * S2 - 4.0 * aV * aD) / (2.0 * k0), (rho[1] * S2 - 4.0 * aH * aD) / (2.0 * k0),
                          (rho[2] * S2 - 2.0 * aH * aV) / (2.0 * k0))
        k0 = 1.0 - 2.0 * aH - 2.0 * aV - 4.0 * aD
        S2 = k0 * k0 + 2.0 * aH * aH + 2.0 * aV * aV + 4.0 * aD * aD
        F = (1.0 - 2.0 * b * td) ** 2 + 4.0 * b * b * tad * ta
        graw = uad * tad / V
        g1 = r * tad * S2 / V
        g = g1 * F
        I = r * g
        beta = b / I
        good = okL & okD
        for q in (V, r, g, k0):
            good &= np.isfinite(q) & (q > 0)
        for q in (graw, g1, aH, aV, aD, beta, I):
            good &= np.isfinite(q)
    iy, ix = np.divmod(np.arange(nby * nbx), nbx)
    out = np.zeros((nby * nbx, NCOL))
    out[:, 0], out[:, 1] = ix, iy
    cols = {2: nmin, 3: graw, 4: g1, 5: g, 6: aH, 7: aV, 8: beta, 9: I, 10: aD}
    gd = good.ravel()
    for c, q in cols.items():
        out[:, c] = np.where(gd, q.ravel(), 0.0)
    return out
