"""numpy restatement of ``csrc/linfit.hip``: the frame sums of a ramp set (``frame_sums``) and the constrained Legendre fit of the
linearity curve (``fit``), the rule of ``rip_cal_linearity_fit`` in ``include/romanhip.h`` and DESIGN.md section 7.

Every float64 operation of the kernel is done here in the kernel's order, vectorised over the pixels: one ``+ - * /`` or
``sqrt`` per statement, masks where the kernel branches (a sample the kernel skips is added here as ``+ 0.0``, which changes no
sum that started at +0.0), one rounding to float32 or to an integer at the end.  No libm function takes part, so the two agree
bit for bit.
"""

import numpy as np

NO_LIN_CORR = np.uint32(1 << 20)
REFERENCE_PIXEL = np.uint32(1 << 31)
MAX_SETS = 8
MAX_ORDER = 10


def decode(cube, fits_be16=False):
    """the unsigned samples of a cube: native uint16, or FITS storage (big-endian int16 with BZERO 32768) held in 16-bit words"""
    w = np.asarray(cube).view(np.uint16) if np.asarray(cube).dtype.itemsize == 2 else np.asarray(cube)
    if fits_be16:
        w = w.byteswap() ^ np.uint16(0x8000)
    return w


def frame_sums(sums, cube, f0=0, rows=None, nx=None, fits_be16=False):
    """``sums[f - f0, y - y0, x] += cube[f, y, x]`` as uint32, in place, for the frames from ``f0``, the rows ``rows`` and the
    first ``nx`` columns"""
    y0, y1 = (0, cube.shape[1]) if rows is None else rows
    nx = sums.shape[2] if nx is None else nx
    sums += decode(cube, fits_be16)[f0:, y0:y1, :nx].astype(np.uint32)
    return sums


def legendre(z, p):
    """P_l(z) and P_l'(z), l = 0 .. p, by the three-term recurrences in the kernel's order"""
    one = np.ones_like(z)
    P, dP = [one, z], [np.zeros_like(z), one]
    for l in range(2, p + 1):
        t1 = (float(2 * l - 1) * z) * P[l - 1]
        t2 = float(l - 1) * P[l - 2]
        P.append((t1 - t2) / float(l))
        dP.append(dP[l - 2] + float(2 * l - 1) * P[l - 1])
    return P[:p + 1], dP[:p + 1]


def _basis(Mi, smin, h, zref, Pr, dPr, p):
    """B_2 .. B_p at the samples ``Mi``"""
    z = (Mi - smin) / h - 1.0
    P, _ = legendre(z, p)
    dz = z - zref
    return [(P[l] - Pr[l]) - dPr[l] * dz for l in range(2, p + 1)]


def fit(sums, counts, first, sref, *, p_order, tframe=3.04, slopecut=0.5, negativepad=500.0, nb=4, bright=0, dark=-1):
    """``sums``: per set a uint32 (frames, ny, nx) array; ``counts``: exposures per set; ``first``: first frame used per set
    (``TSTART - 1``).  Returns the planes of ``rip_cal_linearity_fit`` as a dict of numpy arrays."""
    K, p = len(sums), int(p_order)
    m = p - 1
    tframe, slopecut, negativepad = float(tframe), float(slopecut), float(negativepad)
    sref32 = np.ascontiguousarray(sref, dtype=np.float32)
    ny, nx = sref32.shape
    with np.errstate(all="ignore"):
        M = [np.asarray(s).astype(np.float64) / float(n) for s, n in zip(sums, counts)]
        nf = [a.shape[0] for a in M]
        F = [nf[k] - first[k] for k in range(K)]
        sr = sref32.astype(np.float64)
        ok = np.isfinite(sr)
        t = sr - negativepad
        smin32 = np.where(ok & (t > 0.0), t, 0.0).astype(np.float32)
        # the range of the bright set
        Mb, i0 = M[bright], first[bright]
        n0 = min(4, F[bright] - 1)
        D0 = (Mb[i0 + n0] - Mb[i0]) / float(n0)
        thr = slopecut * D0
        cut = np.full((ny, nx), i0 + F[bright] - 1, np.int32)
        found = np.zeros((ny, nx), bool)
        for i in range(i0, i0 + F[bright] - 1):
            hit = ~found & ((Mb[i + 1] - Mb[i]) < thr)
            cut[hit] = i
            found |= hit
        Mc = np.take_along_axis(Mb, cut[None].astype(np.int64), axis=0)[0]
        v = np.where(Mc < 65535.0, Mc, 65535.0)
        smax32 = v.astype(np.float32)
        up = smax32.astype(np.float64) < v   # Smax is the sample at the cut rounded UP to f32, so that the sample is in range
        smax32 = np.where(up, np.nextafter(smax32, np.float32(np.inf)), smax32).astype(np.float32)
        smin, smax = smin32.astype(np.float64), smax32.astype(np.float64)
        h = (smax - smin) / 2.0
        zref = (sr - smin) / h - 1.0
        bad = ~(D0 > 0.0) | ~ok | (sr >= smax) | ~(smax > smin)
        Pr, dPr = legendre(zref, max(p, 1))

        def used_mask(k, i):
            u = (M[k][i] >= smin) & (M[k][i] <= smax)
            return u & (i <= cut) if k == bright else u

        def uval(k, i):
            return float(2 * (i - first[k])) / float(F[k] - 1) - 1.0

        # pass 0: the used samples of every set; a set with fewer than two takes no part
        nused = []
        for k in range(K):
            c = np.zeros((ny, nx), np.int32)
            for i in range(first[k], nf[k]):
                c += used_mask(k, i)
            nused.append(c)
        part = [c >= 2 for c in nused]
        dof = np.zeros((ny, nx), np.int32)
        for k in range(K):
            dof += np.where(part[k], nused[k] - 2, 0)
        bad |= dof < m

        # pass 1: the normal matrix (lower triangle) and right-hand side with [1, u] projected out per set
        zero = np.zeros((ny, nx))
        N = [[zero.copy() for _ in range(a + 1)] for a in range(m)]
        c = [zero.copy() for _ in range(m)]
        for k in range(K):
            S1, Su, Suu, Sy, Suy = (zero.copy() for _ in range(5))
            s, tt = [zero.copy() for _ in range(m)], [zero.copy() for _ in range(m)]
            for i in range(first[k], nf[k]):
                sel = used_mask(k, i) & part[k]   # the kernel skips the other samples: adding +0.0 changes no sum
                u = uval(k, i)
                y = np.where(sel, M[k][i] - sr, 0.0)
                B = [np.where(sel, b, 0.0) for b in _basis(M[k][i], smin, h, zref, Pr, dPr, p)]
                S1 = S1 + np.where(sel, 1.0, 0.0)
                Su = Su + np.where(sel, u, 0.0)
                Suu = Suu + np.where(sel, u * u, 0.0)
                Sy = Sy + y
                Suy = Suy + u * y
                for a in range(m):
                    s[a] = s[a] + B[a]
                    tt[a] = tt[a] + u * B[a]
                    c[a] = c[a] + B[a] * y
                    for b in range(a + 1):
                        N[a][b] = N[a][b] + B[a] * B[b]
            det = S1 * Suu - Su * Su
            ay = (Suu * Sy - Su * Suy) / det
            by = (S1 * Suy - Su * Sy) / det
            for a in range(m):
                al = (Suu * s[a] - Su * tt[a]) / det
                be = (S1 * tt[a] - Su * s[a]) / det
                c[a] = np.where(part[k], c[a] - (s[a] * ay + tt[a] * by), c[a])
                for b in range(a, m):   # column a of the lower triangle
                    N[b][a] = np.where(part[k], N[b][a] - (s[b] * al + tt[b] * be), N[b][a])

        # Cholesky, forward and back substitution
        L = [[None] * m for _ in range(m)]
        for j in range(m):
            d = N[j][j]
            for q in range(j):
                d = d - L[j][q] * L[j][q]
            bad |= ~((d > 0.0) & (d < np.inf))
            L[j][j] = np.sqrt(d)
            for i in range(j + 1, m):
                e = N[i][j]
                for q in range(j):
                    e = e - L[i][q] * L[j][q]
                L[i][j] = e / L[j][j]
        yv = [None] * m
        for j in range(m):
            e = 0.0 - c[j]
            for q in range(j):
                e = e - L[j][q] * yv[q]
            yv[j] = e / L[j][j]
        qv = [None] * m
        for j in range(m - 1, -1, -1):
            e = yv[j]
            for q in range(j + 1, m):
                e = e - L[q][j] * qv[q]
            qv[j] = e / L[j][j]

        # the stored coefficients
        sumA, sumB = zero.copy(), zero.copy()
        for a in range(m):
            sumA = sumA + qv[a] * dPr[a + 2]
            sumB = sumB + qv[a] * (Pr[a + 2] - dPr[a + 2] * zref)
        c1 = h - sumA
        c0 = (0.0 - h * zref) - sumB

        # pass 2 and 3 per set: a_k, r_k by regression of phi(M) on [1, u]; the largest residual
        rate, err = [], []
        for k in range(K):
            S1, Su, Suu, Sw, Suw = (zero.copy() for _ in range(5))
            W = {}
            for i in range(first[k], nf[k]):
                sel = used_mask(k, i) & part[k]
                u = uval(k, i)
                B = _basis(M[k][i], smin, h, zref, Pr, dPr, p)
                ph = M[k][i] - sr
                for a in range(m):
                    ph = ph + qv[a] * B[a]
                W[i] = ph
                ph = np.where(sel, ph, 0.0)
                S1 = S1 + np.where(sel, 1.0, 0.0)
                Su = Su + np.where(sel, u, 0.0)
                Suu = Suu + np.where(sel, u * u, 0.0)
                Sw = Sw + ph
                Suw = Suw + u * ph
            det = S1 * Suu - Su * Su
            ak = (Suu * Sw - Su * Suw) / det
            rk = (S1 * Suw - Su * Sw) / det
            e = zero.copy()
            for i in range(first[k], nf[k]):
                res = np.abs(W[i] - (ak + rk * uval(k, i)))
                e = np.where(used_mask(k, i) & part[k] & (res > e), res, e)
            rate.append(np.where(part[k], (rk * 2.0) / (float(F[k] - 1) * tframe), 0.0))
            err.append(np.where(e < 65535.0, np.ceil(e), 65535.0))

        border = np.zeros((ny, nx), bool)
        if nb > 0:
            border[:nb] = border[-nb:] = True
            border[:, :nb] = border[:, -nb:] = True
        flagged = bad | border
        data = np.zeros((p + 1, ny, nx), np.float32)
        data[0] = np.where(flagged, (smin + smax) / 2.0 - sr, c0).astype(np.float32)
        data[0][~ok] = np.array([0x7FC00000], np.uint32).view(np.float32)[0]   # Sref not finite: the one quiet NaN
        data[1] = np.where(flagged, h, c1).astype(np.float32)
        for a in range(m):
            data[a + 2] = np.where(flagged, 0.0, qv[a]).astype(np.float32)
        rdark = rate[dark] if dark >= 0 else zero
        lit = [k for k in range(K) if k != dark]   # dark: an index 0 .. K-1, or -1 for none
        pflat = np.zeros((len(lit), ny, nx), np.float32)
        for j, k in enumerate(lit):
            pflat[j] = np.where(flagged | ~part[k], 0.0, rate[k] - rdark).astype(np.float32)
        ramperr = np.zeros((K, ny, nx), np.uint16)
        for k in range(K):
            ramperr[k] = np.where(flagged | ~part[k], 0.0, err[k]).astype(np.uint16)
        dq = np.where(border, REFERENCE_PIXEL, np.where(bad, NO_LIN_CORR, np.uint32(0))).astype(np.uint32)
        dk = np.where(flagged, 0.0, rdark).astype(np.float32)
    return {"data": data, "Smin": smin32, "Smax": smax32, "dq": dq, "pflat": pflat, "dark": dk, "ramperr": ramperr, "cut": cut,
            "nused": nused, "dof": dof, "D0": D0}


def evaluate(data, smin, smax, S):
    """the stored series at the signal ``S``, in float64: sum of c_l P_l(z), z = 2 (S - Smin) / (Smax - Smin) - 1"""
    smin, smax = np.asarray(smin, np.float64), np.asarray(smax, np.float64)
    z = (np.asarray(S, np.float64) - smin) / ((smax - smin) / 2.0) - 1.0
    P, _ = legendre(z, max(data.shape[0] - 1, 1))
    return sum(np.asarray(data[l], np.float64) * P[l] for l in range(data.shape[0]))


def derivative(data, smin, smax, S):
    """d phi / d S of the stored series at ``S``, in float64"""
    smin, smax = np.asarray(smin, np.float64), np.asarray(smax, np.float64)
    h = (smax - smin) / 2.0
    z = (np.asarray(S, np.float64) - smin) / h - 1.0
    _, dP = legendre(z, max(data.shape[0] - 1, 1))
    return sum(np.asarray(data[l], np.float64) * dP[l] for l in range(data.shape[0])) / h
