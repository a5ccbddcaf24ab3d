"""numpy restatement of ``rip_cal_corr_pair`` (csrc/corrstat.hip), a numpy generator of the forward model that
``calfiles.corrstack.solve_summary`` inverts, and the standard errors of its results from planted values.  Test infrastructure,
independent of the library: nothing here calls it but ``standard_errors``, which differentiates ``solve_summary`` numerically.
"""

import numpy as np

SLOTS = 25
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))


def native(cube, fits_be16):
    """the unsigned samples of a cube as stored: native uint16, or FITS storage (big-endian int16 with BZERO = 32768)"""
    if not fits_be16:
        return np.asarray(cube, np.uint16)
    return (np.asarray(cube).view(">i2").astype(np.int32) + 32768).astype(np.uint16)


def to_fits_storage(cube):
    """uint16 samples as the big-endian int16 words of a FITS file with BZERO = 32768"""
    return (np.asarray(cube, np.int32) - 32768).astype(">i2")


def pair_table(cube1, cube2, frames, ny, nx, nb, sy, sx):
    """int64 (ny/sy, nx/sx, 25): every slot as include/romanhip.h states it, with np.sort for the ranks and int64 arithmetic"""
    fa, fb, fc, fd = frames
    S1 = np.asarray(cube1)[[fa, fb, fc, fd], :ny, :nx].astype(np.int64)
    S2 = np.asarray(cube2)[[fa, fb, fc, fd], :ny, :nx].astype(np.int64)
    e = (S1[3] - S1[0]) - (S2[3] - S2[0])
    cds = ((S1[1] - S1[0]) + (S2[1] - S2[0]), (S1[3] - S1[2]) + (S2[3] - S2[2]), (S1[3] - S1[0]) + (S2[3] - S2[0]))
    inside = np.zeros((ny, nx), bool)
    inside[nb:max(ny - nb, nb), nb:max(nx - nb, nb)] = True
    out = np.zeros((ny // sy, nx // sx, SLOTS), np.int64)
    for iy in range(ny // sy):
        for ix in range(nx // sx):
            sl = (slice(iy * sy, (iy + 1) * sy), slice(ix * sx, (ix + 1) * sx))
            ee, v = e[sl], inside[sl]
            n0 = int(v.sum())
            if n0 == 0:
                continue
            srt = np.sort(ee[v])
            q25, q50, q75 = (int(srt[(n0 - 1) // 4]), int(srt[(n0 - 1) // 2]), int(srt[3 * (n0 - 1) // 4]))
            kept = v & (np.abs(ee - q50) * 1349 <= 5000 * (q75 - q25))
            o = out[iy, ix]
            o[0], o[1], o[2] = kept.sum(), ee[kept].sum(), (ee[kept] * ee[kept]).sum()
            for s, (dy, dx) in enumerate(SHIFTS):
                py = slice(0, sy - dy)
                qy = slice(dy, sy)
                px, qx = {1: (slice(0, sx - 1), slice(1, sx)), 0: (slice(0, sx), slice(0, sx)), -1: (slice(1, sx), slice(0, sx - 1))}[dx]
                both = kept[py, px] & kept[qy, qx]
                ep, eq = ee[py, px][both], ee[qy, qx][both]
                o[3 + 4 * s: 7 + 4 * s] = both.sum(), ep.sum(), eq.sum(), (ep * eq).sum()
            for k in range(3):
                o[19 + k] = cds[k][sl][kept].sum()
            o[22], o[23], o[24] = q25, q50, q75
    return out


# ---- the forward model ----------------------------------------------------------------------------------------------------
def ipc(Q, aH, aV, aD):
    """Q' = K * Q with K = [[aD, aV, aD], [aH, k0, aH], [aD, aV, aD]], k0 = 1 - 2 aH - 2 aV - 4 aD; the coefficients are scalars or
    maps that are constant per superpixel; the frame is periodic, so that every pixel has the same statistics"""
    k0 = 1.0 - 2.0 * aH - 2.0 * aV - 4.0 * aD
    r = np.roll
    return (k0 * Q + aH * (r(Q, 1, 1) + r(Q, -1, 1)) + aV * (r(Q, 1, 0) + r(Q, -1, 0))
            + aD * (r(r(Q, 1, 0), 1, 1) + r(r(Q, 1, 0), -1, 1) + r(r(Q, -1, 0), 1, 1) + r(r(Q, -1, 0), -1, 1)))


def make_exposure(rng, nframes, ny, nx, rate, g, aH, aV, aD, beta, timeref=1, pedestal=5000.0, read_noise=7.0):
    """uint16 (nframes, ny, nx): frame k is read at t_k = (k + 1) - timeref frames after the reset.  Q: Poisson increments of
    ``rate`` electrons per frame; Q' = K * Q; S = (Q' - beta Q'^2) / g + pedestal + Gaussian read noise, rounded."""
    out = np.empty((nframes, ny, nx), np.uint16)
    Q = np.zeros((ny, nx))
    lam = np.broadcast_to(np.asarray(rate, np.float64), (ny, nx))
    for k in range(nframes):
        dt = (k + 1 - timeref) if k == 0 else 1
        if dt > 0:
            Q = Q + rng.poisson(lam * dt)
        Qp = ipc(Q, aH, aV, aD)
        S = (Qp - beta * Qp * Qp) / g + pedestal + read_noise * rng.standard_normal((ny, nx))
        out[k] = np.clip(np.rint(S), 0, 65535).astype(np.uint16)
    return out


# ---- expected sums and standard errors from planted values -----------------------------------------------------------------
def sigma2(aH, aV, aD):
    k0 = 1.0 - 2.0 * aH - 2.0 * aV - 4.0 * aD
    return k0 * k0 + 2.0 * aH * aH + 2.0 * aV * aV + 4.0 * aD * aD


def autocorr(aH, aV, aD):
    """the autocorrelation of K at the four shifts of SHIFTS"""
    k0 = 1.0 - 2.0 * aH - 2.0 * aV - 4.0 * aD
    d = 2.0 * k0 * aD + 2.0 * aH * aV
    return (2.0 * k0 * aH + 4.0 * aV * aD, 2.0 * k0 * aV + 4.0 * aH * aD, d, d)


def expected_moments(rate, g, aH, aV, aD, beta, read_noise, times):
    """(V, C[4], mean cds of (a,b), (c,d), (a,d)) of one exposure of the model: the shot noise of a non-linear CDS through the
    IPC kernel, plus twice the read variance and the rounding's 2/12 in V"""
    ta, tb, tc, td = times
    tad, b = td - ta, beta * rate
    F = (1.0 - 2.0 * b * td) ** 2 + 4.0 * b * b * tad * ta
    shot = rate * tad * F / (g * g)
    V = shot * sigma2(aH, aV, aD) + 2.0 * read_noise ** 2 + 1.0 / 6.0
    C = [shot * a for a in autocorr(aH, aV, aD)]

    def cds(p, q):
        return (rate * (q - p) - beta * rate * rate * (q * q - p * p)) / g

    return V, C, (cds(ta, tb), cds(tc, td), cds(ta, td))


def ideal_table(V, C, cds, n, m):
    """the float (1, 1, 1, 25) table of one superpixel whose moments are exactly V, C and cds: n kept pixels and m[s] pairs in all"""
    t = np.zeros((1, 1, 1, SLOTS))
    t[..., 0], t[..., 2] = n, 2.0 * V * n
    for s in range(4):
        t[..., 3 + 4 * s], t[..., 6 + 4 * s] = m[s], 2.0 * C[s] * m[s]
    for k in range(3):
        t[..., 19 + k] = 2.0 * n * cds[k]
    return t


def standard_errors(solve, light, dark, n, m, frames, timeref):
    """Standard errors of the columns of ``solve``'s table for one superpixel, from planted values.  ``light``, ``dark``: the
    ``expected_moments`` of the two sets; ``n``, ``m[4]``: the kept pixels and pairs of a set in all its exposure pairs.  The
    inputs' own errors: Gaussian se(V_X) = V_X sqrt(2 / n), se(C_X,s) = V_X / sqrt(m_s), and se of a mean CDS (2n samples)
    sqrt(V_X / (2n)) (V_X of the longest baseline, an upper bound for the shorter ones); they are taken as independent and
    propagated by central differences of one standard error.  Returns (table row at the planted moments, se per column)."""
    base = [list(light), list(dark)]

    def table(delta):
        sets = []
        for X in range(2):
            V, C, cds = base[X]
            V = V + delta.get((X, "V"), 0.0)
            C = [C[s] + delta.get((X, "C", s), 0.0) for s in range(4)]
            cds = [cds[k] + delta.get((X, "u", k), 0.0) for k in range(3)]
            sets.append(ideal_table(V, C, cds, n, m))
        return solve(sets[0], sets[1], frames, timeref)[0]

    var = np.zeros_like(table({}))
    for X in range(2):
        V = base[X][0]
        errs = {(X, "V"): V * np.sqrt(2.0 / n)}
        errs.update({(X, "C", s): V / np.sqrt(m[s]) for s in range(4)})
        errs.update({(X, "u", k): np.sqrt(V / (2.0 * n)) for k in range(3)})
        for key, se in errs.items():
            var += (0.5 * (table({key: se}) - table({key: -se}))) ** 2
    return table({}), np.sqrt(var)
