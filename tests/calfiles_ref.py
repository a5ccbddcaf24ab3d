"""Independent numpy restatement of the calibration-file derivation (the reference's runs/2026_July/postprocess_calfiles.py and
makemask.py), with every dtype written out instead of left to numpy's promotion rules: float32 planes, Python scalars cast to
float32 where numpy >= 2 treats them as weak.  tests/test_host_calfiles_ref.py holds it against the fixtures the reference's own
scripts produced (tests/golden/calfiles_*.npz); the GPU tests use it where no fixture exists."""

import numpy as np
from scipy.special import legendre_p

F = np.float32


def _lp(n, x):
    return np.reshape(legendre_p(n, x), np.shape(x))


def parse_reads(reads, bframe):
    """(list of (fr1, fr2), xref) -- postprocess_calfiles.py:115-131"""
    r = [int(v) for v in reads]
    ngrp = len(r) // 2
    groups = [(r[2 * j], r[2 * j + 1]) for j in range(ngrp)]
    xref = (groups[bframe][0] + groups[bframe][1] - 1) / 2.0
    return groups, xref


def invlinearity_f32(target, coefs, smin, smax):
    """ipc_linearity.invlinearity (ipc_linearity.py:347-394) on float32 planes: 24 bisection steps of the Legendre series without
    the extrapolation branch."""
    target = np.asarray(target, F)
    nplanes = coefs.shape[0]
    z = np.zeros_like(target)
    with np.errstate(all="ignore"):
        for j in range(1, 25):
            phi = coefs[0].astype(F, copy=True)
            prev = np.ones_like(z)
            poly = z.copy()
            for L in range(1, nplanes):
                phi = phi + coefs[L] * poly
                nxt = F((2 * L + 1) / (L + 1)) * z * poly - F(L / (L + 1)) * prev
                prev, poly = poly, nxt
            z = z + np.where(phi < target, F(1 / 2**j), F(-1 / 2**j))
        return smin + (smax - smin) / F(2.0) * (F(1) + z)


def biascorr(dark_slope, dark_data, coefs, smin, smax, reads, tframe=3.04, bframe=1, nb=4):
    """(biascorr, pred, t0) -- postprocess_calfiles.py:103-140"""
    groups, xref = parse_reads(reads, bframe)
    act = (slice(nb, dark_slope.shape[0] - nb), slice(nb, dark_slope.shape[1] - nb))
    c = np.ascontiguousarray(coefs[(slice(None),) + act])
    lo, hi = smin[act], smax[act]
    with np.errstate(all="ignore"):
        dark = dark_slope[act] * F(tframe)
        pred = np.zeros((len(groups),) + dark.shape, F)
        for j, (fr1, fr2) in enumerate(groups):
            for x in range(fr1, fr2):
                pred[j] = pred[j] + invlinearity_f32(dark * F(x - xref), c, lo, hi)
            pred[j] = pred[j] / F(fr2 - fr1)
        return dark_data[(slice(None),) + act] - pred, pred, tframe * xref


def medfit(arr, N, order):
    """(coef f64, model in arr's dtype) -- sky.py:100-191"""
    ny, nx = arr.shape
    kx, ky = nx // N, ny // N
    px, py = (nx % N) // 2, (ny % N) // 2
    uc = 2 * (px - 0.5 + kx * np.linspace(0.5, N - 0.5, N)) / nx - 1
    vc = 2 * (py - 0.5 + ky * np.linspace(0.5, N - 0.5, N)) / ny - 1
    u, v = np.meshgrid(uc, vc)
    with np.errstate(all="ignore"), __import__("warnings").catch_warnings():
        __import__("warnings").simplefilter("ignore")
        meds = np.nanmedian(arr[py:py + N * ky, px:px + N * kx].reshape(N, ky, N, kx), axis=(1, 3))
    pairs = [(i, j) for i in range(order + 1) for j in range(order + 1 - i)]
    basis = np.stack([_lp(i, u) * _lp(j, v) for i, j in pairs])
    A, b = np.zeros((len(pairs),) * 2), np.zeros(len(pairs))
    for ix in range(N):
        for iy in range(N):
            if not np.isnan(meds[iy, ix]):
                A += np.outer(basis[:, iy, ix], basis[:, iy, ix])
                b += meds[iy, ix] * basis[:, iy, ix]
    coef = np.linalg.solve(A, b)
    LPX = [_lp(i, np.linspace(-1, 1 - 2 / nx, nx)) for i in range(order + 1)]
    LPY = [_lp(j, np.linspace(-1, 1 - 2 / ny, ny)) for j in range(order + 1)]
    model = np.zeros((ny, nx))
    for k, (i, j) in enumerate(pairs):
        model += coef[k] * np.outer(LPY[j], LPX[i])
    return coef, model.astype(arr.dtype)


def pflat(pflat0, gain, g_ideal):
    """(data, dq, coef) -- postprocess_calfiles.py:22-40"""
    coef, model = medfit(pflat0, 6, 2)
    with np.errstate(all="ignore"):
        p = pflat0 / model
        p = p * (F(g_ideal) / np.median(gain))
        dq = ((p < F(0.01)) | (p > F(1.99))).astype(np.uint32)
        return np.clip(p, F(0.01), F(1.99)), dq, coef


def saturation(smax, sref):
    """(data, dq) -- postprocess_calfiles.py:69-97"""
    return np.clip(smax, F(1), F(65535)) - F(1), np.where(smax > sref, 0, 1).astype(np.uint32)


def mask(lin_dq, pflat0, dark_slope, gain_dq, nb=4):
    """makemask.py:12-36"""
    dq = np.zeros(pflat0.shape, np.uint32)
    for sl in ((slice(None, nb), slice(None)), (slice(-nb, None), slice(None)), (slice(None), slice(None, nb)),
               (slice(None), slice(-nb, None))):
        dq[sl] |= np.uint32(2**31)
    with np.errstate(all="ignore"):
        rel = pflat0 / np.median(pflat0)
        dq |= lin_dq
        dq |= np.where(rel < F(0.5), 2**13, 0).astype(np.uint32)
        dq |= np.where(dark_slope > F(0.25), np.where(dark_slope > F(12.5), 2**11, 2**12), 0).astype(np.uint32)
    dq |= gain_dq
    return dq
