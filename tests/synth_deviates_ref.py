"""Plain numpy / f64 restatement of the deviates that make Level-1 exposures (DESIGN.md "Shared device headers", rows 6 to 11):
``synth.hip``'s small-mean increments, ``riprng::poisson_ptrs``, ``riprng::binomial``, ``riprng::normal_f32`` under the tags
0x12 .. 0x15, and ``cr.hip``'s ``poisson_any`` and track uniforms.  Built on ``philox_ref.block``; shared by
``test_host_synth_deviates.py`` (CPU) and ``test_gpu_synth_deviates.py`` (GPU).  Test infrastructure only.

Two kinds of answers.  Where the device works in f64 the restatement replays it step for step and returns ``(k, sure)`` in the
manner of ``philox_ref.device_poisson``: ``sure`` is False where a uniform lies so close to a decision that the device's own
exp / log / lgamma / reciprocal may decide the other way.  Where the device works in f32 (the sequential search of the small
means) the answer is an interval of counts around the f64 quantile, not a replay of the f32 chain."""

import numpy as np
from scipy import special

import philox_ref
from philox_ref import block

TAG_TOTAL, TAG_SHARE, TAG_RESET, TAG_READ, TAG_FILL, TAG_WHITE33 = 0x10, 0x11, 0x12, 0x13, 0x14, 0x15
TAG_CR_COUNT, TAG_CR_TRACK, TAG_CR_DEPOSIT = 0x20, 0x21, 0x22
DOM_SMALL, DOM_PTRS, DOM_BINV, DOM_BTRS = 0x706F6934, 0x70747232, 0x62696E31, 0x62747273
DOM_NORMAL, DOM_CR_POIS, DOM_CR_TRACK = 0x6C317379, 0x63727069, 0x6372746B

# Half-width of the band of uniforms around u inside which the f32 search may stop: the chain has at most 41 partial sums <= 1,
# each erring by at most 2^-25 (20.5 * 2^-24); the relative error of p_k grows by about 2.5 ulp a step and enters weighted by
# p_k: about 25 * 2^-24 at a mean of 10; a few ulp of __expf on every term.  Sum < 64 * 2^-24.  Derived, not tuned.
M_SMALL = 64.0 * 2.0 ** -24
U_TOP = 1.0 - 2.0 ** -32      # the finest tail a 32-bit Philox word can justify: upper end of the interval of the top bins
MARGIN = 1e-9                 # the band around an f64 decision (philox_ref.device_poisson's)
COUNT_MAX = 2.0e9


def _u53(hi, lo):
    return (((hi << np.uint64(21)) | (lo >> np.uint64(11))).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def _u32(w):
    return (w.astype(np.float64) + 0.5) * (1.0 / 4294967296.0)


# ------------------------------------------------------------------------------------------ the host's share table
def share_table(t_reads):
    """p, w, sqrt(w), log(w) per read as ``rip_synth_apportion`` computes them on the host, and ``eff``: the read whose table is
    in force at read r (``apportion_poisson_pixel`` keeps lam, the cdf table and the PtrsPlan while the share moves by no more
    than 1e-12 relative)."""
    t = [float(x) for x in t_reads]
    n, t_end, t_prev = len(t), float(t_reads[-1]), 0.0
    p, w = np.zeros(n), np.zeros(n)
    for r in range(n):
        left = t_end - t_prev
        pr = (t[r] - t_prev) / left if left > 0.0 else 1.0
        p[r] = min(max(pr, 0.0), 1.0)
        wr = (t[r] - t_prev) / t_end if t_end > 0.0 else (1.0 if r == n - 1 else 0.0)
        w[r] = max(wr, 0.0)
        t_prev = t[r]
    eff, w_prev, at = np.zeros(n, dtype=np.int64), -1.0, 0
    for r in range(n):
        if abs(w[r] - w_prev) > 1e-12 * w_prev:
            w_prev, at = w[r], r
        eff[r] = at
    with np.errstate(divide="ignore"):
        lw = np.where(w > 0.0, np.log(np.where(w > 0.0, w, 1.0)), 0.0)
    return {"p": p, "w": w, "sw": np.sqrt(w), "lw": lw, "eff": eff}


def clip_counts(counts):
    """the f32 counts as the kernels take them: f64, clipped to [0, 2e9]; NaN draws nothing"""
    c = np.asarray(counts, dtype=np.float32).astype(np.float64).ravel()
    return np.where(np.isnan(c), 0.0, np.clip(c, 0.0, COUNT_MAX))


# ------------------------------------------------------------------------------------------ small means: the f32 search
def small_bits(seed, pix, nreads):
    """(nreads, npix) the 23-bit value of every (pixel, read): counter {pixel, r & ~3, 0x10, 0x706f6934}, word r & 3, >> 9"""
    pix = np.asarray(pix, dtype=np.uint64)
    out = np.zeros((nreads, pix.size), dtype=np.uint64)
    for r0 in range(0, nreads, 4):
        blk = block(seed, pix, r0, TAG_TOTAL, DOM_SMALL)
        for q in range(min(4, nreads - r0)):
            out[r0 + q] = blk[:, q] >> np.uint64(9)
    return out


def small_uniform(bits):
    """u = ((w >> 9) * 2 + 1) * 2^-24: exact in f32, in (0, 1), at most 1 - 2^-24"""
    return (np.asarray(bits).astype(np.float64) * 2.0 + 1.0) * 2.0 ** -24


def poisson_ppf(q, lam):
    """smallest k with cdf(k; lam) >= q in f64 (scipy.stats.poisson.ppf; 0 for q <= 0), elementwise, by a table of the
    regularised incomplete gamma function per distinct mean -- a frame has few of them"""
    q, lam = np.broadcast_arrays(np.asarray(q, dtype=np.float64), np.asarray(lam, dtype=np.float64))
    out = np.zeros(q.shape)
    ks = np.arange(0, 200, dtype=np.float64)
    for m in np.unique(lam):
        sel = lam == m
        out[sel] = np.searchsorted(special.pdtr(ks, m), q[sel], side="left")
    return out


def small_interval(u, lam):
    """(lo, hi): the counts an f32 search of the documented recipe may return for the uniform u"""
    lo = poisson_ppf(np.maximum(u - M_SMALL, 0.0), lam)
    hi = poisson_ppf(np.minimum(u + M_SMALL, U_TOP), lam)
    return lo, hi


# ------------------------------------------------------------------------------------------ riprng::poisson_ptrs
def _ptrs_candidate(u, v, lam, loglam, aa, bb, inv_alpha, vr, margin):
    us = 0.5 - np.abs(u)
    r = 1.0 / us                       # the device: hardware reciprocal + one Newton step, not the quotient
    arg = (2.0 * aa * r + bb) * u + lam + 0.43
    k = np.floor(arg)
    scale = np.abs(2.0 * aa * r * u) + np.abs(bb * u) + lam + 1.0
    sure = np.abs(arg - np.rint(arg)) > 1e-12 * scale
    sure &= (np.abs(us - 0.07) >= margin) & (np.abs(v - vr) >= margin)
    acc1 = (us >= 0.07) & (v <= vr)
    s2 = (np.abs(us - 0.013) >= margin) & (np.abs(v - us) >= margin)
    rej = (k < 0.0) | ((us < 0.013) & (v > us))
    kk = np.where(k < 0.0, 0.0, k)
    lhs = np.log(v * inv_alpha / (aa * (r * r) + bb))
    rhs = -lam + kk * loglam - special.gammaln(kk + 1.0)
    # the device's log(c) + log(w) and log k! are a few ulp of their magnitude off these
    s3 = np.abs(lhs - rhs) >= margin + 8.0 * np.spacing(np.abs(kk * loglam) + lam)
    acc = acc1 | (~rej & (lhs <= rhs))
    return acc, k, sure & (acc1 | (s2 & (rej | s3)))


def poisson_ptrs(lam, slam, loglam, seed, a, b, tag, margin=MARGIN):
    """(k, sure) of ``riprng::poisson_ptrs`` for plans made by ``ptrs_plan(lam, slam, loglam)``: counter {a, b, tag ^
    attempt << 24, 0x70747232}, candidates (u, v) from words 0, 1 then 2, 3, 32 attempts.  The f32 pre-test of the device gets
    no margin: it claims to decide only outside its error band, so the device must equal the f64 decision made here."""
    lam, slam, loglam, a, b = (np.ravel(x) for x in np.broadcast_arrays(
        np.asarray(lam, dtype=np.float64), np.asarray(slam, dtype=np.float64), np.asarray(loglam, dtype=np.float64),
        np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)))
    bb = 0.931 + 2.53 * slam
    aa = -0.059 + 0.02483 * bb
    inv_alpha = 1.1239 + 1.1328 / (bb - 3.4)
    vr = 0.9277 - 3.6224 / (bb - 2.0)
    k_out, sure = np.floor(lam + 0.5), np.ones(lam.size, dtype=bool)
    pending = np.ones(lam.size, dtype=bool)
    for attempt in range(32):
        idx = np.nonzero(pending)[0]
        if idx.size == 0:
            break
        blk = block(seed, a[idx], b[idx], tag ^ (attempt << 24), DOM_PTRS)
        for iu, iv in ((0, 1), (2, 3)):
            live = pending[idx]
            j, bl = idx[live], blk[live]
            if j.size == 0:
                break
            acc, k, s = _ptrs_candidate(_u32(bl[:, iu]) - 0.5, _u32(bl[:, iv]), lam[j], loglam[j], aa[j], bb[j], inv_alpha[j],
                                        vr[j], margin)
            sure[j] &= s
            k_out[j[acc]] = k[acc]
            pending[j[acc]] = False
    return k_out, sure


# ------------------------------------------------------------------------------------------ rip_synth_apportion, Poisson
class PoissonFrame:
    """What ``rip_synth_apportion(poisson = 1)`` may write for ``counts`` (flat), read times ``t_reads`` and ``seed``:
    per (read, pixel) the interval [lo, hi] of the increment, ``small`` (f32 search) and ``sure`` (rejection reads; True on
    small reads).  ``pix``: the pixel indices of ``counts`` in the frame (default 0 .. n-1)."""

    def __init__(self, counts, t_reads, seed, pix=None):
        c = clip_counts(counts)
        tab = share_table(t_reads)
        nreads = len(tab["w"])
        pix = np.arange(c.size, dtype=np.uint64) if pix is None else np.asarray(pix, dtype=np.uint64)
        eff = tab["eff"]
        lam = c[None, :] * tab["w"][eff][:, None]
        self.lam = lam
        self.small = (lam > 0.0) & (lam < 10.0)
        self.lo, self.hi = np.zeros(lam.shape), np.zeros(lam.shape)
        self.sure = np.ones(lam.shape, dtype=bool)
        self.u = small_uniform(small_bits(seed, pix, nreads))
        if self.small.any():
            lo, hi = small_interval(self.u[self.small], lam[self.small])
            self.lo[self.small], self.hi[self.small] = lo, hi
        big = (lam >= 10.0)
        if big.any():
            with np.errstate(divide="ignore"):
                sc, lc = np.sqrt(c), np.where(c > 0.0, np.log(np.where(c > 0.0, c, 1.0)), 0.0)
            rr, pp = np.nonzero(big)
            k, s = poisson_ptrs(lam[big], sc[pp] * tab["sw"][eff][rr], lc[pp] + tab["lw"][eff][rr], seed, pix[pp], rr, TAG_TOTAL)
            self.lo[big] = self.hi[big] = k
            self.sure[big] = s
        self.pinned = self.sure & (self.lo == self.hi)

    def check(self, out, sentinel=None):
        """``out`` (nreads, npix) int32 from the device: every increment inside its interval (read by read while the running
        sum is below the clip at 2e9), and the running sum itself wherever every read so far is pinned.  Returns the number of
        increments compared."""
        out = np.asarray(out).reshape(self.lo.shape).astype(np.float64)
        if sentinel is not None:
            assert not np.any(out == sentinel), "%d values never written" % np.count_nonzero(out == sentinel)
        d = np.diff(out, axis=0, prepend=0.0)
        open_ = (out < COUNT_MAX) & self.sure
        bad = open_ & ((d < self.lo) | (d > self.hi))
        if bad.any():
            r, p = np.argwhere(bad)[0]
            raise AssertionError("%d of %d increments outside their interval; first at read %d, pixel %d: %g not in [%g, %g], "
                                 "mean %.9g, u %.9g" % (np.count_nonzero(bad), np.count_nonzero(open_), r, p, d[r, p],
                                                        self.lo[r, p], self.hi[r, p], self.lam[r, p], self.u[r, p]))
        prefix = np.logical_and.accumulate(self.pinned, axis=0)
        want = np.minimum(np.cumsum(self.lo, axis=0), COUNT_MAX)
        bad = prefix & (out != want)
        if bad.any():
            r, p = np.argwhere(bad)[0]
            raise AssertionError("running sum differs at read %d, pixel %d: %g, expected %g" % (r, p, out[r, p], want[r, p]))
        return int(np.count_nonzero(open_))


# ------------------------------------------------------------------------------------------ riprng::binomial
def binomial(n, p, seed, a, b, tag, margin=MARGIN):
    """(k, sure) of ``riprng::binomial(n, p, seed, a, b, tag)`` elementwise: inversion under 0x62696e31 (u53 of words 0, 1)
    where n min(p, 1-p) < 10, else BTRS under 0x62747273 (u53 pairs, 64 attempts, lgamma test)."""
    n, p, a, b = (np.ravel(x) for x in np.broadcast_arrays(np.asarray(n, dtype=np.int64), np.asarray(p, dtype=np.float64),
                                                          np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)))
    k_out, sure = np.zeros(n.size), np.ones(n.size, dtype=bool)
    full = (n > 0) & (p >= 1.0)
    k_out[full] = n[full]
    live = (n > 0) & (p > 0.0) & (p < 1.0)
    flip = p > 0.5
    q = np.where(flip, 1.0 - p, p)
    nd = n.astype(np.float64)
    inv = live & (nd * q < 10.0)
    j = np.nonzero(inv)[0]
    if j.size:
        blk = block(seed, a[j], b[j], tag, DOM_BINV)
        u = _u53(blk[:, 0], blk[:, 1])
        nj, qj = nd[j], q[j]
        odds = qj / (1.0 - qj)
        pm = np.exp(nj * np.log1p(-qj))
        cdf, k, s = pm.copy(), np.zeros(j.size), np.ones(j.size, dtype=bool)
        going = np.ones(j.size, dtype=bool)
        while going.any():
            s[going] &= np.abs(u[going] - cdf[going]) >= margin
            going &= (u > cdf) & (k < nj) & (k < 400.0)
            g = np.nonzero(going)[0]
            k[g] += 1.0
            pm[g] *= odds[g] * (nj[g] - k[g] + 1.0) / k[g]
            cdf[g] += pm[g]
        k_out[j], sure[j] = k, s
    j = np.nonzero(live & ~inv)[0]
    if j.size:
        nj, qj = nd[j], q[j]
        sd = np.sqrt(nj * qj * (1.0 - qj))
        bb = 1.15 + 2.53 * sd
        aa = -0.0873 + 0.0248 * bb + 0.01 * qj
        cc = nj * qj + 0.5
        vr = 0.92 - 4.2 / bb
        alpha = (2.83 + 5.1 / bb) * sd
        lr = np.log(qj / (1.0 - qj))
        m = np.floor((nj + 1.0) * qj)
        lpm = -special.gammaln(m + 1.0) - special.gammaln(nj - m + 1.0) + m * lr
        k, s, pending = m.copy(), np.ones(j.size, dtype=bool), np.ones(j.size, dtype=bool)
        for attempt in range(64):
            g = np.nonzero(pending)[0]
            if g.size == 0:
                break
            blk = block(seed, a[j[g]], b[j[g]], tag ^ (attempt << 24), DOM_BTRS)
            u, v = _u53(blk[:, 0], blk[:, 1]) - 0.5, _u53(blk[:, 2], blk[:, 3])
            us = 0.5 - np.abs(u)
            arg = (2.0 * aa[g] / us + bb[g]) * u + cc[g]
            kd = np.floor(arg)
            scale = np.abs(2.0 * aa[g] / us * u) + np.abs(bb[g] * u) + cc[g] + 1.0
            sg = np.abs(arg - np.rint(arg)) > 8.0 * np.spacing(scale)      # (a true quotient here: rounding errors only)
            inside = (kd >= 0.0) & (kd <= nj[g])
            sg &= ~inside | ((np.abs(us - 0.07) >= margin) & (np.abs(v - vr[g]) >= margin))
            acc1 = inside & (us >= 0.07) & (v <= vr[g])
            kc = np.clip(kd, 0.0, nj[g])
            lhs = np.log(v * alpha[g] / (aa[g] / (us * us) + bb[g]))
            rhs = -special.gammaln(kc + 1.0) - special.gammaln(nj[g] - kc + 1.0) + kc * lr[g] - lpm[g]
            # the device's lgamma is a few ulp of its value off scipy's
            band = margin + 8.0 * np.spacing(special.gammaln(nj[g] + 1.0) + np.abs(kc * lr[g]))
            sg &= ~inside | acc1 | (np.abs(lhs - rhs) >= band)
            acc = acc1 | (inside & (lhs <= rhs))
            s[g] &= sg
            k[g[acc]] = kd[acc]
            pending[g[acc]] = False
        k_out[j], sure[j] = k, s
    k_out = np.where(live & flip, nd - k_out, k_out)
    return k_out, sure


def apportion_binomial(counts, t_reads, seed, pix=None):
    """(out, sure) of ``rip_synth_apportion(poisson = 0)``: electrons up to every read, shares ``tab.p`` under tag 0x11, the
    counter's b = read; ``sure`` is False from the first unsure draw of a pixel on (later draws depend on it)."""
    c = clip_counts(counts)
    tab = share_table(t_reads)
    nreads = len(tab["p"])
    pix = np.arange(c.size, dtype=np.uint64) if pix is None else np.asarray(pix, dtype=np.uint64)
    total = c.astype(np.int64)                     # (int) c: towards zero
    got, ok = np.zeros(c.size, dtype=np.int64), np.ones(c.size, dtype=bool)
    out, sure = np.zeros((nreads, c.size), dtype=np.int64), np.ones((nreads, c.size), dtype=bool)
    for r in range(nreads):
        k, s = binomial(total - got, tab["p"][r], seed, pix, r, TAG_SHARE)
        got = got + k.astype(np.int64)
        ok &= s
        out[r], sure[r] = got, ok
    return out, sure


# ------------------------------------------------------------------------------------------ riprng::normal_f32
def normal(seed, a, b, tag):
    """f64 value of ``riprng::normal_f32(seed, a, b, tag)``: Box-Muller on u24 of words 0 and 1 of {a, b, tag, 0x6c317379}"""
    blk = block(seed, a, b, tag, DOM_NORMAL)
    return philox_ref.box_muller(blk[..., 0], blk[..., 1])


def reset_normals(seed, nact):
    """(nact,) ``reset_kernel``: active index and 0"""
    return normal(seed, np.arange(nact), 0, TAG_RESET)


def read_normals(seed, ngrp, nact):
    """(ngrp, nact) ``resultants_kernel``: active index and group"""
    return normal(seed, np.arange(nact)[None, :], np.arange(ngrp)[:, None], TAG_READ)


def fill_normals(seed, ngrp, npix):
    """(ngrp + 1, npix) ``fill_kernel``: full-frame index and group; plane ``ngrp`` is the reset term"""
    return normal(seed, np.arange(npix)[None, :], np.arange(ngrp + 1)[:, None], TAG_FILL)


def white33_normals(seed, ngrp, nchan):
    """(ngrp, nchan) ``amp33_kernel``: index in the (ny, channel width) frame and group"""
    return normal(seed, np.arange(nchan)[None, :], np.arange(ngrp)[:, None], TAG_WHITE33)


# ------------------------------------------------------------------------------------------ cr.hip
def track_uniforms(seed, nrows):
    """(nrows, 5) the uniforms of ``cr_tracks_kernel``: blocks {row, 0..2, 0x21, 0x6372746b}, u53 of words (0, 1), (2, 3), ...
    of the twelve in a row.  Exact in f64."""
    row = np.arange(nrows)
    w = np.concatenate([block(seed, row, b, TAG_CR_TRACK, DOM_CR_TRACK) for b in range(3)], axis=1)
    return np.stack([_u53(w[:, 2 * q], w[:, 2 * q + 1]) for q in range(5)], axis=1)


def poisson_any(lam, seed, a, b, tag, margin=MARGIN):
    """(k, sure) of ``cr.hip``'s ``poisson_any``: below 10 the f64 sequential search on u53 of {a, b, tag, 0x63727069}, from 10
    on ``poisson_ptrs`` with sqrt(lam) and log(lam)"""
    lam, a, b = (np.ravel(x) for x in np.broadcast_arrays(np.asarray(lam, dtype=np.float64), np.asarray(a, dtype=np.uint64),
                                                         np.asarray(b, dtype=np.uint64)))
    k_out, sure = np.zeros(lam.size), np.ones(lam.size, dtype=bool)
    j = np.nonzero((lam > 0.0) & (lam < 10.0))[0]
    if j.size:
        blk = block(seed, a[j], b[j], tag, DOM_CR_POIS)
        u = _u53(blk[:, 0], blk[:, 1])
        lj = lam[j]
        p = np.exp(-lj)
        cdf, k, s = p.copy(), np.zeros(j.size), np.ones(j.size, dtype=bool)
        going = np.ones(j.size, dtype=bool)
        while going.any():
            s[going] &= np.abs(u[going] - cdf[going]) >= margin
            going &= (u > cdf) & (k < 200.0)
            g = np.nonzero(going)[0]
            k[g] += 1.0
            p[g] *= lj[g] / k[g]
            cdf[g] += p[g]
        k_out[j], sure[j] = k, s
    j = np.nonzero(lam >= 10.0)[0]
    if j.size:
        k_out[j], sure[j] = poisson_ptrs(lam[j], np.sqrt(lam[j]), np.log(lam[j]), seed, a[j], b[j], tag, margin)
    return k_out, sure


def per_read(mean, nreads, t0=1.0):
    """(counts value f32, t_reads) of a frame with ``mean`` electrons per read in ``nreads`` equally spaced reads, the first at
    t0 > 0 so that read 0 draws too"""
    return np.float32(mean * nreads), np.arange(1, nreads + 1, dtype=np.float64) * t0
