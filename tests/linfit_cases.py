"""Inputs of the linearity-fit tests (``test_host_linfit.py``, ``test_gpu_linfit.py``): the recovery case of a known curve and the
table of small frames whose pixels cover every branch of ``rip_cal_linearity_fit``.  numpy only.
"""

import numpy as np

import linfit_ref

# ------------------------------------------------------------------------------------------ recovery of a known curve
SREF = 5300.0
TFRAME = 3.15625
TSTART = 3
CLAMP = 58000.0
RECOVERY_SETS = ((420.0, 56), (60.0, 12), (0.3, 56))   # (rate in DN_lin/s, frames): bright flat, low flat, dark
START_DN_LIN = 100.0   # every ramp is 100 DN_lin above Sref two frames before its first one
# max |phi_fit - phi_true| in DN_lin of the numpy restatement at n = 4096 per order, as measured when the rule was written
# (profiles/linearity_fit.txt); the tests hold the restatement and the device to twice these values
RECORDED_ERROR = {5: 0.0020247, 8: 0.0022417, 10: 0.0282326}


def phi_true(S):
    x = (np.asarray(S, np.float64) - SREF) / 50000.0
    return (np.asarray(S, np.float64) - SREF) + 3000.0 * x ** 2 + 1500.0 * x ** 3 + 800.0 * x ** 5


def _inverse(L):
    """S with phi_true(S) = L, by bisection on [Sref - 2000, 70000] (phi_true is increasing there)"""
    lo, hi = np.full_like(L, SREF - 2000.0), np.full_like(L, 70000.0)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        below = phi_true(mid) < L
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    return 0.5 * (lo + hi)


def recovery_sums(n):
    """(sums, counts, first, sref): the three mean ramps as sums of ``n`` copies, copy e holding floor(S + (e + 0.5) / n) -- a
    deterministic dither that controls the 16-bit quantisation.  One pixel, frames (nf, 1, 1)."""
    sums = []
    e = (np.arange(n, dtype=np.float64) + 0.5) / n
    for rate, nf in RECOVERY_SETS:
        L = START_DN_LIN + rate * TFRAME * (np.arange(nf, dtype=np.float64) + 2.0)
        S = np.minimum(_inverse(L), CLAMP)
        sums.append(np.floor(S[:, None] + e[None, :]).sum(axis=1).astype(np.uint32).reshape(nf, 1, 1))
    return sums, [n] * 3, [TSTART - 1] * 3, np.full((1, 1), SREF, np.float32)


def recovery_error(out, sums, counts, first):
    """max |phi_fit - phi_true| in DN_lin on 2001 points of [smallest used sample, Smax] of the one pixel"""
    smin, smax = float(out["Smin"][0, 0]), float(out["Smax"][0, 0])
    lo = smax
    for k, s in enumerate(sums):
        Mk = s[first[k]:, 0, 0].astype(np.float64) / counts[k]
        Mk = Mk[(Mk >= smin) & (Mk <= smax)]
        if Mk.size:
            lo = min(lo, Mk.min())
    S = np.linspace(lo, smax, 2001)
    got = linfit_ref.evaluate(out["data"][:, 0, 0], smin, smax, S)
    return float(np.max(np.abs(got - phi_true(S))))


# ------------------------------------------------------------------------------------------ the table of small frames
NY, NX, NB = 12, 72, 2
LENGTHS = {1: (12,), 2: (12, 7), 3: (5, 12, 7)}
COUNTS = (3, 2, 5)
ORDERS = (1, 2, 3, 8, 10)
FIT_CASES = [(nsets, tstart, p) for nsets in (1, 2, 3) for tstart in (1, 3) for p in ORDERS]
NCLASS = 16
KINDS = ("cut at the first difference", "no cut", "cut in the middle", "Smax capped at 65535", "a set with fewer than two used samples",
         "degrees of freedom one below p - 1", "degrees of freedom at p - 1", "D0 = 0", "D0 < 0", "Sref NaN", "Sref above Smax",
         "Smin clipped at 0", "identical samples in a set")


def signals(nsets, tstart):
    """(S, counts, sref): per set the float64 (frames, NY, NX) mean signal of the table's frame, already within 0..65535"""
    rng = np.random.default_rng(1000 * nsets + tstart)
    lengths, counts = LENGTHS[nsets], COUNTS[:nsets]
    cls = (np.arange(NY * NX).reshape(NY, NX) * 7 // 3) % NCLASS
    sref = (5000.0 + 300.0 * rng.uniform(size=(NY, NX))).astype(np.float32)
    sref[cls == 2] = np.nan
    sref[cls == 3] = 70000.0
    sref[cls == 4] = 200.0
    base = np.where(np.isfinite(sref) & (sref < 60000.0), sref, 5000.0).astype(np.float64) - rng.uniform(0.0, 150.0, size=(NY, NX))
    sat = rng.uniform(30000.0, 75000.0, size=(NY, NX))
    out = []
    for k, nf in enumerate(lengths):
        isdark = nsets > 1 and k == nsets - 1
        i = np.arange(nf, dtype=np.float64)[:, None, None]
        if isdark:
            rate = rng.uniform(0.0, 3.0, size=(NY, NX))
            rate[cls == 5] = 0.0   # identical samples
        elif k == 0:
            rate = rng.uniform(1500.0, 9000.0, size=(NY, NX)) * (12.0 / nf)
            rate[cls == 8] = 900.0   # never near saturation: no cut
        else:
            rate = rng.uniform(300.0, 3000.0, size=(NY, NX))
            fast = (cls >= 9) & (cls <= 12)   # leaves the range after a few frames: the degrees of freedom vary
            rate[fast] = rng.uniform(3000.0, 30000.0, size=(NY, NX))[fast]
        L = rate[None] * i
        if k == 0:
            slow_start = np.where(i <= tstart - 1, 0.0, rate[None] * (i - tstart) + 0.02 * rate[None])
            L = np.where((cls == 7)[None], slow_start, L)       # the first difference used is far below the mean of the first four
            L = np.where((cls == 0)[None], 3000.0, L)           # D0 = 0
            L = np.where((cls == 1)[None], 9000.0 - 700.0 * i, L)   # D0 < 0
        S = np.minimum(base[None] + L - 2.0e-6 * L * L, sat[None])
        if k == 1:
            S = np.where((cls == 6)[None], 66000.0, S)   # out of every range: the set takes no part
        out.append(np.clip(S, 0.0, 65535.0))
    return out, list(counts), sref


def fit_inputs(nsets, tstart):
    """(sums, counts, first, sref, dark) of one frame of the table: set 0 is the bright flat, the last of two or three the dark"""
    S, counts, sref = signals(nsets, tstart)
    sums = [np.clip(np.rint(s * c), 0, 65535 * c).astype(np.uint32) for s, c in zip(S, counts)]
    return sums, counts, [tstart - 1] * nsets, sref, (nsets - 1 if nsets > 1 else -1)


def exposures(nsets, tstart, width=NX):
    """per set its ``COUNTS`` exposures as uint16 (frames, NY, width) cubes -- the signal plus the exposure's number, columns beyond
    NX filled with a pattern that must never be read -- and Sref: the input of the drop-in"""
    S, counts, sref = signals(nsets, tstart)
    sets = []
    for s, c in zip(S, counts):
        cubes = []
        for e in range(c):
            cube = np.full(s.shape[:2] + (width,), 0xA5A5, np.uint16)
            cube[:, :, :NX] = np.clip(np.rint(s) + e, 0, 65535).astype(np.uint16)
            cubes.append(cube)
        sets.append(cubes)
    return sets, sref


def kinds_of(out, sums, counts, first, sref, dark, p):
    """per kind of ``KINDS`` the number of pixels off the border that show it in the restatement's result ``out``"""
    inner = np.zeros((NY, NX), bool)
    inner[NB:-NB, NB:-NB] = True
    i0, last = first[0], sums[0].shape[0] - 1
    cut, dof, m = out["cut"], out["dof"], p - 1
    few = np.zeros((NY, NX), bool)
    for k in range(1, len(sums)):
        few |= out["nused"][k] < 2
    same = np.zeros((NY, NX), bool)
    good = out["dq"] == 0
    for k in range(len(sums)):
        same |= np.all(sums[k][first[k]:] == sums[k][first[k]], axis=0) & (out["nused"][k] >= 2) & good
    with np.errstate(invalid="ignore"):
        n = [np.count_nonzero(inner & c) for c in (
            cut == i0, cut == last, (cut > i0) & (cut < last), out["Smax"] == 65535.0, few, dof == m - 1, dof == m,
            out["D0"] == 0.0, out["D0"] < 0.0, np.isnan(sref), np.isfinite(sref) & (sref > out["Smax"]),
            np.isfinite(sref) & (sref < 500.0) & (out["Smin"] == 0.0), same)]
    return dict(zip(KINDS, n))
