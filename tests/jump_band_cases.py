"""Ramps whose jump significances sit AT the threshold (test_host_jump_band.py, test_gpu_jump_band.py).

The jump detector flags group i where delta / f32(sqrt(var)) > sthresh (oracle/rampfit.py).  The device evaluates var approximately
and accepts the approximate decision outside an error band; a random ramp puts a significance within 1e-6 (relative) of the
threshold about once per 10^6 tested differences, so random ramps cannot tell a band that is too narrow from a sufficient one.
Here every pixel gets one tested difference moved to within +-40 f32 steps of the point where the oracle's decision flips:

  * the knob is the pixel's READ NOISE (an f32 plane that enters only var and err_read: the corrected cube, the slope and the
    threshold do not depend on it, so one oracle run of the front of the chain serves the whole search and the pixels stay
    independent), or -- for the ramp fit as a function, where the Poisson term dominates -- its GAIN (dvardt = slope / gain; in the
    chain the gain also passes through the IPC step and would couple neighbouring pixels),
  * the deciding fit of a pixel is the full ramp if its last group is not saturated, the ramp truncated at its first saturated
    group t >= 3 + start otherwise (pixels that saturate earlier are left alone),
  * the target is the first feasible difference of that fit, cycling over its ``difference_list`` from a start that depends on the
    pixel: feasible = the oracle's decision at the two ends of the knob's range differs (and the threshold itself is the same on
    every host: ``threshold_is_portable``),
  * the knob is bisected on its int32 bit pattern with ``oracle.rampfit.fit_and_flag`` until a hit value and a no-hit value are
    adjacent floats, then the hit value is offset by a seeded integer in [-40, 40] float steps.

A plain module: no fixtures, no test."""

from functools import lru_cache

import numpy as np
from chain_support import F32, F64, oracle_lines, read_pattern

import oracle
from oracle import rampfit
from romanimpreprocess_amd import synth

NB = 4
STEPS = 40
RANGE = {"read": (0.05, 500.0), "gain": (0.02, 200.0)}
NEAR = 3e-6   # |rel| below which a targeted difference counts as near the threshold


def strip_shape(G, k64):
    """40 x 256, or 40 x 512 where a strip of the fused kernel's form is 384 columns wide (chain2_form.h, C2Form::cols)"""
    return (40, 512) if ((G + 1) // 2 * 2 <= 8) == bool(k64) else (40, 256)


def rate_image(cal, rp, ny, nx, seed):
    """DN/s: sources on no sky, plus a rate that grows with the column from 0.1 (the slope lands in [0, IthreshA)) through the
    range; a block at -0.5 in front (slope < 0: dvardt clipped to 0); the last quarter of the columns saturates, row by row, between
    the groups g - 1 and g for every g from 2 to G - 1 (first saturations at every group, slopes above IthreshB among them)"""
    G = len(rp)
    t = synth.group_times(rp)
    rate = synth.make_rate_image(ny, nx, seed, sky=0.0) + 10.0 ** (-1.0 + 5.0 * (np.arange(nx) / nx))[None, :]
    rate[:, :nx // 16] = -0.5
    lin = cal["linearitylegendre"]
    room = cal["saturation"]["data"].astype(np.float64) - lin["Sref"]   # DN between the start of the ramp and saturation
    x0 = nx - nx // 4
    # (the shortest refits get more rows: a cosmic ray has to fall into their few groups to make a difference feasible; so does
    # the longest, which the columns in front of this block do not reach)
    seq = np.array(list(range(2, G)) + [t for t in (4, 3, 4, 5, 4, 3) if t < G] + [G - 1])
    xh = (x0 + nx) // 2   # two halves, the second half a turn ahead: every entry of the list gets its rows
    for xa, xb, turn in ((x0, xh, 0), (xh, nx, seq.size // 2)):
        g = seq[(np.arange(ny) + turn) % seq.size]
        rate[:, xa:xb] = room[:, xa:xb] / np.sqrt(t[g - 1] * t[g])[:, None]
    return rate


@lru_cache(maxsize=2)
def front(G, k64, shape, exclude_first, seed):
    """the CALDIR set, the ramp and the oracle's result with the synthetic read noise (its corrected cube feeds the search)"""
    ny, nx = shape
    rp = read_pattern(G)
    cal = synth.make_caldir(ny, nx, read_pattern=rp, p_order=8, seed=seed, bias_amplitude=2.0, ipc_dtype=F64 if k64 else F32)
    ramp = synth.make_ramp(cal, read_pattern=rp, seed=seed + 1, cr_frac=0.5, saturation_backup=0,
                           rate=rate_image(cal, rp, ny, nx, seed + 2))
    with np.errstate(all="ignore"):
        ref = oracle.calibrate_arrays(ramp, cal, exclude_first=exclude_first)
    return rp, cal, ramp, ref


def deciding_variant(groupdq, G, start):
    """per pixel: 0 = the full ramp, t = the ramp truncated to t groups, -1 = saturated too early for any fit with jump flags"""
    sat = (groupdq & rampfit.SATURATED) != 0
    first = np.where(sat.any(axis=0), sat.argmax(axis=0), G)
    return np.where(first >= G, 0, np.where(first >= 3 + start, first, -1))


class _Search:
    """the oracle's significances of every pixel's deciding fit as a function of one plane (read noise or gain)"""

    def __init__(self, data, gain, read, meta, exclude_first, jump_pars, variant, knob):
        self.G, self.ny, self.nx = data.shape
        self.data = data.reshape(self.G, -1)
        self.planes = {"gain": gain.ravel(), "read": read.ravel()}
        self.meta, self.exclude_first, self.jump_pars, self.knob = meta, exclude_first, jump_pars, knob
        self.start = 1 if exclude_first else 0
        self.variant = variant.ravel()
        self.ndiff = {int(v): len(rampfit.difference_list(int(v) if v else self.G, self.start)) for v in np.unique(self.variant) if v >= 0}
        self.ndmax = max(self.ndiff.values())

    def __call__(self, plane, sel=None):
        """(significances (ndmax, npix) f32, NaN beyond a fit's list and where not selected; slope f32; threshold f64) with the
        knob's plane replaced by `plane` (flat), on the pixels `sel` (flat bool; None: every pixel that has a deciding fit)"""
        npix = self.variant.size
        sm = np.full((self.ndmax, npix), np.nan, F32)
        slope = np.full(npix, np.nan, F32)
        sth = np.full(npix, np.nan, F64)
        for v, nd in self.ndiff.items():
            m = self.variant == v
            if sel is not None:
                m &= sel
            idx = np.flatnonzero(m)
            if idx.size == 0:
                continue
            # (the knob's values in its plane's own dtype: an f64 gain plane keeps dvardt in f64)
            p = {k: (plane.astype(a.dtype) if k == self.knob else a)[idx][None, :] for k, a in self.planes.items()}
            diag = {}
            # a one-row frame of these pixels, C-contiguous as the whole frame is: in another layout the oracle's einsum adds the
            # slope's terms in another order, and the slope comes out an ulp off the whole frame's
            cube = np.ascontiguousarray(self.data[:, idx])[:, None, :]
            with np.errstate(all="ignore"):
                s, _er, _ep, smv = rampfit.fit_and_flag(cube, np.zeros(cube.shape, np.uint8), p["gain"], p["read"], self.meta, 0,
                                                        self.exclude_first, v if v else None, self.jump_pars, diag=diag)
            sm[:nd, idx] = smv[:nd, 0]   # (the cube has a spare row where the list holds di = 1 alone)
            slope[idx] = s[0]
            sth[idx] = diag["sthresh"][0]
        return sm, slope, sth


def threshold_is_portable(slope, jump_pars=None):
    """False where the reference's own threshold depends on the host's numpy: np.log on an f32 array is a SIMD polynomial that is
    up to 2 ulp off the correctly rounded logarithm on a few percent of the inputs, and not the same polynomial on every CPU.  The
    device takes the correctly rounded value ("log of the threshold"), so on these pixels a significance within
    about 1e-7 of the threshold (4e-7 with CROSSING's steeper line) may get either flag.  They keep their synthetic read noise: the
    search puts a difference AT the threshold only where the reference says the same on every host."""
    p = dict(rampfit.DEFAULT_JUMP_PARS, **(jump_pars or {}))
    with np.errstate(all="ignore"):
        x = np.clip(slope, p["IthreshA"], p["IthreshB"]) / p["IthreshA"]   # f32, as fit_and_flag has it
        return np.log(x) == np.log(x.astype(F64)).astype(F32)


def _tune(search, plane0, seed):
    """the tuned plane (flat f32) and the per-pixel record"""
    npix = plane0.size
    lo, hi = (np.full(npix, x, F32) for x in RANGE[search.knob])
    has_fit = search.variant >= 0
    sm_lo, slope, sth = search(lo)
    sm_hi, slope_hi, sth_hi = search(hi)
    assert np.array_equal(slope_hi, slope, equal_nan=True) and np.array_equal(sth_hi, sth, equal_nan=True), "slope or threshold moved with the knob"
    portable = threshold_is_portable(slope, search.jump_pars)
    with np.errstate(invalid="ignore"):
        hit_lo, hit_hi = sm_lo > sth[None], sm_hi > sth[None]
        feasible = (hit_lo != hit_hi) & np.isfinite(sm_lo) & np.isfinite(sm_hi) & (has_fit & portable)[None]
    # the target: cycle over the fit's difference list from a start that depends on the pixel, take the first feasible one
    nd = np.array([search.ndiff.get(int(v), 1) for v in search.variant])
    k = np.full(npix, -1)
    at = np.arange(npix)
    for off in range(search.ndmax):
        cand = (at + off) % nd
        ok = feasible[cand, at] & (k < 0) & (off < nd)
        k[ok] = cand[ok]
    targeted = k >= 0
    kk = np.where(targeted, k, 0)
    # bisection on the bit pattern between a value with a hit (a) and one without (b)
    a = np.where(hit_lo[kk, at], lo.view(np.int32), hi.view(np.int32)).astype(np.int64)
    b = np.where(hit_lo[kk, at], hi.view(np.int32), lo.view(np.int32)).astype(np.int64)
    for _ in range(40):
        open_ = targeted & (np.abs(a - b) > 1)
        if not open_.any():
            break
        mid = (a + b) // 2
        sm, _s, _t = search(mid.astype(np.int32).view(F32), open_)
        with np.errstate(invalid="ignore"):
            hit = sm[kk, at] > sth
        a = np.where(open_ & hit, mid, a)
        b = np.where(open_ & ~hit, mid, b)
    assert np.all(np.abs(a - b)[targeted] == 1), "the search did not end on adjacent floats"
    step = np.random.default_rng(seed).integers(-STEPS, STEPS + 1, size=npix)
    tuned = np.where(targeted, (a + step).astype(np.int32).view(F32), plane0).astype(F32)
    sm, slope2, sth2 = search(tuned)
    assert np.array_equal(slope2, slope, equal_nan=True) and np.array_equal(sth2, sth, equal_nan=True), "slope or threshold moved with the knob"
    with np.errstate(all="ignore"):
        rel_all = sm.astype(F64) / sth[None] - 1.0
        rel = np.where(targeted, rel_all[kk, at], np.nan)
        hit = np.where(targeted, sm[kk, at] > sth, False)
        others = np.where((np.arange(search.ndmax)[:, None] == k[None, :]) | ~np.isfinite(rel_all), np.inf, np.abs(rel_all))
    shape = (search.ny, search.nx)
    active = np.zeros(shape, bool)
    active[NB:-NB, NB:-NB] = True
    rec = {"variant": search.variant.reshape(shape), "k": k.reshape(shape), "rel": rel.reshape(shape), "hit": hit.reshape(shape),
           "slope": slope.reshape(shape), "sthresh": sth.reshape(shape), "portable": portable.reshape(shape),
           "other_rel": others.min(axis=0).reshape(shape), "active": active, "start": search.start, "G": search.G}
    return tuned, rec


def _pars_key(jump_pars):
    return tuple(sorted(jump_pars.items())) if jump_pars else None


@lru_cache(maxsize=8)   # (the case tables below list the cases that several tests use last, so that they meet them here)
def _chain_inputs(G, k64, shape, exclude_first, seed, jp):
    jump_pars = dict(jp) if jp else None
    rp, cal, ramp, ref0 = front(G, k64, shape, exclude_first, seed)
    start = 1 if exclude_first else 0
    variant = deciding_variant(ramp["groupdq"], G, start)
    read0 = cal["read"]["data"]
    search = _Search(ref0["data"], cal["gain"]["data"], read0, ref0["meta"], exclude_first, jump_pars, variant, "read")
    tuned, rec = _tune(search, read0.ravel(), seed + 3)
    cal2 = dict(cal)
    cal2["read"] = dict(cal["read"], data=tuned.reshape(shape))
    with np.errstate(all="ignore"):
        ref = oracle.calibrate_arrays(ramp, cal2, exclude_first=exclude_first, jump_pars=jump_pars)
    assert np.array_equal(ref["data"], ref0["data"], equal_nan=True), "the corrected cube depends on the read noise"
    return cal2, ramp, ref, oracle_lines(ref, G, shape[1] // 128), rec


def near_threshold_inputs(G, kdt, shape, exclude_first, seed, jump_pars=None):
    """(cal, ramp, ref, lines, rec): the CALDIR set with the tuned read-noise plane, the ramp, the oracle's result for that set,
    the channel lines it used, and the per-pixel record -- planes ``variant`` (0 full ramp, t truncated to t groups, -1 none), ``k``
    (index of the targeted difference in the fit's difference_list, -1 not targeted), ``rel`` (smap / sthresh - 1 of the targeted
    difference as the oracle computes it), ``hit``, ``slope`` and ``sthresh`` of the deciding fit, ``other_rel`` (the smallest |rel| among
    the fit's other differences), ``portable`` (threshold_is_portable), ``active``.  Cached: the same arguments give the same objects, which nobody changes."""
    return _chain_inputs(G, kdt == F64, tuple(shape), bool(exclude_first), seed, _pars_key(jump_pars))


@lru_cache(maxsize=2)
def near_threshold_fit_inputs(G, shape, exclude_first, seed, knob):
    """For the ramp fit as a function (fitting.ramp_fit) with an f64 gain plane: (cube, groupdq, pixeldq, gain (f64), read, meta,
    expected, rec) with the plane `knob` ("read" or "gain") tuned under that gain; ``expected`` = (slope, err_read, err_poisson, groupdq,
    pixeldq) of oracle.rampfit.ramp_fit.  The gain takes f32 values held as f64 (the search moves on the f32 bit pattern)."""
    rp, cal, ramp, ref0 = front(G, False, tuple(shape), exclude_first, seed)
    start = 1 if exclude_first else 0
    variant = deciding_variant(ramp["groupdq"], G, start)
    planes = {"gain": cal["gain"]["data"].astype(F64), "read": cal["read"]["data"]}
    search = _Search(ref0["data"], planes["gain"], planes["read"], ref0["meta"], exclude_first, None, variant, knob)
    tuned, rec = _tune(search, planes[knob].ravel().astype(F32), seed + 4)
    planes[knob] = tuned.reshape(shape).astype(planes[knob].dtype)
    rdq, pdq = ramp["groupdq"].copy(), ramp["pixeldq"].copy()
    with np.errstate(all="ignore"):
        s, er, ep = rampfit.ramp_fit(ref0["data"], rdq, pdq, planes["gain"], planes["read"], ref0["meta"], exclude_first, None)
    return ref0["data"], ramp["groupdq"], ramp["pixeldq"], planes["gain"], planes["read"], ref0["meta"], (s, er, ep, rdq, pdq), rec


# ---- the cases of test_gpu_jump_band.py (test_host_jump_band.py holds the generator to its conditions on every one of them)
STEEP = {"SthreshA": 7.0, "SthreshB": 3.0, "IthreshA": 0.3, "IthreshB": 700.0}      # IthreshA != 1, a steeper threshold line
CROSSING = {"SthreshA": 5.5, "SthreshB": -0.5, "IthreshA": 1.0, "IthreshB": 1000.0}  # threshold <= 0 above about 560 DN/s


def _case(G, k64=False, exclude_first=True, jump_pars=None, shape=None):
    name = f"g{G}_{'k64' if k64 else 'f32'}" + ("" if exclude_first else "_start0") + \
        ("" if not jump_pars else "_steep" if jump_pars is STEEP else "_crossing")
    return name, (G, F64 if k64 else F32, shape or strip_shape(G, k64), exclude_first, 500 + 10 * G + 2 * int(k64) + int(not exclude_first),
                  jump_pars)


FUSED = dict([_case(G) for G in (5, 7, 9, 10, 11, 12, 13, 14, 15)] + [_case(G, k64=True) for G in (8, 13, 16)]
             + [_case(G, exclude_first=False) for G in (8, 11)] + [_case(G) for G in (6, 8, 16)])   # every count from 5 to 16
STAGE = dict([_case(G) for G in (6, 8, 16)] + [_case(20, shape=(40, 512))])
CUSTOM = dict([_case(8, jump_pars=STEEP), _case(8, jump_pars=CROSSING)])
CHAIN_CASES = {**{k: v for k, v in FUSED.items() if k not in STAGE}, **CUSTOM, **STAGE}
FIT_CASES = {"g8_read": (8, (40, 256), True, 580, "read"), "g8_gain": (8, (40, 256), True, 580, "gain")}


def regime_counts(rec, jump_pars=None):
    """the oracle's near-threshold cases (targeted differences with |rel| < NEAR on the active region): dict of counts"""
    ia, ib = (dict(rampfit.DEFAULT_JUMP_PARS, **(jump_pars or {}))[k] for k in ("IthreshA", "IthreshB"))
    near = rec["active"] & (rec["k"] >= 0) & (np.abs(rec["rel"]) < NEAR)
    s, v = rec["slope"], rec["variant"]
    with np.errstate(invalid="ignore"):
        out = {"near": int(near.sum()), "hits": int((near & rec["hit"]).sum()), "full": int((near & (v == 0)).sum()),
               "slope<0": int((near & (s < 0)).sum()), "0<=slope<IA": int((near & (s >= 0) & (s < ia)).sum()),
               "slope>IB": int((near & (s > ib)).sum()),
               "full_by_difference": np.bincount(rec["k"][near & (v == 0)], minlength=len(rampfit.difference_list(rec["G"], rec["start"]))).tolist(),
               "trunc": {t: int((near & (v == t)).sum()) for t in range(3 + rec["start"], rec["G"])}}
    return out


def stage_fast_path_errors(cal, ref, rec, guard):
    """numpy emulation of the stage kernel's fast path (device_rampfit.h, fit_variant) on the targeted differences of the active
    region: A, B as plan.hip makes them (f64 sums, rounded to f32), var32 = A s2 + B dv with one rounding per operation, sm = delta /
    sqrt(var32), accepted where |sm - f32(sth)| > f32(guard |sth|).  Returns (accepted decisions that differ from the oracle's,
    differences left to the exact path)."""
    meta, data, G, start = ref["meta"], ref["data"], rec["G"], rec["start"]
    tbar, tau, N = meta["tbar"], meta["tau"].astype(F64), meta["N"].astype(F64)
    gain, read = cal["gain"]["data"], cal["read"]["data"]
    wrong = exact = 0
    for v in np.unique(rec["variant"][rec["k"] >= 0]):
        g = int(v) if v else G
        K = meta["K"] if v == 0 else rampfit.two_point_weights(meta, g, start)
        for k, (i, di) in enumerate(rampfit.difference_list(g, start)):
            m = rec["active"] & (rec["variant"] == v) & (rec["k"] == k)
            if not m.any():
                continue
            dt = tbar[i + di] - tbar[i]
            inv = F32(1.0) / dt
            w = -K.astype(F64)
            w[i + di] += F64(inv)
            w[i] -= F64(inv)
            A = B = 0.0
            for a in range(g):
                A += w[a] * w[a] / N[a]
                B += w[a] * w[a] * tau[a]
                for b in range(a):
                    B += 2.0 * w[a] * w[b] * F64(tbar[b])
            s, sth = rec["slope"][m], rec["sthresh"][m]
            with np.errstate(all="ignore"):
                dv = np.clip(s / np.clip(gain[m], F32(1e-4), F32(1e4)), F32(0.0), None).astype(F32)
                s2 = read[m] * read[m]
                delta = (data[i + di][m] - data[i][m]) / dt - s
                var32 = F32(A) * s2 + F32(B) * dv
                sm = delta / np.sqrt(var32)
                assert sm.dtype == F32 and var32.dtype == F32
                sth32 = sth.astype(F32)
                fast = np.abs(sm - sth32) > (guard * np.abs(sth)).astype(F32)
                wrong += int(np.count_nonzero(fast & ((sm > sth32) != rec["hit"][m])))
                exact += int(np.count_nonzero(~fast))
    return wrong, exact
