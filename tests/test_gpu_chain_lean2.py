"""Second lean pass of the fused kernel (short_forms.h, chain2_kernel.h), bit for bit against the CPU oracle and the stage kernels at
the smallest shapes where it can go wrong:

  * the row loop that ends one step earlier: frames of 24 to 40 rows whose LAST row range has 1, 2 or 3 rows (the drain of the
    loop is then all that range does), at 256 columns (one strip), 384 (two strips, a seam at columns 252 .. 255) and 512 (three,
    the last with four live columns); 5 to 8 groups on the 256-column form, 16 groups at 384 columns on a narrow form, and a
    4096-column frame whose last strip runs in quad mode (wave columns with row ranges of their own, one barrier count);
  * the one-correction quotients on both sides of every vote: planted gains at and beside 1e-4 and 1e4 (the clip of
    rip_slope_errors) and 1e-18 and 1e18 (rcp_safe), linearity spans Smax - Smin at and beside 1e-18 and 1e18 (rcp_safe).  One
    such lane sends its whole wave to the division operator; the waves without one take the short forms.  The flat the chain
    divides by is the file's clipped to 0.1 .. 10 and IPC-deconvolved, so the edges of rip_mid36 (1.5e-11, 6.8e10) cannot be
    reached through a frame -- the host check (test_short_forms_host.py) has them as divisors; planted here: flats at and beside
    the clip's ends and a negative one;
  * the short hypot and its fallback: read noise 0 under a falling ramp (a radicand of 0), 1e19 (a radicand above
    2^120), and read-noise values TUNED, pixel by pixel, so that sqrt(er^2 + ep^2) lies within 12 f64 steps of an f32 rounding
    midpoint, on either side: inside the guard band of rip_hypot_short (32 steps; its root is within 8 of the f64 root), so
    those waves take the full expression.  The tuning is done on the oracle's own intermediates (its corrected cube does not
    depend on the read noise) and the count of such pixels is asserted on the final reference.

Every frame is a few thousand pixels to half a million (quad mode needs 4096 columns); the oracle runs twice per case, cached."""

from functools import lru_cache

import numpy as np
import pytest
import torch  # noqa: F401  before libromanhip is loaded: torch brings its own copy of the HIP runtime, and the first one loaded must be the one both use
from chain_support import (F32, F64, JUMP, SAT, assert_equal_outputs, assert_oracle, chain_context, device_cus, geometry, is_quad, loaded,
                           oracle_lines, read_pattern)

import oracle
from oracle import rampfit
from romanimpreprocess_amd import pipeline, synth

gpu = pytest.mark.gpu
SLOT = 13
NB = 4
MID = 1 << 28          # low 29 bits of an f64 that sits on an f32 rounding midpoint
TUNED_WITHIN = 12      # f64 steps; the guard band of rip_hypot_short is 32, its root within 8 of the f64 root


def up(x, n=1):
    """the float n steps above x (below for negative n), f32"""
    v = np.array([x], dtype=F32)
    for _ in range(abs(n)):
        v = np.nextafter(v, F32(np.inf if n > 0 else -np.inf))
    return float(v[0])


GAINS = [up(1e-4, -1), float(F32(1e-4)), up(1e-4), up(1e4, -1), float(F32(1e4)), up(1e4), float(F32(1e-18)), up(1e-18), up(1e18, -1),
         float(F32(1e18))]
SPANS_SMALL = [float(F32(1e-18)), up(1e-18)]                  # Smin = 0, Smax = these
SPANS_LARGE = [up(1e18, -1), float(F32(1e18))]                # Smax = these (Smin of a few thousand does not change the float)
FLATS = [0.05, up(0.1, -1), float(F32(0.1)), float(F32(10.0)), up(10.0), 20.0, -1.0]   # the chain clips the file's flat to 0.1 .. 10


def hypot_low_bits(er, ep):
    """low 29 bits of the f64 root of the reference's hypot, (float)sqrt((double)a*a + (double)b*b)"""
    a, b = er.astype(F64), ep.astype(F64)
    root = np.sqrt(a * a + b * b)
    return (root.view(np.uint64) & np.uint64(0x1fffffff)).astype(np.int64)


def full_ramp_errors(ref, cal, exclude_first):
    """(err_read, err_poisson) of the full ramp, as they enter the finish step of a pixel that never saturates"""
    meta = ref["meta"]
    scratch = np.zeros(ref["groupdq"].shape, dtype=np.uint8)
    with np.errstate(all="ignore"):
        _, er, ep, _ = rampfit.fit_and_flag(ref["data"], scratch, cal["gain"]["data"], cal["read"]["data"], meta, meta["nborder"], exclude_first)
    return er, ep


@lru_cache(maxsize=3)
def case(G, ny, nx, k64, exclude_first, seed=1200):
    """(set, ramp, oracle's result, channel lines, number of pixels tuned into the guard band below / above a midpoint)"""
    rp = read_pattern(G)
    cal = synth.make_caldir(ny, nx, read_pattern=rp, p_order=8, seed=seed + G, bias_amplitude=0.0, bad_lin_frac=0.005,
                            ipc_dtype=F64 if k64 else F32)
    rate = synth.make_rate_image(ny, nx, seed + 50 + G)
    rate[NB:ny - NB, nx - 28:nx - NB] += (200.0 * 300.0 ** ((np.arange(ny) % 23) / 22.0))[NB:ny - NB, None]   # saturating band
    ramp = synth.make_ramp(cal, read_pattern=rp, seed=seed + 100 + G, cr_frac=0.05, saturation_backup=0, rate=rate)
    # planted values: science pixels on a grid of pitch 5 (no two share a 3 x 3 neighbourhood twice over), in every strip
    rng = np.random.default_rng(seed + 300 + G)
    ys, xs = np.meshgrid(np.arange(NB + 1, ny - NB - 1, 5), np.arange(max(NB + 1, nx - 601), nx - 30, 5), indexing="ij")
    spots = rng.permutation(np.stack([ys.ravel(), xs.ravel()], axis=1))
    take = iter(spots)
    lin = dict(cal["linearitylegendre"])
    gain, flat, read = cal["gain"]["data"].copy(), cal["flat"]["data"].copy(), cal["read"]["data"].copy()
    smin, smax = lin["Smin"].copy(), lin["Smax"].copy()
    for v in GAINS:
        y, x = next(take)
        gain[y, x] = v
    for v in SPANS_SMALL:
        y, x = next(take)
        smin[y, x], smax[y, x] = 0.0, v
    for v in SPANS_LARGE:
        y, x = next(take)
        smax[y, x] = v
    flat_spots = [tuple(next(take)) for _ in FLATS]
    data = ramp["data"].astype(np.int64)
    for _ in range(12):   # a falling ramp: slope < 0, Poisson error 0, and no read noise
        y, x = next(take)
        read[y, x] = 0.0
        data[:, y, x] = data[0, y, x] + 400 - 40 * np.arange(G)
    ramp = dict(ramp, data=data.astype(np.uint16))
    for _ in range(3):
        y, x = next(take)
        read[y, x] = 1e19
    lin["Smin"], lin["Smax"] = smin, smax
    cal = dict(cal, gain=dict(cal["gain"], data=gain), linearitylegendre=lin, read=dict(cal["read"], data=read))
    with np.errstate(all="ignore"):
        ref0 = oracle.calibrate_arrays(ramp, cal, exclude_first=exclude_first)
    for (y, x), v in zip(flat_spots, FLATS):
        flat[y, x] = v
    # read noise tuned into the guard band: er = read * rfac small beside ep, so that er^2 / (2 ep) is half a step of ep
    er0, ep0 = full_ramp_errors(ref0, cal, exclude_first)
    rfac = rampfit.read_factor(ref0["meta"]["K"], ref0["meta"], G)
    never_sat = (ref0["groupdq"][G - 1] & SAT) == 0
    tuned = []
    for y, x in take:
        ep = ep0[y, x]
        if not (never_sat[y, x] and ep > 1e-3 and np.isfinite(ep)):
            continue
        step = np.nextafter(ep, F32(np.inf)) - ep
        r0 = F32(np.sqrt(float(ep) * float(step)) / float(rfac))
        cand = (np.array([r0], dtype=F32).view(np.int32) + np.arange(-300, 301, dtype=np.int32)).view(F32)
        lo = hypot_low_bits((cand * rfac).astype(F32), np.full(cand.shape, ep, dtype=F32))
        side = len(tuned) & 1   # even: below the midpoint, odd: above
        d = np.where((lo > MID) == bool(side), np.abs(lo - MID), 1 << 40)
        k = int(np.argmin(d))
        if d[k] <= TUNED_WITHIN:
            read[y, x] = cand[k]
            tuned.append((y, x))
        if len(tuned) == 24:
            break
    cal = dict(cal, read=dict(cal["read"], data=read), flat=dict(cal["flat"], data=flat))
    with np.errstate(all="ignore"):
        ref = oracle.calibrate_arrays(ramp, cal, exclude_first=exclude_first)
    assert np.array_equal(ref["data"], ref0["data"], equal_nan=True), "the corrected cube depends on the read noise or the flat"
    # what the case is after, on the final reference
    er, ep = full_ramp_errors(ref, cal, exclude_first)
    ty, tx = np.array(tuned).T
    lo = hypot_low_bits(er[ty, tx], ep[ty, tx])
    inside = np.abs(lo - MID) <= TUNED_WITHIN
    below, above = int((inside & (lo < MID)).sum()), int((inside & (lo > MID)).sum())
    assert below >= 5 and above >= 5, f"{below} / {above} pixels tuned below / above a midpoint"
    assert np.count_nonzero((er == 0) & (ep == 0) & never_sat) >= 3, "no pixel with a radicand of zero"
    assert np.count_nonzero(ref["pixeldq"] & JUMP) > 5, "no jump flags in the oracle's output"
    return cal, ramp, ref, oracle_lines(ref, G, nx // 128), (below, above)


def last_range(g, ny):
    return ny - (g["nr"] - 1) * g["rows"]


def height_with_last_range(G, k64, nx, last):
    """a height of 24 to 40 rows (the first beyond, on a device whose CU count leaves none) whose last row range has `last` rows"""
    ncu = device_cus()
    for ny in list(range(24, 41)) + list(range(41, 200)):
        g = geometry(G, F64 if k64 else F32, ny, nx, ncu)
        if g is not None and g["nq"] == 0 and g["nr"] > 1 and last_range(g, ny) == last:
            return ny
    raise AssertionError(f"no height with a last range of {last} rows at {nx} columns on {ncu} CUs")


def check(G, ny, nx, k64, exclude_first, want_geo):
    cal, ramp, ref, lines, sides = case(G, ny, nx, k64, exclude_first)
    kw = dict(exclude_first=exclude_first, channel_lines=lines)
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), SLOT, cal) as cb:
        got = cb.calibrate(SLOT, ramp, **kw)
        assert ctx.last_chain_form() == 2, f"kernel form {ctx.last_chain_form()}: not the fused kernel"
        g = ctx.last_chain_geometry()
        assert want_geo(g), f"not the intended geometry: {g}"
        with ctx.options(fused=0):
            stage = cb.calibrate(SLOT, ramp, **kw)
            assert ctx.last_chain_form() == 0
    what = f"{G} groups, {ny} x {nx}, start {int(exclude_first)}, {sides} pixels in the guard band"
    assert_oracle(got, ref, what)
    assert_equal_outputs(got, stage, f"{what}: fused against the stage kernels")
    return g


# ---- 1. the 256-column form: every group count, one to three strips, last ranges of 1, 2 and 3 rows, both starts
@gpu
@pytest.mark.parametrize("G,nx,last,exclude_first", [(5, 256, 1, True), (6, 384, 2, True), (7, 512, 3, True), (8, 256, 3, True),
                                                     (8, 384, 1, True), (8, 512, 2, True), (5, 384, 3, False), (8, 256, 2, False)])
def test_short_last_range_and_planted_edges(G, nx, last, exclude_first):
    ny = height_with_last_range(G, False, nx, last)
    g = check(G, ny, nx, False, exclude_first, lambda g: g["cols"] == 256 and g["nq"] == 0 and last_range(g, ny) == last)
    assert g["nstrips"] == {256: 1, 384: 2, 512: 3}[nx]


# ---- 2. a narrow form: 16 groups, 384 columns
@gpu
def test_sixteen_groups_short_last_range():
    ny = height_with_last_range(16, False, 384, 2)
    check(16, ny, 384, False, True, lambda g: g["cols"] == 384 and last_range(g, ny) == 2)


# ---- 3. quad mode: the wave columns of a workgroup march down different row ranges and end together
@gpu
def test_quad_mode_frame():
    ncu = device_cus()
    ny = next((ny for ny in range(32, 400) if is_quad(geometry(8, F32, ny, 4096, ncu), 64)), None)
    assert ny is not None, f"no height below 400 rows runs the last strip of 4096 columns in quad mode on {ncu} CUs"
    check(8, ny, 4096, False, True, lambda g: is_quad(g, 64))
