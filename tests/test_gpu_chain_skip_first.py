"""The fused kernel's form that skips an excluded first group (chain2_form.h, "SKIPPED FIRST GROUP"; option "skip_first").

With EXCLUDE_FIRST the fit gives group 0 the weight zero and tests no difference on it, so the kernel may leave group 0 out --
its loads, its reference-pixel tables, its Legendre series, both IPC iterates -- wherever d[0] is known to be finite without being
computed: a CALDIR set that passed the screen at upload (``rip_caldir_first_group_safe``) and a call with a u16 cube, the first
group the single read 0, no corrected cube.  Everything else runs the full form.  Every case here asserts through
``rip_last_chain_first_group`` which form ran, then compares slope, err_read, err_poisson, pixeldq and groupdq bit for bit: the
skipping form against the full form (every bit) and against the CPU oracle (as the other chain tests compare with it: the sign
of a zero aside).  Every case first checks the ORACLE's own output for jump flags and for pixels that went through a truncated
refit."""

from functools import lru_cache

import numpy as np
import pytest
import torch  # before libromanhip is loaded: torch brings its own copy of the HIP runtime, and the first one loaded must be the one both use
from chain_support import (F32, F64, JUMP, SAT, assert_equal_outputs, assert_oracle, band_conditions, calibrate_resident, chain_context,
                           device_cus, device_outputs, find_height, geometry, inputs, is_quad, loaded, oracle_lines, outputs_to_numpy,
                           quad_columns, ramp_to_dev, read_pattern)

import oracle
from romanimpreprocess_amd import _native, pipeline, plan as planmod, synth

SLOT = 12
gpu = pytest.mark.gpu


@lru_cache(maxsize=4)
def clean_inputs(G, shape, p, k64, seed):
    """a CALDIR set that passes the screen (flagged linearity pixels stay: flags do not fail it; no degenerate gains), a ramp
    with cosmic rays and saturating pixels, the oracle's result and the channel lines it used"""
    ny, nx = shape
    rp = read_pattern(G)
    cal = synth.make_caldir(ny, nx, read_pattern=rp, p_order=p, seed=seed, bias_amplitude=2.0, bad_lin_frac=0.01,
                            ipc_dtype=F64 if k64 else F32)
    ramp = synth.make_ramp(cal, read_pattern=rp, seed=seed + 1, cr_frac=0.03, saturation_backup=0)
    with np.errstate(all="ignore"):
        ref = oracle.calibrate_arrays(ramp, cal)
    return rp, cal, ramp, ref, oracle_lines(ref, G, nx // 128)


def oracle_conditions(ref, G, start=1):
    """jump flags, and pixels whose first saturated group has them refitted on a truncated ramp (fitting.py:326-337)"""
    q = ref["groupdq"]
    assert np.count_nonzero(ref["pixeldq"] & JUMP) > 5, "no jump flags in the oracle's output"
    refits = sum(np.count_nonzero((q[g] & SAT) & ~(q[g - 1] & SAT)) for g in range(3 + start, G))
    assert refits > 0, "no truncated refit in the oracle's output"


def run(cb, ctx, ramp, skipped, form=2, **kw):
    """one call; asserts which kernel form ran"""
    got = cb.calibrate(SLOT, ramp, **kw)
    assert ctx.last_chain_form() == form, f"kernel form {ctx.last_chain_form()}, expected {form}"
    assert ctx.last_chain_first_group() == (1 if skipped else 0), "not the expected treatment of group 0"
    return got


def skip_and_full(cb, ctx, ramp, **kw):
    """the same call with the option on and off"""
    skip = run(cb, ctx, ramp, True, **kw)
    with ctx.options(skip_first=0):
        full = run(cb, ctx, ramp, False, **kw)
    return skip, full


# ---- 1. the skipping form against the full form and the oracle
# (G, shape, ipc4d f64, Legendre order): 512 columns = two strips of the 256-column form with a seam (and a third of 8 live
# columns), 768 = three of the 384-column forms'; the orders rotate
CASES = [
    (8, (40, 512), False, 8), (7, (40, 512), False, 3), (5, (40, 512), False, 10), (8, (40, 512), True, 3),
    (16, (48, 768), False, 10), (13, (48, 768), False, 8), (16, (48, 768), True, 3),
    # a last row range of ONE row, shorter than the two halo rows (57 rows: ranges of 8 rows)
    (8, (57, 512), False, 8),
]


@gpu
@pytest.mark.parametrize("G,shape,k64,p", CASES, ids=[f"g{G}_{'k64' if k else 'f32'}_{s[0]}x{s[1]}_np{p + 1}" for G, s, k, p in CASES])
def test_skip_vs_full_and_oracle(G, shape, k64, p):
    rp, cal, ramp, ref, lines = clean_inputs(G, shape, p, k64, 300 + G)
    oracle_conditions(ref, G)
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), SLOT, cal) as cb:
        assert ctx.caldir_first_group_safe(SLOT), "a clean CALDIR set did not pass the screen"
        skip, full = skip_and_full(cb, ctx, ramp, channel_lines=lines)
        if shape[0] == 57:
            g = ctx.last_chain_geometry()
            assert g["nq"] == 0 and shape[0] - (-(-shape[0] // g["rows"]) - 1) * g["rows"] == 1, f"no last range of one row: {g}"
    assert_equal_outputs(skip, full, "skipping against full form")
    assert_oracle(skip, ref, "skipping form")
    assert_oracle(full, ref, "full form")


@gpu
def test_skip_in_quad_mode_of_the_256_column_form():
    """f32 ipc4d x 8 groups on a frame whose last strip has 8 live columns, tall enough for quad mode (the inputs, and the way
    to the shape, of test_gpu_chain_geometry)"""
    G, nx = 8, 512
    ncu = device_cus()
    ny = find_height(1376, 8, lambda ny: is_quad(geometry(G, F32, ny, nx, ncu), 8), "quad mode at nx = 512")
    rp, cal, ramp, ref, lines = inputs(G, False, ny, nx, 10, True)
    band_conditions(ref, G, quad_columns(geometry(G, F32, ny, nx, ncu), nx))
    oracle_conditions(ref, G)
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), SLOT, cal) as cb:
        assert ctx.caldir_first_group_safe(SLOT)
        skip = run(cb, ctx, ramp, True, channel_lines=lines)
        assert is_quad(ctx.last_chain_geometry(), 8), f"not quad mode: {ctx.last_chain_geometry()}"
        with ctx.options(skip_first=0):
            full = run(cb, ctx, ramp, False, channel_lines=lines)
    assert_equal_outputs(skip, full, "skipping against full form")
    assert_oracle(skip, ref, "skipping form in quad mode")


@gpu
def test_skip_through_batch_host_and_device_calls():
    """the pre-pass's own channel lines (no caller's lines): single host calls, rip_calibrate_batch and device-resident calls back
    to back (the second call's pre-pass -- tables of groups 1 .. G-1 only -- runs beside the first call's kernel)"""
    G, ny, nx = 7, 136, 512
    rp = read_pattern(G)
    cal = synth.make_caldir(ny, nx, read_pattern=rp, p_order=8, seed=43, bias_amplitude=2.0)
    ramps = [synth.make_ramp(cal, read_pattern=rp, seed=44 + i, cr_frac=0.02, saturation_backup=0) for i in range(3)]
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), SLOT, cal) as cb:
        assert ctx.caldir_first_group_safe(SLOT)
        both = [skip_and_full(cb, ctx, r) for r in ramps]
        many = cb.calibrate_many(SLOT, ramps, want_groupdq=True)
        assert ctx.last_chain_form() == 2 and ctx.last_chain_first_group() == 1
        pid, _meta = cb.plan_for(rp, synth.FRAME_TIME)
        t = [ramp_to_dev(r) for r in ramps[:2]]
        o = [device_outputs(G, ny, nx) for _ in range(2)]
        torch.cuda.synchronize()
        for i in (0, 1):
            calibrate_resident(cb, SLOT, pid, G, t[i], o[i])
        cb.synchronize()
        assert ctx.last_chain_form() == 2 and ctx.last_chain_first_group() == 1
        got_dev = [outputs_to_numpy(oi) for oi in o]
    assert np.count_nonzero(both[0][0]["pixeldq"] & JUMP) > 5
    for i, (skip, full) in enumerate(both):
        assert_equal_outputs(skip, full, f"ramp {i}: skipping against full form")
        assert_equal_outputs(many[i], full, f"ramp {i}: batch against full form")
    for i in (0, 1):
        assert_equal_outputs(got_dev[i], both[i][1], f"device call {i}")


# ---- 2. independence: what group 0 holds does not reach the results
@gpu
def test_results_do_not_depend_on_group_0():
    G, shape, p = 8, (40, 512), 8
    rp, cal, ramp, ref, lines = clean_inputs(G, shape, p, False, 300 + G)
    oracle_conditions(ref, G)
    rng = np.random.default_rng(5)
    cal2 = {k: dict(v) for k, v in cal.items()}
    cal2["dark"]["data"] = cal["dark"]["data"].copy()
    cal2["dark"]["data"][0] += rng.uniform(-3000.0, 3000.0, size=shape).astype(F32)
    cal2["biascorr"]["data"] = cal["biascorr"]["data"].copy()
    assert cal2["biascorr"]["data"].shape[0] == G   # (biascorr[ngrp_bias - G:] are the ramp's planes: plane 0 is group 0's)
    cal2["biascorr"]["data"][0] = rng.uniform(-500.0, 500.0, size=cal2["biascorr"]["data"][0].shape).astype(F32)
    ramp2 = dict(ramp)
    ramp2["data"] = ramp["data"].copy()
    ramp2["data"][0] = rng.integers(0, 65536, size=shape).astype(np.uint16)
    ramp2["amp33"] = ramp["amp33"].copy()
    ramp2["amp33"][0] = rng.integers(20000, 40000, size=ramp["amp33"][0].shape).astype(np.uint16)
    with np.errstate(all="ignore"):
        ref2 = oracle.calibrate_arrays(ramp2, cal2)
    lines2 = oracle_lines(ref2, G, shape[1] // 128)
    assert not np.array_equal(ref["data"][0], ref2["data"][0]) and not np.array_equal(lines[0], lines2[0])
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), SLOT, cal) as cb:
        a = run(cb, ctx, ramp, True, channel_lines=lines)
        cb.load_caldir(SLOT, cal2)
        assert ctx.caldir_first_group_safe(SLOT)
        b = run(cb, ctx, ramp2, True, channel_lines=lines2)
    assert_equal_outputs(a, b, "other finite values in group 0", keys=("slope", "err_read", "err_poisson", "pixeldq"))
    assert_oracle(a, ref, "first inputs")
    assert_oracle(b, ref2, "second inputs")


# ---- 3. the screen says no: one bad value at one pixel of one array
def _plant(cal, what, where):
    """one bad value; `where`: an interior pixel or one in the 4-pixel border (arrays of the active region: its first row)"""
    y, x = (17, 200) if where == "interior" else (1, 133)
    ya, xa = (y - 4, x - 4) if where == "interior" else (0, 129)
    if what == "dark_nan":
        cal["dark"]["data"][0, y, x] = np.nan
    elif what == "bias_inf":
        cal["biascorr"]["data"][0, ya, xa] = np.inf
    elif what == "span_zero":
        cal["linearitylegendre"]["Smax"][y, x] = cal["linearitylegendre"]["Smin"][y, x]
    elif what == "legendre_nan":
        cal["linearitylegendre"]["data"][2, y, x] = np.nan
    elif what == "gain_zero":
        cal["gain"]["data"][y, x] = 0.0
    elif what == "gain_tiny":
        cal["gain"]["data"][y, x] = 1e-35
    elif what == "ipc_nan":
        cal["ipc4d"]["data"][1, 1, ya, xa] = np.nan
    elif what == "amp33_med_nan":
        cal["read"]["amp33"]["med"][y, x % 128] = np.nan
    else:
        raise ValueError(what)


PLANTS = ("dark_nan", "bias_inf", "span_zero", "legendre_nan", "gain_zero", "gain_tiny", "ipc_nan", "amp33_med_nan")


@gpu
@pytest.mark.parametrize("where", ("interior", "border"))
@pytest.mark.parametrize("what", PLANTS)
def test_screen_says_no(what, where):
    """The set fails the screen, the full form runs and gives the oracle's results -- the NaN slopes of a NaN that only group 0
    carries among them: the case the screen exists for.  (The set with an INFINITE value takes the stage kernels instead of the
    full fused form: the fused kernel's shared-reciprocal divisions give NaN for an infinite numerator where the division
    operator, and the reference, give an infinity -- which the clip of an excluded first group turns into a finite z.  With the
    full fused form that set gave NaN where the oracle has 0.33144894, at 15 of 10240 slopes.)"""
    G, shape, p = 8, (40, 256), 8
    rp, cal0, ramp, _ref0, _lines0 = clean_inputs(G, shape, p, False, 330)
    cal = {k: {kk: (vv.copy() if isinstance(vv, np.ndarray) else vv) for kk, vv in v.items()} for k, v in cal0.items()}
    cal["read"]["amp33"] = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in cal0["read"]["amp33"].items()}
    _plant(cal, what, where)
    with np.errstate(all="ignore"):
        ref = oracle.calibrate_arrays(ramp, cal)
    if what == "dark_nan" and where == "interior":
        nan_slope = np.isnan(ref["slope"])
        assert nan_slope[17, 200] and np.all(np.isfinite(ref["data"][1:, 17, 200])), "no NaN slope from group 0 alone in the oracle's output"
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), SLOT, cal) as cb:
        assert not ctx.caldir_first_group_safe(SLOT), "the screen passed a set with a bad value"
        got = run(cb, ctx, ramp, False, form=0 if what == "bias_inf" else 2, channel_lines=oracle_lines(ref, G, shape[1] // 128))
    assert_oracle(got, ref, f"{what} at an {where} pixel")


# ---- 4. eligibility: calls that take the full form
@gpu
@pytest.mark.parametrize("case", ("include_first", "two_reads_first", "f32_cube", "want_cube", "option_off"))
def test_calls_that_take_the_full_form(case):
    G, shape, p = 8, (40, 256), 8
    if case == "two_reads_first":
        rp = [[0, 1]] + [[r + 1 for r in g] for g in read_pattern(G)[1:]]
        cal = synth.make_caldir(*shape, read_pattern=rp, p_order=p, seed=340, bias_amplitude=2.0, bad_lin_frac=0.01)
        ramp = synth.make_ramp(cal, read_pattern=rp, seed=341, cr_frac=0.03, saturation_backup=0)
    else:
        rp, cal, ramp, _ref, _lines = clean_inputs(G, shape, p, False, 330)
    exclude_first = case != "include_first"
    if case == "f32_cube":
        ramp = dict(ramp)
        ramp["data"] = ramp["data"].astype(F32)
    with np.errstate(all="ignore"):
        ref = oracle.calibrate_arrays(ramp, cal, exclude_first=exclude_first)
    oracle_conditions(ref, G, 1 if exclude_first else 0)
    kw = dict(exclude_first=exclude_first, channel_lines=oracle_lines(ref, G, shape[1] // 128))
    if case == "want_cube":
        kw["want_cube"] = True
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), SLOT, cal) as cb, ctx.options(skip_first=0 if case == "option_off" else 1):
        assert ctx.caldir_first_group_safe(SLOT)
        got = run(cb, ctx, ramp, False, form=0 if case == "f32_cube" else 2, **kw)   # (an f32 cube takes the stage kernels)
    assert_oracle(got, ref, case)


# ---- 5. host side: the plan gives group 0 the weight zero
def _patterns():
    return [synth.READ_PATTERN_6, synth.READ_PATTERN_8, synth.READ_PATTERN_16] + [read_pattern(G) for G in range(5, 17)]


@pytest.mark.parametrize("rp", _patterns(), ids=lambda rp: f"g{len(rp)}_{sum(len(g) for g in rp)}reads")
def test_plan_gives_group_0_the_weight_zero(rp):
    """what skipping group 0 rests on, checked by the library when it makes a plan: K[0] == 0 in the full-ramp weights and in
    the two-point weights of every truncated variant"""
    meta = planmod.exposure_meta(rp, synth.FRAME_TIME)
    G = len(rp)
    lib = _native.load_library()
    K = planmod.construct_weights(planmod.ramp_opt_u(None), meta, True)
    assert K[0] == 0.0 and np.any(K[1:] != 0.0)
    for g in range(G - 1, 3, -1):   # the truncated variants as the library builds them (fitting.py:165-169)
        k = planmod._variant_weights(meta, K, g, 1, False)
        assert k[0] == 0.0 and k[1] != 0.0
    assert lib.rip_plan_desc_first_weight_zero(planmod.plan_desc(meta, K, True)) == 1
    # not with the first group included, and not with a weight on group 0
    K0 = planmod.construct_weights(planmod.ramp_opt_u(None), meta, False)
    assert K0[0] != 0.0
    assert lib.rip_plan_desc_first_weight_zero(planmod.plan_desc(meta, K0, False)) == 0
    Kbad = K.copy()
    Kbad[0] = 1e-30
    assert lib.rip_plan_desc_first_weight_zero(planmod.plan_desc(meta, Kbad, True)) == 0
