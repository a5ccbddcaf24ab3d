"""The jump test AT the threshold: the near-threshold ramps of jump_band_cases.py through every path that decides a jump flag from
an approximate significance and an error band, against the CPU oracle bit for bit -- flags, slope, both errors.

No kernel evaluates the variance of a tested difference in the reference's exact f64 accumulation order on its hot path: the stage
kernel (device_rampfit.h, fit_variant) uses an f32 A sigma^2 + B dvardt and redoes the difference exactly inside the relative band
"guard_band"; the fused kernel's full-ramp fit (fit_full_pk_a / _b) and its truncated refits (trunc_layers -> fit_full_regs) use
__logf, __frsqrt_rn, a reciprocal multiply and a packed fma, and accept the approximate decision outside a band of hand-derived
constants.  On random ramps a band ten times too narrow, a missing term or a wrong table slot in one of the twelve group-count
forms passes; here every case holds thousands of differences within 3e-6 of the threshold, on both sides, in every fit and slope
regime (test_host_jump_band.py holds the generator to that with the oracle alone), so a wrong accepted decision is a wrong flag.
Pixels whose threshold depends on the host's numpy (jump_band_cases.threshold_is_portable: about 4 % of them) are compared like all
others but carry no tuned difference: there the device's correctly rounded logarithm and numpy's may give either flag.

fitting.jump_detect (jumpdetect_kernel) returns the significance cube and has no approximate path: it is not among the cases."""

import numpy as np
import pytest
import torch  # noqa: F401  before libromanhip is loaded: torch brings its own copy of the HIP runtime, and the first one loaded must be the one both use
from chain_support import JUMP, assert_equal_outputs, assert_oracle, chain_context, loaded
from conftest import assert_same_bits

import jump_band_cases as jb
from romanimpreprocess_amd import pipeline
from romanimpreprocess_amd.utils import fitting

pytestmark = pytest.mark.gpu

SLOT = 13
INF = float("inf")
BOTH_FORMS = ("g8_f32", "g11_f32")   # also with skip_first = 0: the full and the skip-first form both meet the set


def _inputs(name):
    G, kdt, shape, exclude_first, seed, jump_pars = jb.CHAIN_CASES[name]
    cal, ramp, ref, lines, rec = jb.near_threshold_inputs(G, kdt, shape, exclude_first, seed, jump_pars)
    assert jb.regime_counts(rec, jump_pars)["near"] >= 1000
    return cal, ramp, ref, rec, dict(exclude_first=exclude_first, jump_pars=jump_pars, channel_lines=lines)


def _fused_against_oracle(name):
    cal, ramp, ref, rec, kw = _inputs(name)
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), SLOT, cal) as cb:
        got = cb.calibrate(SLOT, ramp, **kw)
        assert ctx.last_chain_form() == 2, "the fused kernel did not run"
        skipped = ctx.last_chain_first_group()
        with ctx.options(guard_band=INF):
            exact = cb.calibrate(SLOT, ramp, **kw)
            assert ctx.last_chain_form() == 2
        full = None
        if name in BOTH_FORMS:
            assert skipped == 1, "the form that skips the first group did not run"
            with ctx.options(skip_first=0):
                full = cb.calibrate(SLOT, ramp, **kw)
                assert ctx.last_chain_form() == 2 and ctx.last_chain_first_group() == 0
    assert_oracle(got, ref, f"{name}: fused kernel")
    assert_equal_outputs(got, exact, f"{name}: approximate + band against exact everywhere")
    if full is not None:
        assert_oracle(full, ref, f"{name}: fused kernel, first group not skipped")


def _stages_against_oracle(name):
    cal, ramp, ref, rec, kw = _inputs(name)
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), SLOT, cal) as cb, ctx.options(fused=0, chain2=0):
        got = cb.calibrate(SLOT, ramp, **kw)
        assert ctx.last_chain_form() == 0, "not the stage kernels"
        with ctx.options(guard_band=INF):
            exact = cb.calibrate(SLOT, ramp, **kw)
    assert_oracle(got, ref, f"{name}: stage kernels")
    assert_oracle(exact, ref, f"{name}: stage kernels, exact everywhere")


@pytest.mark.parametrize("name", list(jb.FUSED))
def test_fused_kernel_at_the_threshold(name):
    """every group count from 5 to 16 (f32 ipc4d; f64 for 8, 13 and 16; both starts for 8 and 11), default options"""
    _fused_against_oracle(name)


@pytest.mark.parametrize("name", list(jb.STAGE))
def test_stage_kernels_at_the_threshold(name):
    """the stage path is the only one for a count above 16, and the amplification in RipDiff::relerr grows with the ramp's length"""
    _stages_against_oracle(name)


@pytest.mark.parametrize("path", ("fused", "stages"))
@pytest.mark.parametrize("name", list(jb.CUSTOM))
def test_custom_jump_parameters_at_the_threshold(name, path):
    """steep: IthreshA != 1 (the fused path multiplies by f32(1 / IthreshA) where the reference divides) and a steeper threshold
    line; crossing: the threshold is <= 0 over part of the slope range, where the fused kernel's `pass` is false and every lane
    takes the exact path"""
    (_fused_against_oracle if path == "fused" else _stages_against_oracle)(name)


@pytest.mark.parametrize("guard", (1e-5, INF))
@pytest.mark.parametrize("name", list(jb.FIT_CASES))
def test_ramp_fit_function_with_f64_gain_at_the_threshold(name, guard):
    """fitting.ramp_fit on the oracle's f32 cube with an f64 gain plane (exact_variance<double>, dvardt in f64); the second case
    tunes the gain where the Poisson term dominates"""
    cube, rdq0, pdq0, gain, read, meta, expected, rec = jb.near_threshold_fit_inputs(*jb.FIT_CASES[name])
    assert gain.dtype == np.float64
    rdq, pdq = rdq0.copy(), pdq0.copy()
    caldir = {"gain": {"roman": {"data": gain}}, "read": {"roman": {"data": read}}}
    ctx = chain_context()
    with ctx.options(guard_band=guard):
        s, er, ep = fitting.ramp_fit(cube, rdq, pdq, meta, caldir, None, exclude_first=jb.FIT_CASES[name][2], ctx=ctx)
    assert_same_bits(rdq, expected[3], f"{name}: groupdq")
    assert_same_bits(pdq, expected[4], f"{name}: pixeldq")
    for got, want, what in zip((s, er, ep), expected[:3], ("slope", "err_read", "err_poisson")):
        assert_same_bits(got, want, f"{name}: {what}", zero_sign_ok=True)


def test_without_a_band_the_stage_kernels_miss_the_oracle():
    """The comparison is live on the device: with guard_band = 0 the stage kernels accept every f32 decision, and flags differ from
    the oracle's -- only where the generator put a difference at the threshold (or another difference of the pixel lies within 1e-5
    of it)."""
    cal, ramp, ref, rec, kw = _inputs("g8_f32")
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), SLOT, cal) as cb, ctx.options(fused=0, chain2=0, guard_band=0.0):
        got = cb.calibrate(SLOT, ramp, **kw)
        assert ctx.last_chain_form() == 0
    differs = np.any(got["groupdq"] != ref["groupdq"], axis=0)
    n = int(np.count_nonzero(differs))
    print(f"guard_band = 0: the group flags differ from the oracle's on {n} pixels")
    assert n >= 1, "the stage kernels without a band reproduce every flag: the set does not reach the band"
    assert np.all(((got["groupdq"] ^ ref["groupdq"]) & ~np.uint8(JUMP)) == 0), "flags other than JUMP_DET differ"
    explained = (rec["k"] >= 0) | (rec["other_rel"] < 1e-5)
    assert np.all(explained[differs]), f"{np.count_nonzero(differs & ~explained)} differing pixels have no difference near the threshold"
