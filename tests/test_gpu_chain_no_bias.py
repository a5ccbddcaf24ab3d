"""The fused kernel without its biascorr stream, and the bias state of a CALDIR set (``rip_caldir_bias_state``).

A set has a bias correction to make (PRESENT), has none (ABSENT: no biascorr file), or was given one whose every word is +0 and
that ``rip_caldir_upload`` dropped (DROPPED: ``S - (+0.0f)`` is ``S`` for every f32).  Calls on the last two, and calls whose
stage mask leaves ``STAGE_BIAS`` out, take the fused kernel with a biascorr descriptor of zero records on the base of dark.data:
the hardware's range check drops those loads, which return +0.  Every case asserts its branch -- the state of the set, the
kernel form, ``rip_last_chain_bias_stream``, the treatment of group 0 -- and compares with the CPU oracle bit for bit (as the other
chain tests do: the sign of a zero aside).  dark.data is near 13000 DN, so a descriptor that failed to drop its loads would show
on every science pixel.

Frames of 72 rows x 512 columns: three strips with two seams on the 256-column form, two strips on the 384-column forms, four
reference-pixel channels."""

from functools import lru_cache

import numpy as np
import pytest
import torch  # before libromanhip is loaded: torch brings its own copy of the HIP runtime, and the first one loaded must be the one both use
from chain_support import (F32, F64, JUMP, assert_equal_outputs, assert_oracle, calibrate_resident, chain_context, device_outputs, loaded,
                           make_band_ramp, oracle_lines, outputs_to_numpy, ramp_to_dev, read_pattern)

import oracle
from romanimpreprocess_amd import _native, pipeline, synth
from romanimpreprocess_amd._native import BIAS_ABSENT, BIAS_DROPPED, BIAS_PRESENT

SLOT, SLOT_B = 12, 13
NY, NX = 72, 512
NYA, NXA = NY - 8, NX - 8
gpu = pytest.mark.gpu


@lru_cache(maxsize=8)
def base(G, k64):
    """(read pattern, set WITHOUT biascorr, ramp) of G groups: flagged linearity pixels, cosmic rays, a saturating band"""
    rp = read_pattern(G)
    cal = synth.make_caldir(NY, NX, read_pattern=rp, p_order=8, seed=500 + G, with_biascorr=False, bad_lin_frac=0.005,
                            ipc_dtype=F64 if k64 else F32)
    assert "biascorr" not in cal and 12000.0 < float(cal["dark"]["data"].min())
    return rp, cal, make_band_ramp(cal, rp, NY, NX, 600 + G)


def with_bias(cal, data):
    """a copy of the set (the arrays shared) with this biascorr array; None: without the key"""
    cal2 = dict(cal)
    cal2.pop("biascorr", None)
    if data is not None:
        cal2["biascorr"] = {"data": np.ascontiguousarray(data, dtype=F32), "t0": 0.0}
    return cal2


def zeros(G):
    return np.zeros((G, NYA, NXA), dtype=F32)


def noisy(G, seed=9):
    return (2.0 * np.random.default_rng(seed).normal(size=(G, NYA, NXA))).astype(F32)


@lru_cache(maxsize=8)
def reference(G, k64, exclude_first):
    """the oracle's result on the set without biascorr -- what every set that corrects nothing must give -- and its channel lines"""
    rp, cal, ramp = base(G, k64)
    with np.errstate(all="ignore"):
        ref = oracle.calibrate_arrays(ramp, cal, exclude_first=exclude_first)
    assert np.count_nonzero(ref["pixeldq"] & JUMP) > 5, "no jump flags in the oracle's output"
    return ref, oracle_lines(ref, G, NX // 128)


def run(cb, ctx, slot, ramp, stream, skipped=None, form=2, **kw):
    """one host call; asserts the kernel form, whether the launch carried the bias stream and (where given) group 0's treatment"""
    got = cb.calibrate(slot, ramp, **kw)
    assert ctx.last_chain_form() == form, f"kernel form {ctx.last_chain_form()}, expected {form}"
    assert ctx.last_chain_bias_stream() == (1 if stream else 0), "not the expected bias stream"
    if skipped is not None:
        assert ctx.last_chain_first_group() == (1 if skipped else 0), "not the expected treatment of group 0"
    return got


# ---- 1. no biascorr file
ABSENT = [(6, False), (8, False), (8, True), (16, False), (16, True), (13, False)]


@gpu
@pytest.mark.parametrize("exclude_first", (True, False), ids=("skip", "full"))
@pytest.mark.parametrize("G,k64", ABSENT, ids=[f"g{G}_{'k64' if k else 'f32'}" for G, k in ABSENT])
def test_oracle_parity_without_the_file(G, k64, exclude_first):
    rp, cal, ramp = base(G, k64)
    ref, lines = reference(G, k64, exclude_first)
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), SLOT, cal) as cb:
        assert cb.bias_state(SLOT) == BIAS_ABSENT
        assert ctx.caldir_first_group_safe(SLOT), "a set without biascorr was not screened for the first group"
        got = run(cb, ctx, SLOT, ramp, False, skipped=exclude_first, exclude_first=exclude_first, channel_lines=lines)
    assert_oracle(got, ref, f"no biascorr file, {G} groups")


# ---- 2. the file is there and all +0 (the benchmark's set)
@gpu
@pytest.mark.parametrize("exclude_first", (True, False), ids=("skip", "full"))
@pytest.mark.parametrize("G,k64", [(8, False), (16, True)], ids=("g8_f32", "g16_k64"))
def test_oracle_parity_with_an_all_zero_array(G, k64, exclude_first):
    rp = read_pattern(G)
    cal = synth.make_caldir(NY, NX, read_pattern=rp, p_order=8, seed=520 + G, bias_amplitude=0.0, bad_lin_frac=0.005,
                            ipc_dtype=F64 if k64 else F32)
    assert "biascorr" in cal and not cal["biascorr"]["data"].view(np.uint32).any()
    ramp = make_band_ramp(cal, rp, NY, NX, 620 + G)
    with np.errstate(all="ignore"):
        ref = oracle.calibrate_arrays(ramp, cal, exclude_first=exclude_first)
    kw = dict(exclude_first=exclude_first, channel_lines=oracle_lines(ref, G, NX // 128))
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), SLOT, cal) as cb:
        assert cb.bias_state(SLOT) == BIAS_DROPPED
        assert ctx.caldir_first_group_safe(SLOT)
        got = run(cb, ctx, SLOT, ramp, False, skipped=exclude_first, **kw)
        with ctx.options(fused=0):
            stage = run(cb, ctx, SLOT, ramp, False, form=0, **kw)
    assert_oracle(got, ref, "all-zero biascorr")
    assert_equal_outputs(got, stage, "fused without the stream against the stage kernels")


# ---- 3. what must keep the stream
def _keepers(G):
    minus_zero, tiny, outside = zeros(G), zeros(G), zeros(G + 2)
    minus_zero[3, 20, 100] = -0.0
    tiny[G - 1, NYA - 1, NXA - 1] = 1e-30
    outside[0, 10, 10] = 5.0   # (a ramp of G groups uses the LAST G planes: planes 0 and 1 are not its own)
    return {"minus_zero": minus_zero, "tiny": tiny, "other_plane": outside}


@gpu
@pytest.mark.parametrize("what", ("minus_zero", "tiny", "other_plane"))
def test_one_sample_keeps_the_stream(what):
    G = 8
    rp, cal0, ramp = base(G, False)
    data = _keepers(G)[what]
    assert np.count_nonzero(data.view(np.uint32)) == 1
    cal = with_bias(cal0, data)
    with np.errstate(all="ignore"):
        ref = oracle.calibrate_arrays(ramp, cal)
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), SLOT, cal) as cb:
        assert cb.bias_state(SLOT) == BIAS_PRESENT
        got = run(cb, ctx, SLOT, ramp, True, skipped=True, channel_lines=oracle_lines(ref, G, NX // 128))
    assert_oracle(got, ref, what)


# ---- 4. a stage mask without the bias step
@gpu
@pytest.mark.parametrize("G,k64", [(8, False), (16, True)], ids=("g8_f32", "g16_k64"))
def test_stage_mask_without_bias(G, k64):
    rp, cal0, ramp = base(G, k64)
    ref, lines = reference(G, k64, True)
    cal = with_bias(cal0, noisy(G))
    with np.errstate(all="ignore"):
        ref_bias = oracle.calibrate_arrays(ramp, cal)
    assert not np.array_equal(ref_bias["slope"], ref["slope"]), "the bias correction does not show in the oracle's slopes"
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), SLOT, cal) as cb:
        assert cb.bias_state(SLOT) == BIAS_PRESENT
        got = run(cb, ctx, SLOT, ramp, False, skipped=True, stages=pipeline.STAGE_ALL & ~pipeline.STAGE_BIAS, channel_lines=lines)
        full = run(cb, ctx, SLOT, ramp, True, skipped=True, channel_lines=lines)
    assert_oracle(got, ref, "stage mask without STAGE_BIAS")
    assert_oracle(full, ref_bias, "the same set with every stage")


# ---- 5. errors and entry points
@gpu
@pytest.mark.parametrize("kind", ("all_zero", "non_zero"))
def test_too_few_planes_is_the_same_error(kind):
    G = 8
    rp, cal0, ramp = base(G, False)
    cal = with_bias(cal0, zeros(G - 1) if kind == "all_zero" else noisy(G - 1))
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), SLOT, cal) as cb:
        assert cb.bias_state(SLOT) == (BIAS_DROPPED if kind == "all_zero" else BIAS_PRESENT)
        with pytest.raises(ValueError, match=f"calibrate: biascorr has {G - 1} groups, ramp {G}"):
            cb.calibrate(SLOT, ramp)
        # (without the bias step the planes are not asked for, on either set)
        got = run(cb, ctx, SLOT, ramp, False, stages=pipeline.STAGE_ALL & ~pipeline.STAGE_BIAS, channel_lines=reference(G, False, True)[1])
    assert_oracle(got, reference(G, False, True)[0], "too few planes, no bias step")


@gpu
def test_batch_and_resident_calls_equal_the_host_call():
    G = 8
    rp, cal, _ramp = base(G, False)
    ramps = [make_band_ramp(cal, rp, NY, NX, 640 + i) for i in range(2)]
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), SLOT, cal) as cb:
        single = [run(cb, ctx, SLOT, r, False, skipped=True) for r in ramps]
        many = cb.calibrate_many(SLOT, ramps, want_groupdq=True)
        assert ctx.last_chain_form() == 2 and ctx.last_chain_bias_stream() == 0 and ctx.last_chain_first_group() == 1
        pid, _meta = cb.plan_for(rp, synth.FRAME_TIME)
        t = [ramp_to_dev(r) for r in ramps]
        o = [device_outputs(G, NY, NX) for _ in ramps]
        torch.cuda.synchronize()
        for i in range(2):
            calibrate_resident(cb, SLOT, pid, G, t[i], o[i])
        cb.synchronize()
        assert ctx.last_chain_form() == 2 and ctx.last_chain_bias_stream() == 0 and ctx.last_chain_first_group() == 1
        dev = [outputs_to_numpy(oi) for oi in o]
    for i in range(2):
        assert_equal_outputs(many[i], single[i], f"ramp {i}: batch against the host call")
        assert_equal_outputs(dev[i], single[i], f"ramp {i}: device-resident call")


@gpu
def test_two_slots_called_alternately():
    """the state of the launch is the call's, not the context's"""
    G = 8
    rp, cal0, ramp = base(G, False)
    ref0, lines = reference(G, False, True)
    cal1 = with_bias(cal0, noisy(G, 10))
    with np.errstate(all="ignore"):
        ref1 = oracle.calibrate_arrays(ramp, cal1)
    ctx = chain_context()
    cb = pipeline.Calibrator(ctx=ctx)
    with loaded(cb, SLOT, cal0), loaded(cb, SLOT_B, cal1):
        assert (cb.bias_state(SLOT), cb.bias_state(SLOT_B)) == (BIAS_ABSENT, BIAS_PRESENT)
        for i in range(4):
            a = run(cb, ctx, SLOT, ramp, False, skipped=True, channel_lines=lines)
            b = run(cb, ctx, SLOT_B, ramp, True, skipped=True, channel_lines=lines)
            assert_oracle(a, ref0, f"round {i}: the set without a bias correction")
            assert_oracle(b, ref1, f"round {i}: the set with one")


@gpu
def test_a_slot_reloaded_with_the_other_kind_of_set():
    G = 8
    rp, cal0, ramp = base(G, False)
    ref0, lines = reference(G, False, True)
    cal1 = with_bias(cal0, noisy(G, 11))
    with np.errstate(all="ignore"):
        ref1 = oracle.calibrate_arrays(ramp, cal1)
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), SLOT, cal0) as cb:
        for cal, state, ref in ((cal1, BIAS_PRESENT, ref1), (with_bias(cal0, zeros(G)), BIAS_DROPPED, ref0), (cal1, BIAS_PRESENT, ref1),
                                (cal0, BIAS_ABSENT, ref0)):
            cb.drop_caldir(SLOT)
            with pytest.raises(ValueError):
                ctx.caldir_bias_state(SLOT)
            cb.load_caldir(SLOT, cal)
            assert cb.bias_state(SLOT) == state
            got = run(cb, ctx, SLOT, ramp, state == BIAS_PRESENT, skipped=True, channel_lines=lines)
            assert_oracle(got, ref, f"reloaded, state {state}")
