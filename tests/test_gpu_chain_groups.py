"""The fused kernel's forms for every group count from 5 to 16 (chain2_form.h: an odd count runs the form of the next even count
with the second half of its last pair dead) against the CPU oracle and against the stage kernels, bit for bit.

Every case first checks the ORACLE's own output for the pixels that make the comparison mean something: jump flags, saturated
pixels that went through a truncated refit and -- for odd counts -- a jump into the last real group and pixels whose first
saturated group is the last real one (that is where a dead pair half would show).  The fit puts the flag of a jump between
groups i and j > i on group i, so a jump into the last group G-1 shows as JUMP_DET on group G-2."""

import numpy as np
import pytest
import torch  # before libromanhip is loaded: torch brings its own copy of the HIP runtime, and the first one loaded must be the one both use
from chain_support import (JUMP, OUT, SAT, assert_equal_outputs, assert_oracle, calibrate_resident, chain_context, device_outputs, loaded,
                           oracle_lines, outputs_to_numpy, ramp_to_dev, read_pattern)

import oracle
from romanimpreprocess_amd import pipeline, synth

pytestmark = pytest.mark.gpu

NEW_COUNTS = (5, 7, 9, 10, 11, 12, 13, 14, 15)


def _odd_conditions(ref, G):
    """odd G: the oracle flagged a jump into the last real group, and some pixel first saturates at the last real group"""
    if G % 2 == 0:
        return
    q = ref["groupdq"]
    assert np.count_nonzero(q[G - 2] & JUMP) > 0, "no jump into the last real group in the oracle's output"
    assert np.count_nonzero((q[G - 1] & SAT) & ~(q[G - 2] & SAT)) > 0, "no pixel first saturates at the last real group"


# ---- 1. every new form against the oracle on small frames
# per G: both starts x both ipc4d dtypes, the three Legendre orders rotating so that every (G, order) occurs; every (G, dtype)
# meets one 512-column frame (wider than a strip of any form: 256 or 384 columns), the other start a rotating smaller shape
_ORDERS = (8, 3, 10)
_SHAPES = ((40, 512), (48, 384), (56, 256), (32, 128))


def _small_cases():
    cases = []
    for gi, G in enumerate(NEW_COUNTS):
        for ci, (kdt, exclude_first) in enumerate(((np.float32, True), (np.float32, False), (np.float64, True), (np.float64, False))):
            p = _ORDERS[(gi + ci) % 3]
            shape = _SHAPES[0] if exclude_first else _SHAPES[(gi + ci) % 4]
            name = f"g{G}_np{p + 1}_start{int(exclude_first)}" + ("_k64" if kdt == np.float64 else "")
            cases.append(pytest.param(G, shape, p, exclude_first, kdt, 200 + 10 * gi + ci, id=name))
    return cases


def small_inputs(G, shape, p, exclude_first, kdt, seed):
    ny, nx = shape
    rp = read_pattern(G)
    cal = synth.make_caldir(ny, nx, read_pattern=rp, p_order=p, seed=seed, bias_amplitude=2.0, bad_lin_frac=0.01, ipc_dtype=kdt)
    # degenerate gains: the waves holding them leave the shared-reciprocal division for the division operator
    cal["gain"]["data"][20, 30] = 0.0
    cal["gain"]["data"][21, 40] = 1e-25
    cal["gain"]["data"][22, 50] = -1.5
    # (no backed-up saturation flags: a pixel may first saturate at the last group)
    ramp = synth.make_ramp(cal, read_pattern=rp, seed=seed + 1, cr_frac=0.03, saturation_backup=0)
    with np.errstate(all="ignore"):
        ref = oracle.calibrate_arrays(ramp, cal, exclude_first=exclude_first)
    return rp, cal, ramp, ref


def small_conditions(ref, G):
    assert np.count_nonzero(ref["pixeldq"] & JUMP) > 5
    _odd_conditions(ref, G)


@pytest.mark.parametrize("G,shape,p,exclude_first,kdt,seed", _small_cases())
def test_new_forms_vs_oracle(G, shape, p, exclude_first, kdt, seed):
    ny, nx = shape
    rp, cal, ramp, ref = small_inputs(G, shape, p, exclude_first, kdt, seed)
    small_conditions(ref, G)
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), 4, cal) as cb:
        assert cb.chain_form_for(4, G) == 2
        got = cb.calibrate(4, ramp, exclude_first=exclude_first, want_cube=True, channel_lines=oracle_lines(ref, G, nx // 128))
        assert ctx.last_chain_form() == 2, "the fused kernel did not run"
        assert_oracle(got, ref, "fused kernel", cube=True)


# ---- 2. seams: several column strips and row ranges, fused against stage kernels
SEAMS = [(7, np.float32), (7, np.float64), (11, np.float32), (11, np.float64), (12, np.float32), (10, np.float64), (14, np.float64)]


def seam_inputs(G, kdt):
    ny, nx = 1160, 896
    rp = read_pattern(G)
    cal = synth.make_caldir(ny, nx, read_pattern=rp, p_order=8, seed=31, bias_amplitude=2.0, bad_lin_frac=0.005, ipc_dtype=kdt)
    ramp = synth.make_ramp(cal, read_pattern=rp, seed=32, cr_frac=0.02, saturation_backup=0)
    return rp, cal, ramp


def big_conditions(ref, G):
    assert np.count_nonzero(ref["pixeldq"] & JUMP) > 1000 and np.count_nonzero(ref["pixeldq"] & SAT) > 100
    _odd_conditions(ref, G)


def _fused_vs_stages(cb, ctx, slot, ramp, G):
    outs = []
    for form in (2, 0):   # 2: the fused kernel, 0: stage kernels
        with ctx.options(fused=1 if form else 0, chain2=1 if form else 0):
            outs.append(cb.calibrate(slot, ramp, want_cube=True))
            assert ctx.last_chain_form() == form
    assert_equal_outputs(outs[0], outs[1], "fused vs stage kernels", keys=("cube",) + OUT)


@pytest.mark.parametrize("G,kdt", SEAMS, ids=[f"g{g}_{'k64' if k == np.float64 else 'f32'}" for g, k in SEAMS])
def test_new_forms_agree_with_stage_kernels_across_seams(G, kdt):
    rp, cal, ramp = seam_inputs(G, kdt)
    with np.errstate(all="ignore"):
        ref = oracle.calibrate_arrays(ramp, cal)
    big_conditions(ref, G)
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), 5, cal) as cb:
        _fused_vs_stages(cb, ctx, 5, ramp, G)


# ---- 3. full width: 33 (17) strips, frame-edge lanes emitting
FULL_WIDTH = [(9, np.float32), (13, np.float64)]


def full_width_inputs(G, kdt):
    ny, nx = 264, 4096
    rp = read_pattern(G)
    cal = synth.make_caldir(ny, nx, read_pattern=rp, p_order=8, seed=71, bias_amplitude=2.0, bad_lin_frac=0.005, ipc_dtype=kdt)
    ramp = synth.make_ramp(cal, read_pattern=rp, seed=72, cr_frac=0.02, saturation_backup=0)
    return rp, cal, ramp


@pytest.mark.parametrize("G,kdt", FULL_WIDTH, ids=["g9_f32", "g13_k64"])
def test_new_forms_full_width_vs_oracle_and_stage_kernels(G, kdt):
    rp, cal, ramp = full_width_inputs(G, kdt)
    with np.errstate(all="ignore"):
        ref = oracle.calibrate_arrays(ramp, cal)
    big_conditions(ref, G)
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), 6, cal) as cb:
        got = cb.calibrate(6, ramp, want_cube=True, channel_lines=oracle_lines(ref, G, 4096 // 128))
        assert ctx.last_chain_form() == 2
        assert_oracle(got, ref, "fused kernel", cube=True)
        _fused_vs_stages(cb, ctx, 6, ramp, G)


# ---- 5. the batch and the device-resident entry points
@pytest.mark.parametrize("G", [7, 12])
def test_batch_of_host_ramps_equals_single_calls(G):
    rp = read_pattern(G)
    ny, nx = 72, 256
    cal = synth.make_caldir(ny, nx, read_pattern=rp, p_order=8, seed=41, bias_amplitude=2.0)
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), 2, cal) as cb:
        ramps = [synth.make_ramp(cal, read_pattern=rp, seed=50 + i, cr_frac=0.02, saturation_backup=0) for i in range(4)]
        singles = []
        for r in ramps:
            singles.append(cb.calibrate(2, r))
            assert ctx.last_chain_form() == 2
        many = cb.calibrate_many(2, ramps, want_groupdq=True)
        assert ctx.last_chain_form() == 2
        assert len(many) == len(ramps)
        for i, (a, b) in enumerate(zip(many, singles)):
            assert_equal_outputs(a, b, f"ramp {i}")
        assert np.count_nonzero(singles[0]["pixeldq"] & JUMP) > 5
        assert not np.array_equal(singles[0]["slope"], singles[1]["slope"])


@pytest.mark.parametrize("G", [7, 12])
def test_device_resident_call_equals_host_call(G):
    rp = read_pattern(G)
    ny, nx = 136, 512
    cal = synth.make_caldir(ny, nx, read_pattern=rp, p_order=8, seed=43, bias_amplitude=2.0)
    ramp = synth.make_ramp(cal, read_pattern=rp, seed=44, cr_frac=0.02, saturation_backup=0)
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), 9, cal) as cb:
        host = cb.calibrate(9, ramp)
        assert ctx.last_chain_form() == 2
        pid, _meta = cb.plan_for(rp, synth.FRAME_TIME)
        t, o = ramp_to_dev(ramp), device_outputs(G, ny, nx)
        torch.cuda.synchronize()
        for _ in range(2):   # twice: the second call's pre-pass runs ahead of the first call's kernel
            calibrate_resident(cb, 9, pid, G, t, o)
        cb.synchronize()
        assert ctx.last_chain_form() == 2
        assert_equal_outputs(outputs_to_numpy(o), host, "device-resident against host call")
        assert np.count_nonzero(host["pixeldq"] & JUMP) > 5
