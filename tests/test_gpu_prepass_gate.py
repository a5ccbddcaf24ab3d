"""The gate in front of an overlapped reference-pixel pre-pass (calibrate.hip: prepass_gate; option "prepass_gate").

Every workgroup of a fused launch counts itself in as it starts; the pre-pass of the NEXT call, on the second stream, starts behind
one wave that waits until that count has reached the host's running total (or until its bound, after which it gives up).  The gate
orders nothing that a result needs, so every case here runs a sequence of back-to-back device-resident calls
(``inputs_complete=True``, no synchronisation in between) that alternate between two different ramps -- a stale or early table
would show -- and compares slope, err_read, err_poisson, pixeldq and groupdq of EVERY call bit for bit, gate on against gate off;
the last call of each ramp is compared with the CPU oracle (bit for bit, the sign of a zero aside, with the oracle's channel
lines handed in on the device; with the lines fitted on the device -- the only way to the form that skips group 0 -- flags bit for
bit and values within the tolerance the other chain tests use for device-fitted lines).  What ``rip_last_prepass_gate`` reports
(it waits for the streams) is read in a second pass over the same sequence."""

from functools import lru_cache

import numpy as np
import pytest
import torch  # before libromanhip is loaded: torch brings its own copy of the HIP runtime, and the first one loaded must be the one both use
from conftest import assert_same_bits
from chain_support import (F32, F64, assert_equal_outputs, assert_oracle, chain_context, device_outputs, loaded, oracle_lines,
                           outputs_to_numpy, read_pattern, to_dev)

import oracle
from romanimpreprocess_amd import _native, pipeline, synth

SLOT = 13
GATE_US = 100    # the bound the cases run the gate with (microseconds); the library's default is 0: no gate
NONE, RELEASED, GAVE_UP = 0, 1, 2
gpu = pytest.mark.gpu


@lru_cache(maxsize=4)
def inputs(G, shape, k64, p, seed):
    """a CALDIR set, two different ramps (cosmic rays, saturating pixels), the oracle's results and the channel lines it used"""
    ny, nx = shape
    rp = read_pattern(G)
    cal = synth.make_caldir(ny, nx, read_pattern=rp, p_order=p, seed=seed, bias_amplitude=2.0, bad_lin_frac=0.01,
                            ipc_dtype=F64 if k64 else F32)
    ramps = [synth.make_ramp(cal, read_pattern=rp, seed=seed + 1 + i, cr_frac=0.03, saturation_backup=0) for i in range(2)]
    # distinct reference-output levels: the row corrections of the two ramps differ by much more than rounding
    ramps[1]["amp33"] = (ramps[1]["amp33"].astype(np.int32) + 40 * (np.arange(ny)[None, :, None] % 7)).astype(np.uint16)
    with np.errstate(all="ignore"):
        refs = [oracle.calibrate_arrays(r, cal) for r in ramps]
    assert not np.array_equal(refs[0]["slope"], refs[1]["slope"])
    assert all(np.count_nonzero(r["pixeldq"] & 4) > 5 for r in refs), "no jump flags in the oracle's output"
    assert not np.array_equal(refs[0]["refpix_diag"][1]["channels"], refs[1]["refpix_diag"][1]["channels"])
    return rp, cal, ramps, refs, [oracle_lines(r, G, nx // 128) for r in refs]


class Resident:
    """the two ramps of `inputs` on the device (with group 0 marked DO_NOT_USE, as the host path does for an excluded first
    group) and a plan for them on the context of `cb`; the caller holds the set in `slot`: ``with loaded(cb, slot, res.cal)``"""

    def __init__(self, cb, slot, G, shape, k64, p, seed, own_lines=False):
        self.rp, self.cal, self.ramps, self.refs, self.lines = inputs(G, shape, k64, p, seed)
        self.cb, self.slot, self.G, self.shape = cb, slot, G, shape
        self.pid, _meta = cb.plan_for(self.rp, synth.FRAME_TIME)
        self.t = []
        for r, ln in zip(self.ramps, self.lines):
            g = r["groupdq"].copy()
            g[0] |= 1
            self.t.append([to_dev(r["data"]), to_dev(r["amp33"]), to_dev(g), to_dev(r["pixeldq"]),
                           None if own_lines else to_dev(np.asarray(ln, dtype=np.float64))])
        torch.cuda.synchronize()

    def outputs(self, n):
        return [device_outputs(self.G, *self.shape) for _ in range(n)]

    def call(self, i, o):
        """call i of a sequence (ramp i % 2), queued; device-resident, complete inputs: the pre-pass runs ahead"""
        t = self.t[i % 2]
        rd = _native.RampDesc()
        rd.location, rd.ngrp = _native.RIP_DEVICE, self.G
        rd.data, rd.data_dtype = t[0].data_ptr(), _native.RIP_U16
        rd.amp33, rd.groupdq, rd.pixeldq = t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr()
        rd.channel_lines = None if t[4] is None else t[4].data_ptr()
        rd.inputs_ready = _native.RIP_INPUTS_COMPLETE
        out = _native.Outputs()
        out.location = _native.RIP_DEVICE
        out.slope, out.err_read, out.err_poisson, out.pixeldq, out.groupdq = (x.data_ptr() for x in o)
        self.cb.ctx.calibrate_raw(self.slot, self.pid, pipeline.STAGE_ALL, rd, out)


def as_numpy(o):
    return [outputs_to_numpy(oi) for oi in o]


def unarmed(res):
    """one call WITHOUT the counter, so that the sequence that follows starts like the first call on a context: no gate"""
    with res.cb.ctx.options(prepass_gate=0, fused=1):
        res.call(0, res.outputs(1)[0])
        res.cb.synchronize()


def sequence(res, gate, n=6, fused=None):
    """with the option at `gate`: n calls back to back without a synchronisation, then the same n calls again with
    rip_last_prepass_gate read after each (each pass behind a call without the counter);
    -> (outputs of the first pass, per call; gate state per call of the second pass; kernel form per call; give-ups added)"""
    ctx = res.cb.ctx
    fused = fused or [1] * n
    unarmed(res)
    with ctx.options(prepass_gate=gate):
        _, giveups0 = ctx.last_prepass_gate()
        o = res.outputs(n)
        for i in range(n):
            with ctx.options(fused=fused[i]):
                res.call(i, o[i])
        res.cb.synchronize()
        got = as_numpy(o)
        _, giveups1 = ctx.last_prepass_gate()
    unarmed(res)
    with ctx.options(prepass_gate=gate):
        o2 = res.outputs(n)
        states, forms = [], []
        for i in range(n):
            with ctx.options(fused=fused[i]):
                res.call(i, o2[i])
            states.append(ctx.last_prepass_gate()[0])
            forms.append(ctx.last_chain_form())
    for i, (a, b) in enumerate(zip(got, as_numpy(o2))):
        assert_equal_outputs(a, b, f"call {i}: queued against synchronised")
    return got, states, forms, giveups1 - giveups0


def on_and_off(res, n=6, fused=None, gate=GATE_US):
    """the sequence with the gate at `gate` and with the gate off; every call bit for bit; the last call of each ramp against
    the oracle; -> (states with the gate on, forms, give-ups added with the gate on)"""
    on, states, forms, giveups = sequence(res, gate, n, fused)
    off, states_off, _forms, giveups_off = sequence(res, 0, n, fused)
    assert states_off == [NONE] * n and giveups_off == 0, f"option off: gates {states_off}, give-ups {giveups_off}"
    for i in range(n):
        assert_equal_outputs(on[i], off[i], f"call {i}: gate on against gate off")
    if res.t[0][4] is not None:
        for i in (n - 2, n - 1):
            assert_oracle(on[i], res.refs[i % 2], f"call {i} (ramp {i % 2}), gate on")
            assert_oracle(off[i], res.refs[i % 2], f"call {i} (ramp {i % 2}), gate off")
    return on, states, forms, giveups


def queued(states):
    return [s in (RELEASED, GAVE_UP) for s in states]


# ---- 1. all calls fused, 8 groups, f32 ipc4d: 512 columns = two strips of the 256-column form and a last strip of 8 live columns
@gpu
def test_all_fused_8_groups():
    cb = pipeline.Calibrator(ctx=chain_context())
    res = Resident(cb, SLOT, 8, (64, 512), False, 8, 500)
    with loaded(cb, SLOT, res.cal):
        _on, states, forms, _g = on_and_off(res)
    assert forms == [2] * 6
    assert states[0] == NONE, "a gate on the first call of a sequence that follows a call without the counter"
    assert queued(states) == [False] + [True] * 5, f"gates: {states}"


# ---- 2. the other forms: 16 groups (384 columns, three strips at 768); f64 ipc4d x 8 groups, whose pre-pass runs in front of its
# own ramp by default (no gate) and beside the previous one with overlap = 1 (gate)
@gpu
@pytest.mark.parametrize("G,k64,overlap", [(16, False, -1), (8, True, -1), (8, True, 1)], ids=["g16_f32", "g8_k64_by_situation", "g8_k64_overlap"])
def test_other_forms(G, k64, overlap):
    ctx = chain_context()
    cb = pipeline.Calibrator(ctx=ctx)
    res = Resident(cb, SLOT, G, (64, 768), k64, 3 if k64 else 10, 510 + G)
    with loaded(cb, SLOT, res.cal), ctx.options(overlap=overlap):
        _on, states, forms, _g = on_and_off(res)
    assert forms == [2] * 6
    if k64 and overlap == -1:
        assert states == [NONE] * 6, f"a gate in front of a pre-pass that runs on the main stream: {states}"
    else:
        assert queued(states) == [False] + [True] * 5, f"gates: {states}"


# ---- 3. mixed paths: calls 3 and 4 take the stage kernels.  The bound is long here, so that a running total that had gone wrong
# would show as a give-up instead of passing by timing: every queued gate must be RELEASED by the counter.
@gpu
def test_mixed_fused_and_stage_kernel_calls():
    cb = pipeline.Calibrator(ctx=chain_context())
    fused = [1, 1, 0, 0, 1, 1, 1]
    res = Resident(cb, SLOT, 8, (64, 512), False, 8, 500)
    with loaded(cb, SLOT, res.cal):
        _on, states, forms, giveups = on_and_off(res, n=7, fused=fused, gate=200000)
    assert forms == [2, 2, 0, 0, 2, 2, 2]
    # call 3 follows a fused call (its pre-pass is gated behind THAT launch); calls 4 and 5 follow stage-kernel calls
    assert states == [NONE, RELEASED, RELEASED, NONE, NONE, RELEASED, RELEASED], f"gates: {states}"
    assert giveups == 0, f"{giveups} give-ups in the unsynchronised pass"


# ---- 4. a bound of one microsecond: released or given up, by timing; the results are the same
@gpu
def test_tiny_bound():
    cb = pipeline.Calibrator(ctx=chain_context())
    res = Resident(cb, SLOT, 8, (64, 512), False, 8, 500)
    with loaded(cb, SLOT, res.cal):
        _on, states, _forms, _g = on_and_off(res, gate=1)
    assert states[0] == NONE and queued(states) == [False] + [True] * 5, f"gates: {states}"


# ---- 5. two contexts on one device, calls interleaved (the realisations workload): each has its own counter and total
@gpu
def test_two_contexts_interleaved():
    ctx = chain_context()
    ctx2 = _native.Context(0)   # (a new context starts at the defaults)
    cbs = [pipeline.Calibrator(ctx=ctx), pipeline.Calibrator(ctx=ctx2)]
    n = 6
    try:
        res = [Resident(cbs[0], SLOT, 8, (64, 512), False, 8, 500), Resident(cbs[1], SLOT, 8, (96, 512), False, 8, 520)]
        got, giveups = {}, {}
        with loaded(cbs[0], SLOT, res[0].cal), loaded(cbs[1], SLOT, res[1].cal):
            for gate in (200000, 0):
                with ctx.options(prepass_gate=gate), ctx2.options(prepass_gate=gate):
                    base = [r.cb.ctx.last_prepass_gate()[1] for r in res]
                    o = [r.outputs(n) for r in res]
                    for i in range(n):
                        for r, oo in zip(res, o):
                            r.call(i, oo[i])
                    states = [r.cb.ctx.last_prepass_gate() for r in res]   # (waits for the streams of its context)
                got[gate] = [as_numpy(oo) for oo in o]
                giveups[gate] = [s[1] - b for s, b in zip(states, base)]
                assert [s[0] for s in states] == ([RELEASED] * 2 if gate else [NONE] * 2), f"gate {gate}: last gates {states}"
        assert giveups[200000] == [0, 0], f"give-ups per context: {giveups[200000]}"
        for c, r in enumerate(res):
            for i in range(n):
                assert_equal_outputs(got[200000][c][i], got[0][c][i], f"context {c} call {i}: gate on against gate off")
            for i in (n - 2, n - 1):
                assert_oracle(got[200000][c][i], r.refs[i % 2], f"context {c} call {i}")
    finally:
        ctx2.close()


# ---- 6. both instantiations carry the counter add: the form that skips group 0 (reached only with the lines fitted on the device)
# and the full form
@gpu
@pytest.mark.parametrize("skip", (1, 0))
def test_skip_first_on_and_off(skip):
    ctx = chain_context()
    cb = pipeline.Calibrator(ctx=ctx)
    res = Resident(cb, SLOT, 8, (64, 512), False, 8, 500, own_lines=True)
    with loaded(cb, SLOT, res.cal), ctx.options(skip_first=skip):
        assert ctx.caldir_first_group_safe(SLOT)
        on, states, forms, _g = on_and_off(res)
        assert ctx.last_chain_first_group() == skip, "not the expected treatment of group 0"
        host = [cb.calibrate(SLOT, r) for r in res.ramps]   # the same lines, fitted on the device, through a host call
    assert forms == [2] * 6 and queued(states) == [False] + [True] * 5, f"forms {forms}, gates {states}"
    for i in (4, 5):
        assert_equal_outputs(on[i], host[i % 2], f"call {i} against a host call")
        ref = res.refs[i % 2]
        # device-fitted lines against LAPACK's: flags identical, values within the tolerance of the other chain tests
        assert_same_bits(on[i]["pixeldq"], ref["pixeldq"], f"call {i}: pixeldq (device lines)")
        assert_same_bits(on[i]["groupdq"], ref["groupdq"], f"call {i}: groupdq (device lines)")
        for k in ("slope", "err_read", "err_poisson"):
            np.testing.assert_allclose(on[i][k], ref[k], rtol=1e-5, atol=1e-7, err_msg=f"call {i}: {k} (device lines)")
