"""Level-1 exposures stored with the reference read subtracted (rip_stage_decode_reference_read, rip_ramp_desc::reference_read):
the decode kernel against numpy, and the chain, the batch, the device path and the driver on an encoded ramp against the same
exposure handed over plain."""

import ctypes as C

import numpy as np
import pytest
import torch  # before libromanhip is loaded: torch brings its own copy of the HIP runtime, and the first one loaded must be the one both use
from chain_support import (assert_equal_outputs, assert_oracle, calibrate_resident, chain_context, device_outputs, loaded, oracle_lines,
                           outputs_to_numpy, to_dev)
from conftest import assert_same_bits
from refread_ref import NX, NY, chain_inputs, decode, encode_ramp

import oracle
from oracle import saturation
from romanimpreprocess_amd import _native, calio, pipeline, synth
from romanimpreprocess_amd.L1_to_L2 import gen_cal_image

pytestmark = pytest.mark.gpu

HOST, DEVICE = _native.RIP_HOST, _native.RIP_DEVICE
# the sizes at which the kernel takes another path: below, at and past one octet; a plane that is no multiple of eight (every
# plane but the first then starts off a 16-byte boundary: one thread per pixel, more than one block); whole octets in two blocks
SIZES = (1, 7, 8, 9, 4101, 4096)
OFFSETS = (0, 1000, 65535, -5)
SLOT = 4


def stage_inputs(ngrp, n, seed):
    """random u16 samples with both ends of the range planted in both arrays, so that both clamps and the count are exercised"""
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 65536, size=(ngrp, n), dtype=np.uint16)
    ref = rng.integers(0, 65536, size=n, dtype=np.uint16)
    data[:, 0], ref[0] = 65535, 65535
    if n > 1:
        data[:, -1], ref[-1] = 0, 0
    if n > 4:
        data[0, 1], ref[1], data[0, 2], ref[2] = 65535, 0, 0, 65535
    return data, ref


def decode_host(ctx, data, ref, offset):
    out = np.full(data.shape, 0xABCD, np.uint16)
    count = C.c_uint64(12345)
    ctx.check(ctx.lib.rip_stage_decode_reference_read(ctx.h, data.ctypes.data, data.shape[0], data.shape[1], ref.ctypes.data, offset,
                                                      HOST, out.ctypes.data, C.byref(count)))
    return out, int(count.value)


def decode_device(cb, data, ref, offset, in_place, shift=0):
    """on tensors; shift = 1: every array is a view that starts one element into its allocation"""
    def dev(a):
        flat = np.concatenate([np.zeros(shift, np.uint16), a.reshape(-1)])
        return to_dev(flat)[shift:]

    t_data, t_ref = dev(data), dev(ref)
    t_out = t_data if in_place else dev(np.full(data.shape, 0xABCD, np.uint16))
    torch.cuda.synchronize()
    bad = cb.decode_reference_read(t_data.data_ptr(), data.shape[0], data.shape[1], t_ref.data_ptr(), offset,
                                   None if in_place else t_out.data_ptr(), want_count=True)
    if not in_place:
        assert_same_bits(t_data.cpu().numpy().view(np.uint16).reshape(data.shape), data, "the input of an out-of-place call")
    return t_out.cpu().numpy().view(np.uint16).reshape(data.shape), bad


@pytest.mark.parametrize("where", ["host", "device", "device_in_place"])
def test_decode_against_numpy(where):
    ctx = chain_context()
    cb = pipeline.Calibrator(ctx=ctx)
    low = high = counted = 0
    for n in SIZES:
        for ngrp in (1, 3):
            data, ref = stage_inputs(ngrp, n, 100 * n + ngrp)
            for offset in OFFSETS:
                want, bad = decode(data, ref, offset)
                v = data.astype(np.int64) + ref.astype(np.int64)[None] - offset
                low, high, counted = low + np.count_nonzero(v < 0), high + np.count_nonzero(v > 65535), counted + bad
                if where == "host":
                    got, n_bad = decode_host(ctx, data, ref, offset)
                else:
                    got, n_bad = decode_device(cb, data, ref, offset, where == "device_in_place")
                what = f"{where}: n = {n}, {ngrp} groups, offset {offset}"
                assert_same_bits(got, want, what)
                assert n_bad == bad, f"{what}: {n_bad} samples counted, numpy counts {bad}"
    assert low > 50 and high > 50 and counted == low + high


@pytest.mark.parametrize("n", [4101, 4096])
def test_decode_on_a_misaligned_view(n):
    """tensor views that start one element into their allocation: a base pointer off the 16-byte boundary, one thread per pixel"""
    cb = pipeline.Calibrator(ctx=chain_context())
    data, ref = stage_inputs(3, n, 7)
    want, bad = decode(data, ref, 1000)
    for in_place in (False, True):
        got, n_bad = decode_device(cb, data, ref, 1000, in_place, shift=1)
        assert_same_bits(got, want, f"misaligned, in place {in_place}")
        assert n_bad == bad and bad > 0


def test_decode_refusals():
    """every refusal is an error and touches nothing: neither the output nor the count"""
    ctx = chain_context()
    data, ref = stage_inputs(3, 64, 1)
    buf = np.full(3 * 64 + 8, 0xABCD, np.uint16)
    buf[8:] = data.reshape(-1)
    out = np.full(data.shape, 0xABCD, np.uint16)
    count = C.c_uint64(12345)
    d, r, o, c = data.ctypes.data, ref.ctypes.data, out.ctypes.data, C.addressof(count)
    u16 = 2
    cases = {
        "data NULL": (None, 3, 64, r, 0, HOST, o, c), "reference NULL": (d, 3, 64, None, 0, HOST, o, c),
        "out NULL": (d, 3, 64, r, 0, HOST, None, c), "count NULL": (d, 3, 64, r, 0, HOST, o, None),
        "no group": (d, 0, 64, r, 0, HOST, o, c), "no pixel": (d, 3, 0, r, 0, HOST, o, c),
        "offset above 2^30": (d, 3, 64, r, 2**30 + 1, HOST, o, c), "offset below -2^30": (d, 3, 64, r, -2**30 - 1, HOST, o, c),
        "unknown location": (d, 3, 64, r, 0, 7, o, c),
        "out overlaps data from below": (buf.ctypes.data + 8 * u16, 3, 64, r, 0, HOST, buf.ctypes.data, c),
        "out overlaps data from above": (buf.ctypes.data, 3, 64, r, 0, HOST, buf.ctypes.data + 8 * u16, c),
        "device: out overlaps data": (buf.ctypes.data + 8 * u16, 3, 64, r, 0, DEVICE, buf.ctypes.data, c),
    }
    before = buf.copy()
    for what, args in cases.items():
        rc = ctx.lib.rip_stage_decode_reference_read(ctx.h, *args)
        assert rc == -1, f"{what}: status {rc}"
        with pytest.raises(ValueError):
            ctx.check(rc)
        assert count.value == 12345 and np.all(out == 0xABCD) and np.array_equal(buf, before), what
    ctx.synchronize()
    # the largest offsets that are taken
    for offset in (2**30, -2**30):
        got, n_bad = decode_host(ctx, data, ref, offset)
        want, bad = decode(data, ref, offset)
        assert_same_bits(got, want, f"offset {offset}")
        assert n_bad == bad == data.size


# ---- the chain
def encoded(ramp, offset):
    """the encoded form of the test's own input; the condition everything below rests on: the encoder clipped nothing, so that
    decode o encode is the identity on data[1:] and amp33[1:]"""
    enc, clipped = encode_ramp(ramp, offset)
    assert clipped == 0, f"the encoder clipped {clipped} samples of the test's ramp at offset {offset}"
    return enc


@pytest.mark.parametrize("k64,offset", [(False, 1000), (True, 4000)])
def test_encoded_equals_plain(k64, offset):
    """(a), (b): every bit of the five outputs, against the plain ramp on the device and against the oracle; the fused form ran"""
    cal, ramp, plain, ref = chain_inputs(k64)
    enc = encoded(ramp, offset)
    lines = oracle_lines(ref, 7, NX // 128)
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), SLOT, cal) as cb:
        a = cb.calibrate(SLOT, enc, exclude_first=False, channel_lines=lines)
        assert ctx.last_chain_form() == 2, "the encoded ramp did not take the fused kernel"
        b = cb.calibrate(SLOT, plain, exclude_first=False, channel_lines=lines)
        assert ctx.last_chain_form() == 2
        # only the cube encoded: amp33 as stored
        half = dict(enc, amp33=plain["amp33"], reference_amp33=None)
        c = cb.calibrate(SLOT, half, exclude_first=False, channel_lines=lines)
    assert_equal_outputs(a, b, "encoded against plain")
    assert_equal_outputs(c, b, "cube encoded, amp33 plain, against plain")
    assert_oracle(a, ref, "encoded against the oracle's plain run")
    assert np.count_nonzero(a["pixeldq"] & 4) > 50 and np.count_nonzero(a["pixeldq"] & 2) > 50


def test_encoded_equals_plain_with_device_saturation_flags():
    """(a) with dq-init and saturation flagging on the device behind the decoding: groupdq None, pixeldq the mask"""
    cal, ramp, plain, _ = chain_inputs(False)
    mask = cal["mask"]["dq"].copy()
    enc = dict(encoded(ramp, 4000), groupdq=None, pixeldq=mask)
    r0 = dict(plain, groupdq=np.zeros(plain["data"].shape, np.uint8), pixeldq=mask.copy())
    saturation.flag_saturation(r0, cal["saturation"]["data"], backup=1, skip_firstn=1, sat_dq=cal["saturation"]["dq"])
    with np.errstate(all="ignore"):
        ref = oracle.calibrate_arrays(r0, cal, exclude_first=False)
    lines = oracle_lines(ref, 7, NX // 128)
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), SLOT, cal) as cb:
        a = cb.calibrate(SLOT, enc, exclude_first=False, channel_lines=lines, flag_saturation=True)
        assert ctx.last_chain_form() == 2
        b = cb.calibrate(SLOT, dict(plain, groupdq=None, pixeldq=mask), exclude_first=False, channel_lines=lines, flag_saturation=True)
    assert_equal_outputs(a, b, "encoded against plain, flags made on the device")
    assert_oracle(a, ref, "encoded against the oracle's plain run, flags made on the device")
    assert np.count_nonzero(a["groupdq"] & 2) > 50


def second_ramp(cal):
    return synth.make_ramp(cal, read_pattern=chain_inputs(False)[1]["read_pattern"], seed=33, cr_frac=0.05, saturation_backup=0)


def test_batch_of_encoded_ramps():
    """(c): calibrate_many of two encoded ramps (different exposures, different offsets) equals the two single calls; a batch
    whose second ramp does not decode fails and reports the first as good"""
    cal, ramp, _, _ = chain_inputs(False)
    encs = [encoded(ramp, 1000), encoded(second_ramp(cal), 4000)]
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), SLOT, cal) as cb:
        singles = [cb.calibrate(SLOT, e, exclude_first=False) for e in encs]
        many = cb.calibrate_many(SLOT, encs, exclude_first=False, want_groupdq=True)
        for i, (m, s) in enumerate(zip(many, singles)):
            assert_equal_outputs(m, s, f"batch against single call, ramp {i}")
        assert np.count_nonzero(singles[0]["slope"] != singles[1]["slope"]) > 1000
        bad = dict(encs[1], reference_read=np.zeros((NY, NX), np.uint16), data_encoding_offset=70000)
        with pytest.raises(ValueError, match="ramp 1"):
            cb.calibrate_many(SLOT, [encs[0], bad, encs[1]], exclude_first=False, want_groupdq=True)
        assert ctx.lib.rip_calibrate_batch_completed(ctx.h) == 1
        again = cb.calibrate_many(SLOT, encs, exclude_first=False, want_groupdq=True)
        assert_equal_outputs(again[1], singles[1], "the batch after a refused one")


def test_refusal_and_recovery():
    """(d): pieces that do not belong together raise; the next valid call on the context returns the bits of a clean one"""
    cal, ramp, plain, _ = chain_inputs(False)
    enc = encoded(ramp, 1000)
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), SLOT, cal) as cb:
        good = cb.calibrate(SLOT, enc, exclude_first=False)
        bad = dict(enc, reference_read=np.zeros((NY, NX), np.uint16), data_encoding_offset=70000)
        with pytest.raises(ValueError, match=r"\d+ samples"):
            cb.calibrate(SLOT, bad, exclude_first=False)
        after = cb.calibrate(SLOT, enc, exclude_first=False)
        assert_equal_outputs(after, good, "the call after a refused one")
        assert_equal_outputs(cb.calibrate(SLOT, plain, exclude_first=False), good, "the plain ramp after a refused one")
        # what validate refuses before anything is copied
        with pytest.raises(ValueError, match="uint16"):
            cb.calibrate(SLOT, dict(enc, data=enc["data"].astype(np.float32)), exclude_first=False)
        with pytest.raises(ValueError, match="amp33"):
            cb.calibrate(SLOT, dict(enc, amp33=None), exclude_first=False)
        with pytest.raises(ValueError, match="reference_read"):
            cb.calibrate(SLOT, dict(enc, reference_read=enc["reference_read"].astype(np.int32)), exclude_first=False)
        # the library's own refusals, on descriptors the Python layer would not have made
        pid, _ = cb.plan_for(enc["read_pattern"], enc["frame_time"], False)
        for field, value, text in (("data_dtype", _native.RIP_F32, "needs u16"), ("amp33", None, "without amp33"),
                                   ("data_encoding_offset", 2**30 + 1, "data_encoding_offset")):
            rd, od = _native.RampDesc(), _native.Outputs()
            _res, keep = cb._host_ramp(rd, od, enc, (NY, NX), False, False, 1, 1, None, None, True)
            setattr(rd, field, value)
            with pytest.raises(ValueError, match=text):
                ctx.calibrate_raw(SLOT, pid, pipeline.STAGE_ALL, rd, od)
            with pytest.raises(ValueError, match=text):
                ctx.check(ctx.lib.rip_calibrate_batch(ctx.h, SLOT, pid, pipeline.STAGE_ALL, 1, C.byref(rd), C.byref(od)))
            del keep
        rd, od = _native.RampDesc(), _native.Outputs()
        rd.location = od.location = DEVICE
        rd.ngrp, rd.data_dtype = 7, _native.RIP_U16
        rd.data = rd.reference_read = to_dev(enc["reference_read"]).data_ptr()   # (never read: the call is refused)
        with pytest.raises(ValueError, match="host ramps only"):
            ctx.calibrate_raw(SLOT, pid, pipeline.STAGE_ALL, rd, od)
        assert_equal_outputs(cb.calibrate(SLOT, enc, exclude_first=False), good, "the call after the refusals")


def test_device_path():
    """(e): device tensors decoded in place by decode_reference_read, then calibrate_device: the bits of the host path"""
    cal, ramp, plain, _ = chain_inputs(False)
    enc = encoded(ramp, 4000)
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), SLOT, cal) as cb:
        host = cb.calibrate(SLOT, enc, exclude_first=False)
        pid, _ = cb.plan_for(enc["read_pattern"], enc["frame_time"], False)
        t = [to_dev(enc[k]) for k in ("data", "amp33", "groupdq", "pixeldq")]
        ref, ref33 = to_dev(enc["reference_read"]), to_dev(enc["reference_amp33"])
        o = device_outputs(7, NY, NX)
        torch.cuda.synchronize()
        assert cb.decode_reference_read(t[0].data_ptr(), 7, NY * NX, ref.data_ptr(), 4000) is None
        assert cb.decode_reference_read(t[1].data_ptr(), 7, NY * 128, ref33.data_ptr(), 4000) is None
        calibrate_resident(cb, SLOT, pid, 7, t, o)
        cb.synchronize()
        assert_same_bits(t[0].cpu().numpy().view(np.uint16), plain["data"], "the decoded cube")
        assert_same_bits(t[1].cpu().numpy().view(np.uint16), plain["amp33"], "the decoded amp33")
        assert_equal_outputs(outputs_to_numpy(o), host, "device path against host path")


def caldir_files(tmp_path, cal):
    """the CALDIR set as files (the recipe of test_calibrateimage_files_end_to_end)"""
    caldir = {}
    names = {"dark": "dark", "read": "read", "gain": "gain", "linearitylegendre": "linearitylegendre", "ipc4d": "ipc4d",
             "flat": "pflat", "biascorr": "biascorr", "mask": "mask", "saturation": "saturation"}
    for key, fname in names.items():
        caldir[key] = str(tmp_path / f"roman_wfi_{fname}_TEST_SCA04.asdf")
        calio.write_asdf(caldir[key], {"roman": cal[key]})
    return caldir


def test_calibrateimage_on_an_encoded_tree(tmp_path):
    """(f): the driver on the encoded tree gives the L2 data, dq and err of the plain tree"""
    cal, ramp, plain, _ = chain_inputs(False)
    enc = encoded(ramp, 4000)
    caldir = caldir_files(tmp_path, cal)

    def tree(r, **more):
        meta = {"exposure": {"frame_time": synth.FRAME_TIME, "read_pattern": [list(g) for g in r["read_pattern"]]},
                "instrument": dict({"detector": "WFI04"}, **more)}
        return {"roman": dict({k: r[k] for k in ("data", "amp33", "reference_read", "reference_amp33") if k in r}, meta=meta)}

    cb = pipeline.Calibrator(ctx=chain_context())
    base = {"OUT": None, "CALDIR": caldir, "EXCLUDE_FIRST": False}
    got = gen_cal_image.calibrateimage(dict(base, IN=tree(enc, data_encoding_offset=4000)), verbose=False, calibrator=cb)
    want = gen_cal_image.calibrateimage(dict(base, IN=tree(plain)), verbose=False, calibrator=cb)
    for k in ("data", "dq", "err"):
        assert_same_bits(got["roman"][k], want["roman"][k], f"L2 {k}")
    assert "data_encoding_offset = 4000" in got["processinfo"]["log"] and "data_encoding_offset" not in want["processinfo"]["log"]
    assert np.count_nonzero(got["roman"]["dq"] & 4) > 50
    with pytest.raises(ValueError, match="data_encoding_offset"):
        gen_cal_image.calibrateimage(dict(base, IN=tree(enc)), verbose=False, calibrator=cb)
    wrong = dict(enc, reference_read=np.zeros((NY, NX), np.uint16))
    with pytest.raises(ValueError, match="samples"):
        gen_cal_image.calibrateimage(dict(base, IN=tree(wrong, data_encoding_offset=70000)), verbose=False, calibrator=cb)
