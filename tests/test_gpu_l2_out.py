"""The L2 tree, built on the device: rip_stage_l2_planes and rip_stage_l2_refpix_strips (csrc/l2out.hip) raw, from host arrays and
from device pointers, against the numpy restatement tests/l2_out_ref.py; then calibrateimage end to end, every key the tree had
before compared with a tree assembled here from Calibrator.calibrate's host results (the pinned path) and numpy, the new
members with the restatement.  Bit patterns are compared; NaNs by position.  Device arrays sit inside a larger buffer of a
sentinel byte, so that a store in front of or behind them shows."""

import functools

import l2_out_ref as lr
import numpy as np
import pytest
import torch  # before libromanhip is loaded: torch brings its own copy of the HIP runtime, and the first one loaded must be the one both use
from chain_support import chain_context
from conftest import gpu_context

import romanimpreprocess_amd
from romanimpreprocess_amd import _native, calio, pipeline, plan as planmod, synth
from romanimpreprocess_amd.devarray import to_device
from romanimpreprocess_amd.from_sim import sim_to_isim
from romanimpreprocess_amd.L1_to_L2 import gen_cal_image, oututils
from romanimpreprocess_amd.utils import maskhandling, sky

pytestmark = pytest.mark.gpu

HOST, DEVICE = _native.RIP_HOST, _native.RIP_DEVICE
SENTINEL, GUARD = 0xA5, 64
# (ny, nx, nb): one active pixel; the vector body; the one-pixel path (nb and nx not multiples of 4); more pixels than one pass of
# the bounded grid (2048 blocks of 256 lanes: 524288 items, against 1492 * 374 = 558008 quads and 2.2 million pixels)
FRAMES = [(9, 9, 4), (16, 128, 4), (48, 256, 4), (33, 131, 1), (40, 260, 2), (1500, 1504, 4)]
# (1e-23 squares to 1e-46, under half the smallest float32 subnormal: it underflows like 1e-30; 1e-20 is the value whose square, 1e-40,
# is a subnormal)
PLANTED = [0.0, -0.0, 1e-30, 1e-23, 1e-20, 3e19, np.nan, np.inf]
PLANTED_F16 = [2049.0, 2051.0, 65504.0, 65519.0, 65520.0, 2.0 ** -12, 3 * 2.0 ** -13, 2.0 ** -13]   # test_host_l2_out_ref.py
PLANES = ("data", "dq", "var_rnoise", "var_poisson", "err")
STRIPS = tuple(f"dq_border_ref_pix_{s}" for s in lr.SIDES)
INPUTS = ("slope", "err_read", "err_poisson", "pixeldq")


@functools.lru_cache(maxsize=None)
def frame(ny, nx, nb):
    """(inputs, restatement float32, restatement float16) of a frame, made once and read-only: random planes with the planted
    values in err_read and err_poisson over the first active pixels (as many as fit), alone and against each other"""
    rng = np.random.default_rng(ny * 10007 + nx * 13 + nb)
    a = {"slope": rng.standard_normal((ny, nx)).astype(np.float32), "err_read": (3 * rng.random((ny, nx))).astype(np.float32),
         "err_poisson": (200 * rng.random((ny, nx))).astype(np.float32), "pixeldq": rng.integers(0, 2 ** 32, (ny, nx), dtype=np.uint32)}
    nxa, na = nx - 2 * nb, (ny - 2 * nb) * (nx - 2 * nb)
    er, ep = PLANTED + PLANTED + PLANTED_F16 + [0.0] * 8, PLANTED + PLANTED[::-1] + [0.0] * 8 + PLANTED_F16
    for k in range(min(na, len(er))):
        a["err_read"][nb + k // nxa, nb + k % nxa], a["err_poisson"][nb + k // nxa, nb + k % nxa] = er[k], ep[k]
    a["slope"].reshape(-1)[:3] = np.array([0x7FC12345, 0x80000000, 0xFF800000], np.uint32).view(np.float32)
    a["slope"][ny // 2, nx // 2], a["slope"][ny - nb - 1, nx - nb - 1] = np.float32(-0.0), np.float32(np.nan)
    for v in a.values():
        v.flags.writeable = False
    want = [lr.l2_planes(a["slope"], a["err_read"], a["err_poisson"], a["pixeldq"], nb, float16=h) for h in (False, True)]
    return a, want[0], want[1]


class DevBytes:
    """`nbytes` of device memory `offset` bytes behind a 16-byte boundary, with GUARD sentinel bytes around them"""

    def __init__(self, nbytes, offset=0, fill=None):
        lead = GUARD + offset
        host = np.full(lead + nbytes + GUARD, SENTINEL, np.uint8)
        if fill is not None:
            host[lead:lead + nbytes] = np.frombuffer(fill, np.uint8)
        self.t = torch.from_numpy(host).cuda()
        assert self.t.data_ptr() % 16 == 0
        self.lead, self.nbytes, self.ptr = lead, nbytes, self.t.data_ptr() + lead

    def read(self, dtype=np.uint8, shape=None):
        """the payload, after checking that the guards still hold the sentinel"""
        host = self.t.cpu().numpy()
        assert np.all(host[:self.lead] == SENTINEL), "bytes in front of the array were written"
        assert np.all(host[self.lead + self.nbytes:] == SENTINEL), "bytes behind the array were written"
        out = host[self.lead:self.lead + self.nbytes].copy().view(dtype)
        return out if shape is None else out.reshape(shape)

    def untouched(self):
        return bool(np.all(self.read() == SENTINEL))


def planes_on_device(ctx, a, want, nb, f16, shifted=(), absent=()):
    """rip_stage_l2_planes on device pointers; `shifted`: names of arrays one ELEMENT behind a 16-byte boundary; `absent`: outputs
    handed over as NULL.  Returns the outputs read back (guards checked) after checking that the inputs are unchanged."""
    ny, nx = a["slope"].shape
    ins = {k: DevBytes(a[k].nbytes, 4 if k in shifted else 0, a[k].tobytes()) for k in INPUTS}
    outs = {k: DevBytes(want[k].nbytes, want[k].itemsize if k in shifted else 0) for k in PLANES + STRIPS if k not in absent}
    ctx.call("rip_stage_l2_planes", *(ins[k].ptr for k in INPUTS), ny, nx, nb, _native.RIP_F16 if f16 else _native.RIP_F32, DEVICE,
             *(outs[k].ptr if k in outs else None for k in PLANES + STRIPS))
    ctx.synchronize()
    for k in INPUTS:
        assert ins[k].read().tobytes() == a[k].tobytes(), f"{k} was written"
    return {k: o.read(want[k].dtype, want[k].shape) for k, o in outs.items()}


def check(got, want, what):
    for k, w in want.items():
        if k in got:
            lr.same_bits(got[k], w, f"{what}: {k}")


# ---------------------------------------------------------------------------------------------- 1. the planes entry
@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("shape", FRAMES, ids=lambda s: "x".join(map(str, s)))
def test_planes_from_host_arrays_and_device_pointers(shape, f16):
    ctx = gpu_context()
    a, w32, w16 = frame(*shape)
    want, nb = (w16 if f16 else w32), shape[2]
    got = oututils.l2_planes(a["slope"], a["err_read"], a["err_poisson"], a["pixeldq"], nb, float16=f16, ctx=ctx)
    assert set(got) == set(want)
    check(got, want, f"host arrays {shape}")
    check(planes_on_device(ctx, a, want, nb, f16), want, f"device pointers {shape}")
    # the wrapper on DevArrays: the same planes, left in HBM
    dev = oututils.l2_planes(*(to_device(a[k]) for k in INPUTS), nb, float16=f16, ctx=ctx)
    check({k: v.numpy() for k, v in dev.items()}, want, f"DevArrays {shape}")


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_planes_with_each_pointer_off_the_16_byte_boundary(f16):
    """every input and output in turn one element behind a 16-byte boundary: the call leaves the vector body for the one-pixel
    path and writes nothing outside its arrays; on the large frame that path runs its grid-stride loop more than once"""
    ctx = gpu_context()
    a, w32, w16 = frame(16, 128, 4)
    want = w16 if f16 else w32
    for name in INPUTS + PLANES + STRIPS:
        check(planes_on_device(ctx, a, want, 4, f16, shifted=(name,)), want, f"{name} shifted")
    check(planes_on_device(ctx, a, want, 4, f16, shifted=INPUTS + PLANES + STRIPS), want, "all shifted")
    a, w32, w16 = frame(1500, 1504, 4)
    check(planes_on_device(ctx, a, w16 if f16 else w32, 4, f16, shifted=("err",)), w16 if f16 else w32, "large frame, err shifted")


def test_planted_values_are_in_the_frames():
    """what the comparisons above rest on: the planted values reached the restatement (and so the kernel's inputs)"""
    _, w32, w16 = frame(16, 128, 4)
    vr, e16 = w32["var_rnoise"].reshape(-1), w16["err"].reshape(-1)
    assert vr[0] == 0 and vr[2] == 0 and vr[3] == 0 and 0 < vr[4] < np.finfo(np.float32).tiny
    assert np.isinf(vr[5]) and np.isnan(vr[6]) and np.isinf(vr[7])
    assert np.isnan(w32["err"].reshape(-1)[9])   # the second round sets the values against each other: err_read = -0, err_poisson = NaN
    assert e16[16:21].tolist() == [2048.0, 2052.0, 65504.0, 65504.0, np.inf] and e16[24:29].tolist() == e16[16:21].tolist()
    assert w16["var_rnoise"].reshape(-1)[21:24].view(np.uint16).tolist() == [1, 2, 0]


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_null_outputs_are_honoured(f16):
    ctx = gpu_context()
    a, w32, w16 = frame(48, 256, 4)
    want = w16 if f16 else w32
    names = PLANES + STRIPS
    for keep in (("err",), ("data",), ("dq", "var_poisson"), ("var_rnoise",), STRIPS[:1], STRIPS[2:], ()):
        got = planes_on_device(ctx, a, want, 4, f16, absent=tuple(k for k in names if k not in keep))
        assert set(got) == set(keep)
        check(got, want, f"only {keep}")
    # host arrays: the raw entry with one output
    err = np.full(want["err"].shape, 7, want["err"].dtype)
    ctx.call("rip_stage_l2_planes", *(a[k] for k in INPUTS), 48, 256, 4, _native.RIP_F16 if f16 else _native.RIP_F32, HOST,
             None, None, None, None, err, None, None, None, None)
    lr.same_bits(err, want["err"], "host arrays, err alone")


def test_planes_refusals_leave_the_outputs_alone():
    ctx = gpu_context()
    ny, nx, nb = 16, 128, 4
    a, want, _ = frame(ny, nx, nb)
    ins = {k: DevBytes(a[k].nbytes + 16, 0, a[k].tobytes() + bytes(16)) for k in INPUTS}
    F32, F16 = _native.RIP_F32, _native.RIP_F16

    def attempt(what, part, over=None, dims=(ny, nx, nb), dtype=F32, location=DEVICE, out_over=None):
        outs = {k: DevBytes(want[k].nbytes + 16) for k in PLANES + STRIPS}
        ptrs = {k: ins[k].ptr for k in INPUTS}
        ptrs.update({k: outs[k].ptr for k in outs})
        ptrs.update(over or {})
        ptrs.update(out_over or {})
        args = (*(ptrs[k] for k in INPUTS), *dims, dtype, location, *(ptrs[k] for k in PLANES + STRIPS))
        with pytest.raises(ValueError) as err:
            ctx.call("rip_stage_l2_planes", *args)
        assert "l2_planes" in str(err.value) and part in str(err.value), f"{what}: {err.value}"
        assert ctx.lib.rip_stage_l2_planes(*_native.marshal("rip_stage_l2_planes", (ctx.h, *args))) == _native.RIP_EINVAL, what
        ctx.synchronize()
        for k, o in outs.items():
            assert o.untouched(), f"{what}: {k} was written"

    for k in INPUTS:
        attempt(f"NULL {k}", "NULL", over={k: None})
    attempt("ny = 0", "frame", dims=(0, nx, 0))
    attempt("nx = 0", "frame", dims=(ny, 0, 0))
    attempt("nx < 0", "frame", dims=(ny, -4, 0))
    attempt("nb < 0", "nb", dims=(ny, nx, -1))
    attempt("2 nb = ny", "active region", dims=(ny, nx, 8))
    attempt("2 nb > ny", "active region", dims=(ny, nx, 9))
    attempt("2 nb = nx", "active region", dims=(200, 16, 8))
    attempt("dtype f64", "var_dtype", dtype=_native.RIP_F64)
    attempt("dtype u16", "var_dtype", dtype=_native.RIP_U16)
    attempt("dtype 9", "var_dtype", dtype=9)
    attempt("location 2", "location", location=2)
    attempt("location -1", "location", location=-1)
    for k in INPUTS:
        attempt(f"{k} off its element", "aligned", over={k: ins[k].ptr + 2})
    probe = {k: DevBytes(want[k].nbytes + 16) for k in PLANES + STRIPS}
    for k in PLANES + STRIPS:
        attempt(f"{k} off its element", "aligned", out_over={k: probe[k].ptr + 2})
    for k in ("var_rnoise", "var_poisson", "err"):
        attempt(f"{k} off its float16 element", "aligned", dtype=F16, out_over={k: probe[k].ptr + 1})
    assert all(o.untouched() for o in probe.values())
    # an output that meets an input: its first byte on the input's last one, and inside it
    last = a["slope"].nbytes - 1
    attempt("data on the end of slope", "overlaps", out_over={"data": ins["slope"].ptr + last - 3})
    attempt("err inside err_read", "overlaps", out_over={"err": ins["err_read"].ptr + 64})
    attempt("a strip inside pixeldq", "overlaps", out_over={"dq_border_ref_pix_top": ins["pixeldq"].ptr})
    attempt("dq in front of err_poisson, reaching into it", "overlaps", out_over={"dq": ins["err_poisson"].ptr - 4})
    for k in INPUTS:
        assert ins[k].read().tobytes() == a[k].tobytes() + bytes(16), f"{k} was written"
    # host arrays: refused before any copy
    outs = {k: np.full(want[k].shape, 7, want[k].dtype) for k in PLANES + STRIPS}
    for over, dims, dtype in (({"slope": None}, (ny, nx, nb), F32), ({}, (ny, nx, 8), F32), ({}, (ny, nx, nb), _native.RIP_F64)):
        arrays = dict(a, **over)
        with pytest.raises(ValueError):
            ctx.call("rip_stage_l2_planes", *(arrays[k] for k in INPUTS), *dims, dtype, HOST, *(outs[k] for k in PLANES + STRIPS))
    both = np.full(ny * nx + 8, 7, np.float32)
    with pytest.raises(ValueError, match="overlaps"):
        ctx.call("rip_stage_l2_planes", both[:ny * nx], a["err_read"], a["err_poisson"], a["pixeldq"], ny, nx, nb, F32, HOST,
                 both[8:], None, None, None, None, None, None, None, None)
    assert np.all(both == 7) and all(np.all(o == 7) for o in outs.values())


# ---------------------------------------------------------------------------------------------- 2. the strips entry
def cube_of(dtype, ngrp, ny, nx):
    rng = np.random.default_rng(ngrp * 1000 + ny + nx)
    if dtype == np.uint16:
        cube = rng.integers(1, 65535, (ngrp, ny, nx), dtype=np.uint16)
        cube[:, 0, :3], cube[:, -1, -3:], cube[:, 1, 0], cube[:, -2, -1] = [0, 65535, 0], [65535, 0, 65535], 65535, 0
    else:
        cube = (60000 * rng.random((ngrp, ny, nx))).astype(np.float32)
        cube[:, 0, :3] = np.array([0x7FC12345, 0x80000000, 0x00000001], np.uint32).view(np.float32)
        cube[:, -1, -1] = np.float32(-np.inf)
    return cube


@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=["u16", "f32"])
@pytest.mark.parametrize("ngrp", [1, 6])
def test_refpix_strips(dtype, ngrp):
    ctx = gpu_context()
    for ny, nx, nb in ((16, 128, 4), (33, 131, 1), (40, 260, 2), (9, 9, 4)):
        cube = cube_of(dtype, ngrp, ny, nx)
        want = lr.refpix_strips(cube, nb)
        names = tuple(want)
        if dtype == np.uint16:   # the conversion is exact: every edge sample is the integer it was
            assert all(np.array_equal(w.astype(np.uint16), e) for w, e in zip(want.values(), lr.edges(cube, nb)))
        check(oututils.refpix_strips(cube, nb, ctx=ctx), want, f"host arrays {ngrp} x {ny} x {nx}")
        check({k: v.numpy() for k, v in oututils.refpix_strips(to_device(cube), nb, ctx=ctx).items()}, want, "a DevArray")
        for shifted, absent in (((), ()), (("cube",), ()), (names[:2], names[2:]), (names, ("cube",) + names[:3])):
            src = DevBytes(cube.nbytes, cube.itemsize if "cube" in shifted else 0, cube.tobytes())
            outs = {k: DevBytes(want[k].nbytes, 4 if k in shifted else 0) for k in names if k not in absent}
            ctx.call("rip_stage_l2_refpix_strips", src.ptr, _native.dtype_code(cube), ngrp, ny, nx, nb, DEVICE,
                     *(outs[k].ptr if k in outs else None for k in names))
            ctx.synchronize()
            assert src.read().tobytes() == cube.tobytes()
            check({k: o.read(np.float32, want[k].shape) for k, o in outs.items()}, want, f"device pointers, shifted {shifted}")


@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=["u16", "f32"])
@pytest.mark.parametrize("nb", [0, 1])
def test_refpix_strips_host_and_device_with_null_outputs(dtype, nb):
    """the raw entry at RIP_HOST and at RIP_DEVICE on a 2 x 5 x 12 cube, with every strip, with two and with one: the same bits
    from both, and a strip not asked for is left alone.  nb = 0: the strips hold no element, and nothing is written"""
    ctx = gpu_context()
    ngrp, ny, nx = 2, 5, 12
    cube = cube_of(dtype, ngrp, ny, nx)
    want = lr.refpix_strips(cube, nb)
    names = tuple(want)
    src = DevBytes(cube.nbytes, 0, cube.tobytes())
    for keep in (names, names[:2], names[3:]):
        host = {k: np.full(want[k].shape, 7, np.float32) for k in names}
        ctx.call("rip_stage_l2_refpix_strips", cube, _native.dtype_code(cube), ngrp, ny, nx, nb, HOST,
                 *(host[k] if k in keep else None for k in names))
        outs = {k: DevBytes(want[k].nbytes) for k in names}
        ctx.call("rip_stage_l2_refpix_strips", src.ptr, _native.dtype_code(cube), ngrp, ny, nx, nb, DEVICE,
                 *(outs[k].ptr if k in keep else None for k in names))
        ctx.synchronize()
        for k in names:
            if k in keep:
                lr.same_bits(host[k], want[k], f"host arrays, {k} of {keep}")
                lr.same_bits(outs[k].read(np.float32, want[k].shape), host[k], f"device pointers against host arrays, {k} of {keep}")
            else:
                assert np.all(host[k] == 7) and outs[k].untouched(), f"{k} was not asked for"
    assert src.read().tobytes() == cube.tobytes()


def test_refpix_strips_refusals_leave_the_outputs_alone():
    ctx = gpu_context()
    ngrp, ny, nx, nb = 2, 16, 24, 4
    cube = cube_of(np.uint16, ngrp, ny, nx)
    want = lr.refpix_strips(cube, nb)
    src = DevBytes(cube.nbytes + 16, 0, cube.tobytes() + bytes(16))
    U16 = _native.RIP_U16
    for what, part, c, dtype, dims, location, over in (
            ("NULL cube", "NULL", None, U16, (ngrp, ny, nx, nb), DEVICE, {}), ("ngrp = 0", "cube", src.ptr, U16, (0, ny, nx, nb), DEVICE, {}),
            ("ny = 0", "cube", src.ptr, U16, (ngrp, 0, nx, 0), DEVICE, {}), ("nx = -1", "cube", src.ptr, U16, (ngrp, ny, -1, 0), DEVICE, {}),
            ("nb < 0", "nb", src.ptr, U16, (ngrp, ny, nx, -1), DEVICE, {}), ("nb > ny", "nb", src.ptr, U16, (ngrp, ny, nx, 17), DEVICE, {}),
            ("dtype f64", "cube_dtype", src.ptr, _native.RIP_F64, (ngrp, ny, nx, nb), DEVICE, {}),
            ("dtype f16", "cube_dtype", src.ptr, _native.RIP_F16, (ngrp, ny, nx, nb), DEVICE, {}),
            ("location 3", "location", src.ptr, U16, (ngrp, ny, nx, nb), 3, {}),
            ("cube off its element", "aligned", src.ptr + 1, U16, (ngrp, ny, nx, nb), DEVICE, {}),
            ("f32 cube off its element", "aligned", src.ptr + 2, _native.RIP_F32, (ngrp, ny, nx // 2, nb), DEVICE, {}),
            ("left off its element", "aligned", src.ptr, U16, (ngrp, ny, nx, nb), DEVICE, {"border_ref_pix_left": 2}),
            ("top inside the cube", "overlaps", src.ptr, U16, (ngrp, ny, nx, nb), DEVICE, {"border_ref_pix_top": src.ptr + 8}),
            ("bottom on the cube's last byte", "overlaps", src.ptr, U16, (ngrp, ny, nx, nb), DEVICE,
             {"border_ref_pix_bottom": src.ptr + cube.nbytes - 2})):
        outs = {k: DevBytes(want[k].nbytes + 16) for k in want}
        ptrs = {k: (over[k] if over.get(k, 0) > 16 else outs[k].ptr + over.get(k, 0)) for k in want}
        with pytest.raises(ValueError) as err:
            ctx.call("rip_stage_l2_refpix_strips", c, dtype, *dims, location, *ptrs.values())
        assert "l2_refpix_strips" in str(err.value) and part in str(err.value), f"{what}: {err.value}"
        ctx.synchronize()
        assert all(o.untouched() for o in outs.values()), what
    assert src.read().tobytes() == cube.tobytes() + bytes(16)
    with pytest.raises(TypeError):
        oututils.refpix_strips(cube.astype(np.float64), nb, ctx=ctx)


# ---------------------------------------------------------------------------------------------- 3. calibrateimage
NB = 4
RP = synth.READ_PATTERN_6
JUMP = {"SthreshA": 5.0, "IthreshB": 800.0}


@pytest.fixture(scope="module")
def exposure(tmp_path_factory):
    """the 48 x 256 frame of six groups of test_gpu_fits_out.py's fixture as files, and its EXTRACT_REF form as a tree"""
    tmp = tmp_path_factory.mktemp("l2out")
    cal = synth.make_caldir(48, 256, read_pattern=RP, p_order=3, seed=31, bias_amplitude=1.0)
    ramp = synth.make_ramp(cal, read_pattern=RP, seed=32, cr_frac=0.02)
    caldir = {}
    for key, fname in {"dark": "dark", "read": "read", "gain": "gain", "linearitylegendre": "linearitylegendre", "ipc4d": "ipc4d",
                       "flat": "pflat", "biascorr": "biascorr", "mask": "mask", "saturation": "saturation"}.items():
        caldir[key] = str(tmp / f"roman_wfi_{fname}_TEST_SCA04.asdf")
        calio.write_asdf(caldir[key], {"roman": cal[key]})
    l1meta = {"exposure": {"frame_time": synth.FRAME_TIME, "read_pattern": [list(g) for g in RP]}, "instrument": {"detector": "WFI04"}}
    l1 = {"data": np.ascontiguousarray(ramp["data"]), "amp33": np.ascontiguousarray(ramp["amp33"]), "meta": l1meta}
    assert l1["data"].dtype == np.uint16 and l1["data"].shape == (6, 48, 256)
    calio.write_asdf(str(tmp / "l1.asdf"), {"roman": l1})
    # an exposure without the reference output goes with a read-noise file without it (the library refuses the mixture)
    calio.write_asdf(str(tmp / "l1_noamp33.asdf"), {"roman": {k: v for k, v in l1.items() if k != "amp33"}})
    caldir_noamp33 = dict(caldir, read=str(tmp / "roman_wfi_read_NOAMP33_SCA04.asdf"))
    calio.write_asdf(caldir_noamp33["read"], {"roman": {k: v for k, v in cal["read"].items() if k != "amp33"}})
    enc = sim_to_isim.extract_ref({"data": l1["data"].copy(), "amp33": l1["amp33"].copy(),
                                   "meta": {"exposure": dict(l1meta["exposure"]), "instrument": dict(l1meta["instrument"])}},
                                  {"EXTRACT_REF": {"data_encoding_offset": 4000}})
    assert enc["data"].shape == (5, 48, 256) and enc["meta"]["instrument"]["data_encoding_offset"] == 4000
    base = {"IN": str(tmp / "l1.asdf"), "OUT": str(tmp / "l2.asdf"), "CALDIR": caldir, "SLICEOUT": True, "JUMP_DETECT_PARS": JUMP}
    return {"tmp": tmp, "cal": cal, "caldir": caldir, "caldir_noamp33": caldir_noamp33, "l1": l1, "enc": enc, "base": base, "cb": pipeline.Calibrator(ctx=chain_context()),
            "pinned": {}}


def pinned_results(ex, which):
    """Calibrator.calibrate's host results for the exposure (the pinned path), once per form of it"""
    if which not in ex["pinned"]:
        cb, src = ex["cb"], (ex["enc"] if which == "enc" else ex["l1"])
        rp = [list(map(int, g)) for g in src["meta"]["exposure"]["read_pattern"]]
        ramp = {"data": src["data"], "amp33": None if which == "noamp33" else src["amp33"], "groupdq": None,
                "pixeldq": np.asarray(ex["cal"]["mask"]["dq"], dtype=np.uint32), "read_pattern": rp, "frame_time": synth.FRAME_TIME}
        if which == "enc":
            ramp.update(reference_read=src["reference_read"], reference_amp33=src["reference_amp33"], data_encoding_offset=4000)
        slot = gen_cal_image._caldir_slot(cb, ex["caldir_noamp33" if which == "noamp33" else "caldir"])
        res = cb.calibrate(slot, ramp, exclude_first=which != "enc", jump_pars=JUMP, flag_saturation=True, saturation_read_pattern=True,
                           saturation_backup=1)
        ex["pinned"][which] = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in res.items()}
    return ex["pinned"][which]


def expected_tree(ex, which, config):
    """The L2 tree: what it held before this stage existed -- the numpy finishing steps on the pinned results and the host-array
    mirrors, restated from the driver as it was -- and the new members from the restatement"""
    ctx = ex["cb"].ctx
    res = pinned_results(ex, which)
    src = ex["enc"] if which == "enc" else ex["l1"]
    slope, pdq, rdq = res["slope"], res["pixeldq"], res["groupdq"]
    act = (slice(NB, -NB), slice(NB, -NB))
    m = maskhandling.PixelMask1.build(pdq, ctx=ctx)
    medsky = float(sky.smooth_mode(sky.binkxk(slope, 4, mask=m, ctx=ctx), ctx=ctx)[0])
    data_act = np.ascontiguousarray(slope[act])
    data_withsky = data_act.copy()
    if "SKYORDER" in config:
        skyorder = int(config["SKYORDER"])
        skycoefs = np.asarray(sky.medfit(data_act, order=skyorder, subtract=True, ctx=ctx)[0])
    else:
        skycoefs, skyorder = np.array([]).astype(np.float32), -1
    var_r, var_p = res["err_read"][act] ** 2, res["err_poisson"][act] ** 2
    err, var_flat = np.sqrt(var_r + var_p), np.zeros_like(var_r)
    if config.get("L2_FLOAT16"):   # typefix.py:56
        var_r, var_p, err, var_flat = (a.astype(np.float16) for a in (var_r, var_p, err, var_flat))
    meta = {k: v for k, v in src["meta"].items()}
    roman = {"meta": meta, "data": data_act, "dq": pdq[act].copy(), "var_poisson": var_p, "var_rnoise": var_r, "var_flat": var_flat,
             "err": err, "data_withsky": data_withsky}
    if which != "noamp33":
        roman["amp33"] = src["amp33"]
    more, more_meta = lr.new_members(src["data"], pdq, NB, data_act.shape, romanimpreprocess_amd.__version__)
    roman.update(more)
    roman["meta"] = dict(meta, **more_meta)
    rp = [list(map(int, g)) for g in src["meta"]["exposure"]["read_pattern"]]
    pmeta = planmod.exposure_meta(rp, synth.FRAME_TIME)
    pmeta["nborder"] = NB
    uopt = planmod.DEFAULT_RAMP_OPT_PARS
    gain = np.asarray(ex["cal"]["gain"]["data"])
    medgain = float(np.median(gain))
    log = "Initialized data\n"
    if which == "enc":
        log += "Reference read subtracted in the file (data_encoding_offset = 4000): decoded on the device\n"
    log += "Saturation check on the device\n"
    log += f"\n\nRamp fit optimized for u = {planmod.ramp_opt_u(uopt):11.5E} s**-1\n" + f"weights = {res['K']}\n"
    log += "Reference pixels, bias, linearity, IPC, ramp fit, dark current, flat: complete (GPU)\n" + f"median gain = {medgain:8.5f} e/DN\n"
    processinfo = {"medsky": medsky, "medgain": medgain, "skyorder": skyorder, "skycoefs": skycoefs, "ramp_opt_pars": dict(uopt),
                   "weights": res["K"], "log": log, "config": {k: v for k, v in config.items() if not (k == "IN" and isinstance(v, dict))},
                   "exclude_first": bool(config.get("EXCLUDE_FIRST", True)),
                   "meta": {k: ([list(map(int, g)) for g in v] if k == "read_pattern" else v) for k, v in pmeta.items()}}
    if config.get("SLICEOUT"):
        processinfo["endslice"] = sky.endslice(rdq, NB, ctx=ctx)
    return {"roman": roman, "processinfo": processinfo}


def assert_trees_equal(got, want, where="tree"):
    """keys, types of the leaves that are arrays, and every value; a list may stand for a tuple and an array read from a file for
    the list it was written from"""
    if hasattr(want, "items"):
        assert hasattr(got, "items"), f"{where}: {type(got).__name__} where a mapping is expected"
        assert sorted(got.keys()) == sorted(want.keys()), f"{where}: keys {sorted(set(got.keys()) ^ set(want.keys()))} differ"
        for k in want:
            assert_trees_equal(got[k], want[k], f"{where}.{k}")
    elif isinstance(want, np.ndarray) and want.ndim:
        lr.same_bits(np.asarray(got), want, where)
    elif isinstance(want, (list, tuple)):
        got = got.tolist() if isinstance(got, np.ndarray) else got
        assert len(got) == len(want), f"{where}: {len(got)} entries against {len(want)}"
        for i, (g, w) in enumerate(zip(got, want)):
            assert_trees_equal(g, w, f"{where}[{i}]")
    elif isinstance(want, (float, np.floating)):
        assert float(got) == float(want) or (np.isnan(got) and np.isnan(want)), f"{where}: {got!r} against {want!r}"
    else:
        got = got.item() if isinstance(got, np.generic) else got
        want = want.item() if isinstance(want, np.generic) else want
        assert got == want and type(got) is type(want), f"{where}: {got!r} against {want!r}"


VARIANTS = {   # name -> (form of the exposure, what the configuration adds)
    "plain": ("l1", {}), "skyorder": ("l1", {"SKYORDER": 2}), "no_amp33": ("noamp33", {}), "float16": ("l1", {"L2_FLOAT16": True}),
    "float16_skyorder_no_sliceout": ("l1", {"L2_FLOAT16": True, "SKYORDER": 1, "SLICEOUT": False}),
    "extract_ref": ("enc", {"EXCLUDE_FIRST": False}),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_calibrateimage_tree(exposure, name):
    ex = exposure
    which, more = VARIANTS[name]
    config = dict(ex["base"], OUT=None, **more)
    if which == "noamp33":
        config["IN"], config["CALDIR"] = str(ex["tmp"] / "l1_noamp33.asdf"), ex["caldir_noamp33"]
    if which == "enc":
        config["IN"] = {"roman": ex["enc"]}
    got = gen_cal_image.calibrateimage(config, verbose=False, calibrator=ex["cb"])
    want = expected_tree(ex, which, config)
    assert_trees_equal(got, want)
    r = got["roman"]
    f = np.float16 if more.get("L2_FLOAT16") else np.float32
    assert [r[k].dtype for k in ("err", "var_poisson", "var_rnoise", "var_flat")] == [f] * 4 and r["data"].dtype == np.float32
    assert r["border_ref_pix_left"].shape == (len(ex["enc" if which == "enc" else "l1"]["data"]), 48, 4)
    assert r["dq_border_ref_pix_top"].dtype == np.uint32 and r["dq_border_ref_pix_top"].shape == (4, 256)
    assert r["chisq"].dtype == np.float16 and r["chisq"].shape == r["data"].shape == (40, 248) and not r["dumo"].any()
    assert r["meta"]["calibration_software_name"] == "gen_cal_image / HLWAS PIT" and r["meta"]["dummyfields"] == ["roman.chisq", "roman.dumo"]
    assert r["meta"]["calibration_software_version"] == "romanimpreprocess_amd " + romanimpreprocess_amd.__version__
    assert np.count_nonzero(r["dq"]) > 50 and np.count_nonzero(r["err"].astype(np.float32) > 0) > 5000
    if which == "enc":
        # the strips are the samples as stored, which the decoding changes (offset 4000 less the reference read)
        left = np.asarray(r["border_ref_pix_left"])
        assert np.array_equal(left, ex["enc"]["data"][:, :, :4].astype(np.float32))
        assert not np.array_equal(left, ex["l1"]["data"][1:, :, :4].astype(np.float32))
    # the caller's tree and configuration are as they were
    assert "calibration_software_name" not in ex["enc"]["meta"] and "OUT" in config and config["OUT"] is None


@pytest.mark.parametrize("more", [{}, {"SKYORDER": 2, "L2_FLOAT16": True, "FITSOUT": True}], ids=["plain", "skyorder_float16_fitsout"])
def test_calibrateimage_file_holds_the_tree_of_out_none(exposure, more):
    ex = exposure
    config = dict(ex["base"], OUT=str(ex["tmp"] / f"l2_{len(more)}.asdf"), **more)
    assert gen_cal_image.calibrateimage(config, verbose=False, calibrator=ex["cb"]) is None
    file_tree = calio.read_asdf(config["OUT"])
    want = expected_tree(ex, "l1", config)
    assert_trees_equal({k: file_tree[k] for k in ("roman", "processinfo")}, want, "file")
    memory = gen_cal_image.calibrateimage(dict(config, OUT=None), verbose=False, calibrator=ex["cb"])
    memory["processinfo"]["config"]["OUT"] = config["OUT"]   # the one entry in which the two calls differ
    assert_trees_equal({k: file_tree[k] for k in ("roman", "processinfo")}, memory, "file against OUT = None")
    assert (ex["tmp"] / f"l2_{len(more)}_asdf_to.fits").exists() == bool(more.get("FITSOUT"))
