"""FITS output on the device: rip_stage_fits_encode (csrc/fitsout.hip) raw, calio.write_fits, and the callers that write FITS
files (CombinedMask.convert_file, calibrateimage and generate_all_noise with FITSOUT, the dumps of the three calibration-file drop-ins), against the
numpy restatement tests/fits_out_ref.py.  Everything is compared as BYTES: the encoder moves bits, and a float comparison would
let a NaN payload or a zero's sign pass.  Device destinations sit inside a larger buffer of a sentinel byte, so that a store in
front of or behind the samples shows."""

import contextlib
import io
import struct

import calfiles_cases as cc
import darkstack_cases as dc
import fits_out_ref as fr
import gainfile_cases as gc
import numpy as np
import post_edge_refs as pe
import pytest
import torch  # before libromanhip is loaded: torch brings its own copy of the HIP runtime, and the first one loaded must be the one both use
import yaml
from chain_support import chain_context
from conftest import gpu_context

from oracle import post as opost
from romanimpreprocess_amd import _native, calfiles, calio, pipeline, synth
from romanimpreprocess_amd.calfiles import make_dark_file, make_gain_file, postprocess_calfiles
from romanimpreprocess_amd.devarray import to_device
from romanimpreprocess_amd.dqflags import pixel
from romanimpreprocess_amd.L1_to_L2 import gen_cal_image, gen_noise_image
from romanimpreprocess_amd.utils import maskhandling

pytestmark = pytest.mark.gpu

HOST, DEVICE = _native.RIP_HOST, _native.RIP_DEVICE
SENTINEL = 0xA5
GUARD = 64   # bytes of sentinel on either side of a destination
SIZES = (1, 3, 4, 5, 15, 16, 17, 1023, 4099)
# (bitpix, flip_sign) -> numpy dtype: every allowed pair
KINDS = {(8, 0): np.uint8, (8, 1): np.int8, (16, 0): np.int16, (16, 1): np.uint16, (32, 0): np.int32, (32, 1): np.uint32,
         (-32, 0): np.float32, (-64, 0): np.float64}
SPECIAL_BITS = {
    np.float32: [0x7FC00000, 0x7FC12345, 0xFFC54321, 0x7F800001, 0xFFBFFFFF, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000,
                 0x00000001, 0x807FFFFF, 0x00800000],
    np.float64: [0x7FF8000000000000, 0x7FF8123456789ABC, 0xFFF0000000000001, 0x0000000000000000, 0x8000000000000000,
                 0x7FF0000000000000, 0xFFF0000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x0010000000000000],
}
SPECIAL_VALUES = {np.uint16: [0, 32767, 32768, 65535], np.int16: [0, 32767, -32768, -1], np.uint32: [0, 2**31 - 1, 2**31, 2**32 - 1],
                  np.int32: [0, 2**31 - 1, -2**31, -1], np.int8: [-128, -1, 0, 127], np.uint8: [0, 127, 128, 255]}


def samples(dtype, n, seed=0):
    """n samples of `dtype` whose bytes are all distinct within a sample (byte j = base + 37 j mod 256), the special values of
    the type in front and, where there is room, again at the end"""
    dtype = np.dtype(dtype)
    w = dtype.itemsize
    rng = np.random.default_rng(1000 * w + seed)
    raw = (rng.integers(0, 256, (n, 1)) + 37 * np.arange(w)[None, :]) % 256
    out = np.ascontiguousarray(raw.astype(np.uint8)).view(dtype).reshape(n).copy()
    if dtype.type in SPECIAL_BITS:
        special = np.array(SPECIAL_BITS[dtype.type], dtype=f"u{w}").view(dtype)
    else:
        special = np.array(SPECIAL_VALUES[dtype.type], dtype=dtype)
    k = min(n, special.size)
    out[:k] = special[:k]
    if n >= 4 * special.size:
        out[-special.size:] = special
    return out


def expected(arr):
    """the restatement's bytes; for floats also through the integer view, which cannot touch a NaN"""
    want = fr.stored(arr)
    if arr.dtype.kind == "f":
        u = f"u{arr.dtype.itemsize}"
        assert want == arr.view(u).astype(">" + u).tobytes()
    return want


class DevBytes:
    """`nbytes` of device memory at `offset` bytes behind a 16-byte boundary, with GUARD sentinel bytes around them"""

    def __init__(self, nbytes, offset, fill=None):
        lead = GUARD + offset
        assert GUARD % 16 == 0
        host = np.full(lead + nbytes + GUARD, SENTINEL, np.uint8)
        if fill is not None:
            host[lead:lead + nbytes] = np.frombuffer(fill, np.uint8)
        self.t = torch.from_numpy(host).cuda()
        assert self.t.data_ptr() % 16 == 0
        self.lead, self.nbytes, self.ptr = lead, nbytes, self.t.data_ptr() + lead

    def read(self):
        """the payload, after checking that the guards still hold the sentinel"""
        host = self.t.cpu().numpy()
        assert np.all(host[:self.lead] == SENTINEL), "bytes in front of the destination were written"
        assert np.all(host[self.lead + self.nbytes:] == SENTINEL), "bytes behind the destination were written"
        return host[self.lead:self.lead + self.nbytes].tobytes()


def encode(ctx, src, kind, n, sloc, dst, dloc, mask=None, sense=0, fill=0.0):
    ctx.call("rip_stage_fits_encode", src, kind[0], kind[1], n, sloc, mask, sense, fill, dst, dloc)
    ctx.synchronize()


# ---------------------------------------------------------------------------------------------- 1. the entry, raw
@pytest.mark.parametrize("kind", list(KINDS), ids=lambda k: f"bitpix{k[0]}_flip{k[1]}")
def test_encode_host_arrays(kind):
    ctx = gpu_context()
    for n in SIZES:
        arr = samples(KINDS[kind], n)
        w = arr.itemsize
        out = np.full(2 * GUARD + n * w, SENTINEL, np.uint8)
        encode(ctx, arr, kind, n, HOST, out[GUARD:GUARD + n * w], HOST)
        assert out[GUARD:GUARD + n * w].tobytes() == expected(arr), f"{kind} n={n}"
        assert np.all(out[:GUARD] == SENTINEL) and np.all(out[GUARD + n * w:] == SENTINEL)
        # in place
        work = arr.copy()
        encode(ctx, work, kind, n, HOST, work, HOST)
        assert work.tobytes() == expected(arr), f"{kind} n={n} in place"
        # a host source with a device destination, and back
        d = DevBytes(n * w, w)
        encode(ctx, arr, kind, n, HOST, d.ptr, DEVICE)
        assert d.read() == expected(arr), f"{kind} n={n} host to device"
        s = DevBytes(n * w, 0, arr.tobytes())
        back = np.full(n * w, SENTINEL, np.uint8)
        encode(ctx, s.ptr, kind, n, DEVICE, back, HOST)
        assert back.tobytes() == expected(arr), f"{kind} n={n} device to host"


@pytest.mark.parametrize("kind", list(KINDS), ids=lambda k: f"bitpix{k[0]}_flip{k[1]}")
def test_encode_device_pointers_at_every_alignment(kind):
    """src and dst each 0 to 3 samples behind a 16-byte boundary: equal offsets take the vector body with its head and tail,
    different ones the one-sample path"""
    ctx = gpu_context()
    for n in SIZES:
        arr = samples(KINDS[kind], n, seed=n)
        w, want = arr.itemsize, expected(arr)
        for so in range(4):
            src = DevBytes(n * w, so * w, arr.tobytes())
            for do in range(4):
                dst = DevBytes(n * w, do * w)
                encode(ctx, src.ptr, kind, n, DEVICE, dst.ptr, DEVICE)
                assert dst.read() == want, f"{kind} n={n} src+{so} dst+{do}"
            assert src.read() == arr.tobytes(), "the source was written"
            encode(ctx, src.ptr, kind, n, DEVICE, src.ptr, DEVICE)   # in place
            assert src.read() == want, f"{kind} n={n} src+{so} in place"


# ---------------------------------------------------------------------------------------------- 2. the masked form
def masks_for(n, head):
    """name -> mask bytes: sample 0, the last one, the samples on either side of the two ends of the vector body (the body is
    [head, head + 4 * ((n - head) // 4)) where src and dst share their alignment), all, none, and set bytes other than 1"""
    tail0 = head + (n - head) // 4 * 4 if n >= head else n
    out = {"none": np.zeros(n, np.uint8), "all": np.ones(n, np.uint8)}
    for name, at in (("first", [0]), ("last", [n - 1]), ("body_start", [head - 1, head]), ("body_end", [tail0 - 1, tail0])):
        m = np.zeros(n, np.uint8)
        for i in at:
            if 0 <= i < n:
                m[i] = 1
        out[name] = m
    rng = np.random.default_rng(n)
    out["other_bytes"] = rng.choice(np.array([0, 0, 2, 0x80, 255], np.uint8), n)
    return out


def masked_expected(arr, mask, sense, fill):
    bits = np.where((mask != 0) == bool(sense), np.frombuffer(struct.pack("<f", fill), "<u4")[0], arr.view(np.uint32))
    want = bits.astype(">u4").tobytes()
    assert want == fr.stored(np.where((mask != 0) == bool(sense), np.float32(fill), arr))
    return want


@pytest.mark.parametrize("fill", [-1000.0, -0.0])
def test_masked_encode(fill):
    ctx = gpu_context()
    kind = (-32, 0)
    for n in (1, 5, 17, 4099):
        arr = samples(np.float32, n, seed=7)
        for so, do in ((0, 0), (1, 1), (3, 3), (2, 0)):
            head = min(n, (4 - so) % 4) if so == do else n
            src = DevBytes(n * 4, so * 4, arr.tobytes())
            for name, mask in masks_for(n, head).items():
                for mo in range(4):   # the mask base 0 to 3 bytes behind a 4-byte boundary
                    m = DevBytes(n, mo, mask.tobytes())
                    for sense in (1, 0):
                        dst = DevBytes(n * 4, do * 4)
                        encode(ctx, src.ptr, kind, n, DEVICE, dst.ptr, DEVICE, mask=m.ptr, sense=sense, fill=fill)
                        assert dst.read() == masked_expected(arr, mask, sense, fill), f"n={n} src+{so} dst+{do} mask+{mo} {name} sense {sense}"
                    assert m.read() == mask.tobytes()
        # host arrays (bool masks are bytes of 0 / 1), and in place on the device
        for name, mask in masks_for(n, 0).items():
            out = np.full(n * 4, SENTINEL, np.uint8)
            encode(ctx, arr, kind, n, HOST, out, HOST, mask=mask, sense=1, fill=fill)
            assert out.tobytes() == masked_expected(arr, mask, 1, fill), f"host n={n} {name}"
            out = np.full(n * 4, SENTINEL, np.uint8)
            encode(ctx, arr, kind, n, HOST, out, HOST, mask=mask != 0, sense=0, fill=fill)
            assert out.tobytes() == masked_expected(arr, mask, 0, fill), f"host n={n} {name} bool, sense 0"
            work, m = DevBytes(n * 4, 4, arr.tobytes()), DevBytes(n, 1, mask.tobytes())
            encode(ctx, work.ptr, kind, n, DEVICE, work.ptr, DEVICE, mask=m.ptr, sense=1, fill=fill)
            assert work.read() == masked_expected(arr, mask, 1, fill), f"in place n={n} {name}"


@pytest.mark.parametrize("n", [17, 4099])
def test_masked_encode_between_host_and_device(n):
    """src and mask in one place, dst in the other, against both in the same place: the same bytes, with a mask and without"""
    ctx = gpu_context()
    kind = (-32, 0)
    arr = samples(np.float32, n, seed=9)
    mask = masks_for(n, 0)["other_bytes"]
    for m, want in ((mask, masked_expected(arr, mask, 1, -1000.0)), (None, expected(arr))):
        got = {}
        for sloc, dloc in ((HOST, HOST), (DEVICE, DEVICE), (HOST, DEVICE), (DEVICE, HOST)):
            src, dm = DevBytes(n * 4, 4, arr.tobytes()), None if m is None else DevBytes(n, 1, m.tobytes())
            dst, out = DevBytes(n * 4, 4), np.full(n * 4, SENTINEL, np.uint8)
            mk = None if m is None else (m if sloc == HOST else dm.ptr)
            encode(ctx, arr if sloc == HOST else src.ptr, kind, n, sloc, out if dloc == HOST else dst.ptr, dloc, mask=mk, sense=1, fill=-1000.0)
            got[sloc, dloc] = out.tobytes() if dloc == HOST else dst.read()
            assert src.read() == arr.tobytes() and (dm is None or dm.read() == m.tobytes()), "an input was written"
        assert got[HOST, HOST] == want
        assert all(v == want for v in got.values()), [k for k, v in got.items() if v != want]


def test_masked_sample_carries_the_fill_bits_and_a_nan_keeps_its_payload():
    ctx = gpu_context()
    arr = np.array([0x7FC12345, 0x3F800000, 0xFFC54321, 0x7F800001, 0x40490FDB], np.uint32).view(np.float32)
    mask = np.array([0, 1, 0, 0, 7], np.uint8)
    fill = struct.unpack("<f", struct.pack("<I", 0xC47A0000))[0]
    assert fill == -1000.0
    out = np.zeros(20, np.uint8)
    encode(ctx, arr, (-32, 0), 5, HOST, out, HOST, mask=mask, sense=1, fill=fill)
    assert out.tobytes() == bytes.fromhex("7FC12345" "C47A0000" "FFC54321" "7F800001" "C47A0000")
    encode(ctx, arr, (-32, 0), 5, HOST, out, HOST, mask=mask, sense=0, fill=fill)
    assert out.tobytes() == bytes.fromhex("C47A0000" "3F800000" "C47A0000" "C47A0000" "40490FDB")


# ---------------------------------------------------------------------------------------------- 3. refusals
def test_refusals_leave_the_destination_alone():
    ctx = gpu_context()
    n = 16
    arr = samples(np.float32, n)
    src, msk = DevBytes(4 * n + 16, 0, arr.tobytes() + bytes(16)), DevBytes(n, 0, bytes(n))
    cases = [   # (what, message part, src, bitpix, flip, n, mask, dst or None for a fresh buffer)
        ("bitpix 0", "bitpix", src.ptr, 0, 0, n, None, "new"), ("bitpix -16", "bitpix", src.ptr, -16, 0, n, None, "new"),
        ("bitpix 64", "bitpix", src.ptr, 64, 0, n, None, "new"), ("bitpix 24", "bitpix", src.ptr, 24, 0, n, None, "new"),
        ("flip with f32", "flip_sign", src.ptr, -32, 1, n, None, "new"), ("flip with f64", "flip_sign", src.ptr, -64, 1, n // 2, None, "new"),
        ("mask with 16", "mask", src.ptr, 16, 0, n, msk.ptr, "new"), ("mask with -64", "mask", src.ptr, -64, 0, n // 2, msk.ptr, "new"),
        ("mask with 32", "mask", src.ptr, 32, 1, n, msk.ptr, "new"),
        ("n = 0", "n", src.ptr, -32, 0, 0, None, "new"), ("NULL src", "src", None, -32, 0, n, None, "new"),
        ("NULL dst", "dst", src.ptr, -32, 0, n, None, None),
        ("overlap ahead", "overlaps", src.ptr, -32, 0, n, None, src.ptr + 4), ("overlap behind", "overlaps", src.ptr + 8, -32, 0, n, None, src.ptr),
        ("overlap by one byte", "overlaps", src.ptr, 8, 0, 17, None, src.ptr + 16),
    ]
    for what, part, s, bitpix, flip, count, mask, d in cases:
        dst = DevBytes(4 * n, 0) if d == "new" else None
        with pytest.raises(ValueError) as err:
            ctx.call("rip_stage_fits_encode", s, bitpix, flip, count, DEVICE, mask, 1, -1000.0, dst.ptr if dst else d, DEVICE)
        assert "fits_encode" in str(err.value) and part in str(err.value), f"{what}: {err.value}"
        rc = ctx.lib.rip_stage_fits_encode(*_native.marshal("rip_stage_fits_encode", (ctx.h, s, bitpix, flip, count, DEVICE, mask, 1, -1000.0,
                                                                                       dst.ptr if dst else d, DEVICE)))
        assert rc == _native.RIP_EINVAL, what
        ctx.synchronize()
        if dst:
            assert dst.read() == bytes([SENTINEL]) * (4 * n), what
        assert src.read() == arr.tobytes() + bytes(16), f"{what}: the source was written"
    # host arrays: the same refusals before any copy
    out = np.full(4 * n, SENTINEL, np.uint8)
    for s, bitpix, flip, count, mask, d in ((arr, 12, 0, n, None, out), (arr, -32, 1, n, None, out), (arr, 32, 0, n, np.zeros(n, np.uint8), out),
                                            (arr, -32, 0, 0, None, out), (None, -32, 0, n, None, out), (arr, -32, 0, n, None, None)):
        with pytest.raises(ValueError):
            ctx.call("rip_stage_fits_encode", s, bitpix, flip, count, HOST, mask, 1, 0.0, d, HOST)
    both = np.full(4 * n + 4, SENTINEL, np.uint8)
    with pytest.raises(ValueError):
        ctx.call("rip_stage_fits_encode", both[:4 * n], -32, 0, n, HOST, None, 1, 0.0, both[4:], HOST)
    assert np.all(out == SENTINEL) and np.all(both == SENTINEL)


# ---------------------------------------------------------------------------------------------- 4. write_fits
def five_hdus():
    rng = np.random.default_rng(5)
    cube = rng.standard_normal((3, 37, 53)).astype(np.float32)
    cube.reshape(-1)[:6] = np.array([0x7FC12345, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0xFFC00001], np.uint32).view(np.float32)
    return [{"data": None, "cards": [("ORIGIN", "romanimpreprocess_amd"), ("NHDU", 5)]},
            {"data": cube, "mask": rng.random(cube.shape) < 0.3, "mask_sense": 1, "fill": -1000.0},
            {"data": rng.integers(0, 2**32, (45, 67), dtype=np.uint32), "cards": [("GAIN", 1.5)]},
            {"data": rng.integers(-128, 128, (100, 131), dtype=np.int8), "extname": "MASK"},
            {"data": rng.standard_normal((4, 450)), "extname": "F64"}]   # 14400 bytes: five blocks, no padding


def on_device(items):
    return [dict(it, **{k: to_device(it[k]) for k in ("data", "mask") if it.get(k) is not None}) for it in items]


def test_write_fits(tmp_path):
    ctx = gpu_context()
    items = five_hdus()
    want = fr.fits_file(items)
    assert len(want) % 2880 == 0 and items[4]["data"].nbytes % 2880 == 0
    files = {}
    for name, its, kw in (("host", items, {}), ("host_chunks", items, {"chunk_bytes": 4096}), ("device", on_device(items), {}),
                          ("device_chunks", on_device(items), {"chunk_bytes": 4096}), ("odd_chunks", on_device(items), {"chunk_bytes": 1000})):
        path = tmp_path / f"{name}.fits"
        path.write_bytes(b"an older, longer file" * 10000)   # replaced, not patched
        calio.write_fits(str(path), its, ctx=ctx, **kw)
        files[name] = path.read_bytes()
        assert files[name] == want, f"{name}: the file differs from the restatement"
    assert len(set(files.values())) == 1
    # the restatement's parser and the package's reader on the same file
    hdus = fr.parse_hdus(files["device_chunks"])
    assert len(hdus) == 5 and hdus[0][0]["NAXIS"] == 0 and hdus[0][0]["ORIGIN"] == "romanimpreprocess_amd" and hdus[3][0]["EXTNAME"] == "MASK"
    assert np.array_equal(fr.unit_array(*hdus[2]).astype(np.int64) + 2**31, items[2]["data"])
    assert np.array_equal(fr.unit_array(*hdus[3]).astype(np.int64) - 128, items[3]["data"])
    path = str(tmp_path / "device_chunks.fits")
    masked = np.where(items[1]["mask"], np.float32(-1000.0), items[1]["data"])
    for sel in (4, "F64", "f64 "):
        h, d = calio.read_fits_image(path, sel)
        assert d.dtype == np.dtype(">f8") and d.tobytes() == items[4]["data"].astype(">f8").tobytes() and h["EXTNAME"] == "F64"
    h, d = calio.read_fits_image(path, 1)
    assert d.shape == (3, 37, 53) and d.tobytes() == fr.stored(masked)
    assert calio.read_fits_image(path, 0)[1] is None
    # int16 and uint16 units come back through the reader, by index and by name
    raw = np.random.default_rng(6).integers(-32768, 32768, (9, 41), dtype=np.int16)
    u16 = dc.cube_u16(2, 5, 33, 8)
    calio.write_fits(path, [raw, {"data": to_device(u16), "extname": "DARK"}, {"data": to_device(raw), "extname": "RAW"}], ctx=ctx)
    for sel in (0, 2, "RAW"):
        assert calio.read_fits_image(path, sel)[1].tobytes() == raw.astype(">i2").tobytes()
    h, d = calio.read_fits_image(path, "DARK")
    assert h["BZERO"] == 32768 and h["BSCALE"] == 1 and np.array_equal((d.astype(np.int32) + 32768).astype(np.uint16), u16)
    # what cannot be written is refused before the file is touched
    before = open(path, "rb").read()
    for bad in ([np.zeros(3, np.int64)], [np.zeros(3, bool)], [np.zeros(3, np.float16)], [np.zeros((4, 4), np.float32)[:, ::2]],
                [{"data": np.zeros(3, np.int16), "mask": np.zeros(3, np.uint8)}], [{"data": np.zeros(3, np.float32), "bogus": 1}], []):
        with pytest.raises((TypeError, ValueError)):
            calio.write_fits(path, bad, ctx=ctx)
    assert open(path, "rb").read() == before


# ---------------------------------------------------------------------------------------------- 5. convert_file
GROWN = {1: "DO_NOT_USE", 5: "JUMP_DET", 9: "DEAD", 25: "DROPOUT"}   # PixelMask1's growth of these flags


@pytest.mark.parametrize("turn", range(4))
def test_convert_file(tmp_path, turn):
    """40 x 48, flags of growth 1, 5, 9 and 25 at the corners, on the edges, one pixel in and in the interior; over the four
    turns every position carries every growth"""
    ctx = gpu_context()
    shape = (40, 48)
    rng = np.random.default_rng(40 + turn)
    data = rng.standard_normal(shape).astype(np.float32)
    data[10, 10], data[20, 20], data[0, 0] = np.float32(np.nan), np.float32(-0.0), np.float32(np.nan)   # unmasked, unmasked, masked
    dq = np.zeros(shape, np.uint32)
    by_footprint = np.zeros(shape, bool)
    for k, (y, x) in enumerate(pe.edge_positions(shape)):
        grow = (1, 5, 9, 25)[(k + turn) % 4]
        assert maskhandling.PixelMask1.array[int(getattr(pixel, GROWN[grow])).bit_length() - 1] == grow
        dq[y, x] |= np.uint32(int(getattr(pixel, GROWN[grow])))
        by_footprint |= pe.footprint(shape, y, x, grow)
    dq[10, 30] |= np.uint32(int(pixel.SATURATED))   # not in PixelMask1: masks nothing
    mask_ref = opost.build_mask(dq)
    assert np.array_equal(mask_ref, by_footprint) and not mask_ref[10, 30] and 0 < mask_ref.sum() < mask_ref.size
    l2 = str(tmp_path / "l2.asdf")
    calio.write_asdf(l2, {"roman": {"data": data, "dq": dq}})
    out = str(tmp_path / "sim_L2_mask.fits")
    maskhandling.PixelMask1.convert_file(l2, out, ctx=ctx)
    want = fr.fits_file([{"data": np.where(mask_ref, -1000.0, data).astype(np.float32)},
                         {"data": np.where(mask_ref, 1, 0).astype(np.int8), "extname": "MASK"}])
    got = open(out, "rb").read()
    assert got == want
    hdus = fr.parse_hdus(got)
    assert np.array_equal(fr.unit_array(*hdus[1]).astype(np.int16) - 128, mask_ref.astype(np.int16)) and hdus[1][0]["BZERO"] == -128
    out_asdf = str(tmp_path / "sim_L2_mask.asdf")
    maskhandling.PixelMask1.convert_file(l2, out_asdf, ctx=ctx)
    m = np.asarray(calio.read_asdf(out_asdf)["mask"])
    assert m.dtype == np.bool_ and np.array_equal(m, mask_ref)
    # an .npz mirror of the L2 tree serves too; another ending writes nothing
    calio.save_npz_tree(str(tmp_path / "l2.npz"), {"roman": {"data": data, "dq": dq}})
    maskhandling.PixelMask1.convert_file(str(tmp_path / "l2.npz"), str(tmp_path / "again.fits"), ctx=ctx)
    assert open(tmp_path / "again.fits", "rb").read() == want
    maskhandling.PixelMask1.convert_file(l2, str(tmp_path / "mask.txt"), ctx=ctx)
    assert not (tmp_path / "mask.txt").exists()


# ---------------------------------------------------------------------------------------------- 6, 7. the two drivers
@pytest.fixture(scope="module")
def exposure(tmp_path_factory):
    """the 48 x 256 frame of six groups of test_calibrateimage_files_end_to_end as files, calibrated with and without FITSOUT"""
    tmp = tmp_path_factory.mktemp("fitsout")
    rp = synth.READ_PATTERN_6
    cal = synth.make_caldir(48, 256, read_pattern=rp, p_order=3, seed=31, bias_amplitude=1.0)
    ramp = synth.make_ramp(cal, read_pattern=rp, seed=32, cr_frac=0.02)
    caldir = {}
    for key, fname in {"dark": "dark", "read": "read", "gain": "gain", "linearitylegendre": "linearitylegendre", "ipc4d": "ipc4d",
                       "flat": "pflat", "biascorr": "biascorr", "mask": "mask", "saturation": "saturation"}.items():
        caldir[key] = str(tmp / f"roman_wfi_{fname}_TEST_SCA04.asdf")
        calio.write_asdf(caldir[key], {"roman": cal[key]})
    calio.write_asdf(str(tmp / "l1.asdf"), {"roman": {"data": ramp["data"], "amp33": ramp["amp33"], "meta": {
        "exposure": {"frame_time": synth.FRAME_TIME, "read_pattern": rp}, "instrument": {"detector": "WFI04"}}}})
    config = {"IN": str(tmp / "l1.asdf"), "OUT": str(tmp / "l2.asdf"), "CALDIR": caldir, "SLICEOUT": True,
              "JUMP_DETECT_PARS": {"SthreshA": 5.0, "IthreshB": 800.0}, "FITSOUT": True}
    cb = pipeline.Calibrator(ctx=chain_context())
    # first without the key, to the same OUT: the two L2 files then record configurations that differ in that key alone
    gen_cal_image.calibrateimage(dict(config, FITSOUT=False), verbose=False, calibrator=cb)
    plain = open(config["OUT"], "rb").read()
    assert not (tmp / "l2_asdf_to.fits").exists()
    gen_cal_image.calibrateimage(config, verbose=False, calibrator=cb)
    before = sorted(p.name for p in tmp.iterdir())
    assert gen_cal_image.calibrateimage(dict(config, OUT=None), verbose=False, calibrator=cb)["roman"]["data"].shape == (40, 248)
    assert sorted(p.name for p in tmp.iterdir()) == before   # OUT = None writes nothing, FITSOUT or not
    return tmp, config, plain


def test_calibrateimage_fitsout(exposure):
    tmp, config, plain = exposure
    l2 = calio.read_asdf(config["OUT"])["roman"]
    data, dq = np.asarray(l2["data"]), np.asarray(l2["dq"])
    assert data.dtype == np.float32 and dq.dtype == np.uint32 and data.shape == (40, 248)
    good = ~opost.build_mask(dq)   # of the ACTIVE-region flags, as the reference builds it from im2["dq"]
    assert 0 < np.count_nonzero(~good) < good.size
    got = open(str(tmp / "l2_asdf_to.fits"), "rb").read()
    assert got == fr.fits_file([{"data": data}, {"data": dq}, {"data": np.where(good, data, -1000).astype(np.float32)}])
    hdus = fr.parse_hdus(got)
    assert [h["BITPIX"] for h, _ in hdus] == [-32, 32, -32] and hdus[1][0]["BZERO"] == 2147483648 and "XTENSION" in hdus[2][0]
    # the L2 file is the one written without FITSOUT, bit for bit, but for the key in the configuration it records
    with_key = open(config["OUT"], "rb").read()
    assert with_key.count(b"FITSOUT: true") == 1 and plain.count(b"FITSOUT: false") == 1
    assert with_key.replace(b"FITSOUT: true", b"FITSOUT: false") == plain


@pytest.mark.parametrize("precision", [32, 16])
def test_generate_all_noise_fitsout(exposure, precision):
    tmp, config, _ = exposure
    out = str(tmp / f"noise{precision}.asdf")
    cfg = dict(config, NOISE={"LAYER": ["R"], "TEMP": str(tmp / "tmp.asdf"), "SEED": 11, "OUT": out}, NOISE_PRECISION=precision)
    with contextlib.redirect_stdout(io.StringIO()):
        gen_noise_image.generate_all_noise(cfg)
    noise = np.asarray(calio.read_asdf(out)["noise"])
    assert noise.shape == (1, 40, 248) and noise.dtype == (np.float32 if precision == 32 else np.float16) and np.nanstd(noise.astype(np.float64)) > 0
    got = open(out[:-5] + "_asdf_to.fits", "rb").read()
    assert got == fr.header(noise.shape, np.float32) + fr.data_unit(noise.astype(np.float32))
    (head, raw), = fr.parse_hdus(got)
    assert head["BITPIX"] == -32 and raw == noise.astype(np.float32).astype(">f4").tobytes()
    # without the key no FITS file appears
    quiet = dict(cfg, FITSOUT=False, NOISE=dict(cfg["NOISE"], OUT=str(tmp / f"quiet{precision}.asdf")))
    with contextlib.redirect_stdout(io.StringIO()):
        gen_noise_image.generate_all_noise(quiet)
    assert not (tmp / f"quiet{precision}_asdf_to.fits").exists()
    assert np.asarray(calio.read_asdf(quiet["NOISE"]["OUT"])["noise"]).tobytes() == noise.tobytes()


# ---------------------------------------------------------------------------------------------- 8. a calibration-file dump
def test_make_dark_file_dumps(tmp_path, monkeypatch):
    """the frame of test_make_dark_file_module: the two _asdf_data.fits hold an empty primary HDU and the planes of the trees"""
    rng = np.random.default_rng(21)
    ny, width, nside, reads = cc.NY, cc.NX + 4, cc.NX, cc.READS_PROD
    for j, c in enumerate(dc.dark_exposures(3, 35, ny, width, seed=70)):
        dc.write_dark_fits(tmp_path / f"dark_{j + 1:03d}.fits", c)
    planes = (300 * rng.random((7, ny, width))).astype(np.float32)
    keys = [("DARK1", 3), ("DARK1ERR", 4), ("DARK2", 1), ("DARK2ERR", 2), ("CDS", 0), ("RESET", 6), ("ACN", 1.25), ("C_PINK", 2.5),
            ("U_PINK", 0.75), ("EXTNAME", "NOISE")]
    with open(tmp_path / "summary.fits", "wb") as f:
        f.write(dc.fits_hdu(None))
        f.write(dc.fits_hdu(planes, keys, extension=True))
    with open(tmp_path / "settings_prod.yaml", "w") as f:
        yaml.safe_dump({"READS": reads}, f)
    monkeypatch.chdir(tmp_path)
    out = str(tmp_path / "cal_dark_X.asdf")
    with contextlib.redirect_stdout(io.StringIO()):
        files = make_dark_file.run("prod", str(tmp_path / "dark_001.fits"), str(tmp_path / "summary.fits"), 7, out, nside=nside,
                                   ctx=gpu_context())
    dark, read = calio.roman_branch(files[0]), calio.roman_branch(files[1])
    got = open(str(tmp_path / "cal_dark_X_asdf_data.fits"), "rb").read()
    hdus = fr.parse_hdus(got)
    assert len(hdus) == 5 and hdus[0][0]["NAXIS"] == 0 and hdus[0][1] == b""
    for (head, raw), key in zip(hdus[1:], ("data", "dq", "dark_slope", "dark_slope_err")):
        assert raw == fr.stored(np.asarray(dark[key])), key
        assert [head[f"NAXIS{i}"] for i in range(head["NAXIS"], 0, -1)] == list(np.asarray(dark[key]).shape)
    assert got == fr.fits_file([{"data": None}] + [{"data": np.asarray(dark[k])} for k in ("data", "dq", "dark_slope", "dark_slope_err")])
    got = open(str(tmp_path / "cal_read_X_asdf_data.fits"), "rb").read()
    assert len(fr.parse_hdus(got)) == 3
    assert got == fr.fits_file([{"data": None}, {"data": np.asarray(read["data"])}, {"data": np.asarray(read["resetnoise"])}])


def test_make_gain_file_dumps(tmp_path):
    """the 140 x 140 frame of test_gpu_gainfile's drop-in test: the gain plane, and ipc4d as one (3 ny, 3 nx) image in which
    pixel (y, x) of kernel element (j, i) sits at (j * ny + y, i * nx + x) -- the script's transpose of axes 1 and 2"""
    listfile, _, _ = gc.write_summaries(str(tmp_path), "gainfile_even")
    outfile = str(tmp_path / "roman_wfi_gain_TEST_SCA07.asdf")
    with contextlib.redirect_stdout(io.StringIO()):
        files = make_gain_file.run(listfile, 7, outfile, shape=(140, 140), ctx=gpu_context())
    gain, kernel = (np.asarray(calio.read_asdf(p)["roman"]["data"]) for p in files)
    assert gain.dtype == np.float32 and kernel.dtype == np.float64 and kernel.shape == (3, 3, 132, 132)
    got = open(outfile[:-5] + "_asdf_data.fits", "rb").read()
    assert got == fr.fits_file([{"data": None}, {"data": gain}])
    got = open(files[1][:-5] + "_asdf_data.fits", "rb").read()
    tiled = np.transpose(kernel, axes=(0, 2, 1, 3)).reshape((3 * 132, 3 * 132))
    assert got == fr.fits_file([{"data": None}, {"data": tiled}])
    (_, _), (head, raw) = fr.parse_hdus(got)
    image = fr.unit_array(head, raw)
    assert head["BITPIX"] == -64 and image.shape == (396, 396)
    for j, y, i, x in ((0, 0, 0, 0), (1, 5, 2, 7), (2, 131, 1, 130), (1, 66, 1, 66)):
        assert image[j * 132 + y, i * 132 + x] == kernel[j, i, y, x]


def test_postprocess_calfiles_dump(tmp_path, monkeypatch):
    """the 48 x 256 set of test_gpu_calfiles' drop-in test: biascorr and the predicted dark as one (2 ngrp, ny - 8, nx - 8) cube"""
    ctx = gpu_context()
    rp = synth.READ_PATTERN_6
    cal = synth.make_caldir(48, 256, read_pattern=rp, p_order=3, seed=41)
    lin = dict(cal["linearitylegendre"], pflat=cal["flat"]["data"][None].copy())
    stem = str(tmp_path / "roman_wfi_{}_TEST_SCA04.asdf")
    for key, tree in (("dark", cal["dark"]), ("gain", cal["gain"]), ("linearitylegendre", lin)):
        calio.write_asdf(stem.format(key), {"roman": tree})
    reads = calfiles.reads_of_pattern(rp)
    lpars = {"TFRAME": synth.FRAME_TIME, "BIAS": {"SLICE": 1}}
    with contextlib.redirect_stdout(io.StringIO()):
        files = postprocess_calfiles.run(stem.format("linearitylegendre"), 4, reads=reads, lpars=lpars, ctx=ctx)
    bc = np.asarray(calio.read_asdf(files[2])["roman"]["data"])
    _, _, pred = calfiles.derive_biascorr(cal["dark"]["dark_slope"], cal["dark"]["data"], lin["data"], lin["Smin"], lin["Smax"], reads,
                                          tframe=synth.FRAME_TIME, bframe=1, want_pred=True, ctx=ctx)
    assert bc.shape == pred.shape == (len(rp), 40, 248) and bc.dtype == pred.dtype == np.float32
    got = open(files[2][:-5] + "_asdf_to.fits", "rb").read()
    assert got == fr.fits_file([{"data": np.concatenate([bc, pred])}])
    (head, raw), = fr.parse_hdus(got)
    assert (head["NAXIS3"], head["NAXIS2"], head["NAXIS1"]) == (2 * len(rp), 40, 248)
