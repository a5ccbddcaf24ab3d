"""The six entries that read raw 16-bit samples (csrc/rip_samples.h: rip_cal_group_means, rip_cal_frame_sums, rip_cal_noise_add,
rip_cal_corr_pair, rip_cal_raw_frame, rip_cal_frame_slopes) against ONE numpy decode, at the smallest shapes that still have a
vector body, a row tail and a band.  Per entry every combination of storage (native, FITS; the raw frame also FITS int16), form
(8 samples per lane; one sample per lane, forced by a width that is no multiple of 8 and by a device view that starts one
sample off a 16-byte boundary) and location (host array, device) gives the bits of the numpy restatement the entry already has in
tests/ -- and so the same bits as every other combination.  Every cube holds the words 0x0000, 0x00FF, 0xFF00, 0x7FFF, 0x8000
and 0xFFFF: a missing swap, a missing top-bit flip or swapped halves of a dword change at least one of them."""

import corr_ref as cr
import darkstack_ref as dr
import linfit_ref as lr
import noise_run_ref as nr
import numpy as np
import pytest
import rawframes_ref as rr
from conftest import assert_same_bits, gpu_context

from romanimpreprocess_amd import _native
from romanimpreprocess_amd.calfiles import convert_frames

pytestmark = pytest.mark.gpu

HOST, DEVICE = _native.RIP_HOST, _native.RIP_DEVICE
EDGE_WORDS = (0x0000, 0x00FF, 0xFF00, 0x7FFF, 0x8000, 0xFFFF)
WHERE = ("host", "device", "offset")   # offset: a device view one sample behind a 16-byte boundary (the one-sample form)


def samples(shape, seed, row=0, span=(0, 65536)):
    """random uint16 samples from `span` with the six edge words, in an order of its own per frame, in the columns 2 .. 7 of row
    `row` of every frame: both halves of three dwords, inside every band, crop and border used below"""
    rng = np.random.default_rng(seed)
    a = rng.integers(*span, shape).astype(np.uint16)
    for frame in a.reshape((-1,) + tuple(shape[-2:])):
        frame[row, 2:8] = rng.permutation(EDGE_WORDS)
    assert all((a == w).any() for w in EDGE_WORDS)
    return a


def stored_words(a, stored):
    """the samples as a file of storage `stored` holds them (rawframes_ref.encode), as raw 16-bit words; the one decode that every
    entry is held to gives them back"""
    s = rr.encode(a, stored)
    assert_same_bits(rr.decode(s, stored), a, f"the numpy decode of storage {stored}")
    return np.ascontiguousarray(s).view(np.uint16)


def bits(a):
    """a numpy array as the torch tensor that carries its bits on the device"""
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(f"{'f' if a.dtype.kind == 'f' else 'i'}{a.dtype.itemsize}")).cuda()


def back(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


def put(words, where):
    """(argument, location, what keeps it alive) of a cube of raw words for an entry"""
    import torch

    if where == "host":
        return words, HOST, None
    off = 1 if where == "offset" else 0
    keep = torch.zeros(words.size + 8, dtype=torch.int16, device="cuda")
    keep[off:off + words.size] = bits(words.reshape(-1))
    assert keep.data_ptr() % 16 == 0
    return keep.data_ptr() + 2 * off, DEVICE, keep


def sync():
    import torch

    torch.cuda.synchronize()   # the library works on a stream of its own


# ------------------------------------------------------------------------------------------------ group means, frame sums
# 3 reads of 5 rows, the band y0 = 1, ny = 3: width 24 with nx = 20 (two whole vectors and a tail of 4), width 13 with nx = 13
BAND_SHAPES = [(24, 20), (13, 13)]
NREADS, NY_FILE, Y0, NY = 3, 5, 1, 3
READS = np.array([0, 1, 1, 3], np.int32)   # a group of one read and one of two


@pytest.mark.parametrize("width, nx", BAND_SHAPES)
def test_group_means(width, nx):
    ctx = gpu_context()
    cube = samples((NREADS, NY_FILE, width), 1, row=Y0)
    want = dr.group_means(cube[:, Y0:Y0 + NY], READS, nx)
    for be16 in (0, 1):
        words = stored_words(cube, be16)
        for where in WHERE:
            src, loc, keep = put(words, where)
            stack = bits(np.full((2, 2, NY, nx), -7.0, np.float32))   # (groups, capacity 2, ny, nx): slot 1 is written
            sync()
            ctx.call("rip_cal_group_means", src, loc, NREADS, NY_FILE, width, Y0, NY, nx, READS, 2, be16, stack, 2, 1)
            got = stack.cpu().numpy()
            assert_same_bits(got[:, 1], want, f"width {width} nx {nx} FITS {be16} {where}")
            assert np.all(got[:, 0] == -7.0), "slot 0 was written"


@pytest.mark.parametrize("width, nx", BAND_SHAPES)
@pytest.mark.parametrize("f0", [0, 1])
def test_frame_sums(width, nx, f0):
    """added to sums that are not zero: the read-modify-write, in 16-byte pieces (nx 20) and word by word"""
    ctx = gpu_context()
    cube = samples((NREADS, NY_FILE, width), 2, row=Y0)
    base = np.random.default_rng(3).integers(0, 1 << 31, (NREADS - f0, NY, nx)).astype(np.uint32)
    for be16 in (0, 1):
        words = stored_words(cube, be16)
        want = lr.frame_sums(base.copy(), words, f0, (Y0, Y0 + NY), nx, bool(be16))
        for where in WHERE:
            src, loc, keep = put(words, where)
            sums = bits(base)
            sync()
            ctx.call("rip_cal_frame_sums", src, loc, NREADS, NY_FILE, width, Y0, NY, nx, f0, be16, sums, 1)
            assert_same_bits(back(sums, base), want, f"width {width} nx {nx} f0 {f0} FITS {be16} {where}")


# ------------------------------------------------------------------------------------------------ noise add
@pytest.mark.parametrize("cw", [8, 6])
def test_noise_add(cw):
    """128 rows (the entry's minimum), C = 2 and the reference output, the frames 1 .. 3 of 4; cw = 8 (width 24): one lane per 8
    samples, cw = 6 (width 18): one per sample.  The accumulators start from values that are not zero"""
    ctx = gpu_context()
    ny, C, nreads, f0, n = 128, 2, 4, 1, 3
    width = (C + 1) * cw
    cube = samples((nreads, ny, width), 4)
    rng = np.random.default_rng(5)
    base = nr.new_acc(ny, C, cw, True)
    for k, a in base.items():
        a[...] = rng.integers(-1000 if a.dtype.kind == "i" else 0, 1000, a.shape).astype(a.dtype)
    want = {k: a.copy() for k, a in base.items()}
    want_rowsum = nr.add(want, cube, C, cw, True, f0, n)
    for be16 in (0, 1):
        words = stored_words(cube, be16)
        for where in WHERE:
            src, loc, keep = put(words, where)
            acc = {k: bits(a) for k, a in base.items()}
            rowsum = bits(np.full(want_rowsum.shape, 0xAAAAAAAA, np.uint32))
            sync()
            ctx.call("rip_cal_noise_add", src, loc, nreads, ny, width, C, cw, 1, f0, n, be16, 1,
                     *[acc[k] for k in ("a0", "a1", "b0", "b1", "s0", "s1", "c0", "c1", "m33")], rowsum)
            for k in base:
                assert_same_bits(back(acc[k], base[k]), want[k], f"cw {cw} FITS {be16} {where}: {k}")
            assert_same_bits(back(rowsum, want_rowsum), want_rowsum, f"cw {cw} FITS {be16} {where}: row sums")


# ------------------------------------------------------------------------------------------------ pair statistics
@pytest.mark.parametrize("s", [8, 4])
def test_corr_pair(s):
    """a 16 x 16 frame in a 16 x 24 file, border 1, the frames 0 .. 3 of 5; 8 x 8 superpixels (one lane per 8 samples where all
    eight frames allow it) and 4 x 4 (one per sample); either cube on the host, in HBM or in HBM off the boundary.  The random
    words span 256 values, so the pixels of the edge words are rejected and read a second time"""
    ctx = gpu_context()
    nreads, ny_file, nx_file, ny, nx, nb = 5, 16, 24, 16, 16, 1
    frames = (0, 1, 2, 3)
    c1, c2 = (samples((nreads, ny_file, nx_file), seed, row=2, span=(30000, 30256)) for seed in (6, 7))
    want = cr.pair_table(c1, c2, frames, ny, nx, nb, s, s)
    assert 0 < want[..., 0].sum() < (ny - 2 * nb) * (nx - 2 * nb), "no pixel is rejected"
    for be16 in (0, 1):
        w1, w2 = stored_words(c1, be16), stored_words(c2, be16)
        assert_same_bits(cr.native(w1, be16), c1, "corr_ref's own decode")
        for where1, where2 in (("host", "device"), ("device", "host"), ("device", "device"), ("host", "host"), ("offset", "device"),
                               ("device", "offset")):
            a, la, keep_a = put(w1, where1)
            b, lb, keep_b = put(w2, where2)
            got = np.full(want.shape, -1, np.int64)
            sync()
            ctx.call("rip_cal_corr_pair", a, la, b, lb, nreads, ny_file, nx_file, be16, *frames, ny, nx, nb, s, s, got, HOST)
            assert_same_bits(got, want, f"superpixels of {s} FITS {be16} {where1} / {where2}")


# ------------------------------------------------------------------------------------------------ raw frame, slopes
@pytest.mark.parametrize("ny, nx, nflip", [(4, 16, 8), (3, 12, 5)])
def test_raw_frame(ny, nx, nflip):
    """4 x 16 with 8 mirrored columns: chunks of 8; 3 x 12 with 5: single samples.  Every orientation and all three storages"""
    import torch

    ctx = gpu_context()
    frame = samples((ny, nx), 8)
    for orient in (0, 1, 2):
        want = rr.orient_frame(frame, orient, nflip)
        for stored in rr.STORED:
            words = stored_words(frame, stored)
            for where in WHERE:
                src, loc, keep = put(words, where)
                dst = torch.full((ny, nx), -21846, dtype=torch.int16, device="cuda")   # 0xAAAA
                sync()
                ctx.call("rip_cal_raw_frame", src, loc, ny, nx, orient, nflip, stored, dst)
                assert_same_bits(back(dst, want), want, f"({ny},{nx},{nflip}) orient {orient} stored {stored} {where}")


@pytest.mark.parametrize("npix", [16, 12])
def test_frame_slopes(npix):
    """nc = 4 of 5 planes (the second image is 0 / 0 = NaN in the restatement too); the cube is native and in HBM, on a 16-byte
    boundary and one sample off it; the images to the host and to the device"""
    import torch

    ctx = gpu_context()
    N, nc = 5, 4
    cube = samples((1, N, 1, npix), 9)
    want = rr.slopes(cube, nc)
    w0, de0, w1, de1 = convert_frames.slope_weights(nc)
    for where in ("device", "offset"):
        src, _, keep = put(cube.reshape(-1), where)
        host = np.full((2, 1, npix), -7.0, np.float32)
        dev = torch.full((2, 1, npix), -7.0, dtype=torch.float32, device="cuda")
        sync()
        ctx.call("rip_cal_frame_slopes", src, N, nc, npix, w0, de0, w1, de1, host, HOST)
        ctx.call("rip_cal_frame_slopes", src, N, nc, npix, w0, de0, w1, de1, dev, DEVICE)
        assert_same_bits(host, want, f"npix {npix} {where}, host output")
        assert_same_bits(dev.cpu().numpy(), want, f"npix {npix} {where}, device output")
