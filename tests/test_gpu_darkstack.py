"""The dark-file arithmetic on the device (csrc/darkstack.hip, romanimpreprocess_amd/calfiles/darkstack.py, make_dark_file.py)
against tests/darkstack_ref.py: the masks are compared through the counts, exactly, and the means bit for bit, on EVERY pixel --
tests/test_host_darkstack_ref.py proves that no input used here has a value near a bound.  There is one form of the clip kernel
(512 planes of 64 pixels fit in LDS), so there is no second form to compare it with; the two forms of the group-means kernel
(16-byte loads where the frame width is a multiple of 8, single samples elsewhere) are held against each other."""

import contextlib
import io
import os

import calfiles_cases as cc
import darkstack_cases as dc
import darkstack_ref as dr
import numpy as np
import pytest
import yaml
from conftest import assert_same_bits, gpu_context

from romanimpreprocess_amd import _native, calfiles, calio
from romanimpreprocess_amd.calfiles import make_dark_file
from romanimpreprocess_amd.devarray import DevArray

pytestmark = pytest.mark.gpu

F = np.float32
CLIP = dc.clip_cases()
_REF = {}


def clip_ref(name):
    if name not in _REF:
        stack, kw = CLIP[name]
        _REF[name] = dr.sigma_clip_mean(stack, **kw)[:2]
    return _REF[name]


def dev(a):
    import torch

    if a.dtype == np.uint16:
        return DevArray(torch.from_numpy(a.view(np.int16)).cuda(), np.uint16)
    if a.dtype == np.dtype(">i2"):
        return DevArray(torch.from_numpy(a.view(np.int16)).cuda(), np.int16)
    return DevArray(torch.from_numpy(np.ascontiguousarray(a)).cuda())


# ------------------------------------------------------------------------------------------------ the clip: values
@pytest.mark.parametrize("name", list(CLIP))
def test_clip_equals_the_restatement(name):
    """plane counts 1, 2, 3, 4, 63, 64, 65, 257, 512 and pixel counts 1, 63, 65, 64 k + 7; an outlier of the second round; the
    ladder with maxiters 5 (stops early) and 16 (converges); ties at the median; a constant column; values on a bound (kept) and
    just outside (nothing survives); NaN, +-inf, all-NaN columns; sigma_lower != sigma_upper; negative values and +-0; no round"""
    stack, kw = CLIP[name]
    mean, count = calfiles.sigma_clip_mean(stack, want_count=True, ctx=gpu_context(), **kw)
    rm, rc = clip_ref(name)
    assert_same_bits(count, rc, f"{name} count")
    assert_same_bits(mean, rm, f"{name} mean")
    assert_same_bits(calfiles.sigma_clip_mean(stack, ctx=gpu_context(), **kw), rm, f"{name} without the counts")


def test_clip_ladder_stops_early_and_converges():
    assert np.all(clip_ref("ladder_5")[1] == 11) and np.all(clip_ref("ladder_16")[1] == 9)
    a = dc.ladder()
    for rounds in (7, 15):   # converged after 7 rounds: more rounds change nothing
        m, c = calfiles.sigma_clip_mean(a, maxiters=rounds, want_count=True, ctx=gpu_context())
        assert_same_bits(c, clip_ref("ladder_16")[1])
        assert_same_bits(m, clip_ref("ladder_16")[0])


def test_clip_refusals():
    ctx = gpu_context()
    a = dc.noisy(4, 70, 1)
    with pytest.raises(ValueError, match="513 planes"):
        calfiles.sigma_clip_mean(np.zeros((513, 3), F), ctx=ctx)
    for kw in ({"maxiters": 17}, {"maxiters": -1}, {"sigma": -1.0}, {"sigma": np.inf}, {"sigma_upper": np.nan}):
        with pytest.raises(ValueError):
            calfiles.sigma_clip_mean(a, ctx=ctx, **kw)
    with pytest.raises(TypeError):
        calfiles.sigma_clip_mean(a.astype(np.float64), ctx=ctx)
    mean = np.full(70, 7, F)
    rc = ctx.lib.rip_cal_sigma_clip_mean(ctx.h, a.ctypes.data, _native.RIP_HOST, 4, 69, 70, 3.0, 3.0, 5, mean.ctypes.data, None)
    assert rc == -1 and np.all(mean == 7)   # a plane stride below the plane


# ------------------------------------------------------------------------------------------------ the clip: addressing
def test_clip_of_the_first_planes_of_a_larger_stack_host_and_device_twice():
    ctx = gpu_context()
    a = dc.noisy(37, 199, 120)
    rm, rc, _ = dr.sigma_clip_mean(a[:20])
    m, c = calfiles.sigma_clip_mean(a, n=20, want_count=True, ctx=ctx)            # capacity 37 > n = 20
    assert_same_bits(c, rc, "host count")
    assert_same_bits(m, rm, "host mean")
    d = dev(a)
    runs = [calfiles.sigma_clip_mean(d, n=20, want_count=True, ctx=ctx) for _ in range(2)]
    for dm, dcnt in runs:
        assert isinstance(dm, DevArray) and isinstance(dcnt, DevArray) and dm.shape == (199,) and dcnt.dtype == np.int32
        assert_same_bits(dm.numpy(), m, "device mean against host mean, and run against run")
        assert_same_bits(dcnt.numpy(), c, "device count")
    # a plane stride above the plane: the pixels 7 .. 136 of every plane
    got, cnt = np.empty(130, F), np.empty(130, np.int32)
    ctx.check(ctx.lib.rip_cal_sigma_clip_mean(ctx.h, a[:, 7:].ctypes.data, _native.RIP_HOST, 20, 199, 130, 3.0, 3.0, 5,
                                              got.ctypes.data, cnt.ctypes.data))
    assert_same_bits(got, rm[7:137], "strided mean")
    assert_same_bits(cnt, rc[7:137], "strided count")
    # a stack of more dimensions keeps them
    m3 = calfiles.sigma_clip_mean(a[:, :198].reshape(37, 2, 99)[:20].copy(), ctx=ctx)
    assert_same_bits(m3, rm[:198].reshape(2, 99))


# ------------------------------------------------------------------------------------------------ group means
def stack_of(cubes, reads, ny, nx, cap, be16=False, on_device=False, rows=None):
    st = calfiles.DarkStack(reads, ny, nx, cap, ctx=gpu_context(), rows=rows)
    for c in cubes:
        if be16:
            c = dr.to_fits_be16(c)
        st.add(dev(c) if on_device else c, fits_be16=be16)
    return st


@pytest.mark.parametrize("width, nx", [(140, 130), (67, 67), (144, 130), (72, 72)])
def test_group_means(width, nx):
    """groups of 1, 2 and 16 reads with gaps; a cropped and a full frame in both forms of the kernel (widths 140 and 67: single
    samples; 144 and 72: 16-byte loads, with a partial last vector and with 16-byte stores); samples 0 and 65535; FITS storage
    against native samples; host arrays against device arrays; slots 0 and capacity - 1"""
    cubes = [dc.cube_u16(30, 5, width, 50 + j) for j in range(3)]
    want = [dr.group_means(c, dc.READS_MIXED, nx) for c in cubes]
    st = stack_of(cubes, dc.READS_MIXED, 5, nx, 3)
    got = st.stack.numpy()
    assert got.shape == (4, 3, 5, nx)
    for j in (0, 1, 2):
        assert_same_bits(got[:, j], want[j], f"slot {j}")
    assert want[0][0, 0, 0] == 0 and want[0][0, 0, 1] == 65535 and want[0][1, 1, 2] == F(32767.5)
    for kw in ({"be16": True}, {"on_device": True}, {"be16": True, "on_device": True}):
        assert_same_bits(stack_of(cubes, dc.READS_MIXED, 5, nx, 3, **kw).stack.numpy(), got, str(kw))
    with pytest.raises(ValueError, match="holds 3 exposures already"):
        st.add(cubes[0])


def test_group_means_forms_agree_and_300_reads():
    wide = dc.cube_u16(30, 5, 144, 77)
    narrow = np.ascontiguousarray(wide[:, :, :140])
    a = stack_of([wide], dc.READS_MIXED, 5, 130, 1).stack.numpy()
    b = stack_of([narrow], dc.READS_MIXED, 5, 130, 1).stack.numpy()
    assert_same_bits(a, b, "16-byte loads against single samples")
    reads = [0, 300, 1, 300, 7, 290]
    for width in (24, 21):
        c = dc.cube_300(2, width)
        got = stack_of([c], reads, 2, width, 1).stack.numpy()[:, 0]
        assert_same_bits(got, dr.group_means(c, reads), f"300 reads, width {width}")
        assert np.any(got[0] != c.astype(np.float64).mean(axis=0).astype(F))   # the order of the f32 additions shows


def test_group_means_refusals_come_before_any_launch():
    import torch

    ctx = gpu_context()
    cube = dev(dc.cube_u16(10, 4, 16, 5))
    stack = torch.full((2, 3, 4, 12), -1.0, device="cuda")
    torch.cuda.synchronize()

    def call(reads, ng=None, nreads=10, nx=12, width=16, cap=3, j=0, y0=0, ny=4):
        r = np.array(reads, np.int32)
        return ctx.lib.rip_cal_group_means(ctx.h, cube.ctypes.data, _native.RIP_DEVICE, nreads, 4, width, y0, ny, nx, r.ctypes.data,
                                           len(reads) // 2 if ng is None else ng, 0, stack.data_ptr(), cap, j)

    bad = [dict(reads=[0, 2, 3, 3]), dict(reads=[0, 2, 5, 4]),            # an empty group
           dict(reads=[0, 2, 8, 11]), dict(reads=[-1, 2, 3, 4]),          # beyond the cube
           dict(reads=[0, 2, 3, 4], j=3), dict(reads=[0, 2, 3, 4], j=-1),  # no such slot
           dict(reads=[0, 2, 3, 4], nx=17),                                # wider than the frame
           dict(reads=[0, 2, 3, 4], ng=0), dict(reads=[0, 1] * 65),        # group counts
           dict(reads=[0, 2, 3, 4], y0=2, ny=3)]                           # rows beyond the frame
    for kw in bad:
        assert call(**kw) == -1, kw
        assert ctx.lib.rip_last_error(ctx.h)
    assert bool((stack == -1).all()), "a refused call wrote to the stack"
    assert call([0, 2, 3, 4], j=2) == 0
    got = stack.cpu().numpy()
    assert np.all(got[:, :2] == -1) and np.all(got[:, 2] >= 0)
    st = calfiles.DarkStack([0, 2], 4, 12, 2, ctx=ctx)
    with pytest.raises(TypeError):
        st.add(np.zeros((3, 4, 16), np.int16))              # signed samples are FITS storage or nothing
    with pytest.raises(TypeError):
        st.add(np.zeros((3, 4, 16), np.float32))
    with pytest.raises(ValueError):
        st.add(np.zeros((3, 5, 16), np.uint16))
    with pytest.raises(ValueError):
        st.finish()
    with pytest.raises(MemoryError, match=r"needs \d+ bytes and \d+ bytes"):
        calfiles.DarkStack([0, 1] * 8, 65536, 4096, 512, ctx=ctx)
    with pytest.raises(ValueError):
        calfiles.DarkStack([0, 1], 4, 4, 513, ctx=ctx)


# ------------------------------------------------------------------------------------------------ DarkStack end to end
def test_darkstack_end_to_end_and_row_bands():
    """5 exposures of 20 x 36 x 70, cropped to 64 columns; at 3 sigma five values cannot lose one, at 1.5 sigma they do"""
    cubes = dc.dark_exposures()
    nx = 64
    ref_stack = np.stack([dr.group_means(c, dc.READS_E2E, nx) for c in cubes], axis=1)
    st = stack_of(cubes, dc.READS_E2E, 36, nx, 5)
    assert_same_bits(st.stack.numpy(), ref_stack, "the stack")
    full = {}
    for sigma in (3, 1.5):
        mean, count = st.finish(sigma=sigma, want_count=True)
        assert isinstance(mean, np.ndarray) and mean.shape == (5, 36, nx)
        for g in range(5):
            rm, rc, _ = dr.sigma_clip_mean(ref_stack[g], sigma=sigma)
            assert_same_bits(count[g], rc, f"group {g} count at {sigma} sigma")
            assert_same_bits(mean[g], rm, f"group {g} mean at {sigma} sigma")
        assert_same_bits(st.finish(sigma=sigma), mean)
        full[sigma] = mean
    assert np.all(st.finish(want_count=True)[1] == 5)
    # a band of rows, from host arrays and from device arrays, in a stack with room to spare
    for on_device in (False, True):
        band = stack_of(cubes, dc.READS_E2E, 36, nx, 7, on_device=on_device, rows=(9, 30))
        got = band.finish(sigma=1.5)
        assert isinstance(got, DevArray if on_device else np.ndarray) and got.shape == (5, 21, nx)
        assert_same_bits(got.numpy() if on_device else got, full[1.5][:, 9:30], f"rows 9..29, device arrays: {on_device}")


# ------------------------------------------------------------------------------------------------ the three planes
def test_dark_planes():
    rng = np.random.default_rng(9)
    ny, width, nside = 9, 75, 70
    d1, d2, e1, e2, cds = ((300 * rng.random((ny, width))).astype(F) for _ in range(5))
    d2[0, :4] = [200.0, np.nextafter(F(200), F(0)), np.nextafter(F(200), F(999)), np.nan]   # on, below and above the limit
    d2[1, 69], d2[1, 70] = 250.0, 250.0                                                    # the last column kept, the first dropped
    cds[2, :3] = [0.0, np.inf, np.nan]
    want = dr.dark_planes(d1, d2, e1, e2, cds, nside)
    assert want[0][0, 0] == 200 and want[0][0, 2] == d1[0, 2] and np.isnan(want[0][0, 3])
    got = calfiles.derive_dark_planes(d1, d2, e1, e2, cds, nside=nside, ctx=gpu_context())
    dgot = calfiles.derive_dark_planes(*(dev(a) for a in (d1, d2, e1, e2, cds)), nside=nside, ctx=gpu_context())
    for g, dg, w, what in zip(got, dgot, want, ("dark_slope", "dark_slope_err", "read_noise")):
        assert g.shape == (ny, nside)
        assert_same_bits(g, w, what)
        assert_same_bits(dg.numpy(), w, what + " (device arrays)")
    full = calfiles.derive_dark_planes(d1, d2, e1, e2, cds, ctx=gpu_context())
    assert_same_bits(full[2], dr.dark_planes(d1, d2, e1, e2, cds, width)[2], "no crop")
    with pytest.raises(TypeError):
        calfiles.derive_dark_planes(d1.astype(np.float64), d2, e1, e2, cds, ctx=gpu_context())
    with pytest.raises(TypeError):
        calfiles.derive_dark_planes(d1.astype(">f4"), d2, e1, e2, cds, ctx=gpu_context())


# ------------------------------------------------------------------------------------------------ the drop-in
@pytest.mark.parametrize("with_amp33", [True, False])
def test_make_dark_file_module(tmp_path, monkeypatch, with_amp33):
    """three darks of 35 x 44 x 144 (the frame of tests/calfiles_cases.py and a 4-column reference output), the production table,
    nside = 140; the summary with and without its AMP33 extension"""
    rng = np.random.default_rng(21)
    ny, width, nside, reads = cc.NY, cc.NX + 4, cc.NX, cc.READS_PROD
    cubes = [c for c in dc.dark_exposures(3, 35, ny, width, seed=70)]
    for j, c in enumerate(cubes):
        dc.write_dark_fits(tmp_path / f"dark_{j + 1:03d}.fits", c)
    planes = (300 * rng.random((7, ny, width))).astype(F)
    keys = [("DARK1", 3), ("DARK1ERR", 4), ("DARK2", 1), ("DARK2ERR", 2), ("CDS", 0), ("RESET", 6), ("ACN", 1.25), ("C_PINK", 2.5),
            ("U_PINK", 0.75), ("EXTNAME", "NOISE")]
    a33 = rng.random((2, ny, 8)).astype(F)
    with open(tmp_path / "summary.fits", "wb") as f:
        f.write(dc.fits_hdu(None))
        f.write(dc.fits_hdu(planes, keys, extension=True))
        if with_amp33:
            f.write(dc.fits_hdu(a33, [("EXTNAME", "AMP33"), ("M_PINK", 1.5), ("RU_PINK", 0.125)], extension=True))
    with open(tmp_path / "settings_prod.yaml", "w") as f:
        yaml.safe_dump({"READS": reads}, f)
    monkeypatch.chdir(tmp_path)
    out = str(tmp_path / "cal_dark_X.asdf")
    with contextlib.redirect_stdout(io.StringIO()) as text:
        files = make_dark_file.run("prod", str(tmp_path / "dark_001.fits"), str(tmp_path / "summary.fits"), 7, out, nside=nside,
                                   ctx=gpu_context())
    assert files == (out, str(tmp_path / "cal_read_X.asdf")) and all(os.path.exists(p) for p in files)
    assert "Read pattern: [[0], [1], [2, 3]," in text.getvalue() and "dark_003.fits" in text.getvalue()
    dark, read = calio.roman_branch(files[0]), calio.roman_branch(files[1])
    assert set(dark) == {"meta", "data", "dq", "dark_slope", "dark_slope_err"}
    assert set(read) == {"meta", "data", "resetnoise", "anc", "amp33"}
    assert dark["meta"]["reftype"] == "DARK" and read["meta"]["reftype"] == "READNOISE"
    assert dark["meta"]["exposure"]["ngroups"] == 8 and dark["meta"]["exposure"]["ma_table_name"] == "prod"
    assert dark["meta"]["instrument"]["detector"] == "WFI07"
    ref_stack = np.stack([dr.group_means(c, reads, nside) for c in cubes], axis=1)
    want = np.stack([dr.sigma_clip_mean(ref_stack[g])[0] for g in range(8)])
    assert_same_bits(dark["data"], want, "dark data")
    assert dark["dq"].dtype == np.uint32 and dark["dq"].shape == (nside, nside) and not dark["dq"].any()
    slope, slope_err, rn = dr.dark_planes(planes[3], planes[1], planes[4], planes[2], planes[0], nside)
    assert_same_bits(dark["dark_slope"], slope, "dark_slope")
    assert_same_bits(dark["dark_slope_err"], slope_err, "dark_slope_err")
    assert_same_bits(read["data"], rn, "read noise")
    assert_same_bits(read["resetnoise"], planes[6][:, :nside], "reset noise")
    assert read["anc"] == {"ACN": 1.25, "C_PINK": 2.5, "U_PINK": 0.75, "UNIT": "DN"}
    if with_amp33:
        assert read["amp33"]["valid"] is True and read["amp33"]["M_PINK"] == 1.5 and read["amp33"]["RU_PINK"] == 0.125
        assert_same_bits(read["amp33"]["med"], a33[0])
        assert_same_bits(read["amp33"]["std"], a33[1])
    else:
        assert read["amp33"]["valid"] is False and read["amp33"]["M_PINK"] == 0.0 and read["amp33"]["RU_PINK"] == 0.0
        assert read["amp33"]["med"].shape == (4096, 128) and not read["amp33"]["med"].any() and not read["amp33"]["std"].any()
    with calio.open_tree(files[0]) as t:
        assert "DARK1ERR=" in t["notes"]["noise_header"]
    # row bands give the same file contents, and the dark data feed the bias correction
    banded = make_dark_file.dark_data([str(tmp_path / f"dark_{j:03d}.fits") for j in (1, 2, 3)], reads, nside=nside, band_rows=17,
                                      ctx=gpu_context())
    assert_same_bits(banded, want, "bands of 17 rows")
    a = cc.inputs("calfiles_p9_prod")
    bc, t0 = calfiles.derive_biascorr(a["dark_slope"], dark["data"], a["lin_data"], a["Smin"], a["Smax"], reads, ctx=gpu_context())
    assert bc.shape == (8, ny - 8, nside - 8) and bc.dtype == F and t0 == 3.04
