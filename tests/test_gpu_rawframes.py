"""Raw detector frames to exposure cubes and slope images on the device (csrc/rawframes.hip, romanimpreprocess_amd/calfiles/
convert_frames.py and the drop-ins convert_dark / convert_flt / convert_loflt) against tests/rawframes_ref.py, which tests/
test_host_rawframes_ref.py holds against the reference's own lines.  Every comparison is bit for bit (NaN as NaN)."""

import contextlib
import datetime
import io
import os

import darkstack_cases as dc
import darkstack_ref as dr
import numpy as np
import pytest
import rawframes_ref as rr
from conftest import assert_same_bits, gpu_context

from romanimpreprocess_amd import _native, calfiles, calio
from romanimpreprocess_amd.calfiles import convert_dark, convert_flt, convert_frames, convert_loflt, make_dark_file
from romanimpreprocess_amd.devarray import DevArray

pytestmark = pytest.mark.gpu

HOST, DEVICE = _native.RIP_HOST, _native.RIP_DEVICE
NOW = datetime.datetime(2025, 8, 9, 10, 11, 12)


def words(a):
    """any 16-bit array as native int16 words (what a torch tensor carries)"""
    return np.ascontiguousarray(a).view(np.uint16).view(np.int16)


# ------------------------------------------------------------------------------------------------ the frame kernel
def run_frame(stored_frame, orient, nflip, stored, where):
    """rip_cal_raw_frame on a frame given as stored, from a host array, a device array, or a device array that starts one
    sample behind a 16-byte boundary; the plane it wrote"""
    import torch

    ctx = gpu_context()
    ny, nx = stored_frame.shape
    dst = torch.full((ny * nx,), -21846, dtype=torch.int16, device="cuda")   # 0xAAAA
    if where == "host":
        src, loc, keep = np.ascontiguousarray(stored_frame).view(np.uint16), HOST, None
    else:
        off = 1 if where == "offset" else 0
        keep = torch.zeros(ny * nx + 8, dtype=torch.int16, device="cuda")
        keep[off:off + ny * nx] = torch.from_numpy(words(stored_frame).reshape(-1)).cuda()
        assert keep.data_ptr() % 16 == 0
        src, loc = keep.data_ptr() + 2 * off, DEVICE
    torch.cuda.synchronize()
    ctx.call("rip_cal_raw_frame", src, loc, ny, nx, orient, nflip, stored, DevArray(dst, np.uint16))
    return dst.cpu().numpy().view(np.uint16).reshape(ny, nx)


@pytest.mark.parametrize("ny, nx, nflip", rr.FRAME_SHAPES)
def test_frame_kernel(ny, nx, nflip):
    """every orientation and every stored form, the five edge samples present, from a host frame, a device frame (the wide form
    where the shape allows it) and a device frame one sample off a 16-byte boundary (the narrow form on the same shape)"""
    samples = rr.frame_samples(ny, nx)
    assert all(v in samples for v in rr.EDGE_SAMPLES)
    for orient in (0, 1, 2):
        want = rr.orient_frame(samples, orient, nflip)
        if ny > 1 and ny % 2 and orient == 2:
            assert_same_bits(want[ny // 2], samples[ny // 2], "the middle row stays")
        for stored in rr.STORED:
            frame = rr.encode(samples, stored)
            got = {where: run_frame(frame, orient, nflip, stored, where) for where in ("host", "device", "offset")}
            for where, g in got.items():
                assert_same_bits(g, want, f"({ny},{nx},{nflip}) orient {orient} stored {stored} {where}")
            assert_same_bits(got["device"], got["offset"], "wide against narrow")


def test_frame_refusals_come_before_any_launch():
    import torch

    ctx = gpu_context()
    ny, nx = 4, 16
    n = ny * nx
    buf = torch.full((4 * n,), 7, dtype=torch.int16, device="cuda")
    host = np.zeros((ny + 1, nx), np.uint16)
    torch.cuda.synchronize()
    src, dst = buf.data_ptr(), buf.data_ptr() + 2 * 2 * n

    def call(frame=src, location=DEVICE, ny=ny, nx=nx, orient=1, nflip=8, stored=1, dst=dst):
        return ctx.lib.rip_cal_raw_frame(ctx.h, frame, location, ny, nx, orient, nflip, stored, dst)

    bad = [dict(ny=0), dict(nx=0), dict(ny=-1), dict(nx=-4),                      # a non-positive size
           dict(nflip=-1), dict(nflip=nx + 1),                                    # nflip outside 0..nx
           dict(orient=3), dict(orient=-1), dict(stored=3), dict(stored=-1),      # unknown codes
           dict(location=2), dict(location=-1),
           dict(frame=None), dict(dst=None),                                      # NULL pointers
           dict(frame=host.ctypes.data, location=HOST, dst=None),
           dict(dst=dst + 1), dict(frame=src + 1),                                # not aligned to the sample
           dict(dst=src), dict(dst=src + 2 * (n - 1)), dict(frame=src + 2 * n, dst=src + 2)]   # dst overlapping frame
    for kw in bad:
        assert call(**kw) == _native.RIP_EINVAL, kw
        assert ctx.lib.rip_last_error(ctx.h)
    assert bool((buf == 7).all()), "a refused call wrote"
    assert call(dst=src + 2 * n) == 0 and call(nflip=0) == 0 and call(nflip=nx) == 0   # adjacent is not overlapping
    assert call(frame=host.ctypes.data + 1, location=HOST) == 0                        # a host frame needs no alignment
    with pytest.raises(ValueError, match="nflip"):
        ctx.call("rip_cal_raw_frame", host, HOST, ny, nx, 1, nx + 8, 0, dst)


# ------------------------------------------------------------------------------------------------ the slopes kernel
@pytest.mark.parametrize("N", rr.SLOPE_N)
def test_slopes(N):
    """Nc = N (convert_dark) and Nc = min(N, 10) (the flats); 1, 7, 8 and 64 * 8 + 3 pixels (the wide form, the narrow form, more
    than one wave); random, all 65535, all 0, 65535 under the largest weight only; the NaN table of small frame counts"""
    ctx = gpu_context()
    for Nc in sorted({N, min(N, 10)}):
        nan0, nan1 = rr.nan_table(Nc)
        for npix in rr.SLOPE_NPIX:
            for name, cube in rr.slope_cubes(N, npix, Nc).items():
                want = rr.slopes(cube, Nc)
                got = convert_frames.cube_slopes(cube, Nc, ctx=ctx)
                assert isinstance(got, DevArray) and got.shape == (2, 1, npix) and got.dtype == np.float32
                got = got.numpy()
                assert_same_bits(got, want, f"N {N} Nc {Nc} npix {npix} {name}")
                assert not np.isinf(got).any()
                assert np.isnan(got[0]).all() == nan0 and np.isnan(got[1]).all() == nan1
                assert nan0 or np.isfinite(got[0]).all()
                assert nan1 or np.isfinite(got[1]).all()


def test_slopes_forms_agree_host_output_and_real_row():
    """8448 pixels (two real rows), 13 frames: the wide form, the narrow form on the same cube placed one sample off a 16-byte
    boundary, a (N, ny, nx) DevArray, and the host output of the raw entry"""
    import torch

    ctx = gpu_context()
    N, Nc, ny, nx = 13, 10, 2, 4224
    npix = ny * nx
    cube = np.random.default_rng(77).integers(0, 65536, (1, N, ny, nx)).astype(np.uint16)
    want = rr.slopes(cube, Nc)
    wide = convert_frames.cube_slopes(cube, Nc, ctx=ctx).numpy()
    assert_same_bits(wide, want, "wide")
    dev3 = DevArray(torch.from_numpy(words(cube[0])).cuda(), np.uint16)
    assert_same_bits(convert_frames.cube_slopes(dev3, Nc, ctx=ctx).numpy(), want, "a (N, ny, nx) DevArray")
    off = torch.zeros(N * npix + 8, dtype=torch.int16, device="cuda")
    off[1:1 + N * npix] = torch.from_numpy(words(cube).reshape(-1)).cuda()
    torch.cuda.synchronize()
    w0, de0, w1, de1 = convert_frames.slope_weights(Nc)
    narrow = np.empty((2, ny, nx), np.float32)
    ctx.call("rip_cal_frame_slopes", off.data_ptr() + 2, N, Nc, npix, w0, de0, w1, de1, narrow, HOST)
    assert_same_bits(narrow, wide, "narrow form, host output, against the wide form")
    with pytest.raises(TypeError):
        convert_frames.cube_slopes(cube.astype(np.int16), Nc, ctx=ctx)
    with pytest.raises(ValueError):
        convert_frames.cube_slopes(cube, N + 1, ctx=ctx)


@pytest.mark.parametrize("ny, nx", [(6, 16), (5, 12)])
def test_slopes_host_and_device_outputs_are_the_same_bits(ny, nx):
    """out_location RIP_HOST against RIP_DEVICE on one cube: 96 pixels (a multiple of 8: the wide form where the pointers allow
    it) and 60 (the narrow form), the device slopes on a 16-byte boundary and one float behind it"""
    import torch

    ctx = gpu_context()
    N, Nc, npix = 7, 5, ny * nx
    cube = np.random.default_rng(ny * nx).integers(0, 65536, (1, N, ny, nx)).astype(np.uint16)
    want = rr.slopes(cube, Nc).reshape(2, npix)
    dcube = torch.from_numpy(words(cube).reshape(-1)).cuda()
    w0, de0, w1, de1 = convert_frames.slope_weights(Nc)
    host = np.full((2, npix), 7, np.float32)
    ctx.call("rip_cal_frame_slopes", dcube.data_ptr(), N, Nc, npix, w0, de0, w1, de1, host, HOST)
    assert_same_bits(host, want, "host output")
    for off in (0, 1):
        dev = torch.full((2 * npix + 4,), 7.0, dtype=torch.float32, device="cuda")
        assert dev.data_ptr() % 16 == 0
        torch.cuda.synchronize()
        ctx.call("rip_cal_frame_slopes", dcube.data_ptr(), N, Nc, npix, w0, de0, w1, de1, dev.data_ptr() + 4 * off, DEVICE)
        got = dev.cpu().numpy()
        assert_same_bits(got[off:off + 2 * npix].reshape(2, npix), host, f"device output {off} floats off the boundary against the host output")
        assert np.all(got[:off] == 7) and np.all(got[off + 2 * npix:] == 7), "written outside the slopes"


def test_slopes_refusals_come_before_any_launch():
    import torch

    ctx = gpu_context()
    n, npix = 6, 24
    cube = torch.full((n * npix,), 9, dtype=torch.int16, device="cuda")
    slp = torch.full((2 * npix + 4,), -5.0, dtype=torch.float32, device="cuda")
    w0, de0, w1, de1 = convert_frames.slope_weights(n)
    torch.cuda.synchronize()
    cp, sp, p0, p1 = cube.data_ptr(), slp.data_ptr(), w0.ctypes.data, w1.ctypes.data

    def call(cube=cp, n=n, nc=n, npix=npix, w0=p0, w1=p1, slp=sp, loc=DEVICE):
        return ctx.lib.rip_cal_frame_slopes(ctx.h, cube, n, nc, npix, w0, de0, w1, de1, slp, loc)

    bad = [dict(n=0), dict(n=-2), dict(npix=0),                                # a non-positive size
           dict(nc=0), dict(nc=n + 1), dict(nc=-1),                            # nc outside 1..n
           dict(cube=None), dict(w0=None), dict(w1=None), dict(slp=None),      # NULL pointers
           dict(loc=5), dict(loc=-1),
           dict(cube=cp + 1), dict(slp=sp + 2), dict(slp=sp + 1),              # not aligned to the sample
           dict(slp=cp), dict(slp=cp + 4 * npix)]                              # slp overlapping the cube
    for kw in bad:
        assert call(**kw) == _native.RIP_EINVAL, kw
        assert ctx.lib.rip_last_error(ctx.h)
    assert bool((slp == -5.0).all()) and bool((cube == 9).all()), "a refused call wrote"
    assert call() == 0
    got = slp.cpu().numpy()
    assert np.all(got[:2 * npix] != -5.0) and np.all(got[2 * npix:] == -5.0)


# ------------------------------------------------------------------------------------------------ end to end
NY, NX, NFLIP = 12, 32, 24
KIND = {"dark": ("Total_Noise_exp", "Noise", "convert_dark.py", 7, convert_dark),
        "flt": ("linearity_exp", "Flat", "convert_flt.py", 11, convert_flt),
        "loflt": ("Gain_exp", "LoFlat", "convert_loflt.py", 11, convert_loflt)}


def write_frame(path, samples, date, as_int16=False):
    """one frame file: uint16 samples (BITPIX 16, BZERO 32768) or, as_int16, the same bits as int16 without BZERO"""
    data = samples.view(np.int16) if as_int16 else samples
    calio.write_fits(path, [{"data": np.ascontiguousarray(data), "cards": [("DATE", date)]}], ctx=gpu_context())


def make_exposures(indir, prefix, sca, N, seed):
    """exposure 1: N + 1 frames (the last is not used) and a guide-window file; exposure 2: one frame short; exposure 3: N frames,
    one of them stored as int16 without BZERO; another detector's frames beside them.  Returns j -> (names, frames, dates)."""
    out = {}
    for j, count in ((1, N + 1), (2, N - 1), (3, N)):
        names, frames, dates = [], [], []
        for k in range(count):
            name = f"{prefix}{j}_run_SCU{sca:02d}_{k:03X}.fits"
            f = rr.frame_samples(NY, NX, seed=100 * j + k + seed)
            date = f"2025-07-{j:02d}T00:{k:02d}:00"
            write_frame(os.path.join(indir, name), f, date, as_int16=(j == 3 and k == 2))
            names.append(name), frames.append(f), dates.append(date)
        out[j] = (names, frames, dates)
    write_frame(os.path.join(indir, f"{prefix}1_run_SCU{sca:02d}_000_gw.fits"), rr.frame_samples(NY, NX, seed=5), "x")
    write_frame(os.path.join(indir, f"{prefix}1_run_SCU{sca + 1:02d}_000.fits"), rr.frame_samples(NY, NX, seed=6), "x")
    return out


@pytest.mark.parametrize("sca", [3, 4])
@pytest.mark.parametrize("kind", list(KIND))
def test_convert_end_to_end(tmp_path, kind, sca):
    prefix, outname, proven, N, module = KIND[kind]
    indir, outdir = tmp_path / "in", tmp_path / "out"
    indir.mkdir(), outdir.mkdir()
    made = make_exposures(str(indir), prefix, sca, N, seed=sca)
    with contextlib.redirect_stdout(io.StringIO()) as text:
        files = module.run(str(indir), N, str(outdir), sca, exposures=(1, 2, 3), nflip=NFLIP, now=NOW, ctx=gpu_context())
    assert files == [f"{outdir}/99999999_SCA{sca:02d}_{outname}_{j:03d}.fits" for j in (1, 3)]
    assert sorted(os.listdir(outdir)) == [os.path.basename(f) for f in files]      # the short exposure is skipped
    said = text.getvalue()
    assert f"Looking for files in {indir}/{prefix}2_" in said and f"could not complete SCU{sca:02d}, continuing ..." in said
    assert f"SCU{sca:02d}, found {N + 1:3d} files" in said and f">> {files[0]}" in said and "_gw.fits" not in said
    for j, path in zip((1, 3), files):
        names, frames, dates = made[j]
        want_cube, want_slp = rr.exposure(frames[:N], sca, NFLIP, kind)
        h0, d0 = calio.read_fits_image(path, 0)
        h1, d1 = calio.read_fits_image(path, 1)
        h2, d2 = calio.read_fits_image(path, 2)
        assert d0 is None and h0["TGROUP"] == 3.04 and h0["NAXIS"] == 0
        assert h1["BITPIX"] == 16 and h1["BZERO"] == 32768 and d1.shape == (1, N, NY, NX)
        assert_same_bits(rr.decode(np.array(d1), 1), want_cube, f"{kind} sca {sca} exposure {j}: cube")
        assert h2["BITPIX"] == -32 and h2["BUNIT"] == "DN/frame"
        assert_same_bits(np.array(d2).astype(np.float32), want_slp, f"{kind} sca {sca} exposure {j}: slopes")
        assert np.isfinite(want_slp).all()
        cards = [("PROVEN", proven), ("NMAX", N), ("DATE", "2025-08-09 10:11:12")]
        for k in range(N):
            cards += [(f"FR{k + 1:03d}", names[k]), (f"FRD{k + 1:03d}", dates[k])]
        assert list(h1)[-len(cards):] == [k for k, _ in cards]
        assert [h1[k] for k, _ in cards] == [v for _, v in cards]


def test_frames_to_cube_refusals(tmp_path, monkeypatch):
    import torch

    ctx = gpu_context()
    good = rr.frame_samples(NY, NX)
    write_frame(tmp_path / "a_0.fits", good, "d0")
    write_frame(tmp_path / "a_1.fits", rr.frame_samples(NY + 1, NX), "d1")
    calio.write_fits(tmp_path / "a_2.fits", [{"data": good.astype(np.float32), "cards": [("DATE", "d2")]}], ctx=ctx)
    calio.write_fits(tmp_path / "a_3.fits", [{"data": good.astype(np.uint32), "cards": [("DATE", "d3")]}], ctx=ctx)
    cube, dates = calfiles.frames_to_cube([tmp_path / "a_0.fits"] * 2, 4, nflip=NFLIP, ctx=ctx)
    assert dates == ["d0", "d0"] and cube.shape == (1, 2, NY, NX) and cube.dtype == np.uint16
    assert_same_bits(cube.numpy()[0, 1], good[::-1])
    with pytest.raises(ValueError, match=r"a_1\.fits: a frame of 13 x 32"):
        calfiles.frames_to_cube([tmp_path / "a_0.fits", tmp_path / "a_1.fits"], 4, nflip=NFLIP, ctx=ctx)
    with pytest.raises(ValueError, match=r"a_2\.fits.*BITPIX -32, BZERO None"):
        calfiles.frames_to_cube([tmp_path / "a_0.fits", tmp_path / "a_2.fits"], 4, nflip=NFLIP, ctx=ctx)
    with pytest.raises(ValueError, match=r"a_3\.fits.*BITPIX 32, BZERO 2147483648"):
        calfiles.frames_to_cube([tmp_path / "a_3.fits"], 4, nflip=NFLIP, ctx=ctx)
    with pytest.raises(ValueError, match="nflip"):
        calfiles.frames_to_cube([tmp_path / "a_0.fits"], 3, ctx=ctx)   # the default 4096 columns of a 32-column frame
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (1000, 1 << 30))   # 1000 bytes free
    with pytest.raises(MemoryError, match=rf"needs {2 * 3 * NY * NX} bytes and 1000 bytes"):
        calfiles.frames_to_cube([tmp_path / "a_0.fits"] * 2, 4, nflip=NFLIP, ctx=ctx)


# ------------------------------------------------------------------------------------------------ hand-off to the dark file
def test_cubes_go_to_the_dark_stack_from_files_and_from_hbm(tmp_path):
    """three dark exposures of 7 frames: the group means that make_dark_file.dark_data makes from the written summer2025 files,
    from the DevArray cubes directly, and by tests/darkstack_ref.py from the restated cubes"""
    ctx = gpu_context()
    sca, N, nside, reads = 4, 7, NFLIP, [0, 1, 1, 3, 3, 7]
    indir, outdir = tmp_path / "in", tmp_path / "out"
    indir.mkdir(), outdir.mkdir()
    exposures = dc.dark_exposures(3, N, NY, NX, seed=91)
    for j, c in enumerate(exposures):
        for k in range(N):
            write_frame(indir / f"Total_Noise_exp{j + 1}_d_SCU{sca:02d}_{k:03X}.fits", c[k], f"t{j}{k}")
    with contextlib.redirect_stdout(io.StringIO()):
        files = calfiles.convert("dark", indir, N, outdir, sca, exposures=range(1, 4), nflip=NFLIP, now=NOW, ctx=ctx)
        assert len(files) == 3
        from_files = make_dark_file.dark_data(files, reads, nside=nside, ctx=ctx, layout="summer2025")
        cubes = [calfiles.frames_to_cube(convert_frames.find_frames(indir, "Total_Noise_exp", j, sca), sca, nflip=NFLIP, ctx=ctx)[0]
                 for j in (1, 2, 3)]
        from_hbm = make_dark_file.dark_data(cubes, reads, nside=nside, ctx=ctx)
        banded = make_dark_file.dark_data(cubes, reads, nside=nside, band_rows=5, ctx=ctx)
    ref_cubes = [rr.exposure(list(c), sca, NFLIP, "dark")[0][0] for c in exposures]
    for c, r in zip(cubes, ref_cubes):
        assert_same_bits(c.numpy()[0], r)
    stack = np.stack([dr.group_means(r, reads, nside) for r in ref_cubes], axis=1)
    clipped = [dr.sigma_clip_mean(stack[g]) for g in range(len(reads) // 2)]
    assert not any(b.any() for _, _, b in clipped), "a borderline pixel: the comparison needs another seed"
    want = np.stack([m for m, _, _ in clipped])
    assert from_files.shape == (3, NY, nside)
    assert_same_bits(from_files, want, "from the summer2025 files")
    assert_same_bits(from_hbm, want, "from the cubes in HBM")
    assert_same_bits(banded, want, "from the cubes in HBM, in row bands")
    with pytest.raises(ValueError, match="layout"):
        make_dark_file.dark_data(files, reads, nside=nside, ctx=ctx, layout="winter")
    with pytest.raises(ValueError):   # the primary HDU of such a file holds no cube
        make_dark_file.dark_data(files, reads, nside=nside, ctx=ctx)
