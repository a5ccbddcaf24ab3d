"""GPU: rip_fpa_bin and rip_fpa_render against tests/fpaplot_ref.py (the float64 numpy restatement) and against the fixture that
the reference's own utils/fpaplot.py produced, and the public surface of romanimpreprocess_amd.utils.fpaplot on top of them.

Device means against the restatement: |delta| <= s^2 * 2^-53 * sum|v| / count per bin, the worst case of a float64 sum of s^2
terms in any order (derived, not measured; fpaplot_ref.bin_ref returns it).  The picture is then equal byte for byte except where
the restatement's x * 256 lies within 1e-9 of an integer, which must be below 0.1 % of the SCA pixels.  Against the fixture the
conditions are those of tests/test_host_fpaplot.py (fpaplot_ref.assert_picture, fpaplot_ref.reference_bound)."""

import json
import os
import subprocess
import sys

import fpaplot_ref as fr
import numpy as np
import pytest
from conftest import REPO, gpu_context, load_golden

pytestmark = pytest.mark.gpu

PTYPES = [p[0] for p in fr.PANELS]


def fp():
    from romanimpreprocess_amd.utils import fpaplot
    return fpaplot


@pytest.fixture(scope="module")
def g():
    return load_golden("fpaplot_small")


def check_bin(dq, grow, planes, nside, n1, what=""):
    """device means of these host arrays against the restatement, within the derived bound; returns them"""
    got = fp().bin_planes(dq, planes, nside, n1, mask=grow, ctx=gpu_context()).numpy()
    want, bound = fr.bin_ref(dq, grow, planes, nside, n1)
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: empty bins differ"
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), f"{what}: infinite means differ"
    ok = np.isfinite(want)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)[ok]
    print(f"{what}: largest |delta| / bound = {np.max(err / np.maximum(bound[ok], 1e-300)) if err.size else 0:.3g}")
    assert (err <= bound[ok]).all(), f"{what}: {np.count_nonzero(err > bound[ok])} means outside the bound"
    return got


def mixed_planes(rng, nside):
    """8 planes: float32 and float64, sides nside and nside - 8 (pad 4), values of both signs"""
    return [(rng.standard_normal((m, m)) * 10 ** rng.uniform(-3, 3)).astype(dt)
            for m, dt in [(nside, np.float32), (nside - 8, np.float64), (nside, np.float64), (nside - 8, np.float32)] * 2]


# ---------------------------------------------------------------------------------------------- bin sizes and plane types
@pytest.mark.parametrize("n1", [64, 16, 2, 1])
def test_bin_sizes(n1):
    rng = np.random.default_rng(100 + n1)
    check_bin(fr.random_dq(rng, 64, 0.1), fr.PIXELMASK1, mixed_planes(rng, 64), 64, n1, f"nside 64 n1 {n1}")


def test_production_block_on_a_small_frame():
    rng = np.random.default_rng(7)
    check_bin(fr.random_dq(rng, 256), fr.PIXELMASK1, mixed_planes(rng, 256)[:3], 256, 8, "nside 256 n1 8")


def test_one_plane_and_a_frame_that_is_no_multiple_of_the_tile():
    rng = np.random.default_rng(8)
    for nside, n1 in ((64, 16), (96, 32), (80, 16), (72, 2)):   # s = 4, 3, 5, 36: tiles of 32 x 64 cut the bins anywhere
        check_bin(fr.random_dq(rng, nside, 0.1), fr.PIXELMASK1, [rng.standard_normal((nside - 2, nside - 2)).astype(np.float32)],
                  nside, n1, f"nside {nside} n1 {n1}")


def test_production_index_widths():
    """nside 4096, n1 128, one float32 plane; inputs and reference made with torch on the device"""
    import torch

    from romanimpreprocess_amd.devarray import DevArray
    dev = torch.device("cuda", 0)
    nside, n1, s = 4096, 128, 32
    idx = torch.arange(nside * nside, device=dev, dtype=torch.int64)
    plane = ((idx % 1000003).to(torch.float32) * 1e-3 - 300.0).reshape(nside, nside).contiguous()
    flag1, flag25 = (idx % 9973 == 0).reshape(nside, nside), (idx % 99991 == 17).reshape(nside, nside)
    flag1[-1, -1], flag25[0, 0], flag25[-1, 0] = True, True, True
    dq = (flag1.to(torch.int32) | (flag25.to(torch.int32) << 3)).contiguous()
    grow = np.zeros(32, np.uint8)
    grow[0], grow[3] = 1, 25
    got = fp().bin_planes(DevArray(dq, np.uint32).sync(), [DevArray(plane)], nside, n1, mask=grow, ctx=gpu_context()).t
    masked = flag1 | (torch.nn.functional.max_pool2d(flag25[None, None].to(torch.float32), 5, stride=1, padding=2)[0, 0] > 0)
    v = torch.where(masked, torch.zeros((), device=dev, dtype=torch.float64), plane.to(torch.float64))
    blocks = lambda a: a.reshape(n1, s, n1, s)   # noqa: E731
    count = blocks(~masked).sum(dim=(1, 3))
    want = blocks(v).sum(dim=(1, 3)) / count
    bound = s * s * 2.0**-53 * blocks(v.abs()).sum(dim=(1, 3)) / count
    assert int(count.min()) > 0 and int(count.min()) < s * s
    assert bool(((got[0] - want).abs() <= bound).all())


# ---------------------------------------------------------------------------------------------- mask growth across seams
@pytest.mark.parametrize("growth", [1, 5, 9, 25])
def test_single_flagged_pixel_at_bin_and_tile_corners(growth):
    grow = np.zeros(32, np.uint8)
    grow[11] = growth
    plane = np.arange(128 * 128, dtype=np.float64).reshape(128, 128) + 1.0
    for y, x in ((32, 64), (31, 63), (31, 64), (32, 63), (64, 64), (4, 4), (3, 3)):   # tile seams at rows 32 k, column 64; bins of 4
        dq = np.zeros((128, 128), np.uint32)
        dq[y, x] = 1 << 11
        got = check_bin(dq, grow, [plane], 128, 32, f"growth {growth} at ({y}, {x})")
        clean = fr.bin_ref(None, grow, [plane], 128, 32)[0]
        assert np.count_nonzero(got != clean) == {1: 1, 5: 3, 9: 4, 25: 4}[growth]   # a bin corner: the growth reaches the neighbours


def test_flags_in_the_corners_and_edge_rows_and_no_dq():
    rng = np.random.default_rng(9)
    planes = mixed_planes(rng, 64)[:2]
    dq = np.zeros((64, 64), np.uint32)
    dq[0, 0] = dq[0, -1] = dq[-1, 0] = dq[-1, -1] = 1 << 3   # growth 25
    dq[0, 20:30] = 1 << 10                                  # growth 9
    dq[-1, 5], dq[17, 0], dq[40, -1] = 1 << 2, 1 << 2, 1 << 6   # growth 5
    dq[30, 30] = 1 << 1                                     # a bit PixelMask1 ignores
    for n1 in (64, 16):
        check_bin(dq, fr.PIXELMASK1, planes, 64, n1, f"edges n1 {n1}")
        got = check_bin(None, fr.PIXELMASK1, planes, 64, n1, f"no dq n1 {n1}")
        assert np.isfinite(got).all()
    none = check_bin(dq, np.zeros(32, np.uint8), planes, 64, 16, "no growth at all")
    assert np.array_equal(none, check_bin(None, fr.PIXELMASK1, planes, 64, 16, "no dq"))


# ---------------------------------------------------------------------------------------------- values
def test_masked_blocks_nan_and_infinities():
    rng = np.random.default_rng(10)
    a = rng.standard_normal((64, 64)).astype(np.float32)
    b = rng.standard_normal((56, 56))
    dq = np.zeros((64, 64), np.uint32)
    dq[8:12, 8:12] = 1              # one bin of s = 4 fully masked
    a[0, 0], a[5, 5] = np.nan, np.inf
    a[20, 20], a[21, 21] = np.inf, -np.inf   # in one bin: inf + -inf = NaN
    a[40:44, 40:44] = np.nan        # a bin of NaN only
    b[0, 0], b[1, 1] = -np.inf, np.nan
    for n1 in (16, 1):
        got = check_bin(dq, fr.PIXELMASK1, [a, b], 64, n1, f"values n1 {n1}")
    got = check_bin(dq, fr.PIXELMASK1, [a, b], 64, 16, "values")
    assert np.isnan(got[0, 2, 2]) and np.isnan(got[0, 10, 10]) and np.isnan(got[0, 5, 5]) and got[0, 1, 1] == np.inf
    assert np.isfinite(got[0, 0, 0]) and got[1, 1, 1] == -np.inf and np.isnan(got[1, 2, 2]) and got[1, 0, 0] == 0.0   # the padding


def test_two_calls_give_the_same_bits():
    rng = np.random.default_rng(11)
    dq, planes = fr.random_dq(rng, 256), mixed_planes(rng, 256)
    for n1 in (8, 2):   # finished in the tile, and added from parts
        a = fp().bin_planes(dq, planes, 256, n1, mask=fr.PIXELMASK1, ctx=gpu_context()).numpy()
        b = fp().bin_planes(dq, planes, 256, n1, mask=fr.PIXELMASK1, ctx=gpu_context()).numpy()
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("nside, n1", [(64, 16), (96, 32)])   # finished in the tile (s = 4), and added from parts (s = 3)
def test_bin_locations_give_the_same_bits(nside, n1):
    """the raw entry with dq, the planes and out each in host memory or in HBM, and without dq: one set of bits"""
    import ctypes as C

    from romanimpreprocess_amd import _native
    from romanimpreprocess_amd.devarray import to_device
    ctx = gpu_context()
    rng = np.random.default_rng(nside)
    dq, planes = np.ascontiguousarray(fr.random_dq(rng, nside, 0.1), dtype=np.uint32), mixed_planes(rng, nside)[:4]
    grow = np.ascontiguousarray(fr.PIXELMASK1, dtype=np.uint8)
    H, D = _native.RIP_HOST, _native.RIP_DEVICE
    assert _native.location_of(to_device(dq)) == D and _native.location_of(to_device(dq).t) == D and _native.location_of(dq) == H

    def run(dq_on, planes_on, out_on, with_dq=True):
        q = None if not with_dq else (to_device(dq) if dq_on else dq)
        keep = [to_device(a) if on else a for a, on in zip(planes, planes_on)]
        out = np.full((len(keep), n1, n1), 7.0)
        if out_on:
            out = to_device(out)
        ints = lambda v: np.array(v, dtype=np.intc)   # noqa: E731
        ctx.call("rip_fpa_bin", q, D if dq_on else H, grow, nside, n1, len(keep), (C.c_void_p * len(keep))(*[a.ctypes.data for a in keep]),
                 ints([_native.dtype_code(a) for a in keep]), ints([a.shape[0] for a in keep]), ints([D if on else H for on in planes_on]),
                 out, D if out_on else H)
        return (out.numpy() if out_on else out).tobytes()

    for with_dq in (True, False):
        host = run(False, [False] * 4, False, with_dq)
        assert host == run(True, [True] * 4, True, with_dq), "everything in HBM"
        assert host == run(True, [False, True, True, False], False, with_dq), "mixed, out on the host"
        assert host == run(False, [True, False, False, True], True, with_dq), "mixed, out in HBM"
    want = fp().bin_planes(dq, planes, nside, n1, mask=fr.PIXELMASK1, ctx=ctx).numpy()
    assert run(False, [False] * 4, False) == want.tobytes(), "the wrapper's bits"


def test_render_locations_give_the_same_bits(g):
    """maps and the picture each in host memory or in HBM, with stamps and a font and without (glyphs and stamps NULL)"""
    from romanimpreprocess_amd.devarray import to_device
    ctx = gpu_context()
    n1, ny, nx = 8, 40, 60
    maps = render_case(np.random.default_rng(13), n1, nsca=2)
    present, pos = np.ones((2, 2), np.uint8), np.array([[1, 2], [20, 30]], np.int32)
    stamps = fp().text_stamps(1, (ny, nx), (2, 20), 1, 200, "ab")

    def run(font, maps_on, out_on):
        out = to_device(np.full((ny, 2 * nx + 3, 3), 7, np.uint8)) if out_on else None
        got = fp().render(to_device(maps) if maps_on else maps, present, -1.0, 3.0, (True, False), n1, ny, nx, pos, table=g["table"],
                          font=font, stamps=stamps, ctx=ctx, out=out)
        assert (got is out) if out_on else isinstance(got, np.ndarray)
        return (got.numpy() if out_on else got).tobytes()

    for font in (g["glyphs"], None):
        host = run(font, False, False)
        for maps_on, out_on in ((True, True), (False, True), (True, False)):
            assert run(font, maps_on, out_on) == host, (font is not None, maps_on, out_on)
    assert run(g["glyphs"], False, False) != run(None, False, False), "the stamps are drawn"


def test_bin_refusals_launch_nothing():
    import torch

    from romanimpreprocess_amd.devarray import DevArray
    ctx = gpu_context()
    out = DevArray(torch.full((1, 16, 16), 7.0, dtype=torch.float64, device=torch.device("cuda", 0))).sync()
    plane, bad_grow = np.ones((64, 64), np.float32), fr.PIXELMASK1.copy()
    bad_grow[4] = 3
    for kw, match in ((dict(planes=[np.ones((61, 61), np.float32)]), "cannot be centred"), (dict(planes=[np.ones((66, 66))]), "does not fit"),
                      (dict(n1=12), "power of two"), (dict(n1=128), "power of two"), (dict(mask=bad_grow), "growth 3 of bit 4")):
        args = dict(planes=[plane], n1=16, mask=fr.PIXELMASK1)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            fp().bin_planes(np.zeros((64, 64), np.uint32), args["planes"], 64, args["n1"], mask=args["mask"], ctx=ctx, out=out)
    with pytest.raises(ValueError, match="outside 1..8"):
        fp().bin_planes(None, [plane] * 9, 64, 16, ctx=ctx)
    assert bool((out.t == 7.0).all())


# ---------------------------------------------------------------------------------------------- render
def render_case(rng, n1, nsca=3):
    """maps with values at, between and beyond vmin = -1 and vmax = 3, NaN and infinities among them"""
    maps = rng.uniform(-2.0, 4.0, (2, nsca, n1, n1))
    maps[0, 0].flat[:8] = [-1.0, 3.0, -1.5, 3.5, np.nan, np.inf, -np.inf, -1.0 + 4.0 * 37 / 256]
    maps[1, 1] = np.linspace(-1.0, 3.0, n1 * n1).reshape(n1, n1)
    return maps


def test_render_against_the_restatement(g):
    rng = np.random.default_rng(12)
    n1, ny, nx = 16, 60, 90
    pos = np.array([[2, 3], [10, 12], [30, 70]], np.int32)   # the second SCA overlaps the first and wins there
    maps = render_case(rng, n1)
    present = np.array([[1, 1, 1], [1, 1, 0]], np.uint8)     # the last SCA of panel 1 has no file: zeros
    texts = [(0, 1, 40, 1, 200, "gh"), (1, 2, 60, 1, 0, "abcdef"), (1, 20, 10, 2, 90, "Z")]   # "abcdef" runs off the right edge
    stamps = [s for p, y, x, size, val, txt in texts for s in fp().text_stamps(p, (ny, nx), (y, x), size, val, txt)]
    assert len(stamps) == 2 + 4 + 1
    for scale, font in (((True, False), g["glyphs"]), ((False, False), None), ((True, True), None), ((False, True), g["glyphs"])):
        # the restatement writes the letters of a scale before the other texts: the device gets them in that order
        every = [s for j in range(2) if scale[j] for s in fp().scale_stamps(j, n1, ny, nx, "gain", -1.0, 3.0, "{:4.2f}")] + stamps
        got = fp().render(maps, present, -1.0, 3.0, scale, n1, ny, nx, pos, table=g["table"], font=font, stamps=every, ctx=gpu_context())
        want = fr.compose([fr.panel_ref(maps[j], present[j], -1.0, 3.0, n1, ny, nx, pos, g["table"], font, "gain", "{:4.2f}" if scale[j] else None,
                                        [t[1:] for t in texts if t[0] == j])[0] for j in range(2)], n1)
        assert got.shape == want.shape == (ny, 2 * nx + 5, 3) and np.array_equal(got, want), (scale, font is not None)
    first = fp().render(maps, present, -1.0, 3.0, False, n1, ny, nx, pos, table=g["table"], ctx=gpu_context())
    px = first[2, 3:11].astype(int)   # at vmin, at vmax, below, above, NaN (0: below vmin), +inf, -inf, index 37 exactly
    t = g["table"].astype(int)
    assert np.array_equal(px, t[[0, 255, 0, 255, 64, 255, 0, 37]])
    assert np.array_equal(first[30:46, 70 + nx + 5:86 + nx + 5], np.broadcast_to(g["table"][64], (16, 16, 3)))   # missing: zeros -> x = 0.25
    assert np.array_equal(first[10:26, 12:28], g["table"][fr.color_index(np.clip((maps[0, 1] + 1) / 4, 0, 1))])   # the later SCA won


def test_render_refusals_launch_nothing(g):
    import torch

    from romanimpreprocess_amd.devarray import DevArray
    ctx = gpu_context()
    n1, ny, nx = 8, 40, 60
    maps, present = np.zeros((1, 1, n1, n1)), np.ones((1, 1), np.uint8)
    out = DevArray(torch.full((ny, nx, 3), 7, dtype=torch.uint8, device=torch.device("cuda", 0))).sync()

    def call(pos=((1, 1),), scale=False, stamps=(), n1_=n1, vmax=1.0):
        m = np.zeros((1, 1, n1_, n1_))
        return fp().render(m, present, 0.0, vmax, scale, n1_, ny, nx, np.array(pos, np.int32), font=g["glyphs"], stamps=stamps, nw=1, ctx=ctx,
                           out=out)

    for kw, match in ((dict(scale=True, n1_=4), "needs n1 >= 8"), (dict(pos=((-1, 1),)), "SCA 1 starts outside"),
                      (dict(pos=((1, 60),)), "SCA 1 starts outside"), (dict(pos=((35, 1),)), "reaches past"),
                      (dict(stamps=[[0, -1, 3, 1, 0, 65]]), "stamp 0 starts outside"), (dict(stamps=[[0, 3, 60, 1, 0, 65]]), "stamp 0 starts outside"),
                      (dict(stamps=[[0, 30, 3, 1, 0, 65]]), "reaches past"), (dict(stamps=[[1, 3, 3, 1, 0, 65]]), "panel 1 of 1"),
                      (dict(vmax=0.0), "colour range")):
        with pytest.raises(ValueError, match=match):
            call(**kw)
    assert bool((out.t == 7).all())
    call()   # and the same buffer is drawn into by a call that is accepted
    assert bool((out.t[0, 0] == 255).all()) and not bool((out.t == 7).any())


# ---------------------------------------------------------------------------------------------- the public interface
def write_files(g, tmp_path):
    """the fixture's calibration set as files written with calio; returns (format, font file, geometry file)"""
    from romanimpreprocess_amd import calio
    fmt = str(tmp_path / "roman_wfi_{:s}_GOLDEN_SCA{:02d}.asdf")
    for k, s in enumerate(fr.golden_scas(g)):
        if s is None:
            continue
        lin = np.zeros((4, 64, 64), np.float32)
        lin[2], lin[3] = s["lin2"], s["lin3"]
        ipc = np.zeros((3, 3, 56, 56), s["alphaH"].dtype)
        ipc[1, 0], ipc[0, 1], ipc[0, 0] = s["alphaH"], s["alphaV"], s["alphaD"]
        files = {"linearitylegendre": lin, "ipc4d": ipc, "pflat": s["pflatnorm"], "read": s["read"]}
        if "gain" in s:
            files["gain"] = s["gain"]
        for name, arr in files.items():
            calio.write_asdf(fmt.format(name, k + 1), {"roman": {"data": arr}})
        calio.write_asdf(fmt.format("mask", k + 1), {"roman": {"dq": s["dq"]}})
    font, geom = str(tmp_path / "letters.dat"), str(tmp_path / "geometry.json")
    np.savetxt(font, g["glyphs"].reshape(-1, 6), fmt="%d")
    with open(geom, "w") as f:
        json.dump(fr.SMALL, f)
    return fmt, font, geom


def assert_picture_is_the_restatements(got, scas, n1, g, font=True):
    want, frac, owner, _ = fr.multi_image_ref(scas, n1, fr.PIXELMASK1, fr.SMALL, g["table"], g["glyphs"] if font else None)
    differ = (got != want).any(axis=2)
    near = fr.near_integer(frac)
    assert not (differ & ~near).any(), f"{np.count_nonzero(differ & ~near)} pixels differ away from an index step"
    assert np.count_nonzero(near) < 0.001 * np.count_nonzero(owner >= 0)
    return owner


@pytest.fixture(scope="module")
def files(g, tmp_path_factory):
    return write_files(g, tmp_path_factory.mktemp("fpaplot"))


def test_multi_image_from_files(g, files):
    from romanimpreprocess_amd.utils.maskhandling import PixelMask1
    fmt, font, _ = files
    scas = fr.golden_scas(g)
    for n1, key in ((32, "rgb_n32"), (16, "rgb")):
        got = fp().multi_image(fmt, n1, PixelMask1, font=font, ctx=gpu_context(), geometry=fr.SMALL)
        owner = assert_picture_is_the_restatements(got, scas, n1, g)
        fr.assert_picture(got, g[key], owner, key)   # and the reference's own picture, at its conditions
    bare = fp().multi_image(fmt, 16, PixelMask1, ctx=gpu_context(), geometry=fr.SMALL)   # no font: bar and ticks, no text
    assert_picture_is_the_restatements(bare, scas, 16, g, font=False)
    assert (bare != got).any() and np.array_equal(bare[:20], got[:20])   # the letters are all that is missing


def test_read_sca_image_and_make_big_image(g, files):
    from romanimpreprocess_amd.utils.maskhandling import PixelMask1
    fmt, font, _ = files
    scas = fr.golden_scas(g)
    for j, p in enumerate(PTYPES):
        for n1, want in ((16, g["maps"][j, 0]), (64, g["maps_sca1_n64"][j]), (2, g["maps_sca1_n2"][j]), (1, g["maps_sca1_n1"][j])):
            got = fp().read_sca_image(fmt, n1, p, 1, mask=PixelMask1, ctx=gpu_context(), geometry=fr.SMALL)
            ok = ~np.isnan(want)
            assert np.array_equal(np.isnan(got), ~ok) and (np.abs(got - want)[ok] <= fr.reference_bound(scas[0], p, n1)[ok]).all(), (p, n1)
    kw = dict(ctx=gpu_context(), geometry=fr.SMALL)
    assert not fp().read_sca_image(fmt, 16, "gain", int(g["missing_gain"]), mask=None, **kw).any()   # a missing file: zeros, no mask needed
    with pytest.raises(TypeError, match="mask=None"):
        fp().read_sca_image(fmt, 16, "gain", 1, mask=None, **kw)
    with pytest.raises(KeyError):
        fp().read_sca_image(fmt, 16, "pflat", 1, mask=PixelMask1, **kw)
    ny, nx, pos = fr.layout(16, fr.SMALL)
    owner = np.full((ny, nx), -1)
    for k, (py, px) in enumerate(pos):
        owner[py:py + 16, px:px + 16] = k
    plain = fp().make_big_image(fmt, 16, "gain", vmin=1.2, vmax=2.1, mask=PixelMask1, font=font, **kw)
    fr.assert_picture(plain, g["gain_plain"], owner, "gain_plain")
    scaled = fp().make_big_image(fmt, 16, "gain", vmin=1.2, vmax=2.1, mask=PixelMask1, scaleformat="{:4.2f}", font=font, **kw)
    fr.assert_picture(scaled, g["gain_scale"], np.where((g["gain_scale"] != g["gain_plain"]).any(axis=2), -1, owner), "gain_scale")
    # pflatnorm is not divided by its median: the picture is that of the plain means
    pf = fp().make_big_image(fmt, 16, "pflatnorm", vmin=0.8, vmax=1.2, mask=PixelMask1, **kw)
    j = PTYPES.index("pflatnorm")
    x = np.clip((np.nan_to_num(g["maps"][j, 0]) - 0.8) / (1.2 - 0.8), 0, 1)
    assert np.count_nonzero((pf[pos[0][0]:pos[0][0] + 16, pos[0][1]:pos[0][1] + 16] != g["table"][fr.color_index(x)]).any(axis=2)) <= 1


def test_multi_image_from_device_planes(g, files):
    from romanimpreprocess_amd.devarray import to_device
    from romanimpreprocess_amd.utils.maskhandling import PixelMask1
    fmt, font, _ = files
    scas = fr.golden_scas(g)
    dev = [None if s is None else {k: (to_device(v) if i % 2 == 0 or k == "dq" else v) for i, (k, v) in enumerate(s.items())} for s in scas]
    got = fp().multi_image_from_planes(dev, 16, PixelMask1, font=g["glyphs"], ctx=gpu_context(), geometry=fr.SMALL)
    want = fp().multi_image(fmt, 16, PixelMask1, font=font, ctx=gpu_context(), geometry=fr.SMALL)
    assert np.array_equal(got, want)   # the same planes, wherever they lie: the same bits
    with pytest.raises(ValueError, match="18"):
        fp().multi_image_from_planes(dev[:3], 16, PixelMask1, geometry=fr.SMALL)


def test_command_line(g, files, tmp_path):
    from romanimpreprocess_amd.utils.maskhandling import PixelMask1
    fmt, font, geom = files
    out = str(tmp_path / "panel.png")
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    subprocess.run([sys.executable, "-m", "romanimpreprocess_amd.utils.fpaplot", fmt, out, "--font", font, "--n1", "16", "--geometry", geom],
                   check=True, cwd=REPO, env=env, timeout=300)
    want = fp().multi_image(fmt, 16, PixelMask1, font=font, ctx=gpu_context(), geometry=fr.SMALL)
    assert np.array_equal(fr.read_png(out), want[::-1])   # upside-down, as the script saves it
