"""GPU: rip_view_ranks, rip_view_render and rip_view_plane_diff against tests/visualize_ref.py (the numpy restatement, itself held
to np.percentile and matplotlib by tests/test_host_visualize.py), and romanimpreprocess_amd.utils.visualize / utils.diff on top.

Selection, linear panels, colour bars, ticks, stamps and the plane difference are exact: equal bit for bit.  The power-norm
panels have the one tolerance, visualize_ref.POWER_SLACK_ULPS = 2 float32 steps of the normalised value before the index rule
(device powf 1 ulp, from the HIP math API reference; numpy float32 power 1.006 ulp, measured against float64 pow: the sum, 2.006
ulp, is at most 2 representable steps); the pixels that need it must stay below 1 % of a panel."""

import os
import subprocess
import sys

import fpaplot_ref
import numpy as np
import pytest
import visualize_cases as vc
import visualize_ref as vr
from conftest import REPO, assert_same_bits, gpu_context, load_golden

pytestmark = pytest.mark.gpu


def vz():
    from romanimpreprocess_amd.utils import visualize
    return visualize


def magma():
    from romanimpreprocess_amd.utils import fpaplot
    return fpaplot.MAGMA


@pytest.fixture(scope="module")
def glyphs():
    return load_golden("fpaplot_small")["glyphs"]


def dev(a):
    from romanimpreprocess_amd.devarray import to_device
    return to_device(a)


# ---------------------------------------------------------------------------------------------- selection
@pytest.mark.parametrize("case", vc.SELECT_CASES, ids=[c[0] for c in vc.SELECT_CASES])
def test_ranks_are_the_sorted_values(case):
    name, cube, window, (g0, g1), minus = case
    want = vr.sorted_values(vr.window_values(cube, window, g0, g1, minus))
    n = len(want)
    assert np.array_equal(want, np.sort(vr.window_values(cube, window, g0, g1, minus), axis=None))
    ranks = vc.ranks_for(n)
    host, nan = vz().window_ranks(cube, window, g0, g1, minus, ranks, ctx=gpu_context())
    assert nan == 0 and host.dtype == np.float32
    assert_same_bits(host, want[ranks], name)
    again, _ = vz().window_ranks(cube, window, g0, g1, minus, ranks, ctx=gpu_context())
    there, nan_there = vz().window_ranks(dev(cube), window, g0, g1, minus, ranks, ctx=gpu_context())
    assert host.tobytes() == again.tobytes() == there.tobytes() and nan_there == 0, "two calls, host and HBM: the same bits"
    for some in ([0], [n - 1], [n // 2, n // 2]):   # fewer ranks: other histograms are shared
        got, _ = vz().window_ranks(cube, window, g0, g1, minus, some, ctx=gpu_context())
        assert_same_bits(got, want[some], f"{name} ranks {some}")


def test_every_rank_of_a_small_window():
    cube = vc.zeros_cube(41, (2, 5, 9))
    cube[1, 2, 3:6] = [np.inf, -np.inf, 3.5]
    want = vr.sorted_values(vr.window_values(cube, (1, 7, 0, 4), 0, 2))
    for at in range(0, len(want), 8):
        ranks = list(range(at, min(at + 8, len(want))))
        got, nan = vz().window_ranks(cube, (1, 7, 0, 4), 0, 2, None, ranks, ctx=gpu_context())
        assert_same_bits(got, want[ranks], f"ranks {ranks}")
        assert nan == 0


def test_nan_is_counted_and_makes_the_percentile_nan():
    cube = vc.nan_cube(42)
    for c in (cube, dev(cube)):
        _, nan = vz().window_ranks(c, (0, 89, 0, 19), 0, 3, None, [0, 5], ctx=gpu_context())
        assert nan == 3
        _, nan = vz().window_ranks(c, (0, 89, 0, 19), 0, 3, 0, [7], ctx=gpu_context())   # minus a plane with NaNs: more of them
        assert nan == int(np.isnan(vr.window_values(cube, (0, 89, 0, 19), 0, 3, 0)).sum()) == 5
        assert np.isnan(vz().block_percentiles(c, (0, 89, 0, 19), 50.0, ctx=gpu_context()))
        clean = vz().block_percentiles(c, (10, 89, 0, 19), [2.0, 98.0], planes=(1, 2), ctx=gpu_context())
        for got, q in zip(clean, (2.0, 98.0)):   # a scalar q, as the reference's calls: numpy then works in float32
            assert_same_bits(got, np.percentile(cube[1, :, 10:], q), "a window without the NaNs")
    both = vc.inf_cube(43)
    both[0, 2, 2] = both[1, 2, 2] = np.inf   # inf - inf: a NaN that no sample holds
    assert vz().window_ranks(both, (0, 89, 0, 19), 0, 1, 1, [0], ctx=gpu_context())[1] == 1
    assert np.isnan(vz().block_percentiles(both, (0, 89, 0, 19), 50.0, planes=(0, 1), minus=1, ctx=gpu_context()))
    assert vz().window_ranks(vc.u16_cube(43, (3, 9, 9)), (0, 8, 0, 8), 0, 3, 1, [0], ctx=gpu_context())[1] == 0


def test_block_percentiles_are_numpys():
    for cube in (vc.u16_cube(44), vc.f32_cube(45)):
        w = (5, 250, 3, 60)
        data = vr.window_values(cube, w, 0, 5)
        qs = [0, 100, 2, 98, 37.3, 50.0, 99.9]
        for c in (cube, dev(cube)):
            got = vz().block_percentiles(c, w, qs, ctx=gpu_context())
            for g, q in zip(got, qs):
                assert_same_bits(g, np.percentile(data, q), f"q {q}")
            assert_same_bits(vz().block_percentiles(c, w, 98.0, planes=(4, 5), minus=1, ctx=gpu_context()), np.percentile(data[4] - data[1], 98.0),
                             "the last difference")


def test_rank_refusals_launch_nothing():
    from romanimpreprocess_amd import _native
    ctx = gpu_context()
    cube = vc.u16_cube(46, (3, 9, 11))
    H, U16 = _native.RIP_HOST, _native.RIP_U16
    values, nan, ranks = np.full(8, 7.0, np.float32), np.full(1, 7, np.uint32), np.zeros(8, np.uint32)

    def call(cube_=cube, dtype=U16, loc=H, shape=(3, 9, 11), win=(0, 8, 0, 10), g=(0, 3), minus=-1, nranks=1, ranks_=ranks, values_=values, nan_=nan):
        ctx.call("rip_view_ranks", cube_, dtype, loc, *shape, *win, *g, minus, nranks, ranks_, values_, nan_)

    for kw, match in ((dict(cube_=None), "NULL"), (dict(ranks_=None), "NULL"), (dict(values_=None), "NULL"), (dict(nan_=None), "NULL"),
                      (dict(dtype=_native.RIP_F64), "neither RIP_U16 nor RIP_F32"), (dict(dtype=9), "neither"), (dict(loc=2), "cube_location 2"),
                      (dict(win=(3, 2, 0, 10)), "empty or leaves"), (dict(win=(0, 8, 5, 4)), "empty or leaves"), (dict(win=(-1, 8, 0, 10)), "empty or leaves"),
                      (dict(win=(0, 9, 0, 10)), "empty or leaves"), (dict(win=(0, 8, 0, 11)), "empty or leaves"), (dict(g=(1, 1)), "planes 1..1"),
                      (dict(g=(-1, 2)), "planes"), (dict(g=(0, 4)), "planes"), (dict(minus=3), "minus 3"), (dict(minus=-2), "minus -2"),
                      (dict(nranks=0), "outside 1..8"), (dict(nranks=9), "outside 1..8"),
                      (dict(ranks_=np.array([297], np.uint32)), "rank 297 is not below the 297"), (dict(shape=(0, 9, 11)), "a cube of"),
                      (dict(shape=(70000, 70000, 11), win=(0, 69999, 0, 0), g=(0, 70000)), "2\\^32 or more")):
        with pytest.raises(ValueError, match=match):
            call(**kw)
    assert (values == 7.0).all() and nan[0] == 7
    call(ranks_=np.array([296], np.uint32))   # and the largest rank is accepted
    assert values[0] == cube.max() and nan[0] == 0


# ---------------------------------------------------------------------------------------------- render
def small_cube():
    """float32 with values at, between and beyond the limits -1 and 3, NaN and infinities among them; 7 x 13 pixels"""
    rng = np.random.default_rng(51)
    cube = rng.uniform(-2.0, 4.0, (3, 7, 13)).astype(np.float32)
    cube[0].flat[:8] = [-1.0, 3.0, -1.5, 3.5, np.nan, np.inf, -np.inf, -1.0 + 4.0 * 37 / 256]
    cube[2, 3] = np.linspace(-1.0, 3.0, 13)
    return cube


def render_both(cube, window, panels, limits, zoom, cell, shape, font=None, stamps=()):
    """the device's picture (checked to be the same from host memory and HBM, into host memory and HBM) and the restatement's"""
    import torch

    from romanimpreprocess_amd.devarray import DevArray
    got = vz().render(cube, window, panels, limits, zoom, cell, shape, font=font, stamps=stamps, ctx=gpu_context())
    out = DevArray(torch.full((shape[0], shape[1], 3), 7, dtype=torch.uint8, device=torch.device("cuda", 0))).sync()
    there = vz().render(dev(cube), window, panels, limits, zoom, cell, shape, font=font, stamps=stamps, ctx=gpu_context(), out=out)
    assert there is out and got.tobytes() == out.numpy().tobytes(), "host memory and HBM: the same bytes"
    want, normed = vr.render_ref(cube, window, panels, limits, zoom, cell, shape, magma(), font, stamps)
    return got, want, normed


@pytest.mark.parametrize("zoom", [1, 3])
def test_linear_panels_bars_ticks_and_stamps(zoom, glyphs):
    cube = small_cube()
    window = (0, 12, 0, 6)
    h, w = 7 * zoom, 13 * zoom
    ch, cw = h + 14, w + vr.BAR_GAP + vr.BAR_W + vr.TICK + 20
    # three cells side by side and one above: a difference, a panel without a bar, vmin == vmax
    panels = [[0, -1, 0, 0, 0, 1], [2, 1, 0, 0, cw + 3, 1], [1, -1, 0, ch + 2, 0, 0], [0, -1, 0, ch + 2, cw + 3, 1]]
    limits = [[-1.0, 3.0, 1.0], [-0.7, 1.9, 1.0], [-1.0, 3.0, 1.0], [0.5, 0.5, 1.0]]
    shape = (2 * ch + 2, 2 * cw + 3)
    stamps = [s for p, y, x, size, val, txt in ((0, h + 1, 0, 1, 0, "Gr"), (1, 0, w + 16, 1, 200, "ab"), (3, 2, 1, 1, 90, "Zq"), (2, h, 5, 1, 0, "abcdefgh"))
              for s in fpaplot_ref_text(p, (ch, cw), y, x, size, val, txt)]
    pics = {}
    for font, st in ((None, ()), (glyphs, stamps)):
        got, want, _ = render_both(cube, window, panels, limits, zoom, (ch, cw), shape, font, st)
        assert got.shape == want.shape == shape + (3,) and np.array_equal(got, want), (zoom, font is not None)
        pics[font is not None] = got
    assert (pics[True] != pics[False]).any(), "the stamps are drawn"
    got, t = pics[False], magma().astype(int)
    first = got[0, 0:8 * zoom:zoom].astype(int)   # at vmin, at vmax, below, above, NaN, +inf, -inf, index 37 exactly
    assert np.array_equal(first[[0, 1, 2, 3, 5, 6, 7]], t[[0, 255, 0, 255, 255, 0, 37]]) and (first[4] == 255).all(), "NaN is white"
    assert (got[ch + 2:ch + 2 + h, cw + 3:cw + 3 + w] == magma()[0]).all(), "vmin == vmax: index 0, the NaN sample too"
    assert (got[ch + 2:, w:cw] == 255).all(), "no bar where none is asked for"
    assert (got[0, w + vr.BAR_GAP + vr.BAR_W:w + vr.BAR_GAP + vr.BAR_W + vr.TICK] == 0).all(), "a tick"


def fpaplot_ref_text(panel, shape, y, x, size, val, txt):
    from romanimpreprocess_amd.utils import fpaplot
    return fpaplot.text_stamps(panel, shape, (y, x), size, val, txt)


def test_windows_one_pixel_wide_and_high_and_u16():
    cube = vc.u16_cube(52, (3, 20, 31))
    for window, zoom in (((5, 5, 2, 17), 2), ((3, 29, 19, 19), 1), ((30, 30, 19, 19), 4), ((7, 30, 3, 19), 1)):
        dx, dy = window[1] - window[0] + 1, window[3] - window[2] + 1
        ch, cw = zoom * dy, zoom * dx + vr.BAR_GAP + vr.BAR_W + vr.TICK
        panels = [[0, -1, 0, 0, 0, 1], [2, 1, 0, ch + 1, 0, 1]]
        limits = [[1000.0, 60000.0, 1.0], [-30000.5, 29999.25, 1.0]]
        got, want, _ = render_both(cube, window, panels, limits, zoom, (ch, cw), (2 * ch + 1, cw))
        assert np.array_equal(got, want), window


def test_power_panels_within_the_slack():
    lo, hi = vc.POWER_LIMITS
    cube = vc.POWER_CUBE
    window, zoom = (0, 60, 0, 36), 2
    ch, cw = 37 * zoom, 61 * zoom + vr.BAR_GAP + vr.BAR_W + vr.TICK
    panels = [[0, -1, 1, 0, 0, 1], [0, 1, 1, ch, 0, 1], [0, -1, 0, 2 * ch, 0, 1]]
    limits = [[lo, hi, vr.GAMMA], [-0.05 * hi, hi, vr.GAMMA], [lo, hi, 1.0]]
    got, want, normed = render_both(cube, window, panels, limits, zoom, (ch, cw), (3 * ch, cw))
    assert np.array_equal(got[2 * ch:], want[2 * ch:]), "the linear panel"
    assert np.array_equal(got[:, 61 * zoom:], want[:, 61 * zoom:]), "bars and ticks"
    for p in (0, 1):
        exact, slack, wrong = vr.power_panel_check(got[p * ch:p * ch + 37 * zoom, :61 * zoom], normed[p], magma(), zoom)
        print(f"power panel {p}: {exact} pixels equal, {slack} within {vr.POWER_SLACK_ULPS} ulp, {wrong} beyond")
        assert wrong == 0
        assert slack < 0.01 * (exact + slack)


def test_render_refusals_launch_nothing(glyphs):
    import torch

    from romanimpreprocess_amd.devarray import DevArray
    ctx = gpu_context()
    cube = small_cube()
    out = DevArray(torch.full((30, 60, 3), 7, dtype=torch.uint8, device=torch.device("cuda", 0))).sync()

    def call(window=(0, 12, 0, 6), panel=(0, -1, 0, 0, 0, 1), limit=(-1.0, 3.0, 1.0), zoom=1, cell=(20, 30), stamps=(), font=glyphs, shape=(30, 60),
             out_=out):
        return vz().render(cube, window, [list(panel)], [list(limit)], zoom, cell, shape, font=font, stamps=stamps, ctx=ctx, out=out_)

    for kw, match in ((dict(limit=(3.0, -1.0, 1.0)), "colour range"), (dict(limit=(np.nan, 1.0, 1.0)), "colour range"),
                      (dict(limit=(0.0, np.inf, 1.0)), "colour range"), (dict(panel=(0, -1, 1, 0, 0, 1), limit=(0.0, 1.0, 0.0)), "gamma"),
                      (dict(zoom=0), "zoom 0"), (dict(panel=(0, -1, 0, 11, 0, 1)), "reaches past the picture"),
                      (dict(panel=(0, -1, 0, 0, 31, 1)), "reaches past the picture"), (dict(panel=(0, -1, 0, -1, 0, 1)), "reaches past the picture"),
                      (dict(panel=(3, -1, 0, 0, 0, 1)), "plane 3"), (dict(panel=(0, 3, 0, 0, 0, 1)), "minus 3"), (dict(panel=(0, -1, 2, 0, 0, 1)), "norm kind 2"),
                      (dict(cell=(6, 30)), "does not hold the window"), (dict(cell=(20, 27)), "colour bar of panel 0 does not fit"),
                      (dict(zoom=3), "does not hold the window"), (dict(window=(0, 13, 0, 6)), "empty or leaves"), (dict(window=(5, 4, 0, 6)), "empty or leaves"),
                      (dict(stamps=[[0, -1, 3, 1, 0, 65]]), "stamp 0 starts outside"), (dict(stamps=[[0, 3, 30, 1, 0, 65]]), "stamp 0 starts outside"),
                      (dict(stamps=[[0, 9, 3, 1, 0, 65]]), "reaches past"), (dict(stamps=[[1, 3, 3, 1, 0, 65]]), "panel 1 of 1"),
                      (dict(stamps=[[0, 3, 3, 0, 0, 65]]), "size 0"), (dict(stamps=[[0, 3, 3, 1, 256, 65]]), "value 256"),
                      (dict(stamps=[[0, 3, 3, 1, 0, 256]]), "character 256")):
        with pytest.raises(ValueError, match=match):
            call(**kw)
    from romanimpreprocess_amd import _native
    H, D, F32 = _native.RIP_HOST, _native.RIP_DEVICE, _native.RIP_F32
    pan, lim, tab = np.array([[0, -1, 0, 0, 0, 1]], np.int32), np.array([[-1.0, 3.0, 1.0]], np.float32), np.ascontiguousarray(magma())
    st = np.array([[0, 3, 3, 1, 0, 65]], np.int32)

    def raw(cube_=cube, dtype=F32, loc=H, panels=pan, limits=lim, table=tab, gl=None, nstamps=0, stamps=None, out_=out, out_loc=D, npanel=1):
        ctx.call("rip_view_render", cube_, dtype, loc, 3, 7, 13, 0, 6, 0, 12, npanel, panels, limits, 1, vr.BAR_GAP, vr.BAR_W, vr.TICK, 20, 30, 30, 60,
                 table, gl, nstamps, stamps, out_, out_loc)

    for kw, match in ((dict(cube_=None), "NULL"), (dict(panels=None), "NULL"), (dict(limits=None), "NULL"), (dict(table=None), "NULL"),
                      (dict(out_=None), "NULL"), (dict(nstamps=1, stamps=st), "stamps without a glyph table"), (dict(dtype=1), "neither"),
                      (dict(loc=5), "cube_location 5"), (dict(out_loc=-1), "out_location -1"), (dict(npanel=0), "0 panels")):
        with pytest.raises(ValueError, match=match):
            raw(**kw)
    assert bool((out.t == 7).all())
    call()   # and the same buffer is drawn into by a call that is accepted
    assert bool((out.t[29, 59] == 255).all()) and not bool((out.t == 7).any())


# ---------------------------------------------------------------------------------------------- the whole picture
@pytest.mark.parametrize("ng", [2, 3, 5])
def test_visualize_cube_is_the_restatements_composition(ng, glyphs):
    rng = np.random.default_rng(60 + ng)
    ramp = (rng.integers(900, 1100, (1, 40, 53)) + np.arange(ng)[:, None, None] * rng.integers(0, 3000, (1, 40, 53))).astype(np.uint16)
    cubes = [(ramp, (3, 47, 2, 33), 2.0, None), (ramp.astype(np.float32) + rng.standard_normal(ramp.shape).astype(np.float32), (30, 99, 25, 99), 5.0, 2)]
    for cube, bounds, cut, zoom in cubes:   # the second window's upper bounds are clamped at the frame
        for font in (None, glyphs):
            got, limits = vz().visualize_cube(cube, bounds, percentile_cut=cut, font=font, zoom=zoom, ctx=gpu_context())
            want, want_limits, rows, normed = vr.visualize_ref(cube, bounds, cut, magma(), font, zoom)
            assert list(limits) == list(want_limits) and got.shape == want.shape
            for k in limits:
                assert_same_bits(np.array(limits[k], np.float32), np.array(want_limits[k], np.float32), f"ng {ng} {k}")
            z = zoom or max(1, 512 // max(normed[0].shape))
            h, w = z * normed[0].shape[0], z * normed[0].shape[1]
            power = np.zeros(got.shape[:2], bool)
            for (title, _, _, kind, y, x), t in zip(rows, normed):
                if kind == 1:
                    power[y:y + h, x:x + w] = True
                    exact, slack, wrong = vr.power_panel_check(got[y:y + h, x:x + w], t, magma(), z)
                    print(f"ng {ng} {title}: {exact} equal, {slack} within the slack, {wrong} beyond")
                    assert wrong == 0 and slack < 0.01 * (exact + slack)
            assert np.array_equal(got[~power], want[~power]), "everything but the power panels is byte-identical"
            assert int(power.any()) == int(ng > 2)
    on_device, _ = vz().visualize_cube(dev(cubes[0][0]), cubes[0][1], font=glyphs, ctx=gpu_context())
    host, _ = vz().visualize_cube(cubes[0][0], cubes[0][1], font=glyphs, ctx=gpu_context())
    assert np.array_equal(on_device, host)


def test_visualize_cube_refuses_what_the_reference_cannot_draw():
    cube = vc.u16_cube(70, (3, 12, 12))
    with pytest.raises(IndexError):
        vz().visualize_cube(cube[:1], (0, 5, 0, 5), ctx=gpu_context())
    falling = np.ascontiguousarray(cube[::-1].astype(np.float32) * np.array([3.0, 2.0, 1.0], np.float32)[:, None, None])
    falling[2] = falling[1] - 5.0   # the last difference is negative everywhere: vmin = -0.05 vmax > vmax, PowerNorm raises
    with pytest.raises(ValueError, match="colour range"):
        vz().visualize_cube(falling, (0, 11, 0, 11), ctx=gpu_context())
    cube_nan = falling.copy()
    cube_nan[0, 3, 3] = np.nan
    with pytest.raises(ValueError, match="colour range"):
        vz().visualize_cube(cube_nan, (0, 11, 0, 11), ctx=gpu_context())


# ---------------------------------------------------------------------------------------------- the drop-ins from files
@pytest.fixture(scope="module")
def l1_file(tmp_path_factory):
    from romanimpreprocess_amd import calio
    rng = np.random.default_rng(80)
    cube = (rng.integers(900, 1100, (1, 48, 64)) + np.arange(4)[:, None, None] * rng.integers(0, 3000, (1, 48, 64))).astype(np.uint16)
    d = tmp_path_factory.mktemp("visualize")
    path = str(d / "l1.asdf")
    calio.write_asdf(path, {"roman": {"data": cube}})
    return path, cube, d


def read_pdf_raster(path):
    import re
    import zlib
    raw = open(path, "rb").read()
    assert raw.startswith(b"%PDF-") and raw.endswith(b"%%EOF")
    m = re.search(rb"/Width (\d+) /Height (\d+) .*?/Length (\d+) >>\nstream\n", raw)
    nx, ny, n = (int(g) for g in m.groups())
    return np.frombuffer(zlib.decompress(raw[m.end():m.end() + n]), np.uint8).reshape(ny, nx, 3)


def test_visualize_from_a_file_to_png_and_pdf(l1_file, glyphs):
    path, cube, d = l1_file
    png, pdf, font = str(d / "out.png"), str(d / "out.pdf"), str(d / "letters.dat")
    np.savetxt(font, glyphs.reshape(-1, 6), fmt="%d")
    vz().visualize(["visualize.py", path, "5,40,8,99", png, "3.0"], ctx=gpu_context())
    want, _ = vz().visualize_cube(cube, (5, 40, 8, 47), percentile_cut=3.0, ctx=gpu_context())
    assert np.array_equal(fpaplot_ref.read_png(png), want[::-1])   # top first in the file
    vz().visualize(["visualize.py", path, "5,40,8,30", pdf], font=font, ctx=gpu_context())
    want, _ = vz().visualize_cube(cube, (5, 40, 8, 30), font=glyphs, ctx=gpu_context())
    assert np.array_equal(read_pdf_raster(pdf), want[::-1])


def test_visualize_command_line(l1_file, glyphs):
    path, cube, d = l1_file
    out, font = str(d / "cli.png"), str(d / "letters_cli.dat")
    np.savetxt(font, glyphs.reshape(-1, 6), fmt="%d")
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    subprocess.run([sys.executable, "-m", "romanimpreprocess_amd.utils.visualize", path, "0,63,0,47", out, "2.5", "--font", font], check=True,
                   cwd=REPO, env=env, timeout=300)
    want, _ = vz().visualize_cube(cube, (0, 63, 0, 47), percentile_cut=2.5, font=glyphs, ctx=gpu_context())
    assert np.array_equal(fpaplot_ref.read_png(out), want[::-1])


def test_diff_to_fits(l1_file):
    from romanimpreprocess_amd import calio
    from romanimpreprocess_amd.utils import diff
    path, cube, d = l1_file
    out = str(d / "diff.fits")
    diff.diff(["diff.py", path, out, "3", "1"], ctx=gpu_context())
    header, got = calio.read_fits_image(out)
    want = cube.astype(np.float32)[1] - cube.astype(np.float32)[3]
    assert header["BITPIX"] == -32 and got.shape == want.shape
    assert_same_bits(np.asarray(got).astype(np.float32), want, "diff.py 3 1")   # stored big-endian
    assert (want < 0).any()
    f32 = vc.f32_cube(81, (4, 19, 23))
    for c in (f32, dev(f32)):
        for g1, g2 in ((0, 3), (2, 2), (-1, 0)):
            assert_same_bits(diff.group_difference(c, g1, g2, ctx=gpu_context()).numpy(), f32[g2] - f32[g1], f"f32 {g1} {g2}")
    host_out = np.full((19, 23), 7.0, np.float32)
    assert diff.group_difference(f32, 1, 2, ctx=gpu_context(), out=host_out) is host_out
    assert_same_bits(host_out, f32[2] - f32[1], "into host memory")
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cli = str(d / "cli.fits")
    subprocess.run([sys.executable, "-m", "romanimpreprocess_amd.utils.diff", path, cli, "0", "2"], check=True, cwd=REPO, env=env, timeout=300)
    assert open(cli, "rb").read() != open(out, "rb").read() and os.path.getsize(cli) == os.path.getsize(out)


def test_diff_refusals_launch_nothing():
    import torch

    from romanimpreprocess_amd import _native
    from romanimpreprocess_amd.devarray import DevArray
    from romanimpreprocess_amd.utils import diff
    ctx = gpu_context()
    cube = vc.u16_cube(82, (3, 9, 11))
    out = DevArray(torch.full((9, 11), 7.0, dtype=torch.float32, device=torch.device("cuda", 0))).sync()
    for g1, g2 in ((3, 0), (0, -4)):
        with pytest.raises(IndexError):
            diff.group_difference(cube, g1, g2, ctx=ctx, out=out)
    H, D, U16 = _native.RIP_HOST, _native.RIP_DEVICE, _native.RIP_U16
    for args, match in (((None, U16, H, 3, 9, 11, 0, 1, out, D), "NULL"), ((cube, U16, H, 3, 9, 11, 0, 1, None, D), "NULL"),
                        ((cube, 1, H, 3, 9, 11, 0, 1, out, D), "neither"), ((cube, U16, 3, 3, 9, 11, 0, 1, out, D), "cube_location 3"),
                        ((cube, U16, H, 3, 9, 11, 0, 1, out, 2), "out_location 2"), ((cube, U16, H, 3, 9, 11, 3, 1, out, D), "planes 3 and 1"),
                        ((cube, U16, H, 3, 9, 11, 0, -1, out, D), "planes 0 and -1")):
        with pytest.raises(ValueError, match=match):
            ctx.call("rip_view_plane_diff", *args)
    assert bool((out.t == 7.0).all())
