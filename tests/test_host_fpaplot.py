"""CPU-only: tests/fpaplot_ref.py, the float64 numpy restatement of the focal-plane overview, against the fixture that the
reference's own utils/fpaplot.py produced (tests/golden/fpaplot_small.npz); the package's host-side pieces (layout arithmetic,
text stamps, colour table, PNG writer) against the restatement; and the new entry points' declarations.

Bounds: the reference sums a float32 file in float32, the restatement in float64, so a mean may differ by
s^2 * 2^-24 * sum|v| / count (2^-53 for a float64 file): the worst case of a sum of s^2 terms in any order.  The colour index may
then differ by one step in at most 0.5 % of the SCA pixels -- no channel by more than 3, viridis's neighbours differ by at most
[3, 2, 2] -- and every other pixel is equal byte for byte."""

import ctypes
import os
import re

import fpaplot_ref as fr
import numpy as np
import pytest
from conftest import REPO, load_golden

from romanimpreprocess_amd import _native, calio
from romanimpreprocess_amd.utils import fpaplot

PTYPES = [p[0] for p in fr.PANELS]


@pytest.fixture(scope="module")
def g():
    return load_golden("fpaplot_small")


def test_restatement_maps_against_the_reference(g):
    scas = fr.golden_scas(g)
    n1 = int(g["n1"])
    for j, p in enumerate(PTYPES):
        for k, sca in enumerate(scas):
            want = g["maps"][j, k]
            if sca is None or p not in sca:
                assert not want.any(), f"{p} SCA {k + 1}: a missing file is all zero"
                continue
            got = fr.bin_ref(sca["dq"], fr.PIXELMASK1, [sca[p]], 64, n1)[0][0]
            assert np.array_equal(np.isnan(got), np.isnan(want))
            ok = ~np.isnan(want)
            assert (np.abs(got - want)[ok] <= fr.reference_bound(sca, p, n1)[ok]).all(), f"{p} SCA {k + 1}"
    for n in (64, 2, 1):   # s = 1, 32 and 64: one pixel a bin, and the whole frame one bin
        for j, p in enumerate(PTYPES):
            got = fr.bin_ref(scas[0]["dq"], fr.PIXELMASK1, [scas[0][p]], 64, n)[0][0]
            want = g[f"maps_sca1_n{n}"][j]
            ok = ~np.isnan(want)
            assert np.array_equal(np.isnan(got), ~ok) and (np.abs(got - want)[ok] <= fr.reference_bound(scas[0], p, n)[ok]).all(), (p, n)
    assert np.isnan(g["maps_sca1_n64"]).any()   # at s = 1 a masked pixel is an empty bin


def test_restatement_pictures_against_the_reference(g):
    scas, table, glyphs = fr.golden_scas(g), g["table"], g["glyphs"]
    for n1, key in ((int(g["n1"]), "rgb"), (32, "rgb_n32")):
        pic, _, owner, _ = fr.multi_image_ref(scas, n1, fr.PIXELMASK1, fr.SMALL, table, glyphs)
        fr.assert_picture(pic, g[key], owner, key)
    n1 = int(g["n1"])
    ny, nx, pos = fr.layout(n1, fr.SMALL)
    j = PTYPES.index("gain")
    maps = np.stack([np.zeros((n1, n1)) if s is None or "gain" not in s else fr.bin_ref(s["dq"], fr.PIXELMASK1, [s["gain"]], 64, n1)[0][0]
                     for s in scas])
    present = [s is not None and "gain" in s for s in scas]
    for key, fmt in (("gain_plain", None), ("gain_scale", "{:4.2f}")):
        pic, _, owner = fr.panel_ref(maps, present, 1.2, 2.1, n1, ny, nx, pos, table, glyphs, "gain", fmt)
        fr.assert_picture(pic, g[key], owner, key)
    # the pieces of the layout, named: white background, the bar's ends, a tick, text pixels, the gap between panels
    rgb = g["rgb"]
    assert (rgb[0, 0] == 255).all() and (rgb[ny:ny + 1 + n1 // 4] == 255).all() and (rgb[:, nx:nx + 1 + n1 // 4] == 255).all()
    assert (rgb[ny - 1, nx // 2 - n1] == table[0]).all() and (rgb[ny - 1, nx // 2 + n1 - 1] == table[255]).all()
    assert (rgb[ny - n1 // 8 - 1, nx // 2] == 0).all() and (rgb[ny - n1 // 8 - 1, nx // 2 + 1] != 0).any()
    assert np.count_nonzero((g["gain_scale"] != g["gain_plain"]).any(axis=2)) > 2 * n1 * (n1 // 8)   # bar, ticks and letters
    assert j == 2 and (rgb[:ny, :nx] != g["gain_scale"]).any()   # panel 0 is lin2, not gain


def test_recorded_checkpix(g):
    """the reference's workflow test looks at these pixels of the full-size picture (row, column, R, G, B; tolerance 16): kept as
    data; DESIGN.md 7 records the one comparison made with them"""
    cp = g["checkpix"]
    assert cp.shape == (6, 5) and cp.dtype == np.int16 and (cp[3] == [0, -1, 255, 255, 255]).all()


def test_layout_and_stamps_of_the_package_are_the_restatements(g):
    for n1 in (16, 32, 64):
        ny, nx, pos = fpaplot.panel_layout(n1, fr.SMALL)
        ry, rx, rpos = fr.layout(n1, fr.SMALL)
        assert (ny, nx) == (ry, rx) and np.array_equal(pos, rpos) and pos.dtype == np.int32
    assert fpaplot.panel_layout(128)[:2] == (516, 832)   # the full focal plane at the script's n1
    assert [tuple(p) for p in fpaplot.PANELS] == [tuple(p) for p in fr.PANELS] and fpaplot.LABEL == fr.LABELS
    glyphs = g["glyphs"]
    ny, nx, _ = fr.layout(16, fr.SMALL)
    for j, (ptype, vmin, vmax, fmt) in enumerate(fr.PANELS):
        blank = np.full((ny, nx, 3), 255, np.uint8)
        pic = fr.panel_ref(np.zeros((0, 16, 16)), [], vmin, vmax, 16, ny, nx, [], g["table"], glyphs, ptype, fmt)[0]
        bar = fr.panel_ref(np.zeros((0, 16, 16)), [], vmin, vmax, 16, ny, nx, [], g["table"], None, ptype, fmt)[0]
        for st in fpaplot.scale_stamps(j, 16, ny, nx, ptype, vmin, vmax, fmt):
            assert st[0] == j
            for c in range(3):
                fpaplot.write_text(bar[:, :, c], (st[1], st[2]), st[3], st[4], chr(st[5]), font=glyphs)
        assert np.array_equal(bar, pic) and (pic != blank).any()
    # a string that runs off the right edge loses its tail, letter by letter
    assert [s[2] for s in fpaplot.text_stamps(3, (40, 30), (5, 2), 1, 9, "abcdef")] == [2, 10, 18]
    assert fpaplot.text_stamps(0, (40, 30), (30, 2), 1, 9, "a") == [] and fpaplot.text_stamps(0, (40, 30), (4, 2), 2, 9, "ab")[0][3] == 2
    with pytest.raises(ValueError, match="font"):
        fpaplot.write_text(np.zeros((20, 20)), (0, 0), 1, 1, "a")
    with pytest.raises(ValueError, match="256 x 12 x 6"):
        fpaplot.load_font(np.zeros((12, 6)))


def test_shipped_colour_table(g):
    assert fpaplot.VIRIDIS.shape == (256, 3) and fpaplot.VIRIDIS.dtype == np.uint8
    assert np.array_equal(fpaplot.VIRIDIS, g["table"])   # made with matplotlib when the fixture was
    assert (np.abs(np.diff(fpaplot.VIRIDIS.astype(int), axis=0)).max(axis=0) == [3, 2, 2]).all()
    assert fpaplot.color_table("viridis") is fpaplot.VIRIDIS
    with pytest.raises(ValueError, match="no_such_map"):
        fpaplot.color_table("no_such_map")
    try:
        import matplotlib
    except ImportError:
        return
    assert np.array_equal(matplotlib.colormaps["viridis"](np.arange(256), bytes=True)[:, :3], fpaplot.VIRIDIS)
    assert np.array_equal(fpaplot.color_table("magma"), matplotlib.colormaps["magma"](np.arange(256), bytes=True)[:, :3])
    x = np.linspace(0.0, 1.0, 100001)   # the index rule of the render entry is the colour map's own
    assert np.array_equal(matplotlib.colormaps["viridis"](x, bytes=True)[:, :3], fpaplot.VIRIDIS[fr.color_index(x)])


def test_write_png_round_trip(tmp_path, g):
    arr = g["rgb"]
    path = str(tmp_path / "panel.png")
    calio.write_png(path, arr[::-1])
    assert np.array_equal(fr.read_png(path), arr[::-1])
    odd = np.random.default_rng(5).integers(0, 256, (7, 13, 3), dtype=np.uint8)
    calio.write_png(path, odd)
    assert np.array_equal(fr.read_png(path), odd)
    try:
        from PIL import Image
    except ImportError:
        pass
    else:
        assert np.array_equal(np.asarray(Image.open(path)), odd)
    for bad in (odd[:, :, :2], odd.astype(np.int16), odd[0]):
        with pytest.raises(ValueError, match="write_png"):
            calio.write_png(path, bad)


def test_reference_quirks_kept_without_a_device(tmp_path):
    fmt = str(tmp_path / "roman_wfi_{:s}_T_SCA{:02d}.asdf")
    with pytest.raises(KeyError):
        fpaplot.load_sca(fmt, 1, ["pflat"])
    assert fpaplot.load_sca(fmt, 1, ["gain", "read"]) is None   # no file: the caller draws zeros
    for shape in ((8,), (1, 1, 1, 8, 8)):
        with pytest.raises(ValueError, match="Incorrect array dimension"):
            fpaplot._plane_of(np.zeros(shape), "gain")
    cube = np.arange(4 * 3 * 3.0).reshape(4, 3, 3)
    assert np.array_equal(fpaplot._plane_of(cube, "lin2"), cube[2]) and np.array_equal(fpaplot._plane_of(cube, "lin3"), cube[3])
    k = np.arange(81.0).reshape(3, 3, 3, 3)
    assert np.array_equal(fpaplot._plane_of(k, "alphaH"), k[1, 0]) and np.array_equal(fpaplot._plane_of(k, "alphaV"), k[0, 1])
    assert np.array_equal(fpaplot._plane_of(k, "alphaD"), k[0, 0])
    calio.write_asdf(fmt.format("gain", 1), {"roman": {"data": np.ones((8, 8), np.float32)}})
    with pytest.raises((FileNotFoundError, OSError)):   # a data file without its mask file
        fpaplot.load_sca(fmt, 1, ["gain"])


def test_new_entries_are_declared_listed_and_exported():
    hdr = open(os.path.join(REPO, "include", "romanhip.h")).read()
    host = open(os.path.join(REPO, "romanimpreprocess_amd", "csrc", "rip_host.h")).read()
    mk = open(os.path.join(REPO, "romanimpreprocess_amd", "csrc", "Makefile")).read()
    assert "#define RIP_VERSION 100 " in hdr and "fpaplot.hip" in mk
    lib = _native.load_library()
    assert lib.rip_version() == 100
    for name, nargs in (("rip_fpa_bin", 13), ("rip_fpa_render", 21)):
        assert re.search(rf"\bint {name}\(", hdr) and name in host
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
        assert len(_native.SYMBOLS[name][1]) == nargs
    assert _native.RIP_FPA_MAX_PLANES == 8
