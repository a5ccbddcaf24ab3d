"""Host: the numpy restatement tests/visualize_ref.py against its witnesses (np.percentile; matplotlib where it is installed), the
PDF writer, and the host side of romanimpreprocess_amd.utils.visualize / utils.diff with the device calls stubbed out."""

import re
import zlib

import numpy as np
import pytest
import visualize_cases as vc
import visualize_ref as vr
from conftest import assert_same_bits

from romanimpreprocess_amd import calio
from romanimpreprocess_amd.utils import fpaplot, visualize

QS = (0, 100, 2, 98, 37.3, 50, 25, 2.0, 99.5)   # q = 50 of n = 3 and q = 25 of n = 5: the virtual index is an integer


# ---------------------------------------------------------------------------------------------- percentile
@pytest.mark.parametrize("n", [1, 2, 3, 5, 1000])
def test_restated_percentile_is_numpys(n):
    rng = np.random.default_rng(n)
    windows = [rng.standard_normal(n).astype(np.float32) * np.float32(1e3), rng.integers(0, 65536, n).astype(np.uint16).astype(np.float32),
               (rng.integers(0, 65536, n).astype(np.float32) - rng.integers(0, 65536, n).astype(np.float32)),
               np.full(n, 7.25, np.float32), np.repeat(rng.standard_normal((n + 1) // 2).astype(np.float32), 2)[:n]]
    for v in windows:
        s = vr.sorted_values(v)
        assert np.array_equal(s, np.sort(v))
        for q in QS:
            want = np.percentile(v, q)
            assert want.dtype == np.float32
            assert_same_bits(vr.percentile_from_sorted(s, q), want, f"n {n} q {q}")
            lo, hi, t = visualize.percentile_ranks(n, q)
            assert_same_bits(visualize.lerp(s[lo], s[hi], t), want, f"package: n {n} q {q}")


def test_restated_percentile_with_nan_and_infinities():
    v = np.array([1.0, np.inf, -np.inf, 3.0, 2.0], np.float32)
    for q in QS:
        with np.errstate(invalid="ignore"):
            want = np.percentile(v, q)
        assert_same_bits(vr.percentile_from_sorted(vr.sorted_values(v), q), want, f"q {q}")
    v[0] = np.nan
    with np.errstate(invalid="ignore"):
        assert np.isnan(vr.percentile_from_sorted(vr.sorted_values(v), 50.0)) and np.isnan(np.percentile(v, 50.0))


def test_sorted_values_tell_the_zeros_apart():
    v = np.array([0.0, -0.0, 1.0, -0.0, -1.0, 0.0], np.float32)
    assert vr.sorted_values(v).view(np.uint32).tolist() == np.array([-1.0, -0.0, -0.0, 0.0, 0.0, 1.0], np.float32).view(np.uint32).tolist()


def test_case_table_stays_small():
    for name, cube, (x0, x1, y0, y1), (g0, g1), minus in vc.SELECT_CASES:
        assert cube.ndim == 3 and all(a <= b for a, b in zip(cube.shape, vc.FULL)), name
        assert 0 <= x0 <= x1 < cube.shape[2] and 0 <= y0 <= y1 < cube.shape[1] and 0 <= g0 < g1 <= cube.shape[0], name
        assert minus is None or 0 <= minus < cube.shape[0], name


# ---------------------------------------------------------------------------------------------- matplotlib as the witness
def norm_inputs():
    rng = np.random.default_rng(3)
    lo, hi = np.float32(-12.3), np.float32(1000.7)   # hi - lo is no float32: Normalize's float64 quotient shows
    x = rng.uniform(-100.0, 1200.0, 20000).astype(np.float32)
    x[:12] = [lo, hi, np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf)), -1e30, 1e30, np.nan, np.inf, -np.inf,
              0.0, -0.0, lo + (hi - lo) * np.float32(37 / 256)]
    return x, lo, hi


def mpl_bytes(norm, x):
    """cmap(norm(x), bytes=True)[..., :3] over a white page: the bad colour is transparent"""
    import matplotlib
    rgba = matplotlib.colormaps["magma"](norm(x), bytes=True)
    return np.where(rgba[..., 3:] == 0, np.uint8(255), rgba[..., :3])


def test_restated_norms_and_colours_are_matplotlibs():
    colors = pytest.importorskip("matplotlib.colors")
    x, lo, hi = norm_inputs()
    for a, b in ((lo, hi), (np.float32(0.0), np.float32(1.0)), (np.float32(-3.0), np.float32(-3.0)), (np.float32(1e-3), np.float32(3e4))):
        for kind, norm in ((0, colors.Normalize(vmin=a, vmax=b)), (1, colors.PowerNorm(gamma=2.0 / 3.0, vmin=a, vmax=b))):
            t = vr.norm_ref(x, a, b, kind)
            assert_same_bits(t, np.asarray(norm(x).data, dtype=np.float32), f"norm {kind} {a}..{b}")
            assert np.array_equal(vr.colours(t, fpaplot.MAGMA), mpl_bytes(norm, x)), (kind, a, b)
    assert np.array_equal(vr.colours(np.array([np.nan], np.float32), fpaplot.MAGMA), [[255, 255, 255]])
    with pytest.raises(ValueError):
        colors.Normalize(vmin=2.0, vmax=1.0)(x)   # what rip_view_render refuses, matplotlib refuses too


def test_restated_bar_is_matplotlibs():
    matplotlib = pytest.importorskip("matplotlib")
    for h in (1, 2, 7, 256, 511):
        want = matplotlib.colormaps["magma"](np.linspace(0, 1, h), bytes=True)[:, :3]
        assert np.array_equal(vr.colours(np.linspace(0, 1, h), fpaplot.MAGMA), want), h


def test_magma_is_matplotlibs():
    matplotlib = pytest.importorskip("matplotlib")
    assert np.array_equal(fpaplot.MAGMA, matplotlib.colormaps["magma"](np.arange(256), bytes=True)[:, :3])
    assert fpaplot.color_table("magma") is fpaplot.MAGMA and fpaplot.MAGMA.shape == (256, 3) and fpaplot.MAGMA.dtype == np.uint8


def test_power_restatement_against_float64_pow_stays_inside_the_cap():
    """the restatement's float32 power against float64 pow on the power panels' inputs: its error is what POWER_SLACK_ULPS
    counts for numpy, and the pixels a slack of that size can move stay far below 1 % of a panel"""
    lo, hi = vc.POWER_LIMITS
    v = vc.POWER_CUBE[0]
    t = vr.norm_ref(v, lo, hi, 1)
    lin = (v - lo) / (hi - lo)
    pos = lin > 0
    exact = np.power(lin[pos].astype(np.float64), np.float64(np.float32(vr.GAMMA)))
    err = np.abs(t[pos].astype(np.float64) - exact) / np.spacing(exact.astype(np.float32)).astype(np.float64)
    print(f"float32 power against float64 pow: {err.max():.4f} ulp at most over {pos.sum()} values")
    assert 1.0 + err.max() < vr.POWER_SLACK_ULPS + 1   # with the device's 1 ulp: at most POWER_SLACK_ULPS representable steps apart
    moved = np.zeros(t.shape, bool)
    for k in (-vr.POWER_SLACK_ULPS, vr.POWER_SLACK_ULPS):
        moved |= vr.color_index(np.where(t > 0, vr.shift_ulps(t, k), t)) != vr.color_index(t)
    print(f"pixels within {vr.POWER_SLACK_ULPS} ulp of an index step: {moved.sum()} of {t.size}")
    assert moved.sum() < 0.01 * t.size
    true = lin.astype(np.float64)
    true[pos] = exact
    differ = vr.color_index(true) != vr.color_index(t)
    print(f"pixels whose index differs from that of float64 pow: {differ.sum()} of {t.size}")
    assert differ.sum() < 0.01 * t.size


# ---------------------------------------------------------------------------------------------- PDF
def test_write_pdf_image_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (23, 41, 3), dtype=np.uint8)
    path = tmp_path / "p.pdf"
    calio.write_pdf_image(path, img)
    raw = path.read_bytes()
    assert raw.startswith(b"%PDF-") and raw.endswith(b"%%EOF")
    m = re.search(rb"/Subtype /Image /Width (\d+) /Height (\d+) /ColorSpace /DeviceRGB /BitsPerComponent 8 /Filter /FlateDecode /Length (\d+) >>\nstream\n",
                  raw)
    nx, ny, n = (int(g) for g in m.groups())
    assert (ny, nx) == img.shape[:2]
    stream = raw[m.end():m.end() + n]
    assert raw[m.end() + n:].startswith(b"\nendstream")
    assert np.array_equal(np.frombuffer(zlib.decompress(stream), np.uint8).reshape(ny, nx, 3), img)
    xref = int(re.search(rb"startxref\n(\d+)\n%%EOF$", raw)[1])
    assert raw[xref:xref + 4] == b"xref"
    for i, off in enumerate(re.findall(rb"(\d{10}) 00000 n \n", raw)):   # every object where the table says
        assert raw[int(off):].startswith(b"%d 0 obj\n" % (i + 1))
    assert raw.count(b" 0 obj\n") == 5 and b"/MediaBox [0 0 41 23]" in raw
    with pytest.raises(ValueError):
        calio.write_pdf_image(path, img[..., 0])


# ---------------------------------------------------------------------------------------------- the host side, device stubbed
@pytest.fixture
def stub(monkeypatch):
    """window_ranks and render answered by the restatement / recorded: no GPU"""
    calls = {"ranks": [], "render": []}

    def window_ranks(cube, window, g0, g1, minus, ranks, ctx=None):
        calls["ranks"].append((tuple(cube.shape), tuple(window), g0, g1, minus, list(ranks)))
        s = vr.sorted_values(vr.window_values(np.asarray(cube), window, g0, g1, minus))
        return s[np.asarray(ranks, dtype=np.int64)], int(np.isnan(s).sum())

    def render(cube, window, panels, limits, zoom, cell, shape, table=None, font=None, stamps=(), ctx=None, out=None):
        calls["render"].append(dict(cube=tuple(cube.shape), window=tuple(window), panels=[list(p) for p in panels],
                                    limits=[list(v) for v in limits], zoom=zoom, cell=tuple(cell), shape=tuple(shape), stamps=list(stamps)))
        img = np.zeros((shape[0], shape[1], 3), np.uint8)
        img[0, :, 0] = 200   # the bottom row is told apart
        return img

    monkeypatch.setattr(visualize, "window_ranks", window_ranks)
    monkeypatch.setattr(visualize, "render", render)
    return calls


def test_block_percentiles_through_the_stub_are_numpys(stub):
    cube = vc.f32_cube(31, (4, 20, 30))
    w = (3, 17, 2, 11)
    data = vr.window_values(cube, w, 0, 4)
    got = visualize.block_percentiles(cube, w, list(QS))
    assert got.dtype == np.float32 and got.shape == (len(QS),)
    for g, q in zip(got, QS):
        assert_same_bits(g, np.percentile(data, q), f"q {q}")
    assert len(stub["ranks"]) == 3 and all(len(c[5]) <= 8 for c in stub["ranks"])   # 9 percentiles, 4 a call
    one = visualize.block_percentiles(cube, w, 98.0, planes=(3, 4), minus=1)
    assert_same_bits(one, np.percentile(data[3] - data[1], 98.0), "one plane minus another")
    cube[2, 5, 5] = np.nan
    assert np.isnan(visualize.block_percentiles(cube, w, 50.0)) and not np.isnan(visualize.block_percentiles(cube, w, 50.0, planes=(0, 2)))
    with pytest.raises(ValueError, match="range"):
        visualize.block_percentiles(cube, w, 101.0)


def test_visualize_cube_panels_limits_and_bounds(stub):
    cube = vc.u16_cube(32, (4, 20, 30))
    img, limits = visualize.visualize_cube(cube, (25, 40, 15, 99), percentile_cut=5.0)   # the upper bounds are clamped at the frame
    call = stub["render"][0]
    assert call["window"] == (25, 29, 15, 19) and call["zoom"] == 512 // 5 and call["cube"] == (4, 20, 30)
    _, want, rows, _ = vr.visualize_ref(cube, (25, 40, 15, 99), 5.0, fpaplot.MAGMA)
    assert list(limits) == list(want) == ["Group 0", "Group 1", "Group 2", "Group 3", "Grp0-Grp1", "Grp2-Grp1", "Grp3-Grp1"]
    for k in want:
        assert_same_bits(np.array(limits[k], np.float32), np.array(want[k], np.float32), k)
        assert all(isinstance(v, np.float32) for v in limits[k])
    assert [p[:5] for p in call["panels"]] == [r[1:6] for r in rows] and all(p[5] == 1 for p in call["panels"])
    ch, cw, ny, nx = vr.layout(4, 5, 5, call["zoom"], False)
    assert call["cell"] == (ch, cw) and call["shape"][:2] == (ny, nx) and img.shape == (ny, nx, 3) and call["stamps"] == []
    # two groups: no power panel, but the last difference's percentile is still taken
    stub["ranks"].clear()
    _, limits = visualize.visualize_cube(cube[:2], (0, 29, 0, 19), zoom=1)
    assert list(limits) == ["Group 0", "Group 1", "Grp0-Grp1"] and stub["ranks"][-1][2:5] == (1, 2, 1) and stub["render"][-1]["zoom"] == 1
    for bad in ((-1, 5, 0, 5), (0, 5, -2, 5), (6, 5, 0, 5), (0, 5, 7, 6), (30, 31, 0, 5), (0, 5, 20, 25)):
        with pytest.raises(ValueError):
            visualize.visualize_cube(cube, bad)
    with pytest.raises(IndexError):
        visualize.visualize_cube(cube[:1], (0, 5, 0, 5))
    with pytest.raises(ValueError, match="zoom"):
        visualize.visualize_cube(cube, (0, 5, 0, 5), zoom=0)
    with pytest.raises(ValueError, match="uint16 or float32"):
        visualize.visualize_cube(cube[0], (0, 5, 0, 5))
    assert visualize.default_zoom(4096, 10) == 1 and visualize.default_zoom(512, 512) == 1 and visualize.default_zoom(100, 171) == 2


def test_visualize_cube_stamps_with_a_font(stub):
    glyphs = np.ones((256, 12, 6), np.uint8)
    cube = vc.u16_cube(33, (3, 40, 30))
    visualize.visualize_cube(cube, (0, 29, 0, 39), font=glyphs, zoom=1)
    call = stub["render"][0]
    ch, cw, ny, nx = vr.layout(3, 30, 40, 1, True)
    assert call["cell"] == (ch, cw) == (40 + vr.TITLE_H, 30 + vr.BAR_GAP + vr.BAR_W + vr.TICK + vr.LABEL_W) and call["shape"][:2] == (ny, nx)
    by_panel = {p: "".join(chr(s[5]) for s in call["stamps"] if s[0] == p and s[1] == 42) for p in range(5)}
    assert by_panel == {0: "Group 0", 1: "Group 1", 2: "Group 2", 3: "Grp0-Grp1", 4: "Grp2-Grp1"}
    lo, hi = call["limits"][0][:2]
    x = 30 + vr.BAR_GAP + vr.BAR_W + vr.TICK + 1
    assert "".join(chr(s[5]) for s in call["stamps"] if s[0] == 0 and s[1] == 0) == f"{lo:.4g}"
    assert "".join(chr(s[5]) for s in call["stamps"] if s[0] == 0 and s[1] == 28) == f"{hi:.4g}"
    assert all(s[2] >= x for s in call["stamps"] if s[1] in (0, 28)) and all(s[3] == 1 and s[4] == 0 for s in call["stamps"])


def test_visualize_script_arguments(stub, tmp_path, capsys):
    cube = vc.u16_cube(34, (3, 50, 60))
    path = str(tmp_path / "l1.asdf")
    calio.write_asdf(path, {"roman": {"data": cube}})
    assert visualize.visualize(["visualize.py", path, "1,2,3,4"]) is None
    text = capsys.readouterr().out
    assert "This is a simple visualization script." in text and "xmin,xmax,ymin,ymax outfile.pdf [percentile_cut]" in text
    assert not stub["render"]
    import fpaplot_ref
    png, pdf = str(tmp_path / "o.png"), str(tmp_path / "o.PDF")
    visualize.visualize(["visualize.py", path, "10,20,30,45", png, "7.5"])
    call = stub["render"][-1]
    assert call["cube"] == (3, 16, 60) and call["window"] == (10, 20, 0, 15), "only the window's rows travel"
    want = np.percentile(cube[:, 30:46, 10:21].astype(np.float32), 7.5)
    assert_same_bits(np.float32(call["limits"][0][0]), want, "percentile_cut from argv")
    pic = fpaplot_ref.read_png(png)
    assert (pic[-1, :, 0] == 200).all() and not pic[0].any(), "the rows are written top first"
    visualize.visualize(["visualize.py", path, "10,20,30,99", pdf])   # ymax clamped; the default cut
    assert stub["render"][-1]["cube"] == (3, 20, 60) and open(pdf, "rb").read(5) == b"%PDF-"
    assert_same_bits(np.float32(stub["render"][-1]["limits"][0][0]), np.percentile(cube[:, 30:, 10:21].astype(np.float32), 2.0), "default cut")
    n = len(stub["render"])
    for args, exc, match in ((["v", path, "1,2,3,4", str(tmp_path / "o.jpg")], ValueError, r"\.png or \.pdf"),
                             (["v", path, "-1,2,3,4", png], ValueError, "negative"), (["v", path, "5,2,3,4", png], ValueError, "empty"),
                             (["v", path, "1,2,50,60", png], ValueError, "outside the frame"), (["v", path, "60,70,3,4", png], ValueError, "empty")):
        with pytest.raises(exc, match=match):
            visualize.visualize(args)
    assert len(stub["render"]) == n
    font = str(tmp_path / "letters.dat")
    np.savetxt(font, np.ones((256 * 12, 6)), fmt="%d")
    visualize.main(["visualize.py", path, "--font", font, "0,5,0,5", png, "3"])   # the option may stand anywhere
    assert stub["render"][-1]["stamps"] and stub["render"][-1]["window"] == (0, 5, 0, 5)
    assert_same_bits(np.float32(stub["render"][-1]["limits"][0][0]), np.percentile(cube[:, :6, :6].astype(np.float32), 3.0), "cut beside --font")


def test_diff_script_usage_and_indices(capsys):
    from romanimpreprocess_amd.utils import diff
    assert diff.diff(["diff.py", "a", "b", "1"]) is None
    assert capsys.readouterr().out.strip() == "Calling format: python diff.py <asdf in> <fits out> <group1> <group2>"
