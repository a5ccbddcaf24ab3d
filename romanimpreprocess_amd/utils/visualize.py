"""Quick look at a window of a Level-1 cube on the GPU -- the reference's ``utils/visualize.py`` (line numbers below are that
file's): every group of the window under one percentile stretch, and its differences against group 1.

The cube (uint16 or float32) is read where it lies, in host memory or in HBM.  The percentiles are exact order statistics of
the window (``rip_view_ranks``: no float32 copy, no sort), interpolated on the host as ``np.percentile`` does; one
``rip_view_render`` call then draws the whole picture, which is downloaded once.  The reference casts the window to float32,
sorts it five times and hands matplotlib a vector figure.

The panels and stretches are those of :58-111.  Top row: ``Group j`` for every group, all under the window's own
``percentile_cut`` / ``100 - percentile_cut`` percentiles.  Bottom row: ``Grp0-Grp1`` under its own two percentiles; nothing
under group 1; ``Grpj-Grp1`` for j >= 2 under ``PowerNorm(gamma=2/3)`` with ``vmax = percentile(Grp(ng-1)-Grp1, 100 - cut)`` and
``vmin = -0.05 vmax``.  The colour map is ``magma``.

Deviations, on purpose: the result is a raster (an (H, W, 3) uint8 array, PNG or a one-page PDF that holds that raster), not
matplotlib's vector figure with TeX labels; axis labels are not drawn; and the layout is this package's own:

  * every sample is ``zoom`` x ``zoom`` pixels (default: the largest integer with ``zoom * max(dx, dy) <= 512``, at least 1);
  * a panel is a cell: the window from the cell's lower left corner; ``BAR_GAP`` = 4 columns right of it the colour bar,
    ``BAR_W`` = 8 columns wide and as high as the window, ``linspace(0, 1, height)`` from the bottom; right of the bar three ticks
    (``TICK`` = 3 columns, one row) at its bottom, middle and top row;
  * with a font the cell has ``TITLE_H`` = 14 more rows above the window for the title (2 rows above it) and ``LABEL_W`` = 80 more
    columns right of the ticks for the bar's end values (``"{:.4g}"``: vmin at the bottom row, vmax 12 rows below the top where
    the bar is at least 25 rows high), all in glyph cells of one pixel; without a font there are bars and ticks and no text;
  * the cells stand ``GAP`` = 8 pixels apart, the difference row below the group row.

As with ``utils/fpaplot.py``, row 0 of the returned picture is its BOTTOM row; ``visualize`` writes the rows top first.

``python -m romanimpreprocess_amd.utils.visualize infile.asdf xmin,xmax,ymin,ymax outfile.{png,pdf} [percentile_cut] [--font FILE]``
"""

import sys

import numpy as np

from .. import _native, calio
from ..devarray import is_dev
from . import fpaplot

GAP, BAR_GAP, BAR_W, TICK, TITLE_H, LABEL_W = 8, 4, 8, 3, 14, 80
GAMMA = 2.0 / 3.0
USAGE = ("This is a simple visualization script.\n"
         "Calling format: python visualize.py infile.asdf xmin,xmax,ymin,ymax outfile.pdf [percentile_cut]")


# ---------------------------------------------------------------------------------------------- the two device calls
def _cube(cube):
    """the cube as the library takes it: a DevArray as it is, anything else as a C-contiguous uint16 or float32 array"""
    if not is_dev(cube):
        cube = np.asarray(cube)
        cube = np.ascontiguousarray(cube if cube.dtype in (np.uint16, np.float32) else cube.astype(np.float32))
    if cube.ndim != 3 or cube.dtype not in (np.uint16, np.float32):
        raise ValueError(f"visualize: the cube is {cube.dtype}{tuple(cube.shape)}, expected uint16 or float32 (ng, ny, nx)")
    return cube


def window_ranks(cube, window, g0, g1, minus, ranks, ctx=None):
    """``rip_view_ranks``: (the float32 elements of the 0-based ``ranks`` (at most 8) in ascending order, the number of NaNs) of the
    window ``(x0, x1, y0, y1)`` (inclusive) of the planes ``g0 .. g1 - 1``, each minus plane ``minus`` where that is not None"""
    ctx = ctx or _native.default_context()
    cube = _cube(cube)
    x0, x1, y0, y1 = window
    ranks = np.ascontiguousarray(ranks, dtype=np.uint32)
    values, nan = np.empty(len(ranks), np.float32), np.zeros(1, np.uint32)
    ctx.call("rip_view_ranks", cube, _native.dtype_code(cube), _native.location_of(cube), *cube.shape, y0, y1, x0, x1, g0, g1,
             -1 if minus is None else minus, len(ranks), ranks, values, nan)
    return values, int(nan[0])


def render(cube, window, panels, limits, zoom, cell, shape, table=None, font=None, stamps=(), ctx=None, out=None):
    """``rip_view_render``: the (NY, NX, 3) uint8 picture ``shape`` of the panels ``panels`` (rows of [plane, minus or -1, norm
    kind, y, x, colour bar]) with ``limits`` (rows of [vmin, vmax, gamma]), every panel a cell of ``cell`` = (height, width)
    pixels; ``stamps`` are drawn only with ``font``.  ``out``: a uint8 ``DevArray`` to draw into instead (it is returned, and
    nothing is downloaded)."""
    ctx = ctx or _native.default_context()
    cube = _cube(cube)
    x0, x1, y0, y1 = window
    panels = np.ascontiguousarray(panels, dtype=np.int32).reshape(-1, 6)
    limits = np.ascontiguousarray(limits, dtype=np.float32).reshape(-1, 3)
    if len(panels) != len(limits):
        raise ValueError(f"visualize: {len(panels)} panels, {len(limits)} rows of limits")
    glyphs = fpaplot.load_font(font)
    st = np.ascontiguousarray(np.asarray(list(stamps) if glyphs is not None else [], dtype=np.int32).reshape(-1, 6))
    shape = (int(shape[0]), int(shape[1]), 3)
    img = out if out is not None else np.empty(shape, np.uint8)
    if tuple(img.shape) != shape:
        raise ValueError(f"visualize: the picture is {shape}, out is {tuple(img.shape)}")
    ctx.call("rip_view_render", cube, _native.dtype_code(cube), _native.location_of(cube), *cube.shape, y0, y1, x0, x1, len(panels),
             panels, limits, zoom, BAR_GAP, BAR_W, TICK, cell[0], cell[1], shape[0], shape[1],
             np.ascontiguousarray(fpaplot.MAGMA if table is None else table, dtype=np.uint8).reshape(256, 3), glyphs, len(st),
             st if len(st) else None, img, _native.location_of(img))
    return img


# ---------------------------------------------------------------------------------------------- percentiles
def percentile_ranks(n, q):
    """What ``np.percentile(a, q)`` (method "linear") of ``n`` float32 values needs of their sorted order: the two 0-based ranks
    and the float32 weight of the upper one, in numpy's own arithmetic for float32 input -- the quantile ``q / float32(100)``
    and the virtual index ``(n - 1) * quantile`` are float32."""
    quantile = np.true_divide(q, np.float32(100))
    if not 0.0 <= quantile <= 1.0:
        raise ValueError("Percentiles must be in the range [0, 100]")
    virtual = np.float32((n - 1) * quantile)
    if virtual >= n - 1:
        return n - 1, n - 1, np.float32(0.0)
    below = np.floor(virtual)   # float32, and so is numpy's "next index" below + 1
    return int(below), min(int(below + 1), n - 1), np.float32(virtual - below)


def lerp(a, b, t):
    """numpy's ``_lerp`` on float32 scalars: ``a + (b - a) t``, from the other end where ``t >= 0.5``"""
    a, b, t = np.float32(a), np.float32(b), np.float32(t)
    with np.errstate(invalid="ignore", over="ignore"):
        d = b - a
        return np.float32(b - d * (np.float32(1) - t)) if t >= 0.5 else np.float32(a + d * t)


def _window(shape, bounds):
    """(x0, x1, y0, y1) of ``bounds`` = (xmin, xmax, ymin, ymax) in a frame of ``shape``: an upper bound past the frame is clamped,
    as the reference's slice does; a negative bound or an empty window raises"""
    xmin, xmax, ymin, ymax = (int(b) for b in bounds)
    if min(xmin, xmax, ymin, ymax) < 0:
        raise ValueError(f"visualize: negative bound in {xmin},{xmax},{ymin},{ymax}")
    xmax, ymax = min(xmax, shape[-1] - 1), min(ymax, shape[-2] - 1)
    if xmax < xmin or ymax < ymin:
        raise ValueError(f"visualize: the window {xmin},{xmax},{ymin},{ymax} of the frame {tuple(shape[-2:])} is empty")
    return xmin, xmax, ymin, ymax


def block_percentiles(cube, bounds, q, planes=None, minus=None, ctx=None):
    """``np.percentile(data[g0:g1, ymin:ymax+1, xmin:xmax+1].astype(np.float32) - data[minus, ...], q)`` of a numpy array or a
    ``DevArray`` (ng, ny, nx): a float32 scalar, or an array of them where ``q`` is a sequence.  ``bounds`` = (xmin, xmax, ymin,
    ymax), ``planes`` = (g0, g1) or None for all, ``minus`` a plane or None.  NaN where the window holds a NaN, as numpy."""
    cube = _cube(cube)
    win = _window(cube.shape, bounds)
    g0, g1 = (0, cube.shape[0]) if planes is None else (int(planes[0]), int(planes[1]))
    n = (g1 - g0) * (win[3] - win[2] + 1) * (win[1] - win[0] + 1)
    qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
    parts = [percentile_ranks(n, float(x)) for x in qs]
    out = np.empty(len(qs), np.float32)
    per = _native.RIP_VIEW_MAX_RANKS // 2
    for at in range(0, len(qs), per):
        some = parts[at:at + per]
        values, nan = window_ranks(cube, win, g0, g1, minus, [r for lo, hi, _ in some for r in (lo, hi)], ctx)
        for i, (_, _, t) in enumerate(some):
            out[at + i] = np.nan if nan else lerp(values[2 * i], values[2 * i + 1], t)
    return out[0] if np.ndim(q) == 0 else out


# ---------------------------------------------------------------------------------------------- the picture
def default_zoom(dx, dy):
    return max(1, 512 // max(dx, dy))


def layout(ng, dx, dy, zoom, text):
    """(cell height, cell width, picture height, picture width, [(y, x) of the group cells], [(y, x) of the difference cells]) of
    the module docstring's layout; ``text``: a font is given"""
    h, w = zoom * dy, zoom * dx
    ch, cw = h + (TITLE_H if text else 0), w + BAR_GAP + BAR_W + TICK + (LABEL_W if text else 0)
    xs = [j * (cw + GAP) for j in range(ng)]
    return ch, cw, 2 * ch + GAP, ng * cw + (ng - 1) * GAP, [(ch + GAP, x) for x in xs], [(0, x) for x in xs]


def cell_stamps(panel, ch, cw, h, w, title, vmin, vmax):
    """the letters of one panel: its title and the end values of its bar"""
    x = w + BAR_GAP + BAR_W + TICK + 1
    out = fpaplot.text_stamps(panel, (ch, cw), (h + 2, 0), 1, 0, title) + fpaplot.text_stamps(panel, (ch, cw), (0, x), 1, 0, f"{vmin:.4g}")
    if h >= 25:
        out += fpaplot.text_stamps(panel, (ch, cw), (h - 12, x), 1, 0, f"{vmax:.4g}")
    return out


def visualize_cube(cube, bounds, percentile_cut=2.0, font=None, zoom=None, ctx=None):
    """The picture of :58-111 for the window ``bounds`` = (xmin, xmax, ymin, ymax) of ``cube`` (ng, ny, nx), uint16 or float32, a
    numpy array or a ``DevArray``: ((H, W, 3) uint8, row 0 at the bottom; {title: (vmin, vmax)} of every panel).  ``font``: as
    ``fpaplot.load_font``.  ``ng < 2`` raises ``IndexError``, as ``data[1]`` does; a stretch that matplotlib refuses (vmin > vmax
    or not finite, as under a NaN in the window) raises ``ValueError``."""
    cube = _cube(cube)
    ng = cube.shape[0]
    win = _window(cube.shape, bounds)
    if ng < 2:
        raise IndexError(f"index 1 is out of bounds for axis 0 with size {ng}")
    cut = float(percentile_cut)
    dx, dy = win[1] - win[0] + 1, win[3] - win[2] + 1
    zoom = default_zoom(dx, dy) if zoom is None else int(zoom)
    if zoom < 1:
        raise ValueError(f"visualize: zoom {zoom} is below 1")
    vmin, vmax = block_percentiles(cube, win, [cut, 100.0 - cut], ctx=ctx)
    dmin, dmax = block_percentiles(cube, win, [cut, 100.0 - cut], planes=(0, 1), minus=1, ctx=ctx)
    pmax = block_percentiles(cube, win, 100.0 - cut, planes=(ng - 1, ng), minus=1, ctx=ctx)
    pmin = np.float32(-0.05) * pmax   # -0.05 * vmax of a float32 scalar is float32 arithmetic
    glyphs = fpaplot.load_font(font)
    ch, cw, ny, nx, top, bottom = layout(ng, dx, dy, zoom, glyphs is not None)
    rows = [(f"Group {j:d}", j, -1, 0, top[j], vmin, vmax) for j in range(ng)]
    rows.append(("Grp0-Grp1", 0, 1, 0, bottom[0], dmin, dmax))
    rows += [(f"Grp{j:d}-Grp1", j, 1, 1, bottom[j], pmin, pmax) for j in range(2, ng)]
    stamps = []
    if glyphs is not None:
        for p, (title, _, _, _, _, lo, hi) in enumerate(rows):
            stamps += cell_stamps(p, ch, cw, zoom * dy, zoom * dx, title, lo, hi)
    img = render(cube, win, [[g, m, kind, y, x, 1] for _, g, m, kind, (y, x), _, _ in rows],
                 [[lo, hi, GAMMA] for *_, lo, hi in rows], zoom, (ch, cw), (ny, nx), font=glyphs, stamps=stamps, ctx=ctx)
    return img, {title: (lo, hi) for title, *_, lo, hi in rows}


def read_window_rows(path, ymin, ymax):
    """rows ymin .. ymax (clamped at the frame) of ``roman.data`` of an ASDF file as a uint16 or float32 array (ng, rows, nx)"""
    with calio.open_tree(path) as f:
        data = f["roman"]["data"]
        if len(data.shape) != 3:
            raise ValueError(f"visualize: roman.data of {path} has the shape {tuple(data.shape)}, expected (ng, ny, nx)")
        return _cube(np.asarray(data[:, ymin:min(ymax, data.shape[1] - 1) + 1, :]))


def visualize(argv, font=None, ctx=None):
    """Visualizes a block of an ASDF file.  ``argv``: [dummy, input_file, "xmin,xmax,ymin,ymax", outfile, percentile_cut
    (optional)], as the reference's; ``outfile`` ends in ``.png`` or ``.pdf``.  Only the window's rows travel to the device."""
    if len(argv) < 4:
        print(USAGE)
        return
    xmin, xmax, ymin, ymax = (int(b) for b in argv[2].split(",")[:4])
    out = str(argv[3])
    if not out.lower().endswith((".png", ".pdf")):
        raise ValueError(f"visualize: the output file {out!r} must end in .png or .pdf")
    if min(xmin, xmax, ymin, ymax) < 0 or xmax < xmin or ymax < ymin:
        raise ValueError(f"visualize: the window {xmin},{xmax},{ymin},{ymax} is empty or has a negative bound")
    rows = read_window_rows(argv[1], ymin, ymax)
    if rows.shape[1] < 1:
        raise ValueError(f"visualize: the window {xmin},{xmax},{ymin},{ymax} is empty: it lies outside the frame")
    cut = float(argv[4]) if len(argv) > 4 else 2.0
    img, _ = visualize_cube(rows, (xmin, xmax, 0, rows.shape[1] - 1), percentile_cut=cut, font=font, ctx=ctx)
    (calio.write_png if out.lower().endswith(".png") else calio.write_pdf_image)(out, img[::-1])


def main(argv=None):
    argv = list(sys.argv if argv is None else argv)
    font = None
    if "--font" in argv:
        at = argv.index("--font")
        if at + 1 >= len(argv):
            raise SystemExit("--font needs a file")
        font = argv[at + 1]
        del argv[at:at + 2]
    visualize(argv, font=font)


if __name__ == "__main__":
    main()
