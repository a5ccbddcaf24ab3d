"""numpy restatement of romanimpreprocess_amd.utils.visualize (the reference's utils/visualize.py:46-111) for the tests: the
window's values, sorted order -> percentile, both norms, the colour index rule, the colour bar, a panel's cell and the whole
picture.  Everything here is host numpy; the percentile of the end-to-end picture is np.percentile itself.

The layout is restated on purpose (not imported): cells GAP apart, difference row below the group row; in a cell the window
zoomed from the lower left corner, BAR_GAP columns, a bar of BAR_W columns as high as the window, three ticks of TICK columns and
one row at the bar's bottom, middle and top row; with a font TITLE_H rows above the window and LABEL_W columns right of the
ticks.  Row 0 of a picture is its bottom row."""

import numpy as np

GAP, BAR_GAP, BAR_W, TICK, TITLE_H, LABEL_W = 8, 4, 8, 3, 14, 80
GAMMA = 2.0 / 3.0


# ---------------------------------------------------------------------------------------------- values and their order
def window_values(cube, window, g0, g1, minus=None):
    """data[g0:g1, ymin:ymax+1, xmin:xmax+1].astype(float32) [- data[minus]] (visualize.py:46, :77)"""
    x0, x1, y0, y1 = window
    v = cube[g0:g1, y0:y1 + 1, x0:x1 + 1].astype(np.float32)
    if minus is not None:
        with np.errstate(invalid="ignore"):
            v = v - cube[minus, y0:y1 + 1, x0:x1 + 1].astype(np.float32)[None]
    return v


def keys(v):
    """the order-preserving uint32 key of float32 values: -0 just below +0, NaNs beyond the infinities on the side of their sign"""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).ravel()
    return np.where(b >> 31, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def sorted_values(v):
    """the values in the order of their keys: np.sort, with the zeros told apart by their sign"""
    k = np.sort(keys(v))
    return np.where(k >> 31, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def percentile_ranks(n, q):
    """the two ranks and the float32 weight np.percentile(method="linear") uses for n float32 values"""
    quantile = np.true_divide(q, np.float32(100))
    virtual = np.float32((n - 1) * quantile)
    if virtual >= n - 1:
        return n - 1, n - 1, np.float32(0)
    below = np.floor(virtual)
    return int(below), min(int(below + 1), n - 1), np.float32(virtual - below)


def percentile_from_sorted(s, q):
    """np.percentile(values, q) from the sorted float32 values s"""
    if np.isnan(s).any():
        return np.float32(np.nan)
    lo, hi, t = percentile_ranks(len(s), q)
    a, b = s[lo], s[hi]
    with np.errstate(invalid="ignore", over="ignore"):
        d = b - a
        return np.float32(b - d * (1 - t)) if t >= 0.5 else np.float32(a + d * t)


# ---------------------------------------------------------------------------------------------- norms and colours
def norm_ref(v, vmin, vmax, kind, gamma=GAMMA):
    """matplotlib's Normalize (kind 0) / PowerNorm (kind 1) of float32 data for float32-representable bounds, as float32"""
    v = np.array(v, dtype=np.float32)
    vmin, vmax = np.float32(vmin), np.float32(vmax)
    if vmin == vmax:
        return np.zeros_like(v)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = v - vmin
        if kind == 0:
            return (t.astype(np.float64) / (np.float64(vmax) - np.float64(vmin))).astype(np.float32)
        t /= (vmax - vmin)
        t[t > 0] = np.power(t[t > 0], float(gamma))
    return t


def color_index(t):
    """cmap(t, bytes=True)'s index into a 256-entry table, in t's own precision; -1 for NaN (the bad colour)"""
    t = np.asarray(t)
    with np.errstate(invalid="ignore", over="ignore"):
        x = t * t.dtype.type(256)
        idx = np.where(x < 0, 0, np.where(x >= 256, 255, np.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64)))
    return np.where(np.isnan(t), -1, idx)


def colours(t, table):
    """the RGB bytes of normalised values: NaN is white (magma's bad colour is transparent over a white page)"""
    idx = color_index(t)
    return np.where((idx < 0)[..., None], np.uint8(255), table[np.maximum(idx, 0)])


def shift_ulps(t, k):
    """float32 values moved k representable steps (k < 0: down)"""
    t = np.array(t, dtype=np.float32)
    for _ in range(abs(k)):
        t = np.nextafter(t, np.float32(np.inf if k > 0 else -np.inf))
    return t


# ---------------------------------------------------------------------------------------------- cells and pictures
def layout(ng, dx, dy, zoom, text):
    h, w = zoom * dy, zoom * dx
    ch, cw = h + (TITLE_H if text else 0), w + BAR_GAP + BAR_W + TICK + (LABEL_W if text else 0)
    return ch, cw, 2 * ch + GAP, ng * cw + (ng - 1) * GAP


def stamp(cell, glyphs, y, x, size, val, code):
    on = np.kron(glyphs[code][::-1] > 0, np.ones((size, size), bool))
    cell[y:y + 12 * size, x:x + 6 * size][on] = val


def text(cell, glyphs, y, x, string):
    """letters of size 1, black, advance 8; the rest is dropped once a letter does not fit"""
    for ch in string:
        if x + 6 > cell.shape[1] or y + 12 > cell.shape[0]:
            break
        stamp(cell, glyphs, y, x, 1, 0, ord(ch))
        x += 8


def render_ref(cube, window, panels, limits, zoom, cell, shape, table, glyphs=None, stamps=()):
    """the picture of rip_view_render and, per panel, the float32 normalised window (before the index rule)"""
    x0, x1, y0, y1 = window
    ch, cw = cell
    h, w = zoom * (y1 - y0 + 1), zoom * (x1 - x0 + 1)
    img = np.full((shape[0], shape[1], 3), 255, np.uint8)
    normed = []
    for p, ((g, minus, kind, y, x, bar), (lo, hi, gamma)) in enumerate(zip(panels, limits)):
        c = np.full((ch, cw, 3), 255, np.uint8)
        t = norm_ref(window_values(cube, window, g, g + 1, None if minus < 0 else minus)[0], lo, hi, kind, gamma)
        normed.append(t)
        c[:h, :w] = np.repeat(np.repeat(colours(t, table), zoom, axis=0), zoom, axis=1)
        if bar:
            c[:h, w + BAR_GAP:w + BAR_GAP + BAR_W] = colours(np.linspace(0, 1, h), table)[:, None, :]
            for row in (0, h // 2, h - 1):
                c[row, w + BAR_GAP + BAR_W:w + BAR_GAP + BAR_W + TICK] = 0
        if glyphs is not None:
            for sp, sy, sx, size, val, code in stamps:
                if sp == p:
                    stamp(c, glyphs, sy, sx, size, val, code)
        img[y:y + ch, x:x + cw] = c
    return img, normed


def visualize_ref(cube, bounds, cut, table, glyphs=None, zoom=None):
    """the picture of visualize_cube from np.percentile itself: (picture, {title: (vmin, vmax)}, panel rows [title, plane, minus,
    kind, y, x], normalised windows)"""
    ng, ny, nx = cube.shape
    xmin, xmax, ymin, ymax = bounds
    window = (xmin, min(xmax, nx - 1), ymin, min(ymax, ny - 1))
    data = window_values(cube, window, 0, ng)
    dx, dy = data.shape[2], data.shape[1]
    zoom = max(1, 512 // max(dx, dy)) if zoom is None else zoom
    vmin, vmax = np.percentile(data, cut), np.percentile(data, 100 - cut)
    with np.errstate(invalid="ignore"):
        diff = data - data[1][None]
    dmax, dmin = np.percentile(diff[0], 100 - cut), np.percentile(diff[0], cut)
    pmax = np.percentile(diff[-1], 100 - cut)
    pmin = -0.05 * pmax
    ch, cw, NY, NX = layout(ng, dx, dy, zoom, glyphs is not None)
    col = lambda j: j * (cw + GAP)   # noqa: E731
    rows = [[f"Group {j:d}", j, -1, 0, ch + GAP, col(j), vmin, vmax] for j in range(ng)]
    rows.append(["Grp0-Grp1", 0, 1, 0, 0, 0, dmin, dmax])
    rows += [[f"Grp{j:d}-Grp1", j, 1, 1, 0, col(j), pmin, pmax] for j in range(2, ng)]
    img, normed = render_ref(cube, window, [r[1:6] + [1] for r in rows], [[r[6], r[7], GAMMA] for r in rows], zoom, (ch, cw), (NY, NX), table)
    if glyphs is not None:
        h, w = zoom * dy, zoom * dx
        for title, _, _, _, y, x, lo, hi in rows:
            c = img[y:y + ch, x:x + cw]
            text(c, glyphs, h + 2, 0, title)
            text(c, glyphs, 0, w + BAR_GAP + BAR_W + TICK + 1, f"{lo:.4g}")
            if h >= 25:
                text(c, glyphs, h - 12, w + BAR_GAP + BAR_W + TICK + 1, f"{hi:.4g}")
    return img, {r[0]: (r[6], r[7]) for r in rows}, [r[:6] for r in rows], normed


# ---------------------------------------------------------------------------------------------- the power-norm tolerance
# The device's powf and numpy's float32 power need not agree in the last bits.
#   device powf: 1 ulp, the figure of the HIP math API reference's table of single-precision functions (maximum ulp difference to
#     the correctly rounded result over its tested range);
#   numpy float32 power: 1.006 ulp of the result, the largest difference to float64 pow measured on the CPU over 10^7 random
#     arguments in (0, 50] with the exponent float32(2/3) (tests/test_host_visualize.py measures it again for the case table).
# Their sum, 2.006 ulp, separates two float32 values by at most POWER_SLACK_ULPS = 2 representable steps.
POWER_SLACK_ULPS = 2


def power_panel_check(got, t, table, zoom):
    """(pixels that equal the restatement's colour, pixels that equal it only after moving t by up to POWER_SLACK_ULPS steps,
    pixels that do neither) of a device panel `got` (zoomed) against the restatement's normalised window t"""
    big = lambda a: np.repeat(np.repeat(a, zoom, axis=0), zoom, axis=1)   # noqa: E731
    exact = (got == big(colours(t, table))).all(axis=2)
    ok = exact.copy()
    for k in range(1, POWER_SLACK_ULPS + 1):
        for s in (-k, k):
            moved = np.where(t > 0, shift_ulps(t, s), t)   # only a powered value may move
            ok |= (got == big(colours(moved, table))).all(axis=2)
    return int(exact.sum()), int((ok & ~exact).sum()), int((~ok).sum())
