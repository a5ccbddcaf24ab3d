"""numpy restatement, in float64, of the two focal-plane entries (``rip_fpa_bin``, ``rip_fpa_render``) and of the picture that
``utils/fpaplot.py`` composes from them -- independent of the device code and of the package's Python mirror.  The fixtures
``tests/golden/fpaplot_*.npz`` were made by the reference's own functions (tools/make_fpaplot_goldens.py); the host tests hold this
file to them, the GPU tests hold the device to this file."""

import struct
import zlib

import numpy as np

# a 64-pixel focal plane: the reference's centres and bounding box divided by 64 (18 SCAs, the same arrangement)
SMALL = {
    "nside": 64,
    "ctrs": [[35, 19], [35, -58], [35, -128], [104, 33], [105, -44], [105, -114], [173, 66], [174, -11], [176, -80],
             [-35, 19], [-35, -58], [-35, -128], [-104, 33], [-105, -44], [-105, -114], [-173, 66], [-174, -11], [-176, -80]],
    "bbox": {"xmin": -208, "xmax": 208, "ymin": -160, "ymax": 98},
}
PANELS = (("lin2", -100.0, 2900.0, "{:4.0f}"), ("lin3", -100.0, 1500.0, "{:4.0f}"), ("gain", 1.2, 2.1, "{:4.2f}"),
          ("alphaD", 0.0, 0.004, "{:5.3f}"), ("alphaH", 0.005, 0.025, "{:5.3f}"), ("alphaV", 0.005, 0.025, "{:5.3f}"),
          ("pflatnorm", 0.8, 1.2, "{:4.2f}"), ("read", 4.0, 9.0, "{:4.1f}"))
LABELS = {"gain": "gain (e/DN)", "alphaH": "IPC_h", "alphaV": "IPC_v", "alphaD": "IPC_d", "lin2": "c2 (DN)", "lin3": "c3 (DN)",
          "pflatnorm": "pflatnorm", "read": "rn (DN)"}
# the growth table of maskhandling.PixelMask1, by bit
PIXELMASK1 = np.zeros(32, np.uint8)
for _bit, _g in {0: 1, 2: 5, 3: 25, 4: 1, 5: 1, 6: 5, 8: 1, 9: 1, 10: 9, 11: 9, 12: 1, 13: 9, 15: 1, 18: 9, 19: 9, 20: 9, 21: 9,
                 22: 1, 23: 9, 24: 9, 25: 9, 28: 9, 30: 9}.items():
    PIXELMASK1[_bit] = _g


# ---------------------------------------------------------------------------------------------- binning
def grown_mask(dq, grow):
    """True where a pixel is masked: the layer of bit b grown to grow[b] pixels (1 itself, 5 plus, 9 3x3, 25 5x5), zero padded"""
    ny, nx = dq.shape
    out = np.zeros((ny, nx), bool)
    for b in range(32):
        g = int(grow[b])
        if g == 0:
            continue
        layer = np.pad((dq >> np.uint32(b)) & np.uint32(1), 2).astype(bool)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                reach = {1: dy == 0 and dx == 0, 5: abs(dy) + abs(dx) <= 1, 9: max(abs(dy), abs(dx)) <= 1, 25: True}[g]
                if reach:
                    out |= layer[2 + dy:2 + dy + ny, 2 + dx:2 + dx + nx]
    return out


def bin_ref(dq, grow, planes, nside, n1):
    """(means, bound): means (nplanes, n1, n1) float64 and, per bin, the bound s^2 * 2^-53 * sum|v| / count of the difference
    between two float64 sums of its s^2 terms taken in any order (0 where nothing finite is summed)"""
    s = nside // n1
    masked = grown_mask(dq, grow) if dq is not None else np.zeros((nside, nside), bool)
    means = np.empty((len(planes), n1, n1))
    bound = np.zeros((len(planes), n1, n1))
    for i, p in enumerate(planes):
        v = np.asarray(p, dtype=np.float64)
        v = np.pad(v, (nside - v.shape[0]) // 2)
        ok = ~masked & ~np.isnan(v)
        blocks = lambda a: a.reshape(n1, s, n1, s)   # noqa: E731
        with np.errstate(invalid="ignore", divide="ignore"):
            total = blocks(np.where(ok, v, 0.0)).sum(axis=(1, 3))
            count = blocks(ok).sum(axis=(1, 3))
            means[i] = total / count
            mag = blocks(np.where(ok & np.isfinite(v), np.abs(v), 0.0)).sum(axis=(1, 3))
            bound[i] = np.where(count > 0, s * s * 2.0**-53 * mag / np.maximum(count, 1), 0.0)
    return means, bound


# ---------------------------------------------------------------------------------------------- rendering
def layout(n1, geometry):
    """(ny, nx) of a panel and the (posy, posx) of each SCA in it"""
    nside, bbox = geometry["nside"], geometry["bbox"]
    scale = nside // n1
    nx = (bbox["xmax"] - bbox["xmin"] + 1) // scale
    ny = (bbox["ymax"] - bbox["ymin"] + 1) // scale
    pos = [((cy - nside // 2 - bbox["ymin"]) // scale, (cx - nside // 2 - bbox["xmin"]) // scale) for cx, cy in geometry["ctrs"]]
    return ny, nx, np.array(pos, dtype=np.int32)


def color_index(x):
    """index into a 256-entry table of x in [0, 1]: what cmap(x, bytes=True) looks up"""
    return np.minimum((np.asarray(x, dtype=np.float64) * 256.0).astype(np.int64), 255)


def stamp_text(img, glyphs, y, x, size, val, text, frac=None, owner=None):
    """letters of `text` from (y, x) on the 2-D or 3-D image: cell = size pixels, glyph rows bottom-up, advance 8 * size; stops at
    the first letter that does not fit; returns the stamps it made.  A stamped pixel is no SCA pixel any more (frac, owner)."""
    made = []
    for ch in text:
        if x + 6 * size > img.shape[1] or y + 12 * size > img.shape[0]:
            break
        made.append([y, x, size, val, ord(ch)])
        if glyphs is not None:
            on = np.kron(glyphs[ord(ch)][::-1] > 0, np.ones((size, size), bool))
            img[y:y + 12 * size, x:x + 6 * size][on] = val
            if frac is not None:
                frac[y:y + 12 * size, x:x + 6 * size][on] = np.nan
                owner[y:y + 12 * size, x:x + 6 * size][on] = -1
        x += 8 * size
    return made


def panel_ref(maps, present, vmin, vmax, n1, ny, nx, pos, table, glyphs=None, ptype=None, fmt=None, texts=(), exact=None):
    """One panel: (image, frac, owner).  frac (ny, nx): x * 256 before the clip of the SCA pixel drawn there, where a rounding of
    the mean can move it -- 0.5 where it cannot (an absent file, an empty bin or an infinite mean: the value is 0 or +-DBL_MAX by
    rule; a value further than half a step outside vmin .. vmax; a mean that `exact` (nsca, n1, n1) marks as the same in any
    order of summation) -- and NaN where no SCA is drawn; owner: the SCA index drawn there or -1.  `fmt` draws the scale; `texts`: further rows (y, x, size, value, string)."""
    img = np.full((ny, nx, 3), 255, np.uint8)
    frac = np.full((ny, nx), np.nan)
    owner = np.full((ny, nx), -1)
    for k, (py, px) in enumerate(pos):
        m = np.nan_to_num(maps[k]) if present[k] else np.zeros((n1, n1))
        x = np.clip((m - vmin) / (vmax - vmin), 0.0, 1.0)
        img[py:py + n1, px:px + n1] = table[color_index(x)]
        free = np.isfinite(maps[k]) if present[k] else np.zeros((n1, n1), bool)
        if exact is not None:
            free &= ~exact[k]
        with np.errstate(invalid="ignore", over="ignore"):
            frac[py:py + n1, px:px + n1] = np.where(free, np.clip((maps[k] - vmin) / (vmax - vmin) * 256.0, -0.5, 256.5), 0.5)
        owner[py:py + n1, px:px + n1] = k
    if fmt is not None:
        sc = max(n1, 64) // 64
        bar = slice(ny - n1 // 8, ny), slice(nx // 2 - n1, nx // 2 + n1)
        img[bar] = table[color_index(np.linspace(0, 1, 2 * n1))][None]
        frac[bar], owner[bar] = np.nan, -1
        for j in range(3):
            tick = slice(ny - n1 // 8 - 2 * sc, ny - n1 // 8), slice(nx // 2 - n1 + j * n1, nx // 2 - n1 + j * n1 + sc)
            img[tick] = 0
            frac[tick], owner[tick] = np.nan, -1
            txt = fmt.format(j / 2.0 * (vmax - vmin) + vmin)
            stamp_text(img, glyphs, ny - n1 // 8 - 15 * sc, nx // 2 - n1 + n1 * j - 3 * sc * len(txt), sc, 0, txt, frac, owner)
        stamp_text(img, glyphs, ny - n1 // 8 - 27 * sc, nx // 2 - 3 * sc * len(LABELS[ptype]), sc, 0, LABELS[ptype], frac, owner)
    for y, x, size, val, text in texts:
        stamp_text(img, glyphs, y, x, size, val, text, frac, owner)
    return img, frac, owner


def compose(panels, n1, nw=2):
    """the panels `nw` abreast with a gap of 1 + n1 // 4, white between; works on images (3-D, fill 255) and on frac / owner
    planes (2-D, fill NaN / -1)"""
    ny, nx = panels[0].shape[:2]
    nh = (len(panels) - 1) // nw + 1
    gap = 1 + n1 // 4
    fill = 255 if panels[0].ndim == 3 else (np.nan if panels[0].dtype.kind == "f" else -1)
    out = np.full((ny * nh + gap * (nh - 1), nx * nw + gap * (nw - 1)) + panels[0].shape[2:], fill, panels[0].dtype)
    for i, p in enumerate(panels):
        y, x = (i // nw) * (ny + gap), (i % nw) * (nx + gap)
        out[y:y + ny, x:x + nx] = p
    return out


def multi_image_ref(scas, n1, grow, geometry, table, glyphs=None, panels=PANELS):
    """(picture, frac, owner, maps): `scas` per SCA None or {ptype: plane, "dq": dq}; maps (npanel, nsca, n1, n1)"""
    nside = geometry["nside"]
    ny, nx, pos = layout(n1, geometry)
    maps = np.zeros((len(panels), len(scas), n1, n1))
    present = np.zeros((len(panels), len(scas)), bool)
    exact = np.zeros(maps.shape, bool)   # a bin whose counted values are all zero (the padding): 0.0 however it is summed
    for k, sca in enumerate(scas):
        for j, (ptype, *_) in enumerate(panels):
            if sca is not None and sca.get(ptype) is not None:
                means, bound = bin_ref(sca["dq"], grow, [sca[ptype]], nside, n1)
                maps[j, k], exact[j, k] = means[0], bound[0] == 0.0
                present[j, k] = True
    parts = [panel_ref(maps[j], present[j], vmin, vmax, n1, ny, nx, pos, table, glyphs, ptype, fmt, exact=exact[j])
             for j, (ptype, vmin, vmax, fmt) in enumerate(panels)]
    return tuple(compose([p[i] for p in parts], n1) for i in range(3)) + (maps,)


def near_integer(frac, tol=1e-9):
    """where x * 256 of an SCA pixel (panel_ref's frac) lies within `tol` of an integer: there the colour index may go either way"""
    with np.errstate(invalid="ignore"):
        return np.abs(frac - np.rint(frac)) <= tol


# ---------------------------------------------------------------------------------------------- the fixture
def golden_scas(g):
    """per SCA None or {ptype: plane, "dq": dq}, as the fixture's files held them"""
    scas = []
    for k in range(18):
        if k + 1 == int(g["missing_all"]):
            scas.append(None)
            continue
        i = int(g["sca_set"][k])
        s = {p: g[f"set{i}_{p}"] for p, *_ in PANELS if not (k + 1 == int(g["missing_gain"]) and p == "gain")}
        s["dq"] = g[f"set{i}_dq"]
        scas.append(s)
    return scas


def reference_bound(sca, ptype, n1):
    """the derived bound on |restatement - reference| of one SCA's map: the file's own precision in place of 2^-53"""
    _, b = bin_ref(sca["dq"], PIXELMASK1, [sca[ptype]], 64, n1)
    return b[0] * (2.0**53 * (2.0**-24 if sca[ptype].dtype == np.float32 else 2.0**-53))


def assert_picture(got, want, owner, what):
    """every pixel that is no SCA pixel equal; SCA pixels at most one colour step apart, in at most 0.5 % of them"""
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, what
    differ = (got != want).any(axis=2)
    assert not (differ & (owner < 0)).any(), f"{what}: layout pixels differ"
    step = np.abs(got.astype(int) - want.astype(int)).max(axis=(0, 1)) if differ.any() else np.zeros(3, int)
    assert (step <= [3, 2, 2]).all(), f"{what}: a colour is {step} away, more than one index step"
    assert np.count_nonzero(differ) <= 0.005 * np.count_nonzero(owner >= 0), f"{what}: {np.count_nonzero(differ)} SCA pixels differ"


# ---------------------------------------------------------------------------------------------- inputs
def smooth_field(rng, side, lo, hi):
    """a smooth field inside lo..hi: a plane plus two low waves, 10 % .. 90 % of the range"""
    y, x = np.mgrid[0:side, 0:side] / max(side - 1, 1)
    a, b, c, d = rng.uniform(0.5, 2.0, 4)
    f = 0.5 + 0.2 * np.sin(a * y * np.pi + d) * np.cos(b * x * np.pi) + 0.15 * (x - y) * np.sin(c) + 0.05 * rng.standard_normal((side, side))
    return lo + (hi - lo) * np.clip(f, 0.1, 0.9)


def random_dq(rng, nside, frac=0.05):
    """uint32 flags: `frac` of the pixels carry one random bit of PixelMask1's growths 1, 5, 9, 25 (or a bit it ignores)"""
    dq = np.zeros((nside, nside), np.uint32)
    hit = rng.random((nside, nside)) < frac
    bits = rng.choice([0, 2, 3, 10, 11, 1, 7, 30], size=(nside, nside))
    dq[hit] = (np.uint32(1) << bits[hit].astype(np.uint32))
    return dq


def read_png(path):
    """the (ny, nx, 3) uint8 array of an 8-bit RGB PNG without interlace whose scanlines are unfiltered"""
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    at, idat, head = 8, b"", None
    while at < len(raw):
        n, kind = struct.unpack(">I4s", raw[at:at + 8])
        body = raw[at + 8:at + 8 + n]
        assert struct.unpack(">I", raw[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF, "chunk CRC"
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        at += 12 + n
    nx, ny, depth, colour, comp, filt, lace = head
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(ny, 1 + 3 * nx)
    assert not rows[:, 0].any(), "a filtered scanline"
    return rows[:, 1:].reshape(ny, nx, 3).copy()
