"""Focal-plane overview of a calibration set on the GPU -- same call surface as the reference's ``utils/fpaplot.py``
(``read_sca_image``, ``write_text``, ``make_big_image``, ``multi_image``; line numbers below are that file's).

Per SCA one ``rip_fpa_bin`` call reads ``dq`` once, grows the mask on the fly and bins every quantity under it; only the
``n1 x n1`` means stay in HBM, and one ``rip_fpa_render`` call draws the whole picture, which is downloaded once.  The
reference opens each file and rebuilds the grown mask for each of its 8 quantities.

Kept from the reference, on purpose:
  * ``"pflatnorm"`` is NOT divided by its median (the test ``ptype == "pflat"`` at :236 never matches) and ``"pflat"`` raises
    ``KeyError`` (:91-100 has no such key);
  * a missing data file draws as zeros (:114-117); a data file without its mask file raises; an array of 1 or more than 4
    dimensions raises ``ValueError`` (:129);
  * ``mask=None`` with an existing data file raises (``TypeError``; the reference crashes on ``None.build``).
The glyph table (``utils/letters.dat`` of the reference) is not part of this package: labels are drawn when the caller passes
``font=`` (a (256, 12, 6) array or the path of such a text file); without it the bar and ticks are drawn and no text.

``python -m romanimpreprocess_amd.utils.fpaplot <format> <out.png> [--font FILE] [--n1 128] [--geometry FILE]`` is the script of
:361-372.
"""

import ctypes as C
import os
import sys

import numpy as np

from .. import _native, calio
from ..devarray import DevArray, is_dev

# focal plane parameters (:29-54), in pixels (= 0.01 mm); the bounding box includes the reference pixels
DEFAULT_GEOMETRY = {
    "nside": 4096,
    "ctrs": [[2214, 1215], [2229, -3703], [2244, -8206], [6642, 2090], [6692, -2828], [6742, -7306], [11070, 4220], [11148, -698],
             [11264, -5106], [-2214, 1215], [-2229, -3703], [-2244, -8206], [-6642, 2090], [-6692, -2828], [-6742, -7306],
             [-11070, 4220], [-11148, -698], [-11264, -5106]],
    "bbox": {"xmin": -13312, "xmax": 13312, "ymin": -10254, "ymax": 6268},
}

# ptype -> file, leading coordinates of a 3-D / 4-D array, label of the scale (:91-111, :259-268)
FILESTRING = {"gain": "gain", "alphaH": "ipc4d", "alphaV": "ipc4d", "alphaD": "ipc4d", "lin2": "linearitylegendre",
              "lin3": "linearitylegendre", "pflatnorm": "pflat", "read": "read"}
POS = {"gain": None, "alphaH": [1, 0], "alphaV": [0, 1], "alphaD": [0, 0], "lin2": [2], "lin3": [3], "pflat": None, "read": None}
LABEL = {"gain": "gain (e/DN)", "alphaH": "IPC_h", "alphaV": "IPC_v", "alphaD": "IPC_d", "lin2": "c2 (DN)", "lin3": "c3 (DN)",
         "pflatnorm": "pflatnorm", "read": "rn (DN)"}
# the panels of multi_image (:300-343): ptype, vmin, vmax, scaleformat
PANELS = (("lin2", -100.0, 2900.0, "{:4.0f}"), ("lin3", -100.0, 1500.0, "{:4.0f}"), ("gain", 1.2, 2.1, "{:4.2f}"),
          ("alphaD", 0.0, 0.004, "{:5.3f}"), ("alphaH", 0.005, 0.025, "{:5.3f}"), ("alphaV", 0.005, 0.025, "{:5.3f}"),
          ("pflatnorm", 0.8, 1.2, "{:4.2f}"), ("read", 4.0, 9.0, "{:4.1f}"))

# matplotlib.colormaps["viridis"](np.arange(256), bytes=True)[:, :3] (matplotlib 3.10), 256 x RGB
VIRIDIS = np.frombuffer(bytes.fromhex(
    "44015444025544035745055845065a45085b46095c460b5e460c5f460e61470f6247116347126547146647156747166947186a48196b481a6c481c6e"
    "481d6f481e70482071482172482273482374472575472676472777472878472a79472b7a472c7b462d7c462f7c46307d46317e45327f45347f453580"
    "453681443781443982433a83433b83433c84423d84423e854240854141864142864043874044873f45873f47883e48883e49893d4a893d4b893d4c89"
    "3c4d8a3c4e8a3b508a3b518a3a528b3a538b39548b39558b38568b38578c37588c37598c365a8c365b8c355c8c355d8c345e8d345f8d33608d33618d"
    "32628d32638d31648d31658d31668d30678d30688d2f698d2f6a8d2e6b8e2e6c8e2e6d8e2d6e8e2d6f8e2c708e2c718e2c728e2b738e2b748e2a758e"
    "2a768e2a778e29788e29798e287a8e287a8e287b8e277c8e277d8e277e8e267f8e26808e26818e25828e25838d24848d24858d24868d23878d23888d"
    "23898d22898d228a8d228b8d218c8d218d8c218e8c208f8c20908c20918c1f928c1f938b1f948b1f958b1f968b1e978a1e988a1e998a1e998a1e9a89"
    "1e9b891e9c891e9d881e9e881e9f881ea0871fa1871fa2861fa38620a48520a58521a68521a78422a78423a88323a98224aa8225ab8126ac8127ad80"
    "28ae7f29af7f2ab07e2bb17d2cb17d2eb27c2fb37b30b47a32b57a33b67935b77836b87738b97639b9763bba753dbb743ebc7340bd7242be7144be70"
    "45bf6f47c06e49c16d4bc26c4dc26b4fc36951c46853c56755c66657c66559c7645bc8625ec96160c96062ca5f64cb5d67cc5c69cc5b6bcd596dce58"
    "70ce5672cf5574d05477d05279d1517cd24f7ed24e81d34c83d34b86d44988d5478bd5468dd64490d64392d74195d73f97d83e9ad83c9dd93a9fd938"
    "a2da37a5da35a7db33aadb32addc30afdc2eb2dd2cb5dd2bb7dd29bade27bdde26bfdf24c2df22c5df21c7e01fcae01ecde01dcfe11cd2e11bd4e11a"
    "d7e219dae218dce218dfe318e1e318e4e318e7e419e9e419ece41aeee51bf1e51cf3e51ef6e61ff8e621fae622fde724"
), dtype=np.uint8).reshape(256, 3)

# matplotlib.colormaps["magma"](np.arange(256), bytes=True)[:, :3] (matplotlib 3.10): the map of utils/visualize.py
MAGMA = np.frombuffer(bytes.fromhex(
    "00000300000400000601000701010901010b02020d02020f03031104031304041505041706051907051b08061d09071f0a07220b08240c09260d0a28"
    "0e0a2a0f0b2c100c2f110c31120d33140d35150e38160e3a170f3c180f3f1a10411b10441c10461e10491f114b20114d221150231152251155261157"
    "2811592a115c2b115e2d10602f1062301065321067341068350f6a370f6c390f6e3b0f6f3c0f713e0f72400f73420f74430f75450f76470f77481078"
    "4a10794b10794d117a4f117b50127b52127c53137c55137d57147d58157e5a157e5b167e5d177e5e177f60187f61187f63197f651a80661a80681b80"
    "691c806b1c806c1d806e1e816f1e81711f81731f817420817621817721817922817a22817c23817e24817f2481812581822581842681852681872781"
    "8928818a28818c29808d29808f2a80912a80922b80942b80952c80972c7f992d7f9a2d7f9c2e7f9e2e7e9f2f7ea12f7ea3307ea4307da6317da7317d"
    "a9327cab337cac337bae347bb0347bb1357ab3357ab53679b63679b83778b93778bb3877bd3977be3976c03a75c23a75c33b74c53c74c63c73c83d72"
    "ca3e72cb3e71cd3f70ce4070d0416fd1426ed3426dd4436dd6446cd7456bd9466ada4769dc4869dd4968de4a67e04b66e14c66e24d65e44e64e55063"
    "e65162e75262e85461ea5560eb5660ec585fed595fee5b5eee5d5def5e5df0605df1615cf2635cf3655cf3675bf4685bf56a5bf56c5bf66e5bf6705b"
    "f7715bf7735cf8755cf8775cf9795cf97b5df97d5dfa7f5efa805efa825ffb8460fb8660fb8861fb8a62fc8c63fc8e63fc9064fc9265fc9366fd9567"
    "fd9768fd9969fd9b6afd9d6bfd9f6cfda16efda26ffda470fea671fea873feaa74feac75feae76feaf78feb179feb37bfeb57cfeb77dfeb97ffebb80"
    "febc82febe83fec085fec286fec488fec689fec78bfec98dfecb8efdcd90fdcf92fdd193fdd295fdd497fdd698fdd89afdda9cfddc9dfddd9ffddfa1"
    "fde1a3fce3a5fce5a6fce6a8fce8aafceaacfcecaefceeb0fcf0b1fcf1b3fcf3b5fcf5b7fbf7b9fbf9bbfbfabdfbfcbf"
), dtype=np.uint8).reshape(256, 3)


def color_table(cmap="viridis"):
    """The (256, 3) uint8 table of a colour map: viridis and magma are shipped; any other name is matplotlib's where that is
    importable and the map has 256 entries, otherwise it is refused by name."""
    if cmap == "viridis":
        return VIRIDIS
    if cmap == "magma":
        return MAGMA
    try:
        import matplotlib  # noqa: PLC0415

        cm = matplotlib.colormaps[cmap]
    except (ImportError, KeyError):
        raise ValueError(f"fpaplot: colour map {cmap!r} is not shipped (only 'viridis' and 'magma') and matplotlib does not supply it") from None
    if cm.N != 256:
        raise ValueError(f"fpaplot: colour map {cmap!r} has {cm.N} entries, not 256")
    return np.ascontiguousarray(cm(np.arange(256), bytes=True)[:, :3])


def load_font(font):
    """The glyph table as (256, 12, 6) uint8: ``font`` is such an array, the path of a text file of 256 * 12 rows of 6 numbers
    (the layout of the reference's ``letters.dat``), or None."""
    if font is None:
        return None
    if isinstance(font, (str, os.PathLike)):
        font = np.loadtxt(font)
    font = np.asarray(font)
    if font.size != 256 * 12 * 6:
        raise ValueError(f"fpaplot: a glyph table holds 256 x 12 x 6 cells, got {font.size}")
    return np.ascontiguousarray(np.clip(font.reshape(256, 12, 6), 0, 255).astype(np.uint8))


def text_stamps(panel, shape, origin, size, val, string):
    """What ``write_text`` would put on an image of ``shape`` = (ny, nx), as stamps [panel, y, x, size, value, character], one per
    letter: the advance is 8 * size and the rest of the string is dropped once a letter does not fit (:174-182)."""
    posy, posx = int(origin[0]), int(origin[1])
    out = []
    for ch in string:
        if posx + size * 6 > shape[-1] or posy + size * 12 > shape[-2]:
            break
        if ord(ch) > 255:
            raise ValueError(f"fpaplot: character {ch!r} is outside the glyph table")
        out.append([int(panel), posy, posx, int(size), int(val), ord(ch)])
        posx += size * 8
    return out


def write_text(image, origin, size, val, string, font=None):
    """Writes ``string`` on the 2-D ``image`` from ``origin`` = (y, x) in brightness ``val``, every glyph cell ``size`` pixels
    wide and high (:150-182): the host form, on a numpy array."""
    letters = load_font(font)
    if letters is None:
        raise ValueError("fpaplot.write_text needs font= (the glyph table is not part of this package)")
    for _, posy, posx, _, _, code in text_stamps(0, np.shape(image), origin, size, val, string):
        card = np.repeat(np.repeat(letters[code, ::-1, :], size, axis=0), size, axis=1)
        box = image[posy:posy + size * 12, posx:posx + size * 6]
        image[posy:posy + size * 12, posx:posx + size * 6] = np.where(card > 0, val, box)


def _geometry(geometry):
    g = DEFAULT_GEOMETRY if geometry is None else geometry
    return int(g["nside"]), np.asarray(g["ctrs"], dtype=np.int64).reshape(-1, 2), g["bbox"]


def panel_layout(n1, geometry=None):
    """(ny, nx) of one panel and the (nsca, 2) int32 (posy, posx) of every SCA in it, with the integer arithmetic of :224-226 and
    :241-242 (floor division, also of negative numbers)."""
    nside, ctrs, bbox = _geometry(geometry)
    scale = nside // n1
    nx = (bbox["xmax"] - bbox["xmin"] + 1) // scale
    ny = (bbox["ymax"] - bbox["ymin"] + 1) // scale
    pos = np.array([[(int(cy) - nside // 2 - bbox["ymin"]) // scale, (int(cx) - nside // 2 - bbox["xmin"]) // scale]
                    for cx, cy in ctrs], dtype=np.int32)
    return ny, nx, pos


def scale_stamps(panel, n1, ny, nx, ptype, vmin, vmax, scaleformat):
    """the letters of one panel's scale: the three tick values and the label (:249-273)"""
    sc = max(n1, 64) // 64
    out = []
    posy = ny - n1 // 8 - 15 * sc
    for j in range(3):
        txt = scaleformat.format(j / 2.0 * (vmax - vmin) + vmin)
        out += text_stamps(panel, (ny, nx), (posy, nx // 2 - n1 + n1 * j - 3 * sc * len(txt)), sc, 0, txt)
    label = LABEL[ptype]
    out += text_stamps(panel, (ny, nx), (ny - n1 // 8 - 27 * sc, nx // 2 - 3 * sc * len(label)), sc, 0, label)
    return out


# ---------------------------------------------------------------------------------------------- the two device calls
def _torch_device(ctx):
    import torch  # noqa: PLC0415

    return torch, torch.device("cuda", ctx.device)


def bin_planes(dq, planes, nside, n1, mask=None, ctx=None, out=None):
    """``rip_fpa_bin``: the masked block means of up to 8 square planes of one SCA as a float64 ``DevArray`` (nplanes, n1, n1) in
    HBM.  ``dq``: (nside, nside) uint32, numpy or ``DevArray``, or None (nothing masked); ``planes``: float32 / float64 arrays,
    numpy (uploaded) or ``DevArray`` (used where they lie), of sides up to nside; ``mask``: a ``CombinedMask`` (its growth
    table), a 32-entry growth table or None (no bit masks).  ``out``: such a ``DevArray`` to write into."""
    ctx = ctx or _native.default_context()
    grow = np.zeros(32, np.uint8) if mask is None else np.ascontiguousarray(getattr(mask, "array", mask), dtype=np.uint8)
    if grow.shape != (32,):
        raise ValueError("fpaplot: the growth table has 32 entries")
    if len(planes) < 1 or len(planes) > _native.RIP_FPA_MAX_PLANES:
        raise ValueError(f"fpaplot: {len(planes)} planes, outside 1..{_native.RIP_FPA_MAX_PLANES}")
    keep = [a if is_dev(a) else _native.float_array(a) for a in planes]
    for i, a in enumerate(keep):
        if a.ndim != 2 or a.shape[0] != a.shape[1]:
            raise ValueError(f"fpaplot: plane {i} of shape {a.shape} is not square")
    ptrs = (C.c_void_p * len(keep))(*[a.ctypes.data for a in keep])
    as_int = lambda v: np.array(v, dtype=np.intc)   # noqa: E731
    if dq is not None:
        if not is_dev(dq):
            dq = np.ascontiguousarray(dq, dtype=np.uint32)
        if dq.dtype != np.uint32 or tuple(dq.shape) != (nside, nside):
            raise ValueError(f"fpaplot: dq is {dq.dtype}{tuple(dq.shape)}, expected uint32 ({nside}, {nside})")
    if out is None:
        torch, dev = _torch_device(ctx)
        out = DevArray(torch.empty((len(planes), max(int(n1), 1), max(int(n1), 1)), dtype=torch.float64, device=dev)).sync()
    ctx.call("rip_fpa_bin", dq, _native.RIP_HOST if dq is None else _native.location_of(dq), grow, nside, n1, len(planes), ptrs,
             as_int([_native.dtype_code(a) for a in keep]), as_int([a.shape[0] for a in keep]),
             as_int([_native.location_of(a) for a in keep]), out, _native.location_of(out))
    return out


def render(maps, present, vmin, vmax, scale, n1, ny, nx, sca_pos, table=None, font=None, stamps=(), nw=2, gap=None, ctx=None,
           out=None):
    """``rip_fpa_render``: the (NY, NX, 3) uint8 picture of ``npanel`` panels of (ny, nx) pixels, ``nw`` abreast with ``gap``
    (default 1 + n1 // 4) between them.  ``maps``: (npanel, nsca, n1, n1) float64, ``DevArray`` or numpy; ``present``: (npanel,
    nsca) flags; ``vmin``, ``vmax``, ``scale``: per panel; ``sca_pos``: (nsca, 2) (posy, posx) in a panel; ``stamps``: rows of
    [panel, y, x, size, value, character], drawn only with ``font``.  ``out``: a uint8 ``DevArray`` to draw into instead (it is
    returned, and nothing is downloaded)."""
    ctx = ctx or _native.default_context()
    present = np.ascontiguousarray(present, dtype=np.uint8)
    npanel, nsca = present.shape
    if tuple(maps.shape) != (npanel, nsca, n1, n1) or maps.dtype != np.float64:
        raise ValueError(f"fpaplot: maps are {maps.dtype}{tuple(maps.shape)}, expected float64 {(npanel, nsca, n1, n1)}")
    glyphs = load_font(font)
    st = np.ascontiguousarray(np.asarray(list(stamps) if glyphs is not None else [], dtype=np.int32).reshape(-1, 6))
    gap = (1 + n1 // 4) if gap is None else gap
    nh = (npanel - 1) // nw + 1
    shape = (ny * nh + gap * (nh - 1), nx * nw + gap * (nw - 1), 3)
    img = out if out is not None else np.empty(shape, np.uint8)
    if tuple(img.shape) != shape:
        raise ValueError(f"fpaplot: the picture is {shape}, out is {tuple(img.shape)}")
    if not is_dev(maps):
        maps = np.ascontiguousarray(maps)
    as_f64 = lambda v: np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (npanel,)))   # noqa: E731
    ctx.call("rip_fpa_render", n1, nsca, npanel, nw, gap, ny, nx, maps, _native.location_of(maps), present,
             np.ascontiguousarray(sca_pos, dtype=np.int32).reshape(nsca, 2), as_f64(vmin), as_f64(vmax),
             np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=bool), (npanel,)), dtype=np.uint8),
             np.ascontiguousarray(VIRIDIS if table is None else table, dtype=np.uint8).reshape(256, 3), glyphs,
             len(st), st if len(st) else None, img, _native.location_of(img))
    return img


# ---------------------------------------------------------------------------------------------- the reference's surface
def _plane_of(obj, ptype):
    """the 2-D plane of ``ptype`` in the data array of its file (:120-129), as a numpy array; only that plane is materialised"""
    s = np.shape(obj)
    if len(s) == 2:
        return np.asarray(obj)
    if len(s) == 3:
        return np.asarray(obj[POS[ptype][0]])
    if len(s) == 4:
        return np.asarray(obj[POS[ptype][0], POS[ptype][1]])
    raise ValueError("fpaplot.read_sca_image: Incorrect array dimension.")


def load_sca(infile_format, scanum, ptypes):
    """What one SCA's files hold for ``ptypes``: {ptype: plane, ..., "dq": the mask file's dq} with every file opened once; a
    ptype whose file does not exist is left out (:116-117); None where no file exists.  A data file without its mask file raises."""
    files = {}
    for ptype in ptypes:
        files.setdefault(infile_format.format(FILESTRING[ptype], scanum), []).append(ptype)
    out = {}
    for file, names in files.items():
        if not os.path.exists(file):
            continue
        with calio.open_tree(file) as f:
            obj = f["roman"]["data"]
            for ptype in names:
                out[ptype] = _plane_of(obj, ptype)
    if not out:
        return None
    with calio.open_tree(infile_format.format("mask", scanum)) as m:
        out["dq"] = np.asarray(m["roman"]["dq"])
    return out


def _bin_sca(sca, ptypes, n1, nside, mask, ctx):
    """(the ptypes present, their means as a DevArray) of one SCA's dict, or ([], None)"""
    have = [p for p in ptypes if sca is not None and sca.get(p) is not None]
    if not have:
        return have, None
    if mask is None:
        raise TypeError("fpaplot: mask=None, but there is data to mask (pass a CombinedMask such as maskhandling.PixelMask1)")
    if sca.get("dq") is None:
        raise KeyError("fpaplot: an SCA with data needs its 'dq'")
    return have, bin_planes(sca["dq"], [sca[p] for p in have], nside, n1, mask=mask, ctx=ctx)


def read_sca_image(infile_format, n1, ptype, scanum, mask=None, ctx=None, geometry=None):
    """The image of quantity ``ptype`` of SCA ``scanum`` (1..18), binned to (n1, n1) float64 (:57-142).  The legal ptypes are
    'gain', 'alphaH', 'alphaV', 'alphaD', 'lin2', 'lin3', 'pflatnorm' and 'read'."""
    nside = _geometry(geometry)[0]
    have, means = _bin_sca(load_sca(infile_format, scanum, [ptype]), [ptype], n1, nside, mask, ctx or _native.default_context())
    return means.numpy()[0] if have else np.zeros((n1, n1))


def multi_image_from_planes(planes, n1, masktype, panels=PANELS, cmap="viridis", font=None, ctx=None, geometry=None, nw=2):
    """``multi_image`` of planes the caller holds: ``planes`` is, per SCA, None (no file) or a dict {ptype: square plane, ...,
    "dq": (nside, nside) uint32}, each a numpy array or a ``DevArray`` -- what ``calfiles.derive_*`` left in HBM is used where it
    lies.  A ptype missing from an SCA's dict draws as zeros.  ``panels``: (ptype, vmin, vmax, scaleformat or None) each, ``nw``
    abreast."""
    ctx = ctx or _native.default_context()
    nside, ctrs, _ = _geometry(geometry)
    if len(planes) != len(ctrs):
        raise ValueError(f"fpaplot: {len(planes)} SCAs given, the geometry has {len(ctrs)}")
    table = color_table(cmap)
    ny, nx, pos = panel_layout(n1, geometry)
    ptypes = [p[0] for p in panels]
    for p in ptypes:
        FILESTRING[p]   # "pflat" and other unknown quantities: KeyError, as :113
    torch, dev = _torch_device(ctx)
    maps = torch.zeros((len(panels), len(ctrs), n1, n1), dtype=torch.float64, device=dev)
    present = np.zeros((len(panels), len(ctrs)), np.uint8)
    uniq = list(dict.fromkeys(ptypes))
    for k, sca in enumerate(planes):
        for lo in range(0, len(uniq), _native.RIP_FPA_MAX_PLANES):
            have, means = _bin_sca(sca, uniq[lo:lo + _native.RIP_FPA_MAX_PLANES], n1, nside, masktype, ctx)
            for i, p in enumerate(have):   # the call above has returned: its kernels are done
                for j in (j for j, q in enumerate(ptypes) if q == p):
                    maps[j, k].copy_(means.t[i])
                    present[j, k] = 1
    stamps = []
    for j, (ptype, vmin, vmax, fmt) in enumerate(panels):
        if fmt is not None:
            stamps += scale_stamps(j, n1, ny, nx, ptype, vmin, vmax, fmt)
    return render(DevArray(maps).sync(), present, [p[1] for p in panels], [p[2] for p in panels], [p[3] is not None for p in panels],
                  n1, ny, nx, pos, table=table, font=font, stamps=stamps, nw=nw, ctx=ctx)


def make_big_image(infile_format, n1, ptype, vmin=0.0, vmax=1.0, mask=None, cmap="viridis", scaleformat=None, font=None, ctx=None,
                   geometry=None):
    """An RGB image (ny, nx, 3) uint8 of quantity ``ptype`` over the focal plane (:185-275)."""
    FILESTRING[ptype]
    nsca = len(_geometry(geometry)[1])
    planes = [load_sca(infile_format, k, [ptype]) for k in range(1, nsca + 1)]
    return multi_image_from_planes(planes, n1, mask, panels=((ptype, vmin, vmax, scaleformat),), cmap=cmap, font=font, ctx=ctx,
                                   geometry=geometry, nw=1)


def multi_image(infile_format, n1, masktype, font=None, ctx=None, geometry=None):
    """The multi-panel picture of the focal plane (:278-358): the 8 quantities of ``PANELS``, two abreast.  One pass per SCA:
    every file is opened once, ``dq`` and the planes are uploaded and binned by one call; one render, one download."""
    ctx = ctx or _native.default_context()
    nsca = len(_geometry(geometry)[1])
    ptypes = [p[0] for p in PANELS]

    def scas():   # one SCA's arrays at a time: the previous one's are released while the next is read
        for k in range(1, nsca + 1):
            yield load_sca(infile_format, k, ptypes)

    return multi_image_from_planes(_Lazy(scas(), nsca), n1, masktype, font=font, ctx=ctx, geometry=geometry)


class _Lazy:
    """a sequence of known length whose items are made as they are walked"""

    def __init__(self, it, n):
        self.it, self.n = it, n

    def __len__(self):
        return self.n

    def __iter__(self):
        return self.it


def main(argv=None):
    import argparse  # noqa: PLC0415

    from .maskhandling import PixelMask1  # noqa: PLC0415

    ap = argparse.ArgumentParser(prog="python -m romanimpreprocess_amd.utils.fpaplot", description=__doc__.split("\n\n")[0])
    ap.add_argument("format", help="format string of the input files: format.format(filestring, scanum)")
    ap.add_argument("out", help="the PNG file to write")
    ap.add_argument("--font", default=None, help="glyph table (text, 256 * 12 rows of 6 numbers); without it no text is drawn")
    ap.add_argument("--n1", type=int, default=128, help="bins per SCA side (a power of two)")
    ap.add_argument("--geometry", default=None, help="JSON file with nside, ctrs and bbox of another focal plane (default: the WFI's)")
    a = ap.parse_args(argv)
    geometry = None
    if a.geometry:
        import json  # noqa: PLC0415

        with open(a.geometry) as f:
            geometry = json.load(f)
    arr = multi_image(a.format, a.n1, PixelMask1, font=a.font, geometry=geometry)
    calio.write_png(a.out, arr[::-1, :, :])   # upside-down, as the script saves it (:371)


if __name__ == "__main__":
    main(sys.argv[1:])
