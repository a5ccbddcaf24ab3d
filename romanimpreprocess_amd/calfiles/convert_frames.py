"""The reference's three converters of the raw test-stand frames -- ``runs/summer2025run/convert_dark.py``, ``convert_flt.py`` and
``convert_loflt.py`` -- on the GPU (``csrc/rawframes.hip``): the N single-frame files of an exposure go to the device as stored,
are decoded, turned from the detector frame to the science frame and stacked into a ``(1, N, ny, nx)`` uint16 cube in HBM
(``frames_to_cube``), the two unweighted slope images are made from the resident cube in one launch (``cube_slopes``), and the
three-HDU file is written from HBM (``convert``, through ``calio.write_fits``).  The cube can go on to ``DarkStack.add``
(``make_dark_file.dark_data`` takes such cubes) without touching the disk.  Line numbers below are ``convert_flt.py``'s.

The cube is the script's in every bit and so are the slopes: their arithmetic is exact up to one float64 division and one
conversion to float32 (``rip_cal_frame_slopes`` in ``include/romanhip.h``).  ``calio`` writes cards without comments, so ``PROVEN``,
``NMAX`` and ``FRDnnn`` carry the script's values and not its comments; a file name that does not fit into one card is refused by
name (astropy would write ``CONTINUE`` cards).
"""

import datetime
import glob
import os
import re
import sys

import numpy as np

from .. import _native, calio
from ..devarray import DevArray, is_dev, to_device

# kind -> (prefix of the input files, name in the output file, PROVEN, exposures looked for, Nc clamped to 10)
KINDS = {
    "dark": ("Total_Noise_exp", "Noise", "convert_dark.py", range(1, 101), False),
    "flt": ("linearity_exp", "Flat", "convert_flt.py", range(1, 51), True),
    "loflt": ("Gain_exp", "LoFlat", "convert_loflt.py", range(1, 51), True),
}
_FRAME_FILE = re.compile(r"[0123456789ABCDEFabcdef]\.fits$")   # :43, strips out the guide window files


def find_frames(indir, prefix, j, sca):
    """``:24-45``: the files ``<indir>/<prefix>{j}_*SCU{sca:02d}*.fits`` in sorted order, without the guide-window files (only
    names that end in a hexadecimal digit before ``.fits`` are kept).  Needs no GPU."""
    pattern = os.path.join(glob.escape(os.fspath(indir)), f"{prefix}{int(j):d}_*SCU{int(sca):02d}*.fits")
    return [f for f in sorted(glob.glob(pattern)) if _FRAME_FILE.search(f)]


def slope_weights(nc):
    """``:70-78`` on the host, in float64 as the script: ``(w0, de0, w1, de1)`` with ``w0[k] = k - nc / 2.0`` for ``k = 1 .. nc-1``,
    ``w1[k] = k - (nc // 2) / 2.0`` for ``k = 1 .. nc // 2 - 1`` (the other entries 0) and ``de`` the running sums of their squares."""
    nc = int(nc)
    w0, w1 = np.zeros(nc, np.float64), np.zeros(nc, np.float64)
    de0 = 0.0
    for k in range(1, nc):
        w0[k] = k - nc / 2.0
        de0 = de0 + (k - nc / 2.0) ** 2
    de1 = 0.0
    for k in range(1, nc // 2):
        w1[k] = k - (nc // 2) / 2.0
        de1 = de1 + (k - (nc // 2) / 2.0) ** 2
    return w0, de0, w1, de1


def _open_frame(path):
    """(header, samples as stored viewed as uint16, ``stored`` code of ``rip_cal_raw_frame``) of the primary HDU of ``path``"""
    hdr, _ = calio.read_fits_image(path, 0, header_only=True)
    bitpix, bzero, bscale = hdr.get("BITPIX"), hdr.get("BZERO", 0), hdr.get("BSCALE", 1)
    if bitpix != 16 or bscale != 1 or bzero not in (0, 32768) or hdr.get("NAXIS") != 2:
        raise ValueError(f"{path}: a frame of 16-bit samples is needed (BITPIX 16 with BZERO 32768, or without BZERO), not "
                         f"BITPIX {bitpix}, BZERO {hdr.get('BZERO')}, BSCALE {hdr.get('BSCALE')}, NAXIS {hdr.get('NAXIS')}")
    hdr, data = calio.read_fits_image(path, 0)
    return hdr, data.view(np.uint16), 1 if bzero == 32768 else 2


def _dev_empty(shape, dtype, ctx):
    import torch

    tdt = {np.dtype(np.uint16): torch.int16, np.dtype(np.float32): torch.float32}[np.dtype(dtype)]
    return DevArray(torch.empty(shape, dtype=tdt, device=f"cuda:{ctx.device}"), dtype)


def frames_to_cube(files, sca, nflip=4096, ctx=None):
    """``:53-63``: the primary HDUs of ``files`` as one ``(1, N, ny, nx)`` uint16 cube in the science frame, a ``DevArray``, and
    the list of their ``DATE`` cards.  ``sca % 3 == 0``: the columns ``0 .. nflip-1`` of every row are reversed (the reference
    output behind them stays); otherwise the rows are.  ``ny`` and ``nx`` are the first file's; a file of another shape is refused
    by name.  Each file is mapped (``calio.read_fits_image``) and its samples go to the device as stored."""
    import torch

    ctx = ctx or _native.default_context()
    files = [os.fspath(f) for f in files]
    if not files:
        raise ValueError("frames_to_cube: no files")
    _, first, _ = _open_frame(files[0])
    ny, nx = first.shape
    del first
    need = 2 * (len(files) + 1) * ny * nx   # the cube, and one frame as stored
    free = int(torch.cuda.mem_get_info(ctx.device)[0])
    if need > free:
        raise MemoryError(f"the cube of {len(files)} frames of {ny} x {nx} needs {need} bytes and {free} bytes of device memory are free")
    cube = _dev_empty((1, len(files), ny, nx), np.uint16, ctx)
    cube.sync()
    orient = 1 if int(sca) % 3 == 0 else 2
    dates = []
    for k, name in enumerate(files):
        hdr, data, stored = _open_frame(name)
        if data.shape != (ny, nx):
            raise ValueError(f"{name}: a frame of {data.shape[0]} x {data.shape[1]} samples in an exposure of {ny} x {nx} frames "
                             f"({files[0]})")
        dates.append(hdr["DATE"])
        ctx.call("rip_cal_raw_frame", data, _native.RIP_HOST, ny, nx, orient, int(nflip), stored, DevArray(cube.t[0, k], np.uint16))
    return cube, dates


def cube_slopes(cube, nc, ctx=None):
    """``:65-79``: the two slope images of ``cube`` -- uint16 ``(1, N, ny, nx)`` or ``(N, ny, nx)``, a ``DevArray`` or a numpy array
    (uploaded) -- from its first ``nc`` frames, the very first dropped: float32 ``(2, ny, nx)``, a ``DevArray``."""
    ctx = ctx or _native.default_context()
    if not is_dev(cube):
        cube = np.asarray(cube)
    if cube.dtype != np.dtype(np.uint16) or cube.ndim not in (3, 4) or (cube.ndim == 4 and cube.shape[0] != 1):
        raise TypeError(f"a uint16 cube (1, N, ny, nx) or (N, ny, nx) is needed, not {cube.dtype.name} {tuple(cube.shape)}")
    if not is_dev(cube):
        cube = to_device(cube, ctx.device)
    n, ny, nx = cube.shape[-3:]
    if min(n, ny, nx) < 1 or not 1 <= int(nc) <= n:
        raise ValueError(f"nc = {nc} frames of a cube of {n} frames of {ny} x {nx}")
    w0, de0, w1, de1 = slope_weights(nc)
    slp = _dev_empty((2, ny, nx), np.float32, ctx)
    cube.sync()
    ctx.call("rip_cal_frame_slopes", cube, n, int(nc), ny * nx, w0, de0, w1, de1, slp, _native.RIP_DEVICE)
    return slp


def exposure_cards(proven, N, files, dates, now=None):
    """``:84-92``: the cards of the cube's HDU in the script's order -- ``PROVEN``, ``NMAX``, ``DATE`` (local time, or ``now``),
    then ``FRnnn`` (base name of file n) and ``FRDnnn`` (its ``DATE``) alternating.  A name that does not fit into one card is
    refused by name.  Needs no GPU."""
    now = datetime.datetime.now() if now is None else now
    cards = [("PROVEN", proven), ("NMAX", int(N)), ("DATE", now.strftime("%Y-%m-%d %H:%M:%S"))]
    for k in range(int(N)):
        fname = files[k].split("/")[-1]
        try:
            calio.fits_header(None, None, cards=[(f"FR{k + 1:03d}", fname)])
        except ValueError as e:
            raise ValueError(f"{fname}: the file name does not go into one FITS card (CONTINUE cards are not written): {e}") from None
        cards += [(f"FR{k + 1:03d}", fname), (f"FRD{k + 1:03d}", dates[k])]
    return cards


def convert(kind, indir, N, outdir, sca, *, exposures=None, nflip=4096, now=None, ctx=None):
    """The converter ``kind`` (``dark``, ``flt``, ``loflt``) with the script's arguments: for every exposure ``j`` (1..100 for the
    darks, 1..50 for the flats; ``exposures`` narrows that) that has ``N`` frame files of ``sca`` in ``indir``, write
    ``<outdir>/99999999_SCA{sca:02d}_{Noise|Flat|LoFlat}_{j:03d}.fits``: an empty primary HDU with ``TGROUP``, the uint16 cube
    ``(1, N, ny, nx)`` with the cards of ``exposure_cards`` and the float32 slopes ``(2, ny, nx)`` with ``BUNIT``, both data units
    from HBM.  ``now`` (a ``datetime``) fixes the ``DATE`` card.  Prints the script's progress lines; returns the files written."""
    if kind not in KINDS:
        raise ValueError(f"kind {kind!r} is not one of {', '.join(KINDS)}")
    prefix, outname, proven, js, clamp = KINDS[kind]
    ctx = ctx or _native.default_context()
    N, sca = int(N), int(sca)
    if N < 1:
        raise ValueError(f"{N} frames")
    written = []
    for j in js:
        if exposures is not None and j not in exposures:
            continue
        print("Looking for files in", os.fspath(indir) + f"/{prefix}{j:d}_")
        files = find_frames(indir, prefix, j, sca)
        print(f"SCU{sca:02d}, found {len(files):3d} files")
        if len(files) < N:
            print(f"could not complete SCU{sca:02d}, continuing ...")
            continue
        files = files[:N]
        cube, dates = frames_to_cube(files, sca, nflip=nflip, ctx=ctx)
        slp = cube_slopes(cube, min(N, 10) if clamp else N, ctx=ctx)
        outfile = os.fspath(outdir) + f"/99999999_SCA{sca:02d}_{outname}_{j:03d}.fits"
        print(">>", outfile)
        cards = exposure_cards(proven, N, files, dates, now)
        for name in files:
            print(name.split("/")[-1])
        sys.stdout.flush()
        calio.write_fits(outfile, [{"data": None, "cards": [("TGROUP", 3.04)]}, {"data": cube, "cards": cards},
                                   {"data": slp, "cards": [("BUNIT", "DN/frame")]}], ctx=ctx)
        written.append(outfile)
        del cube, slp
    return written


def main(kind, argv):
    """the scripts' command line: <input directory> <Number of frames> <output directory> <sca>"""
    convert(kind, argv[1], int(argv[2]), argv[3], int(argv[4]))
