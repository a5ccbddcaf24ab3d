"""Drop-in for the reference's ``runs/2026_July/make_dark_file.py``: the ``dark`` and ``read`` (read noise) files of one read
pattern from a set of dark exposures and the noise summary solid-waffle made of them, computed on the GPU.

    python -m romanimpreprocess_amd.calfiles.make_dark_file <pattern> <first noise file> <noise summary> <sca> <outfile>

Same conventions: ``settings_<pattern>.yaml`` (``READS``) is read from the working directory, the exposures are ``<first noise
file>`` with its ``001.fits`` counted up until a file is missing (500 at most), the read-noise file's name is ``<outfile>`` with
``_dark_`` replaced by ``_read_``, and the two trees have the script's layout and keys (``data``, ``dq``, ``dark_slope``,
``dark_slope_err``; ``data``, ``resetnoise``, ``anc``, ``amp33`` with the script's placeholder where the summary has no ``AMP33``
extension).  Every exposure is read ONCE (the script opens each once per group): its samples go to the device as stored and
``DarkStack`` keeps the group means of all exposures in HBM; where they do not fit, the frame is worked in row bands and the
exposures are read once per band.  The two ``_asdf_data.fits`` display dumps of the script are written too (``calio.write_fits``:
an empty primary HDU and the planes of each tree, byte order made on the device).  The clipped mean follows the rule of ``rip_cal_sigma_clip_mean``; parity with astropy is unpinned.
Where the noise summary does not exist yet, ``run(..., noise_out=None, noise_args=[...])`` makes it in the same pass over the
exposures (``noise_run.Feeder``, ``NoiseStack``), writes it where ``noise_run`` would and goes on with its planes from HBM.
"""

import sys
from datetime import datetime, timezone
from os.path import exists
from os.path import split as pathsplit

import numpy as np
import yaml

from .. import _native, calio
from ..devarray import DevArray, is_dev
from .darkstack import DarkStack, derive_dark_planes

NSIDE = 4096   # dimension of H4RG (make_dark_file.py:26)
CHANNELWIDTH = 128   # columns of a read-out channel and of the reference output


def _meta(pattern, sca, ng, reftype):
    return {
        "author": "make_dark_file.py",
        "description": "make_dark_file.py",
        "exposure": {"groupgap": 0, "ma_table_name": pattern, "ma_table_number": 1000000, "nframes": 1, "ngroups": ng,
                     "p_exptype": "WFI_IMAGE|", "type": "WFI_IMAGE"},
        "instrument": {"detector": f"WFI{sca:02d}", "name": "WFI", "optical_element": "F158"},
        "origin": "PIT - romanimpreprocess",
        "date": datetime.now(timezone.utc).isoformat(),
        "pedigree": "DUMMY",
        "reftype": reftype,
        "telescope": "ROMAN",
        "useafter": "!time/time-1.2.0 2020-01-01T00:00:00.000",
    }


def noise_files(target):
    """``make_dark_file.py:38-48``: ``target[:-8] + "NNN.fits"`` for NNN = 001, 002, ... while the file exists, 500 at most."""
    out = []
    while len(out) < 500:
        name = target[:-8] + f"{len(out) + 1:03d}.fits"
        if not exists(name):
            break
        out.append(name)
    return out


LAYOUTS = ("2026_July", "summer2025")


def _open_dark(path, layout="2026_July"):
    """the (nreads, ny, width) samples of one dark exposure as stored.  ``2026_July``: the primary HDU; ``summer2025``
    (``runs/summer2025run/make_dark_file.py:60-66``, the files of ``convert_dark``): element 0 of the (1, N, ny, nx) cube of HDU 1"""
    summer = layout == "summer2025"
    hdr, data = calio.read_fits_image(path, 1 if summer else 0)
    if summer and data is not None and data.ndim == 4 and data.shape[0] >= 1:
        data = data[0]
    if data is None or data.ndim != 3 or hdr.get("BITPIX") != 16 or hdr.get("BZERO", 0) != 32768 or hdr.get("BSCALE", 1) != 1:
        raise ValueError(f"{path}: a cube of unsigned 16-bit samples (BITPIX 16, BZERO 32768) is needed")
    return data


def _dev_cube(cube):
    """an exposure that is in HBM already (``convert_frames.frames_to_cube``): uint16 (1, N, ny, nx) or (N, ny, nx)"""
    if cube.dtype != np.dtype(np.uint16) or cube.ndim not in (3, 4) or (cube.ndim == 4 and cube.shape[0] != 1):
        raise TypeError(f"a uint16 DevArray cube (1, N, ny, nx) or (N, ny, nx) is needed, not {cube.dtype.name} {tuple(cube.shape)}")
    return DevArray(cube.t[0], np.uint16) if cube.ndim == 4 else cube


def dark_data(files, reads, nside=NSIDE, band_rows=None, ctx=None, layout="2026_July", each=None):
    """The clipped mean of the group means of ``files``, float32 (ng, ny, min(nside, width)): one pass over the files, or one
    per band of ``band_rows`` rows (default: as many rows as fit into four fifths of the free device memory).  ``layout``: where
    an exposure sits in its file (``_open_dark``).  ``files`` may also be a list of ``DevArray`` cubes, uint16 (1, N, ny, nx) or
    (N, ny, nx) in native samples: they are read where they are and no file is opened.  ``each(cube, fits_be16)`` is handed
    every exposure of the first pass as well (``noise_run.Feeder.feed``: the noise summary from the same read)."""
    import torch

    if layout not in LAYOUTS:
        raise ValueError(f"layout {layout!r} is not one of {', '.join(LAYOUTS)}")
    ctx = ctx or _native.default_context()
    resident = len(files) > 0 and all(is_dev(f) for f in files)
    first = _dev_cube(files[0]) if resident else _open_dark(files[0], layout)
    _, ny, width = first.shape
    nx = min(int(nside), width)
    ng = len(reads) // 2
    if band_rows is None:
        free = int(torch.cuda.mem_get_info(ctx.device)[0])
        nreads_bytes = 0 if resident else first.shape[0] * width * 2   # the staged samples of one exposure, per row
        band_rows = max(1, min(ny, int(0.8 * free) // (4 * ng * len(files) * nx + nreads_bytes)))
    del first
    out = np.empty((ng, ny, nx), np.float32)
    for y0 in range(0, ny, int(band_rows)):
        y1 = min(ny, y0 + int(band_rows))
        stack = DarkStack(reads, ny, nx, len(files), ctx=ctx, rows=(y0, y1))
        for j, name in enumerate(files):
            if j % 10 == 0:
                print("loading groups", y0, j)
                sys.stdout.flush()
            cube = _dev_cube(name) if resident else _open_dark(name, layout)
            stack.add(cube, fits_be16=not resident)
            if each is not None and y0 == 0:
                each(cube, not resident)
        mean = stack.finish(sigma=3)
        out[:, y0:y1, :] = mean.numpy() if is_dev(mean) else mean
        del stack
    return out


def run(pattern, target, noise_out, sca, outfile, *, reads=None, nside=NSIDE, band_rows=None, ctx=None, layout="2026_July",
        noise_args=None, channelwidth=CHANNELWIDTH):
    """Write the dark file ``outfile`` and its read-noise sibling; returns their two paths.  ``reads`` (the flat ``READS`` list)
    replaces the yaml of the working directory; ``nside`` is the script's constant (smaller frames: for tests); ``layout``
    ``"summer2025"`` reads the exposures as ``convert_dark`` writes them (``dark_data``).  ``noise_out`` None: there is no noise
    summary yet; it is made in the same pass over the exposures from ``noise_args``, the options of the job's ``noise_run`` line
    (``["-f", "1", "-o", <summary>, "-n", "100", "-t", "3", "-tn", "34", "-ro", ...]``; ``-i`` is ``target``), written to its
    ``-o`` as ``noise_run`` writes it, and its planes go on from HBM; the two files are the ones a run on that summary gives."""
    sca, nside = int(sca), int(nside)
    if reads is None:
        with open("settings_" + pattern + ".yaml") as f:
            reads = yaml.safe_load(f)["READS"]
    ng = len(reads) // 2
    print("Read pattern:", [list(range(int(reads[2 * j]), int(reads[2 * j + 1]))) for j in range(ng)])
    files = noise_files(target)
    print(files)
    if not files:
        raise FileNotFoundError(f"no noise file {target[:-8]}001.fits")
    feeder = None
    if noise_out is None:
        from . import noise_run

        if noise_args is None:
            raise ValueError("without a noise summary, noise_args (the options of the noise_run line) are needed")
        na = noise_run.parse(["-i", target] + [str(v) for v in noise_args])
        feeder = noise_run.Feeder(na.tstart, na.nframe, na.ref_out, na.tframe, nside=nside, cw=channelwidth, ndark=na.ndark, ctx=ctx)
    darkave = dark_data(files, reads, nside=nside, band_rows=band_rows, ctx=ctx, layout=layout, each=feeder and feeder.feed)

    # the dark current maps, read noise and reset noise of the summary
    if feeder is not None:
        made = feeder.finish()
        noise_out = na.out
        noise_run.write(noise_out, made, na.cdscut, na.rowover, ctx=ctx)
        header, summary = calio.read_fits_image(noise_out, 1, header_only=True)[0], made.planes   # the planes stay in HBM
    else:
        header, summary = calio.read_fits_image(noise_out, 1)

    def plane(key):
        if feeder is not None:
            return DevArray(summary.t[int(header[key])], np.float32)
        return np.asarray(summary[int(header[key])], dtype=np.float32)

    dark_slope, dark_slope_err, read_noise = derive_dark_planes(plane("DARK1"), plane("DARK2"), plane("DARK1ERR"), plane("DARK2ERR"),
                                                                plane("CDS"), nside=nside, ctx=ctx)
    reset_noise = plane("RESET")
    if feeder is not None:
        dark_slope, dark_slope_err, read_noise, reset_noise = (a.numpy() for a in (dark_slope, dark_slope_err, read_noise, reset_noise))
    reset_noise = np.ascontiguousarray(reset_noise[:, :nside])
    try:   # AMP33 if it is there
        if feeder is not None:
            if made.amp33 is None:
                raise KeyError("AMP33")
            h33, d33 = calio.read_fits_image(noise_out, "AMP33", header_only=True)[0], made.amp33.numpy()
        else:
            h33, d33 = calio.read_fits_image(noise_out, "AMP33")
        amp33 = {"valid": True, "med": np.array(d33[0], dtype=np.float32), "std": np.array(d33[1], dtype=np.float32),
                 "M_PINK": float(h33["M_PINK"]), "RU_PINK": float(h33["RU_PINK"])}
    except (KeyError, ValueError, TypeError):   # placeholders
        amp33 = {"valid": False, "med": np.zeros((4096, 128), dtype=np.float32), "std": np.zeros((4096, 128), dtype=np.float32),
                 "M_PINK": 0.0, "RU_PINK": 0.0}

    dq = np.zeros((nside, nside), np.uint32)
    calio.write_asdf(outfile, {
        "roman": {"meta": _meta(pattern, sca, ng, "DARK"), "data": darkave, "dq": dq,
                  "dark_slope": dark_slope, "dark_slope_err": dark_slope_err},
        "notes": {"noise_header": header.text}})
    # this stuff is just so that we can also display the images in ds9 (make_dark_file.py:143-151, 208-210)
    calio.write_fits(outfile[:-5] + "_asdf_data.fits", [None, darkave, dq, dark_slope, dark_slope_err], ctx=ctx)
    head, tail = pathsplit(outfile)
    outfile2 = head + "/" + tail.replace("_dark_", "_read_")
    calio.write_asdf(outfile2, {
        "roman": {"meta": _meta(pattern, sca, ng, "READNOISE"), "data": read_noise, "resetnoise": reset_noise,
                  # this information won't be read by romancal, but some simulators may want it
                  "anc": {"ACN": header["ACN"], "C_PINK": header["C_PINK"], "U_PINK": header["U_PINK"], "UNIT": "DN"},
                  "amp33": amp33},
        "notes": {"noise_header": header.text}})
    calio.write_fits(outfile2[:-5] + "_asdf_data.fits", [None, read_noise, reset_noise], ctx=ctx)
    return outfile, outfile2


if __name__ == "__main__":
    run(sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4]), sys.argv[5])
