"""Drop-in for the line ``python -m solid_waffle.linearity_run linearity_pars_NN.json`` of the reference's
``runs/2026_July/make_sca_files_2026Jul.job``: the ``linearitylegendre`` file of one SCA from its flat, low-flat and dark ramps,
computed on the GPU.

    python -m romanimpreprocess_amd.calfiles.linearity_run <json>

The JSON is the one ``write_linearity_config.pl`` writes: ``SCA``, ``RAMPS`` (per set ``FORMAT`` -- 1: the ``2026_July`` layout, 6:
``summer2025`` --, ``FILE``, ``START``, ``NRAMP``, ``TSTART``), ``DARK`` (a Python-style index into ``RAMPS``; absent: none), ``TFRAME``
(default 3.04), ``P_ORDER``, ``OUTPUT``, ``SIGN`` (1 only), ``SLOPECUT``, ``BIAS`` (``FILE``, ``PATH``, ``SLICE``: the ``Sref`` plane) and
``NEGATIVEPAD``.  ``STOP`` and every other key are refused by name.  The bright set is the first entry of ``RAMPS`` that is not
the dark one (the Perl writer puts the high-intensity flat first).  Each exposure is read once, one set after the other, its
samples going to the device as stored (``RampStack``); where the sums of all sets do not fit into device memory, the frame is
worked in row bands and every exposure is read once per band.  Written are the ASDF tree ``roman: {meta, data, dq, Smin, Smax,
Sref, dark, pflat, ramperr}`` and the ``_asdf_to.fits`` dump of ``data``.  The fit follows the rule of ``rip_cal_linearity_fit``;
solid-waffle's source is not part of the reference and parity with it is unpinned.
"""

import json
import sys
from collections import namedtuple
from datetime import datetime, timezone

import numpy as np

from .. import _native, calio
from .make_dark_file import NSIDE, _open_dark

TFRAME = 3.04
FORMATS = {1: "2026_July", 6: "summer2025"}
TOP_KEYS = ("SCA", "RAMPS", "DARK", "TFRAME", "P_ORDER", "OUTPUT", "SIGN", "SLOPECUT", "BIAS", "NEGATIVEPAD")
RAMP_KEYS = ("FORMAT", "FILE", "START", "NRAMP", "TSTART")
BIAS_KEYS = ("FILE", "PATH", "SLICE")
MAX_SETS, MAX_ORDER, MAX_EXPOSURES = 8, 10, 65536   # linfit.hip

Ramp = namedtuple("Ramp", "layout files tstart")
Pars = namedtuple("Pars", "sca ramps dark bright tframe p_order output slopecut bias negativepad")


def _meta(sca):
    return {
        "author": "linearity_run.py",
        "description": "linearity_run.py",
        "instrument": {"detector": f"WFI{sca:02d}", "name": "WFI"},
        "origin": "PIT - romanimpreprocess",
        "date": datetime.now(timezone.utc).isoformat(),
        "pedigree": "DUMMY",
        "reftype": "LINEARITYLEGENDRE",
        "telescope": "ROMAN",
        "useafter": "!time/time-1.2.0 2020-01-01T00:00:00.000",
    }


def ramp_files(first, start, nramp):
    """``first[:-8] + "NNN.fits"`` for NNN = start .. start + nramp - 1: the numbering of ``make_dark_file.noise_files``"""
    return [first[:-8] + f"{j:03d}.fits" for j in range(int(start), int(start) + int(nramp))]


def _need(d, keys, known, where):
    for k in d:
        if k not in known:
            raise ValueError(f"{where}: unknown key {k!r}" + (" (a part of the image only: not supported)" if k == "STOP" else ""))
    for k in keys:
        if k not in d:
            raise ValueError(f"{where}: key {k!r} is missing")


def parse_config(cfg):
    """The dict of a ``linearity_pars_NN.json`` as ``Pars``; ValueError naming the key on anything this step does not do."""
    _need(cfg, ("SCA", "RAMPS", "P_ORDER", "OUTPUT", "SLOPECUT", "BIAS", "NEGATIVEPAD"), TOP_KEYS, "linearity_run")
    if int(cfg.get("SIGN", 1)) != 1:
        raise ValueError(f"linearity_run: SIGN {cfg['SIGN']} (only 1, an increasing ramp, is supported)")
    p = int(cfg["P_ORDER"])
    if not 1 <= p <= MAX_ORDER:
        raise ValueError(f"linearity_run: P_ORDER {p} (1..{MAX_ORDER} supported)")
    slopecut = float(cfg["SLOPECUT"])
    if not 0.0 < slopecut < 1.0:
        raise ValueError(f"linearity_run: SLOPECUT {slopecut} (must lie in (0, 1))")
    sets = cfg["RAMPS"]
    if not isinstance(sets, list) or not 1 <= len(sets) <= MAX_SETS:
        raise ValueError(f"linearity_run: RAMPS holds {len(sets) if isinstance(sets, list) else 'no'} sets (1..{MAX_SETS} supported)")
    ramps = []
    for j, r in enumerate(sets):
        _need(r, RAMP_KEYS, RAMP_KEYS, f"linearity_run: RAMPS[{j}]")
        if int(r["FORMAT"]) not in FORMATS:
            raise ValueError(f"linearity_run: RAMPS[{j}]: FORMAT {r['FORMAT']} (known: {sorted(FORMATS)})")
        if not 1 <= int(r["NRAMP"]) <= MAX_EXPOSURES:
            raise ValueError(f"linearity_run: RAMPS[{j}]: NRAMP {r['NRAMP']} (1..{MAX_EXPOSURES} supported)")
        if int(r["TSTART"]) < 1:
            raise ValueError(f"linearity_run: RAMPS[{j}]: TSTART {r['TSTART']} (frames count from 1)")
        if int(r["START"]) < 0 or not str(r["FILE"]).endswith(".fits") or len(str(r["FILE"])) < 8:
            raise ValueError(f"linearity_run: RAMPS[{j}]: FILE {r['FILE']!r}, START {r['START']} (a name that ends in NNN.fits is needed)")
        ramps.append(Ramp(FORMATS[int(r["FORMAT"])], ramp_files(str(r["FILE"]), r["START"], r["NRAMP"]), int(r["TSTART"])))
    dark = -1
    if "DARK" in cfg:
        dark = int(cfg["DARK"])
        if not -len(ramps) <= dark < len(ramps):
            raise ValueError(f"linearity_run: DARK {dark} outside the {len(ramps)} sets of RAMPS")
        dark %= len(ramps)
    lit = [j for j in range(len(ramps)) if j != dark]
    if not lit:
        raise ValueError("linearity_run: DARK names the only set of RAMPS: no flat is left")
    bias = cfg["BIAS"]
    _need(bias, BIAS_KEYS, BIAS_KEYS, "linearity_run: BIAS")
    if not isinstance(bias["PATH"], list):
        raise ValueError("linearity_run: BIAS: PATH must be the list of keys that leads to the array")
    tframe, negativepad = float(cfg.get("TFRAME", TFRAME)), float(cfg["NEGATIVEPAD"])
    if not tframe > 0.0:
        raise ValueError(f"linearity_run: TFRAME {tframe} (must be positive)")
    if not negativepad >= 0.0:
        raise ValueError(f"linearity_run: NEGATIVEPAD {negativepad} (must not be negative)")
    return Pars(int(cfg["SCA"]), ramps, dark, lit[0], tframe, p, str(cfg["OUTPUT"]), slopecut,
                (str(bias["FILE"]), [str(k) for k in bias["PATH"]], int(bias["SLICE"])), negativepad)


def read_sref(bias):
    """the ``Sref`` plane: element ``SLICE`` of the array at ``PATH`` of the ASDF file ``FILE``, as float32"""
    path, keys, index = bias
    with calio.open_tree(path) as f:
        node = f
        for k in keys:
            node = node[k]
        return np.ascontiguousarray(np.asarray(node[index]), dtype=np.float32)


def run(config, *, nside=NSIDE, nb=4, band_rows=None, ctx=None):
    """Write the file ``OUTPUT`` of ``config`` (a path to the JSON, or its dict) and its ``_asdf_to.fits`` sibling; returns the
    two paths.  ``nside``: the side of the detector (smaller frames: for tests); ``band_rows``: rows per band (default: the whole
    frame where the sums of all sets fit into four fifths of the free device memory)."""
    import torch

    from .linfit import KEYS, RampStack, derive_linearity

    if not isinstance(config, dict):
        with open(config) as f:
            config = json.load(f)
    pars = parse_config(config)
    ctx = ctx or _native.default_context()
    sref = read_sref(pars.bias)
    if sref.ndim != 2:
        raise ValueError(f"linearity_run: BIAS: element SLICE of PATH is {sref.shape}, not a plane")
    ny = sref.shape[0]
    nx = min(int(nside), sref.shape[1])
    sref = np.ascontiguousarray(sref[:, :nx])
    shapes = [_open_dark(r.files[0], r.layout).shape for r in pars.ramps]
    for j, (r, s) in enumerate(zip(pars.ramps, shapes)):
        if s[1] != ny or s[2] < nx:
            raise ValueError(f"linearity_run: RAMPS[{j}]: {r.files[0]} holds {s[1]} x {s[2]} frames, Sref is {ny} x {nx}")
        if s[0] - (r.tstart - 1) < 2:
            raise ValueError(f"linearity_run: RAMPS[{j}]: TSTART {r.tstart} leaves fewer than 2 of the {s[0]} frames")
    if band_rows is None:
        free = int(torch.cuda.mem_get_info(ctx.device)[0])
        per_row = sum(4 * s[0] * nx for s in shapes) + max(2 * s[0] * s[2] for s in shapes) + nx * (4 * (pars.p_order + 8) + 2 * len(shapes))
        band_rows = max(1, min(ny, int(0.8 * free) // per_row))
    nlit = len(pars.ramps) - (pars.dark >= 0)
    out = {"data": np.empty((pars.p_order + 1, ny, nx), np.float32), "dq": np.empty((ny, nx), np.uint32),
           "Smin": np.empty((ny, nx), np.float32), "Smax": np.empty((ny, nx), np.float32), "Sref": sref,
           "dark": np.empty((ny, nx), np.float32), "pflat": np.empty((nlit, ny, nx), np.float32),
           "ramperr": np.empty((len(pars.ramps), ny, nx), np.uint16)}
    for y0 in range(0, ny, int(band_rows)):
        y1 = min(ny, y0 + int(band_rows))
        stacks = []
        for j, (r, s) in enumerate(zip(pars.ramps, shapes)):
            stack = RampStack(s[0], ny, nx, ctx=ctx, rows=(y0, y1))
            for name in r.files:
                print("ramp set", j, "rows", y0, y1, name)
                sys.stdout.flush()
                stack.add(_open_dark(name, r.layout), fits_be16=True)
            stacks.append(stack)
        planes = derive_linearity(stacks, sref[y0:y1], p_order=pars.p_order, tframe=pars.tframe, slopecut=pars.slopecut,
                                  negativepad=pars.negativepad, tstart=[r.tstart for r in pars.ramps],
                                  dark=None if pars.dark < 0 else pars.dark, bright=pars.bright, nb=nb, rows=(y0, ny), ctx=ctx)
        for k in KEYS:
            if k != "Sref":
                out[k][..., y0:y1, :] = planes[k].numpy()
        del stacks, planes
    print("linearity quality -->", np.count_nonzero(out["dq"][nb:ny - nb, nb:nx - nb]), "science pixels flagged.")
    calio.write_asdf(pars.output, {"roman": {"meta": _meta(pars.sca), **{k: out[k] for k in KEYS}},
                                   "notes": {"config": json.dumps(config)}})
    dump = pars.output[:-5] + "_asdf_to.fits"
    calio.write_fits(dump, [out["data"]], ctx=ctx)
    return pars.output, dump


if __name__ == "__main__":
    run(sys.argv[1])
