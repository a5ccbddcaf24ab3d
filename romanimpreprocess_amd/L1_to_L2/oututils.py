"""What the reference adds to the L2 tree after ``make_asdf`` -- ``L1_to_L2/oututils.py`` (``add_in_ref_data`` :42-55,
``add_in_provenance`` :106-110) and ``utils/typefix.py`` (``fix`` :22-56) -- and the planes of the tree itself, made on the GPU.

  * ``l2_planes``: the active-region planes (data, dq, var_rnoise, var_poisson, err; the last three float32 or float16) and the
    four flag strips ``dq_border_ref_pix_*`` from the chain's full-frame results: ``rip_stage_l2_planes`` (``csrc/l2out.hip``);
  * ``refpix_strips``: ``border_ref_pix_*``, the float32 edges of the Level-1 cube: ``rip_stage_l2_refpix_strips``;
  * ``add_in_provenance``, ``add_dummy_fields``: the metadata and the placeholder planes, on the host (no arithmetic).
Both stage functions take numpy arrays (and return numpy arrays) or ``DevArray``s (and return ``DevArray``s that are complete).
``update_flags`` is commented out at the reference's call site (``gen_cal_image.py:677``) and has no counterpart here; the schema
validation loop of ``typefix.fix`` needs ``asdf``: its outcome is the configuration key ``L2_FLOAT16`` of ``calibrateimage``.
"""

import numpy as np

from .. import __version__, _native
from ..devarray import DevArray, is_dev

SIDES = ("left", "right", "top", "bottom")
SOFTWARE_NAME = "gen_cal_image / HLWAS PIT"   # the reference's value (oututils.py:107): readers may key on it
DUMMY_FIELDS = ("chisq", "dumo")              # typefix.py:23


def empty_arrays(dev, like, specs):
    """name -> an uninitialised array of (shape, numpy dtype): a ``DevArray`` on the device of the ``DevArray`` ``like`` (uint32
    bits in an int32 tensor) where ``dev``, else a numpy array"""
    if not dev:
        return {name: np.empty(shape, dtype) for name, (shape, dtype) in specs.items()}
    import torch

    carrier = {"float32": torch.float32, "float16": torch.float16, "uint32": torch.int32, "uint8": torch.uint8}
    return {name: DevArray(torch.empty(shape, dtype=carrier[np.dtype(dtype).name], device=like.t.device), dtype)
            for name, (shape, dtype) in specs.items()}


def _same_place(arrays, what):
    dev = [is_dev(a) for a in arrays]
    if any(dev) and not all(dev):
        raise TypeError(f"{what}: the arrays are all numpy arrays or all DevArrays")
    return dev[0]


def l2_planes(slope, err_read, err_poisson, pixeldq, nb, float16=False, ctx=None):
    """dict(data, dq, var_rnoise, var_poisson, err, dq_border_ref_pix_left / _right / _top / _bottom) from the (ny, nx) results of
    the chain: the first five over the active region (ny - 2 nb, nx - 2 nb), ``var_* = err_* ** 2`` and ``err = sqrt(var_rnoise +
    var_poisson)`` in float32, stored as float32 or (``float16``) rounded to float16 as ``astype(np.float16)`` rounds; the strips
    are ``pixeldq[:, :nb]``, ``[:, -nb:]``, ``[-nb:, :]``, ``[:nb, :]``."""
    ctx = ctx or _native.default_context()
    dev = _same_place((slope, err_read, err_poisson, pixeldq), "l2_planes")
    if not dev:
        slope, err_read, err_poisson = (np.ascontiguousarray(a, dtype=np.float32) for a in (slope, err_read, err_poisson))
        pixeldq = np.ascontiguousarray(pixeldq, dtype=np.uint32)
    ny, nx = slope.shape
    for a in (err_read, err_poisson, pixeldq):
        if tuple(a.shape) != (ny, nx):
            raise ValueError(f"l2_planes: planes of shapes {(ny, nx)} and {tuple(a.shape)}")
    if nb < 0 or 2 * nb >= ny or 2 * nb >= nx:
        raise ValueError(f"l2_planes: a border of {nb} leaves no active region in a {ny} x {nx} frame")
    act, vt = (ny - 2 * nb, nx - 2 * nb), (np.float16 if float16 else np.float32)
    specs = {"data": (act, np.float32), "dq": (act, np.uint32), "var_rnoise": (act, vt), "var_poisson": (act, vt), "err": (act, vt)}
    specs.update({f"dq_border_ref_pix_{s}": ((ny, nb) if s in ("left", "right") else (nb, nx), np.uint32) for s in SIDES})
    out = empty_arrays(dev, slope, specs)
    ctx.call("rip_stage_l2_planes", slope, err_read, err_poisson, pixeldq, ny, nx, nb, _native.RIP_F16 if float16 else _native.RIP_F32,
             _native.location_of(slope), *(out[k] if out[k].size else None for k in specs))
    if dev:
        ctx.synchronize()
    return out


def refpix_strips(cube, nb, ctx=None):
    """dict(border_ref_pix_left / _right (ngrp, ny, nb), _top / _bottom (ngrp, nb, nx)) float32: ``cube[:, :, :nb]``,
    ``cube[:, :, -nb:]``, ``cube[:, -nb:, :]``, ``cube[:, :nb, :]`` of a uint16 or float32 Level-1 cube (oututils.py:46-49)."""
    ctx = ctx or _native.default_context()
    dev = is_dev(cube)
    if not dev:
        cube = np.ascontiguousarray(cube)
    if cube.dtype not in (np.uint16, np.float32) or cube.ndim != 3:
        raise TypeError(f"refpix_strips: a uint16 or float32 cube (ngrp, ny, nx), not {cube.dtype} {tuple(cube.shape)}")
    ngrp, ny, nx = cube.shape
    if nb < 0 or nb > ny or nb > nx:
        raise ValueError(f"refpix_strips: nb = {nb} in a {ny} x {nx} frame")
    specs = {f"border_ref_pix_{s}": ((ngrp, ny, nb) if s in ("left", "right") else (ngrp, nb, nx), np.float32) for s in SIDES}
    out = empty_arrays(dev, cube, specs)
    ctx.call("rip_stage_l2_refpix_strips", cube, _native.dtype_code(cube), ngrp, ny, nx, nb,
             _native.location_of(cube), *(out[k] if out[k].size else None for k in specs))
    if dev:
        ctx.synchronize()
    return out


def add_in_provenance(rstruct):
    """``meta.calibration_software_name`` (the reference's) and ``_version`` (this package's) of an L2 ``roman`` branch
    (oututils.py:106-110)"""
    rstruct["meta"]["calibration_software_name"] = SOFTWARE_NAME
    rstruct["meta"]["calibration_software_version"] = "romanimpreprocess_amd " + __version__


def add_dummy_fields(rstruct):
    """``chisq`` and ``dumo`` as float16 zeros of the shape of ``data`` where absent, each listed in ``meta.dummyfields``
    (typefix.py:22-31)"""
    for fld in DUMMY_FIELDS:
        if fld not in rstruct:
            rstruct[fld] = np.zeros(np.shape(rstruct["data"]), dtype=np.float16)
            rstruct["meta"].setdefault("dummyfields", []).append(f"roman.{fld}")
