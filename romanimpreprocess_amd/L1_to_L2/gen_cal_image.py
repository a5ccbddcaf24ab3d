"""L1 -> L2 driver on the GPU: same entry point and configuration surface as the reference's
``L1_to_L2/gen_cal_image.py`` (``calibrateimage(config, verbose=True)`` :480, CLI ``python -m
romanimpreprocess_amd.L1_to_L2.gen_cal_image config.yaml`` :742-746).

What runs where
  * the per-pixel chain of ``calibrateimage`` lines 531-629 (reference pixels, bias, linearity, IPC, ramp fit
    with jump detection, dark rate, error split, flat) -> one ``rip_calibrate`` call (HIP kernels);
  * the host keeps what the reference does on the host in microseconds: metadata (:123-145), ramp weights
    (:434-444), the process log, file I/O (ASDF through ``asdf`` when installed, else the in-repo reader/writer,
    or ``.npz`` mirrors -- see ``calio``);
  * steps whose source is NOT in the reference tree are restated from their call sites and documented
    behaviour (parity unpinned): dq-init (:118, mask -> pixeldq, zero groupdq), saturation flagging
    (:148-185, on the device: ``rip_ramp_desc::flag_saturation``; its numpy restatement is ``oracle/saturation.py``), and
    the L2 tree layout of ``romanisim.image.make_asdf`` (:653-662);
  * the post-path reductions (:632-651, 697-712: median gain, sky mode, SKYORDER model, SLICEOUT) -> ``utils/sky.py``,
    ``utils/maskhandling.py`` (HIP kernels);
  * the pixel-area map of the flat division (:616-622): from the exposure's WCS, ``config["FITSWCS"]`` (a FITS header as text,
    :64-87, read by ``wcs_from_config``), through ``utils/coordutils.py`` and one HIP kernel (``rip_stage_pixel_area``) over the
    full frame, border included, as the reference's ``N=np.shape(slope)[-1]``.  The repository's own ``AREAFACTOR`` key (a
    file with an (N,N) f64 array) takes precedence when both are given; with neither, AreaFactor = 1;
  * not done here (outside the hot path): the gwcs object of the L2 tree (:660), dark decay, WFI18 transient,
    romancal likelihood ramp fit.  Asking for one of those raises NotImplementedError;
  * between the chain and the file the exposure stays in HBM: one upload (``_exposure_to_device``), ``calibrate_device``, the grown mask,
    the sky mode, the sky model and the end slices on ``DevArray``s, and every plane of the L2 tree -- the crop, the two variances,
    ``err``, float32 or float16 (``L2_FLOAT16``), the flag strips and the reference-pixel strips the reference adds with
    ``oututils.add_in_ref_data`` (:674) -- from one HIP stage (``oututils.py``, ``csrc/l2out.hip``); each plane is downloaded once, the
    group flags never; provenance (:679) and the placeholder planes of ``typefix.fix`` (:721) are set on the host;
  * ``FITSOUT`` (:725-736): the three-HDU ``_asdf_to.fits`` beside the L2 file, through ``calio.write_fits`` -- the data units are
    put into FITS byte order, and the masked image is made, on the device (``rip_stage_fits_encode``).
"""

import sys

import numpy as np

from .. import calio, pars, pipeline, plan as planmod
from ..devarray import DevArray, to_device
from ..dqflags import group
from ..utils import coordutils, flatutils, maskhandling, processlog, sky
from . import oututils

_cal_cache = {}  # (ctx id, tuple of CALDIR paths) -> slot


def wcs_from_config(config):
    """The exposure's WCS from the configuration (gen_cal_image.py:64-87): ``config["FITSWCS"]`` is the path of a FITS header
    written as text (``sim_to_isim.py:986-987``), returned as a validated ``coordutils.FitsWCS``; None without the key."""
    if "FITSWCS" in config:
        return coordutils.FitsWCS.from_file(config["FITSWCS"])
    return None


def initializationstep(config, caldir, mylog):
    """Read the L1 file and the mask: data (u16 cube), amp33, groupdq (zeros), pixeldq (mask dq), meta.

    An exposure stored with its reference read subtracted (the EXTRACT_REF block of ``sim_to_isim.py:711-730``; the reference
    leaves the decoding to romancal's dq-init, :117-118) also yields ``reference_read``, ``reference_amp33`` (None where amp33
    is not encoded) and ``data_encoding_offset``: data, amp33 and the read pattern stay as stored, one group fewer than the
    exposure had, and the chain call decodes on the device.  ValueError when such a tree does not say its offset."""
    with calio.open_tree(config["IN"]) as f:
        r = f["roman"]
        data = np.ascontiguousarray(r["data"])
        amp33 = np.ascontiguousarray(r["amp33"]) if "amp33" in r else None
        encoded = {}
        if "reference_read" in r:
            instrument = r["meta"]["instrument"] if "instrument" in r["meta"] else {}
            if "data_encoding_offset" not in instrument:
                raise ValueError("the L1 tree has reference_read but no meta.instrument.data_encoding_offset")
            encoded = {"reference_read": np.ascontiguousarray(r["reference_read"]),
                       "reference_amp33": np.ascontiguousarray(r["reference_amp33"]) if "reference_amp33" in r else None,
                       "data_encoding_offset": int(instrument["data_encoding_offset"])}
        exposure = r["meta"]["exposure"]
        frame_time = float(exposure["frame_time"])
        read_pattern = [list(map(int, g)) for g in exposure["read_pattern"]]
        l1meta = calio._materialise(r["meta"])
    if data.dtype != np.uint16:
        data = data.astype(np.float32)
    if "mask" in caldir:
        with calio.open_tree(caldir["mask"]) as f:
            pixeldq = np.array(f["roman"]["dq"], dtype=np.uint32)
    else:
        pixeldq = np.zeros(data.shape[1:], dtype=np.uint32)
    groupdq = np.zeros(data.shape, dtype=np.uint8)
    meta = planmod.exposure_meta(read_pattern, frame_time)
    if config.get("EXCLUDE_FIRST", True):
        groupdq[0] |= np.uint8(group.DO_NOT_USE)
    return dict({"data": data, "amp33": amp33, "groupdq": groupdq, "pixeldq": pixeldq, "meta": l1meta}, **encoded), meta


def load_caldir_arrays(caldir):
    """``roman`` branches of the CALDIR files the per-pixel chain needs (KeyError on a missing required key)."""
    cal = {}
    for key in ("dark", "read", "gain", "linearitylegendre", "flat"):
        cal[key] = calio.roman_branch(caldir[key])
    for key in ("ipc4d", "biascorr", "saturation"):   # optional (no ipc4d: "skipping IPC correction", ipc_linearity.py:170-176)
        if key in caldir:
            cal[key] = calio.roman_branch(caldir[key])
    return cal


def _file_stamp(path):
    """(mtime, size) of a calibration file: a file rewritten in place must not be served stale from HBM"""
    import os

    try:
        st = os.stat(path)
        return (st.st_mtime_ns, st.st_size)
    except OSError:
        return None


_medgain_cache = {}  # (gain file, its (mtime, size)) -> median gain: an unchanged file is read once


def _median_gain(path, ctx):
    """``np.median`` of the gain file's plane (gen_cal_image.py:632-637), found on the device for a float32 plane; kept per file
    and stamp, so that a series of exposures on one CALDIR set reads the 67 MB plane once."""
    key = (path, _file_stamp(path) if isinstance(path, str) else None)
    if key[1] is not None and key in _medgain_cache:
        return _medgain_cache[key]
    with calio.open_tree(path) as g_:
        gain_plane = np.asarray(g_["roman"]["data"])
    if gain_plane.dtype == np.float32 and gain_plane.ndim == 2:
        medgain = float(sky.block_nanmedians(gain_plane, 1, ctx=ctx)[0, 0])  # = np.median for a NaN-free f32 plane
    else:
        medgain = float(np.median(gain_plane))
    if key[1] is not None:
        if len(_medgain_cache) >= 64:
            _medgain_cache.clear()
        _medgain_cache[key] = medgain
    return medgain


def _caldir_slot(cb, caldir):
    """The CALDIR slot holding this set of files on the calibrator's context, uploading it first if need be.  The cache key
    holds the paths AND each file's (mtime, size); a slot is taken from the top (31 downwards) only if nobody owns it or its
    owner is one of this cache's own, older entries -- a slot a caller loaded explicitly (``Calibrator.load_caldir``) is never
    replaced silently."""
    files = tuple(sorted((k, str(v), _file_stamp(str(v))) for k, v in caldir.items() if isinstance(v, str)))
    key = (id(cb.ctx), files)
    slot = _cal_cache.get(key)
    if slot is not None and cb.slot_owner(slot) == key:   # still ours
        return slot
    for cand in range(31, 7, -1):   # from the top: low slot numbers are left to explicit load_caldir calls
        if cand not in cb.shapes:    # never loaded on this context
            slot = cand
            break
    else:
        # every slot is taken: evict the oldest entry of this cache (never an explicitly loaded slot)
        slot = None
        for k_old, s_old in list(_cal_cache.items()):
            if k_old[0] == id(cb.ctx) and cb.slot_owner(s_old) == k_old:
                slot = s_old
                del _cal_cache[k_old]
                break
        if slot is None:
            raise RuntimeError("no free CALDIR slot: slots 8..31 are all held by explicit load_caldir calls")
    cb.load_caldir(slot, load_caldir_arrays(caldir), owner=key)
    _cal_cache[key] = slot
    return slot


def _download(cb, a):
    """The one copy of a complete ``DevArray`` to the host, as the numpy array that goes into the tree: into memory of the
    context's result pool, which has been touched before (``pipeline.ResultPool``)."""
    import torch

    host = cb.ctx.result_pool.empty(a.shape, a.dtype)
    if a.size:
        torch.from_numpy(host.view(np.int32) if a.dtype == np.uint32 else host).copy_(a.t)
    return host


def _exposure_to_device(cb, slot, ramp, nb):
    """One upload of the exposure: (cube, amp33 or None, mask dq) as ``DevArray``s the chain takes, and the reference-pixel strips
    ``border_ref_pix_*`` of the cube (``oututils.refpix_strips``, in HBM).  For an exposure stored with its reference read
    subtracted the strips are the samples AS STORED -- the reference copies them from the file (oututils.py:46-49) -- and the
    device copies of cube and amp33 are decoded afterwards (``rip_stage_decode_reference_read``); ValueError where the pieces do
    not belong together, with the checks ``Calibrator.calibrate`` makes of a host ramp."""
    data = ramp["data"]
    frame = cb.shapes[slot]
    if tuple(data.shape[1:]) != tuple(frame):
        raise ValueError(f"ramp shape {data.shape} does not match the CALDIR frame {frame}")
    G, ny, nx = data.shape
    amp33 = None if ramp["amp33"] is None else np.ascontiguousarray(ramp["amp33"], dtype=np.uint16)
    ref = ref33 = None
    if ramp.get("reference_read") is not None:
        ref = cb._reference_plane(ramp["reference_read"], (ny, nx), "ramp reference_read")
        if data.dtype != np.uint16:
            raise ValueError(f"ramp reference_read needs uint16 data, not {data.dtype}")
    if ramp.get("reference_amp33") is not None:
        if amp33 is None:
            raise ValueError("ramp reference_amp33 without amp33")
        ref33 = cb._reference_plane(ramp["reference_amp33"], (ny, amp33.shape[-1]), "ramp reference_amp33")
    dev = cb.ctx.device
    cube = to_device(data, dev)
    a33 = None if amp33 is None else to_device(amp33, dev)
    mask_dq = to_device(np.ascontiguousarray(ramp["pixeldq"], dtype=np.uint32), dev)
    strips = oututils.refpix_strips(cube, nb, ctx=cb.ctx)
    bad = 0
    if ref is not None:
        ref_dev = to_device(ref, dev)   # (named: it has to outlive the call, which allocates its counting word)
        bad += cb.decode_reference_read(cube.ctypes.data, G, ny * nx, ref_dev.ctypes.data, ramp["data_encoding_offset"], want_count=True)
    if ref33 is not None:
        ref33_dev = to_device(ref33, dev)
        bad += cb.decode_reference_read(a33.ctypes.data, G, ny * amp33.shape[-1], ref33_dev.ctypes.data, ramp["data_encoding_offset"],
                                        want_count=True)
    if bad:
        raise ValueError(f"calibrateimage: {bad} samples of the decoded ramp lie outside 0..65535: reference_read, data and "
                         "data_encoding_offset do not belong together")
    return cube, a33, mask_dq, strips


def calibrateimage(config, verbose=True, calibrator=None):
    """Run the calibrations specified by ``config`` (dict, normally from YAML) and write the L2 file.  Beyond the reference's
    surface: ``config["IN"]`` may be an L1 tree (dict) instead of a path, and with ``config["OUT"] = None`` the L2 tree is
    returned instead of written (the noise-layer driver keeps its intermediate exposures in memory that way).

    The exposure is uploaded once and stays in HBM from the chain to the file: the grown mask, the sky mode, the sky model, the
    end slices and the planes of the tree are made there, the group flags are never downloaded, and each plane comes to the
    host once.  ``config["L2_FLOAT16"]`` (this package's key; the reference decides by validating against the installed schema,
    ``typefix.py:38-56``): true = ``err``, ``var_poisson``, ``var_rnoise`` and ``var_flat`` are float16, the first three rounded
    on the device; absent or false = float32."""
    for unsupported in ("romancal_ramp_fit", "correct_wfi18_transient"):
        if config.get(unsupported):
            raise NotImplementedError(f"{unsupported} is outside the GPU L1->L2 path of this package")
    mylog = processlog.ProcessLog()
    caldir = config["CALDIR"]
    if "dark_decay" in caldir:
        raise NotImplementedError("dark_decay is a romancal step outside the GPU L1->L2 path of this package")
    backup = config.get("SATURATION_BACKUP", 1)

    ramp, meta = initializationstep(config, caldir, mylog)
    meta["nborder"] = pars.nborder
    nb = pars.nborder
    mylog.append("Initialized data\n")
    if ramp.get("reference_read") is not None:
        mylog.append(f"Reference read subtracted in the file (data_encoding_offset = {ramp['data_encoding_offset']}): decoded on the device\n")

    cb = calibrator or pipeline.Calibrator()
    slot = _caldir_slot(cb, caldir)
    # saturation flagging (gen_cal_image.py:148-185): on the device, inside the calibrate call
    if "saturation" not in caldir:
        raise KeyError("saturation")  # the reference opens caldir["saturation"] unconditionally (:174)
    sat_on_device = True
    mylog.append("Saturation check on the device\n")
    exclude_first = config.get("EXCLUDE_FIRST", True)
    area = None
    if "AREAFACTOR" in config:
        with calio.open_tree(config["AREAFACTOR"]) as f:
            area = np.asarray(f["roman"]["data"], dtype=np.float64)
    elif "FITSWCS" in config:
        # the ratio of the true pixel area to the reference area (0.11 arcsec)^2 over the full frame (:618-621)
        area = cb.area_factor(wcs_from_config(config), *ramp["data"].shape[-2:])
        mylog.append("pixel-area map from FITSWCS (GPU)\n")
    ramp["read_pattern"], ramp["frame_time"] = meta["read_pattern"], meta["frame_time"]
    # the exposure goes to HBM once and stays there: the strips of the cube as stored, the decoding of an encoded exposure, the
    # chain (group flags: zeros + DO_NOT_USE on the first group, made on the device), the post-path and the planes of the tree
    float16 = bool(config.get("L2_FLOAT16", False))
    cube, a33, mask_dq, strips = _exposure_to_device(cb, slot, ramp, nb)
    if area is None:
        area_dev = None
    elif "AREAFACTOR" in config:
        area_dev = to_device(area, cb.ctx.device)
    else:
        area_dev = DevArray(cb.area_factor(wcs_from_config(config), *ramp["data"].shape[-2:], device=True)).sync()
    pid, plan_meta = cb.plan_for(ramp["read_pattern"], ramp["frame_time"], exclude_first, config.get("RAMP_OPT_PARS"),
                                 config.get("JUMP_DETECT_PARS"))
    frame = cube.shape[1:]
    chain = {"slope": (frame, np.float32), "err_read": (frame, np.float32), "err_poisson": (frame, np.float32), "pixeldq": (frame, np.uint32)}
    if config.get("SLICEOUT"):   # the only reader of the group flags, and it reads them where they are
        chain["groupdq"] = (cube.shape, np.uint8)
    chain = oututils.empty_arrays(True, cube, chain)
    cb.calibrate_device(slot, pid, cube.shape[0], cube.ctypes.data, cube.dtype == np.uint16, None if a33 is None else a33.ctypes.data,
                        None, mask_dq.ctypes.data, chain["slope"].ctypes.data, chain["err_read"].ctypes.data,
                        chain["err_poisson"].ctypes.data, chain["pixeldq"].ctypes.data,
                        groupdq_out_ptr=chain["groupdq"].ctypes.data if "groupdq" in chain else None,
                        area_ptr=None if area_dev is None else area_dev.ctypes.data, flag_saturation=sat_on_device,
                        saturation_backup=backup, read_pattern=ramp["read_pattern"])
    cb.synchronize()
    del cube, a33, mask_dq, area_dev
    K = plan_meta["K"]
    uopt = config.get("RAMP_OPT_PARS", planmod.DEFAULT_RAMP_OPT_PARS)
    mylog.append(f"\n\nRamp fit optimized for u = {planmod.ramp_opt_u(uopt):11.5E} s**-1\n")
    mylog.append(f"weights = {K}\n")
    mylog.append("Reference pixels, bias, linearity, IPC, ramp fit, dark current, flat: complete (GPU)\n")
    if area is not None:   # the flat the slope was divided by, f32(flat / AreaFactor), as the reference logs it (:622-626)
        flat = (flatutils.get_flat(caldir, meta, None, ipc_deconvolve="ipc4d" in caldir, ctx=cb.ctx) / area).astype(np.float32)
        mylog.append("acquired flat field\n")
        for p in [1, 2, 5, 10, 25, 50, 75, 90, 95, 98, 99]:
            mylog.append(f" {p:2d}%ile = {np.percentile(flat, p):6.4f},")
        mylog.append("\n")
        del flat

    medgain = _median_gain(caldir["gain"], cb.ctx)
    mylog.append(f"median gain = {medgain:8.5f} e/DN\n")

    # sky information (gen_cal_image.py:639-651): grown mask, mode of the 4x4-binned unmasked image, optional low-order
    # sky model subtraction -- all on the GPU (utils/maskhandling.py, utils/sky.py)
    m = maskhandling.PixelMask1.build_device(chain["pixeldq"], ctx=cb.ctx)
    medsky, _ = sky.smooth_mode(sky.binkxk(chain["slope"], 4, mask=m, ctx=cb.ctx), ctx=cb.ctx)
    medsky = float(medsky)
    del m
    # every plane of the tree is made in HBM by one stage (csrc/l2out.hip) and comes to the host once, as the array that is written
    planes = oututils.l2_planes(chain["slope"], chain["err_read"], chain["err_poisson"], chain["pixeldq"], nb, float16=float16, ctx=cb.ctx)
    data_withsky = _download(cb, planes["data"])
    if "SKYORDER" in config:
        skyorder = int(config["SKYORDER"])
        skycoefs, _ = sky.medfit(planes["data"], order=skyorder, subtract=True, ctx=cb.ctx, want_model=False)
        skycoefs = np.asarray(skycoefs)
        data_act = _download(cb, planes["data"])
    else:
        skycoefs = np.array([]).astype(np.float32)
        skyorder = -1  # not used
        data_act = cb.ctx.result_pool.empty(data_withsky.shape, np.float32)
        np.copyto(data_act, data_withsky)

    im2 = {
        "meta": ramp["meta"],
        "data": data_act,
        "dq": _download(cb, planes["dq"]),
        "var_poisson": _download(cb, planes["var_poisson"]),
        "var_rnoise": _download(cb, planes["var_rnoise"]),
        "var_flat": np.zeros(data_act.shape, np.float16 if float16 else np.float32),
        "err": _download(cb, planes["err"]),
        "data_withsky": data_withsky,
    }
    if ramp["amp33"] is not None:
        im2["amp33"] = ramp["amp33"]
    # what the reference adds after make_asdf (oututils.add_in_ref_data :42-55, add_in_provenance :106-110, typefix.fix :22-31)
    for k, v in strips.items():
        im2[k] = _download(cb, v)
    for side in oututils.SIDES:
        im2[f"dq_border_ref_pix_{side}"] = _download(cb, planes[f"dq_border_ref_pix_{side}"])
    oututils.add_in_provenance(im2)
    oututils.add_dummy_fields(im2)
    processinfo = {
        "medsky": medsky, "medgain": medgain, "skyorder": skyorder, "skycoefs": skycoefs,
        "ramp_opt_pars": dict(uopt), "weights": K, "log": mylog.output,
        "config": {k: v for k, v in config.items() if not (k == "IN" and isinstance(v, dict))},
        "exclude_first": bool(exclude_first),
        # the full meta, read_pattern included (a list of lists): the reference's noise driver reads it from the L2 file
        # (gen_noise_image.py:208-212), so files written here can be fed to it
        "meta": {k: ([list(map(int, g)) for g in v] if k == "read_pattern" else v) for k, v in meta.items()},
    }
    if config.get("SLICEOUT"):
        endslice = sky.endslice(chain["groupdq"], nb, ctx=cb.ctx)  # raises ValueError("too many groups") for >= 128 groups
        processinfo["endslice"] = endslice
    if verbose:
        print(mylog.output)
    if config.get("OUT") is None:   # in-memory use (the noise-layer driver): the L2 tree instead of a file
        return {"roman": im2, "processinfo": processinfo}
    calio.write_asdf(config["OUT"], {"roman": im2, "processinfo": processinfo})
    if config.get("FITSOUT"):
        # the image, its flags and the image with -1000 outside the grown mask of the ACTIVE-region flags (gen_cal_image.py:
        # 725-736; saturated pixels are accepted there too): mask and substitution on the device, from the planes still in HBM
        bad = maskhandling.PixelMask1.build_device(planes["dq"], ctx=cb.ctx)
        calio.write_fits(config["OUT"][:-5] + "_asdf_to.fits",
                         [{"data": planes["data"]}, {"data": planes["dq"]},
                          {"data": planes["data"], "mask": bad, "mask_sense": 1, "fill": -1000.0}], ctx=cb.ctx)
    return


if __name__ == "__main__":
    import yaml

    with open(sys.argv[1]) as f:
        calibrateimage(yaml.safe_load(f))
