"""Array-level driver of the L1->L2 chain on one GPU.

``Calibrator`` owns a context, the device-resident CALDIR sets (one slot per SCA) and the ramp-fit
plans; ``calibrate`` runs the chain of ``calibrateimage`` (``gen_cal_image.py:531-629``) on numpy
arrays (host) or on device pointers (e.g. torch tensors' ``data_ptr()``), through ``rip_calibrate``.
"""


import numpy as np

from . import _native, pars, plan as planmod
from ._native import (STAGE_ALL, STAGE_BIAS, STAGE_DARK, STAGE_FLAT, STAGE_IPC, STAGE_LIN, STAGE_RAMPFIT,  # noqa: F401
                      STAGE_REFPIX)


def read_pattern_dilution(read_pattern):
    """mean(read indices) / last read index per group (f64; 0/0 = NaN for a group holding only read 0: never flags): the
    factor stcal applies to the saturation threshold of groups that average several reads (rip_ramp_desc::sat_dilution)."""
    with np.errstate(all="ignore"):
        return np.ascontiguousarray([np.float64(np.mean(r)) / np.float64(r[-1]) for r in read_pattern], dtype=np.float64)


class _Block:
    """Memory of a result array that goes back to its pool when the last array (or view of one) that refers to it is gone."""

    def __init__(self, pool, mem):
        self._pool, self._mem = pool, mem
        self.__array_interface__ = {"shape": mem.shape, "typestr": "|u1", "data": (mem.ctypes.data, False), "version": 3}

    def __del__(self):
        try:
            self._pool._give_back(self._mem)
        except Exception:   # interpreter shutdown
            pass


class ResultPool:
    """Result arrays made of memory that has been touched before.  A fresh ``np.empty`` of the four result planes and the group
    flags of a 4096 x 4096 x 8 ramp (0.4 GB) costs 100 000 page faults when the copy from the device first writes it: 33 ms on top
    of the 16 ms the calibration takes (bench.py, ``host_path``).  Arrays from this pool are ordinary numpy arrays that own their
    memory through a base object; when the caller drops the last reference the memory returns here and serves the next call.  At
    most ``keep`` spare blocks per size are held."""

    def __init__(self, keep=12):
        self.keep, self.free = keep, {}

    def _give_back(self, mem):
        spare = self.free.setdefault(mem.nbytes, [])
        if len(spare) < self.keep:
            spare.append(mem)

    def empty(self, shape, dtype):
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dtype.itemsize
        if nbytes < (1 << 20):
            return np.empty(shape, dtype)
        spare = self.free.get(nbytes)
        mem = spare.pop() if spare else np.empty(nbytes, np.uint8)
        return np.asarray(_Block(self, mem)).view(dtype).reshape(shape)


class Calibrator:
    def __init__(self, device=None, ctx=None):
        self.ctx = ctx if ctx is not None else _native.default_context(device)
        # CALDIR slots, plans and the pool of result arrays belong to the context: every Calibrator on it sees them
        self.shapes = self.ctx.shapes
        if self.ctx.result_pool is None:
            self.ctx.result_pool = ResultPool()

    # ---- CALDIR ---------------------------------------------------------------------------
    def load_caldir(self, slot, cal, nborder=pars.nborder, owner=None):
        """Upload one SCA's calibration arrays (dict of dicts, ``roman`` branch layout) into ``slot``.  ``owner``: tag kept
        with the slot (``slot_owner``) so that a cache of file-based CALDIR sets can tell when its slot was reused."""
        rslope = planmod.refout_slope(cal["read"])
        self.shapes[slot] = self.ctx.upload_caldir(slot, cal, nborder=nborder, refout_slope=rslope)
        self.ctx.caldir_owner[slot] = owner
        return self.shapes[slot]

    def drop_caldir(self, slot):
        """Free ``slot`` on the device and forget its frame shape and owner: a later call on it raises KeyError."""
        self.ctx.drop_caldir(slot)
        self.shapes.pop(slot, None)
        self.ctx.caldir_owner.pop(slot, None)

    def bias_state(self, slot):
        """``_native.BIAS_ABSENT`` / ``BIAS_PRESENT`` / ``BIAS_DROPPED`` for the CALDIR set of ``slot`` (``rip_caldir_bias_state``): a
        set without biascorr, or with one that is +0 everywhere (dropped at upload), runs the fused kernel without that stream."""
        return self.ctx.caldir_bias_state(slot)

    def slot_owner(self, slot):
        return self.ctx.caldir_owner.get(slot)

    def chain_form_for(self, slot, ngroups):
        """2 where a ramp of ``ngroups`` groups on the CALDIR set of ``slot`` has a fused-kernel form (Legendre order, ipc4d and
        gain dtypes of the set as uploaded), 0 where it takes the stage kernels.  The limits of ``_native.chain_form_for``
        apply: the plan's difference mask and the set's flag words are not looked at."""
        if int(slot) not in self.ctx.caldir_dtypes:
            raise ValueError(f"chain_form_for: no CALDIR set is loaded in slot {slot}")
        nplanes, ipc_dtype, gain_dtype = self.ctx.caldir_dtypes[int(slot)]
        return _native.chain_form_for(nplanes, ngroups, ipc_dtype, gain_dtype)

    def chain_geometry_for(self, slot, ngroups, ncu, reserve=None, quad_ok=True):
        """Launch geometry of the fused kernel (``_native.chain_geometry_for``) for a ramp of ``ngroups`` groups on the CALDIR set
        of ``slot`` -- its frame shape and dtypes -- on a device of ``ncu`` compute units; None where the stage kernels run.
        ``reserve`` None: the default of the option "chain_reserve".  ``Context.last_chain_geometry`` tells what a call really used."""
        if int(slot) not in self.ctx.caldir_dtypes:
            raise ValueError(f"chain_geometry_for: no CALDIR set is loaded in slot {slot}")
        nplanes, ipc_dtype, gain_dtype = self.ctx.caldir_dtypes[int(slot)]
        ny, nx = self.shapes[slot]
        return _native.chain_geometry_for(nplanes, ngroups, ipc_dtype, ny, nx, ncu, reserve, quad_ok, gain_dtype)

    # ---- plans ----------------------------------------------------------------------------
    def plan_for(self, read_pattern, frame_time, exclude_first=True, ramp_opt_pars=None, jump_pars=None):
        """(plan id, meta) for an MA table; cached per configuration."""
        key = (repr(read_pattern), float(frame_time), bool(exclude_first), repr(ramp_opt_pars), repr(jump_pars))
        if key in self.ctx.plans:
            return self.ctx.plans[key]
        meta = planmod.exposure_meta(read_pattern, frame_time)
        meta["nborder"] = pars.nborder
        meta["K"] = planmod.construct_weights(planmod.ramp_opt_u(ramp_opt_pars), meta, exclude_first)
        if jump_pars:
            meta["jump_detect_pars"] = jump_pars
        desc = planmod.plan_desc(meta, meta["K"], exclude_first, list(read_pattern[0]) == [0], jump_pars)
        pid = self.ctx.create_plan(desc)
        self.ctx.plans[key] = (pid, meta)
        return pid, meta

    # ---- host arrays in, host arrays out --------------------------------------------------
    def calibrate(self, slot, ramp, exclude_first=True, ramp_opt_pars=None, jump_pars=None, area_factor=None,
                  stages=STAGE_ALL, want_groupdq=True, want_cube=False, channel_lines=None, flag_saturation=False,
                  saturation_backup=1, saturation_skip_firstn=1, out=None, saturation_read_pattern=False):
        """Run the chain on one ramp given as numpy arrays.

        ``ramp``: dict(data u16|f32 (G,ny,nx), amp33 u16 (G,ny,128)|None, groupdq u8, pixeldq u32,
        read_pattern, frame_time).  Returns dict(slope, err_read, err_poisson, pixeldq[, groupdq][, cube], K, meta).

        An exposure stored with its reference read subtracted (``sim_to_isim.extract_ref``) also carries ``reference_read`` u16
        (ny,nx), ``data_encoding_offset`` and -- where amp33 is encoded too -- ``reference_amp33`` u16 (ny,128): data, amp33 and
        read_pattern are then the stored ones (one group fewer than the exposure had), and the library decodes its device copies
        before the chain.  ValueError when the pieces do not belong together (a decoded sample outside 0..65535).

        ``flag_saturation``: dq-init + saturation flagging on the device before the chain (the CALDIR slot must hold
        ``saturation``); ``ramp["groupdq"]`` may then be None and ``ramp["pixeldq"]`` is the mask dq.
        ``saturation_read_pattern``: compare groups of several reads with threshold * mean(reads) / last read (the read-pattern
        rule of stcal the reference's call enables, gen_cal_image.py:172-185).

        ``out``: optional dict of preallocated C-contiguous result arrays (any of slope, err_read, err_poisson f32 (ny,nx),
        pixeldq u32 (ny,nx), groupdq u8 (G,ny,nx), cube f32 (G,ny,nx)) that are filled instead of new ones.  With page-locked
        arrays (``Calibrator.pinned_empty``) on both sides the copies run at PCIe rate (tools/gpu_checks/host_path_timing.py).
        """
        ny, nx = self.shapes[slot]
        pid, meta = self.plan_for(ramp["read_pattern"], ramp["frame_time"], exclude_first, ramp_opt_pars, jump_pars)
        dil = read_pattern_dilution(ramp["read_pattern"]) if (flag_saturation and saturation_read_pattern) else None
        rd, od = _native.RampDesc(), _native.Outputs()
        res, keep = self._host_ramp(rd, od, ramp, (ny, nx), exclude_first, flag_saturation, saturation_backup,
                                    saturation_skip_firstn, dil, out, want_groupdq, want_cube, area_factor, channel_lines)
        self.ctx.calibrate_raw(slot, pid, stages, rd, od)
        del keep
        if not (stages & STAGE_RAMPFIT):
            for k in ("slope", "err_read", "err_poisson"):
                res.pop(k)
            res.pop("groupdq", None)
        res["K"], res["meta"] = meta["K"], meta
        return res

    def _host_ramp(self, rd, od, ramp, frame, exclude_first, flag_saturation, saturation_backup, saturation_skip_firstn, dil,
                   given, want_groupdq, want_cube=False, area_factor=None, channel_lines=None, i=None):
        """Fills ``rd`` / ``od`` (``RampDesc`` / ``Outputs``) for one ramp of numpy arrays (see ``calibrate``) and returns (the
        result dict, the input arrays the call reads: they must outlive it).  ``dil``: the saturation step's dilution factors or
        None; ``given``: a dict of preallocated result arrays or None; ``i``: the ramp's index in a batch, for error texts."""
        ny, nx = frame
        data = np.ascontiguousarray(ramp["data"])
        if data.dtype not in (np.uint16, np.float32):
            data = data.astype(np.float32)
        G = data.shape[0]
        if data.shape != (G, ny, nx):
            raise ValueError(f"{'ramp' if i is None else f'ramp {i}:'} shape {data.shape} does not match the CALDIR frame {frame}")
        gdq = None
        if ramp.get("groupdq") is not None:
            gdq = np.ascontiguousarray(ramp["groupdq"], dtype=np.uint8)   # (DO_NOT_USE on an excluded first group: set on the
            #                                                              library's device copy, rd.or_first_group below)
        elif not flag_saturation:
            what = "ramp['groupdq']" if i is None else f"ramp {i}: groupdq"
            raise ValueError(f"{what} is required unless flag_saturation is set")
        pdq = np.ascontiguousarray(ramp["pixeldq"], dtype=np.uint32)
        amp33 = None if ramp.get("amp33") is None else np.ascontiguousarray(ramp["amp33"], dtype=np.uint16)
        area = None if area_factor is None else np.ascontiguousarray(area_factor, dtype=np.float64)
        lines = None if channel_lines is None else np.ascontiguousarray(channel_lines, dtype=np.float64)
        who = "ramp" if i is None else f"ramp {i}:"
        ref = ref33 = None
        if ramp.get("reference_read") is not None:   # stored with the reference read subtracted (rip_ramp_desc::reference_read)
            if ramp.get("data_encoding_offset") is None:
                raise ValueError(f"{who} reference_read without data_encoding_offset")
            ref = self._reference_plane(ramp["reference_read"], (ny, nx), f"{who} reference_read")
            if data.dtype != np.uint16:
                raise ValueError(f"{who} reference_read needs uint16 data, not {data.dtype}")
        if ramp.get("reference_amp33") is not None:
            if ramp.get("data_encoding_offset") is None:
                raise ValueError(f"{who} reference_amp33 without data_encoding_offset")
            if amp33 is None:
                raise ValueError(f"{who} reference_amp33 without amp33")
            ref33 = self._reference_plane(ramp["reference_amp33"], (ny, amp33.shape[-1]), f"{who} reference_amp33")

        rd.location, rd.ngrp = _native.RIP_HOST, G
        rd.data, rd.data_dtype = data.ctypes.data, _native.dtype_code(data)
        rd.amp33 = None if amp33 is None else amp33.ctypes.data
        rd.groupdq, rd.pixeldq = (None if gdq is None else gdq.ctypes.data), pdq.ctypes.data
        rd.flag_saturation = 1 if flag_saturation else 0
        rd.or_first_group = 1 if (exclude_first and gdq is not None) else 0   # gen_cal_image.py:142-143, the caller's array untouched
        rd.sat_backup, rd.sat_skip_firstn = int(saturation_backup), int(saturation_skip_firstn)
        rd.sat_dilution = None if dil is None else dil.ctypes.data
        rd.area_factor = None if area is None else area.ctypes.data
        rd.channel_lines = None if lines is None else lines.ctypes.data
        rd.reference_read = None if ref is None else ref.ctypes.data
        rd.reference_amp33 = None if ref33 is None else ref33.ctypes.data
        rd.data_encoding_offset = 0 if (ref is None and ref33 is None) else int(ramp["data_encoding_offset"])

        def result(name, shape, dtype):
            a = None if given is None else given.get(name)
            if a is None:
                return self.ctx.result_pool.empty(shape, dtype)
            if a.shape != shape or a.dtype != dtype or not a.flags.c_contiguous:
                where = "out" if i is None else f"out[{i}]"
                raise ValueError(f"{where}[{name!r}] must be a C-contiguous {np.dtype(dtype).name} array of shape {shape}")
            return a

        res = {"slope": result("slope", frame, np.float32), "err_read": result("err_read", frame, np.float32),
               "err_poisson": result("err_poisson", frame, np.float32), "pixeldq": result("pixeldq", frame, np.uint32)}
        od.location = _native.RIP_HOST
        od.slope, od.err_read = res["slope"].ctypes.data, res["err_read"].ctypes.data
        od.err_poisson, od.pixeldq = res["err_poisson"].ctypes.data, res["pixeldq"].ctypes.data
        if want_groupdq:
            res["groupdq"] = result("groupdq", (G, ny, nx), np.uint8)
            od.groupdq = res["groupdq"].ctypes.data
        if want_cube:
            res["cube"] = result("cube", (G, ny, nx), np.float32)
            od.cube = res["cube"].ctypes.data
        return res, (data, gdq, pdq, amp33, area, lines, ref, ref33)

    @staticmethod
    def _reference_plane(a, shape, what):
        """the reference plane of an encoded ramp as the library takes it: C-contiguous uint16 of ``shape`` (no silent cast: a
        plane of another dtype is not what the encoder wrote)"""
        a = np.asarray(a)
        if a.dtype != np.uint16 or a.shape != tuple(shape):
            raise ValueError(f"{what} must be a uint16 array of shape {tuple(shape)}, not {a.dtype} {a.shape}")
        return np.ascontiguousarray(a)

    # ---- a batch of ramps in host memory, pipelined over PCIe --------------------------------
    def calibrate_many(self, slot, ramps, exclude_first=True, ramp_opt_pars=None, jump_pars=None, want_groupdq=False,
                       flag_saturation=False, saturation_backup=1, saturation_skip_firstn=1, out=None, saturation_read_pattern=False):
        """Run the whole chain on a list of ramps (dicts as for ``calibrate``; same read pattern, frame time and data
        dtype) with ``rip_calibrate_batch``: upload, chain and download of consecutive ramps overlap.  ``out``: optional
        list of dicts of preallocated result arrays (see ``calibrate``).  Returns the list of result dicts.  Page-locked
        arrays (``pinned_empty``) on both sides give the full PCIe rate.  ``saturation_read_pattern``: as in ``calibrate``
        (the read-pattern rule of the saturation step; ``calibrateimage`` and the harness switch it on)."""
        ramps = list(ramps)
        if not ramps:
            return []
        ny, nx = self.shapes[slot]
        pid, meta = self.plan_for(ramps[0]["read_pattern"], ramps[0]["frame_time"], exclude_first, ramp_opt_pars, jump_pars)
        n = len(ramps)
        # the read-pattern rule of the saturation step, as calibrateimage applies it (gen_cal_image.py:172-185)
        dil = read_pattern_dilution(ramps[0]["read_pattern"]) if (flag_saturation and saturation_read_pattern) else None
        descs, outs, results, keep = (_native.RampDesc * n)(), (_native.Outputs * n)(), [], []
        for i, ramp in enumerate(ramps):
            if list(map(list, ramp["read_pattern"])) != list(map(list, ramps[0]["read_pattern"])):
                raise ValueError(f"ramp {i}: read pattern differs from ramp 0")
            res, arrays = self._host_ramp(descs[i], outs[i], ramp, (ny, nx), exclude_first, flag_saturation, saturation_backup,
                                          saturation_skip_firstn, dil, None if out is None else out[i], want_groupdq, i=i)
            keep.append(arrays)
            res["K"], res["meta"] = meta["K"], meta
            results.append(res)
        self.ctx.call("rip_calibrate_batch", slot, pid, STAGE_ALL, n, descs, outs)
        del keep
        return results

    # ---- device pointers in, device pointers out (asynchronous) ---------------------------
    def calibrate_device(self, slot, plan_id, ngrp, data_ptr, data_is_u16, amp33_ptr, groupdq_ptr, pixeldq_ptr,
                         slope_ptr, err_read_ptr, err_poisson_ptr, pixeldq_out_ptr, groupdq_out_ptr=None,
                         area_ptr=None, stages=STAGE_ALL, flag_saturation=False, saturation_backup=1,
                         saturation_skip_firstn=1, read_pattern=None, inputs_complete=False, ready_event=None):
        """``groupdq_ptr`` may be None with ``flag_saturation`` (dq-init + saturation flagging on the device).
        ``read_pattern``: with ``flag_saturation``, the exposure's read pattern for the read-pattern rule of the saturation
        step (groups averaging several reads are compared with a diluted threshold, as ``calibrateimage`` does: the reference
        hands the pattern to stcal at gen_cal_image.py:172-185); None = every group against the full threshold.
        Ordering of the inputs (``rip_ramp_desc::inputs_ready`` / ``ready_event``): by default the call is ordered behind
        everything queued on the context's stream; ``inputs_complete=True`` = the caller vouches that the device arrays are
        complete now (keeps the overlap of the reference-pixel pre-pass with the previous call's kernel); ``ready_event`` =
        a raw ``hipEvent_t`` (e.g. ``torch.cuda.Event.cuda_event``) recorded behind the work that writes them."""
        rd = _native.RampDesc()
        rd.location, rd.ngrp = _native.RIP_DEVICE, int(ngrp)
        rd.data, rd.data_dtype = data_ptr, (_native.RIP_U16 if data_is_u16 else _native.RIP_F32)
        rd.amp33, rd.groupdq, rd.pixeldq, rd.area_factor = amp33_ptr, groupdq_ptr, pixeldq_ptr, area_ptr
        rd.flag_saturation = 1 if flag_saturation else 0
        rd.sat_backup, rd.sat_skip_firstn = int(saturation_backup), int(saturation_skip_firstn)
        dil = read_pattern_dilution(read_pattern) if (flag_saturation and read_pattern is not None) else None
        if dil is not None:
            rd.sat_dilution = dil.ctypes.data   # host pointer, read during the call
        rd.inputs_ready = _native.RIP_INPUTS_COMPLETE if inputs_complete else _native.RIP_INPUTS_STREAM_ORDERED
        rd.ready_event = ready_event
        out = _native.Outputs()
        out.location = _native.RIP_DEVICE
        out.slope, out.err_read, out.err_poisson = slope_ptr, err_read_ptr, err_poisson_ptr
        out.pixeldq, out.groupdq = pixeldq_out_ptr, groupdq_out_ptr
        self.ctx.calibrate_raw(slot, plan_id, stages, rd, out)

    def decode_reference_read(self, data_ptr, ngrp, n, ref_ptr, offset, out_ptr=None, want_count=False):
        """``rip_stage_decode_reference_read`` on device memory: (ngrp, n) u16 samples at ``data_ptr`` stored with the reference
        read at ``ref_ptr`` (n u16) subtracted become ``clip(i32(data) + i32(reference) - offset, 0, 65535)`` at ``out_ptr`` (None:
        in place).  For the cube n = ny * nx, for amp33 n = ny * 128 with reference_amp33.  Asynchronous on the context's stream,
        where ``calibrate_device`` finds the result.  ``want_count=True`` waits and returns the number of samples the clip
        changed (non-zero: the pieces do not belong together); otherwise None and no synchronisation."""
        import torch

        count = torch.zeros(1, dtype=torch.int64, device=torch.device("cuda", self.ctx.device))
        torch.cuda.current_stream(count.device).synchronize()   # torch's fill runs on torch's stream, the entry on the context's
        self.ctx.call("rip_stage_decode_reference_read", data_ptr, ngrp, n, ref_ptr, offset, _native.RIP_DEVICE,
                      data_ptr if out_ptr is None else out_ptr, count)
        if not want_count:
            self.ctx.refread_count = count   # the kernel adds to it: alive until the next call replaces it
            return None
        self.ctx.synchronize()
        return int(count.item())

    # ---- pixel-area map ------------------------------------------------------------------
    def area_factor(self, wcs, ny, nx, device=False):
        """AreaFactor = pixel solid angle / Omega_ideal (gen_cal_image.py:618-621) of an (ny, nx) frame from a ``FitsWCS``, made on
        the device (``rip_stage_pixel_area``): a read-only numpy array, or with ``device=True`` a torch tensor in HBM (what
        ``calibrate_device`` takes as ``area_ptr``).  Cached on the context by WCS digest, shape and place; at most two maps are
        kept (a host map of a 4096 x 4096 frame is 134 MB)."""
        from .utils import coordutils

        key = (wcs.digest(), int(ny), int(nx), bool(device))
        cache = self.ctx.area_cache
        if key in cache:
            cache[key] = cache.pop(key)   # most recently used last
            return cache[key]
        area = coordutils.pixelarea_map(wcs, ny, nx, scale=pars.Omega_ideal, device=device, ctx=self.ctx)
        if not device:
            area.flags.writeable = False
        while len(cache) >= 2:
            cache.pop(next(iter(cache)))
        cache[key] = area
        return area

    def pinned_empty(self, shape, dtype):
        """A page-locked numpy array: host buffers the library copies from / to at PCIe rate."""
        return self.ctx.pinned_empty(shape, dtype)

    def synchronize(self):
        self.ctx.synchronize()


def lapack_channel_lines(bottom_top, nrows):
    """(m, c) of the line through (1.5, bottom), (nrows-2.5, top) from LAPACK's least squares, exactly as
    ``reference_subtraction.py:57-60`` obtains it; ``bottom_top`` (..., 2) f32 -> (..., 2) f64."""
    bt = np.asarray(bottom_top)
    A = np.vstack([(1.5, nrows - 2.5), np.ones(2)]).T
    out = np.zeros(bt.shape, dtype=np.float64)
    flat_in, flat_out = bt.reshape(-1, 2), out.reshape(-1, 2)
    for i in range(flat_in.shape[0]):
        flat_out[i] = np.linalg.lstsq(A, (flat_in[i, 0], flat_in[i, 1]), rcond=None)[0]
    return out
