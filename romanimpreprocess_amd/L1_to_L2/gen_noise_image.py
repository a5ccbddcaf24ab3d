"""Noise layers -- same entry points and configuration surface as the reference's ``L1_to_L2/gen_noise_image.py``
(``make_noise_cube`` :60, ``generate_all_noise`` :334, CLI :392-400); SURVEY.md 8f row 3.

A layer re-runs the whole L1 -> L2 chain on a noise-injected copy of the Level-1 cube and keeps the difference of the
two slope images.  What runs where
  * both chain runs: ``calibrateimage`` of this package (HIP kernels);
  * the injection of white read noise into the cube (``:120-134``): ``inject_read_noise`` (HIP kernel of ``csrc/noise.hip``;
    exact given the normal deviates);
  * clipping (``z``) and sky-mode removal (``S``): ``utils/sky.py`` (HIP kernels);
Random numbers.  The reference draws from ``galsim`` generators, which are not available offline and whose streams cannot be
reproduced; here ``rng`` may be ``None`` / an integer seed (deviates drawn ON THE DEVICE from a counter-based generator:
reproducible, no host random numbers) or a ``numpy.random.Generator`` (deviates drawn on the host in the reference's order
and handed to the kernel).  Layers are therefore statistically, not bit-wise, comparable with the reference's.
  * resampled Poisson layers (``P..r``, ``:262-331``): ``rip_stage_poisson_resample`` (HIP kernel: deviates, their
    accumulation into the resultants and the ramp-fit weights of every pixel's end slice in one pass; exact given the
    deviates).
  * the correlated part of a read-noise layer (``sim_to_isim.fill_in_refdata_and_1f`` :306-402: fresh reference pixels,
    reference output, 1/f noise): ``rip_synth_fill`` on the device (``from_sim.sim_to_isim.L1Synth.fill``: pinned by goldens made by
    executing the reference's function); the 1/f frames -- 34 Fourier transforms of 2^20 points per group -- come from hipFFT
    with device deviates, the white deviates from the device or, with a host generator, from it in the reference's order
    (``NOISE: {CORRELATED: false}`` switches the step off).
The pseudo-Poisson layers (``O``): moment ratios on the host (``GalPoisson/find_tilnus.py``), Pearson-family deviates on the
    device (``GalPoisson/draw_with_tilnus.draw_from_Pearson``, ``csrc/pearson.hip``; parameters pinned by goldens, deviates from
    the device's counter-based generator).
The directives are interpreted by ONE layer loop (``make_noise_cube``); it works on numpy arrays or, by default, on arrays that
stay in HBM across the layers, through two small back ends that differ in where an array lives and how a chain run is invoked.
"""

import re
import sys
from copy import deepcopy

import numpy as np

from .. import _native, calio, pars
from ..devarray import DevArray, is_dev
from ..utils import sky
from .GalPoisson.draw_with_tilnus import draw_from_Pearson
from .GalPoisson.find_tilnus import get_tilde_nus
from .gen_cal_image import calibrateimage


def _get_subscript(arr, ch):
    """The subscript of directive ``ch``: what follows it up to the next capital letter
    (``_get_subscript('RS2Pg4', 'S') -> '2'``, ``('RS2Pg4', 'P') -> 'g4'``; gen_noise_image.py:32-57)."""
    return re.split(r"(?=[A-Z])", arr.split(ch)[-1])[0]


def inject_read_noise(data, read_noise, read_pattern, nb=pars.nborder, normals=None, seed=0, layer=0, ctx=None):
    """White read noise into a u16 cube (gen_noise_image.py:120-134).  ``normals`` (ngrp, ny-2nb, nx-2nb) f32 or None
    (drawn on the device from ``seed``, ``layer``).  Host arrays give a new cube; a ``DevArray`` cube (u16 bits in an int16
    tensor; the read-noise plane may be one too) is updated in place and returned."""
    ctx = ctx or _native.default_context()
    if not is_dev(data):
        data = np.ascontiguousarray(data)
    if data.dtype != np.uint16:
        raise TypeError(f"the Level-1 cube is {data.dtype}, expected uint16")
    G, ny, nx = data.shape
    read = read_noise if is_dev(read_noise) else np.ascontiguousarray(read_noise, dtype=np.float32)
    if read.dtype != np.float32 or read.size != ny * nx:
        raise ValueError("the read noise must be a float32 plane of the cube's frame")
    nreads = np.array([len(g) for g in read_pattern], dtype=np.int32)
    if normals is not None:
        normals = np.ascontiguousarray(normals, dtype=np.float32)
        if normals.shape != (G, ny - 2 * nb, nx - 2 * nb):
            raise ValueError(f"normals have shape {normals.shape}")
    out = data if is_dev(data) else np.empty_like(data)   # the entry point allows in == out
    ctx.call("rip_stage_noise_inject", data, G, ny, nx, nb, read, nreads, normals, int(seed) & (2**64 - 1), layer, out)
    return out


def noise_1f_frames(nframes, rows=pars.nside, width=pars.channelwidth, normals=None, seed=0, stream=0, ctx=None):
    """``nframes`` frames (rows, width) f32 of 1/f noise (``sim_to_isim.noise_1f_frame`` :265-303) on the GPU (hipFFT).
    ``normals`` (nframes, 4*rows*width) f64 standard normal deviates or None (drawn on the device)."""
    ctx = ctx or _native.default_context()
    if normals is not None:
        normals = np.ascontiguousarray(normals, dtype=np.float64)
        if normals.shape != (nframes, 4 * rows * width):
            raise ValueError(f"normals have shape {normals.shape}, expected {(nframes, 4 * rows * width)}")
    out = np.empty((nframes, rows, width), np.float32)
    ctx.call("rip_stage_noise_1f", rows, width, nframes, normals, int(seed) & (2**64 - 1), int(stream) & 0xFFFFFFFF, out)
    return out


def ramp_weight_vectors(processinfo, ngrp):
    """The weights the ramp fit applied to a pixel as a function of its end slice (gen_noise_image.py:236-252): the stored
    optimal weights for a full ramp, the two-point weights for one truncated at ``iend``.  Returns (w (ngrp,ngrp) f32,
    has (ngrp,) u8, endslice i8 with non-positive entries mapped to ngrp - 1)."""
    meta = processinfo["meta"]
    w = np.zeros((ngrp, ngrp), dtype=np.float32)
    has = np.zeros(ngrp, dtype=np.uint8)
    w[-1] = np.asarray(processinfo["weights"], dtype=np.float32)
    has[-1] = 1
    start = 1 if processinfo["exclude_first"] else 0
    for iend in range(start + 2, ngrp):
        Kt = np.zeros(ngrp, dtype=np.float32)
        Kt[iend - 1] = 1.0 / (meta["tbar"][iend - 1] - meta["tbar"][start])
        Kt[start] = -Kt[iend - 1]
        w[iend - 1] = Kt
        has[iend - 1] = 1
    es = np.asarray(processinfo["endslice"])
    endslice = np.where(es > 0, es, ngrp - 1).astype(np.int8)
    return w, has, endslice


def poisson_resample(diff, skylevel, gain, frame_time, read_pattern, weights, has_weights, endslice, samples=None, seed=0,
                     layer=0, ctx=None):
    """Adds a resampled-Poisson realisation to ``diff`` (f32, in place; gen_noise_image.py:262-331).  ``gain`` already
    clipped; ``samples`` (nsamp, ny, nx) f64 Poisson deviates of mean clip(skylevel*gain*frame_time, 0) or None (device)."""
    ctx = ctx or _native.default_context()
    # every array may be a DevArray (resident in HBM): the entry point takes either kind of pointer
    if not ((isinstance(diff, np.ndarray) or is_dev(diff)) and diff.dtype == np.float32 and diff.flags.c_contiguous):
        raise TypeError("diff must be a C-contiguous float32 array (updated in place)")
    ngrp = len(read_pattern)
    first = np.array([g[0] for g in read_pattern], dtype=np.int32)
    count = np.array([len(g) for g in read_pattern], dtype=np.int32)
    for g in read_pattern:
        if list(g) != list(range(g[0], g[0] + len(g))):
            raise ValueError("groups must hold consecutive reads")
    nsamp = int(read_pattern[-1][-1]) + 1
    sky_ = skylevel if is_dev(skylevel) else np.ascontiguousarray(skylevel, dtype=np.float32)
    g_ = gain if is_dev(gain) else np.ascontiguousarray(gain)
    if g_.dtype not in (np.float32, np.float64):
        g_ = g_.astype(np.float64)
    if sky_.dtype != np.float32 or sky_.size != diff.size or g_.size != diff.size:
        raise ValueError("skylevel (float32) and gain must have the shape of diff")
    w = np.ascontiguousarray(weights, dtype=np.float32)
    hw = np.ascontiguousarray(has_weights, dtype=np.uint8)
    es = endslice if is_dev(endslice) else np.ascontiguousarray(endslice, dtype=np.int8)
    if es.dtype != np.int8 or es.size != diff.size:
        raise ValueError("endslice must be int8 of the shape of diff")
    if samples is not None:
        samples = np.ascontiguousarray(samples, dtype=np.float64)
        if samples.shape != (nsamp,) + diff.shape:
            raise ValueError(f"samples have shape {samples.shape}, expected {(nsamp,) + diff.shape}")
    ctx.call("rip_stage_poisson_resample", sky_, g_, _native.dtype_code(g_), diff.size, frame_time, ngrp, first, count, w, hw, es,
             samples, nsamp, int(seed) & (2**64 - 1), layer, diff)
    return diff


class _Files:
    """The files a layer list keeps coming back to (read, dark, gain, the L2 output), each read once per call."""

    def __init__(self):
        self.trees = {}

    def tree(self, src):
        if isinstance(src, dict):
            return src if "roman" in src else {"roman": src}
        key = str(src)
        if key not in self.trees:
            with calio.open_tree(src) as f:
                self.trees[key] = calio._materialise(f if isinstance(f, dict) else dict(f))
        return self.trees[key]

    def roman(self, src):
        return self.tree(src)["roman"]


def _device_path_applies(config, rng, tree=None):
    """The layer loop keeps its arrays in HBM when the exposures stay in memory, the deviates are the device's and nothing asks for a
    host-side ingredient (an ``AREAFACTOR`` file; a ``FITSWCS`` pixel-area map is made on the device and stays there).  An
    exposure stored with its reference read subtracted (``config["IN"]`` a tree with ``reference_read``, or ``tree`` = the tree
    read from it) keeps its layers on host arrays: every chain run is then a ``calibrateimage`` call, which decodes."""
    if not bool(config["NOISE"].get("IN_MEMORY", True)) or not bool(config["NOISE"].get("DEVICE_RESIDENT", True)):
        return False
    src = tree if tree is not None else config.get("IN")
    if isinstance(src, dict) and "reference_read" in (src["roman"] if "roman" in src else src):
        return False
    if isinstance(rng, np.random.Generator) or "AREAFACTOR" in config or not config["NOISE"].get("CORRELATED", True):
        return False
    return "saturation" in config["CALDIR"]


class _HostArrays:
    """Back end of ``make_noise_cube`` on numpy arrays: a chain run is a ``calibrateimage`` call on an L1 tree."""

    ctx = None   # the mirrors take the default context

    def __init__(self, config, files, base_tree, host_rng):
        self.config, self.tree, self.rng = config, base_tree, host_rng
        # config["NOISE"]["IN_MEMORY"] (default true): the noise-injected exposures and their L2 images stay in memory instead of going
        # through the TEMP files of the reference (same arithmetic; a layer then costs its two chain runs and the noise generation,
        # not four full-frame ASDF round trips); the dark-based reference image of the layers without 'a' is computed once
        self.in_memory = bool(config["NOISE"].get("IN_MEMORY", True))
        self.orig = np.asarray(files.roman(config["OUT"])["data"])
        self.dark_ref = None   # L2 "data" of the dark cube itself

    def up(self, a):
        return np.ascontiguousarray(a)

    def host(self, a):
        return a

    def zeros(self):
        return np.zeros(self.orig.shape, dtype=np.float32)

    def exposure(self, dark):
        """A fresh copy of the Level-1 cube (or of the dark standing in for it) and of amp33, and the L2 image they refer to."""
        roman = self.tree["roman"]
        cube = np.array(roman["data"] if dark is None else dark)
        a33 = None if roman.get("amp33") is None else np.array(roman["amp33"])
        if dark is None:
            return cube, a33, self.orig
        if not self.in_memory:
            return cube, a33, self.l2_data(cube, a33, "_refL2.asdf")
        if self.dark_ref is None:
            self.dark_ref = self.l2_data(cube, a33)
        return cube, a33, self.dark_ref

    def l2_data(self, cube, a33, out="_L2.asdf"):
        roman = dict(self.tree["roman"], data=cube)
        if a33 is not None:
            roman["amp33"] = a33
        tree = dict(self.tree, roman=roman)
        if self.in_memory:
            return np.asarray(calibrateimage(dict(self.config, IN=tree, OUT=None))["roman"]["data"])
        temp = self.config["NOISE"]["TEMP"]
        calio.write_asdf(temp, tree)
        config2 = deepcopy(self.config)
        config2["IN"] = temp
        config2["OUT"] = temp[:-5] + out
        calibrateimage(config2)
        with calio.open_tree(config2["OUT"]) as f_out:
            return np.array(f_out["roman"]["data"])

    def fill(self, synth, cube, a33, seed):
        """``L1Synth.fill`` on an upload of the exposure; the white deviates of a host generator are handed in in the reference's
        order, otherwise everything is drawn on the device."""
        import torch

        t_cube = torch.from_numpy(np.ascontiguousarray(cube).view(np.int16)).to(synth.dev)
        t_a33 = None if a33 is None else torch.from_numpy(np.ascontiguousarray(a33).view(np.int16)).to(synth.dev)
        normals = white33 = None
        if self.rng is not None:
            normals = self.rng.standard_normal((cube.shape[0] + 1,) + cube.shape[1:], dtype=np.float32)
            if t_a33 is not None:
                white33 = self.rng.standard_normal(tuple(t_a33.shape), dtype=np.float32)
        synth.fill(t_cube, t_a33, seed, banding=True, normals=normals, white33=white33)
        synth.ctx.synchronize()
        return t_cube.cpu().numpy().view(np.uint16), None if t_a33 is None else t_a33.cpu().numpy().view(np.uint16)

    def sub(self, a, b):
        return a - b

    def clip(self, a, lo, hi):
        return np.clip(a, lo, hi)

    def product(self, a, b):
        return a * b

    def add_ratio(self, diff, noise, gain):
        return (diff + noise / gain).astype(np.float32)   # f32 array += (f32 / gain dtype), cast back

    def pixels(self, endslice, k):
        pix = np.where(endslice == k)
        return pix, len(pix[0])

    def take(self, a, pix):
        return a[pix]

    def put(self, a, pix, values):
        a[pix] = values


class _DeviceArrays:
    """Back end of ``make_noise_cube`` with every full-frame array resident in HBM across the layers ("natural
    batch for the GPU"): the Level-1 cube and its dark-based counterpart, the L2 planes the layers refer to, the masks and weights
    are uploaded ONCE; a layer is then injection -> fresh reference pixels + correlated noise -> the fused chain -> sky model ->
    difference -> clip / resampled Poisson / pseudo-Poisson -> sky model, all through the same kernels as with host arrays
    (whose results it reproduces bit for bit: tests/test_gpu_noise.py), with only the finished layer (67 MB) going back to the
    host.  The few scalar steps (percentile interpolation, the 6 x 6 normal equations of the sky model, the moment ratios of the
    pseudo-Poisson layers) stay on the host as in the mirrors.  Arrays are ``DevArray``s whose torch work is complete (the
    library runs on its own stream)."""

    def __init__(self, config, files, base_tree, read_pattern):
        import torch

        from .. import pipeline
        from .gen_cal_image import _caldir_slot, wcs_from_config

        self.torch = torch
        caldir, roman = config["CALDIR"], base_tree["roman"]
        self.cb = cb = pipeline.Calibrator()
        self.ctx = cb.ctx
        self.slot = _caldir_slot(cb, caldir)
        self.dev = torch.device("cuda", self.ctx.device)
        self.read_pattern = read_pattern
        self.pid, _meta = cb.plan_for(read_pattern, float(roman["meta"]["exposure"]["frame_time"]), config.get("EXCLUDE_FIRST", True),
                                      config.get("RAMP_OPT_PARS"), config.get("JUMP_DETECT_PARS"))
        self.backup = config.get("SATURATION_BACKUP", 1)
        self.skyorder = int(config["SKYORDER"]) if "SKYORDER" in config else None
        self.cube = self.up(roman["data"])
        self.a33 = None if roman.get("amp33") is None else self.up(roman["amp33"])
        _G, ny, nx = self.cube.shape
        if "mask" in caldir:
            self.mask = self.up(np.array(files.roman(caldir["mask"])["dq"], dtype=np.uint32).view(np.int32))
        else:
            self.mask = self._done(torch.zeros((ny, nx), dtype=torch.int32, device=self.dev))
        thewcs = wcs_from_config(config)   # AreaFactor in HBM, the same map calibrateimage divides by
        self.area = None if thewcs is None else cb.area_factor(thewcs, ny, nx, device=True)
        self.orig = self.up(np.asarray(files.roman(config["OUT"])["data"], dtype=np.float32))
        self.outs = [torch.empty((ny, nx), dtype=torch.float32, device=self.dev) for _ in range(3)] + \
                    [torch.empty((ny, nx), dtype=torch.int32, device=self.dev)]
        self.dark_ref = None

    def _done(self, t, dtype=None):
        return DevArray(t.contiguous(), dtype).sync()

    def up(self, a):
        a = np.ascontiguousarray(a)   # u16 bits travel in an int16 tensor
        return self._done(self.torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(self.dev), a.dtype)

    def host(self, a):
        return a.numpy()

    def zeros(self):
        return self._done(self.torch.zeros(self.orig.shape, dtype=self.torch.float32, device=self.dev))

    def exposure(self, dark):
        """A clone of the Level-1 cube (or of the dark standing in for it) and of amp33, and the L2 image they refer to."""
        cube = self._done((self.cube if dark is None else dark).t.clone(), np.uint16)
        a33 = None if self.a33 is None else self._done(self.a33.t.clone(), np.uint16)
        if dark is None:
            return cube, a33, self.orig
        if self.dark_ref is None:
            self.dark_ref = self.l2_data(dark, self.a33)
        return cube, a33, self.dark_ref

    def l2_data(self, cube, a33):
        """roman.data of calibrateimage for a device-resident exposure: the chain, the active region, minus the sky model"""
        nb, o = pars.nborder, self.outs
        G, ny, nx = cube.shape
        self.cb.calibrate_device(self.slot, self.pid, G, cube.ctypes.data, True, None if a33 is None else a33.ctypes.data, None,
                                 self.mask.ctypes.data, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(),
                                 area_ptr=None if self.area is None else self.area.data_ptr(), flag_saturation=True,
                                 saturation_backup=self.backup, read_pattern=self.read_pattern)
        self.cb.synchronize()
        data = self._done(o[0][nb:ny - nb, nb:nx - nb])
        if self.skyorder is not None:
            sky.medfit(data, order=self.skyorder, subtract=True, ctx=self.ctx, want_model=False)
        return data

    def fill(self, synth, cube, a33, seed):
        synth.fill(cube.t, None if a33 is None else a33.t, seed, banding=True)   # in place, on the context's stream like the chain
        return cube, a33

    def sub(self, a, b):
        return self._done(a.t - b.t)

    def clip(self, a, lo, hi):
        return self._done(self.torch.clamp(a.t, float(lo), float(hi)))

    def product(self, a, b):
        return self._done((a.t * b.t).to(self.torch.float64))   # promoted like numpy's product, then the f64 the draws take

    def add_ratio(self, diff, noise, gain):
        return self._done((diff.t + noise.t / gain.t).to(self.torch.float32))   # numpy: f32 array += (f32 / gain dtype), cast back

    def pixels(self, endslice, k):
        pix = self.torch.nonzero(endslice.t == k, as_tuple=True)
        return pix, int(pix[0].numel())

    def take(self, a, pix):
        return self._done(a.t[pix])

    def put(self, a, pix, values):
        a.t[pix] = values.t.to(a.t.dtype)
        a.sync()


def make_noise_cube(config, rng=None):
    """The noise realisations listed in ``config["NOISE"]["LAYER"]``: array (N_noise, ny_active, nx_active) f32.  One layer loop;
    where the arrays live (numpy, or HBM when ``_device_path_applies``) and how a chain run is invoked is the back end's."""
    layers = config["NOISE"]["LAYER"]
    caldir = config["CALDIR"]
    files = _Files()
    host_rng = rng if isinstance(rng, np.random.Generator) else None
    seed = config["NOISE"].get("SEED", 0) if (rng is None or host_rng is not None) else int(rng)
    nb = pars.nborder
    with calio.open_tree(config["IN"]) as f_in:
        base_tree = calio._materialise(f_in if isinstance(f_in, dict) else dict(f_in))
    exposure = base_tree["roman"]["meta"]["exposure"]
    read_pattern = [list(map(int, g)) for g in exposure["read_pattern"]]
    ngrp = len(read_pattern)
    cube_dtype = np.asarray(base_tree["roman"]["data"]).dtype
    # the chain's u16 path is what the HBM-resident back end drives; a cube of anything else stays on the host
    if _device_path_applies(config, rng, base_tree) and cube_dtype == np.uint16:
        be = _DeviceArrays(config, files, base_tree, read_pattern)
    else:
        be = _HostArrays(config, files, base_tree, host_rng)
    read = be.up(np.asarray(files.roman(caldir["read"])["data"], dtype=np.float32))
    dark = synth = gain = None   # dark cube as data; from_sim.sim_to_isim.L1Synth of this CALDIR set; the inputs of 'O' and 'P' layers
    sky_models = {}
    noiseimage = np.zeros((len(layers),) + be.orig.shape, dtype=np.float32)
    for i_noise, cmd in enumerate(layers):
        diff = be.zeros()
        if "R" in cmd:
            noiseflags = _get_subscript(cmd, "R")
            if "a" not in noiseflags and dark is None:  # start from the dark instead of the data
                d = np.asarray(files.roman(caldir["dark"])["data"])
                de = d.shape[0] - ngrp
                if de not in [0, 1]:
                    raise ValueError("Dark date cube has the wrong shape.")
                dark = be.up(d.astype(cube_dtype)[de:, :, :])
            cube, a33, ref_data = be.exposure(None if "a" in noiseflags else dark)
            normals = None
            if host_rng is not None:  # one draw per group, in the reference's order
                na = (cube.shape[1] - 2 * nb, cube.shape[2] - 2 * nb)
                normals = np.stack([host_rng.standard_normal(na, dtype=np.float32) for _ in range(cube.shape[0])])
            cube = inject_read_noise(cube, read, read_pattern, nb=nb, normals=normals, seed=seed, layer=i_noise, ctx=be.ctx)
            # correlated noise: fresh reference pixels, reference output and 1/f noise (sim_to_isim.fill_in_refdata_and_1f), on the
            # device (from_sim.sim_to_isim.L1Synth.fill)
            if config["NOISE"].get("CORRELATED", True):
                if synth is None:
                    from ..from_sim.sim_to_isim import L1Synth

                    synth = L1Synth({k: files.roman(caldir[k]) for k in ("read", "gain", "dark")}, read_pattern, 1.0, ctx=be.ctx, nb=nb)
                cube, a33 = be.fill(synth, cube, a33, (int(seed) + 7919 * (i_noise + 1)) & (2**64 - 1))
            diff = be.sub(be.l2_data(cube, a33), ref_data)
            if "z" in noiseflags:
                zclip = float(_get_subscript(noiseflags.upper(), "Z"))
                p25, med, p75 = sky.nanpercentiles(diff, [25.0, 50.0, 75.0], ctx=be.ctx)
                iqr = p75 - p25
                print("***", noiseflags, zclip, iqr, med)
                diff = be.clip(diff, med - zclip * iqr / 1.34896, med + zclip * iqr / 1.34896)
        if ("O" in cmd or "P" in cmd) and gain is None:
            l2 = files.tree(config["OUT"])
            pinfo = l2["processinfo"]
            g = np.clip(np.asarray(files.roman(caldir["gain"])["data"]), 1e-4, 1e4)
            ws = np.asarray(l2["roman"]["data_withsky"], dtype=np.float32)
            d = (g.shape[-1] - ws.shape[-1]) // 2
            gain, withsky = be.up(g[d:-d, d:-d] if d > 0 else g), be.up(ws)
            w_all, has_all, es = ramp_weight_vectors(pinfo, ngrp)
            endslice = be.up(es)
        if "O" in cmd:
            # pseudo-Poisson layer (gen_noise_image.py:173-240): per end slice, the moment ratios of the ramp-fit slope under
            # Poisson noise (host), then one Pearson-family deviate per pixel of that end slice (device) scaled by the pixel's
            # gain * rate
            t_fr = l2["roman"]["meta"]["exposure"]["frame_time"]   # from the L2 file, like the read pattern below
            gI = be.product(gain, withsky)
            start = 1 if pinfo["exclude_first"] else 0
            rp_l2 = pinfo["meta"].get("read_pattern", read_pattern)   # from the L2 file, as gen_noise_image.py:208-212 reads it
            a_beta = np.array([rp_l2[k][0] for k in range(ngrp)], dtype=int)
            N_beta = np.array([len(rp_l2[k]) for k in range(ngrp)], dtype=int)
            noise_array = be.zeros()
            for k in range(start + 1, ngrp):
                tilnu21, tilnu31, tilnu41, _tilnu42 = get_tilde_nus(N_beta, a_beta, w_all[k])
                tilnu21 *= t_fr          # e/frame -> e/s
                tilnu31 *= t_fr**2
                tilnu41 *= t_fr**3
                pixels, npx = be.pixels(endslice, k)
                print("n pix", npx, "tilnus", tilnu21, tilnu31, tilnu41)
                sys.stdout.flush()
                if npx:
                    be.put(noise_array, pixels, draw_from_Pearson(
                        tilnu21, tilnu31, tilnu41, be.take(gI, pixels),
                        rng=host_rng if host_rng is not None else np.random.default_rng([int(seed) & 0xFFFFFFFF, i_noise, k]),
                        stream=100 * (i_noise + 1) + k, ctx=be.ctx))
            diff = be.add_ratio(diff, noise_array, gain)
        if "P" in cmd:
            noiseflags = _get_subscript(cmd, "P")
            t_fr = exposure["frame_time"]   # from the Level-1 file
            skylevel = withsky
            if "b" in noiseflags:  # background only: the low-order sky model (one per order for the whole list)
                sky_order = int("0" + _get_subscript(noiseflags.upper(), "B"))
                if sky_order not in sky_models:
                    sky_models[sky_order] = be.up(sky.medfit(withsky, order=sky_order, ctx=be.ctx)[1])
                skylevel = sky_models[sky_order]
            if "r" in noiseflags:
                samples = None
                if host_rng is not None:
                    e = np.clip(skylevel * gain * t_fr, 0.0, None)
                    samples = np.stack([host_rng.poisson(e.astype(np.float64)).astype(np.float64)
                                        for _ in range(int(read_pattern[-1][-1]) + 1)])
                poisson_resample(diff, skylevel, gain, t_fr, read_pattern, w_all, has_all, endslice, samples=samples, seed=seed,
                                 layer=1000 + i_noise, ctx=be.ctx)
        if "S" in cmd:
            sky_order = int("0" + _get_subscript(cmd, "S"))
            sky.medfit(diff, order=sky_order, subtract=True, ctx=be.ctx, want_model=False)
        noiseimage[i_noise] = be.host(diff)
    return noiseimage


def generate_all_noise(config):
    """Driver (gen_noise_image.py:334-389): ``config["NOISE"]`` holds LAYER (list of directives), TEMP (scratch file), SEED
    and OUT; the configuration must have been run through ``calibrateimage`` already."""
    noiseimage = make_noise_cube(config, None)
    print(np.shape(noiseimage))
    print("percentiles:")
    per_layer = [sky.nanpercentiles(layer, [5.0, 25.0, 50.0, 75.0, 95.0]) for layer in noiseimage]   # selection on the device
    for i, q in enumerate([5, 25, 50, 75, 95]):
        print(q, np.array([p[i] for p in per_layer]))
    if "NOISE_PRECISION" in config:
        if config["NOISE_PRECISION"] == 16:
            noiseimage = noiseimage.astype(np.float16)
        if config["NOISE_PRECISION"] not in [16, 32]:
            raise ValueError("Unsupported noise precision.")
    calio.write_asdf(config["NOISE"]["OUT"], {"config": config, "noise": noiseimage})
    if config.get("FITSOUT", False):
        # FITS has no float16: such a cube is widened first (gen_noise_image.py:387-391); the byte order is made on the device
        calio.write_fits(config["NOISE"]["OUT"][:-5] + "_asdf_to.fits", [np.ascontiguousarray(noiseimage, dtype=np.float32)])


if __name__ == "__main__":
    import yaml

    with open(sys.argv[1]) as f:
        cfg = yaml.safe_load(f)
    calibrateimage(cfg | {"SLICEOUT": True})
    generate_all_noise(cfg)
