"""ctypes binding of ``libromanhip.so`` (C-ABI: ``include/romanhip.h``).

This is the only door between the Python host code and the HIP kernels.  There is no CPU
fallback: if the library is missing or no MI355X is visible, the calls raise.
"""

import contextlib
import ctypes as C
import os

import numpy as np

from . import _header
from .devarray import DevArray

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ROMANHIP_LIB") or os.path.join(_HERE, "libromanhip.so")   # the env var: A/B timing of library variants

# The C interface is stated once, in include/romanhip.h; everything below is read from it (``_header.parse``).
with open(os.path.join(os.path.dirname(_HERE), "include", "romanhip.h")) as _f:
    HEADER = _header.parse(_f.read())
PROTOTYPES = HEADER.prototypes   # name -> _header.Proto: per parameter its name, ctypes type and pointee

# every constant of the header under its own name (RIP_F32, RIP_HOST, RIP_PROJ_TAN, RIP_MAX_GROUPS, RIP_EINVAL, ...); the stage
# bits and the bias states also without the prefix (STAGE_REFPIX .. STAGE_ALL, BIAS_ABSENT / BIAS_PRESENT / BIAS_DROPPED)
globals().update(HEADER.constants)
globals().update({k[4:]: v for k, v in HEADER.constants.items() if k.startswith(("RIP_STAGE_", "RIP_BIAS_"))})

# the structs; a pointer field of any kind is a c_void_p that the caller fills with an address
CaldirDesc = HEADER.structs["rip_caldir_desc"]
PlanDesc = HEADER.structs["rip_plan_desc"]
RampDesc = HEADER.structs["rip_ramp_desc"]
Outputs = HEADER.structs["rip_outputs"]
SynthCal = HEADER.structs["rip_synth_cal"]    # DEVICE pointers
CrParams = HEADER.structs["rip_cr_params"]    # the cosmic-ray model's constants (defaults: romanisim's)
WcsDesc = HEADER.structs["rip_wcs_desc"]      # a FITS zenithal (+SIP) WCS, crpix 0-based, angles in degrees

# every symbol the header declares: name -> (restype, argtypes).  Pointers to a header struct are POINTER(mirror), const char *
# is c_char_p, every other pointer c_void_p: raw callers pass ndarray.ctypes.data, data_ptr(), byref(...) and ctypes arrays.
SYMBOLS = {name: (p.restype, [q.ctype for q in p.params]) for name, p in PROTOTYPES.items()}

_lib = None


def load_library():
    """dlopen the in-tree library and bind every declared symbol (no GPU needed for this)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C romanimpreprocess_amd/csrc`).  romanimpreprocess_amd has no CPU fallback."
        )
    # PyTorch (used by the device-resident mirrors for device memory) ships its own HIP runtime under the same soname: whichever
    # of the two is loaded first serves both, and only PyTorch's own copy leaves PyTorch with its devices.  So it goes first,
    # whenever it is installed; without it the library runs on the system's runtime alone.
    try:
        import torch  # noqa: F401, PLC0415
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    ver = lib.rip_version()
    if ver >= RIP_TIMING_BUILD_FLAG and os.environ.get("ROMANHIP_ALLOW_TIMING_BUILD") != "1":
        raise RuntimeError(f"{LIB_PATH} is a timing build (compiled with -DRIP_TIMING_BUILD: its kernels may skip phases, results "
                           "invalid by construction); set ROMANHIP_ALLOW_TIMING_BUILD=1 to load it for timing experiments")
    _lib = lib
    return lib


# ---- one checked call path ------------------------------------------------------------------------------------------------
# numpy dtype of a pointer's element type (``Param.elem``); void, rip_ctx and pointers to pointers are not in it: anything goes
_ELEM_DTYPE = {name: np.dtype(t) for name, t in _header.SCALARS.items() if name != "char"}
_CTYPES = (C._SimpleCData, C.Array, C.Structure, C._Pointer, type(C.byref(C.c_int())))


def _convert(fn, p, x):
    """``x`` as the library takes it for parameter ``p`` of ``fn``; TypeError where it is not what the header declares"""
    t = type(x)
    if p.depth == 0:
        to = float if p.ctype is C.c_double or p.ctype is C.c_float else int
        if t is int or t is float or t is bool or getattr(x, "shape", None) == ():   # Python and numpy scalars, never an array
            try:
                return to(x)
            except (TypeError, ValueError):
                pass
        raise TypeError(f"{fn}: parameter '{p.name}' is a scalar ({p.ctext}), got {_describe(x)}")
    if x is None or t is int:
        return x
    want = _ELEM_DTYPE.get(p.elem) if p.depth == 1 else None
    if t is np.ndarray or (hasattr(x, "ctypes") and hasattr(x, "dtype")):   # a numpy array or a DevArray
        if (want is not None or p.elem == "void") and x.flags.c_contiguous \
                and (want is None or x.dtype == want or (want == np.uint8 and x.dtype == np.bool_)):
            return x.ctypes.data
    elif hasattr(x, "data_ptr"):   # a torch tensor: u16 / u32 bits live in int16 / int32 tensors, so width and kind are compared
        if (want is not None or p.elem == "void") and x.is_contiguous() \
                and (want is None or (x.element_size() == want.itemsize and not x.dtype.is_complex
                                      and x.dtype.is_floating_point == (want.kind == "f"))):
            return x.data_ptr()
    elif isinstance(x, _CTYPES):   # byref(...), ctypes arrays and pointers, a handle; a struct goes by reference
        return C.byref(x) if isinstance(x, C.Structure) else x
    elif p.ctype is C.c_char_p and isinstance(x, (str, bytes)):
        return x.encode() if isinstance(x, str) else x
    elif isinstance(x, np.integer):
        return int(x)
    raise TypeError(f"{fn}: parameter '{p.name}' ({p.ctext}): expected a C-contiguous array of "
                    f"{want.name if want is not None else p.elem}, None or an address, got {_describe(x)}")


def _describe(x):
    if hasattr(x, "data_ptr"):
        return f"a {'contiguous' if x.is_contiguous() else 'non-contiguous'} tensor of {x.dtype}"
    if hasattr(x, "dtype") and hasattr(x, "flags"):
        return f"a {'C-contiguous' if x.flags.c_contiguous else 'non-contiguous'} array of {x.dtype}"
    return f"{type(x).__name__} {x!r}"[:80]


def marshal(name, args):
    """The arguments of entry ``name`` checked against its prototype in the header and converted to what ctypes passes on: an
    array (numpy, ``DevArray``, torch tensor) must be contiguous and of the pointer's element type and gives its address; None
    is NULL; an int is an address; ``byref(...)`` and ctypes objects go through (a struct by reference); scalars are converted
    by their C type.  It checks, it never casts.  Needs no GPU and no context."""
    params = PROTOTYPES[name].params
    if len(args) != len(params):
        raise TypeError(f"{name} takes {len(params)} arguments ({', '.join(p.name for p in params)}), got {len(args)}")
    return [_convert(name, p, x) for p, x in zip(params, args)]


def _fail(lib, h, rc, exc=RuntimeError):
    msg = lib.rip_last_error(h)
    text = msg.decode() if msg else f"status {rc}"
    raise (ValueError if rc == RIP_EINVAL else exc)(f"libromanhip: {text}")


def call(name, *args):
    """Entry ``name`` of the library on ``marshal``-ed arguments.  A negative return of an ``int`` entry raises (ValueError for
    RIP_EINVAL, RuntimeError otherwise) with the library's message.  This is the form for the entries without a context
    (``rip_chain_form_for``, ``rip_option_info``, ...); ``Context.call`` puts the handle in front."""
    lib = load_library()
    rc = getattr(lib, name)(*marshal(name, args))
    if rc is not None and rc < 0 and PROTOTYPES[name].restype is C.c_int:
        _fail(lib, args[0] if _takes_ctx(name) else None, rc)
    return rc


def _takes_ctx(name):
    params = PROTOTYPES[name].params
    return bool(params) and params[0].elem == "rip_ctx" and params[0].depth == 1


def chain_form_for(lin_nplanes, ngroups, ipc_dtype=RIP_F32, gain_dtype=RIP_F32):
    """2 where the library has a fused-kernel form for a complete chain on a ramp of ``ngroups`` groups with ``lin_nplanes``
    Legendre planes and these ipc4d / gain dtypes (RIP_F32, RIP_F64), 0 where the stage kernels run.  Needs no GPU.  It does not
    know the plan or the CALDIR set: a ramp also takes the stage kernels when the plan's differences are not the full set or
    the set's flag words cannot be merged (``Context.last_chain_form`` tells what a call really ran)."""
    return call("rip_chain_form_for", lin_nplanes, ngroups, ipc_dtype, gain_dtype)


def option_table():
    """The library's option table (``rip_option_info``) as name -> (default, lowest, highest accepted value); the one f64 option,
    "guard_band", appears with its values cut to int.  Needs no GPU."""
    table = {}
    name, d, lo, hi = C.c_char_p(), C.c_int(), C.c_int(), C.c_int()
    while call("rip_option_info", len(table), C.byref(name), C.byref(d), C.byref(lo), C.byref(hi)):
        table[name.value.decode()] = (d.value, lo.value, hi.value)
    return table


GEOMETRY_FIELDS = ("cols", "nstrips", "live_last", "nr", "rows", "nq", "rows_q", "grid")


def chain_geometry_for(lin_nplanes, ngroups, ipc_dtype, ny, nx, ncu, reserve=None, quad_ok=True, gain_dtype=RIP_F32):
    """The fused kernel's launch geometry for such a ramp on an (ny, nx) frame and a device of ``ncu`` compute units, as a dict
    with the keys ``GEOMETRY_FIELDS`` (``rip_chain_geometry_for``: ``nq`` > 0 means quad mode), or None where the stage kernels
    run.  ``reserve`` None: the default of the option "chain_reserve".  Needs no GPU; ``Context.last_chain_geometry`` tells
    what a call really used."""
    if reserve is None:
        reserve = option_table()["chain_reserve"][0]
    out = (C.c_int * 8)()
    rc = call("rip_chain_geometry_for", lin_nplanes, ngroups, ipc_dtype, gain_dtype, ny, nx, ncu, reserve, bool(quad_ok), out)
    return dict(zip(GEOMETRY_FIELDS, out)) if rc == 2 else None


def float_array(a):
    """C-contiguous float32 or float64 array of ``a`` (any other dtype becomes float64): what goes to a ``const void *`` parameter
    that comes with a ``dtype_code``"""
    a = np.ascontiguousarray(a)
    return a if a.dtype in (np.float32, np.float64) else a.astype(np.float64)


def dtype_code(arr):
    code = {np.dtype(np.float32): RIP_F32, np.dtype(np.float64): RIP_F64, np.dtype(np.uint16): RIP_U16}.get(arr.dtype)
    if code is None:
        raise TypeError(f"unsupported dtype {arr.dtype}")
    return code


def location_of(a):
    """The ``location`` argument that goes with array ``a``: RIP_DEVICE for a ``DevArray`` or a torch tensor on the GPU, RIP_HOST
    for a numpy array; TypeError for anything else (a torch tensor in host memory included: ``.numpy()`` it)"""
    if isinstance(a, np.ndarray):
        return RIP_HOST
    t = a.t if isinstance(a, DevArray) else a
    if hasattr(t, "data_ptr") and getattr(t, "is_cuda", False):
        return RIP_DEVICE
    raise TypeError(f"location_of: a numpy array, a DevArray or a tensor on the GPU, got {_describe(a)}")


class Context:
    """One rip_ctx (one GPU).  Raises RuntimeError when the library or the GPU is unavailable."""

    def __init__(self, device=0):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.rip_ctx_create(*marshal("rip_ctx_create", (device, C.byref(h))))
        if rc != 0:   # no context to ask: the message of the last failed create
            msg = self.lib.rip_last_error(None)
            raise RuntimeError(f"rip_ctx_create(device={device}) failed: {msg.decode() if msg else rc}")
        self.h = h
        self.device = int(device)
        self.caldir_dtypes = {}   # slot -> (Legendre planes, ipc4d dtype, gain dtype) of the set uploaded there
        # what every pipeline.Calibrator on this context shares
        self.shapes = {}          # slot -> (ny, nx) of the set uploaded there
        self.caldir_owner = {}    # slot -> the owner tag given to Calibrator.load_caldir
        self.plans = {}           # plan configuration -> (plan id, meta)
        self.result_pool = None   # the pipeline.ResultPool of result arrays (made by the first Calibrator)
        self.area_cache = {}      # (WCS digest, ny, nx, on the device) -> pixel-area map, at most two
        self.refread_count = None   # the device word the last asynchronous decode_reference_read adds to: kept alive here
        self.fits_staging = None    # the two page-locked chunk buffers of calio.write_fits, kept from call to call

    def close(self):
        if getattr(self, "h", None):
            self.lib.rip_ctx_destroy(self.h)   # direct: this also runs at interpreter exit, when the module's globals may be gone
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def call(self, name, *args):
        """Entry ``name`` on this context: the handle goes in front where the entry's first parameter is ``rip_ctx *``, the
        arguments through ``marshal``.  A negative return of an ``int`` entry raises as ``check`` does; a non-negative one is
        returned as int, other return types as they are."""
        return call(name, self.h, *args) if _takes_ctx(name) else call(name, *args)

    def check(self, rc, exc=RuntimeError):
        """for raw callers of ``ctx.lib``: raise on a non-zero status with the library's message"""
        if rc != 0:
            _fail(self.lib, self.h, rc, exc)

    def synchronize(self):
        self.call("rip_synchronize")

    def pinned_empty(self, shape, dtype):
        """A numpy array in page-locked host memory (``rip_host_alloc``), freed with the array."""
        import weakref

        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = self.call("rip_host_alloc", nbytes)
        if not p:
            self.check(RIP_ENOMEM, MemoryError)
        buf = (C.c_ubyte * max(nbytes, 1)).from_address(p)
        arr = np.frombuffer(buf, dtype=np.uint8, count=nbytes).view(dtype).reshape(shape)
        weakref.finalize(buf, call, "rip_host_free", self.h, p).atexit = False   # at exit the process returns it
        return arr

    def set_option(self, name, value):
        self.call("rip_set_option", name, value)

    def set_option_f64(self, name, value):
        """floating-point options of this context ("guard_band")"""
        self.call("rip_set_option_f64", name, value)

    def get_option(self, name):
        v = C.c_int()
        self.call("rip_get_option", name, C.byref(v))
        return v.value

    def get_option_f64(self, name):
        v = C.c_double()
        self.call("rip_get_option_f64", name, C.byref(v))
        return v.value

    def reset_options(self):
        """every option back to the library's default (``option_table``)"""
        self.call("rip_reset_options")

    @contextlib.contextmanager
    def options(self, **values):
        """``with ctx.options(fused=0, guard_band=float("inf")):`` sets these options for the block and puts back, in reverse
        order and on an exception too, what they held before.  float values are the f64 options."""
        calls = {name: ((self.get_option_f64, self.set_option_f64) if isinstance(v, float) else (self.get_option, self.set_option))
                 for name, v in values.items()}
        old = []
        try:
            for name, v in values.items():
                get, set_ = calls[name]
                before = get(name)
                set_(name, v)
                old.append((set_, name, before))
            yield self
        finally:
            for set_, name, before in reversed(old):
                set_(name, before)

    def last_chain_form(self):
        """0 = stage kernels, 2 = the fused kernel (last calibrate call; 1 and 3 were the general and wave-private fused kernels of rounds 1-2)."""
        return self.call("rip_last_chain_form")

    def last_chain_first_group(self):
        """1 = the fused launch of the last calibrate call skipped group 0 (option "skip_first"), 0 = it did not (or stage kernels)."""
        return self.call("rip_last_chain_first_group")

    def last_prepass_gate(self):
        """(state, give-ups) of the gate in front of the last calibrate call's overlapped pre-pass (option "prepass_gate"): state 0 =
        none queued, 1 = released by the fused kernel's workgroup count, 2 = gave up at its bound; give-ups of this context so far.
        Waits for the context's streams."""
        n = C.c_int(0)
        return self.call("rip_last_prepass_gate", C.byref(n)), n.value

    def caldir_first_group_safe(self, slot):
        """True where the set in ``slot`` passed the upload screen that lets the fused kernel skip an excluded first group."""
        return self.call("rip_caldir_first_group_safe", slot) == 1

    def caldir_bias_state(self, slot):
        """``BIAS_ABSENT`` (no biascorr in the set of ``slot``), ``BIAS_PRESENT`` (subtracted by every call with ``STAGE_BIAS``) or
        ``BIAS_DROPPED`` (given, every word +0: no device copy is kept and calls subtract nothing)"""
        return self.call("rip_caldir_bias_state", slot)

    def last_chain_bias_stream(self):
        """1 = the fused launch of the last calibrate call streamed the biascorr planes, 0 = it ran without them (or stage kernels)."""
        return self.call("rip_last_chain_bias_stream")

    def last_chain_geometry(self):
        """launch geometry of the last calibrate call's fused kernel (keys ``GEOMETRY_FIELDS``); all zeros after a stage-kernel run"""
        out = (C.c_int * 8)()
        self.call("rip_last_chain_geometry", out)
        return dict(zip(GEOMETRY_FIELDS, out))

    def profile(self, on=True):
        self.call("rip_profile_enable", bool(on))

    def profile_read(self):
        """(ms per stage [refpix pre-pass, cube stage, ipc, ramp fit], number of calls) since the last read."""
        ms = (C.c_double * 4)()
        n = C.c_int(0)
        self.call("rip_profile_read", ms, C.byref(n))
        return list(ms), n.value

    @property
    def stream(self):
        return self.call("rip_stream")

    # ---- CALDIR ------------------------------------------------------------------------
    def upload_caldir(self, slot, cal, nborder=4, refout_slope=None):
        """``cal``: dict of dicts of numpy arrays, layout of the ``roman`` branch of each CALDIR file."""
        d = CaldirDesc()
        keep = []

        def P(a, dt):
            """address of ``a`` converted to ``dt`` (the copy is kept until the upload is done), None for None"""
            if a is None:
                return None
            keep.append(np.ascontiguousarray(a, dtype=dt))
            return keep[-1].ctypes.data

        gain = float_array(cal["gain"]["data"])
        ny, nx = gain.shape
        d.ny, d.nx, d.nborder = ny, nx, nborder
        dark = cal.get("dark")
        if dark is not None:
            if "data" in dark and dark["data"] is not None:
                d.ngrp_dark = dark["data"].shape[0]
                d.dark_data = P(dark["data"], np.float32)
            d.dark_slope = P(dark.get("dark_slope"), np.float32)
            d.dark_dq = P(dark.get("dq"), np.uint32)
        rd = cal["read"]
        d.read_noise = P(rd["data"], np.float32)
        a33 = rd.get("amp33")
        if a33 is not None:
            d.amp33_med = P(a33["med"], np.float32)
            d.refout_slope = float(refout_slope)
        d.gain = gain.ctypes.data
        d.gain_dtype = dtype_code(gain)
        lin = cal.get("linearitylegendre")
        if lin is not None:
            d.lin_nplanes = lin["data"].shape[0]
            d.lin_coefs = P(lin["data"], np.float32)
            d.lin_smin = P(lin["Smin"], np.float32)
            d.lin_smax = P(lin["Smax"], np.float32)
            d.lin_sref = P(lin["Sref"], np.float32)
            d.lin_dq = P(lin["dq"], np.uint32)
        if cal.get("ipc4d") is not None:
            k = float_array(cal["ipc4d"]["data"])
            if k.shape != (3, 3, ny - 2 * nborder, nx - 2 * nborder):
                raise ValueError(f"ipc4d shape {k.shape} does not match frame {ny}x{nx} with border {nborder}")
            d.ipc4d = k.ctypes.data
            d.ipc_dtype = dtype_code(k)
        if cal.get("flat") is not None:
            d.flat = P(cal["flat"]["data"], np.float32)
        if cal.get("biascorr") is not None:
            b = cal["biascorr"]["data"]
            d.ngrp_bias = b.shape[0]
            d.biascorr = P(b, np.float32)
        if cal.get("saturation") is not None:  # only needed for flag_saturation (device dq-init + saturation flagging)
            d.saturation = P(cal["saturation"]["data"], np.float32)
            d.saturation_dq = P(cal["saturation"].get("dq"), np.uint32)
        self.call("rip_caldir_upload", slot, d)
        # what rip_chain_form_for asks about (Calibrator.chain_form_for)
        self.caldir_dtypes[int(slot)] = (int(d.lin_nplanes), int(d.ipc_dtype), int(d.gain_dtype))
        return (ny, nx)

    def drop_caldir(self, slot):
        self.call("rip_caldir_drop", slot)
        self.caldir_dtypes.pop(int(slot), None)

    # ---- plans -------------------------------------------------------------------------
    def create_plan(self, desc):
        pid = C.c_int(-1)
        self.call("rip_plan_create", desc, C.byref(pid))
        return pid.value

    def destroy_plan(self, pid):
        self.call("rip_plan_destroy", pid)

    # ---- the chain ---------------------------------------------------------------------
    def calibrate_raw(self, slot, plan, stages, ramp_desc, outputs):
        self.call("rip_calibrate", slot, plan, stages, ramp_desc, outputs)


_default = {}


def default_context(device=None):
    """Process-wide context for ``device`` (default: LOCAL_RANK, else 0)."""
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0"))
    if device not in _default:
        _default[device] = Context(device)
    return _default[device]
