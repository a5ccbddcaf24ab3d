"""What the GPU tests of the chain share (test_gpu_chain*.py, test_gpu_prepass_gate.py): the context every test starts from, CALDIR
slots that are dropped whatever happens, the comparisons with the oracle and between device results, device-resident calls, and
the shapes and inputs that reach a chosen launch geometry of the fused kernel.  A plain module: no fixtures, no test."""

import contextlib
from functools import lru_cache

import numpy as np
import torch  # before libromanhip is loaded: torch brings its own copy of the HIP runtime, and the first one loaded must be the one both use
from conftest import assert_same_bits, gpu_context

import oracle
from romanimpreprocess_amd import _native, synth

JUMP, SAT = 4, 2
F32, F64 = np.float32, np.float64
OUT = ("slope", "err_read", "err_poisson", "pixeldq", "groupdq")
MAX_NY = 1600


def read_pattern(G):
    """G groups of uneven lengths (1, 1, 2, 3, 5, 2, 1, 4, ... reads), consecutive reads, the first group the single read 0; the
    16 lengths repeat for a count above 16"""
    lens = [1, 1, 2, 3, 5, 2, 1, 4, 2, 3, 1, 2, 6, 1, 2, 1]
    rp, at = [], 0
    for g in range(G):
        rp.append(list(range(at, at + lens[g % 16])))
        at += lens[g % 16]
    return rp


def oracle_lines(ref, G, nch):
    """(G, nch, 2) LAPACK (m, c) the oracle used for the science channels."""
    lines = np.zeros((G, nch, 2))
    for g in range(G):
        lines[g] = ref["refpix_diag"][g]["channels"][:nch, 2:4]
    return lines


# ---- the context and its slots
def chain_context():
    """the process-wide context with every option at the library's default, whatever ran before"""
    ctx = gpu_context()
    ctx.reset_options()
    return ctx


@contextlib.contextmanager
def loaded(cb, slot, cal):
    """the CALDIR set `cal` in `slot` of the calibrator `cb`; the slot is dropped on the way out, after a failure too, and with it
    what the calibrator knows of it (a test that expects a never-loaded slot must not meet an earlier test's frame shape)"""
    cb.load_caldir(slot, cal)
    try:
        yield cb
    finally:
        cb.drop_caldir(slot)


# ---- comparisons
def assert_oracle(got, ref, what, cube=False):
    """flags bit for bit; corrected cube (where asked), slope and errors bit for bit, the sign of a zero aside"""
    if cube:
        assert_same_bits(got["cube"], ref["data"], f"{what}: corrected cube", zero_sign_ok=True)
    assert_same_bits(got["groupdq"], ref["groupdq"], f"{what}: groupdq")
    assert_same_bits(got["pixeldq"], ref["pixeldq"], f"{what}: pixeldq")
    for k in ("slope", "err_read", "err_poisson"):
        assert_same_bits(got[k], ref[k], f"{what}: {k}", zero_sign_ok=True)


def assert_equal_outputs(a, b, what, keys=OUT):
    """two device results: every bit, the sign of a zero included"""
    for k in keys:
        assert_same_bits(a[k], b[k], f"{what}: {k}")


# ---- device-resident calls
def to_dev(a):
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).to(torch.device("cuda", 0))


def ramp_to_dev(ramp):
    """[data, amp33, groupdq, pixeldq] of a host ramp on the device"""
    return [to_dev(ramp[k]) for k in ("data", "amp33", "groupdq", "pixeldq")]


def device_outputs(G, ny, nx):
    """the five result tensors of a device-resident call, in the order of OUT"""
    dev = torch.device("cuda", 0)
    return [torch.empty((ny, nx), dtype=torch.float32, device=dev) for _ in range(3)] + [
        torch.empty((ny, nx), dtype=torch.int32, device=dev), torch.empty((G, ny, nx), dtype=torch.uint8, device=dev)]


def calibrate_resident(cb, slot, pid, G, t, o, **kw):
    """Calibrator.calibrate_device on the tensors t = [data (u16), amp33, groupdq or None, pixeldq] and o = device_outputs(...)"""
    cb.calibrate_device(slot, pid, G, t[0].data_ptr(), True, t[1].data_ptr(), None if t[2] is None else t[2].data_ptr(),
                        t[3].data_ptr(), *(x.data_ptr() for x in o), **kw)


def outputs_to_numpy(o):
    """device_outputs(...) after a synchronisation, as the dict a host call returns (keys OUT)"""
    a = [x.cpu().numpy() for x in o]
    return dict(zip(OUT, (a[0], a[1], a[2], a[3].view(np.uint32), a[4])))


# ---- launch geometry of the fused kernel: shapes that reach a branch, inputs that make it show
def device_cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def geometry(G, kdt, ny, nx, ncu, reserve=None, quad_ok=True):
    return _native.chain_geometry_for(9, G, _native.RIP_F64 if kdt == F64 else _native.RIP_F32, ny, nx, ncu, reserve, quad_ok)


def find_height(ny0, step, has_property, what, lo=16):
    """ny0 where it has the property (the shapes are designed for 256 CUs), else the first height of the search that has it"""
    for ny in [ny0] + list(range(lo, MAX_NY + 1, step)):
        if has_property(ny):
            return ny
    raise AssertionError(f"no height up to {MAX_NY} rows gives {what} on this device ({device_cus()} CUs)")


def is_quad(g, live=None):
    return g is not None and g["nq"] > 0 and g["rows_q"] > 0 and (live is None or g["live_last"] == live)


def quad_columns(g, nx):
    """the science columns the quad workgroups emit: lanes 2 .. live-3 of the last strip's window, short of the 4 reference columns"""
    return slice((g["nstrips"] - 1) * (g["cols"] - 4) + 2, nx - 4)


def make_band_ramp(cal, rp, ny, nx, seed):
    """sources as everywhere, plus the bright band over the last 24 science columns"""
    rate = synth.make_rate_image(ny, nx, seed)
    band = 200.0 * 300.0 ** ((np.arange(ny) % 97) / 96.0)
    rate[4:ny - 4, nx - 28:nx - 4] += band[4:ny - 4, None]
    return synth.make_ramp(cal, read_pattern=rp, seed=seed, cr_frac=0.05, saturation_backup=0, rate=rate)


# built once per (G, dtype, shape, order, start), shared by the cases that use the same
@lru_cache(maxsize=2)
def inputs(G, k64, ny, nx, p, exclude_first, seed=31):
    rp = read_pattern(G)
    cal = synth.make_caldir(ny, nx, read_pattern=rp, p_order=p, seed=seed, bias_amplitude=2.0, bad_lin_frac=0.005,
                            ipc_dtype=F64 if k64 else F32)
    ramp = make_band_ramp(cal, rp, ny, nx, seed + 1)
    with np.errstate(all="ignore"):
        ref = oracle.calibrate_arrays(ramp, cal, exclude_first=exclude_first)
    return rp, cal, ramp, ref, oracle_lines(ref, G, nx // 128)


def band_conditions(ref, G, cols):
    """the oracle's own output, on the science columns `cols`: jumps, and first saturations at every group"""
    q = ref["groupdq"][:, :, cols]
    njump = np.count_nonzero(ref["pixeldq"][:, cols] & JUMP)
    assert njump >= 10, f"{njump} jump pixels in the oracle's output on columns {cols}"
    for g in range(1, G):
        n = np.count_nonzero((q[g] & SAT) & ~(q[g - 1] & SAT))
        assert n >= 10, f"{n} pixels first saturate at group {g} in the oracle's output on columns {cols}"
