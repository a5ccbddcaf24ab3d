"""The measured record of the FITS encoder (csrc/fitsout.hip) and writer (calio.write_fits), written to profiles/fits_out.txt:

    python tools/gpu_checks/fits_encode_timing.py [--out FILE] [--launches 30] [--batches 9] [--variant LIB] [--file /dev/shm/x.fits]

    (a) rip_stage_fits_encode of a noise cube, 8 x 4088 x 4088 float32 (535 MB), device to device: `launches` launches queued back
        to back on the context's stream, one synchronisation; `batches` such batches after a warm-up one.  Beside it
        hipMemcpyDtoDAsync of the same bytes on the same stream, in the same process, timed the same way: the kernel moves
        exactly the copy's bytes.  Also in place, and float64 / int16 samples of the same byte count.
    (b) the same with a byte mask (one more byte read per four-byte sample).
    (c) calio.write_fits of that cube from a DevArray to `--file`, against numpy on the downloaded cube: astype(">f4").tofile,
        with and without the download counted.
    --variant LIB: a second build of the library (csrc/fitsout.hip compiled with -DRIP_FITS_PLAIN_STORES=1: no non-temporal stores,
        linked with the other objects), loaded into the SAME process and timed in turn with the first for (a), (b).  The library
        itself stores non-temporally where dst is not src, and plainly in place.

A record, not a gate.  Wall times of the host (time.perf_counter around queue + synchronise); medians with minimum and maximum."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fits_out.txt"))
ap.add_argument("--launches", type=int, default=30)
ap.add_argument("--batches", type=int, default=9)
ap.add_argument("--variant", default=None)
ap.add_argument("--file", default="/dev/shm/fits_encode_timing.fits")
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from romanimpreprocess_amd import _native, calio  # noqa: E402
from romanimpreprocess_amd.devarray import DevArray  # noqa: E402

L, N = 8, 4088
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def hip_runtime():
    """the HIP runtime this process has loaded (torch's own copy where torch is installed)"""
    with open("/proc/self/maps") as f:
        paths = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
    if not paths:
        raise RuntimeError("no libamdhip64 is mapped into this process")
    return C.CDLL(paths[0]), paths[0]


def spread(ms):
    return f"median {statistics.median(ms):8.4f} ms   min {min(ms):8.4f}   max {max(ms):8.4f}"


ctx = _native.default_context(0)
dev = torch.device("cuda", 0)
prop = torch.cuda.get_device_properties(0)
hip, hip_path = hip_runtime()
say("FITS output (csrc/fitsout.hip, calio.write_fits): the measured record")
say(f"command : python tools/gpu_checks/fits_encode_timing.py --launches {args.launches} --batches {args.batches}"
    + (" --variant <library built with -DRIP_FITS_PLAIN_STORES=1>" if args.variant else ""))
say(f"box     : {prop.name} ({prop.gcnArchName}), {prop.multi_processor_count} CUs, {prop.total_memory / 2**30:.0f} GiB; torch {torch.__version__}, HIP {torch.version.hip}")
say(f"runtime : {os.path.basename(hip_path)}")
say()

# the library under test, and the variant with its own context on the same device
libs = [("the library", ctx.lib, ctx.h)]
if args.variant:
    vlib = C.CDLL(os.path.abspath(args.variant))
    for name in ("rip_ctx_create", "rip_stage_fits_encode", "rip_synchronize", "rip_stream"):
        getattr(vlib, name).restype, getattr(vlib, name).argtypes = _native.SYMBOLS[name]
    vh = C.c_void_p()
    if vlib.rip_ctx_create(0, C.byref(vh)) != 0:
        raise RuntimeError("the variant library gave no context")
    libs.append(("plain stores only", vlib, vh))

rng = np.random.default_rng(1)
host = rng.standard_normal((L, N, N), dtype=np.float32)
cube = torch.from_numpy(host).to(dev)
other = torch.empty_like(cube)
mask = (torch.rand((L, N, N), device=dev) < 0.2).to(torch.uint8)
torch.cuda.synchronize()
n, nbytes = cube.numel(), cube.numel() * 4
hip.hipMemcpyDtoDAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
hip.hipMemcpyDtoDAsync.restype = C.c_int


def encoder(lib, h, bitpix, count, src, dst, m=None):
    def run():
        rc = lib.rip_stage_fits_encode(h, src, bitpix, 0, count, _native.RIP_DEVICE, m, 1, -1000.0, dst, _native.RIP_DEVICE)
        if rc != 0:
            raise RuntimeError(f"rip_stage_fits_encode: {rc}")
    return run


def copier(lib, h):
    stream = C.c_void_p(lib.rip_stream(h))

    def run():
        rc = hip.hipMemcpyDtoDAsync(other.data_ptr(), cube.data_ptr(), nbytes, stream)
        if rc != 0:
            raise RuntimeError(f"hipMemcpyDtoDAsync: error {rc}")
    return run


def batches(call, lib, h):
    ms = []
    for b in range(args.batches + 1):
        t0 = time.perf_counter()
        for _ in range(args.launches):
            call()
        if lib.rip_synchronize(h) != 0:
            raise RuntimeError("rip_synchronize")
        if b:   # the first batch warms up
            ms.append((time.perf_counter() - t0) * 1e3 / args.launches)
    return ms


def rate(ms, moved):
    return f"{moved / 1e9 / (statistics.median(ms) * 1e-3):7.0f} GB/s of {moved / 1e6:.0f} MB moved"


# correctness of what is timed, once: the bytes of the device-to-device call against numpy
ctx.call("rip_stage_fits_encode", cube.data_ptr(), -32, 0, n, _native.RIP_DEVICE, None, 1, 0.0, other.data_ptr(), _native.RIP_DEVICE)
ctx.synchronize()
assert other[0, :64].cpu().numpy().tobytes() == host[0, :64].astype(">f4").tobytes()

say(f"(a), (b) device to device, {L} x {N} x {N} float32 ({nbytes / 1e6:.0f} MB), {args.launches} launches back to back, {args.batches} batches, per launch:")
medians = {}
for turn in range(2):   # each twice, the libraries in turn
    for label, lib, h in libs:
        rows = [("encode f32", encoder(lib, h, -32, n, cube.data_ptr(), other.data_ptr()), 2 * nbytes),
                ("encode f32, in place", encoder(lib, h, -32, n, other.data_ptr(), other.data_ptr()), 2 * nbytes),
                ("encode f64 (same bytes)", encoder(lib, h, -64, n // 2, cube.data_ptr(), other.data_ptr()), 2 * nbytes),
                ("encode i16 (same bytes)", encoder(lib, h, 16, n * 2, cube.data_ptr(), other.data_ptr()), 2 * nbytes),
                ("encode f32, masked", encoder(lib, h, -32, n, cube.data_ptr(), other.data_ptr(), mask.data_ptr()), 2 * nbytes + n),
                ("hipMemcpyDtoD", copier(lib, h), 2 * nbytes)]
        for name, call, moved in rows:
            ms = batches(call, lib, h)
            medians.setdefault((label, name), []).extend(ms)
            say(f"   {label:20s} {name:26s} {spread(ms)}   {rate(ms, moved)}")
say()
for label, _, _ in libs:
    c = statistics.median(medians[(label, "hipMemcpyDtoD")])
    say(f"   {label}: " + ", ".join(f"{name} / copy = {statistics.median(ms) / c:.3f}" for (lab, name), ms in medians.items()
                                    if lab == label and name != "hipMemcpyDtoD"))
if len(libs) == 2:
    say("   the library / plain stores only: " + ", ".join(
        f"{name} {statistics.median(medians[(libs[0][0], name)]) / statistics.median(medians[(libs[1][0], name)]):.3f}"
        for (lab, name) in medians if lab == libs[0][0] and name != "hipMemcpyDtoD"))
say()

# ---- (c) the file
del other, mask
torch.cuda.empty_cache()
darr = DevArray(cube)
t_write, t_numpy, t_numpy_dl = [], [], []
for i in range(4):
    t0 = time.perf_counter()
    calio.write_fits(args.file, [darr], ctx=ctx)
    t1 = time.perf_counter()
    if i:
        t_write.append((t1 - t0) * 1e3)
    size = os.path.getsize(args.file)
    os.remove(args.file)
    t0 = time.perf_counter()
    down = cube.cpu().numpy()
    t1 = time.perf_counter()
    with open(args.file, "wb") as f:
        f.write(calio.fits_header(down.shape, down.dtype))
        down.astype(">f4").tofile(f)
        f.write(b"\0" * (-down.nbytes % 2880))
    t2 = time.perf_counter()
    if i:
        t_numpy.append((t2 - t1) * 1e3)
        t_numpy_dl.append((t2 - t0) * 1e3)
    assert os.path.getsize(args.file) == size
    os.remove(args.file)
    del down
# the two writers give the same file (checked once, on the first 64 MB and the last block)
calio.write_fits(args.file, [darr], ctx=ctx)
with open(args.file, "rb") as f:
    headblock = f.read(2880 + (64 << 20))
    f.seek(-2880, os.SEEK_END)
    last = f.read()
os.remove(args.file)
want = calio.fits_header(host.shape, host.dtype) + host.reshape(-1)[:(64 << 20) // 4].astype(">f4").tobytes()
assert headblock == want
assert last == (host.reshape(-1)[-720:].astype(">f4").tobytes() + b"\0" * (-nbytes % 2880))[-2880:]
say(f"(c) the cube as a FITS file on {os.path.dirname(args.file)} ({size / 1e6:.0f} MB), 3 runs each after a warm-up one:")
say(f"   calio.write_fits from a DevArray (encode on the device, two staging buffers)   {spread(t_write)}   {size / 1e6 / statistics.median(t_write):6.2f} GB/s")
say(f"   numpy astype('>f4').tofile of the cube already on the host                     {spread(t_numpy)}   {size / 1e6 / statistics.median(t_numpy):6.2f} GB/s")
say(f"   the same with the download (tensor.cpu()) counted                              {spread(t_numpy_dl)}   {size / 1e6 / statistics.median(t_numpy_dl):6.2f} GB/s")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
