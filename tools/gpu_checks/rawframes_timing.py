"""Time of the raw-frame conversion (csrc/rawframes.hip) at production size: frames of 4096 x 4224 samples, an exposure of 56 frames.

  (a) rip_cal_raw_frame, frame and cube resident in HBM, FITS storage with BZERO: columns reversed (sca % 3 == 0) and rows reversed,
      against a device-to-device copy of the same 34.6 MB (torch.Tensor.copy_, the runtime's DtoD copy) in the same process
  (b) the same call from a host array (pageable memory, as calio.read_fits_image maps a file: the frame crosses PCIe)
  (c) rip_cal_frame_slopes on the resident cube at Nc = 10 (the flat converters) and Nc = N = 56 (convert_dark), against a
      device-to-device copy of the bytes the kernel reads
  (d) tests/rawframes_ref.py (numpy, one core) on one exposure: orientation and slopes of 11 frames (flat) and of 56 (dark); the
      device results are compared with it bit for bit
A record, not a gate.  Writes profiles/rawframes.txt (or the file named by the first argument).
RAWFRAMES_TIMING_KERNEL_ONLY=1: a few calls of each kernel, for `rocprofv3 --kernel-trace --stats -- python <this file>`.
"""
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")
REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime for both)
import rawframes_ref as ref  # noqa: E402

from romanimpreprocess_amd import _native  # noqa: E402
from romanimpreprocess_amd.calfiles import convert_frames  # noqa: E402
from romanimpreprocess_amd.devarray import DevArray  # noqa: E402

NY, NX, NFLIP, N, REPS = 4096, 4224, 4096, 56, 20
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "rawframes.txt")
kernel_only = os.environ.get("RAWFRAMES_TIMING_KERNEL_ONLY") == "1"
ctx = _native.default_context(0)
HOST, DEVICE = _native.RIP_HOST, _native.RIP_DEVICE
npix = NY * NX
gen = torch.Generator(device="cuda").manual_seed(7)
lines = []


def say(text):
    print(text)
    sys.stdout.flush()
    lines.append(text)


def timed(fn, reps=REPS, warm=3):
    """(mean, min, max) ms of `reps` calls after `warm`; every fn ends in a device synchronise"""
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.mean(ms)), min(ms), max(ms)


def copy_ms(nbytes):
    a = torch.empty(nbytes // 2, dtype=torch.int16, device="cuda")
    b = torch.empty_like(a)

    def fn():
        b.copy_(a)
        torch.cuda.synchronize()

    return timed(fn)


# the frames as stored (big-endian int16, BZERO 32768) and the cube, in HBM
samples = torch.randint(0, 65536, (N, NY, NX), device="cuda", generator=gen, dtype=torch.int32).to(torch.int16)   # the low 16 bits
host_samples = samples.cpu().numpy().view(np.uint16)
stored_host = [ref.encode(host_samples[k], 1) for k in range(N)]
stored = torch.stack([torch.from_numpy(s.view(np.uint16).view(np.int16)) for s in stored_host[:2]]).cuda()
cube = DevArray(torch.empty((1, N, NY, NX), dtype=torch.int16, device="cuda"), np.uint16)
torch.cuda.synchronize()


def frame(k, orient, src=None, loc=DEVICE):
    ctx.call("rip_cal_raw_frame", stored[k % 2].data_ptr() if src is None else src, loc, NY, NX, orient, NFLIP, 1,
             DevArray(cube.t[0, k], np.uint16))


w10, w56 = convert_frames.slope_weights(10), convert_frames.slope_weights(N)
slp = DevArray(torch.empty((2, NY, NX), dtype=torch.float32, device="cuda"))


def slopes(nc, w):
    ctx.call("rip_cal_frame_slopes", cube, N, nc, npix, w[0], w[1], w[2], w[3], slp, DEVICE)


if kernel_only:
    for orient in (1, 2):
        for k in range(4):
            frame(k, orient)
    for _ in range(3):
        slopes(10, w10)
        slopes(N, w56)
    sys.exit(0)

say(f"raw frames {NY} x {NX} u16 ({2 * npix / 1e6:.1f} MB a frame), exposure of {N} frames ({torch.cuda.get_device_name(0)}); "
    f"mean (min .. max) of {REPS} calls, host clock around calls that end in a device synchronise")
fb = 2 * npix
c_mean, c_min, c_max = copy_ms(fb)
say(f"  device-to-device copy of one frame:                       {c_mean:8.3f} ms ({c_min:.3f} .. {c_max:.3f})  {2 * fb / c_mean / 1e6:6.0f} GB/s read + written")
for orient, what in ((1, "columns 0..4095 reversed"), (2, "rows reversed          ")):
    m, lo, hi = timed(lambda: frame(1, orient))
    say(f"  (a) frame_kernel, resident, {what}:     {m:8.3f} ms ({lo:.3f} .. {hi:.3f})  {2 * fb / m / 1e6:6.0f} GB/s read + written, "
        f"x{m / c_mean:.2f} of the copy")
m, lo, hi = timed(lambda: frame(1, 1, stored_host[1].view(np.uint16), HOST), reps=5, warm=1)
say(f"  (b) the same from a host array (pageable), 5 calls:       {m:8.2f} ms ({lo:.2f} .. {hi:.2f})  {fb / m / 1e6:6.1f} GB/s over PCIe")

# the whole exposure into the cube, both orientations, for the comparison with numpy
results = {}
for sca in (3, 4):
    t0 = time.perf_counter()
    for k in range(N):
        frame(k, 1 if sca % 3 == 0 else 2, stored_host[k].view(np.uint16), HOST)
    upload_ms = 1e3 * (time.perf_counter() - t0)
    for nc, w in ((10, w10), (N, w56)):
        slopes(nc, w)
        results[(sca, nc)] = slp.numpy().copy()
    if sca == 3:
        cube3 = cube.numpy()[:, :11].copy()
say(f"      a whole exposure of {N} host frames into the cube:      {upload_ms:8.1f} ms")
for nc, w in ((10, w10), (N, w56)):
    rb = (nc - 1) * fb
    c_mean, c_min, c_max = copy_ms(rb)
    m, lo, hi = timed(lambda: slopes(nc, w))
    say(f"  (c) slopes_kernel, Nc = {nc:2d}: {rb / 1e6:7.1f} MB read, {4 * fb / 1e6:.1f} MB written: {m:8.3f} ms ({lo:.3f} .. {hi:.3f})  "
        f"{(rb + 4 * fb) / m / 1e6:6.0f} GB/s; copy of the bytes read {c_mean:.3f} ms ({c_min:.3f} .. {c_max:.3f}), "
        f"{2 * rb / c_mean / 1e6:.0f} GB/s read + written: x{m / c_mean:.2f} of the copy")
cube4 = cube.numpy()

# (d) numpy on one core
frames = [host_samples[k] for k in range(N)]
t0 = time.perf_counter()
flat_cube, flat_slp = ref.exposure(frames[:11], 3, NFLIP, "flt")
flat_s = time.perf_counter() - t0
t0 = time.perf_counter()
dark_cube, dark_slp = ref.exposure(frames, 4, NFLIP, "dark")
dark_s = time.perf_counter() - t0


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return bool(np.array_equal(a.view(np.uint32 if a.dtype == np.float32 else a.dtype), b.view(np.uint32 if b.dtype == np.float32 else b.dtype)))


# (the flat's slopes come from its first 10 frames, so the 56-frame cube of sca 3 gives the same images)
say(f"  (d) numpy restatement, one core: 11 frames (flat, sca 3, Nc = 10) {flat_s:.1f} s, {N} frames (dark, sca 4, Nc = {N}) {dark_s:.1f} s; "
    f"same bits as the device: cube {same(flat_cube, cube3)} / {same(dark_cube, cube4)}, slopes {same(flat_slp, results[(3, 10)])} / "
    f"{same(dark_slp, results[(4, N)])}")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
