"""Times of the noise-summary kernels (csrc/noisestat.hip) on one production exposure: a 36-frame cube of 4096 x 4224 samples (1.25
GB), 32 channels of 128 and the reference output, the job's -t 3 -tn 34.

  (a) rip_cal_noise_add on the cube resident in HBM, between two events on the library's stream; 5 calls after 1, median (minimum)
  (b) the same call on the cube in page-locked host memory: the 34 frames used travel first (1.18 GB)
  (c) rip_cal_noise_rowstats of that exposure's row sums
  (d) rip_cal_noise_planes
  (e) rip_cal_group_means of the same resident cube with the production table's 10 groups, for comparison: the pass that
      make_dark_file makes over the same samples
The kernel of (a) reads 2 n bytes per pixel and reads and writes 52 (56) bytes of accumulators: 2 n + 112.
"""
import os
import sys

os.environ.setdefault("OMP_NUM_THREADS", "1")
REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime for both)

from romanimpreprocess_amd import _native  # noqa: E402
from romanimpreprocess_amd.calfiles import DarkStack, NoiseStack  # noqa: E402
from romanimpreprocess_amd.devarray import DevArray  # noqa: E402

NY, WIDTH, NREADS, C, CW, F0, N = 4096, 4224, 36, 32, 128, 2, 34
CALLS, WARM = 5, 1
READS = [0, 1, 1, 2, 2, 4, 4, 8, 8, 12, 12, 16, 16, 20, 20, 24, 24, 30, 30, 36]
ctx = _native.default_context(0)
stream = torch.cuda.ExternalStream(ctx.lib.rip_stream(ctx.h))


def timed(fn, calls=CALLS, warm=WARM):
    """median and minimum, in ms, of the device time between two events on the library's stream around fn()"""
    ms = []
    for i in range(warm + calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        if i >= warm:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


gen = torch.Generator(device="cuda").manual_seed(5)
cube = DevArray((8000 + 40 * torch.randn((NREADS, NY, WIDTH), generator=gen, device="cuda")).round().to(torch.int32).to(torch.int16),
                np.uint16)
torch.cuda.synchronize()
stack = NoiseStack(NY, WIDTH, C, CW, F0, N, True, ctx=ctx)
a, t = stack.acc, stack.tables


def add(c):
    # count stays 0: the timed calls add the same exposure again and again, which the integer sums do not mind
    ctx.call("rip_cal_noise_add", c, _native.location_of(c), NREADS, NY, WIDTH, C, CW, True, F0, N, False, 0, a["a0"], a["a1"], a["b0"],
             a["b1"], a["s0"], a["s1"], a["c0"], a["c1"], a["m33"], stack.rowsum)


def rowstats():
    ctx.call("rip_cal_noise_rowstats", stack.rowsum, N, NY, C, True, t["h1"], t["h2"], t["t1"], t["t2"], t["ht"], t["q1"], t["q2"])


print(f"noise summary, one exposure {NREADS} x {NY} x {WIDTH}, -t {F0 + 1} -tn {N}, {C} channels of {CW} + reference output "
      f"({torch.cuda.get_device_name(0)}); device times between events, median (minimum) of {CALLS} calls after {WARM}:")
npix = NY * (C + 1) * CW
moved = npix * (2 * N + 104) + NY * CW * 8
med, mn = timed(lambda: add(cube))
print(f"  (a) rip_cal_noise_add, resident cube   {med:8.3f} ms ({mn:.3f}); {moved / 1e9:.3f} GB moved -> {moved / med / 1e9:.2f} TB/s")
host = ctx.pinned_empty((NREADS, NY, WIDTH), np.uint16)
host[...] = cube.numpy()
med, mn = timed(lambda: add(host), calls=3)
print(f"  (b) rip_cal_noise_add, page-locked host cube {med:8.3f} ms ({mn:.3f}); {N * NY * WIDTH * 2 / 1e9:.3f} GB over the link -> "
      f"{N * NY * WIDTH * 2 / med / 1e6:.1f} GB/s")
del host
med, mn = timed(rowstats)
print(f"  (c) rip_cal_noise_rowstats             {med:8.3f} ms ({mn:.3f})")
stack.count = 2
med, mn = timed(lambda: stack.finish())
print(f"  (d) NoiseStack.finish: rip_cal_noise_planes, tables and CDS plane to the host, noise_params {med:8.3f} ms ({mn:.3f})")
planes = torch.empty((6, NY, C * CW), dtype=torch.float32, device="cuda")
amp33 = torch.empty((2, NY, CW), dtype=torch.float32, device="cuda")
med, mn = timed(lambda: ctx.call("rip_cal_noise_planes", a["a0"], a["a1"], a["b0"], a["b1"], a["s0"], a["s1"], a["c0"], a["c1"], a["m33"],
                                 2, N, NY, C, CW, True, 3.04, _native.RIP_DEVICE, planes, amp33))
print(f"      rip_cal_noise_planes alone         {med:8.3f} ms ({mn:.3f}); {(npix * 52 + NY * C * CW * 24) / 1e9:.3f} GB moved")
del planes, amp33, stack
ds = DarkStack(READS, NY, 4096, 1, ctx=ctx)


def means():
    ds.n = 0
    ds.add(cube)


med, mn = timed(means)
print(f"  (e) rip_cal_group_means, same cube, {len(READS) // 2} groups {med:8.3f} ms ({mn:.3f}); "
      f"{(NREADS * NY * WIDTH * 2 + len(READS) // 2 * NY * 4096 * 4) / 1e9:.3f} GB moved")
