"""Time of the quick-look percentiles (csrc/view.hip, utils/visualize.py) at production size: a (16, 4096, 4096) uint16 cube
resident in HBM, the whole frame as the window.  A record, not a gate.

  (a) block_percentiles(cube, frame, [2, 98]): one rip_view_ranks call of four ranks, wall clock around the synchronous call (three
      passes over the 0.54 GB cube, their scans and the download of the result); the bytes the three passes read over that time
  (b) the same of the last group minus group 1 (two planes read per sample)
  (c) np.percentile of the same values on the host, once for each q as the reference calls it, after the download and the cast
      to float32 (both timed apart); the device's results must equal it bit for bit
  (d) visualize_cube of a 512 x 512 window of the 16 groups: five percentile calls and the render of the picture
"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime for both)

from romanimpreprocess_amd import _native  # noqa: E402
from romanimpreprocess_amd.devarray import DevArray  # noqa: E402
from romanimpreprocess_amd.utils import visualize  # noqa: E402

NG, N, CALLS, WARM = 16, 4096, 7, 2
ctx = _native.default_context(0)
gen = torch.Generator(device="cuda").manual_seed(91)
ramp = torch.randint(900, 1100, (1, N, N), generator=gen, device="cuda", dtype=torch.int32) \
    + torch.arange(NG, device="cuda", dtype=torch.int32)[:, None, None] * torch.randint(0, 3000, (1, N, N), generator=gen, device="cuda", dtype=torch.int32)
cube = DevArray(ramp.to(torch.int16).contiguous(), np.uint16).sync()   # the low 16 bits of values below 2^16: the uint16 samples
del ramp
frame = (0, N - 1, 0, N - 1)


def wall(fn, calls=CALLS, warm=WARM):
    out, last = [], None
    for i in range(warm + calls):
        t0 = time.perf_counter()
        last = fn()
        if i >= warm:
            out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), float(np.min(out)), last


print(f"quick-look percentiles, ({NG}, {N}, {N}) uint16 in HBM ({torch.cuda.get_device_name(0)}); wall clock around synchronous calls, median "
      f"(minimum) of {CALLS} after {WARM}:")
nbytes = 3 * cube.size * 2
med, mn, all_q = wall(lambda: visualize.block_percentiles(cube, frame, [2.0, 98.0], ctx=ctx))
print(f"  (a) 2nd and 98th percentile of all {cube.size / 1e6:.0f} M samples: {med:8.2f} ms ({mn:.2f}); three passes read {nbytes / 1e9:.2f} GB -> "
      f"{nbytes / med / 1e9:.2f} TB/s over the whole call")
med, mn, last_q = wall(lambda: visualize.block_percentiles(cube, frame, 98.0, planes=(NG - 1, NG), minus=1, ctx=ctx))
print(f"  (b) 98th percentile of group {NG - 1} minus group 1 ({N * N / 1e6:.0f} M samples):   {med:8.2f} ms ({mn:.2f})")
t0 = time.perf_counter()
host = cube.numpy()
t1 = time.perf_counter()
data = host.astype(np.float32)
t2 = time.perf_counter()
want = [np.percentile(data, 2.0), np.percentile(data, 98.0)]
t3 = time.perf_counter()
want_last = np.percentile(data[-1] - data[1], 98.0)
print(f"  (c) on the host: download {t1 - t0:.2f} s, astype(float32) {t2 - t1:.2f} s, np.percentile twice {t3 - t2:.2f} s; the device's results "
      f"equal numpy's bit for bit: {bool(all_q[0].tobytes() == want[0].tobytes() and all_q[1].tobytes() == want[1].tobytes())}, "
      f"of the difference: {bool(last_q.tobytes() == want_last.tobytes())}")
del data, host
med, mn, (pic, _) = wall(lambda: visualize.visualize_cube(cube, (1000, 1511, 2000, 2511), ctx=ctx), calls=5)
print(f"  (d) visualize_cube of a 512 x 512 window, picture {pic.shape}: {med:8.2f} ms ({mn:.2f})")
