"""Times of the pair statistics (csrc/corrstat.hip) on one production pair: two cubes of 16 frames of 4096 x 4224 samples (277 MB
each), TIME 2 8 9 15, the [:4096] crop, NBIN 32 32 (1024 superpixels of 128 x 128), border 4.

  (a) rip_cal_corr_pair on the pair resident in HBM, the table in HBM, between two events on the library's stream; 5 calls after
      1, median (minimum)
  (b) a device-to-device copy (hipMemcpyAsync by way of torch's copy_ of a contiguous tensor, on the same stream) of as many bytes
      as the kernel reads: 8 frames of 4096 x 4096 samples, 268 MB
  (c) the call of (a) with the table in host memory (200 KB come back)
  (d) the call on two cubes in page-locked host memory: the rows of the 8 frames used travel first (8 x 4096 x 4224 samples, 277 MB)
  (e) the call of (a) on a pair with one pixel in a thousand hot: the samples of a rejected pixel are read a second time
The kernel reads 16 bytes per pixel and writes 200 bytes per superpixel.
"""
import os
import sys

os.environ.setdefault("OMP_NUM_THREADS", "1")
REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime for both)

from romanimpreprocess_amd import _native  # noqa: E402
from romanimpreprocess_amd.devarray import DevArray  # noqa: E402

NREADS, NY, WIDTH, NSIDE, NB, S = 16, 4096, 4224, 4096, 4, 128
FRAMES = (1, 7, 8, 14)
CALLS, WARM = 5, 1
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


def flat(seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    ramp = 6000 + 330 * torch.arange(NREADS, device="cuda", dtype=torch.float32)[:, None, None]
    return (ramp + 45 * torch.randn((NREADS, NY, WIDTH), generator=gen, device="cuda")).round().to(torch.int32).to(torch.int16)


def pair(c1, c2, table):
    ctx.call("rip_cal_corr_pair", c1, _native.location_of(c1), c2, _native.location_of(c2), NREADS, NY, WIDTH, False, *FRAMES, NSIDE, NSIDE, NB,
             S, S, table, _native.location_of(table))


t1, t2 = flat(5), flat(6)
c1, c2 = DevArray(t1, np.uint16), DevArray(t2, np.uint16)
torch.cuda.synchronize()
dtab = DevArray(torch.zeros((NSIDE // S, NSIDE // S, 25), dtype=torch.int64, device="cuda"), np.int64)
htab = np.zeros((NSIDE // S, NSIDE // S, 25), np.int64)
read = 8 * NSIDE * NSIDE * 2
print(f"pair statistics, two cubes {NREADS} x {NY} x {WIDTH}, TIME {' '.join(str(f + 1) for f in FRAMES)}, frame {NSIDE} x {NSIDE}, "
      f"superpixels {S} x {S}, border {NB} ({torch.cuda.get_device_name(0)}); device times between events, median (minimum) of "
      f"{CALLS} calls after {WARM}:")
med, mn = timed(lambda: pair(c1, c2, dtab))
print(f"  (a) rip_cal_corr_pair, resident pair, table in HBM   {med:8.3f} ms ({mn:.3f}); {read / 1e6:.0f} MB read -> {read / med / 1e9:.2f} TB/s")
kept = dtab.numpy()[..., 0]
print(f"      kept pixels per superpixel: {kept.min()} .. {kept.max()} of {S * S}")
src = torch.empty(read // 2, dtype=torch.int16, device="cuda")
dst = torch.empty_like(src)
torch.cuda.synchronize()


def copy():
    with torch.cuda.stream(stream):
        dst.copy_(src)


med, mn = timed(copy)
print(f"  (b) device-to-device copy of {read / 1e6:.0f} MB               {med:8.3f} ms ({mn:.3f}); read + write -> {2 * read / med / 1e9:.2f} TB/s")
del src, dst
med, mn = timed(lambda: pair(c1, c2, htab))
print(f"  (c) as (a), table in host memory                     {med:8.3f} ms ({mn:.3f})")
assert np.array_equal(htab, dtab.numpy())
h1, h2 = ctx.pinned_empty((NREADS, NY, WIDTH), np.uint16), ctx.pinned_empty((NREADS, NY, WIDTH), np.uint16)
h1[...] = c1.numpy()
h2[...] = c2.numpy()
link = 8 * NY * WIDTH * 2
med, mn = timed(lambda: pair(h1, h2, htab), calls=3)
print(f"  (d) page-locked host cubes                           {med:8.3f} ms ({mn:.3f}); {link / 1e6:.0f} MB over the link -> "
      f"{link / med / 1e6:.1f} GB/s")
assert np.array_equal(htab, dtab.numpy())
del h1, h2
gen = torch.Generator(device="cuda").manual_seed(7)
hot = torch.rand((NY, WIDTH), generator=gen, device="cuda") < 1e-3
t1[FRAMES[3]] += (hot * 4000).to(torch.int16)
torch.cuda.synchronize()
med, mn = timed(lambda: pair(c1, c2, dtab))
kept = dtab.numpy()[..., 0]
print(f"  (e) as (a), one pixel in a thousand hot              {med:8.3f} ms ({mn:.3f}); kept {kept.min()} .. {kept.max()}")
