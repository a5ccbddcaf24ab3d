"""Time of the focal-plane overview (csrc/fpaplot.hip, utils/fpaplot.py) at production size: 18 SCAs x 8 planes of 4096 x 4096
(the three ipc4d planes 4088 x 4088), n1 = 128, PixelMask1 on a dq with 5 % of the pixels flagged.  A record, not a gate.

  (a) rip_fpa_bin of one SCA from planes resident in HBM, between two events on the library's stream: the one launch; the bytes it
      reads (dq + 8 planes) divided by the time
  (b) the same call from host (numpy) arrays, wall clock: the uploads of 0.6 GB are in it
  (c) rip_fpa_render of the 8-panel picture from resident means, into HBM (events) and into a host array (wall clock)
  (d) multi_image end to end from files, wall clock: the 7 files of one SCA are written once and linked under the names of the
      other 17, so every SCA is read (from the page cache) and binned
FPAPLOT_TIMING_KERNEL_ONLY=1: 5 calls of (a) and of (c) and nothing else, for `rocprofv3 --kernel-trace --stats -- python <this file>`.
"""
import os
import sys
import tempfile
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")
REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime for both)
import fpaplot_ref as fr  # noqa: E402

from romanimpreprocess_amd import _native, calio  # noqa: E402
from romanimpreprocess_amd.devarray import DevArray, to_device  # noqa: E402
from romanimpreprocess_amd.utils import fpaplot  # noqa: E402
from romanimpreprocess_amd.utils.maskhandling import PixelMask1  # noqa: E402

N, NA, N1, CALLS, WARM = 4096, 4088, 128, 15, 3
kernel_only = os.environ.get("FPAPLOT_TIMING_KERNEL_ONLY") == "1"
ctx = _native.default_context(0)
lib_stream = torch.cuda.ExternalStream(ctx.lib.rip_stream(ctx.h))
rng = np.random.default_rng(78)


def field(side, lo, hi):
    return (lo + (hi - lo) * rng.random((side, side), dtype=np.float32))


ptypes = [p[0] for p in fpaplot.PANELS]
host = {p: field(NA if p.startswith("alpha") else N, lo, hi) for p, lo, hi, _ in fpaplot.PANELS}
dq = fr.random_dq(rng, N)
dev = {p: to_device(a) for p, a in host.items()}
ddq = to_device(dq)
nbytes = dq.nbytes + sum(a.nbytes for a in host.values())


def timed(fn, stream, calls=CALLS, warm=WARM):
    """median and minimum, in ms, of the device time between two events on `stream` around fn()"""
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


def wall(fn, calls=3):
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), float(np.min(out))


out = DevArray(torch.empty((8, N1, N1), dtype=torch.float64, device="cuda")).sync()
ny, nx, pos = fpaplot.panel_layout(N1)
maps = DevArray(torch.rand((8, 18, N1, N1), dtype=torch.float64, device="cuda")).sync()
present = np.ones((8, 18), np.uint8)
stamps = [s for j, (p, lo, hi, f) in enumerate(fpaplot.PANELS) for s in fpaplot.scale_stamps(j, N1, ny, nx, p, lo, hi, f)]
glyphs = (rng.random((256, 12, 6)) < 0.4).astype(np.uint8)   # any glyph table costs the same
pic = DevArray(torch.empty((4 * ny + 3 * (1 + N1 // 4), 2 * nx + 1 + N1 // 4, 3), dtype=torch.uint8, device="cuda")).sync()


def bin_resident():
    fpaplot.bin_planes(ddq, [dev[p] for p in ptypes], N, N1, mask=PixelMask1, ctx=ctx, out=out)


def render(to):
    return fpaplot.render(maps, present, 0.0, 1.0, True, N1, ny, nx, pos, font=glyphs, stamps=stamps, ctx=ctx, out=to)


if kernel_only:
    for _ in range(5):
        bin_resident()
        render(pic)
    sys.exit(0)

print(f"focal-plane overview, {N}x{N} frames, n1 {N1}, 8 planes an SCA ({torch.cuda.get_device_name(0)}); device times between events on the "
      f"library's stream, median (minimum) of {CALLS} calls after {WARM}; wall-clock times median (minimum) of 3:")
med, mn = timed(bin_resident, lib_stream)
print(f"  (a) rip_fpa_bin, one SCA, resident planes: {med:8.3f} ms ({mn:.3f}); {nbytes / 1e9:.3f} GB read -> {nbytes / med / 1e9:.2f} TB/s "
      f"({nbytes / mn / 1e9:.2f} at the minimum); 18 SCAs: {18 * med:.1f} ms")
want, bound = fr.bin_ref(dq[:256, :256], fr.PIXELMASK1, [host["gain"][:256, :256]], 256, 8)
part = fpaplot.bin_planes(dq[:256, :256].copy(), [host["gain"][:256, :256].copy()], 256, 8, mask=PixelMask1, ctx=ctx).numpy()
print(f"      a 256 x 256 corner against the numpy restatement: within the derived bound: {bool((np.abs(part - want) <= bound).all())}")
med, mn = wall(lambda: fpaplot.bin_planes(dq, [host[p] for p in ptypes], N, N1, mask=PixelMask1, ctx=ctx, out=out))
print(f"  (b) the same from host arrays, wall clock:  {med:8.1f} ms ({mn:.1f}); {nbytes / med / 1e6:.1f} GB/s of uploads and launch")
med, mn = timed(lambda: render(pic), lib_stream)
print(f"  (c) rip_fpa_render, {pic.shape[0]} x {pic.shape[1]} picture into HBM: {med:8.3f} ms ({mn:.3f}); {pic.size / 1e6:.2f} MB stored, "
      f"{maps.size * 8 / 1e6:.2f} MB of means read -> {(pic.size + maps.size * 8) / med / 1e6:.1f} GB/s")
med, mn = wall(lambda: render(None))
print(f"      the same into a host array, wall clock: {med:8.3f} ms ({mn:.3f})")

with tempfile.TemporaryDirectory(prefix="fpaplot_timing_") as tmp:
    fmt = os.path.join(tmp, "roman_wfi_{:s}_TIMING_SCA{:02d}.asdf")
    lin = np.zeros((4, N, N), np.float32)
    lin[2], lin[3] = host["lin2"], host["lin3"]
    ipc = np.zeros((3, 3, NA, NA), np.float32)
    ipc[1, 0], ipc[0, 1], ipc[0, 0] = host["alphaH"], host["alphaV"], host["alphaD"]
    files = {"linearitylegendre": {"data": lin}, "ipc4d": {"data": ipc}, "gain": {"data": host["gain"]}, "pflat": {"data": host["pflatnorm"]},
             "read": {"data": host["read"]}, "mask": {"dq": dq}}
    size = 0
    for name, roman in files.items():
        calio.write_asdf(fmt.format(name, 1), {"roman": roman})
        size += os.path.getsize(fmt.format(name, 1))
        for k in range(2, 19):
            os.symlink(fmt.format(name, 1), fmt.format(name, k))
    del lin, ipc, files
    t = []
    for _ in range(2):
        t0 = time.perf_counter()
        arr = fpaplot.multi_image(fmt, N1, PixelMask1, font=glyphs, ctx=ctx)
        t.append(time.perf_counter() - t0)
    print(f"  (d) multi_image from files, 18 SCAs of {size / 1e9:.2f} GB in 6 files each (whole files are read: {18 * size / 1e9:.1f} GB; "
          f"{18 * nbytes / 1e9:.1f} GB go to the device), picture {arr.shape}: {t[0]:.1f} s, then {t[1]:.1f} s")
print("  context: profiles/r04_stream_bound.txt measured 4.73 TB/s for the streams of the fused chain on this kind of device; no threshold is set here.")
