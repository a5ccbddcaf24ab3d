"""Time of the gain / ipc4d expansion (csrc/gainfile.hip) at production size: 4096 x 4096 frame, 32 x 32 superpixels, border 4,
the (3,3,4088,4088) kernel as float64 (1.20 GB) and as float32 (0.60 GB), resident in HBM.

  (a) rip_cal_gain_ipc4d writing the kernel alone, between two events on the library's stream: the upload of the tables (20 KB),
      the one launch and nothing else; 25 calls after 3 of warm-up, median and minimum
  (b) the same call with all four outputs (gain, its flags, the kernel, its flags)
  (c) a plain device fill of the kernel's bytes in the same process (torch's fill_ and zero_ on the same tensor), same events:
      the store bound on this box
  (d) tests/gainfile_ref.py (numpy, one core) for the whole frame, once: what the drop-in replaces; same bits on 16 rows
GAINFILE_TIMING_KERNEL_ONLY=1: 5 calls of (a) per dtype and nothing else, for `rocprofv3 --kernel-trace --stats -- python <this file>`.
"""
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")
REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime for both)
import gainfile_ref as ref  # noqa: E402

from romanimpreprocess_amd import _native, calfiles  # noqa: E402

N, NS, NB, CALLS, WARM = 4096, 32, 4, 25, 3
NA = N - 2 * NB
kernel_only = os.environ.get("GAINFILE_TIMING_KERNEL_ONLY") == "1"
ctx = _native.default_context(0)
lib_stream = torch.cuda.ExternalStream(ctx.lib.rip_stream(ctx.h))
rng = np.random.default_rng(77)
u = rng.random((4, NS, NS))
means = {"g": 1.4 + 0.3 * u[0], "aH": 0.012 + 0.006 * u[1], "aV": 0.015 + 0.007 * u[2], "aD": 0.0011 + 0.0009 * u[3]}
good = np.ones((NS, NS), bool)
good[17, 5] = False


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


def derive(dtype, outputs):
    return calfiles.derive_gain_ipc4d(means, good, shape=(N, N), nb=NB, ipc_dtype=dtype, on_device=True, ctx=ctx, outputs=outputs)


if kernel_only:
    for dtype in (np.float64, np.float32):
        for _ in range(5):
            derive(dtype, ("kernel",))
    sys.exit(0)

print(f"gain / ipc4d expansion {N}x{N}, {NS}x{NS} superpixels, border {NB} ({torch.cuda.get_device_name(0)}); device times between events, "
      f"median (minimum) of {CALLS} calls after {WARM}:")
for dtype in (np.float64, np.float32):
    nbytes = 9 * NA * NA * np.dtype(dtype).itemsize
    # torch allocates anew in every call; the allocator hands the same block back, so the timed calls allocate nothing
    k_med, k_min = timed(lambda: derive(dtype, ("kernel",)), lib_stream)
    all_med, all_min = timed(lambda: derive(dtype, calfiles.GAIN_OUTPUTS), lib_stream)
    extra = 2 * N * N * 4 + NA * NA * 4
    t = torch.empty((3, 3, NA, NA), dtype=torch.float64 if dtype is np.float64 else torch.float32, device="cuda")
    cur = torch.cuda.current_stream()
    f_med, f_min = timed(lambda: t.fill_(1.0), cur)
    z_med, z_min = timed(lambda: t.zero_(), cur)
    del t
    name = np.dtype(dtype).name
    print(f"  {name}: (a) kernel alone        {k_med:7.3f} ms ({k_min:.3f}); {nbytes / 1e9:.3f} GB stored -> {nbytes / k_med / 1e9:.2f} TB/s "
          f"({nbytes / k_min / 1e9:.2f} at the minimum)")
    print(f"  {name}: (b) all four outputs    {all_med:7.3f} ms ({all_min:.3f}); {(nbytes + extra) / 1e9:.3f} GB stored -> "
          f"{(nbytes + extra) / all_med / 1e9:.2f} TB/s")
    print(f"  {name}: (c) plain fill_ / zero_ {f_med:7.3f} ms ({f_min:.3f}) / {z_med:.3f} ms ({z_min:.3f}) -> {nbytes / f_med / 1e9:.2f} / "
          f"{nbytes / z_med / 1e9:.2f} TB/s; (a) is x{k_med / f_med:.2f} of the fill_, x{k_med / z_med:.2f} of the zero_")

# (d) the numpy restatement on one core, whole frame, once
t0 = time.perf_counter()
gain, dq, K, kdq = ref.derive(means, good, (N, N), nb=NB)
d_s = time.perf_counter() - t0
rows = np.r_[0:4, 120:128, NA - 4:NA]
got = derive(np.float64, ("kernel",))[2]
same = np.array_equal(got.t[:, :, torch.as_tensor(rows, device="cuda")].cpu().numpy().view(np.uint64), K[:, :, rows].view(np.uint64))
print(f"  (d) numpy restatement of all four outputs, one core, whole frame: {d_s:.1f} s; same bits as the device on {rows.size} rows: {same}")
