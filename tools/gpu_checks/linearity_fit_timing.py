"""Time of the linearitylegendre derivation (csrc/linfit.hip) at production size: a 4096 x 4096 frame, the bright flat, low flat
and dark of 56 + 12 + 56 frames (TSTART 3), order 8.  Recorded only: the feature is new and nothing is compared with a parent.

  (a) one rip_cal_linearity_fit launch, sums resident in HBM: warm-up, then 30 calls, each timed with the steady clock around the
      synchronous entry (median, min, max); the share of flagged pixels
  (b) one rip_cal_frame_sums call on a resident 56-frame cube of 4224-wide frames (4096 columns used), 30 calls, against
      hipMemcpyDtoD of the cube's bytes in the same process, 30 calls
LINFIT_TIMING_ORDER=<p> times another order.
"""
import ctypes
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime for both)

from romanimpreprocess_amd import _native, calfiles  # noqa: E402
from romanimpreprocess_amd.devarray import DevArray  # noqa: E402

N, WIDTH, REPS = 4096, 4224, 30
SETS = ((420.0, 56, 50), (60.0, 12, 30), (0.3, 56, 30))   # rate in DN_lin/s, frames, exposures
TFRAME, TSTART = 3.15625, 3
order = int(os.environ.get("LINFIT_TIMING_ORDER", "8"))
ctx = _native.default_context(0)
gen = torch.Generator(device="cuda").manual_seed(7)
sref = 5000 + 600 * torch.rand((N, N), device="cuda", generator=gen)
qe = 0.8 + 0.4 * torch.rand((N, N), device="cuda", generator=gen)
sat = 52000 + 12000 * torch.rand((N, N), device="cuda", generator=gen)
curve = 1.5e-6 + 1.0e-6 * torch.rand((N, N), device="cuda", generator=gen)


def stats(ms):
    return f"median {np.median(ms):8.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}, {len(ms)} calls)"


stacks = []
for rate, nf, nexp in SETS:
    sums = torch.empty((nf, N, N), dtype=torch.int32, device="cuda")
    for i in range(nf):
        lin = 100.0 + rate * qe * TFRAME * (i + 2)
        s = torch.minimum(sref + lin - curve * lin * lin, sat).clamp_(0, 65535)
        sums[i] = (s * nexp).round_().to(torch.int32)   # below 2^31: 65535 x 50
    stacks.append((DevArray(sums, np.uint32), nexp))
torch.cuda.synchronize()


def fit():
    return calfiles.derive_linearity(stacks, DevArray(sref), p_order=order, tframe=TFRAME, tstart=TSTART, dark=-1, ctx=ctx)


out = fit()
fit()
fit_ms = []
for _ in range(REPS):
    t0 = time.perf_counter()
    out = fit()   # allocates its result planes as well: torch's caching allocator, no hipMalloc after the warm-up
    fit_ms.append(1e3 * (time.perf_counter() - t0))
flagged = float((out["dq"].t[4:-4, 4:-4] != 0).float().mean())
nsamples = sum(nf - (TSTART - 1) for _, nf, _ in SETS)
sums_gb = sum(nf for _, nf, _ in SETS) * N * N * 4 / 1e9
print(f"linearity fit {N}x{N}, {'+'.join(str(nf) for _, nf, _ in SETS)} frames, order {order} ({torch.cuda.get_device_name(0)}):")
print(f"  (a) derive_linearity, sums resident:   {stats(fit_ms)}; {nsamples} samples per pixel, {sums_gb:.2f} GB of sums, "
      f"{100 * flagged:.2f} % of the science pixels flagged")
del out

# (b) frame sums against a device-to-device copy of the same bytes
nf = SETS[0][1]
cube = torch.randint(-32768, 32767, (nf, N, WIDTH), dtype=torch.int16, device="cuda", generator=gen)
stack = calfiles.RampStack(nf, N, N, ctx=ctx)
torch.cuda.synchronize()
stack.add(DevArray(cube, np.uint16))
sum_ms = []
for _ in range(REPS):
    t0 = time.perf_counter()
    stack.add(DevArray(cube, np.uint16))
    sum_ms.append(1e3 * (time.perf_counter() - t0))
same = bool((stack.sums.t == (cube[:, :, :N].to(torch.int32) & 0xFFFF) * stack.count).all())
hip = None
with open("/proc/self/maps") as f:   # the HIP runtime this process has loaded already (PyTorch's own copy)
    for line in f:
        if "libamdhip64" in line:
            hip = ctypes.CDLL(line.split()[-1])
            break
dst = torch.empty_like(cube)
nbytes = cube.numel() * 2
copy_ms = []
if hip is not None:
    hip.hipMemcpyDtoD.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    hip.hipMemcpyDtoD.restype = ctypes.c_int
    for j in range(REPS + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = hip.hipMemcpyDtoD(dst.data_ptr(), cube.data_ptr(), nbytes)
        torch.cuda.synchronize()
        if rc != 0:
            raise RuntimeError(f"hipMemcpyDtoD: {rc}")
        if j >= 2:
            copy_ms.append(1e3 * (time.perf_counter() - t0))
used_gb = (nf * N * N * 2 + 2 * nf * N * N * 4) / 1e9
print(f"  (b) frame sums of a resident {nf}-frame cube ({nbytes / 1e9:.2f} GB, {N} of {WIDTH} columns): {stats(sum_ms)}; "
      f"{used_gb:.2f} GB of samples read and sums read and written -> {used_gb / (np.median(sum_ms) / 1e3):.0f} GB/s; sums exact: {same}")
if copy_ms:
    print(f"      hipMemcpyDtoD of the cube's {nbytes / 1e9:.2f} GB: {stats(copy_ms)} -> {2 * nbytes / 1e9 / (np.median(copy_ms) / 1e3):.0f} GB/s "
          f"read + written; frame sums take {np.median(sum_ms) / np.median(copy_ms):.2f} of that time")
else:
    print("      hipMemcpyDtoD: the loaded HIP runtime was not found")
