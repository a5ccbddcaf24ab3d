"""Time of the pixel-area map of a 4096 x 4096 frame (rip_stage_pixel_area, csrc/post.hip) on the device, against the numpy
restatement (tests/wcs_area_ref.py) on one CPU core.  The WCS is the TAN-SIP header of the reference's workflow test.

Device: 50 calls writing to device memory queued back to back on the library's stream, wall time / 50 (the kernel dominates:
one launch per call, no copies); plus one call with the host download (134 MB over PCIe).  Kernel-only numbers:
rocprofv3 --kernel-trace --stats -- python tools/gpu_checks/pixel_area_timing.py"""
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")
REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402, F401  (before the library: one HIP runtime for both)
import wcs_area_ref as ref  # noqa: E402

from romanimpreprocess_amd import _native, calio, pars  # noqa: E402
from romanimpreprocess_amd.utils import coordutils  # noqa: E402

N = pars.nside
w = coordutils.FitsWCS(calio.parse_fits_header(ref.header_text(ref.WORKFLOW_CARDS)))
ctx = _native.default_context(0)
d = w.desc()
out = torch.empty((N, N), dtype=torch.float64, device=torch.device("cuda", ctx.device))
torch.cuda.synchronize()
for _ in range(3):   # warm-up (code object load, clocks)
    ctx.check(ctx.lib.rip_stage_pixel_area(ctx.h, d, N, N, pars.Omega_ideal, _native.RIP_DEVICE, out.data_ptr()))
ctx.synchronize()
reps = 50
t0 = time.perf_counter()
for _ in range(reps):
    ctx.check(ctx.lib.rip_stage_pixel_area(ctx.h, d, N, N, pars.Omega_ideal, _native.RIP_DEVICE, out.data_ptr()))
ctx.synchronize()
dev_ms = 1e3 * (time.perf_counter() - t0) / reps
t0 = time.perf_counter()
host = coordutils.pixelarea_map(w, N, N, scale=pars.Omega_ideal, ctx=ctx)
host_ms = 1e3 * (time.perf_counter() - t0)
assert np.array_equal(host, out.cpu().numpy())
t0 = time.perf_counter()
cpu = ref.pixel_area(w, N, N, scale=pars.Omega_ideal)
cpu_ms = 1e3 * (time.perf_counter() - t0)
print(f"pixel-area map {N}x{N} ({(N + 2) ** 2 / 1e6:.1f} M WCS evaluations + halo recompute):")
print(f"  device, {reps} calls back to back: {dev_ms:.3f} ms per map")
print(f"  one call with the host download:    {host_ms:.1f} ms")
print(f"  numpy restatement, one CPU core:    {cpu_ms:.0f} ms  (x{cpu_ms / dev_ms:.0f})")
print(f"  max relative difference device vs numpy: {np.max(np.abs(host / cpu - 1.0)):.2e}; AreaFactor {host.min():.4f} .. {host.max():.4f}")
