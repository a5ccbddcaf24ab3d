"""Time of the dark-file arithmetic (csrc/darkstack.hip) at production size: 4096 x 4096 crop of 4224-wide frames, the production
8-group table (35 reads), 100 dark exposures.

  (a) DarkStack.add per exposure, cube resident in HBM (35 x 4096 x 4224 u16 = 1.21 GB read once, 8 planes of 4096^2 f32 written)
  (b) DarkStack.add per exposure from a host array in FITS storage (pageable memory: the cube crosses PCIe)
  (c) the clipped mean over the 100 exposures per group (rip_cal_sigma_clip_mean on 100 x 4096^2 f32 = 6.7 GB), and finish() for
      the 8 groups; how many values the clip removed
  (d) derive_dark_planes on 4096 x 4224 planes resident in HBM
  (e) tests/darkstack_ref.py (numpy, one core) on a strip of 8 rows, EXTRAPOLATED to 4096 rows: the group means of one exposure and
      the clip of one group
DARKSTACK_TIMING_KERNEL_ONLY=1: 3 resident adds and one finish, for `rocprofv3 --kernel-trace --stats -- python <this file>`.
"""
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")
REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime for both)
import darkstack_ref as ref  # noqa: E402

from romanimpreprocess_amd import _native, calfiles, synth  # noqa: E402
from romanimpreprocess_amd.devarray import DevArray  # noqa: E402

N, WIDTH, NEXP, ROWS = 4096, 4224, 100, 8
reads = calfiles.reads_of_pattern(synth.READ_PATTERN_8)
nreads, ng = reads[-1], len(reads) // 2
ctx = _native.default_context(0)
kernel_only = os.environ.get("DARKSTACK_TIMING_KERNEL_ONLY") == "1"
nexp = 3 if kernel_only else NEXP

gen = torch.Generator(device="cuda").manual_seed(5)
base = 1000 + 200 * torch.rand((N, WIDTH), device="cuda", generator=gen)
rate = 0.5 * torch.rand((N, WIDTH), device="cuda", generator=gen)
ramp = torch.arange(nreads, device="cuda", dtype=torch.float32)[:, None, None]


def exposure():
    """a dark-like cube on the device: pedestal, dark current, read noise of 6 DN, a step of up to 400 DN in 3 % of the pixels"""
    c = base + rate * ramp + 6 * torch.randn((nreads, N, WIDTH), device="cuda", generator=gen)
    hit = torch.rand((N, WIDTH), device="cuda", generator=gen) < 0.03
    c[nreads // 2:] += torch.where(hit, 400 * torch.rand((N, WIDTH), device="cuda", generator=gen), 0.0)
    return DevArray(c.round_().clamp_(0, 65535).to(torch.int32).to(torch.int16), np.uint16)   # the low 16 bits: uint16 samples


stack = calfiles.DarkStack(reads, N, N, nexp, ctx=ctx)
add_ms = []
first = None
for j in range(nexp):
    cube = exposure()
    torch.cuda.synchronize()
    if first is None:
        first = cube.numpy()
    t0 = time.perf_counter()
    stack.add(cube)
    add_ms.append(1e3 * (time.perf_counter() - t0))
    del cube
a_ms = float(np.mean(add_ms[1:]))

t0 = time.perf_counter()
dark = stack.finish(want_count=True)
finish_ms = 1e3 * (time.perf_counter() - t0)
if kernel_only:
    sys.exit(0)
mean, count = dark[0].numpy(), dark[1].numpy()
clip_ms = []
for g in range(ng):
    t0 = time.perf_counter()
    calfiles.sigma_clip_mean(DevArray(stack.stack.t[g]), ctx=ctx)
    clip_ms.append(1e3 * (time.perf_counter() - t0))

# (b) a host array in FITS storage, through a stack of its own
be = ref.to_fits_be16(first)
host_stack = calfiles.DarkStack(reads, N, N, 3, ctx=ctx)
host_ms = []
for _ in range(3):
    t0 = time.perf_counter()
    host_stack.add(be, fits_be16=True)
    host_ms.append(1e3 * (time.perf_counter() - t0))
same_add = np.array_equal(host_stack.stack.t[:, 0].cpu().numpy().view(np.uint32), stack.stack.t[:, 0].cpu().numpy().view(np.uint32))
del host_stack

# (d)
planes = [DevArray(300 * torch.rand((N, WIDTH), device="cuda", generator=gen)) for _ in range(5)]
torch.cuda.synchronize()
calfiles.derive_dark_planes(*planes, nside=N, ctx=ctx)
t0 = time.perf_counter()
for _ in range(10):
    calfiles.derive_dark_planes(*planes, nside=N, ctx=ctx)
d_ms = 1e3 * (time.perf_counter() - t0) / 10

# (e) numpy on a strip
y0 = 2000
t0 = time.perf_counter()
gm = ref.group_means(first[:, y0:y0 + ROWS], reads, N)
e_gm_ms = 1e3 * (time.perf_counter() - t0) * N / ROWS
same_gm = np.array_equal(gm.view(np.uint32), stack.stack.t[:, 0, y0:y0 + ROWS].cpu().numpy().view(np.uint32))
strip = stack.stack.t[4, :, y0:y0 + ROWS].cpu().numpy()
t0 = time.perf_counter()
rm, rc, border = ref.sigma_clip_mean(strip)
e_clip_ms = 1e3 * (time.perf_counter() - t0) * N / ROWS
ok = ~border
same_clip = np.array_equal(rc[ok], count[4, y0:y0 + ROWS][ok]) and np.array_equal(rm[ok].view(np.uint32),
                                                                                  mean[4, y0:y0 + ROWS][ok].view(np.uint32))

cube_gb = nreads * N * WIDTH * 2 / 1e9
kept = count.sum() / count.size
print(f"dark stack {N}x{N} of {WIDTH}-wide frames, {ng} groups / {nreads} reads, {NEXP} exposures ({torch.cuda.get_device_name(0)}):")
print(f"  (a) add, cube resident in HBM, mean of {NEXP - 1} calls:     {a_ms:9.2f} ms  ({min(add_ms[1:]):.2f} .. {max(add_ms[1:]):.2f}; first call "
      f"{add_ms[0]:.1f}); {cube_gb:.2f} GB in + {ng * N * N * 4 / 1e9:.2f} GB out -> {(cube_gb + ng * N * N * 4 / 1e9) / (a_ms / 1e3):.0f} GB/s")
print(f"  (b) add from a host array in FITS storage, 3 calls:   {host_ms[0]:9.1f} {host_ms[1]:.1f} {host_ms[2]:.1f} ms; same bits as (a): {same_add}")
print(f"  (c) clipped mean of {NEXP} planes, per group:            {np.mean(clip_ms):9.2f} ms  ({min(clip_ms):.2f} .. {max(clip_ms):.2f}); finish() of "
      f"{ng} groups with counts: {finish_ms:.1f} ms; kept {kept:.3f} of {NEXP} values per pixel on average")
print(f"  (d) derive_dark_planes, resident, mean of 10 calls:   {d_ms:9.2f} ms")
print(f"  (e) numpy restatement, one core, EXTRAPOLATED from {ROWS} rows: group means of one exposure {e_gm_ms / 1e3:.1f} s (x {NEXP} exposures), "
      f"clip of one group {e_clip_ms / 1e3:.0f} s (x {ng} groups); same bits on the strip: means {same_gm}, clip {same_clip} "
      f"({int(border.sum())} borderline pixels left out)")
total_gpu = NEXP * a_ms + finish_ms
total_np = NEXP * e_gm_ms + ng * e_clip_ms
print(f"  whole dark_data: {total_gpu / 1e3:.2f} s resident on the device against {total_np / 1e3:.0f} s of numpy on one core (extrapolated), "
      f"x{total_np / total_gpu:.0f}")
