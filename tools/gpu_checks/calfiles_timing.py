"""Time of the bias-correction derivation (rip_cal_biascorr, csrc/calfiles.hip) on a 4096 x 4096 set with the production 8-group
table (35 reads) and 9 Legendre planes, against what the library offered before it: one rip_stage_invlinearity call per read
with the accumulation of postprocess_calfiles.py:129-136 in numpy.

  (a) derive_biascorr, inputs and outputs resident in HBM: mean wall time of 20 calls after 3 warm-up calls (a call returns when
      its kernel is done; it includes the device-to-device staging copies of the entry point)
  (b) the same through host arrays (every plane crosses PCIe once in, the results once out)
  (c) the composition of 35 rip_stage_invlinearity calls, once
  (d) the kernel's algorithmic bytes: NP + 3 input planes, ngrp dark planes in, ngrp out
  (e) tests/calfiles_ref.py (numpy, one core) on a strip of 8 active rows, EXTRAPOLATED to 4088 rows
CALFILES_TIMING_KERNEL_ONLY=1: only the warm-up and 5 calls of (a), for `rocprofv3 --kernel-trace --stats -- python <this file>`.
"""
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")
REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime for both)
import calfiles_ref as ref  # noqa: E402

from romanimpreprocess_amd import _native, calfiles, pars, synth  # noqa: E402
from romanimpreprocess_amd.devarray import DevArray  # noqa: E402
from romanimpreprocess_amd.utils import ipc_linearity  # noqa: E402

N, NB = pars.nside, 4
rp = synth.READ_PATTERN_8
reads = calfiles.reads_of_pattern(rp)
cal = synth.make_caldir(N, N, read_pattern=rp, p_order=8, seed=7)
lin, dark = cal["linearitylegendre"], cal["dark"]
host = (dark["dark_slope"], dark["data"], lin["data"], lin["Smin"], lin["Smax"])
ctx = _native.default_context(0)
devs = tuple(DevArray(torch.from_numpy(np.ascontiguousarray(a)).cuda()) for a in host)
torch.cuda.synchronize()


def timed(args, reps, warm=3):
    for _ in range(warm):
        out = calfiles.derive_biascorr(*args, reads, want_pred=True, ctx=ctx)
    t0 = time.perf_counter()
    for _ in range(reps):
        out = calfiles.derive_biascorr(*args, reads, want_pred=True, ctx=ctx)
    return 1e3 * (time.perf_counter() - t0) / reps, out


if os.environ.get("CALFILES_TIMING_KERNEL_ONLY") == "1":
    timed(devs, 5)
    sys.exit(0)

a_ms, (dbc, t0_, dpred) = timed(devs, 20)
b_ms, (hbc, _, hpred) = timed(host, 20)
assert np.array_equal(dbc.numpy().view(np.uint32), hbc.view(np.uint32))

F = np.float32
t0 = time.perf_counter()
xref = calfiles.parse_reads(reads, 1)[2]
dk = dark["dark_slope"][NB:-NB, NB:-NB] * F(calfiles.TFRAME)
cold = np.zeros((len(rp),) + dk.shape, F)
for j in range(len(rp)):
    for x in range(reads[2 * j], reads[2 * j + 1]):
        cold[j] += ipc_linearity.invlinearity(dk * F(x - xref), lin, origin=(NB, NB), ctx=ctx)[0]
    cold[j] /= F(reads[2 * j + 1] - reads[2 * j])
cold_bc = dark["data"][:, NB:-NB, NB:-NB] - cold
c_ms = 1e3 * (time.perf_counter() - t0)
same = np.array_equal(cold.view(np.uint32), hpred.view(np.uint32)) and np.array_equal(cold_bc.view(np.uint32), hbc.view(np.uint32))

npl, ngrp = lin["data"].shape[0], len(rp)
gbytes = 4 * ((npl + 3 + ngrp) * N * N + ngrp * (N - 2 * NB) ** 2) / 1e9
rows = 8
strip = (slice(0, rows + 2 * NB), slice(None))
t0 = time.perf_counter()
ref.biascorr(dark["dark_slope"][strip], dark["data"][(slice(None),) + strip], lin["data"][(slice(None),) + strip], lin["Smin"][strip],
             lin["Smax"][strip], reads)
e_ms = 1e3 * (time.perf_counter() - t0) * (N - 2 * NB) / rows

print(f"biascorr {N}x{N}, {ngrp} groups / {reads[-1]} reads, {npl} Legendre planes ({torch.cuda.get_device_name(0)}):")
print(f"  (a) device-resident, mean of 20 calls:          {a_ms:9.2f} ms")
print(f"  (b) host arrays, mean of 20 calls:              {b_ms:9.2f} ms")
print(f"  (c) 35 x rip_stage_invlinearity + numpy, once:  {c_ms:9.0f} ms  (x{c_ms / a_ms:.0f} of (a), x{c_ms / b_ms:.1f} of (b)); same bits: {same}")
print(f"  (d) algorithmic bytes of the kernel:            {gbytes:9.3f} GB  -> {gbytes / (a_ms / 1e3):.0f} GB/s at (a): compute-bound")
print(f"  (e) numpy restatement, one core, EXTRAPOLATED from {rows} rows: {e_ms / 1e3:.0f} s")
