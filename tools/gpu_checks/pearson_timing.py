"""Time rip_stage_pearson on 4 M elements resident in HBM, one call per Pearson type: python tools/gpu_checks/pearson_timing.py"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from romanimpreprocess_amd import _native  # noqa: E402

ctx = _native.default_context(0)
dev = torch.device("cuda", ctx.device)
n = 1 << 22
out = torch.empty(n, dtype=torch.float64, device=dev)
for name, (t21, t31, t41), I in (("type 1", (1.0, 1.0, 1.0), 3.0), ("type 4", (1.0, 0.5, 1.0), 40.0), ("type 6", (1.0, 1.0, 1.7), 30.0)):
    d_I = torch.full((n,), I, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ts = []
    for it in range(6):
        t0 = time.perf_counter()
        ctx.check(ctx.lib.rip_stage_pearson(ctx.h, n, d_I.data_ptr(), t21, t31, t41, 11, it, out.data_ptr(), None, None))
        ctx.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    print(f"pearson {name}, {n} elements: min {min(ts[1:]):.3f} ms, median {sorted(ts[1:])[2]:.3f} ms (first call {ts[0]:.2f})")
