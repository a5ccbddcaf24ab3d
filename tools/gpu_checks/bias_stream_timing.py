"""ms per ramp of the device-resident chain on a 4096 x 4096 x 8 ramp, by what the CALDIR set holds for a bias correction:

    python tools/gpu_checks/bias_stream_timing.py [--tree DIR] [--steps 300] [--warmup 50] [noisy] [absent] [zero]

    noisy    biascorr made with bias_amplitude = 2.0: the fused kernel streams its planes (the path that must not pay for the
             launches that run without them)
    absent   no biascorr in the set: the stage kernels before rip_caldir_bias_state, the fused kernel without the stream since
    zero     biascorr all +0, what bench.py's set holds: streamed before, dropped at upload since

--tree DIR imports romanimpreprocess_amd from DIR instead of this repository: a checkout of another commit with its own built
library, for a same-job A/B (one process per run; the caller alternates the trees).  The binding of a commit older than the
queries prints "-" for them.  Per set: `warmup` calls, then `steps` calls queued back to back in batches of 30 with one
synchronisation each (wall time per ramp, the overlapped pre-pass included); median, minimum and maximum of the batch means."""
import argparse
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--warmup", type=int, default=50)
ap.add_argument("--tag", default=None)
ap.add_argument("sets", nargs="*", default=["noisy"])
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from romanimpreprocess_amd import pipeline, synth, synth_gpu  # noqa: E402

N, G, BATCH = 4096, 8, 30
tag = args.tag or os.path.basename(os.path.abspath(args.tree))
cb = pipeline.Calibrator(device=0)
dev = torch.device("cuda", 0)
for which in args.sets:
    amplitude = 2.0 if which == "noisy" else 0.0
    rp = synth.READ_PATTERN_8
    cal = synth_gpu.make_caldir(N, N, read_pattern=rp, p_order=8, seed=1, bias_amplitude=amplitude)
    if which == "absent":
        del cal["biascorr"]
    ramp = synth_gpu.make_ramp(cal, read_pattern=rp, seed=2)
    cb.load_caldir(0, cal)
    state = cb.bias_state(0) if hasattr(cb, "bias_state") else "-"
    pid, _meta = cb.plan_for(rp, ramp["frame_time"])
    t = [torch.from_numpy(np.ascontiguousarray(ramp[k]).view(v)).to(dev)
         for k, v in (("data", np.int16), ("amp33", np.int16), ("groupdq", np.uint8), ("pixeldq", np.int32))]
    o = [torch.empty((N, N), dtype=torch.float32, device=dev) for _ in range(3)] + [
        torch.empty((N, N), dtype=torch.int32, device=dev), torch.empty((G, N, N), dtype=torch.uint8, device=dev)]
    del cal, ramp
    torch.cuda.synchronize()

    def call():
        cb.calibrate_device(0, pid, G, t[0].data_ptr(), True, t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                            o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), o[4].data_ptr(), inputs_complete=True)

    for _ in range(args.warmup):
        call()
    cb.synchronize()
    ms = []
    for _ in range(max(1, args.steps // BATCH)):
        t0 = time.perf_counter()
        for _ in range(BATCH):
            call()
        cb.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / BATCH)
    ctx = cb.ctx
    stream = ctx.last_chain_bias_stream() if hasattr(ctx, "last_chain_bias_stream") else "-"
    checksum = float(o[0].nan_to_num(0.0, 0.0, 0.0).double().sum().item())
    print(f"tree={tag} set={which} state={state} form={ctx.last_chain_form()} first_group_skipped={ctx.last_chain_first_group()} "
          f"bias_stream={stream} median {statistics.median(ms):.4f} ms  min {min(ms):.4f}  max {max(ms):.4f}  "
          f"({len(ms)} batches of {BATCH})  slope checksum {checksum:.6e}", flush=True)
    del t, o
    cb.drop_caldir(0)
    torch.cuda.empty_cache()
