"""ms per ramp of the whole chain on device-resident 4096 x 4096 ramps, per group count and ipc4d dtype:

    python tools/gpu_checks/group_count_timing.py [G[:k64] ...]              the working build
    python tools/gpu_checks/group_count_timing.py --ab <tag> [G[:k64] ...]   same-box A/B: romanimpreprocess_amd/libromanhip_<tag>.so
                                                                             and the working build, two rounds, alternating, one
                                                                             process per run (ALTLIB selects the library in it)

A library older than the 5-to-16-group forms runs the stage kernels for the counts it has no fused form for, so the A/B compares
a count's fused form with the stage kernels it replaced and with the 8- / 16-group form it extends.  Per configuration: 3 warm-up calls, then SAMPLES batches of BATCH calls
queued back to back with one synchronisation each (wall time per ramp: the overlapped pre-pass included); median, min and max of
the batch means, and the form that ran."""
import os
import statistics
import sys
import time

if len(sys.argv) > 2 and sys.argv[1] == "--ab":
    import subprocess
    for _round in range(2):
        for lib in (f"libromanhip_{sys.argv[2]}.so", None):
            env = dict(os.environ)
            env.pop("ALTLIB", None)
            if lib:
                env["ALTLIB"] = lib
            rc = subprocess.run([sys.executable, os.path.abspath(__file__)] + sys.argv[3:], env=env, timeout=280).returncode
            if rc:   # nothing more is started on the GPU after a failure
                sys.exit(rc)
    sys.exit(0)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from romanimpreprocess_amd import _native
if os.environ.get("ALTLIB"):
    _native.LIB_PATH = os.path.join(os.path.dirname(_native.__file__), os.environ["ALTLIB"])
    import ctypes
    if not hasattr(ctypes.CDLL(_native.LIB_PATH), "rip_chain_form_for"):   # a library older than that query
        _native.SYMBOLS.pop("rip_chain_form_for")
from romanimpreprocess_amd import pipeline, synth

N, SAMPLES, BATCH = 4096, 5, 10
LENS = [1, 1, 2, 3, 5, 2, 1, 4, 2, 3, 1, 2, 6, 1, 2, 1]


def read_pattern(G):
    if G == 8:
        return synth.READ_PATTERN_8
    if G == 16:
        return synth.READ_PATTERN_16
    if G == 6:
        return synth.READ_PATTERN_6
    rp, at = [], 0
    for g in range(G):
        rp.append(list(range(at, at + LENS[g])))
        at += LENS[g]
    return rp


DEFAULT = ["5", "6", "7", "8", "10", "12", "13", "15", "16", "7:k64", "8:k64", "10:k64", "13:k64", "14:k64", "16:k64"]
cb = pipeline.Calibrator(device=0)
dev = torch.device("cuda", 0)
tag = os.environ.get("ALTLIB", "working build")
for spec in sys.argv[1:] or DEFAULT:
    G = int(spec.split(":")[0])
    kdt = np.float64 if spec.endswith(":k64") else np.float32
    rp = read_pattern(G)
    cal, ramp = synth.make_tiled_inputs(N, N, read_pattern=rp, p_order=8, seed=1, strip_rows=64, ipc_dtype=kdt)
    cb.load_caldir(0, cal)
    pid, _meta = cb.plan_for(rp, ramp["frame_time"])
    g = ramp["groupdq"].copy()
    g[0] |= 1
    t = [torch.from_numpy(ramp["data"].view(np.int16)).to(dev), torch.from_numpy(ramp["amp33"].view(np.int16)).to(dev),
         torch.from_numpy(g).to(dev), torch.from_numpy(ramp["pixeldq"].view(np.int32)).to(dev)]
    o = [torch.empty((N, N), dtype=torch.float32, device=dev) for _ in range(3)] + [
        torch.empty((N, N), dtype=torch.int32, device=dev), torch.empty((G, N, N), dtype=torch.uint8, device=dev)]
    torch.cuda.synchronize()

    def call():
        cb.calibrate_device(0, pid, G, t[0].data_ptr(), True, t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                            o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), o[4].data_ptr(), inputs_complete=True)

    for _ in range(3):
        call()
    cb.synchronize()
    ms = []
    for _ in range(SAMPLES):
        t0 = time.perf_counter()
        for _ in range(BATCH):
            call()
        cb.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / BATCH)
    print(f"lib={tag} G={G} ipc4d={'f64' if kdt == np.float64 else 'f32'} form={cb.ctx.last_chain_form()} "
          f"median {statistics.median(ms):.3f} ms  min {min(ms):.3f}  max {max(ms):.3f}", flush=True)
    del t, o
    cb.ctx.drop_caldir(0)
    torch.cuda.empty_cache()
