"""The measured record of the L2-output stage (csrc/l2out.hip) and of calibrateimage around it, kept in profiles/l2_out.txt:

    python tools/gpu_checks/l2_out_timing.py planes [--variant LIB] [--launches 30] [--batches 9] [--out FILE]
    python tools/gpu_checks/l2_out_timing.py calibrate [--repo DIR] [--scratch DIR] [--calls 5] [--out FILE]

planes     rip_stage_l2_planes on a 4096 x 4096 frame, nb = 4, device to device, every output wanted: `launches` launches queued
           back to back on the context's stream, one synchronisation; `batches` such batches after a warm-up one; float32 and
           float16 variance planes.  Beside it hipMemcpyDtoDAsync of as many bytes as the kernel moves (half of reads + writes
           is the copy's length: a copy reads and writes each byte), on the same stream, in the same process, timed the same way.
           --variant LIB: a second build of the library (csrc/l2out.hip compiled with -DRIP_L2_PLAIN_STORES=1, linked with the
           other objects), loaded into the SAME process and timed in turn with the first.
calibrate  calibrateimage on a synthetic 4096 x 4096 x 8 uint16 exposure (synth_gpu, as noise_layers_fullsize.py makes it), files
           in `--scratch` (made there if absent, so that two processes share them), CALDIR resident, SKYORDER 2, SLICEOUT, L2 file
           to the scratch directory: `calls` calls after a warm-up one; the median, the spread, and where the time goes.  --repo
           DIR: import the package from DIR instead of this tree -- a build of another commit, for the same script in another
           process.  The breakdown wraps the functions a commit has; what it does not have is not listed.

A record, not a gate.  Wall times of the host (time.perf_counter), medians with minimum and maximum."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["planes", "calibrate"])
ap.add_argument("--out", default=None)
ap.add_argument("--launches", type=int, default=30)
ap.add_argument("--batches", type=int, default=9)
ap.add_argument("--variant", default=None)
ap.add_argument("--repo", default=HERE)
ap.add_argument("--scratch", default="/dev/shm/rip_l2_out_timing")
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--label", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.repo))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from romanimpreprocess_amd import _native, calio, pipeline, synth  # noqa: E402

lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def spread(ms):
    return f"median {statistics.median(ms):9.4f} ms   min {min(ms):9.4f}   max {max(ms):9.4f}"


def finish():
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


prop = torch.cuda.get_device_properties(0)
box = f"{prop.name} ({prop.gcnArchName}), {prop.multi_processor_count} CUs; torch {torch.__version__}, HIP {torch.version.hip}"


# ------------------------------------------------------------------------------------------------------------------- planes
def planes():
    with open("/proc/self/maps") as f:
        paths = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
    ctx = _native.default_context(0)
    hip = C.CDLL(paths[0])
    hip.hipMemcpyDtoDAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    hip.hipMemcpyDtoDAsync.restype = C.c_int
    say("L2 planes stage (csrc/l2out.hip: rip_stage_l2_planes): the measured record")
    say(f"command : python tools/gpu_checks/l2_out_timing.py planes --launches {args.launches} --batches {args.batches}"
        + (" --variant <library built with -DRIP_L2_PLAIN_STORES=1>" if args.variant else ""))
    say(f"box     : {box}")
    say()
    libs = [("the library (non-temporal stores)", ctx.lib, ctx.h)]
    if args.variant:
        vlib = C.CDLL(os.path.abspath(args.variant))
        for name in ("rip_ctx_create", "rip_stage_l2_planes", "rip_synchronize", "rip_stream"):
            getattr(vlib, name).restype, getattr(vlib, name).argtypes = _native.SYMBOLS[name]
        vh = C.c_void_p()
        if vlib.rip_ctx_create(0, C.byref(vh)) != 0:
            raise RuntimeError("the variant library gave no context")
        libs.append(("plain stores only", vlib, vh))
    N, nb = 4096, 4
    na = (N - 2 * nb) ** 2
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    ins = [torch.rand((N, N), device=dev, generator=gen) for _ in range(3)] + [torch.randint(0, 2 ** 31 - 1, (N, N), device=dev, dtype=torch.int32)]
    f32 = [torch.empty(na, dtype=torch.float32, device=dev) for _ in range(4)] + [torch.empty(na, dtype=torch.int32, device=dev)]
    f16 = [torch.empty(na, dtype=torch.float16, device=dev) for _ in range(3)]
    strips = [torch.empty(N * nb, dtype=torch.int32, device=dev) for _ in range(4)]
    copy_src, copy_dst = torch.empty(9 * na * 4 // 2, dtype=torch.uint8, device=dev), torch.empty(9 * na * 4 // 2, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    P = [t.data_ptr() for t in ins]

    def stage(lib, h, half):
        v = f16 if half else f32[1:4]
        a = (h, P[0], P[1], P[2], P[3], N, N, nb, _native.RIP_F16 if half else _native.RIP_F32, _native.RIP_DEVICE, f32[0].data_ptr(),
             f32[4].data_ptr(), v[0].data_ptr(), v[1].data_ptr(), v[2].data_ptr(), *(s.data_ptr() for s in strips))

        def run():
            if lib.rip_stage_l2_planes(*a) != 0:
                raise RuntimeError("rip_stage_l2_planes failed")
        return run

    def copier(lib, h, nbytes):
        stream = C.c_void_p(lib.rip_stream(h))

        def run():
            if hip.hipMemcpyDtoDAsync(copy_dst.data_ptr(), copy_src.data_ptr(), nbytes, stream) != 0:
                raise RuntimeError("hipMemcpyDtoDAsync failed")
        return run

    def batches(call, lib, h):
        ms = []
        for b in range(args.batches + 1):
            t0 = time.perf_counter()
            for _ in range(args.launches):
                call()
            if lib.rip_synchronize(h) != 0:
                raise RuntimeError("rip_synchronize")
            if b:
                ms.append((time.perf_counter() - t0) * 1e3 / args.launches)
        return ms

    moved = {False: 9 * na * 4, True: 6 * na * 4 + 3 * na * 2}   # four reads and five writes over the active region
    say(f"frame {N} x {N}, nb = {nb}, device to device, all five planes and the four flag strips, {args.launches} launches back to back, "
        f"{args.batches} batches, per launch (the strips' four small launches included):")
    med = {}
    for turn in range(2):
        for label, lib, h in libs:
            for half in (False, True):
                kind = "float16" if half else "float32"
                for name, call in ((f"planes, {kind} variances", stage(lib, h, half)),
                                   (f"hipMemcpyDtoD of {moved[half] // 2 / 1e6:.0f} MB ({kind} traffic)", copier(lib, h, moved[half] // 2))):
                    ms = batches(call, lib, h)
                    med.setdefault((label, name), []).extend(ms)
                    say(f"   {label:34s} {name:46s} {spread(ms)}   {moved[half] / 1e9 / (statistics.median(ms) * 1e-3):6.0f} GB/s")
    say()
    for label, _, _ in libs:
        for half in (False, True):
            kind = "float16" if half else "float32"
            k = statistics.median(med[(label, f"planes, {kind} variances")])
            c = statistics.median(med[(label, f"hipMemcpyDtoD of {moved[half] // 2 / 1e6:.0f} MB ({kind} traffic)")])
            say(f"   {label}: {kind}: kernel / copy = {k / c:.3f}")
    if len(libs) == 2:
        for half in (False, True):
            name = f"planes, {'float16' if half else 'float32'} variances"
            say(f"   non-temporal / plain stores, {name}: {statistics.median(med[(libs[0][0], name)]) / statistics.median(med[(libs[1][0], name)]):.3f}")


# ---------------------------------------------------------------------------------------------------------------- calibrate
class Clock:
    """wall time per label, accumulated by wrappers around the functions a commit has"""

    def __init__(self):
        self.t, self.depth = {}, 0

    def wrap(self, owner, name, label):
        fn = getattr(owner, name, None)
        if fn is None:
            return
        clock = self

        def timed(*a, **k):
            if clock.depth:   # inside another timed function: its time is counted there
                return fn(*a, **k)
            clock.depth += 1
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                clock.depth -= 1
                clock.t[label] = clock.t.get(label, 0.0) + (time.perf_counter() - t0) * 1e3
        setattr(owner, name, timed)


def calibrate():
    from romanimpreprocess_amd import synth_gpu
    from romanimpreprocess_amd.L1_to_L2 import gen_cal_image
    from romanimpreprocess_amd.utils import maskhandling, sky

    label = args.label or os.path.abspath(args.repo)
    scratch = args.scratch
    rp, N = synth.READ_PATTERN_8, 4096
    names = {"dark": "dark", "read": "read", "gain": "gain", "linearitylegendre": "linearitylegendre", "ipc4d": "ipc4d", "flat": "pflat",
             "biascorr": "biascorr", "mask": "mask", "saturation": "saturation"}
    caldir = {k: os.path.join(scratch, f"roman_wfi_{v}_TEST_SCA04.asdf") for k, v in names.items()}
    if not os.path.exists(os.path.join(scratch, "l1.asdf")):
        os.makedirs(scratch, exist_ok=True)
        t0 = time.perf_counter()
        cal = synth_gpu.make_caldir(N, N, read_pattern=rp, p_order=8, seed=1001)
        ramp = synth_gpu.make_ramp(cal, read_pattern=rp, seed=1)
        for key, path in caldir.items():
            calio.write_asdf(path, {"roman": cal[key]})
        calio.write_asdf(os.path.join(scratch, "l1.asdf"), {"roman": {"data": ramp["data"], "amp33": ramp["amp33"], "meta": {
            "exposure": {"frame_time": synth.FRAME_TIME, "read_pattern": rp}, "instrument": {"detector": "WFI04"}}}})
        print(f"synthetic exposure + CALDIR written to {scratch} in {time.perf_counter() - t0:.1f} s", flush=True)
        del cal, ramp
    config = {"IN": os.path.join(scratch, "l1.asdf"), "OUT": os.path.join(scratch, "l2.asdf"), "CALDIR": caldir, "SLICEOUT": True,
              "SKYORDER": 2}
    clock = Clock()
    for owner, name, what in (
            (gen_cal_image, "initializationstep", "read (L1 file, mask file)"),
            (gen_cal_image, "_exposure_to_device", "upload (cube, amp33, mask; strips of the cube)"),
            (pipeline.Calibrator, "calibrate", "chain, host staging (upload + kernels + download of 4 planes and groupdq)"),
            (pipeline.Calibrator, "calibrate_device", "chain (kernels, waited for)"), (pipeline.Calibrator, "synchronize", "chain (kernels, waited for)"),
            (maskhandling.CombinedMask, "build", "post-path (mask, sky mode, sky model, end slices; their copies)"),
            (maskhandling.CombinedMask, "build_device", "post-path (mask, sky mode, sky model, end slices; their copies)"),
            (sky, "binkxk", "post-path (mask, sky mode, sky model, end slices; their copies)"),
            (sky, "smooth_mode", "post-path (mask, sky mode, sky model, end slices; their copies)"),
            (sky, "medfit", "post-path (mask, sky mode, sky model, end slices; their copies)"),
            (sky, "endslice", "post-path (mask, sky mode, sky model, end slices; their copies)"),
            (sky, "block_nanmedians", "median gain (gain file read + selection)"),
            (getattr(gen_cal_image, "oututils", None), "l2_planes", "planes stage (kernel, waited for)"),
            (gen_cal_image, "_download", "download (each plane once)"),
            (calio, "write_asdf", "write (L2 file)")):
        if owner is not None:
            clock.wrap(owner, name, what)
    cb = pipeline.Calibrator()
    totals, parts = [], []
    for i in range(args.calls + 1):
        clock.t = {}
        t0 = time.perf_counter()
        gen_cal_image.calibrateimage(config, verbose=False, calibrator=cb)
        total = (time.perf_counter() - t0) * 1e3
        if i:   # the first call uploads the CALDIR and warms up
            totals.append(total)
            parts.append(dict(clock.t, **{"finishing and everything else (numpy passes, log, tree)": total - sum(clock.t.values())}))
    size = os.path.getsize(config["OUT"])
    say(f"calibrateimage, {label}")
    say(f"box     : {box}")
    say(f"exposure: {N} x {N} x {len(rp)} uint16 (synth_gpu), CALDIR resident, SKYORDER 2, SLICEOUT, L2 file of {size / 1e6:.0f} MB to {scratch}; "
        f"{args.calls} calls after a warm-up one")
    say(f"   total per call   {spread(totals)}   max - min {max(totals) - min(totals):9.4f} ms")
    say("   calls (ms): " + ", ".join(f"{t:.1f}" for t in totals))
    for k in parts[0]:
        say(f"      {k:86s} {spread([p.get(k, 0.0) for p in parts])}")


(planes if args.what == "planes" else calibrate)()
finish()
