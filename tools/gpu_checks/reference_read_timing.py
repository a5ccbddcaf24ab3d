"""The measured record of the reference-read decoding (csrc/refread.hip), written to profiles/reference_read.txt:

    python tools/gpu_checks/reference_read_timing.py [--out FILE] [--launches 30] [--batches 9]

    kernel   rip_stage_decode_reference_read on a 4096 x 4096 x 7 u16 cube, in place, device-resident: `launches` launches queued
             back to back on the context's stream, one synchronisation; `batches` such batches after a warm-up one
    copy     hipMemcpyDtoDAsync of the same cube bytes on the same stream, in the same process, timed the same way.  The kernel
             moves (2 G + 1) / (2 G) of the copy's bytes (the cube in and out, the reference plane once)
    rotating both again with consecutive launches on four different cubes (0.94 GB, past the last-level cache, which holds one
             235 MB cube but not the copy's source and destination together)
    host     one Calibrator.calibrate of a page-locked host ramp (page-locked results, group flags included), the exposure
             stored with its reference read subtracted and the same 7 groups plain: 6 calls each, alternating, the first pair
             not counted

A record, not a gate.  Wall times of the host (time.perf_counter around queue + synchronise); medians with minimum and maximum."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "reference_read.txt"))
ap.add_argument("--launches", type=int, default=30)
ap.add_argument("--batches", type=int, default=9)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from romanimpreprocess_amd import _native, pipeline, synth  # noqa: E402
from romanimpreprocess_amd.from_sim import sim_to_isim  # noqa: E402

N, G, OFFSET = 4096, 7, 4000
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def hip_runtime():
    """the HIP runtime this process has loaded (torch's own copy where torch is installed)"""
    with open("/proc/self/maps") as f:
        paths = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
    if not paths:
        raise RuntimeError("no libamdhip64 is mapped into this process")
    return C.CDLL(paths[0]), paths[0]


def spread(ms):
    return f"median {statistics.median(ms):8.4f} ms   min {min(ms):8.4f}   max {max(ms):8.4f}"


cb = pipeline.Calibrator(device=0)
ctx = cb.ctx
dev = torch.device("cuda", 0)
prop = torch.cuda.get_device_properties(0)
hip, hip_path = hip_runtime()
say("Reference-read decoding (csrc/refread.hip): the measured record")
say(f"command : python tools/gpu_checks/reference_read_timing.py --launches {args.launches} --batches {args.batches}")
say(f"box     : {prop.name} ({prop.gcnArchName}), {prop.multi_processor_count} CUs, {prop.total_memory / 2**30:.0f} GiB; torch {torch.__version__}, HIP {torch.version.hip}")
say(f"runtime : {os.path.basename(hip_path)}")
say()

# ---- kernel against copy
rng = np.random.default_rng(1)
cube = torch.from_numpy(rng.integers(0, 65536, size=(G, N, N), dtype=np.uint16).view(np.int16)).to(dev)
# (reference = offset everywhere: decoding in place is then the identity, launch after launch, and no sample leaves the range)
ref = torch.full((N, N), OFFSET, dtype=torch.int16, device=dev)
other = torch.empty_like(cube)
count = torch.zeros(1, dtype=torch.int64, device=dev)
torch.cuda.synchronize()
nbytes = cube.numel() * 2
stream = C.c_void_p(ctx.stream)
hip.hipMemcpyDtoDAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
hip.hipMemcpyDtoDAsync.restype = C.c_int


def decode():
    ctx.check(ctx.lib.rip_stage_decode_reference_read(ctx.h, cube.data_ptr(), G, N * N, ref.data_ptr(), OFFSET, _native.RIP_DEVICE,
                                                      cube.data_ptr(), count.data_ptr()))


def copy():
    rc = hip.hipMemcpyDtoDAsync(other.data_ptr(), cube.data_ptr(), nbytes, stream)
    if rc != 0:
        raise RuntimeError(f"hipMemcpyDtoDAsync: error {rc}")


def batches(call):
    ms = []
    for b in range(args.batches + 1):
        t0 = time.perf_counter()
        for _ in range(args.launches):
            call()
        ctx.synchronize()
        if b:   # the first batch warms up
            ms.append((time.perf_counter() - t0) * 1e3 / args.launches)
    return ms


before = cube.clone()
t_kernel, t_copy = batches(decode), batches(copy)
t_kernel2, t_copy2 = batches(decode), batches(copy)   # once more, the other way round in time
assert torch.equal(cube, before) and torch.equal(other, before) and int(count.item()) == 0
del before
# consecutive launches on different cubes: what a stream of exposures does to the caches
ring = [cube, other] + [cube.clone() for _ in range(2)]
torch.cuda.synchronize()
turn = [0]


def decode_rotating():
    c = ring[turn[0] % 4]
    turn[0] += 1
    ctx.check(ctx.lib.rip_stage_decode_reference_read(ctx.h, c.data_ptr(), G, N * N, ref.data_ptr(), OFFSET, _native.RIP_DEVICE,
                                                      c.data_ptr(), count.data_ptr()))


def copy_rotating():
    src, dst = ring[turn[0] % 4], ring[(turn[0] + 1) % 4]
    turn[0] += 2
    rc = hip.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), nbytes, stream)
    if rc != 0:
        raise RuntimeError(f"hipMemcpyDtoDAsync: error {rc}")


t_kernel_r, t_copy_r = batches(decode_rotating), batches(copy_rotating)
assert int(count.item()) == 0
moved_kernel, moved_copy = (2 * G + 1) * N * N * 2, 2 * nbytes
say(f"1. device-resident {N} x {N} x {G} u16 cube ({nbytes / 1e6:.0f} MB), in place, {args.launches} launches back to back, {args.batches} batches, per launch:")
for name, ms, moved in (("decode kernel", t_kernel, moved_kernel), ("hipMemcpyDtoD", t_copy, moved_copy),
                        ("decode kernel (again)", t_kernel2, moved_kernel), ("hipMemcpyDtoD (again)", t_copy2, moved_copy)):
    say(f"   {name:22s} {spread(ms)}   {moved / 1e9 / (statistics.median(ms) * 1e-3):7.0f} GB/s of {moved / 1e6:.0f} MB moved")
ratio = statistics.median(t_kernel + t_kernel2) / statistics.median(t_copy + t_copy2)
say(f"   kernel / copy = {ratio:.3f} (bytes moved: {(2 * G + 1) / (2 * G):.3f})")
say("   consecutive launches on four different cubes (0.94 GB in turn):")
for name, ms, moved in (("decode kernel", t_kernel_r, moved_kernel), ("hipMemcpyDtoD", t_copy_r, moved_copy)):
    say(f"   {name:22s} {spread(ms)}   {moved / 1e9 / (statistics.median(ms) * 1e-3):7.0f} GB/s of {moved / 1e6:.0f} MB moved")
say(f"   kernel / copy = {statistics.median(t_kernel_r) / statistics.median(t_copy_r):.3f}")
del cube, ref, other, ring
torch.cuda.empty_cache()
say()

# ---- one calibrate of a page-locked host ramp, encoded and plain
rp = synth.READ_PATTERN_8
cal, ramp = synth.make_tiled_inputs(N, N, read_pattern=rp, p_order=8, seed=1, strip_rows=128)
cb.load_caldir(0, cal)
tree = {"data": ramp["data"], "amp33": ramp["amp33"]}
plain = {"data": ramp["data"][1:], "amp33": ramp["amp33"][1:], "groupdq": ramp["groupdq"][1:], "pixeldq": ramp["pixeldq"]}
sim_to_isim.extract_ref(tree, {"EXTRACT_REF": {"data_encoding_offset": OFFSET}})
enc = dict(plain, data=tree["data"], amp33=tree["amp33"], reference_read=tree["reference_read"], reference_amp33=tree["reference_amp33"])
# where the encoder clipped (a ramp that spans more than 65535 - offset), the decoded sample is not the original: the plain ramp
# the encoded run is compared with is then the decoded one
clipped = 0
for key, refkey in (("data", "reference_read"), ("amp33", "reference_amp33")):
    dec = np.clip(enc[key].astype(np.int32) + enc[refkey].astype(np.int32)[None] - OFFSET, 0, 65535).astype(np.uint16)
    clipped += int(np.count_nonzero(dec != plain[key]))
    plain[key] = dec


def pinned(arrays):
    out = {}
    for k, v in arrays.items():
        out[k] = cb.pinned_empty(v.shape, v.dtype)
        out[k][...] = v
    return out


enc_p = dict(pinned(enc), read_pattern=rp[1:], frame_time=ramp["frame_time"], data_encoding_offset=OFFSET)
plain_p = dict(pinned(plain), read_pattern=rp[1:], frame_time=ramp["frame_time"])
outs = [{"slope": cb.pinned_empty((N, N), np.float32), "err_read": cb.pinned_empty((N, N), np.float32),
         "err_poisson": cb.pinned_empty((N, N), np.float32), "pixeldq": cb.pinned_empty((N, N), np.uint32),
         "groupdq": cb.pinned_empty((G, N, N), np.uint8)} for _ in range(2)]
t_enc, t_plain = [], []
for i in range(6):
    for r, o, ts in ((enc_p, outs[0], t_enc), (plain_p, outs[1], t_plain)):
        t0 = time.perf_counter()
        cb.calibrate(0, r, exclude_first=False, out=o)
        if i:
            ts.append((time.perf_counter() - t0) * 1e3)
form = ctx.last_chain_form()
same = all(np.array_equal(outs[0][k].view(np.uint8), outs[1][k].view(np.uint8)) for k in outs[0])
say(f"2. Calibrator.calibrate of one page-locked host ramp, {N} x {N} x {G} groups (CALDIR of 8), page-locked results with group flags, 5 calls each:")
say(f"   stored with the reference read subtracted   {spread(t_enc)}")
say(f"   the same groups, plain                      {spread(t_plain)}")
say(f"   difference of the medians {statistics.median(t_enc) - statistics.median(t_plain):.3f} ms (the upload of the two reference planes, "
    f"{(N * N + N * 128) * 2 / 1e6:.1f} MB, and the two decode launches); chain form {form}; "
    f"the encoder clipped {clipped} of {enc['data'].size + enc['amp33'].size} samples, the plain ramp holds the decoded ones; "
    f"all five outputs equal bit for bit: {same}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
