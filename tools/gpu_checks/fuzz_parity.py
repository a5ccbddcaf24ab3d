"""Randomised parity sweep: the whole chain on the GPU against the numpy oracle, bit for bit, over random frame shapes, MA
tables, Legendre orders, dtypes, jump parameters and cosmic-ray / bad-pixel densities.
    python tools/gpu_checks/fuzz_parity.py [ncases] [seed] [skip_first]
skip_first (0 or 1) given: the option "skip_first" is set to it and the corrected cube is NOT asked for (a call that wants the cube
always takes the full kernel form), so that with 1 the form that skips an excluded first group is in the sweep; the tally at the
end tells how many fused launches skipped group 0."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

import oracle
from oracle import saturation
from romanimpreprocess_amd import _native, pipeline, synth

ncases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
skip_mode = int(sys.argv[3]) if len(sys.argv) > 3 else None   # None: the sweep as it always was (cube compared, option untouched)
ctx = _native.default_context(0)
if skip_mode is not None:
    ctx.set_option("skip_first", skip_mode)
skipped = 0
cb = pipeline.Calibrator(ctx=ctx)


def random_pattern(gmin=3, gmax=16):
    """one case in five each: the 8-, 6- and 16-group patterns of the tests; otherwise gmin..gmax groups of 1..4 reads.  The fused
    kernel has a form for every count from 5 to 16, odd ones included; the default draw keeps 3 and 4 groups as well, so that the
    stage kernels of the shortest ramps stay in the sweep (the multi-strip tenth of the cases draws 5..16 only)"""
    kind = rng.integers(0, 5)
    if kind == 0:
        return synth.READ_PATTERN_8
    if kind == 1:
        return synth.READ_PATTERN_6
    if kind == 2:
        return synth.READ_PATTERN_16
    g = int(rng.integers(gmin, gmax + 1))
    rp, t = [], 0
    for _ in range(g):
        n = int(rng.integers(1, 5))
        rp.append(list(range(t, t + n)))
        t += n
    return rp


def same(a, b, zero_sign_ok=False):
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    bad = (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))
    if zero_sign_ok:
        bad &= ~((a == 0) & (b == 0))
    return not bad.any()


fails, forms = 0, {0: 0, 1: 0, 2: 0, 3: 0}
by_groups = {}   # group count -> [cases, of them on the fused kernel]
by_geometry = {}   # (window columns, 5-8 / 9-16 groups, uniform / quad) -> fused launches, from rip_last_chain_geometry
t0 = time.time()
for case in range(ncases):
    rp = random_pattern()
    ny, nx = int(rng.integers(4, 13)) * 8, int(rng.choice([128, 256, 384]))
    if rng.random() < 0.1:
        # a tenth of the cases: frames of several strips and row ranges (up to 9 strips of the narrow forms, ranges that do
        # not divide the rows), with a group count the fused kernel is instantiated for; 768 and 1152 columns -- multiples of 384,
        # where the 384-column forms have a last strip narrow enough for quad mode -- with heights up to 1400 rows, tall enough
        # for quad mode to win on a device of 256 CUs (the tally at the end tells what the sweep reached)
        rp = random_pattern(5, 16)
        ny, nx = int(rng.integers(13, 76)) * 4, int(rng.choice([512, 640, 768, 1024, 1152]))
        if nx in (768, 1152) or rng.random() < 0.25:
            ny = int(rng.integers(52, 1401))
    p = int(rng.choice([3, 8, 10]))
    gdt = np.float64 if rng.random() < 0.2 else np.float32
    kdt = np.float64 if rng.random() < 0.4 else np.float32
    excl = bool(rng.random() < 0.7) or len(rp) < 4
    if len(rp) == 3:
        excl = False
    jump = None
    if rng.random() < 0.5:
        jump = {"SthreshA": float(rng.uniform(3, 8)), "SthreshB": float(rng.uniform(3, 6)), "IthreshA": float(rng.uniform(0.1, 2)),
                "IthreshB": float(rng.uniform(200, 2000))}
    seed = int(rng.integers(1, 10**6))
    cal = synth.make_caldir(ny, nx, read_pattern=rp, p_order=p, seed=seed, gain_dtype=gdt, ipc_dtype=kdt,
                            bias_amplitude=float(rng.uniform(0, 3)), bad_lin_frac=float(rng.uniform(0, 0.02)))
    ramp = synth.make_ramp(cal, read_pattern=rp, seed=seed + 1, cr_frac=float(rng.uniform(0, 0.08)))
    # one case in three: dq-init + saturation flagging on the device (with or without the read-pattern rule) against the numpy
    # restatement, thresholds lowered so that a few per cent of the pixels saturate at various groups
    sat = rng.random() < 0.33
    sat_kw = {}
    if sat:
        thr = np.quantile(ramp["data"].astype(np.float32), float(rng.uniform(0.6, 0.95)), axis=0).astype(np.float32)
        thr[rng.random((ny, nx)) < 0.95] = 65535.0
        sdq = np.where(rng.random((ny, nx)) < 0.01, np.uint32(1 << 21), np.uint32(0)).astype(np.uint32)   # NO_SAT_CHECK
        cal = dict(cal)
        cal["saturation"] = {"data": thr, "dq": sdq}
        backup, use_rp = int(rng.integers(0, 3)), bool(rng.random() < 0.5)
        h = {"data": ramp["data"], "groupdq": np.zeros(ramp["data"].shape, np.uint8), "pixeldq": ramp["pixeldq"].copy()}
        saturation.flag_saturation(h, thr, backup=backup, skip_firstn=1, n_pix_grow_sat=1, sat_dq=sdq, read_pattern=rp if use_rp else None)
        if excl:
            h["groupdq"][0] |= np.uint8(1)
        mask_dq = ramp["pixeldq"].copy()
        ramp = dict(ramp, groupdq=h["groupdq"], pixeldq=h["pixeldq"])
        sat_kw = dict(flag_saturation=True, saturation_backup=backup, saturation_read_pattern=use_rp)
    with np.errstate(all="ignore"):
        ref = oracle.calibrate_arrays(ramp, cal, exclude_first=excl, jump_pars=jump)
    lines = np.zeros((len(rp), nx // 128, 2))
    for g in range(len(rp)):
        lines[g] = ref["refpix_diag"][g]["channels"][:nx // 128, 2:4]
    ctx.set_option("fused", int(rng.random() < 0.8))
    ctx.set_option("chain2", int(rng.random() < 0.8))
    cb.load_caldir(1, cal)
    dev_ramp = dict(ramp, groupdq=None, pixeldq=mask_dq) if sat else ramp
    got = cb.calibrate(1, dev_ramp, exclude_first=excl, jump_pars=jump, want_cube=skip_mode is None, channel_lines=lines, **sat_kw)
    forms[ctx.last_chain_form()] += 1
    skipped += ctx.last_chain_first_group()
    tally = by_groups.setdefault(len(rp), [0, 0])
    tally[0] += 1
    tally[1] += ctx.last_chain_form() == 2
    if ctx.last_chain_form() == 2:
        geo = ctx.last_chain_geometry()
        key = (f"{'f64' if kdt == np.float64 else 'f32'} ipc4d, {'5-8' if len(rp) <= 8 else '9-16'} groups, {geo['cols']} columns",
               "quad" if geo["nq"] else "uniform")
        by_geometry[key] = by_geometry.get(key, 0) + 1
    ok = ((skip_mode is not None or same(got["cube"], ref["data"], True)) and same(got["groupdq"], ref["groupdq"]) and same(got["pixeldq"], ref["pixeldq"])
          and all(same(got[k], ref[k], True) for k in ("slope", "err_read", "err_poisson")))
    if not ok:
        fails += 1
        print(f"MISMATCH case {case}: G={len(rp)} rp={rp} shape=({ny},{nx}) p={p} gain={gdt.__name__} ipc={kdt.__name__} excl={excl} "
              f"jump={jump} seed={seed} form={ctx.last_chain_form()} sat={sat_kw}", flush=True)
    if (case + 1) % 25 == 0:
        print(f"{case + 1} cases, {fails} mismatches, forms {forms}, {time.time() - t0:.0f} s", flush=True)
ctx.set_option("fused", 1)
ctx.set_option("chain2", 1)
print(f"done: {ncases} cases, {fails} mismatches; kernel forms used (0 stage kernels, 2 fused kernel): {forms}")
print(f"skip_first option: {'default' if skip_mode is None else skip_mode}; fused launches that skipped group 0: {skipped}")
print("groups: cases / on the fused kernel --", ", ".join(f"{g}: {n} / {f}" for g, (n, f) in sorted(by_groups.items())))
print("fused launches by (form, launch geometry) --", ", ".join(f"{form} {mode}: {n}" for (form, mode), n in sorted(by_geometry.items())))
sys.exit(1 if fails else 0)
