#!/usr/bin/env python3
"""Generate tests/golden/fpaplot_small.npz by running the REFERENCE's own ``utils/fpaplot.py``, unmodified.

Runs only where the reference is mounted (see tools/make_goldens.py, whose stand-ins for ``asdf`` and ``roman_datamodels`` this
tool uses; matplotlib and PIL, which the module imports, are real).  The module's focal-plane globals ``nside_base``, ``ctrs`` and
``bbox`` are set to the 64-pixel focal plane of tests/fpaplot_ref.py; ``read_sca_image``, ``make_big_image`` and ``multi_image``
then run as they are on small calibration arrays drawn with a fixed seed: smooth fields inside each panel's vmin .. vmax, 5 % of
the pixels flagged.  The file names handed to the reference exist as empty files (it asks ``os.path.exists``); their contents are
served from memory.

The fixture stores the inputs (6 distinct sets shared by the 18 SCAs, only the planes the picture reads), the binned maps, the
RGB arrays, the glyph table and the ``checkpix`` list of the reference's workflow test as recorded data.  While making it the tool
compares the float64 restatement with the reference's colour indices and prints the share that differs.

Usage:  python tools/make_fpaplot_goldens.py [--out DIR]
"""

import ast
import os
import shutil
import sys
import tempfile

import numpy as np

import make_goldens as mg   # installs the stand-ins and puts the reference on the path

import fpaplot_ref as fr  # noqa: E402
from romanimpreprocess.utils import fpaplot as ref_fp  # noqa: E402

NSETS = 6
MISSING_GAIN = 7      # this SCA has no gain file
MISSING_ALL = 12      # this SCA has no file at all
N1 = 16
SINGLE_N1 = (64, 2, 1)   # read_sca_image of SCA 1 at these bin counts too


def input_sets(seed=20250521):
    """per set: the planes the picture reads, float32 as the calibration files hold them, but the ipc4d planes of the odd sets
    float64 (what make_gain_file writes); ipc4d planes are 56 x 56 (no reference pixels), the others 64 x 64"""
    rng = np.random.default_rng(seed)
    rng_of = {p[0]: p[1:3] for p in fr.PANELS}
    sets = []
    for i in range(NSETS):
        s = {"dq": fr.random_dq(rng, 64)}
        for ptype, (lo, hi) in rng_of.items():
            side = 56 if ptype.startswith("alpha") else 64
            dt = np.float64 if ptype.startswith("alpha") and i % 2 else np.float32
            s[ptype] = fr.smooth_field(rng, side, lo, hi).astype(dt)
        sets.append(s)
    return sets


def file_arrays(s):
    """the arrays of the six files of one SCA, with the planes of set `s` where the picture reads them and zeros elsewhere"""
    lin = np.zeros((4, 64, 64), np.float32)
    lin[2], lin[3] = s["lin2"], s["lin3"]
    ipc = np.zeros((3, 3, 56, 56), s["alphaH"].dtype)
    ipc[1, 0], ipc[0, 1], ipc[0, 0] = s["alphaH"], s["alphaV"], s["alphaD"]
    return {"linearitylegendre": lin, "ipc4d": ipc, "gain": s["gain"], "pflat": s["pflatnorm"], "read": s["read"]}


def main(argv):
    out_dir = mg.OUT
    if "--out" in argv:
        out_dir = mg.OUT = os.path.abspath(argv[argv.index("--out") + 1])
    ref_fp.nside_base = fr.SMALL["nside"]
    ref_fp.ctrs = np.array(fr.SMALL["ctrs"], dtype=np.int32)
    ref_fp.bbox = dict(fr.SMALL["bbox"])
    sets = input_sets()
    sca_set = np.array([k % NSETS for k in range(18)], dtype=np.int32)
    tmp = tempfile.mkdtemp(prefix="fpaplot_golden_")
    try:
        fmt = os.path.join(tmp, "roman_wfi_{:s}_GOLDEN_SCA{:02d}.asdf")
        for k in range(18):
            if k + 1 == MISSING_ALL:
                continue
            s = sets[sca_set[k]]
            files = dict(file_arrays(s), mask=None)
            if k + 1 == MISSING_GAIN:
                del files["gain"]
            for name, arr in files.items():
                path = fmt.format(name, k + 1)
                open(path, "w").close()
                mg.register(path, {"dq": s["dq"]} if name == "mask" else {"data": arr})
        mask = mg.ref_mh.PixelMask1
        ptypes = [p[0] for p in fr.PANELS]
        maps = np.stack([np.stack([ref_fp.read_sca_image(fmt, N1, p, k + 1, mask=mask) for k in range(18)]) for p in ptypes])
        single = {f"maps_sca1_n{n}": np.stack([ref_fp.read_sca_image(fmt, n, p, 1, mask=mask) for p in ptypes]) for n in SINGLE_N1}
        rgb = ref_fp.multi_image(fmt, N1, mask)
        rgb32 = ref_fp.multi_image(fmt, 32, mask)
        gain_plain = ref_fp.make_big_image(fmt, N1, "gain", vmin=1.2, vmax=2.1, mask=mask)
        gain_scale = ref_fp.make_big_image(fmt, N1, "gain", vmin=1.2, vmax=2.1, mask=mask, scaleformat="{:4.2f}")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

    # the workflow test's recorded pixels (tests/romanimpreprocess/test_workflow.py:493-503), as data
    wf = ast.parse(open(os.path.join(os.path.dirname(mg.REF_SRC), "tests", "romanimpreprocess", "test_workflow.py")).read())
    checkpix = next(np.array(ast.literal_eval(n.value.args[0]), dtype=np.int16) for n in ast.walk(wf)
                    if isinstance(n, ast.Assign) and ast.unparse(n.targets[0]) == "checkpix")

    # the share of SCA pixels whose colour index the float64 restatement gives differently (the reference sums float32 in float32)
    glyphs = np.asarray(ref_fp.letters, dtype=np.uint8)
    table = np.asarray(ref_fp.matplotlib.colormaps["viridis"](np.arange(256), bytes=True)[:, :3])
    scas = [None if k + 1 == MISSING_ALL else {p: v for p, v in sets[sca_set[k]].items() if not (k + 1 == MISSING_GAIN and p == "gain")}
            for k in range(18)]
    pic, _, owner, _ = fr.multi_image_ref(scas, N1, fr.PIXELMASK1, fr.SMALL, table, glyphs)
    differ = (pic != rgb).any(axis=2)
    print(f"  restatement vs reference at n1 {N1}: {np.count_nonzero(differ & (owner >= 0))} of {np.count_nonzero(owner >= 0)} SCA pixels "
          f"differ in colour, {np.count_nonzero(differ & (owner < 0))} other pixels differ, largest channel step "
          f"{np.abs(pic.astype(int) - rgb.astype(int)).max()}")

    arrays = {"sca_set": sca_set, "missing_gain": np.int32(MISSING_GAIN), "missing_all": np.int32(MISSING_ALL), "n1": np.int32(N1),
              "maps": maps, "rgb": rgb, "rgb_n32": rgb32, "gain_plain": gain_plain, "gain_scale": gain_scale, "glyphs": glyphs,
              "table": table, "checkpix": checkpix, **single}
    for i, s in enumerate(sets):
        for key, v in s.items():
            arrays[f"set{i}_{key}"] = v
    mg.OUT = out_dir
    mg.save("fpaplot_small", **arrays)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
