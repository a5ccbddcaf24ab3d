"""Inputs of the gain / ipc4d cases (tests/golden/gainfile_*.npz, tools/make_goldens.py case `gainfile`): solid-waffle summary
tables made from seeded uniform deviates with IEEE arithmetic only (no libm call), so that every machine regenerates the same
bits.  The frames are the smallest at which the expansion kernel can still go wrong:

  gainfile_even   140 x 140, active 132 (even, a multiple of 4 and of no 64 or 256), 4 x 10 superpixels of 35 x 14 pixels: the
                  seams fall on odd columns, so 16-byte stores straddle them; 3 summary files; superpixel (2,1) has N = 0 in
                  every file (it takes the array means, its flags are 2**19), (7,3) in all but the last; aD of (4,2) is negative
  gainfile_odd    45 x 45, active 37 (odd: no row of a plane but the first starts on a 16-byte boundary), 3 x 5 superpixels of
                  15 x 9 pixels, 1 summary file, every superpixel good

(With a border of 4 no 15 x 9 superpixel lies inside the border; superpixels smaller than the border are covered by the
non-square frames of tests/test_gpu_gainfile.py, against tests/gainfile_ref.py.)
The values are non-dyadic (a + b * u with u uniform), so that the float32 rounding, the halved sums and the order of the
nine-term sum all show in the last bits."""

import os

import numpy as np

NB = 4
NCOL = 12   # X, Y, N at 0-2, g, aH, aV at 5-7, aD at 10 (make_gain_file.py:21); the other columns are never read

# name -> seed, frame side, superpixels across and down, summary files, superpixels (sy, sx) without data: in every file / in
# all but the last, and one with a negative aD
CASES = {
    "gainfile_even": dict(seed=411, nside=140, nsx=4, nsy=10, nfiles=3, empty=(2, 1), nearly_empty=(7, 3), negative=(4, 2)),
    "gainfile_odd": dict(seed=412, nside=45, nsx=3, nsy=5, nfiles=1, empty=None, nearly_empty=None, negative=(1, 1)),
}


def inputs(name):
    """the case's summary tables, float64 (nfiles, nsy * nsx, NCOL), rows in (Y, X) row-major order as solid-waffle writes them"""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    nsy, nsx, nf = c["nsy"], c["nsx"], c["nfiles"]
    sy, sx = np.divmod(np.arange(nsy * nsx), nsx)
    t = rng.random((nf, nsy * nsx, NCOL))          # the unread columns keep plain deviates
    u = rng.random((4, nf, nsy * nsx))
    t[:, :, 0], t[:, :, 1] = sx, sy
    t[:, :, 2] = np.floor(200 + 800 * rng.random((nf, nsy * nsx)))
    t[:, :, 5] = 1.4 + 0.3 * u[0]
    t[:, :, 6] = 0.012 + 0.006 * u[1]
    t[:, :, 7] = 0.015 + 0.007 * u[2]
    t[:, :, 10] = 0.0011 + 0.0009 * u[3]
    r = c["negative"][0] * nsx + c["negative"][1]
    t[:, r, 10] = -0.0003 - 0.0002 * u[3][:, r]
    if c["empty"] is not None:
        r = c["empty"][0] * nsx + c["empty"][1]
        t[:, r, 2] = 0
        t[0, r, 5:11] = 0.0                         # as solid-waffle leaves a superpixel it could not fit; the others keep garbage
    if c["nearly_empty"] is not None:
        r = c["nearly_empty"][0] * nsx + c["nearly_empty"][1]
        t[:-1, r, 2] = 0
        t[0, r, 5], t[0, r, 6] = np.nan, 1.0e9      # behind N = 0: never read
    return t


def write_summaries(dirpath, name):
    """The case as the files make_gain_file.py reads: ``<dirpath>/<name>_<k>_summary.txt`` (17 significant digits: np.loadtxt
    returns the same float64), their ``..._config.txt`` siblings, and the list file, whose path is returned with the list of
    summary paths and the text that belongs in ``notes.solid_waffle_config``."""
    t = inputs(name)
    paths, notes = [], []
    for k in range(t.shape[0]):
        p = os.path.join(dirpath, f"{name}_{k}_summary.txt")
        np.savetxt(p, t[k], fmt="%.17e")
        cfg = p[:-11] + "config.txt"
        lines = [f"DETECTOR: SCA{k}", "FORMAT: 4  ", f"NBIN: {CASES[name]['nsx']} {CASES[name]['nsy']}", ""]
        with open(cfg, "w") as f:
            f.write("\n".join(lines) + "\n")
        paths.append(p)
        notes.append("# " + cfg)
        notes.extend(s.rstrip() for s in lines)
    listfile = os.path.join(dirpath, f"{name}_summaries.txt")
    with open(listfile, "w") as f:
        f.write("\n".join(paths) + "\n")
    return listfile, paths, "\n".join(notes)
