"""Inputs of the calibration-file cases (tests/golden/calfiles_*.npz, tools/make_goldens.py case `calfiles`): a small
linearitylegendre / dark / gain set per case, made from seeded uniform deviates with IEEE arithmetic only (no libm call), so
that every machine regenerates the same bits.  The frame is 44 x 140 with a border of 4: 36 x 132 = 4752 active pixels (no
multiple of 64 or 256, more than one workgroup, rows that are no multiple of the wave width), and 44 // 6 = 7, 140 // 6 = 23
give medfit(N=6) blocks with a remainder on both axes (row 0, row 43, column 0 and column 139 lie outside every block).

The p-flat and gain planes a case's p-flat / mask outputs were computed from are stored IN the fixture (`pflat0`, `gain`):
tools/make_goldens.py plants pixels that land exactly on the 0.01 and 1.99 limits after the division by the reference's own
model, which only it can know."""

import numpy as np

NY, NX, NB = 44, 140, 4

READS_PROD = [0, 1, 1, 2, 2, 4, 4, 10, 10, 26, 26, 32, 32, 34, 34, 35]                    # the production 8-group table: 35 reads
_B16 = [0, 1, 2, 3, 4, 6, 8, 10, 13, 16, 19, 22, 25, 28, 31, 34, 35]
READS_16 = [v for i in range(16) for v in (_B16[i], _B16[i + 1])]
READS_GAPS = [0, 2, 3, 4, 6, 10, 12, 13, 13, 20]                                          # skipped reads, a 2-read bias group
READS_SINGLE = [0, 1, 1, 2, 3, 4, 7, 8, 15, 16, 16, 17]                                   # every group a single read

# name -> seed, Legendre planes, READS, the linearity_pars json, how the gain plane is made
CASES = {
    "calfiles_p9_prod": dict(seed=301, nplanes=9, reads=READS_PROD, lpars={}, gain="border"),
    "calfiles_p4_g16": dict(seed=302, nplanes=4, reads=READS_16, lpars={"TFRAME": 3.08, "BIAS": {"SLICE": 2}}, gain="plain"),
    "calfiles_p11_gaps": dict(seed=303, nplanes=11, reads=READS_GAPS, lpars={"BIAS": {"SLICE": 0}}, gain="nan"),
    "calfiles_p9_single": dict(seed=304, nplanes=9, reads=READS_SINGLE, lpars={"BIAS": {}}, gain="border"),
}

# planted pixels of the bias correction, full-frame (row, column)
HOT = (10, 22)          # its targets leave the range on both sides of xref: the bisection runs to +-(1 - 2^-24)
NAN_COEF = (11, 20)
SMAX_EQ_SMIN = (11, 21)
SMAX_LT_SMIN = (11, 22)


def frame_pars(lpars):
    tframe, bframe = 3.04, 1
    if "TFRAME" in lpars:
        tframe = float(lpars["TFRAME"])
    if "BIAS" in lpars and "SLICE" in lpars["BIAS"]:
        bframe = int(lpars["BIAS"]["SLICE"])
    return tframe, bframe


def inputs(name):
    """dict of the case's arrays: lin_data (nplanes,ny,nx), Smin, Smax, Sref, lin_dq, pflat (1,ny,nx), dark_slope, dark_data
    (ngrp,ny,nx), gain, gain_dq -- float32 / uint32 as the reference's files hold them."""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    ny, nx, nb, npl = NY, NX, NB, c["nplanes"]
    ngrp = len(c["reads"]) // 2
    tframe, _ = frame_pars(c["lpars"])
    y, x = np.mgrid[0:ny, 0:nx]
    u = lambda: rng.random((ny, nx))  # noqa: E731

    smin = (4500 + 1000 * u()).astype(np.float32)
    smax = (56000 + 9000 * u()).astype(np.float32)
    sref = (smin + 300 + 100 * (x % 2)).astype(np.float32)
    coefs = np.zeros((npl, ny, nx), np.float32)
    if npl > 2:
        coefs[2] = 20 + 180 * u()
    for L in range(3, npl):
        coefs[L] = (2.0 / L**2) * (2 * u() - 1)
    zref = 2 * (sref.astype(np.float64) - smin) / (smax.astype(np.float64) - smin) - 1
    c1 = (smax.astype(np.float64) - smin) / 2.0 - 3 * coefs[2].astype(np.float64) * zref
    coefs[1] = c1
    coefs[0] = -(c1 * zref) - coefs[2].astype(np.float64) * (1.5 * zref * zref - 0.5)

    v = u()
    dark_slope = (0.005 + 2.0 * v * v * v * v).astype(np.float32)
    for sl in ((slice(None), slice(0, nb)), (slice(None), slice(nx - nb, nx)), (slice(0, nb), slice(None)),
               (slice(ny - nb, ny), slice(None))):
        dark_slope[sl] = 0.0
    dark_slope[10, 20], dark_slope[10, 21] = -0.7, 0.0
    dark_slope[HOT] = 3.0e4
    dark_slope[10, 23], dark_slope[10, 24], dark_slope[10, 25] = np.nan, np.inf, -np.inf
    dark_slope[12, 30], dark_slope[12, 31] = 0.25, 12.5            # exactly on the mask's warm and hot limits
    dark_slope[12, 32], dark_slope[12, 33] = np.nextafter(np.float32(0.25), np.float32(1)), np.nextafter(np.float32(12.5), np.float32(99))
    coefs[2][NAN_COEF] = np.nan
    smax[SMAX_EQ_SMIN] = smin[SMAX_EQ_SMIN]
    smax[SMAX_LT_SMIN] = smin[SMAX_LT_SMIN] - np.float32(100)
    # the saturation file's edges: Smax below 1, above 65535, NaN, equal to Sref
    smax[13, 40], smax[13, 41], smax[13, 42] = 0.25, 70000.0, np.nan
    smax[13, 43] = sref[13, 43]
    smax[13, 44], smax[13, 45] = 1.0, 65535.0

    t = np.array([tframe * (c["reads"][2 * j] + c["reads"][2 * j + 1] - 1) / 2.0 for j in range(ngrp)])
    with np.errstate(all="ignore"):
        dark_data = np.stack([13000 + 200 * u() + dark_slope.astype(np.float64) * t[j] for j in range(ngrp)]).astype(np.float32)

    pflat = (0.9 + 0.1 * x / nx - 0.2 * (y / ny * (1 - y / ny)) + 0.02 * (u() - 0.5)).astype(np.float32)
    pflat[rng.random((ny, nx)) < 0.01] = 0.2            # low QE
    pflat[20, 51], pflat[20, 52] = -0.5, 4.0
    if c["gain"] != "plain":                             # ("plain": no NaN, so makemask's median is finite and LOW_QE is set)
        pflat[20, 50] = np.nan
        pflat[1:8, 1:24] = np.nan                        # one block of medfit(N=6) is empty
    gain = (1.3 + 0.2 * u()).astype(np.float32)   # median 1.4: g_ideal / median > 1, so 1.99 is reached from below 2
    if c["gain"] in ("border", "nan"):                   # zero border: the median still sits in the interior
        gain[:nb], gain[-nb:], gain[:, :nb], gain[:, -nb:] = 0, 0, 0, 0
    if c["gain"] == "nan":                               # one NaN: np.median is NaN, the whole p-flat NaN and unflagged
        gain[30, 100] = np.nan
    lin_dq = np.where(rng.random((ny, nx)) < 0.01, 2**20, 0).astype(np.uint32)
    gain_dq = np.where(rng.random((ny, nx)) < 0.01, 2**19, 0).astype(np.uint32)
    return {"lin_data": coefs, "Smin": smin, "Smax": smax, "Sref": sref, "lin_dq": lin_dq, "pflat": pflat[None].copy(),
            "dark_slope": dark_slope, "dark_data": dark_data, "gain": gain, "gain_dq": gain_dq}
