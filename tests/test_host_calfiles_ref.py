"""CPU-only: tests/calfiles_ref.py, the numpy restatement of the calibration-file derivation, against the fixtures that the
reference's own postprocess_calfiles.py and makemask.py produced (tests/golden/calfiles_*.npz), bit for bit; and the READS /
xref / t0 bookkeeping of the package against hand values."""

import os
import re

import calfiles_cases as cc
import calfiles_ref as cr
import numpy as np
import pytest
from conftest import REPO, assert_same_bits, load_golden

from romanimpreprocess_amd import calfiles, pars
from romanimpreprocess_amd.calfiles import postprocess_calfiles as pc


@pytest.fixture(scope="module", params=list(cc.CASES))
def case(request):
    return request.param, cc.inputs(request.param), load_golden(request.param)


def test_ref_biascorr_reproduces_the_fixture(case):
    name, a, g = case
    bc, pred, t0 = cr.biascorr(a["dark_slope"], a["dark_data"], a["lin_data"], a["Smin"], a["Smax"], g["reads"],
                               tframe=float(g["tframe"]), bframe=int(g["bframe"]), nb=cc.NB)
    assert_same_bits(pred, g["pred"], f"{name} pred")
    assert_same_bits(bc, g["biascorr"], f"{name} biascorr")
    assert t0 == float(g["t0"]) and cr.parse_reads(g["reads"], int(g["bframe"]))[1] == float(g["xref"])


def test_ref_pflat_saturation_mask_reproduce_the_fixture(case):
    name, a, g = case
    assert float(g["g_ideal"]) == pars.g_ideal
    data, dq, coef = cr.pflat(g["pflat0"], g["gain"], pars.g_ideal)
    assert_same_bits(data, g["pflat_data"], f"{name} pflat")
    assert_same_bits(dq, g["pflat_dq"], f"{name} pflat dq")
    np.testing.assert_allclose(coef, g["pflat_coefs"], rtol=1e-12, atol=0)   # the same LAPACK solve on the same medians
    sat, sdq = cr.saturation(a["Smax"], a["Sref"])
    assert_same_bits(sat, g["sat_data"], f"{name} saturation")
    assert_same_bits(sdq, g["sat_dq"], f"{name} saturation dq")
    assert_same_bits(cr.mask(a["lin_dq"], g["pflat0"], a["dark_slope"], a["gain_dq"], nb=cc.NB), g["mask_dq"], f"{name} mask")


def test_fixtures_hold_the_edges_they_are_meant_to():
    """the planted pixels do what their comments say, in the reference's own outputs"""
    g = load_golden("calfiles_p9_prod")
    a = cc.inputs("calfiles_p9_prod")
    lo, hi = np.float32(0.01), np.float32(1.99)
    p, dq = g["pflat_data"], g["pflat_dq"]
    assert np.count_nonzero((p[0] == lo) & (dq[0] == 0)) >= 1 and np.count_nonzero((p[0] == lo) & (dq[0] == 1)) >= 1
    assert np.count_nonzero((p[-1] == hi) & (dq[-1] == 0)) >= 1 and np.count_nonzero((p[-1] == hi) & (dq[-1] == 1)) >= 1
    assert np.isnan(p[20, 50]) and dq[20, 50] == 0 and dq[20, 51] == 1 and dq[20, 52] == 1
    n = load_golden("calfiles_p11_gaps")   # one NaN in the gain plane: everything NaN and unflagged
    assert np.isnan(n["pflat_data"]).all() and not n["pflat_dq"].any()
    m = g["mask_dq"]
    assert m[12, 30] & 0x1800 == 0 and m[12, 32] & 0x1800 == 0x1000 and m[12, 31] & 0x1800 == 0x1000 and m[12, 33] & 0x1800 == 0x800
    assert m[0, 0] >> 31 == 1 and m[cc.NB, cc.NB] >> 31 == 0
    assert not (m & 0x2000).any()   # the p-flat holds NaNs: its median is NaN and nothing is LOW_QE; without NaNs:
    assert np.count_nonzero(load_golden("calfiles_p4_g16")["mask_dq"] & 0x2000) > 10
    s, sdq = g["sat_data"], g["sat_dq"]
    assert s[13, 40] == 0 and s[13, 41] == 65534 and np.isnan(s[13, 42]) and sdq[13, 42] == 1 and sdq[13, 43] == 1
    assert s[13, 44] == 0 and s[13, 45] == 65534
    ya, xa = cc.HOT[0] - cc.NB, cc.HOT[1] - cc.NB   # the hot pixel: Smin + eps below xref, Smax - eps above, NaN at x == xref
    lo_s, hi_s = a["Smin"][cc.HOT], a["Smax"][cc.HOT]
    half = (hi_s - lo_s) / np.float32(2)
    assert g["pred"][0, ya, xa] == lo_s + half * (np.float32(1) + np.float32(-1 + 2.0**-24))
    assert g["pred"][2, ya, xa] == lo_s + half * (np.float32(1) + np.float32(1 - 2.0**-24))
    assert np.isfinite(g["pred"][1, ya, xa])   # inf * 0 would be NaN; 3e4 * 0 is 0: an ordinary target
    # a NaN target compares false at every step: the bisection runs down to Smin + eps, as for -inf
    assert_same_bits(g["pred"][0, 10 - cc.NB, 23 - cc.NB], a["Smin"][10, 23] + (a["Smax"][10, 23] - a["Smin"][10, 23]) / np.float32(2)
                     * (np.float32(1) + np.float32(-1 + 2.0**-24)), "NaN dark slope")


def test_reads_parsing_against_hand_values():
    r, ngrp, xref = calfiles.parse_reads(cc.READS_PROD, 1)
    assert (ngrp, xref, r.dtype, r.size) == (8, 1.0, np.int32, 16)
    assert calfiles.parse_reads(cc.READS_PROD, 0)[2] == 0.0
    assert calfiles.parse_reads(cc.READS_PROD, 4)[2] == 17.5          # reads 10..25
    assert calfiles.parse_reads(cc.READS_GAPS, 0)[2] == 0.5            # a 2-read bias group: a half-integer
    assert calfiles.parse_reads(cc.READS_GAPS, 4)[2] == 16.0
    assert calfiles.parse_reads([0, 1, 1, 2, 5], 1)[1] == 2            # an odd tail is ignored, as len(READS) // 2 does
    for bad in (-1, 8):
        with pytest.raises(ValueError):
            calfiles.parse_reads(cc.READS_PROD, bad)
    from romanimpreprocess_amd import synth
    assert calfiles.reads_of_pattern(synth.READ_PATTERN_8) == cc.READS_PROD
    assert calfiles.reads_of_pattern(synth.READ_PATTERN_16) == cc.READS_16
    assert pc.frame_pars({}) == (3.04, 1) and pc.frame_pars({"TFRAME": "3.08", "BIAS": {"SLICE": 2}}) == (3.08, 2)
    assert pc.frame_pars({"BIAS": {}}) == (3.04, 1)
    for name, c in cc.CASES.items():
        g = load_golden(name)
        tframe, bframe = pc.frame_pars(c["lpars"])
        assert tframe * calfiles.parse_reads(c["reads"], bframe)[2] == float(g["t0"]), name
    assert 3.04 * 1.0 == float(load_golden("calfiles_p9_prod")["t0"])


def test_new_entries_are_declared_and_listed():
    hdr = open(os.path.join(REPO, "include", "romanhip.h")).read()
    host = open(os.path.join(REPO, "romanimpreprocess_amd", "csrc", "rip_host.h")).read()
    assert "calibration-file derivation" in hdr
    for name in ("rip_cal_biascorr", "rip_cal_pflat", "rip_cal_saturation", "rip_cal_mask"):
        assert re.search(rf"\bint {name}\(", hdr), name
    assert "rip_cal_biascorr, _pflat, _saturation" in host
