"""The noise-summary estimator without a GPU: tests/noise_run_ref.py (the numpy restatement of csrc/noisestat.hip) recovers the
parameters planted in its generator of dark frames -- the inverse of the reference's noise model -- and
calfiles/noisestack.noise_params, the package's own expression of the last step, agrees with it on the same tables; the command
line of calfiles/noise_run.py parses the job's line and refuses by name what it does not support.

Tolerances (profiles/noise_run.txt): 10 % for the four 1/f parameters (six seeds of the restatement: worst case 5.7 %); for ACN,
planted 0.6, four times the standard deviation the restatement showed over six seeds, 4 x 0.0156 = 0.0625 DN."""

import os
import re

import noise_run_ref as ref
import numpy as np
import pytest
from conftest import REPO

from romanimpreprocess_amd import _native
from romanimpreprocess_amd.calfiles import noise_run, noisestack

PLANTED, ACN, ACN_TOL, CASE, round_trip_case = ref.PLANTED, ref.ACN, ref.ACN_TOL, ref.CASE, ref.round_trip_case


def test_restatement_recovers_the_planted_parameters():
    got = round_trip_case()[1][-1]
    for k, want in PLANTED.items():
        print(k, got[k], want)
        assert abs(got[k] / want - 1) < 0.10, (k, got[k])
        assert abs(got[k] / want - 1) < 0.06, f"{k}: the committed seed must sit well inside the tolerance"
    print("ACN", got["ACN"])
    assert abs(got["ACN"] - ACN) < ACN_TOL


def test_noise_params_agrees_with_the_restatement():
    """two numpy expressions of the same rule on the same tables: reordering only"""
    c = CASE
    _, (_, _, tab, pl, _, want) = round_trip_case()
    vbar = float(np.mean(pl[4].astype(np.float64) ** 2))
    got = noisestack.noise_params(tab, c["N"], c["nreads"], c["ny"], c["C"], c["cw"], vbar)
    assert got.keys() == want.keys()
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-9), k
    # without a reference output: no M_PINK, RU_PINK; the rest unchanged
    tab2 = dict(tab, ht=None)
    tab2.update({k: tab[k][..., :c["C"]] for k in ("h1", "h2", "q1", "q2")})
    got2 = noisestack.noise_params(tab2, c["N"], c["nreads"], c["ny"], c["C"], c["cw"], vbar)
    assert sorted(got2) == ["ACN", "C_PINK", "U_PINK"] and all(got2[k] == got[k] for k in got2)
    with pytest.raises(ValueError, match="-n 1"):
        noisestack.noise_params(tab, 1, c["nreads"], c["ny"], c["C"], c["cw"], vbar)


def test_restatement_planes_recover_rate_noise_and_reset():
    cubes, (acc, rows, tab, pl, a33, _) = round_trip_case()
    c = CASE
    assert pl.shape == (6, c["ny"], c["C"] * c["cw"]) and a33.shape == (2, c["ny"], c["cw"]) and pl.dtype == a33.dtype == np.float32
    dark1, dark2, cds, reset = pl[0], pl[2], pl[4], pl[5]
    # 1.5 DN/frame planted.  Per pixel and exposure the slope of 8 frames has sigma 7.4 sqrt(12 / 504) = 1.1, d_0 7.4 sqrt 2; the
    # mean over 16 x 32768 of them, correlated within a frame by the 1/f terms only, stays far inside these
    assert abs(dark2.mean() * 3.04 - 1.5) < 0.05 and abs(dark1.mean() * 3.04 - 1.5) < 0.3
    # a sample's variance: white 5^2, alternating 0.6^2, and the 1/f series of unit amplitude has sum_{f=1}^{m/2} 1/f, m = 2 ny cw
    pixel = 25.0 + 0.36 + (1.5 ** 2 + 1.0) * (1.0 / np.arange(1, c["ny"] * c["cw"] + 1)).sum()
    assert abs(np.median(cds) / np.sqrt(2 * pixel) - 1) < 0.10
    assert abs(np.median(reset) / np.sqrt(400.0 + pixel) - 1) < 0.10   # the median of a 15-dof sample sigma is 2 % low
    assert abs(a33[0].mean() - 6000.0) < 1.0
    assert np.array_equal(a33[1], (ref.planes(acc, c["N"], c["nreads"], c["C"], c["cw"], True)[1][1]))
    # the row sums are what they say
    x = cubes[-1].astype(np.uint32)
    assert np.array_equal(rows[-1][:, :, 2, 1], x[:, :, 2 * c["cw"] + 1:3 * c["cw"]:2].sum(-1))
    assert ref.scales(128) == 1 and ref.scales(255) == 1 and ref.scales(256) == 2 and ref.scales(4096) == 6 and ref.scales(1 << 15) == 6
    assert [noisestack.scales(v) for v in (128, 255, 256, 4096, 1 << 15)] == [1, 1, 2, 6, 6]


# ------------------------------------------------------------------------------------------------ the command line
JOB = "-f 1 -i /d/99999999_SCA01_Noise_001.fits -o /d/noise_SCA01.fits -n 100 -t 3 -cd 5.0 -rh 7 -tn 34 -ro".split()


def test_the_jobs_line_parses():
    a = noise_run.parse(JOB)
    assert (a.format, a.first, a.out, a.ndark, a.tstart, a.cdscut, a.rowover, a.nframe, a.ref_out, a.tframe) == \
        (1, "/d/99999999_SCA01_Noise_001.fits", "/d/noise_SCA01.fits", 100, 3, 5.0, 7, 34, True, 3.04)
    b = noise_run.parse([w for w in JOB if w != "-ro"] + ["--tframe", "2.5"])
    assert b.ref_out is False and b.tframe == 2.5 and b.nframe == 34 and b.tstart == 3
    assert noise_run.geometry(4224) == (32, 128) and noise_run.geometry(4096) == (32, 128) and noise_run.geometry(83, 64, 16) == (4, 16)


def _with(opt, value):
    line = list(JOB)
    line[line.index(opt) + 1] = value
    return line


@pytest.mark.parametrize("line, text", [
    (_with("-f", "2"), "-f 2"), (_with("-n", "1"), "-n 1"), (_with("-n", "513"), "-n 513"), (_with("-t", "0"), "-t 0"),
    (_with("-tn", "1"), "-tn 1"), (_with("-tn", "65"), "-tn 65"), (JOB + ["--tframe", "0"], "--tframe"),
])
def test_the_command_line_refuses_by_name(line, text):
    with pytest.raises(ValueError, match=re.escape(text)):
        noise_run.parse(line)


def test_geometry_refusals_name_the_option():
    ok = dict(ny=128, nx_file=80, C=4, cw=16, f0=1, n=5, ref_out=True)
    noisestack.check_geometry(**ok)
    for kw, text in (({"n": 1}, "-tn 1"), ({"n": 65}, "-tn 65"), ({"f0": -1}, "-t 0"), ({"cw": 15}, "channel width 15"),
                     ({"cw": 258}, "channel width 258"), ({"ny": 127}, "127 rows"), ({"nx_file": 79}, "frame of 79"),
                     ({"C": 0}, "0 channels")):
        with pytest.raises(ValueError, match=text):
            noisestack.check_geometry(**dict(ok, **kw))
    noisestack.check_geometry(**dict(ok, ref_out=False, nx_file=64))


def test_new_entries_are_declared_bound_and_listed():
    hdr = open(os.path.join(REPO, "include", "romanhip.h")).read()
    host = open(os.path.join(REPO, "romanimpreprocess_amd", "csrc", "rip_host.h")).read()
    mk = open(os.path.join(REPO, "romanimpreprocess_amd", "csrc", "Makefile")).read()
    for name in ("rip_cal_noise_add", "rip_cal_noise_rowstats", "rip_cal_noise_planes"):
        assert re.search(rf"\bint {name}\(", hdr) and name in _native.SYMBOLS and name in host, name
    assert "noisestat.hip" in mk and "65535 n^2 / 2" in hdr and "parity with solid-waffle is unpinned" in hdr
