"""tests/rawframes_ref.py against the reference's own lines (where its tree is present), the NaN table of small frame counts, and
the parts of romanimpreprocess_amd/calfiles/convert_frames.py that need no GPU: discovery, weights, header cards."""

import datetime
import hashlib
import os
import textwrap

import numpy as np
import pytest
import rawframes_ref as rr
from conftest import assert_same_bits

from romanimpreprocess_amd import calio
from romanimpreprocess_amd.calfiles import convert_frames

# the reference tree, where tools/make_goldens.py expects it too (or where ROMANIMPREPROCESS_REFERENCE says)
REFERENCE_RUN = os.path.join(os.environ.get("ROMANIMPREPROCESS_REFERENCE", "/root/reference"), "runs", "summer2025run")
_FULL = {}


def full_size_cube():
    """one random (1, 11, 4096, 4224) uint16 cube, shared: convert_dark takes its first 6 frames"""
    if "cube" not in _FULL:
        _FULL["cube"] = np.random.default_rng(5).integers(0, 65536, (1, 11, 4096, 4224), dtype=np.uint16)
    return _FULL["cube"]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).data).hexdigest()


# ------------------------------------------------------------------------------------------------ against the scripts
@pytest.mark.parametrize("sca", [3, 4])
@pytest.mark.parametrize("script, kind, N", [("convert_dark.py", "dark", 6), ("convert_flt.py", "flt", 11)])
def test_restatement_equals_the_scripts_own_lines(script, kind, N, sca):
    """the lines from "raw data was in Detector frame" to just before "write to a FITS file", read at test time and executed on a
    full-size cube (they hold the frame size): cube and float32 slopes have the digests of the restatement's"""
    path = os.path.join(REFERENCE_RUN, script)
    if not os.path.exists(path):
        pytest.skip("the reference tree is not present")
    with open(path) as f:
        lines = f.read().splitlines()
    first = next(i for i, s in enumerate(lines) if "raw data was in Detector frame" in s)
    last = next(i for i, s in enumerate(lines) if "write to a FITS file" in s)
    block = textwrap.dedent("\n".join(lines[first:last]))
    raw = np.ascontiguousarray(full_size_cube()[:, :N])
    ns = {"numpy": np, "cube": raw.copy(), "N": N, "sca": sca}
    with np.errstate(all="ignore"):
        exec(compile(block, script, "exec"), ns)   # noqa: S102 (the reference's own arithmetic, nothing of it is kept)
    want_cube, want_slp = digest(ns["cube"]), digest(ns["slp"].astype(np.float32))
    assert ns["cube"].shape == raw.shape and ns["cube"].dtype == np.uint16
    del ns
    cube = rr.orient_cube(raw, sca, 4096)
    assert digest(cube) == want_cube
    assert digest(rr.slopes(cube, rr.nc_of(kind, N))) == want_slp
    one = rr.orient_frame(raw[0, 2], 1 if sca % 3 == 0 else 2, 4096)   # the per-frame form the kernel tests use
    assert_same_bits(one, cube[0, 2])


# ------------------------------------------------------------------------------------------------ small frame counts
@pytest.mark.parametrize("N", range(1, 14))
def test_nan_table_and_exactness(N):
    rng = np.random.default_rng(N)
    cube = rng.integers(0, 65536, (1, N, 3, 9)).astype(np.uint16)
    cube[0, :, 0, 0], cube[0, :, 0, 1] = 0, 65535
    for Nc in sorted({N, min(N, 10)}):
        slp = rr.slopes(cube, Nc)
        nan0, nan1 = rr.nan_table(Nc)
        assert not np.isinf(slp).any()
        assert np.isnan(slp[0]).all() if nan0 else np.isfinite(slp[0]).all()
        assert np.isnan(slp[1]).all() if nan1 else np.isfinite(slp[1]).all()
        # the device's statement: host weights and denominators, the sum in ANY order (here backwards), one division, one cast
        w0, de0, w1, de1 = convert_frames.slope_weights(Nc)
        a0, a1 = np.zeros((3, 9)), np.zeros((3, 9))
        for k in range(Nc - 1, 0, -1):
            a0 = a0 + cube[0, k].astype(np.float64) * w0[k]
            if k < Nc // 2:
                a1 = a1 + cube[0, k].astype(np.float64) * w1[k]
        with np.errstate(all="ignore"):
            assert_same_bits((a0 / de0).astype(np.float32), slp[0], f"N {N} Nc {Nc} slp[0]")
            assert_same_bits((a1 / de1).astype(np.float32), slp[1], f"N {N} Nc {Nc} slp[1]")
        assert w0[0] == 0 and not w1[max(Nc // 2, 1):].any() and w1[0] == 0


def test_stored_forms_decode_to_the_samples():
    s = rr.frame_samples(5, 11)
    for stored in rr.STORED:
        assert_same_bits(rr.decode(rr.encode(s, stored), stored), s, f"stored {stored}")
    assert rr.encode(s, 1).dtype == np.dtype(">i2") and rr.encode(np.array([0, 65535], np.uint16), 1).tolist() == [-32768, 32767]
    assert rr.encode(np.array([32768, 65535], np.uint16), 2).tolist() == [-32768, -1]   # the bit pattern, kept


# ------------------------------------------------------------------------------------------------ discovery
def test_find_frames(tmp_path):
    names = ["linearity_exp3_a_SCU07_00B.fits", "linearity_exp3_a_SCU07_00A.fits", "linearity_exp3_a_SCU07_009.fits",
             "linearity_exp3_a_SCU07_00f.fits",
             "linearity_exp3_a_SCU07_00A_gw.fits",      # a guide-window file
             "linearity_exp3_a_SCU08_00A.fits",         # another detector
             "linearity_exp30_a_SCU07_00A.fits",        # exposure 30, not 3
             "Gain_exp3_a_SCU07_00A.fits",              # another prefix
             "linearity_exp3_a_SCU07_00A.fits.txt"]
    for n in names:
        (tmp_path / n).write_bytes(b"")
    got = convert_frames.find_frames(tmp_path, "linearity_exp", 3, 7)
    assert got == [str(tmp_path / n) for n in ("linearity_exp3_a_SCU07_009.fits", "linearity_exp3_a_SCU07_00A.fits",
                                               "linearity_exp3_a_SCU07_00B.fits", "linearity_exp3_a_SCU07_00f.fits")]
    assert got == sorted(got)
    assert convert_frames.find_frames(tmp_path, "linearity_exp", 30, 7) == [str(tmp_path / "linearity_exp30_a_SCU07_00A.fits")]
    assert convert_frames.find_frames(tmp_path, "Total_Noise_exp", 3, 7) == []
    assert convert_frames.find_frames(tmp_path, "linearity_exp", 3, 9) == []


# ------------------------------------------------------------------------------------------------ header cards
def test_header_cards_in_order_and_an_overlong_name_refused():
    N = 3
    files = [f"/data/in/linearity_exp1_x_SCU03_00{k}.fits" for k in range(N)]
    dates = [f"2025-07-0{k + 1}T01:02:03" for k in range(N)]
    now = datetime.datetime(2025, 8, 9, 10, 11, 12)
    cards = convert_frames.exposure_cards("convert_flt.py", N, files, dates, now)
    want = [("PROVEN", "convert_flt.py"), ("NMAX", 3), ("DATE", "2025-08-09 10:11:12")]
    for k in range(N):
        want += [(f"FR{k + 1:03d}", f"linearity_exp1_x_SCU03_00{k}.fits"), (f"FRD{k + 1:03d}", dates[k])]
    assert cards == want
    parsed = calio.parse_fits_header(calio.fits_header((1, N, 12, 32), np.uint16, extension=True, cards=cards))
    assert list(parsed)[-len(want):] == [k for k, _ in want]
    assert [parsed[k] for k, _ in want] == [v for _, v in want]
    assert parsed["BITPIX"] == 16 and parsed["BZERO"] == 32768 and [parsed[f"NAXIS{i}"] for i in (1, 2, 3, 4)] == [32, 12, N, 1]
    assert calio.parse_fits_header(calio.fits_header(None, None, cards=[("TGROUP", 3.04)]))["TGROUP"] == 3.04
    assert calio.parse_fits_header(calio.fits_header((2, 12, 32), np.float32, extension=True, cards=[("BUNIT", "DN/frame")]))["BUNIT"] == "DN/frame"
    assert convert_frames.exposure_cards("p", 1, ["/d/" + "a" * 63 + ".fits"], dates)[3][1] == "a" * 63 + ".fits"   # 68: fits
    long_name = "b" * 64 + ".fits"
    with pytest.raises(ValueError, match=long_name):
        convert_frames.exposure_cards("p", 2, [files[0], "/d/" + long_name], dates)
    assert isinstance(convert_frames.exposure_cards("p", 1, files, dates)[2][1], str)   # DATE: local time


def test_kinds_follow_the_scripts():
    k = convert_frames.KINDS
    assert k["dark"][:3] == ("Total_Noise_exp", "Noise", "convert_dark.py") and list(k["dark"][3]) == list(range(1, 101))
    assert k["flt"][:3] == ("linearity_exp", "Flat", "convert_flt.py") and list(k["flt"][3]) == list(range(1, 51))
    assert k["loflt"][:3] == ("Gain_exp", "LoFlat", "convert_loflt.py") and list(k["loflt"][3]) == list(range(1, 51))
    assert [k[n][4] for n in ("dark", "flt", "loflt")] == [False, True, True]
    with pytest.raises(ValueError, match="kind"):
        convert_frames.convert("bright", ".", 3, ".", 1)
