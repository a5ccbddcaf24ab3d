"""The numpy restatement of the L2-output stage (tests/l2_out_ref.py) against hand-written literals, and the list of members the
reference's three helpers add to the L2 tree.  Needs no GPU."""

import l2_out_ref as lr
import numpy as np


def bits16(a):
    return [int(v) for v in np.asarray(a, np.float16).reshape(-1).view(np.uint16)]


def test_one_active_pixel():
    """9 x 9 with a border of 4: the active region is pixel (4, 4)"""
    slope = np.arange(81, dtype=np.float32).reshape(9, 9)
    er, ep = np.full((9, 9), 7.0, np.float32), np.full((9, 9), 11.0, np.float32)
    er[4, 4], ep[4, 4] = 3.0, 4.0
    pdq = (np.arange(81, dtype=np.uint32) * np.uint32(0x01010101)).reshape(9, 9)
    out = lr.l2_planes(slope, er, ep, pdq, 4)
    assert {k: v.shape for k, v in out.items()} == {
        "data": (1, 1), "dq": (1, 1), "var_rnoise": (1, 1), "var_poisson": (1, 1), "err": (1, 1), "dq_border_ref_pix_left": (9, 4),
        "dq_border_ref_pix_right": (9, 4), "dq_border_ref_pix_top": (4, 9), "dq_border_ref_pix_bottom": (4, 9)}
    assert out["data"].tolist() == [[40.0]] and out["dq"].tolist() == [[40 * 0x01010101]]
    assert out["var_rnoise"].tolist() == [[9.0]] and out["var_poisson"].tolist() == [[16.0]] and out["err"].tolist() == [[5.0]]
    assert all(out[k].dtype == np.float32 for k in ("data", "var_rnoise", "var_poisson", "err")) and out["dq"].dtype == np.uint32
    f = 0x01010101
    assert out["dq_border_ref_pix_left"][2].tolist() == [18 * f, 19 * f, 20 * f, 21 * f]
    assert out["dq_border_ref_pix_right"][2].tolist() == [23 * f, 24 * f, 25 * f, 26 * f]
    assert out["dq_border_ref_pix_top"][:, 0].tolist() == [45 * f, 54 * f, 63 * f, 72 * f]      # the LAST four rows
    assert out["dq_border_ref_pix_bottom"][:, 8].tolist() == [8 * f, 17 * f, 26 * f, 35 * f]    # the first four, corner included
    assert out["dq_border_ref_pix_top"][3, 8] == out["dq_border_ref_pix_right"][8, 3] == 80 * f   # a corner is in both


def test_cube_strips_and_their_corners():
    cube = np.arange(5 * 6 * 7, dtype=np.uint16).reshape(5, 6, 7)
    cube[0, 0, 0], cube[4, 5, 6] = 65535, 0
    out = lr.refpix_strips(cube, 2)
    assert {k: v.shape for k, v in out.items()} == {"border_ref_pix_left": (5, 6, 2), "border_ref_pix_right": (5, 6, 2),
                                                    "border_ref_pix_top": (5, 2, 7), "border_ref_pix_bottom": (5, 2, 7)}
    assert all(v.dtype == np.float32 and v.flags.c_contiguous for v in out.values())
    left, right, top, bottom = (out[f"border_ref_pix_{s}"] for s in lr.SIDES)
    assert left[0, 0].tolist() == [65535.0, 1.0] and left[4, 5].tolist() == [203.0, 204.0]
    assert right[0, 0].tolist() == [5.0, 6.0] and right[4, 5].tolist() == [208.0, 0.0]
    assert top[0, :, 0].tolist() == [28.0, 35.0] and top[4, :, 6].tolist() == [202.0, 0.0]          # rows 4 and 5
    assert bottom[0, :, 0].tolist() == [65535.0, 7.0] and bottom[4, :, 6].tolist() == [174.0, 181.0]   # rows 0 and 1
    assert bottom[1, 1, 6] == right[1, 1, 1] == 42 + 13
    # float32 samples pass unchanged; no border, no strip
    f = lr.refpix_strips(cube.astype(np.float32) + np.float32(0.5), 2)
    assert f["border_ref_pix_right"][0, 0].tolist() == [5.5, 6.5]
    assert lr.refpix_strips(cube, 0)["border_ref_pix_top"].shape == (5, 0, 7)


def test_float16_rounding():
    """err = sqrt(er^2 + 0) = er exactly for these er; var_rnoise = er^2"""
    er = np.zeros((3, 11), np.float32)
    row = [2049.0, 2051.0, 65504.0, 65519.0, 65520.0, 2.0 ** -12, 3 * 2.0 ** -13, 2.0 ** -13, 0.0, np.nan, np.inf]
    er[1] = row
    out = lr.l2_planes(np.zeros_like(er), er, np.zeros_like(er), np.zeros(er.shape, np.uint32), 0, float16=True)
    assert out["err"].dtype == out["var_rnoise"].dtype == out["var_poisson"].dtype == np.float16 and out["data"].dtype == np.float32
    assert out["err"].shape == (3, 11)
    err = out["err"][1]
    # ties go to the even significand: 2049 -> 2048, 2051 -> 2052; 65504 is the largest float16, 65520 is the tie with 2^16 -> inf
    assert err[:5].tolist() == [2048.0, 2052.0, 65504.0, 65504.0, np.inf]
    assert bits16(err[:5]) == [0x6800, 0x6802, 0x7BFF, 0x7BFF, 0x7C00]
    assert bits16(err[5:9]) == [0x0C00, 0x0E00, 0x0800, 0x0000]   # 2^-12, 1.5 * 2^-12, 2^-13: normal float16 values
    assert np.isnan(err[9]) and np.isposinf(err[10])
    var = out["var_rnoise"][1]
    assert np.all(np.isposinf(var[:5]))                    # 2049^2 is beyond float16
    assert bits16(var[5:9]) == [0x0001, 0x0002, 0x0000, 0x0000]   # 2^-24 is the smallest subnormal; 2.25 * 2^-24 -> 2 * 2^-24; 2^-26 -> 0
    assert np.isnan(var[9]) and np.isposinf(var[10]) and not out["var_poisson"].any()


def test_float32_edge_values():
    er = np.array([[0.0, -0.0, 1e-30, 1e-23, 1e-20, 3e19, np.nan, np.inf]], np.float32)
    out = lr.l2_planes(np.zeros_like(er), er, er[:, ::-1].copy(), np.zeros(er.shape, np.uint32), 0)
    v = out["var_rnoise"][0]
    assert v[0] == 0 and v[1] == 0 and not np.signbit(v[1])           # (-0)^2 = +0
    assert v[2] == 0 and v[3] == 0                                     # 1e-60 and 1e-46 underflow (the smallest subnormal is 1.4e-45)
    assert v[4].view(np.uint32) == 71362 and np.isposinf(v[5])          # 1e-40: a subnormal, 71362 * 2^-149; 9e38 overflows
    assert np.isnan(v[6]) and np.isposinf(v[7])
    e = out["err"][0]   # err_poisson runs the other way: inf, nan, 3e19, 1e-20, 1e-23, ...
    assert np.isposinf(e[0]) and np.isnan(e[1]) and np.isposinf(e[2]) and np.isnan(e[6]) and np.isposinf(e[7])
    # sqrt(0 + 1e-40) and sqrt(1e-40 + 0): the root of the subnormal 71362 * 2^-149, 9.999973e-21 (a float64 root rounded once
    # more to float32 is the correctly rounded float32 root: 53 >= 2 * 24 + 2 bits)
    root = np.float32(np.sqrt(np.float64(71362) * 2.0 ** -149))
    assert e[3] == root and e[4] == root and abs(float(root) / 9.999973e-21 - 1) < 1e-6


def test_members_the_reference_adds():
    assert lr.REFERENCE_ADDED_ROMAN_KEYS == [
        "amp33", "border_ref_pix_left", "border_ref_pix_right", "border_ref_pix_top", "border_ref_pix_bottom",
        "dq_border_ref_pix_left", "dq_border_ref_pix_right", "dq_border_ref_pix_top", "dq_border_ref_pix_bottom", "chisq", "dumo"]
    cube = np.arange(2 * 10 * 12, dtype=np.uint16).reshape(2, 10, 12)
    pdq = np.arange(120, dtype=np.uint32).reshape(10, 12)
    roman, meta = lr.new_members(cube, pdq, 4, (2, 4), "9.9.9")
    assert sorted(roman) == sorted(k for k in lr.REFERENCE_ADDED_ROMAN_KEYS if k != "amp33")
    assert roman["chisq"].dtype == roman["dumo"].dtype == np.float16 and roman["chisq"].shape == (2, 4) and not roman["dumo"].any()
    assert roman["border_ref_pix_top"].shape == (2, 4, 12) and roman["border_ref_pix_top"][1, 0, 0] == 120 + 72
    assert roman["dq_border_ref_pix_right"].dtype == np.uint32 and roman["dq_border_ref_pix_right"][9].tolist() == [116, 117, 118, 119]
    assert meta == {"calibration_software_name": "gen_cal_image / HLWAS PIT", "calibration_software_version": "romanimpreprocess_amd 9.9.9",
                    "dummyfields": ["roman.chisq", "roman.dumo"]}
    assert list(meta) == lr.REFERENCE_ADDED_META_KEYS


def test_same_bits_leaves_a_nan_open_and_nothing_else():
    import pytest

    a = np.array([0x7FC00000, 0x00000000], np.uint32).view(np.float32)
    lr.same_bits(a, np.array([0xFFC12345, 0x00000000], np.uint32).view(np.float32))
    with pytest.raises(AssertionError):
        lr.same_bits(a, np.array([0x7FC00000, 0x80000000], np.uint32).view(np.float32))   # -0 is not +0
    with pytest.raises(AssertionError):
        lr.same_bits(a, np.array([0.0, 0.0], np.float32))
    with pytest.raises(AssertionError):
        lr.same_bits(a, a.astype(np.float64))
