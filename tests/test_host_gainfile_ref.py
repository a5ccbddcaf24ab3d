"""CPU-only: tests/gainfile_ref.py, the closed-form numpy restatement of the gain / ipc4d derivation, against the fixtures
that the reference's own make_gain_file.py produced (tests/golden/gainfile_*.npz), bit for bit; the package's summary_means
against the same tables; and the new entry point's declaration."""

import ctypes
import os
import re

import gainfile_cases as gc
import gainfile_ref as gr
import numpy as np
import pytest
from conftest import REPO, assert_same_bits, load_golden

from romanimpreprocess_amd import _native, calfiles


@pytest.fixture(scope="module", params=list(gc.CASES))
def case(request):
    return request.param, gc.CASES[request.param], gc.inputs(request.param), load_golden(request.param)


def fixture_tables(g):
    return {e: g["mean_" + e] for e in gr.NAMES}, g["good"]


def test_ref_reproduces_the_fixture(case):
    name, c, tables, g = case
    shape = (c["nside"], c["nside"])
    means, good, tmean = gr.summary_means(tables)
    for e in gr.NAMES:
        assert_same_bits(means[e], g["mean_" + e], f"{name} mean {e}")
    assert_same_bits(good, g["good"], f"{name} good")
    assert_same_bits(np.array([tmean[e] for e in gr.NAMES]), g["tmean"], f"{name} tmean")
    gain, dq, kernel, kdq = gr.derive(means, good, shape, nb=gc.NB)
    assert_same_bits(gain, g["gain"], f"{name} gain")
    assert_same_bits(dq, g["gain_dq"], f"{name} gain dq")
    assert g["kernel"].shape == (3, 3, c["nside"] - 8, c["nside"] - 8) and g["kernel"].dtype == np.float64
    for j in range(9):
        assert_same_bits(kernel[j // 3, j % 3], g["kernel"][j // 3, j % 3], f"{name} K[{j // 3},{j % 3}]")
    assert_same_bits(kdq, g["kernel_dq"], f"{name} ipc4d dq")
    rows = [0, 5, c["nside"] - 9]   # chosen rows give the rows of the whole
    assert_same_bits(gr.ipc4d(means, shape, gc.NB, rows=rows), g["kernel"][:, :, rows], f"{name} rows")


def test_ref_float32_kernel_is_the_fixture_rounded_once(case):
    name, c, _, g = case
    means, _ = fixture_tables(g)
    k32 = gr.ipc4d(means, (c["nside"], c["nside"]), gc.NB, ipc_dtype=np.float32)
    assert_same_bits(k32, g["kernel"].astype(np.float32), f"{name} float32 kernel")


def test_summary_means_reproduces_the_fixture(case):
    name, c, tables, g = case
    means, good, tmean = calfiles.summary_means(tables)
    assert sorted(means) == sorted(gr.NAMES) and sorted(tmean) == sorted(gr.NAMES)
    for e in gr.NAMES:
        assert_same_bits(means[e], g["mean_" + e], f"{name} mean {e}")
        assert_same_bits(np.float64(tmean[e]), g["tmean"][gr.NAMES.index(e)], f"{name} tmean {e}")
    assert_same_bits(good, g["good"], f"{name} good")
    assert good.shape == (c["nsy"], c["nsx"])
    with pytest.raises(ValueError, match="superpixels"):
        calfiles.summary_means(tables[:, :-1])


def test_fixtures_hold_the_edges_they_are_meant_to():
    g, c = load_golden("gainfile_even"), gc.CASES["gainfile_even"]
    t = gc.inputs("gainfile_even")
    good = g["good"]
    assert not good[c["empty"]] and good[c["nearly_empty"]] and np.count_nonzero(~good) == 1
    for j, e in enumerate(gr.NAMES):   # the empty superpixel holds the array mean, the nearly empty one its last file's value
        assert g["mean_" + e][c["empty"]] == g["tmean"][j]
        assert g["mean_" + e][c["nearly_empty"]] == t[-1, c["nearly_empty"][0] * c["nsx"] + c["nearly_empty"][1], gr.COLS[e]]
    assert g["mean_aD"][c["negative"]] < 0 and np.isfinite(g["tmean"]).all()
    ry, rx = c["nside"] // c["nsy"], c["nside"] // c["nsx"]
    dq, gain = g["gain_dq"], g["gain"]
    assert rx % 2 == 1 and (dq[:4] == 2**19).all() and (dq[:, -4:] == 2**19).all() and (gain[-4:] == 0).all()
    y0, x0 = c["empty"][0] * ry, c["empty"][1] * rx
    assert (dq[y0:y0 + ry, x0:x0 + rx] == 2**19).all() and np.count_nonzero(dq[4:-4, 4:-4]) == ry * rx
    K = g["kernel"]
    assert not g["kernel_dq"].any()   # the script's all-zero convolution kernel: nothing is ever flagged
    assert (K[0, :, 0] == 0).all() and (K[2, :, -1] == 0).all() and (K[:, 0, :, 0] == 0).all() and (K[:, 2, :, -1] == 0).all()
    assert (K[0, 1, 1:] != 0).all() and (K[1, 0, :, 1:] != 0).all()
    assert np.abs(K.sum(axis=(0, 1)) - 1.0).max() <= 2 * np.finfo(np.float64).eps
    # across a seam the value is the mean of both sides: neither side's own
    xs = rx - 1 - gc.NB   # active column whose right neighbour lies in the next superpixel
    assert K[1, 2, 10, xs] != K[1, 2, 10, xs - 1] and K[1, 2, 10, xs] != K[1, 2, 10, xs + 1]
    assert_same_bits(K[1, 2, 10, xs], K[1, 0, 10, xs + 1], "symmetry across the seam")
    o = load_golden("gainfile_odd")
    assert o["kernel"].shape[-1] % 2 == 1 and o["good"].all()


def test_new_entry_is_declared_listed_and_exported():
    hdr = open(os.path.join(REPO, "include", "romanhip.h")).read()
    host = open(os.path.join(REPO, "romanimpreprocess_amd", "csrc", "rip_host.h")).read()
    mk = open(os.path.join(REPO, "romanimpreprocess_amd", "csrc", "Makefile")).read()
    assert re.search(r"\bint rip_cal_gain_ipc4d\(", hdr) and "#define RIP_VERSION 100 " in hdr
    assert "rip_cal_gain_ipc4d" in host and "gainfile.hip" in mk
    lib = _native.load_library()
    assert isinstance(lib.rip_cal_gain_ipc4d, ctypes._CFuncPtr)
    assert lib.rip_version() == 100
    assert len(_native.SYMBOLS["rip_cal_gain_ipc4d"][1]) == 14
