"""Host side of the bias state of a CALDIR set (``rip_caldir_bias_state``) and of the fused launch without a biascorr stream
(``rip_last_chain_bias_stream``): the C ABI and its Python mirror, and the f32 identity the change rests on.  No GPU."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
from conftest import REPO

from romanimpreprocess_amd import _native, pipeline

NEW = ("rip_caldir_bias_state", "rip_last_chain_bias_stream")


def _header():
    return open(os.path.join(REPO, "include", "romanhip.h")).read()


def test_new_queries_are_declared_bound_and_exported():
    hdr = _header()
    lib = _native.load_library()
    for name, args in zip(NEW, ([C.c_void_p, C.c_int], [C.c_void_p])):
        assert re.search(r"\bint\s+%s\s*\(rip_ctx \*ctx" % name, hdr), f"{name} is not declared in include/romanhip.h"
        assert _native.SYMBOLS[name] == (C.c_int, args), name
        assert hasattr(lib, name)
    for method in ("caldir_bias_state", "last_chain_bias_stream"):
        assert callable(getattr(_native.Context, method))
    assert callable(pipeline.Calibrator.bias_state)


def test_state_constants_match_the_header(tmp_path):
    """the three states as gcc reads them from the header == the Python constants"""
    src = tmp_path / "states.c"
    src.write_text('#include <stdio.h>\n#include "romanhip.h"\nint main(void){printf("%d %d %d %d\\n", RIP_BIAS_ABSENT, '
                   "RIP_BIAS_PRESENT, RIP_BIAS_DROPPED, RIP_VERSION);return 0;}\n")
    exe = tmp_path / "states"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got[:3] == [_native.BIAS_ABSENT, _native.BIAS_PRESENT, _native.BIAS_DROPPED]
    assert len(set(got[:3])) == 3
    assert got[3] == 100


def test_version_is_100():
    assert _native.load_library().rip_version() == 100
    assert re.search(r"#define\s+RIP_VERSION\s+100\b", _header())


def test_queries_refuse_a_null_context():
    lib = _native.load_library()
    assert lib.rip_caldir_bias_state(None, 0) == -1   # RIP_EINVAL
    assert lib.rip_last_chain_bias_stream(None) == -1


def test_subtracting_plus_zero_changes_no_bit_and_minus_zero_does():
    """x - (+0.0f) has the bits of x for every f32 -- what lets a set drop an all +0 biascorr, and the fused kernel take the 0 a
    dropped load returns for a bias sample -- while x - (-0.0f) turns an x of -0 into +0: why the test at upload is on bits."""
    f32 = np.float32
    tiny, big = np.finfo(f32).tiny, np.finfo(f32).max
    x = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, tiny / 2, -tiny / 2, tiny, -tiny, big, -big, 1.0, -1.5, 13000.25],
                 dtype=f32)
    assert np.signbit(x[1]) and np.isnan(x[4]) and x[5] > 0 and x[5] < tiny   # -0, NaN and denormals are really there
    with np.errstate(all="ignore"):
        same = x - f32(0.0)
        other = x - f32(-0.0)
    assert same.dtype == f32
    assert np.array_equal(same.view(np.uint32), x.view(np.uint32))
    differs = other.view(np.uint32) != x.view(np.uint32)
    assert differs[1] and other.view(np.uint32)[1] == 0, "-0 - (-0) is +0"
    assert not differs[np.arange(x.size) != 1].any()
    # the word a dropped load returns is +0.0f
    assert np.array([0], dtype=np.uint32).view(f32)[0] == 0.0 and not np.signbit(np.array([0], dtype=np.uint32).view(f32)[0])
