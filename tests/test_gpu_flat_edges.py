"""flatutils.get_flat (misc.hip: flat_prepare_kernel, then the embedded ipc4d stack and ipc_cube_kernel) against
oracle.finish.get_flat at the decision edges of the preparation: f32(0.1) and 10.0 of the flat, gain <= 0.1 in f32 and in f64,
the gain clip that happens only when a pixeldq is given, zeros, denormals and non-finite values, on frames of one 256-thread
block and of no whole number of them, down to an active region of 1 x 3.  Bit for bit (NaN where the restatement has NaN); no
tolerance.  The cases are satflag_cases.flat_case; test_host_satflag_cases.py asks of the restatement alone what makes them
mean something."""

import numpy as np
import pytest
import torch  # noqa: F401  before libromanhip is loaded: the first HIP runtime loaded must be the one both use
from conftest import assert_same_bits, gpu_context

import satflag_cases as sc
from oracle import finish
from romanimpreprocess_amd.utils import flatutils

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def _name(dt):
    return "f32" if dt == F32 else "f64"


@pytest.mark.parametrize("deconvolve", [True, False], ids=["ipc", "noipc"])
@pytest.mark.parametrize("with_pdq", [True, False], ids=["pdq", "nopdq"])
@pytest.mark.parametrize("kdt", [F32, F64], ids=["k32", "k64"])
@pytest.mark.parametrize("gdt", [F32, F64], ids=["g32", "g64"])
@pytest.mark.parametrize("frame", sc.FLAT_FRAMES, ids=[f"{ny}x{nx}_nb{nb}" for ny, nx, nb in sc.FLAT_FRAMES])
def test_get_flat_at_the_edges_of_the_preparation(frame, gdt, kdt, with_pdq, deconvolve):
    ny, nx, nb = frame
    c = sc.flat_case(ny, nx, nb, gdt, kdt)
    want_pdq = c["pixeldq"].copy() if with_pdq else None
    with np.errstate(all="ignore"):
        want = finish.get_flat(c["flat"], c["gain"], c["K"], nb, want_pdq, ipc_deconvolve=deconvolve)
    # the case's own conditions, on the numpy side, before the device is asked
    assert want.dtype == F32 and np.all(want[c["border"]] == 1.0)
    if with_pdq:
        flags = sc.flat_plant_flags(c)
        if not deconvolve:
            flags &= ~np.uint32(sc.NO_GAIN_VALUE)
        assert_same_bits(want_pdq, c["pixeldq"] | flags, "the restatement's flags vs the plants' own")
    caldir = {"flat": {"roman": {"data": c["flat"]}}, "gain": {"roman": {"data": c["gain"]}}, "ipc4d": {"roman": {"data": c["K"]}}}
    pdq = c["pixeldq"].copy() if with_pdq else None
    out = flatutils.get_flat(caldir, {"nborder": nb}, pdq, ipc_deconvolve=deconvolve, ctx=gpu_context())
    nan = np.isnan(want)
    ndiff = int(np.count_nonzero((out.view(np.uint32) != want.view(np.uint32)) & ~(nan & np.isnan(out))))
    nflag = 0 if pdq is None else int(np.count_nonzero(pdq != c["pixeldq"]))
    print(f"{ny}x{nx} nb {nb} gain {_name(gdt)} ipc4d {_name(kdt)} pdq {with_pdq} deconvolve {deconvolve}: {len(c['plants'])} plants, "
          f"{nflag} pixels flagged, {int(np.count_nonzero(nan))} NaN, {ndiff} differing words")
    assert_same_bits(np.isnan(out), nan, "NaN-ness")
    assert_same_bits(out, want, "flat")
    if with_pdq:
        assert_same_bits(pdq, want_pdq, "pixeldq")
    # the border comes out as 1, unflagged, whatever the arrays hold there
    assert np.all(out[c["border"]] == 1.0)
    if with_pdq:
        assert_same_bits(pdq[c["border"]], c["pixeldq"][c["border"]], "border flags")
