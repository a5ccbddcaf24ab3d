"""The reference-pixel image drop-ins (reference_subtraction.ref_subtraction_row / ref_subtraction_channel / row_medians, and
rip_stage_refpix_row / _channel / _image under them) at small and odd frames against the numpy oracle (oracle/refpix.py),
bit for bit: every count at which the in-LDS median of csrc/refpix.hip takes another path (odd, padded, below, at and over
the block size, the 128 KiB limits), every update form, and values a sort can get wrong (ties, signed zeros, infinities,
NaN).  The cases and what they exercise: refpix_dropin_cases.py; test_host_refpix_dropin_cases.py proves them on the CPU.
"""

import numpy as np
import pytest
from conftest import assert_same_bits, gpu_context

import refpix_dropin_cases as rc
from oracle import refpix as orp
from romanimpreprocess_amd import _native
from romanimpreprocess_amd.utils import reference_subtraction as rs

pytestmark = pytest.mark.gpu

MODES = {np.float64: _native.RIP_ROW_SLOPE_F64, np.float32: _native.RIP_ROW_SLOPE_F32, float: _native.RIP_ROW_SLOPE_F32}


def _status(ctx, name, *args):
    """the library's return code of entry `name`, not raised"""
    return getattr(ctx.lib, name)(*_native.marshal(name, (ctx.h,) + args))


# ---------------------------------------------------------------------------------------------------------------- row step
@pytest.mark.parametrize("name", [c.name for c in rc.ROW_CASES])
def test_row_step(name):
    """ref_subtraction_row / row_medians and rip_stage_refpix_row (image, ref_med, sci_med, ctr) against oracle.refpix.row_step"""
    c = rc.ROW_BY_NAME[name]
    ctx = gpu_context()
    img0 = rc.row_image(c)
    ny, w = img0.shape
    want, want_ref, want_sci, want_ctr, slope = rc.row_oracle(c, img0)
    ref, sci, ctr = np.empty(ny, np.float32), np.empty(ny, np.float32), np.empty(1, np.float32)
    if c.form == "medians":
        img = img0.copy()
        m_ref, m_sci, m_ctr = rs.row_medians(img, use_ref_channel=c.use_ref, nside=c.nside, ctx=ctx)
        assert_same_bits(img, img0, "row_medians: image untouched")
        assert_same_bits(m_ref, want_ref, "row_medians: ref_med")
        assert_same_bits(m_sci, want_sci, "row_medians: sci_med")
        assert_same_bits(m_ctr, want_ctr, "row_medians: ctr")
        m_ref, none, m_ctr = rs.row_medians(img, use_ref_channel=c.use_ref, nside=c.nside, science=False, ctx=ctx)
        assert none is None
        assert_same_bits(m_ref, want_ref, "row_medians(science=False): ref_med")
        assert_same_bits(m_ctr, want_ctr, "row_medians(science=False): ctr")
        mode, s = _native.RIP_ROW_MEDIANS_ONLY, 0.0
    else:
        img = img0.copy()
        out = rs.ref_subtraction_row(img, use_ref_channel=c.use_ref, slope=rc.ROW_SLOPES[c.form], nside=c.nside, ctx=ctx)
        assert out is img
        assert_same_bits(img, want, "ref_subtraction_row: image")
        mode, s = MODES[type(slope)], float(slope)
    img = img0.copy()
    ctx.call("rip_stage_refpix_row", img, ny, w, c.nside, c.use_ref, mode, s, ref, sci, ctr)
    assert_same_bits(img, want, "rip_stage_refpix_row: image")
    assert_same_bits(ref, want_ref, "rip_stage_refpix_row: ref_med")
    assert_same_bits(sci, want_sci, "rip_stage_refpix_row: sci_med")
    assert_same_bits(ctr[0], want_ctr, "rip_stage_refpix_row: ctr")
    if ny == 1:   # ctr is the single median: every pixel comes back as x - 0
        assert_same_bits(ref[0], want_ctr, "ny = 1: ctr is the row's median")
        assert np.array_equal(img, img0)


# ------------------------------------------------------------------------------------------------------------ channel step
@pytest.mark.parametrize("name", [c.name for c in rc.CHAN_CASES])
def test_channel_step(name):
    """ref_subtraction_channel and rip_stage_refpix_channel against oracle.refpix.channel_step: (a) with the oracle's LAPACK lines
    handed in, image and medians bit for bit; (b) with the device's own line, bit for bit against the two-point formula restated
    in float64, and against the LAPACK result within the tolerance of test_ref_subtraction_default_arguments"""
    c = rc.CHAN_BY_NAME[name]
    ctx = gpu_context()
    img0 = rc.chan_image(c)
    ny, w = img0.shape
    nwin = rc.chan_windows(c)
    kw = dict(channel_start=c.start, channel_end=c.end, use_ref_channel=c.use_ref, n_channels=c.n_channels, ctx=ctx)
    want_a, table = rc.chan_oracle(c, img0)
    lines = np.ascontiguousarray(table[:, 2:4])
    # (a)
    img, bt = img0.copy(), np.empty((nwin, 2), np.float32)
    ctx.call("rip_stage_refpix_channel", img, ny, w, c.start, c.end, nwin, lines, bt)
    assert_same_bits(bt, table[:, :2].astype(np.float32), "LAPACK lines: bottom_top")
    assert_same_bits(img, want_a, "LAPACK lines: image")
    img = img0.copy()
    assert rs.ref_subtraction_channel(img, lines=lines, **kw) is img
    assert_same_bits(img, want_a, "ref_subtraction_channel(lines=): image")
    # (b)
    want_b, table_b = rc.channel_step_two_point(img0.copy(), c.start, c.end, nwin)
    img = rs.ref_subtraction_channel(img0.copy(), **kw)
    assert_same_bits(img, want_b, "ref_subtraction_channel: image vs the two-point line")
    np.testing.assert_allclose(img, want_a, rtol=1e-5, atol=1e-4)
    img = img0.copy()
    ctx.call("rip_stage_refpix_channel", img, ny, w, c.start, c.end, nwin, None, bt)
    assert_same_bits(img, want_b, "rip_stage_refpix_channel: image vs the two-point line")
    assert_same_bits(bt, table_b[:, :2].astype(np.float32), "rip_stage_refpix_channel: bottom_top")


# ------------------------------------------------------------------------------------------------- rip_stage_refpix_image
@pytest.mark.parametrize("ny,nx,do_row,do_chan", rc.IMAGE_CASES)
def test_refpix_image(ny, nx, do_row, do_chan):
    """rip_stage_refpix_image against row_step followed by channel_step: ref_med, ctr, bottom_top out, lines in and not"""
    ctx = gpu_context()
    img0 = rc.image_case_image(ny, nx)
    nch = nx // 128 + 1
    work = img0.copy()
    want_ref = want_ctr = None
    if do_row:
        work, want_ref, want_ctr = orp.row_step(work, nx, True, rc.IMAGE_SLOPE)
    after_row = work.copy()
    lines = None
    if do_chan:
        work, table = orp.channel_step(work, nx, True)
        lines = np.ascontiguousarray(table[:, 2:4])
    for ln in ((lines, None) if do_chan else (None,)):
        want, want_bt = work, (table[:, :2].astype(np.float32) if do_chan else None)
        if do_chan and ln is None:
            want, tb = rc.channel_step_two_point(after_row.copy(), 0, 128, nch)
            want_bt = tb[:, :2].astype(np.float32)
        img = img0.copy()
        ref, ctr, bt = np.full(ny, 77, np.float32), np.full(1, 77, np.float32), np.full((nch, 2), 77, np.float32)
        ctx.call("rip_stage_refpix_image", img, ny, nx, float(rc.IMAGE_SLOPE), do_row, do_chan, ln, ref, ctr, bt)
        assert_same_bits(img, want, "image")
        if do_row:
            assert_same_bits(ref, want_ref, "ref_med")
            assert_same_bits(ctr[0], want_ctr, "ctr")
        else:   # outputs of a step that did not run are left alone
            assert np.all(ref == 77) and ctr[0] == 77
        if do_chan:
            assert_same_bits(bt, want_bt, "bottom_top")
            if ln is None:
                np.testing.assert_allclose(img, work, rtol=1e-5, atol=1e-4)
        else:
            assert np.all(bt == 77)


# ------------------------------------------------------------------------------------------------ limits the code accepts
def test_limit_ctr_over_32768_rows():
    """ny = 32768, nside = 16: the sort of the row medians takes 128 KiB of dynamic LDS; one row more is refused"""
    ctx = gpu_context()
    ny, nside = rc.LIMIT_ROW_NY["ny"], rc.LIMIT_ROW_NY["nside"]
    img0 = rc.limit_image(ny, nside, 1)
    want, want_ref, want_ctr = orp.row_step(img0.copy(), nside, False, np.float64(0.3371))
    img = rs.ref_subtraction_row(img0.copy(), slope=np.float64(0.3371), nside=nside, ctx=ctx)
    assert_same_bits(img, want, "image")
    ref, _, ctr = rs.row_medians(img0, nside=nside, science=False, ctx=ctx)
    assert_same_bits(ref, want_ref, "ref_med")
    assert_same_bits(ctr, want_ctr, "ctr")
    over = np.zeros((ny + 1, nside), np.float32)
    assert _status(ctx, "rip_stage_refpix_row", over, ny + 1, nside, nside, False, _native.RIP_ROW_MEDIANS_ONLY, 0.0, None, None,
                   None) == _native.RIP_EINVAL
    with pytest.raises(ValueError):
        rs.ref_subtraction_row(over, slope=0.5, nside=nside, ctx=ctx)


def test_limit_science_medians_over_32768_pixels():
    """nside = 32776, ny = 8: the science medians take 128 KiB of LDS; one column more is refused"""
    ctx = gpu_context()
    ny, nside = rc.LIMIT_ROW_NSIDE["ny"], rc.LIMIT_ROW_NSIDE["nside"]
    img0 = rc.limit_image(ny, nside, 2)
    ref, sci, ctr = rs.row_medians(img0, nside=nside, ctx=ctx)
    _, want_ref, want_ctr = orp.row_step(img0.copy(), nside, False, 0.0)
    assert_same_bits(sci, np.median(img0[:, 4:nside - 4], axis=1), "sci_med")
    assert_same_bits(ref, want_ref, "ref_med")
    assert_same_bits(ctr, want_ctr, "ctr")
    over = np.zeros((ny, nside + 1), np.float32)
    sci = np.empty(ny, np.float32)
    assert _status(ctx, "rip_stage_refpix_row", over, ny, nside + 1, nside + 1, False, _native.RIP_ROW_MEDIANS_ONLY, 0.0, None, sci,
                   None) == _native.RIP_EINVAL
    with pytest.raises(ValueError):
        rs.row_medians(over, nside=nside + 1, ctx=ctx)


def test_limit_window_of_8192_columns():
    """window (0, 8192), ny = 8, one window: 4 x 8192 values; a window of 8193 columns is refused"""
    ctx = gpu_context()
    ny, start, end = (rc.LIMIT_CHAN_WINDOW[k] for k in ("ny", "start", "end"))
    img0 = rc.limit_image(ny, end, 3)
    want, table = orp.channel_step(img0.copy(), end, False, start, end, n_channels=1)
    img, bt = img0.copy(), np.empty((1, 2), np.float32)
    ctx.call("rip_stage_refpix_channel", img, ny, end, start, end, 1, np.ascontiguousarray(table[:, 2:4]), bt)
    assert_same_bits(bt, table[:, :2].astype(np.float32), "bottom_top")
    assert_same_bits(img, want, "image")
    want_b, _ = rc.channel_step_two_point(img0.copy(), start, end, 1)
    img = rs.ref_subtraction_channel(img0.copy(), start, end, n_channels=1, ctx=ctx)
    assert_same_bits(img, want_b, "image vs the two-point line")
    over = np.zeros((ny, end + 1), np.float32)
    assert _status(ctx, "rip_stage_refpix_channel", over, ny, end + 1, start, end + 1, 1, None, None) == _native.RIP_EINVAL
    with pytest.raises(ValueError):
        rs.ref_subtraction_channel(over, start, end + 1, n_channels=1, ctx=ctx)


def test_refusals():
    """what the library and the wrapper refuse: ny = 7 for the channel step, frames and windows that do not fit, lines of the
    wrong shape, images that are not C-contiguous float32"""
    ctx = gpu_context()
    img = rc.limit_image(7, 128, 4)
    assert _status(ctx, "rip_stage_refpix_channel", img, 7, 128, 0, 128, 1, None, None) == _native.RIP_EINVAL
    with pytest.raises(ValueError):
        rs.ref_subtraction_channel(img, n_channels=1, ctx=ctx)
    img = rc.limit_image(8, 160, 5)
    keep = img.copy()
    for kw in (dict(nside=15), dict(nside=161), dict(nside=33, use_ref_channel=True)):
        with pytest.raises(ValueError):
            rs.ref_subtraction_row(img, slope=0.5, ctx=ctx, **kw)
        with pytest.raises(ValueError):
            rs.row_medians(img, ctx=ctx, **kw)
        ns, ref = kw["nside"], bool(kw.get("use_ref_channel"))
        assert _status(ctx, "rip_stage_refpix_row", img, 8, 160, ns, ref, _native.RIP_ROW_SLOPE_F32, 0.5, None, None,
                       None) == _native.RIP_EINVAL
    for kw in (dict(n_channels=2), dict(n_channels=1, use_ref_channel=True), dict(channel_end=161, n_channels=1),
               dict(channel_start=-1, n_channels=1), dict(channel_start=8, channel_end=8, n_channels=1)):
        with pytest.raises(ValueError):
            rs.ref_subtraction_channel(img, ctx=ctx, **kw)
    for lines in (np.zeros((2, 2)), np.zeros(2), np.zeros((1, 3))):
        with pytest.raises(ValueError):
            rs.ref_subtraction_channel(img, n_channels=1, lines=lines, ctx=ctx)
    assert_same_bits(img, keep, "a refused call leaves the image alone")
    for bad in (img.astype(np.float64), img[:, ::2], img.T, img[0]):
        with pytest.raises(TypeError):
            rs.ref_subtraction_row(bad, slope=0.5, nside=16, ctx=ctx)
        with pytest.raises(TypeError):
            rs.ref_subtraction_channel(bad, n_channels=1, ctx=ctx)
        with pytest.raises(TypeError):
            rs.row_medians(bad, nside=16, ctx=ctx)
