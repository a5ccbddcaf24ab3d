"""The arithmetic of the Level-1 synthesis at its edges: every kernel of synth.hip behind rip_synth_resultants, rip_synth_fill
and rip_synth_extract_ref, and invlin_kernel behind rip_stage_invlinearity, bit for bit against oracle/l1sim.py and
oracle/linearity.py (numpy, every deviate handed in) on the cases of synth_edge_cases.py.  No tolerance anywhere.

What the cases hold -- the ties, the clips, the planted read sequences, the coverage of the instantiation table -- is shown
without a GPU by test_host_synth_edge_cases.py."""

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: both bring a HIP runtime)
from conftest import assert_same_bits, gpu_context

import synth_edge_cases as sec
from romanimpreprocess_amd import _native
from romanimpreprocess_amd.from_sim import sim_to_isim

pytestmark = pytest.mark.gpu

F4, F8 = sec.F4, sec.F8


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _garbage(shape, dev):
    return torch.from_numpy(np.full(shape, sec.GARBAGE, np.uint16).view(np.int16)).to(dev)


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def _synth(c, channelwidth=None):
    return sim_to_isim.L1Synth(c["cal"], c["rp"], sec.READ_TIME, ctx=gpu_context(), nb=c["nb"],
                               channelwidth=channelwidth or c["nx"])


def _resultants(s, c, group_count=None):
    """rip_synth_resultants called directly, on output buffers that hold garbage: a cube of 0xA5A5, resultants and reset image
    of NaN.  Returns (start_e, resultants, cube) as numpy arrays."""
    reads_e, nr, nd = (_dev(c[k], s.dev) for k in ("reads_e", "n_reset", "n_read"))
    start = torch.full((s.nya, s.nxa), float("nan"), dtype=torch.float32, device=s.dev)
    res = torch.full((s.ngrp, s.nya, s.nxa), float("nan"), dtype=torch.float32, device=s.dev)
    cube = _garbage((s.ngrp, s.ny, s.nx), s.dev)
    torch.cuda.synchronize()     # torch's fills and copies are not on the context's stream
    try:
        s.ctx.call("rip_synth_resultants", s.desc, s.ngrp, s.group_count if group_count is None else group_count, reads_e, nr,
                   nd, 1, start, res, cube)
    finally:
        s.ctx.synchronize()
    return start.cpu().numpy(), res.cpu().numpy(), _u16(cube)


def _check_resultants(s, c):
    start, res, cube = _resultants(s, c)
    assert not np.isnan(start).any() and not np.isnan(res).any(), "an active pixel was not written"
    assert_same_bits(start, c["start"], "reset-noise image")
    assert_same_bits(res, c["want"], "resultants")
    nb, ny, nx = c["nb"], c["ny"], c["nx"]
    border = np.ones((ny, nx), bool)
    border[nb:ny - nb, nb:nx - nb] = False
    assert not cube[:, border].any(), "the border is not all zero"
    assert np.array_equal(cube, c["cube"])


# ---- 2. instantiations and geometry ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(sec.RES_TABLE)), ids=sec.res_id)
def test_resultants_every_plane_count_dtype_pair_and_geometry(i):
    """resultants_kernel<GT, KT, NP> at every NP = 2..17 over the four (gain, ipc4d) dtype pairs and a null ipc4d, reset_kernel
    with and without biascorr, zero_border_kernel at borders 4, 2 and 0 (not launched), frames narrower than a workgroup and
    with a partial one, three read patterns; outputs prefilled with garbage"""
    c = sec.resultants_case(i)
    s = _synth(c)
    assert s.desc.nplanes == sec.RES_TABLE[i][0]
    _check_resultants(s, c)


def test_resultants_refusals_leave_the_context_usable():
    c = sec.resultants_case(1)
    lin = c["cal"]["linearitylegendre"]
    for n in (1, 18):
        planes = np.concatenate([lin["data"]] * 9)[:n]
        bad = dict(c, cal=dict(c["cal"], linearitylegendre=dict(lin, data=np.ascontiguousarray(planes))))
        with pytest.raises(ValueError, match=rf"synth_resultants: {n} coefficient planes \(2\.\.17 supported\)"):
            _resultants(_synth(bad), bad)
    s = _synth(c)
    counts = s.group_count.copy()
    counts[-1] = 0
    with pytest.raises(ValueError, match=rf"synth_resultants: resultant {len(counts) - 1} has 0 reads"):
        _resultants(s, c, group_count=counts)
    _check_resultants(s, c)


# ---- 3. planted read sequences ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", range(len(sec.WARM_VARIANTS)))
def test_warm_bisection_on_planted_read_sequences(v):
    """rip_invlin_pixel_warm on reads that repeat, creep, jump, fall back and leave the series' range at both ends, among
    ordinary ramps in the same waves: the oracle evaluates every read on its own"""
    c = sec.warm_case(v)
    _check_resultants(_synth(c), c)


# ---- 4. ties and the clip --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", range(len(sec.TIE_VARIANTS)))
def test_resultants_round_half_even_and_clip_the_cube_only(v):
    c = sec.tie_clip_case(v)
    s = _synth(c)
    start, res, cube = _resultants(s, c)
    k = c["tie_k"]
    assert np.array_equal(res[:, sec.TIE_ROW, sec.TIE_COLS].astype(F8), k + k % 2), "a tie not rounded to even"
    assert_same_bits(start, c["start"], "reset-noise image")
    assert_same_bits(res, c["want"], "resultants")
    assert res.max() > 65535 and res.min() < 0          # unclipped here ...
    assert np.array_equal(cube, c["cube"])              # ... clipped there


# ---- 5. the fill -----------------------------------------------------------------------------------------------------------------
def _fill(c):
    s = _synth(c, channelwidth=c["cw"])
    assert (s.cw, s.nch) == (c["cw"], c["nx"] // c["cw"])
    cube = _dev(c["cube_in"].view(np.int16), s.dev)
    amp33 = _garbage((s.ngrp, s.ny, s.cw), s.dev) if c["with_amp33"] else None
    normals, frames, white33 = (None if c[k] is None else _dev(c[k], s.dev) for k in ("normals", "frames", "white33"))
    torch.cuda.synchronize()
    s.fill(cube, amp33, 1, banding=c["banding"], normals=normals, frames=frames, white33=white33)
    s.ctx.synchronize()
    return _u16(cube), None if amp33 is None else _u16(amp33)


def _check_fill(c, cube, amp33):
    assert np.array_equal(cube, c["cube_want"])
    if c["with_amp33"]:
        assert np.array_equal(amp33, c["amp33_want"])


@pytest.mark.parametrize("g", range(len(sec.FILL_GEOMETRIES)), ids=["%dx%dw%db%d" % f for f in sec.FILL_GEOMETRIES])
@pytest.mark.parametrize("call", sec.FILL_CALLS)
def test_fill_channel_counts_borders_ties_and_casts(g, call):
    """fill_kernel and amp33_kernel with 2, 3 and 32 channels and borders of 4 and 2; border pixels exactly at -5, the ties
    0.5 / 1.5 / 2.5 / 65534.5 / 65535.5 and 70000; reference-output levels below 0 and above 65535 (a C cast, not a clip)"""
    c = sec.fill_case(g, call)
    cube, amp33 = _fill(c)
    ny, nx, cw, nb = sec.FILL_GEOMETRIES[g]
    for y, x, i in sec.edge_pixels(ny, nx, cw):
        assert np.all(cube[:, y, x] == sec.EDGE_WANT[i]), (y, x, sec.EDGE_DARKS[i], cube[:, y, x])
    if not c["banding"]:
        act = (slice(None), slice(nb, ny - nb), slice(nb, nx - nb))
        assert np.array_equal(cube[act], c["cube_in"][act])
    if c["banding"] and c["with_amp33"]:
        for y, xc, i in sec.amp33_pixels():
            assert np.all(amp33[:, y, xc] == sec.AMP33_WANT[i]), (sec.AMP33_MEDS[i], amp33[:, y, xc])
    _check_fill(c, cube, amp33)


def test_fill_mirrors_the_odd_channel():
    c = sec.fill_mirror_case()
    cube, amp33 = _fill(c)
    cw = c["cw"]
    ch0, ch1 = cube[:, :, :cw].astype(np.int64), cube[:, :, cw:2 * cw].astype(np.int64)
    assert np.all(np.diff(ch0, axis=2) > 0)                 # the planted ramp ...
    assert np.array_equal(ch1, ch0[:, :, ::-1])             # ... runs the other way in channel 1
    u = float(c["cal"]["read"]["anc"]["U_PINK"])
    for j, grp in enumerate(c["rp"]):
        assert np.all(np.abs(ch1[j, :, 0] - ch0[j, :, 0] - sec.MIRROR_STEP * u / len(grp) ** 0.5 * (cw - 1)) <= 1)
    _check_fill(c, cube, amp33)


# ---- 6. EXTRACT_REF --------------------------------------------------------------------------------------------------------------
GUARD = 64


def _extract(ctx, dev, data, offset, want_ref):
    """the call on a tensor with GUARD elements of garbage on either side of the data and of the reference read"""
    ngrp, n = data.shape
    buf = np.full(ngrp * n + 2 * GUARD, sec.GARBAGE, np.uint16)
    buf[GUARD:GUARD + ngrp * n] = data.ravel()
    t = torch.from_numpy(buf.view(np.int16)).to(dev)
    r = _garbage((n + 2 * GUARD,), dev)
    torch.cuda.synchronize()
    ctx.call("rip_synth_extract_ref", t[GUARD:GUARD + ngrp * n], ngrp, n, offset, r[GUARD:GUARD + n] if want_ref else None)
    ctx.synchronize()
    got, ref = _u16(t), _u16(r)
    assert np.all(got[:GUARD] == sec.GARBAGE) and np.all(got[-GUARD:] == sec.GARBAGE), "written outside the data"
    assert np.all(ref[:GUARD] == sec.GARBAGE) and np.all(ref[-GUARD:] == sec.GARBAGE), "written outside the reference read"
    return got[GUARD:-GUARD].reshape(ngrp, n), ref[GUARD:-GUARD]


@pytest.mark.parametrize("n", sec.EXTRACT_N)
def test_extract_ref_sizes_group_counts_offsets_and_clips(n):
    ctx = gpu_context()
    dev = torch.device("cuda", ctx.device)
    for ngrp in sec.EXTRACT_NGRP:
        for offset in sec.EXTRACT_OFFSETS:
            c = sec.extract_case(n, ngrp, offset)
            got, ref = _extract(ctx, dev, c["data"], offset, True)
            assert np.array_equal(ref, c["ref"]), (ngrp, offset)
            assert np.array_equal(got[0], c["data"][0]) and np.array_equal(got[1:], c["rest"]), (ngrp, offset)


def test_extract_ref_without_a_reference_read():
    """reference_read = NULL: the later resultants are rescaled in place and nothing else is written"""
    ctx = gpu_context()
    dev = torch.device("cuda", ctx.device)
    c = sec.extract_case(257, 5, 1000)
    got, ref = _extract(ctx, dev, c["data"], 1000, False)
    assert np.all(ref == sec.GARBAGE)
    assert np.array_equal(got[0], c["data"][0]) and np.array_equal(got[1:], c["rest"])


# ---- 7. the stage entry of the inverse linearity ---------------------------------------------------------------------------------
def _invlin(ctx, c, coefs=None):
    t = c["target"]
    coefs = c["coefs"] if coefs is None else coefs
    ny, nx = t.shape
    S, ex = np.full_like(t, np.nan), np.full((ny, nx), 0xA5, np.uint8)
    ctx.call("rip_stage_invlinearity", np.ascontiguousarray(t), _native.dtype_code(t), ny, nx, coefs.shape[0],
             np.ascontiguousarray(coefs), np.ascontiguousarray(c["Smin"]), np.ascontiguousarray(c["Smax"]), S, ex)
    return S, ex


@pytest.mark.parametrize("dtype", [F4, F8], ids=["f32", "f64"])
@pytest.mark.parametrize("nplanes", range(2, 18))
def test_invlinearity_every_plane_count_in_f32_and_f64(nplanes, dtype):
    """invlin_kernel<ZT, NP> at every NP = 2..17 in both dtypes: targets far outside the series' range, infinite ones, and
    targets EQUAL to the series value at z = 0 and +-0.5 (the comparison is a strict <)"""
    c = sec.invlin_case(nplanes, dtype)
    S, ex = _invlin(gpu_context(), c)
    assert_same_bits(S, c["S"], "S")
    assert np.array_equal(ex, c["ex"].astype(np.uint8)) and not ex.any()


def test_invlinearity_refusals_leave_the_context_usable():
    ctx = gpu_context()
    c = sec.invlin_case(9, F8)
    for n in (1, 18):
        with pytest.raises(ValueError, match=rf"invlinearity: {n} coefficient planes \(2\.\.17 supported\)"):
            _invlin(ctx, c, np.concatenate([c["coefs"]] * 2)[:n])
    S, ex = _invlin(ctx, c)
    assert_same_bits(S, c["S"], "S")
