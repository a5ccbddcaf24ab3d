"""The HIP stage kernels at the ends of their domain, against oracle/ bit for bit (stage_limit_cases.py builds the inputs,
test_host_stage_limits.py checks the cases and the oracle at these shapes without a GPU).

The stage kernels run every ramp of more than 16 groups, every Legendre order other than 3, 8 or 10, and the function-level
drop-ins.  Here: ramps of 17 to 64 groups through fitting.ramp_fit / fitting.jump_detect (both sides of the 48 KiB steps of
their dynamic LDS: hipFuncSetAttribute above 32 resp. 48 groups, 96 KiB at 64) and through the whole chain; Legendre sets of
1 to 32 planes; ipc_cube_kernel with the active edge on tile seams, on the frame edge, inside a frame smaller than a tile and
behind borders of 8 and 15; ipc_rev to orders 1 to 5 (both parities of the image path's buffer ping-pong).

Float planes are compared with zero_sign_ok=True as in test_gpu_stages.py, flags exactly.  The GPU work of every case is
milliseconds; the wall time is the numpy oracle's, computed once per case and shared by the variants.  Measured on an MI355X
host: the whole module 35 to 40 s, of which the two 64-group ramp_fit cases take 11 s (f32 gain) and 9 s (f64 gain) -- the
oracle's 60 truncated refits of up to 63 groups; they are kept for the 96 KiB launch -- then 49 and 48 groups 3.6 s and 3.3 s,
the chain at 33 groups 1.2 s, and every other case less than a second."""

import numpy as np
import pytest
import torch  # noqa: F401  before libromanhip is loaded: the first HIP runtime loaded must be the one both use
from chain_support import assert_oracle, chain_context, loaded, oracle_lines
from conftest import assert_same_bits, gpu_context

import oracle
import stage_limit_cases as slc
from oracle import ipc as oipc
from oracle import linearity as olin
from oracle import rampfit as orf
from romanimpreprocess_amd import _native, pipeline, synth
from romanimpreprocess_amd import plan as planmod
from romanimpreprocess_amd.utils import fitting, ipc_linearity
from romanimpreprocess_amd.utils.processlog import ProcessLog

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
INF = float("inf")


def _name(dt):
    return {None: "none", F32: "f32", F64: "f64"}[dt]


# ---- fitting.ramp_fit, 17 to 64 groups -----------------------------------------------------------------------------------------
def _caldir(c):
    return {"gain": {"roman": {"data": c["gain"]}}, "read": {"roman": {"data": c["read"]}}}


def _device_meta(c):
    """meta as the package's own host code makes it; it must be the oracle's, bit for bit"""
    meta = planmod.exposure_meta(c["read_pattern"], synth.FRAME_TIME)
    meta["nborder"] = slc.NB
    meta["K"] = fitting.construct_weights(0.4 / 1.8 / 6.5**2, meta, exclude_first=c["exclude_first"])
    for k in ("K", "tbar", "tau", "N"):
        assert_same_bits(meta[k], c["meta"][k], k)
    return meta


# (G, f64 gain, guard_band, exclude_first)
RAMP_FIT = ([(G, False, 1e-5, True) for G in slc.LONG_COUNTS] + [(33, True, 1e-5, True), (64, True, 1e-5, True)]
            + [(17, False, INF, True), (33, False, INF, True), (17, False, 1e-5, False)])


@pytest.mark.parametrize("G,gain64,guard,exclude_first", RAMP_FIT,
                         ids=[f"g{G}_{'g64' if g64 else 'g32'}_guard{gd:g}_start{int(ef)}" for G, g64, gd, ef in RAMP_FIT])
def test_ramp_fit_long_ramps(G, gain64, guard, exclude_first):
    """every truncated variant is fitted by some pixel of the staircase (a wrong k_ofs / diff_ofs at the tail of the plan's
    tables shows), jumps are flagged in the full ramp and inside the longest, a middle and the shortest truncated variant"""
    res = slc.oracle_ramp_fit(G, gain64, exclude_first)
    slc.assert_long_ramp_conditions(res, need_truncated=True)
    c = res["case"]
    assert c["gain"].dtype == (F64 if gain64 else F32)
    meta = _device_meta(c)
    ctx = gpu_context()
    rdq, pdq = c["groupdq"].copy(), c["pixeldq"].copy()
    ctx.set_option_f64("guard_band", guard)
    try:
        slope, er, ep = fitting.ramp_fit(c["data"], rdq, pdq, meta, _caldir(c), ProcessLog(), exclude_first=exclude_first, ctx=ctx)
    finally:
        ctx.set_option_f64("guard_band", 1e-5)
    assert_same_bits(rdq, res["groupdq"], "groupdq")
    assert_same_bits(pdq, res["pixeldq"], "pixeldq")
    assert_same_bits(slope, res["slope"], "slope", zero_sign_ok=True)
    assert_same_bits(er, res["err_read"], "err_read", zero_sign_ok=True)
    assert_same_bits(ep, res["err_poisson"], "err_poisson", zero_sign_ok=True)


# ---- fitting.jump_detect, 17 to 64 groups --------------------------------------------------------------------------------------
JUMP_DETECT = [(17, None), (48, None), (49, None), (64, None), (49, 48), (49, 3)]


@pytest.mark.parametrize("G,truncate", JUMP_DETECT, ids=[f"g{G}" + (f"_t{t}" if t else "") for G, t in JUMP_DETECT])
def test_jump_detect_long_ramps(G, truncate):
    c = slc.long_ramp_case(G)
    meta = _device_meta(c)
    want_flags = np.zeros_like(c["groupdq"])
    diag = {}
    with np.errstate(all="ignore"):
        ws, wer, wep, wsmap = orf.fit_and_flag(c["data"], want_flags, c["gain"], c["read"], c["meta"], slc.NB, True, truncate,
                                               None, diag=diag)
    g = G if truncate is None else truncate
    act = (slice(slc.NB, -slc.NB), slice(slc.NB, -slc.NB))
    assert wsmap.shape[0] == 2 * (g - 1) - 3 and diag["sthresh"].shape == ws.shape
    assert np.count_nonzero(wsmap[(slice(None),) + act] > diag["sthresh"][act]) > 0      # the pass does flag something here
    assert np.count_nonzero(want_flags) > 0 and not np.any(want_flags[g:])
    loc = np.zeros_like(c["groupdq"])
    s, er, ep, smap = fitting.jump_detect(c["data"], loc, c["pixeldq"], meta, _caldir(c), ProcessLog(), exclude_first=True,
                                          truncate_ramp=truncate, ctx=gpu_context())
    assert_same_bits(s, ws, "slope", zero_sign_ok=True)
    assert_same_bits(er, wer, "err_read", zero_sign_ok=True)
    assert_same_bits(ep, wep, "err_poisson", zero_sign_ok=True)
    assert smap.shape == wsmap.shape
    for k in range(smap.shape[0]):
        assert_same_bits(smap[k], wsmap[k], f"smap plane {k}", zero_sign_ok=True)
    assert_same_bits(loc, want_flags, "flags")


# ---- the chain on the stage route ----------------------------------------------------------------------------------------------
STAGE_ROUTE = 0   # rip_chain_form_for / rip_last_chain_form: 0 = the stage kernels, 2 = the fused kernel


@pytest.mark.parametrize("G,p_order", [(17, 5), (33, 3)])
def test_chain_of_long_ramps_takes_the_stage_kernels_and_matches_the_oracle(G, p_order):
    ny, nx = 40, 128
    rp = slc.long_read_pattern(G)
    cal = synth.make_caldir(ny, nx, read_pattern=rp, p_order=p_order, seed=61, bias_amplitude=1.0, bad_lin_frac=0.01)
    ramp = synth.make_ramp(cal, read_pattern=rp, seed=62, cr_frac=0.03)
    with np.errstate(all="ignore"):
        ref = oracle.calibrate_arrays(ramp, cal)
    assert np.count_nonzero(ref["pixeldq"] & slc.JUMP) > 5 and np.count_nonzero(ref["pixeldq"] & slc.SAT) > 5
    assert np.count_nonzero(ref["pixeldq"] & olin.NO_LIN_CORR) > 0
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), 8, cal) as cb:
        assert cb.chain_form_for(8, G) == STAGE_ROUTE
        # a long ramp is no fused form whatever the Legendre order and the dtypes
        for planes in (4, 9, 11):
            for kdt in (_native.RIP_F32, _native.RIP_F64):
                assert _native.chain_form_for(planes, G, kdt) == STAGE_ROUTE
        got = cb.calibrate(8, ramp, want_cube=True, channel_lines=oracle_lines(ref, G, nx // 128))
        assert ctx.last_chain_form() == STAGE_ROUTE, "a fused form was chosen for a ramp of more than 16 groups"
    assert_oracle(got, ref, "stage kernels", cube=True)


def test_65_groups_are_refused_by_name():
    """RIP_MAX_GROUPS is 64: rip_plan_create and rip_calibrate name the count they refuse, and the context stays usable"""
    assert _native.RIP_MAX_GROUPS == 64
    ctx = chain_context()
    c = slc.long_ramp_case(17)
    meta = _device_meta(c)
    with pytest.raises(ValueError, match="too many groups"):   # the Python side stops before it overruns the descriptor's arrays
        planmod.plan_desc({"ngrp": 65}, None)
    desc = planmod.plan_desc(meta, meta["K"], True, True, None)
    desc.ngrp = 65
    with pytest.raises(ValueError, match="plan: 65 groups unsupported"):
        ctx.create_plan(desc)
    ny, nx = 40, 128
    rp = slc.long_read_pattern(17)
    cal = synth.make_caldir(ny, nx, read_pattern=rp, p_order=3, seed=61)
    with loaded(pipeline.Calibrator(ctx=ctx), 8, cal) as cb:
        pid, _ = cb.plan_for(rp, synth.FRAME_TIME)
        with pytest.raises(ValueError, match="calibrate: 65 groups unsupported"):
            cb.calibrate_device(8, pid, 65, None, True, None, None, None, None, None, None, None)
        ramp = synth.make_ramp(cal, read_pattern=rp, seed=62, cr_frac=0.03)
        got = cb.calibrate(8, ramp)      # the next call succeeds
        assert ctx.last_chain_form() == STAGE_ROUTE and np.all(np.isfinite(got["slope"]))


# ---- ipc_linearity.multilin, 1 to 32 planes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_attempt", [False, True], ids=["all_groups", "attempt_corr"])
@pytest.mark.parametrize("dnff", [True, False], ids=["first_clipped", "first_flagged"])
@pytest.mark.parametrize("nplanes", slc.LIN_PLANES)
def test_multilin_plane_counts(nplanes, dnff, with_attempt):
    """1 plane: the loop of rip_legendre_series never runs; 2 planes: no recurrence term is used; 32: the LDS maximum.  The
    planted samples at Smin, Smax and across the f32 rounding of z decide `ex`, the clip of group 0 and NO_LIN_CORR."""
    c = slc.legendre_case(nplanes)
    ac = c["attempt_corr"] if with_attempt else None
    want_phi, want_dq = olin.multilin(c["S"], c["coefs"], c["Smin"], c["Smax"], c["Sref"], c["lin_dq"], do_not_flag_first=dnff,
                                      attempt_corr=ac)
    new = (want_dq & ~c["lin_dq"] & olin.NO_LIN_CORR) != 0
    assert 10 < np.count_nonzero(new) < new.size
    phi, dq = ipc_linearity.multilin(c["S"], slc.lin_file(c), do_not_flag_first=dnff, attempt_corr=ac, ctx=gpu_context())
    assert_same_bits(phi, want_phi, "phi", zero_sign_ok=True)
    assert_same_bits(dq, want_dq, "dq")


@pytest.mark.parametrize("nplanes", slc.LIN_PLANES)
def test_multilin_plane_counts_on_a_window(nplanes):
    c = slc.legendre_case(nplanes)
    want_phi, want_dq = olin.multilin(c["S"], c["coefs"], c["Smin"], c["Smax"], c["Sref"], c["lin_dq"], attempt_corr=c["attempt_corr"])
    win = (slice(None), slice(1, 20), slice(3, 38))     # holds planted samples of both groups
    assert sum(1 for _, y, x, _ in c["plants"] if 1 <= y < 20 and 3 <= x < 38) >= 8
    phi, dq = ipc_linearity.multilin(c["S"][win], slc.lin_file(c), origin=(3, 1), attempt_corr=c["attempt_corr"][win], ctx=gpu_context())
    assert_same_bits(phi, want_phi[win], "phi window", zero_sign_ok=True)
    assert_same_bits(dq, want_dq[win[1:]], "dq window")


@pytest.mark.parametrize("nplanes", [0, 33])
def test_multilin_refuses_0_and_33_planes_and_the_context_goes_on(nplanes):
    c = slc.legendre_case(3)
    ny, nx = slc.LIN_SHAPE
    bad = dict(slc.lin_file(c)["roman"], data=np.zeros((nplanes, ny, nx), F32))
    ctx = gpu_context()
    with pytest.raises(ValueError, match=f"linearity: {nplanes} Legendre planes unsupported"):
        ipc_linearity.multilin(c["S"], {"roman": bad}, ctx=ctx)
    want_phi, want_dq = olin.multilin(c["S"], c["coefs"], c["Smin"], c["Smax"], c["Sref"], c["lin_dq"])
    phi, dq = ipc_linearity.multilin(c["S"], slc.lin_file(c), ctx=ctx)
    assert_same_bits(phi, want_phi, "phi after the refusal", zero_sign_ok=True)
    assert_same_bits(dq, want_dq, "dq after the refusal")


# ---- ipc_linearity.correct_cube on the six geometries --------------------------------------------------------------------------
CUBE_CASES = ([(f, k, g) for f in slc.IPC_MIXED for k in (F32, F64) for g in (None, F32, F64)]
              + [(f, F32, F32) for f in slc.IPC_FRAMES if f not in slc.IPC_MIXED])


@pytest.mark.parametrize("frame,kdt,gdt", CUBE_CASES, ids=[f"{f[0]}x{f[1]}_nb{f[2]}_k{_name(k)}_g{_name(g)}" for f, k, g in CUBE_CASES])
def test_correct_cube_geometries(frame, kdt, gdt):
    ny, nx, nb = frame
    c = slc.ipc_geometry_case(ny, nx, nb, kdt, gdt)
    want = oipc.correct_cube(c["cube"].copy(), c["K"], c["gain"])
    cube = c["cube"].copy()
    log = ProcessLog()
    ipc_linearity.correct_cube(cube, {"roman": {"data": c["K"]}}, log,
                               gain_file=None if c["gain"] is None else {"roman": {"data": c["gain"]}}, ctx=gpu_context())
    assert f"excluding {nb:d} border pixels" in log.output
    border = np.ones((ny, nx), bool)
    border[nb:ny - nb, nb:nx - nb] = False
    assert np.count_nonzero(border) == ny * nx - (ny - 2 * nb) * (nx - 2 * nb)
    assert_same_bits(cube[:, border], c["cube"][:, border], "border")
    assert np.count_nonzero(cube[:, ~border] != c["cube"][:, ~border]) > 0.9 * c["cube"][:, ~border].size
    assert_same_bits(cube, want, "correct_cube", zero_sign_ok=True)


# ---- ipc_rev to orders 1 to 5, ipc_fwd -------------------------------------------------------------------------------------------
def _image_operands(which, idt):
    if which == "active_12x20":      # the active block of the frame smaller than a tile
        c = slc.ipc_geometry_case(12, 20, 4, F32, F32)
        return c["cube"][0, 4:-4, 4:-4].astype(idt), c["K"], c["gain"][4:-4, 4:-4]
    c = slc.ipc_image_case(33, 257, idt, F32, F64 if idt == F64 else None)   # one row block plus one column of the image kernels
    return c["image"], c["K"], c["gain"]


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("idt", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("which", ["active_12x20", "33x257"])
def test_ipc_rev_orders(which, idt, order):
    """the image path ends in the output buffer whatever the parity of `order` (order 2 is what the goldens run)"""
    img, K, gain = _image_operands(which, idt)
    ctx = gpu_context()
    want = oipc.ipc_rev(img, K, order=order)
    # the order before differs in nearly every pixel: a result left in the wrong parity's buffer would not pass
    before = oipc.ipc_rev(img, K, order=order - 1) if order > 1 else img.astype(want.dtype)
    assert np.count_nonzero(want != before) > 0.9 * want.size
    assert_same_bits(ipc_linearity.ipc_rev(img, K, order=order, ctx=ctx), want, f"order {order}", zero_sign_ok=True)
    if gain is not None:
        assert_same_bits(ipc_linearity.ipc_rev(img, K, order=order, gain=gain, ctx=ctx), oipc.ipc_rev(img, K, order=order, gain=gain),
                         f"order {order} with gain", zero_sign_ok=True)


@pytest.mark.parametrize("order", [1, 3, 4])
def test_ipc_rev_orders_f64_kernel_on_f32_image(order):
    """the result is f64 while x = gain * image stays f32 (ipc_image_typed with T = double, XT = float): the first iterate
    reads out_0 = x and x from the f32 buffer, every later one out_n in f64 and x in f32, into either buffer of the ping-pong;
    the gain product is rounded to f32 before anything else"""
    c = slc.ipc_image_case(33, 257, F32, F64, F32)
    img, K, gain = c["image"], c["K"], c["gain"]
    ctx = gpu_context()
    for g in (None, gain):
        want = oipc.ipc_rev(img, K, order=order, gain=g)
        assert want.dtype == F64 and (img if g is None else g * img).dtype == F32
        assert_same_bits(ipc_linearity.ipc_rev(img, K, order=order, gain=g, ctx=ctx), want,
                         f"order {order}, gain {'none' if g is None else 'f32'}", zero_sign_ok=True)


@pytest.mark.parametrize("idt", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("which", ["active_12x20", "33x257"])
def test_ipc_fwd_and_order_0(which, idt):
    img, K, gain = _image_operands(which, idt)
    ctx = gpu_context()
    assert_same_bits(ipc_linearity.ipc_fwd(img, K, ctx=ctx), oipc.ipc_fwd(img, K), "fwd", zero_sign_ok=True)
    if gain is not None:
        assert_same_bits(ipc_linearity.ipc_fwd(img, K, gain=gain, ctx=ctx), oipc.ipc_fwd(img, K, gain=gain), "fwd with gain",
                         zero_sign_ok=True)
    with pytest.raises(ValueError, match="ipc_rev: order must be >= 1"):
        ipc_linearity.ipc_rev(img, K, order=0, ctx=ctx)
    assert_same_bits(ipc_linearity.ipc_rev(img, K, order=1, ctx=ctx), oipc.ipc_rev(img, K, order=1), "order 1 after the refusal",
                     zero_sign_ok=True)
