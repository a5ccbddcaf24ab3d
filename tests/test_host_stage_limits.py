"""The cases of stage_limit_cases.py and the oracle at their shapes, without a GPU.

The goldens pin oracle/ bit for bit only at the fixtures' shapes (40 x 72 or 40 x 256 frames, 3 to 16 groups, 4 / 9 / 11 planes,
a border of 4, IPC order 2).  test_gpu_stage_limits.py compares the HIP stage kernels with oracle/ far outside them, so here
(1) the cases are shown to hold what makes those comparisons mean something and (2) the oracle is checked at the new shapes
against independent restatements: a per-pixel scalar loop for the IPC operators, the recurrence of ipc_rev step by step, and
numpy's own Legendre evaluation in f64 for the series and its linear continuation."""

import numpy as np
import pytest
from conftest import assert_same_bits
from numpy.polynomial import legendre as npleg

import stage_limit_cases as slc
from oracle import ipc as oipc
from oracle import linearity as olin
from oracle import rampfit as orf

F32, F64 = np.float32, np.float64


# ---- 1. preconditions of the cases -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,exclude_first", [(G, True) for G in slc.LONG_COUNTS] + [(17, False)])
def test_long_ramps_cover_every_first_saturation_and_raise_jumps(G, exclude_first):
    """Every group 0..G-1 is the first saturated one of an active pixel, one active pixel never saturates, and ONE pass of the
    oracle over the full ramp (fit_and_flag: what ramp_fit keeps for the pixels whose last group is not saturated) raises new
    JUMP_DET flags there, the planted step of the never-saturated staircase pixel among them.  (The whole ramp_fit of the
    oracle takes 10 to 25 s at 64 groups; the truncated variants are asked of it at 17 and 33 groups below, and at every count by the
    GPU tests, which compute it anyway.)"""
    c = slc.long_ramp_case(G, exclude_first=exclude_first)
    ny, nx = c["data"].shape[1:]
    assert (ny, nx) == slc.long_frame(G) and nx >= G + 13
    act = (slice(slc.NB, -slc.NB), slice(slc.NB, -slc.NB))
    fs = slc.first_saturation(c["groupdq"])[act]
    assert [g for g in range(G + 1) if not np.any(fs == g)] == []
    flags = np.zeros_like(c["groupdq"])
    with np.errstate(all="ignore"):
        orf.fit_and_flag(c["data"], flags, c["gain"], c["read"], c["meta"], slc.NB, exclude_first)
    kept = ((flags & slc.JUMP) != 0) & ((c["groupdq"][-1] & slc.SAT) == 0)[None] & ((c["groupdq"] & slc.JUMP) == 0)
    assert np.count_nonzero(kept) > 0
    assert kept[G // 2 - 1, slc.PLANT_ROW, slc.STAIR_COL0 + G]


@pytest.mark.parametrize("G,exclude_first", [(17, True), (17, False), (33, True)])
def test_long_ramps_raise_jumps_inside_truncated_variants(G, exclude_first):
    """the oracle's ramp_fit flags the planted steps inside the longest, a middle and the shortest truncated variant"""
    res = slc.oracle_ramp_fit(G, False, exclude_first)
    slc.assert_long_ramp_conditions(res, need_truncated=True)
    start = 1 if exclude_first else 0
    fs = slc.first_saturation(res["case"]["groupdq"])
    truncated = (fs >= 3 + start) & (fs < G)
    assert np.count_nonzero(slc.new_jumps(res) & truncated[None]) >= 3


@pytest.mark.parametrize("nplanes", slc.LIN_PLANES)
def test_planted_linearity_samples_land_where_intended(nplanes):
    """z as the oracle forms it (f32): the bound itself gives -+1 exactly; the next f32 beyond it lies outside [Smin, Smax] and
    its z is within an ulp of the quotient (2 eps) of -+1 (the rounding of z decides the flag); `last` is in range and its successor `cross` is not"""
    c = slc.legendre_case(nplanes)
    seen = set()
    for g, y, x, kind in c["plants"]:
        S, lo, hi = c["S"][g, y, x], c["Smin"][y, x], c["Smax"][y, x]
        z = slc.z_of(S, lo, hi)
        assert z.dtype == F32 and c["lin_dq"][y, x] == 0 and c["attempt_corr"][g, y, x] != 0
        what, side = kind.split("_")
        end = F32(1.0 if side == "max" else -1.0)
        if what == "at":
            assert S == (hi if side == "max" else lo) and z == end
        elif what == "ulp":
            assert (S > hi if side == "max" else S < lo)
            assert abs(abs(z) - F32(1)) <= 2 * np.finfo(F32).eps   # one ulp of the quotient 2 t / span, which is near 2
        elif what == "last":
            assert z == end and (S >= hi if side == "max" else S <= lo)
        else:
            assert abs(z) > 1 and np.sign(z) == end and (S > hi if side == "max" else S < lo)
            assert abs(slc.z_of(np.nextafter(S, F32(lo)), lo, hi)) <= 1   # its predecessor is still in range
        seen.add((g, kind))
    assert seen == {(g, k) for g in slc.PLANT_GROUPS for k in slc.PLANT_KINDS}
    # the flag decisions these samples make, in the oracle: with do_not_flag_first group 0 is clipped and never flags
    for dnff in (True, False):
        _, dq = olin.multilin(c["S"], c["coefs"], c["Smin"], c["Smax"], c["Sref"], c["lin_dq"], do_not_flag_first=dnff,
                              attempt_corr=c["attempt_corr"])
        for g, y, x, kind in c["plants"]:
            others = [gg for gg in range(slc.LIN_GROUPS) if gg != g and not (gg == 0 and dnff)]
            quiet = all(abs(slc.z_of(c["S"][gg, y, x], c["Smin"][y, x], c["Smax"][y, x])) <= 1 or c["attempt_corr"][gg, y, x] == 0
                        for gg in others)
            if not quiet:
                continue
            out = abs(slc.z_of(c["S"][g, y, x], c["Smin"][y, x], c["Smax"][y, x])) > 1 and not (g == 0 and dnff)
            assert bool(dq[y, x] & olin.NO_LIN_CORR) == bool(out), (g, y, x, kind, dnff)


@pytest.mark.parametrize("ny,nx,nb", slc.IPC_FRAMES)
def test_ipc_geometries_give_their_border_back(ny, nx, nb):
    c = slc.ipc_geometry_case(ny, nx, nb)
    assert oipc.border_of(nx, c["K"]) == nb and c["K"].shape == (3, 3, ny - 2 * nb, nx - 2 * nb)
    assert np.count_nonzero(c["K"] == 0) > 0 and abs(float(np.mean(c["K"][1, 1])) - 0.94) < 0.005


# ---- 2. the oracle against independent restatements -----------------------------------------------------------------------------
def fwd_loop(im, K):
    """ipc_fwd pixel by pixel: the nine products in the documented order (centre, (1,0), (-1,0), (0,1), (0,-1), (1,1), (1,-1),
    (-1,1), (-1,-1)), each rounded, then added, in numpy scalars of the arrays' dtypes; a source outside the image adds no term"""
    ny, nx = im.shape
    out = np.empty((ny, nx), np.result_type(im.dtype, K.dtype))
    for y in range(ny):
        for x in range(nx):
            acc = im[y, x] * K[1, 1, y, x]
            for dy, dx in ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1)):
                sy, sx = y - dy, x - dx
                if 0 <= sy < ny and 0 <= sx < nx:
                    acc = acc + im[sy, sx] * K[1 + dy, 1 + dx, sy, sx]
            out[y, x] = acc
    return out


def correct_cube_loop(data, K, gain, nb):
    """correct_cube restated from the reference's lines: data[i, act] = ipc_rev(data[i, act] * g, K) / g with ipc_rev's two
    steps out = out + x - ipc_fwd(out)"""
    out = data.copy()
    ny, nx = data.shape[1:]
    act = (slice(nb, ny - nb), slice(nb, nx - nb))
    g = 1.0 if gain is None else gain[act]
    for i in range(data.shape[0]):
        x = data[i][act] * g
        o = x
        for _ in range(2):
            o = o + x - fwd_loop(o, K)
        out[i][act] = o / g
    return out


LOOP_FRAMES = [f for f in slc.IPC_FRAMES if f[2] == 0 or f == (12, 20, 4)]
LOOP_CASES = [(f, F32, None) for f in LOOP_FRAMES] + [((32, 128, 0), F32, F32), ((32, 128, 0), F64, F64), ((12, 20, 4), F64, F32),
                                                      ((12, 20, 4), F32, F64), ((17, 65, 0), F64, None)]


@pytest.mark.parametrize("frame,kdt,gdt", LOOP_CASES)
def test_oracle_ipc_equals_a_per_pixel_loop(frame, kdt, gdt):
    ny, nx, nb = frame
    c = slc.ipc_geometry_case(ny, nx, nb, kdt, gdt)
    act = (slice(nb, ny - nb), slice(nb, nx - nb))
    img = c["cube"][0][act]
    assert_same_bits(oipc.ipc_fwd(img, c["K"]), fwd_loop(img, c["K"]), "ipc_fwd")
    if c["gain"] is not None:
        g = c["gain"][act]
        assert_same_bits(oipc.ipc_fwd(img, c["K"], gain=g), fwd_loop(g * img, c["K"]) / g, "ipc_fwd with gain")
    got = oipc.correct_cube(c["cube"].copy(), c["K"], c["gain"])
    want = correct_cube_loop(c["cube"], c["K"], c["gain"], nb)
    assert_same_bits(got, want, "correct_cube")
    border = np.ones((ny, nx), bool)
    border[act] = False
    assert_same_bits(got[:, border], c["cube"][:, border], "border")
    assert np.count_nonzero(got != c["cube"]) > 0.9 * c["cube"][:, ~border].size


@pytest.mark.parametrize("idt,kdt,gdt", [(F32, F32, None), (F64, F32, None), (F32, F64, F32), (F32, F32, F64)])
def test_oracle_ipc_rev_obeys_its_recurrence_to_order_5(idt, kdt, gdt):
    """out_0 = x, out_{n+1} = (out_n + x) - fwd(out_n): every order from the one before, bit for bit"""
    c = slc.ipc_geometry_case(12, 20, 4, kdt, gdt)
    img = c["cube"][0, 4:-4, 4:-4].astype(idt)
    g = None if c["gain"] is None else c["gain"][4:-4, 4:-4]
    x = img if g is None else g * img
    prev = x
    for order in range(1, 6):
        nxt = (prev + x) - oipc.ipc_fwd(prev, c["K"])
        got = oipc.ipc_rev(img, c["K"], order=order, gain=g)
        assert_same_bits(got, nxt if g is None else nxt / g, f"order {order}")
        assert not np.array_equal(nxt, prev)
        prev = nxt


# largest |oracle - f64| / (eps32 * sum_L (1 + L^2) |c_L|) measured over these cases, per plane count: inside the range against
# numpy.polynomial.legendre.legval, outside it against the linear continuation from -+1 formed in f64
LEGENDRE_RATIO_INSIDE = {1: 0.0, 2: 0.2740, 3: 0.4407, 32: 2.0644}
LEGENDRE_RATIO_OUTSIDE = {1: 0.0, 2: 0.2753, 3: 0.4443, 32: 1.9149}


def _legendre_operands(nplanes):
    c = slc.legendre_case(nplanes)
    co = c["coefs"].reshape(nplanes, -1)
    L = np.arange(nplanes)[:, None]
    norm = np.finfo(F32).eps * np.sum((1 + L**2) * np.abs(co.astype(F64)), axis=0)
    return co, norm, np.random.default_rng(5)


@pytest.mark.parametrize("nplanes", [1, 2, 3, 32])
def test_oracle_legendre_series_inside_the_range(nplanes):
    """oracle.linearity.legendre_series (f32 recurrence) against numpy.polynomial.legendre.legval in f64 at |z| <= 1, the ends
    and 0 included.  This catches a wrong recurrence constant, not rounding: a constant off by 1e-3 moves P_L by 1e-3, and the
    series by 1e-3 |c_L|, thousands of times the bound.  Measured: the largest |oracle - f64| / (eps32 * sum_L (1 + L^2) |c_L|)
    is 0 for 1 plane (the series is c_0), 0.2740 for 2, 0.4407 for 3 and 2.0644 for 32 planes (the test prints what it finds);
    asserted at four times that."""
    co, norm, rng = _legendre_operands(nplanes)
    worst = 0.0
    for _ in range(8):
        z = rng.uniform(-1, 1, size=co.shape[1]).astype(F32)
        z[:3] = (-1, 0, 1)
        phi, ex = olin.legendre_series(z, co)
        assert phi.dtype == F32 and not ex.any()
        ref = npleg.legval(z.astype(F64), co.astype(F64), tensor=False)
        worst = max(worst, float(np.max(np.abs(phi - ref) / norm)))
    print(f"{nplanes} planes, inside: ratio {worst:.4f}")
    assert worst <= 4 * LEGENDRE_RATIO_INSIDE[nplanes]


@pytest.mark.parametrize("nplanes", [1, 2, 3, 32])
def test_oracle_legendre_series_outside_the_range(nplanes):
    """1 < |z| <= 1.02 (400 DN beyond a range of 50000 is 1.016): the series equals sum_L c_L (+-1)^L (1 + L (L + 1) / 2 (|z| - 1))
    formed in f64, under the same rule.  Measured ratios: 0, 0.2753, 0.4443 and 1.9149 for 1, 2, 3 and 32 planes;
    asserted at four times that."""
    co, norm, rng = _legendre_operands(nplanes)
    L = np.arange(nplanes)[:, None]
    worst = 0.0
    for _ in range(8):
        z = (1 + rng.uniform(0, 0.02, size=co.shape[1])).astype(F32) * np.where(rng.uniform(size=co.shape[1]) < 0.5, -1, 1).astype(F32)
        keep = np.abs(z) > 1
        z, c, nrm = z[keep], co[:, keep], norm[keep]
        phi, ex = olin.legendre_series(z, c)
        assert phi.dtype == F32 and ex.all()
        z64 = z.astype(F64)
        ref = np.sum(c.astype(F64) * np.sign(z64)[None] ** L * (1 + (L * (L + 1) / 2) * (np.abs(z64) - 1)[None]), axis=0)
        worst = max(worst, float(np.max(np.abs(phi - ref) / nrm)))
    print(f"{nplanes} planes, outside: ratio {worst:.4f}")
    assert worst <= 4 * LEGENDRE_RATIO_OUTSIDE[nplanes]
