"""The cases of synth_edge_cases.py hold what they claim, without a GPU: asked of the ORACLE's values alone.

test_gpu_synth_edges.py compares the synthesis kernels with oracle/l1sim.py and oracle/linearity.py bit for bit on these cases;
a comparison at a rounding tie, at the u16 clip or on a planted read sequence only means something if the case really holds
the tie, the clip or the sequence.  Conditions, not measurements: a planted pixel that misses fails the test."""

import numpy as np
import pytest
from conftest import assert_same_bits, l1sim_golden_cal, load_golden

import synth_edge_cases as sec
from oracle import l1sim, linearity

F4, F8 = sec.F4, sec.F8


# ---- the oracle generalisations ------------------------------------------------------------------------------------------------
def test_oracle_keywords_leave_the_pinned_fixture_as_it_was():
    """the executed-reference fixture through the generalised oracle: 32 channels, a border of 4 -- and the unrounded resultants
    round to the pinned ones"""
    g = load_golden("l1sim")
    cal, rp = l1sim_golden_cal(g)
    res, start, pre = l1sim.make_l1_fullcal(g["counts"], rp, cal, float(g["read_time"]), g["normals_reset"], g["reads_e"],
                                            g["normals_read"], unrounded=True)
    assert_same_bits(res, g["resultants"], "resultants")
    assert_same_bits(np.round(pre), g["resultants"], "rounded unrounded resultants")
    assert not np.array_equal(pre, res)
    im, a33 = g["im_before"].copy(), np.zeros_like(g["amp33_after"])
    l1sim.fill_in_refdata_and_1f(im, cal, l1sim.read_pattern_to_tij(rp, float(g["read_time"])), g["normals_fill"],
                                 frames=g["frames"], white33=g["white33"], amp33=a33, channelwidth=16)
    assert g["frames"].shape[1] == 34 and np.array_equal(im, g["im_after"]) and np.array_equal(a33, g["amp33_after"])


def test_oracle_accepts_a_zero_border():
    ny, nx, nb = 32, 520, 0
    c = sec.resultants_case(next(i for i, r in enumerate(sec.RES_TABLE) if sec.GEOMETRIES[r[3]] == (ny, nx, nb)))
    assert c["want"].shape[1:] == (ny, nx) == c["start"].shape and c["cube"].shape[1:] == (ny, nx)
    assert np.array_equal(c["cube"], np.clip(c["want"], 0, 65535).astype(np.uint16)) and np.count_nonzero(c["cube"]) > 0.99 * c["cube"].size


@pytest.mark.parametrize("ny,nx,nb", sec.GEOMETRIES + (sec.WARM_FRAME, sec.TIE_FRAME))
def test_frame_heights_give_the_border(ny, nx, nb):
    assert sec.border_rule(ny - 2 * nb) == nb


# ---- 2. the dtype / plane-count table ------------------------------------------------------------------------------------------
def test_table_covers_every_plane_count_and_dtype_pair():
    rows = sec.RES_TABLE
    assert sorted({r[0] for r in rows}) == list(range(2, 18))
    with_ipc = [r for r in rows if r[2] is not None]
    for pair in ((F4, F4), (F4, F8), (F8, F4), (F8, F8)):
        assert sum((r[1], r[2]) == pair for r in with_ipc) >= 3, pair
    ff = sorted(r[0] for r in with_ipc if (r[1], r[2]) == (F8, F8))
    assert ff[0] == 2 and ff[-1] == 17 and any(2 < n < 17 for n in ff)
    assert len({r[0] for r in rows if r[2] is None}) == 2
    assert {r[3] for r in rows} == set(range(len(sec.GEOMETRIES))) and {r[4] for r in rows} == set(sec.PATTERNS)
    assert {r[5] for r in rows} == {True, False}
    assert len({sec.res_id(i) for i in range(len(rows))}) == len(rows)


@pytest.mark.parametrize("i", range(len(sec.RES_TABLE)), ids=sec.res_id)
def test_resultants_cases_are_what_the_table_says(i):
    n, gdt, kdt, geom, pat, bias = sec.RES_TABLE[i]
    c = sec.resultants_case(i)
    cal = c["cal"]
    ny, nx, nb = sec.GEOMETRIES[geom]
    assert cal["linearitylegendre"]["data"].shape == (n, ny, nx) and cal["gain"]["data"].dtype == gdt
    assert ("ipc4d" in cal) == (kdt is not None) and ("biascorr" in cal) == bias
    if kdt is not None:
        assert cal["ipc4d"]["data"].dtype == kdt and cal["ipc4d"]["data"].shape == (3, 3, ny - 2 * nb, nx - 2 * nb)
    if bias:
        assert np.count_nonzero(cal["biascorr"]["data"]) > 0
    assert c["reads_e"].shape == (sum(len(g) for g in c["rp"]), ny - 2 * nb, nx - 2 * nb) and c["reads_e"].dtype == np.int32
    # nothing undefined reaches the u16 cast, and the comparison is not one of constants
    assert np.all(np.isfinite(c["pre"])) and np.all(np.isfinite(c["start"]))
    assert len(np.unique(c["want"])) > 100 and np.all(c["want"] == np.round(c["want"]))
    if nb:
        assert not c["cube"][:, :nb].any() and not c["cube"][:, -nb:].any() and not c["cube"][:, :, :nb].any() \
            and not c["cube"][:, :, -nb:].any()


# ---- 3. planted read sequences -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", range(len(sec.WARM_VARIANTS)))
def test_planted_sequences_are_present_and_behave(v):
    c = sec.warm_case(v)
    plants = sec.warm_plants()
    kinds = {k for k, _, _ in plants}
    assert kinds == set(sec.WARM_KINDS) and {f"jump_{r}" for r in range(1, 11)} <= kinds
    assert c["reads_e"].shape[0] == 11 and c["reads_e"].dtype == np.int32
    lanes = {(x // 64) for _, y, x in plants if y == sec.WARM_ROW}
    assert lanes == {0, 1, 2, 3, 4}    # every wave of the row, the workgroup of 8 lanes included
    dn = per = sec.per_read_dn(c)
    assert np.all(np.isfinite(dn)) and np.all(np.isfinite(c["want"]))
    lin = c["cal"]["linearitylegendre"]
    nb = c["nb"]
    smin, smax = (lin[k][nb:-nb, nb:-nb].astype(F8) for k in ("Smin", "Smax"))
    lowest, highest = smin + (smax - smin) / 2 * 2.0**-24, smin + (smax - smin) / 2 * (2 - 2.0**-24)
    for kind, y, x in plants:
        e, s = c["reads_e"][:, y, x], per[:, y, x]
        assert np.array_equal(e, sec.planted_sequence(kind)), kind
        if kind == "constant":
            assert np.all(s == s[0]) and smin[y, x] + 100 < s[0] < smax[y, x] - 100     # the same DN in all reads: the path is reused
        elif kind == "plus_one":
            assert np.all(np.diff(s) >= 0) and s[-1] > s[0]
        elif kind.startswith("jump_"):
            r = int(kind[5:])
            assert s[r] - s[r - 1] > 10000 and np.all(np.abs(np.diff(s[:r])) < 2000)      # the reads differ across the jump
        elif kind == "fall_back":
            assert s[5] - s[4] > 10000 and s[5] - s[6] > 10000                         # non-monotone
        elif kind == "full":
            assert np.all(np.abs(s - highest[y, x]) < 0.01)                            # every step up: z = 1 - 2^-24
        elif kind == "negative":
            assert np.all(np.abs(s - lowest[y, x]) < 0.01)                             # every step down
        elif kind == "alternate":
            assert np.all(np.abs(s[1::2] - highest[y, x]) < 0.01) and np.all(s[0::2] < highest[y, x] - 10000)
        elif kind == "zeros":
            assert np.all(s == s[0]) or "ipc4d" in c["cal"]
    # the pixels around are ordinary ramps: every planted lane shares its wave with lanes that must evaluate
    ordinary = np.ones(c["reads_e"].shape[1:], bool)
    for kind, y, x in plants:
        ordinary[y - 1:y + 2, x - 1:x + 2] = False
    d = np.diff(c["reads_e"].astype(np.int64), axis=0)[:, ordinary]
    assert np.all(d >= 0) and np.all(c["reads_e"][-1][ordinary] >= 50) and ordinary[sec.WARM_ROW].sum() > 200


# ---- 4. ties and the clip of the resultants ------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", range(len(sec.TIE_VARIANTS)))
def test_every_planted_tie_is_a_tie_and_the_clip_is_hit_from_both_sides(v):
    c = sec.tie_clip_case(v)
    pre, want, cube, nb = c["pre"], c["want"], c["cube"], c["nb"]
    assert pre.dtype == F4 and np.all(np.isfinite(pre))
    tie, k = pre[:, sec.TIE_ROW, sec.TIE_COLS].astype(F8), c["tie_k"]
    assert tie.shape == (5, 60) and np.array_equal(tie, k + 0.5), f"{np.count_nonzero(tie != k + 0.5)} of {tie.size} planted ties miss"
    assert np.array_equal(k % 2, np.tile(np.arange(60) % 2, (5, 1)))                 # both parities, alternately
    rounded = want[:, sec.TIE_ROW, sec.TIE_COLS].astype(F8)
    assert np.array_equal(rounded, k + (k % 2)) and np.all(rounded % 2 == 0)         # to even: the even k down, the odd k up
    assert np.all((k > 1000) & (k < 60000))
    clip = want[:, sec.CLIP_ROW, sec.CLIP_COLS]
    up, down = clip[:, sec.CLIP_COLS % 2 == 0], clip[:, sec.CLIP_COLS % 2 == 1]
    assert np.all(up > 70000) and np.all(down < -30000)                              # `resultants` keeps the unclipped values
    inner = cube[:, nb:-nb, nb:-nb]
    assert np.all(inner[:, sec.CLIP_ROW, sec.CLIP_COLS][:, sec.CLIP_COLS % 2 == 0] == 65535)
    assert np.all(inner[:, sec.CLIP_ROW, sec.CLIP_COLS][:, sec.CLIP_COLS % 2 == 1] == 0)
    assert np.any(cube == 65535) and np.any(inner == 0) and np.any(pre > 65535.5) and np.any(pre < -0.5)
    for y, x, counts in sec.BRIGHT:
        assert c["reads_e"][-1, y, x] == int(counts) and want[-1, y, x] > 50000     # at the top of the series


# ---- 5. the fill ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", range(len(sec.FILL_GEOMETRIES)))
@pytest.mark.parametrize("call", sec.FILL_CALLS)
def test_fill_cases_hold_the_exact_edges(g, call):
    c = sec.fill_case(g, call)
    ny, nx, cw, nb = sec.FILL_GEOMETRIES[g]
    assert nx % cw == 0 and c["cube_in"].shape == (5, ny, nx) and sec.border_rule(ny - 2 * nb) == nb
    for a in (c["normals"], c["frames"], c["white33"], c["cal"]["dark"]["data"], c["cal"]["read"]["data"],
              c["cal"]["read"]["resetnoise"], c["cal"]["read"]["amp33"]["med"], c["cal"]["read"]["amp33"]["std"]):
        assert a is None or np.all(np.isfinite(a))
    if c["banding"]:
        assert c["frames"].shape == (5, nx // cw + 2, ny, cw)
    want = c["cube_want"]
    dark = c["cal"]["dark"]["data"]
    seen = set()
    for y, x, i in sec.edge_pixels(ny, nx, cw):
        assert y < nb or y >= ny - nb or x < nb or x >= nx - nb, "not a border pixel"
        # no white noise and no 1/f noise here: the value before rounding IS the dark
        assert np.all(c["normals"][:, y, x] == 0) and np.all(dark[:, y, x] == F4(sec.EDGE_DARKS[i]))
        assert np.all(want[:, y, x] == sec.EDGE_WANT[i]), (y, x, sec.EDGE_DARKS[i], want[:, y, x])
        seen.add((x // cw) % 2)
    assert seen == {0, 1}    # even and odd (mirrored) channels
    assert min(sec.EDGE_DARKS) < 0 and max(sec.EDGE_DARKS) > 65535 and np.any(want == 0) and np.any(want == 65535)
    # the active pixels: as they came, unless banding moves them
    act = (slice(None), slice(nb, ny - nb), slice(nb, nx - nb))
    if not c["banding"]:
        assert np.array_equal(want[act], c["cube_in"][act])
    else:
        assert np.count_nonzero(want[act] != c["cube_in"][act]) > 0.5 * want[act].size
    assert np.any(c["cube_in"][act] == 0) and np.any(c["cube_in"][act] == 65535)
    a33 = c["amp33_want"]
    if not c["with_amp33"]:
        assert a33 is None
    elif not c["banding"]:
        assert np.all(a33 == sec.GARBAGE)
    else:
        for y, xc, i in sec.amp33_pixels():
            assert np.all(a33[:, y, xc] == sec.AMP33_WANT[i]), (sec.AMP33_MEDS[i], a33[:, y, xc])
        level = np.array(sec.AMP33_MEDS, F4)
        assert np.array_equal(level.astype(np.int64).astype(np.uint16), np.array(sec.AMP33_WANT, np.uint16))
        assert np.count_nonzero(a33 == sec.GARBAGE) == 0


def test_fill_channel_counts():
    assert sorted(nx // cw for _, nx, cw, _ in sec.FILL_GEOMETRIES) == [2, 2, 3, 32]
    assert {nb for *_, nb in sec.FILL_GEOMETRIES} == {2, 4}


def test_fill_mirror_case_mirrors_in_the_oracle():
    c = sec.fill_mirror_case()
    cw, want = c["cw"], c["cube_want"].astype(np.int64)
    ch0, ch1 = want[:, :, :cw], want[:, :, cw:2 * cw]
    assert np.array_equal(ch1, ch0[:, :, ::-1])
    step = np.diff(ch0, axis=2)
    u = float(c["cal"]["read"]["anc"]["U_PINK"])
    for j, grp in enumerate(c["rp"]):
        planted = sec.MIRROR_STEP * u / len(grp) ** 0.5
        assert np.all(np.abs(step[j] - planted) <= 1) and np.all(step[j] > 0)
        assert np.all(np.abs(ch1[j, :, 0] - ch0[j, :, 0] - planted * (cw - 1)) <= 1)


# ---- 6. EXTRACT_REF ------------------------------------------------------------------------------------------------------------
def test_extract_cases_hit_both_clips():
    low = high = 0
    for n in sec.EXTRACT_N:
        for ngrp in sec.EXTRACT_NGRP:
            for off in sec.EXTRACT_OFFSETS:
                c = sec.extract_case(n, ngrp, off)
                assert c["data"].shape == (ngrp, n) and c["rest"].shape == (ngrp - 1, n) and np.array_equal(c["ref"], c["data"][0])
                raw = c["data"][1:].astype(np.int64) - c["data"][0].astype(np.int64) + off
                assert np.array_equal(np.clip(raw, 0, 65535), c["rest"])
                if ngrp > 1:
                    low += int(np.any(raw < 0))
                    high += int(np.any(raw > 65535))
    assert low >= 10 and high >= 10


# ---- 7. inverse linearity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F4, F8], ids=["f32", "f64"])
@pytest.mark.parametrize("nplanes", range(2, 18))
def test_invlin_cases(nplanes, dtype):
    c = sec.invlin_case(nplanes, dtype)
    t, S, ex = c["target"], c["S"], c["ex"]
    assert c["coefs"].shape == (nplanes,) + sec.INVLIN_SHAPE and t.dtype == dtype and S.dtype == dtype
    assert not ex.any()                                            # |z| never exceeds 1 - 2^-23 at an evaluation
    assert np.all(np.isfinite(S)) and not np.isnan(t).any()
    fin = np.isfinite(t)
    assert np.count_nonzero(t[fin] < c["phi_lo"][fin]) >= 1 and np.count_nonzero(t[fin] > c["phi_hi"][fin]) > 10    # outside the series' range
    smin, smax = c["Smin"].astype(F8), c["Smax"].astype(F8)
    half = (smax - smin) / 2
    zend = (S.astype(F8) - smin) / half - 1
    row = sec.INVLIN_INF_ROW
    assert np.all(np.abs(zend[row, :18] - 1) < 1e-6) and np.all(np.abs(zend[row, 18:] + 1) < 1e-6)
    # a target EQUAL to the series value at z is not above it (the comparison is a strict <), and z is reached: from z = 0 the
    # first step goes up towards + 0.5 and down towards - 0.5
    for r, z0 in sec.INVLIN_ROWS:
        phi, _ = linearity.legendre_series(np.full(sec.INVLIN_SHAPE[1], z0, dtype), c["coefs"][:, r], linextrap=False)
        assert phi.dtype == F4 and np.array_equal(phi.astype(dtype), t[r])
        phi0, _ = linearity.legendre_series(np.zeros(sec.INVLIN_SHAPE[1], dtype), c["coefs"][:, r], linextrap=False)
        if z0 > 0:
            assert np.all(phi0 < t[r])
        elif z0 < 0:
            assert not np.any(phi0 < t[r])
        assert np.all(zend[r] < z0 + 1e-6) and np.all(zend[r] > z0 - 0.5 - 1e-6), (r, z0)
