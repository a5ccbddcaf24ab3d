"""The cases of satflag_cases.py and the numpy restatement of saturation flagging, without a GPU.

Parity of oracle/saturation.py with stcal is unpinned, so the restatement is the specification test_gpu_satflag.py holds the HIP
kernels to.  Here it is guarded twice on every case: by a scalar loop per pixel and group written from its docstring, and by the
flags the plants themselves declare (satflag_cases.expected_sat).  Then the cases are shown to hold what makes the comparison on
the device mean something: the footprints of lone plants, every class of the table and its decisiveness, no flag on a pixel
that is not checked, and never more than half of a frame flagged."""

import math

import numpy as np
import pytest
from conftest import assert_same_bits

import satflag_cases as sc

SAT = sc.SAT


# ---- the second statement: one pixel, one group at a time --------------------------------------------------------------------
def scalar_exceeds(c):
    """(G, ny, nx) bool: the pixel is checked and its own sample of group g >= skip reaches its own threshold (under the
    read-pattern rule: f64(threshold) * mean(reads) / last read).  f32 and u16 values are exact as Python floats."""
    G, ny, nx = c.data.shape
    dil = [float(np.mean(r)) / float(r[-1]) if r[-1] != 0 else float("nan") for r in c.rp] if c.rule else None
    exceeds = np.zeros((G, ny, nx), bool)
    data, thr, sdq = c.data.tolist(), c.thr.tolist(), c.sdq.tolist()
    for y in range(ny):
        for x in range(nx):
            t = thr[y][x]
            if not math.isfinite(t) or (sdq[y][x] & sc.NO_SAT_CHECK):
                continue
            for g in range(c.skip, G):
                exceeds[g, y, x] = data[g][y][x] >= (t if dil is None else t * dil[g])
    return exceeds


def scalar_flags(c, backup, exceeds):
    """A group g >= skip is saturated if any pixel of its clipped 3 x 3 neighbourhood is checked and exceeds its threshold in
    some group g' with skip <= g' <= g + backup; pixeldq gets the bit if any group has it.  The given flags are kept."""
    G, ny, nx = c.data.shape
    gdq = np.zeros((G, ny, nx), np.uint8) if c.groupdq is None else c.groupdq.copy()
    pdq = c.pixeldq.copy()
    near = np.zeros((ny, nx), bool)    # (only the neighbourhoods that hold an exceeding pixel are visited)
    for y, x in np.argwhere(exceeds.any(axis=0)):
        near[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
    for y, x in np.argwhere(near):
        for g in range(c.skip, G):
            hit = False
            for yy in range(max(y - 1, 0), min(y + 2, ny)):
                for xx in range(max(x - 1, 0), min(x + 2, nx)):
                    for g2 in range(c.skip, min(g + backup, G - 1) + 1):
                        hit = hit or bool(exceeds[g2, yy, xx])
            if hit:
                gdq[g, y, x] |= SAT
                pdq[y, x] |= SAT
    return gdq, pdq


def test_the_scalar_statement_uses_the_restatement_s_factors():
    from oracle import saturation
    rp = sc.plan_pattern(16)
    want = saturation.read_pattern_dilution(rp)
    got = np.array([float(np.mean(r)) / float(r[-1]) if r[-1] != 0 else float("nan") for r in rp])
    assert_same_bits(got, want, "dilution")
    assert np.isnan(want[0]) and want[1] == 1.0 and np.all(want[2:7] < 1.0)


@pytest.mark.parametrize("name", sc.case_names())
def test_three_statements_of_the_rule_agree(name):
    """the restatement, the scalar loop and the plants' own declaration: bit for bit, every backup of the case"""
    c = sc.case(name)
    given = np.zeros(c.data.shape, np.uint8) if c.groupdq is None else c.groupdq
    exceeds = scalar_exceeds(c)
    for backup in c.backups:
        gdq, pdq = sc.flag_host(c, backup)
        want = sc.expected_sat(c, backup)
        assert_same_bits((gdq & SAT) != 0, want | ((given & SAT) != 0), f"{name}, backup {backup}: restatement vs plants")
        assert_same_bits((pdq & SAT) != 0, want.any(axis=0), f"{name}, backup {backup}: pixeldq vs plants")
        assert_same_bits(gdq & ~np.uint8(SAT), given & ~np.uint8(SAT), f"{name}: given group bits")
        assert_same_bits(pdq & ~np.uint32(SAT), c.pixeldq, f"{name}: given pixel bits")
        sg, sp = scalar_flags(c, backup, exceeds)
        assert_same_bits(gdq, sg, f"{name}, backup {backup}: restatement vs scalar loop, groupdq")
        assert_same_bits(pdq, sp, f"{name}, backup {backup}: restatement vs scalar loop, pixeldq")
        # a case that flags everything cannot show a missed flag
        assert np.count_nonzero(pdq & SAT) <= c.ny * c.nx // 2, f"{name}: more than half of the pixels are flagged"
    # backups beyond the group count say the same
    G = c.G
    ref = sc.flag_host(c, max(G - 1, 0))
    for backup in (G, G + 6, 70):
        got = sc.flag_host(c, backup)
        assert_same_bits(got[0], ref[0], f"{name}: backup {backup} vs {G - 1}")
        assert_same_bits(got[1], ref[1], f"{name}: backup {backup} vs {G - 1}, pixeldq")


@pytest.mark.parametrize("name", sc.case_names())
def test_lone_plants_have_footprints_of_9_6_and_4_pixels(name):
    """from the restatement's output alone: taking a lone flagged plant out changes exactly its clipped 3 x 3 footprint"""
    c = sc.case(name)
    size = {"interior": 9, "edge": 6, "corner": 4}
    gdq, _ = sc.flag_host(c, 0)
    for p in c.plants:
        if p["where"] is None or p["first"] is None:
            continue
        without, _ = sc.flag_host(c.edited(c.removal(p)), 0)
        changed = (gdq != without).any(axis=0)
        assert np.count_nonzero(changed) == size[p["where"]], f"{name}: plant at ({p['y']}, {p['x']})"
        assert_same_bits(changed, sc.footprint(c.ny, c.nx, p["y"], p["x"]), f"{name}: footprint of ({p['y']}, {p['x']})")
        # the flag starts at the plant's group, not before
        rose = ((gdq & SAT) != 0)[:, p["y"], p["x"]]
        if c.groupdq is not None:
            rose = rose & ((c.groupdq & SAT) == 0)[:, p["y"], p["x"]]
        assert list(np.flatnonzero(rose)) == list(range(p["first"], c.G))


@pytest.mark.parametrize("name", sc.case_names())
def test_every_plant_is_decisive(name):
    """taking a flagged plant out, or moving an unflagged one by one unit, changes the restatement's flags on its pixel; an
    unflagged plant's own pixel carries no flag of the case's making unless a neighbour's footprint covers it"""
    c = sc.case(name)
    backup = c.backups[1] if len(c.backups) > 1 else c.backups[0]
    gdq, pdq = sc.flag_host(c, backup)
    given = np.zeros(c.data.shape, np.uint8) if c.groupdq is None else c.groupdq
    first = sc.expected_first(c)
    for p in c.plants:
        y, x = p["y"], p["x"]
        if p["first"] is not None:
            other, _ = sc.flag_host(c.edited(c.removal(p)), backup)
            # (somewhere on its footprint: on its own pixel an earlier neighbour may decide)
            assert np.any(gdq != other), f"{name}: removing the plant at ({y}, {x}) changes nothing"
            continue
        if first[y, x] == c.G:
            assert not np.any((gdq[:, y, x] & SAT) & ~given[:, y, x]), \
                f"{name}: the unflagged plant at ({y}, {x}) is flagged"
            assert not (pdq[y, x] & SAT)
        if "nothing_checked" in p["kinds"]:
            assert c.skip == c.G     # skip == G: no edit of the data can flag anything
            continue
        assert p["alt"], f"{name}: the unflagged plant at ({y}, {x}) names no edit that would flag it"
        other, _ = sc.flag_host(c.edited(p["alt"]), backup)
        assert np.any(other[:, y, x] & SAT) and np.any(gdq[:, y, x] != other[:, y, x]), \
            f"{name}: the plant at ({y}, {x}) ({p['kinds']}) is not decisive"


def test_every_class_of_the_table_is_present():
    have = set()
    for c in sc.cases():
        have |= c.kinds()
    missing = [k for k in sc.REQUIRED_KINDS if k not in have]
    assert not missing, f"classes without a plant: {missing}"
    by = {c.name: c for c in sc.cases()}
    # frames, group counts, skips and backups of the list
    shapes = {(c.ny, c.nx, c.G) for c in sc.cases()}
    assert {(16, 16, 1), (16, 16, 2), (16, 16, 3), (16, 20, 8), (24, 1032, 8)} <= shapes
    assert {(16, 16, G) for G in (31, 32, 33, 63, 64)} <= shapes
    for G in (1, 2, 3):
        assert {c.skip for c in sc.cases() if c.G == G and c.name.startswith("pos_")} == {s for s in (0, 1, 2, G - 1, G) if s <= G}
    assert {c.skip for c in sc.cases() if (c.ny, c.nx, c.G) == (16, 20, 8) and c.name.startswith("pos_")} == {0, 1, 2, 7, 8}
    for c in sc.cases():
        if c.name.startswith("pos_"):
            assert set(c.backups) == {0, 1, 2, max(c.G - 1, 0), c.G, c.G + 6}
    assert by["pos_16x16_g64_skip64"].skip == 64 and by["pos_16x16_g64_skip1"].kinds() >= {f"first_at_{g}" for g in (1, 30, 31, 32, 62, 63)}
    assert by["pos_16x16_g33_skip1"].kinds() >= {f"first_at_{g}" for g in (1, 30, 31, 32)}
    # dtypes, the rule, given flags
    assert {(c.dtype.name, c.rule) for c in sc.cases()} == {("uint16", False), ("uint16", True), ("float32", False), ("float32", True)}
    for ef in (0, 1):
        q = by[f"given_groupdq_start{ef}"]
        assert by[f"given_none_start{ef}"].groupdq is None and q.exclude_first == bool(ef)
        for bit in sc.GIVEN_GROUP_BITS:
            assert np.count_nonzero(q.groupdq & bit) > 20
        assert np.any(q.groupdq[:q.skip] & SAT) and not np.any(q.groupdq[q.skip:] & SAT)
        assert np.count_nonzero(q.pixeldq >> 31) > 100 and all(np.any(q.pixeldq & b) for b in sc.MASK_BITS)
    # only the cases of one group stay off the device
    assert [c.name for c in sc.cases() if not c.runs_on_device] == ["pos_16x16_g1_skip0", "pos_16x16_g1_skip1"]
    assert all(not c.exclude_first for c in sc.cases() if c.G == 2)


def test_unchecked_pixels_carry_no_flag_whatever_their_samples():
    """a pixel that is not checked raises nothing, not even under an infinite sample; it still receives its neighbours' flags"""
    n = 0
    for c in sc.cases():
        unchecked = ~np.isfinite(c.thr) | ((c.sdq & sc.NO_SAT_CHECK) != 0)
        if not unchecked.any():
            continue
        n += int(np.count_nonzero(unchecked))
        first = sc.expected_first(c)
        for backup in c.backups:
            gdq, pdq = sc.flag_host(c, backup)
            lone = unchecked & (first == c.G)
            assert np.count_nonzero(lone) >= 3
            assert not np.any(gdq[:, lone] & SAT) and not np.any(pdq[lone] & SAT), c.name
    assert n >= 15
    c = sc.case("samples_f32")
    inf_there = np.isposinf(c.data).any(axis=0) & (~np.isfinite(c.thr) | ((c.sdq & sc.NO_SAT_CHECK) != 0))
    assert np.count_nonzero(inf_there) == 4


def test_the_f32_product_would_decide_the_planted_samples_the_other_way():
    c = sc.case("rule_u16")
    (p,) = [p for p in c.plants if "rule_f32_product_differs" in p["kinds"]]
    T, n, f = c.thr[p["y"], p["x"]], int(c.data[2, p["y"], p["x"]]), np.float64(2.5) / np.float64(3.0)
    assert (n >= np.float64(T) * f) == (p["first"] is not None) and (np.float32(n) >= T * np.float32(f)) == (p["first"] is None)
    c = sc.case("rule_f32")
    assert sum("rule_f32cube_product_differs" in p["kinds"] for p in c.plants) >= 1


# ---- flat and gain preparation: the cases of test_gpu_flat_edges.py, asked of oracle.finish.get_flat alone ----------------------
FLAT_COMBOS = [(f, g, k) for f in sc.FLAT_FRAMES for g in (np.float32, np.float64) for k in (np.float32, np.float64)]


def _get_flat(c, with_pdq=True, deconvolve=True):
    from oracle import finish
    pdq = c["pixeldq"].copy() if with_pdq else None
    with np.errstate(all="ignore"):
        return finish.get_flat(c["flat"], c["gain"], c["K"], c["nb"], pdq, ipc_deconvolve=deconvolve), pdq


@pytest.mark.parametrize("frame,gdt,kdt", FLAT_COMBOS, ids=[f"{f[0]}x{f[1]}_g{np.dtype(g).itemsize * 8}_k{np.dtype(k).itemsize * 8}" for f, g, k in FLAT_COMBOS])
def test_flat_cases_raise_every_flag_class_and_keep_the_border_out(frame, gdt, kdt):
    ny, nx, nb = frame
    c = sc.flat_case(ny, nx, nb, gdt, kdt)
    assert c["gain"].dtype == gdt and c["K"].dtype == kdt and c["K"].shape == (3, 3, ny - 2 * nb, nx - 2 * nb)
    assert c["complete"] == (frame != (9, 11, 4)) and c["isolated"] == (frame == (12, 300, 1))
    out, pdq = _get_flat(c)
    new = pdq & ~c["pixeldq"]
    assert_same_bits(new, sc.flat_plant_flags(c), "flags vs the plants' own")
    assert not np.any(new[c["border"]]) and np.all(out[c["border"]] == 1.0)
    # sick values sit in the border of both arrays, and healthy ones there give the same plane: the border is never read
    assert np.any(np.isnan(c["flat"][c["border"]])) and np.any(~(c["gain"][c["border"]] > 0.1))
    healthy = dict(c, flat=np.where(c["border"], np.float32(1.0), c["flat"]), gain=np.where(c["border"], gdt(1.5), c["gain"]))
    assert_same_bits(_get_flat(healthy)[0], out, "border replaced by healthy values")
    kinds = {k for k, _, _, _ in c["plants"]}
    flagged = {k for k, y, x, _ in c["plants"] if new[y, x]}
    if c["complete"]:
        assert kinds == {k for k, _ in sc.FLAT_PLANTS} | {k for k, _ in sc.gain_plants(gdt)}
        assert flagged == {"flat_below_tenth", "flat_above_ten", "flat_zero", "flat_minus_zero", "flat_negative", "flat_denormal",
                           "flat_pinf", "flat_ninf", "gain_tenth", "gain_below_tenth", "gain_zero", "gain_negative"}
        assert {"flat_tenth", "flat_ten", "flat_nan", "gain_above_tenth", "gain_nan", "gain_pinf"} <= kinds - flagged
        if gdt == np.float64:
            assert "gain_f32_tenth" in kinds - flagged
    else:
        assert len(c["plants"]) == 3 and flagged == {"flat_below_tenth", "gain_below_tenth"} and "flat_tenth" in kinds
    # the gain is clipped only under a pixeldq: without one the planes differ where a gain was far enough below 0.1 (zero,
    # negative; one ulp below it need not show in f32)
    assert not c["complete"] or np.count_nonzero(_get_flat(c, with_pdq=False)[0].view(np.uint32) != out.view(np.uint32)) > 0
    # without the deconvolution no gain is looked at
    plain, pdq2 = _get_flat(c, deconvolve=False)
    assert not np.any(pdq2 & sc.NO_GAIN_VALUE) and np.all((plain[~c["border"]] >= np.float32(0.1)) | np.isnan(plain[~c["border"]]))


@pytest.mark.parametrize("gdt,kdt", [(np.float32, np.float32), (np.float64, np.float64)])
def test_a_planted_nan_reaches_as_far_as_the_order_of_the_deconvolution(gdt, kdt):
    """ipc_rev runs two iterations, each of which carries a NaN one pixel on (a NaN times a zero tap is a NaN): pixels one and
    two away from the planted NaN flat are NaN, pixels three away are not (on the frame whose plants are six apart)"""
    ny, nx, nb = 12, 300, 1
    c = sc.flat_case(ny, nx, nb, gdt, kdt)
    assert c["isolated"]
    ((y, x),) = [(y, x) for k, y, x, _ in c["plants"] if k == "flat_nan"]
    out, _ = _get_flat(c)
    act = np.zeros((ny, nx), bool)
    act[nb:ny - nb, nb:nx - nb] = True
    yy, xx = np.mgrid[0:ny, 0:nx]
    dist = np.maximum(np.abs(yy - y), np.abs(xx - x))
    for d, want in ((0, True), (1, True), (2, True), (3, False)):
        ring = act & (dist == d)
        assert np.count_nonzero(ring) >= 1 and np.all(np.isnan(out[ring]) == want), f"distance {d}"
    plain, _ = _get_flat(c, deconvolve=False)
    assert np.isnan(plain[y, x]) and np.count_nonzero(np.isnan(plain)) == 1
