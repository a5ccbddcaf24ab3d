"""rip_chain_geometry_for: the launch geometry of the fused kernel (chain2_form.h: chain2_geometry, c2_form_geometry), asked on the
host.  No GPU needed: the library loads without one.

For every geometry the query returns, the pixels the grid would emit are rebuilt here from the documented contract alone (the
strip geometry comment of chain2_form.h and the prologue of chain2_kernel.h), NOT from the selection code:
  - the window of strip s starts at column s * (cols - 4); a window of wl lanes emits its lanes 2 .. wl-3, plus the lanes that hold
    the frame's columns 0, 1 and nx-2, nx-1; lanes beyond the frame emit nothing;
  - uniform grid: block b < nr * nstrips is strip b % nstrips and row range b / nstrips, wl = cols;
  - quad mode: blocks b < nr * (nstrips - 1) as above on the nstrips - 1 full strips; block nr * (nstrips - 1) + q is the LAST strip,
    its wave column w (cols / 64 of them) a 64-lane window on row range q * (cols / 64) + w of rows_q rows;
  - row range i of `rows` rows is [min(ny, i * rows), min(ny, i * rows + rows)).
Every pixel of the frame must be emitted exactly once.  The count is kept factored (per strip: columns x rows), which is exact
because a block emits a rectangle; a brute-force pixel count over block ids checks the factoring on a sample."""

from functools import lru_cache

import numpy as np
import pytest

from romanimpreprocess_amd import _native

F32, F64 = _native.RIP_F32, _native.RIP_F64

# the four forms (chain2_form.h): a representative group count, the ipc4d dtype, window columns, workgroups per CU
FORMS = {
    "f32_5to8": (8, F32, 256, 2),
    "f64_5to8": (8, F64, 384, 1),
    "f32_9to16": (16, F32, 384, 1),
    "f64_9to16": (16, F64, 256, 1),
}
NCUS = (8, 32, 64, 128, 256, 304)
NXS = tuple(range(128, 6273, 128))
NYS = tuple(range(16, 301)) + (301, 333, 384, 400, 511, 512, 513, 640, 703, 704, 720, 999, 1000, 1001, 1024, 1160, 1376, 1599, 1600,
                               2047, 2048, 2049, 3000, 4088, 4095, 4096, 4097, 4224)


def reserves(ncu, per_cu):
    """none, the default, and more than the form has slots"""
    return (0, 8, ncu * per_cu + 5)


def geo(G, kdt, ny, nx, ncu, reserve, quad_ok=True, planes=9):
    return _native.chain_geometry_for(planes, G, kdt, ny, nx, ncu, reserve, quad_ok)


# ---- the contract, restated
def strip_count(cols, nx):
    return max(1, -(-(nx - 4) // (cols - 4)))


def window_emits(start, wl, nx):
    """frame columns a window of wl lanes at column `start` emits"""
    w = np.arange(wl)
    c = start + w
    return c[(c < nx) & ((w >= 2) | (c < 2)) & ((w < wl - 2) | (c >= nx - 2))]


@lru_cache(maxsize=None)
def column_counts_ok(cols, nx, quad):
    """every column of the frame is emitted by exactly one strip (the last strip a 64-lane window in quad mode)"""
    n = strip_count(cols, nx)
    cnt = np.zeros(nx, dtype=np.int64)
    for s in range(n):
        cnt[window_emits(s * (cols - 4), 64 if (quad and s == n - 1) else cols, nx)] += 1
    return bool((cnt == 1).all())


def range_counts(ny, n, rows):
    r0 = np.minimum(ny, np.arange(n) * rows)
    r1 = np.minimum(ny, r0 + rows)
    d = np.bincount(r0, minlength=ny + 1) - np.bincount(r1, minlength=ny + 1)
    return np.cumsum(d)[:ny]


@lru_cache(maxsize=None)
def row_counts_ok(ny, n, rows):
    """n row ranges of `rows` rows emit every row of the frame exactly once"""
    return rows >= 1 and bool((range_counts(ny, n, rows) == 1).all())


def blocks_ok(nfull, nr):
    """block ids 0 .. nfull * nr - 1 meet every (strip, row range) cell once"""
    b = np.arange(nfull * nr)
    return bool((np.bincount((b % nfull) * nr + b // nfull, minlength=nfull * nr) == 1).all())


def check_geometry(g, cols, ny, nx, what):
    assert g is not None, what
    wc = cols // 64
    n = strip_count(cols, nx)
    assert (g["cols"], g["nstrips"], g["live_last"]) == (cols, n, nx - (n - 1) * (cols - 4)), what
    quad = g["nq"] > 0
    assert quad == (g["rows_q"] > 0), what
    assert g["nr"] >= 1 and g["rows"] >= 1, what
    nfull = n - 1 if quad else n
    assert g["grid"] == g["nr"] * nfull + g["nq"], what
    if quad:
        assert n > 1 and g["live_last"] <= 64, what
        assert row_counts_ok(ny, wc * g["nq"], g["rows_q"]), f"{what}: rows of the quad strip"
    assert row_counts_ok(ny, g["nr"], g["rows"]), f"{what}: rows of the full-width strips"
    assert column_counts_ok(cols, nx, quad), f"{what}: columns"


def pixel_counts(g, ny, nx):
    """brute force: the emission count of every pixel, block by block"""
    cols, wc, n = g["cols"], g["cols"] // 64, g["nstrips"]
    quad = g["nq"] > 0
    nfull = n - 1 if quad else n
    cnt = np.zeros((ny, nx), dtype=np.int64)
    for b in range(g["grid"]):
        if b < nfull * g["nr"]:
            cells = [(b % nfull, cols, (b // nfull) * g["rows"], g["rows"])]
        else:
            cells = [(nfull, 64, ((b - nfull * g["nr"]) * wc + w) * g["rows_q"], g["rows_q"]) for w in range(wc)]
        for strip, wl, r0, rows in cells:
            r0 = min(ny, r0)
            r1 = min(ny, r0 + rows)
            cnt[r0:r1, window_emits(strip * (cols - 4), wl, nx)] += 1
    return cnt


# ---- the sweep
@pytest.mark.parametrize("ncu", NCUS)
@pytest.mark.parametrize("form", list(FORMS))
def test_every_pixel_is_emitted_exactly_once(form, ncu):
    G, kdt, cols, per_cu = FORMS[form]
    blocks_seen = set()
    nquad = 0
    for reserve in reserves(ncu, per_cu):
        for nx in NXS:
            for ny in NYS:
                what = f"{form} {ny} x {nx}, {ncu} CUs, reserve {reserve}"
                g = geo(G, kdt, ny, nx, ncu, reserve)
                check_geometry(g, cols, ny, nx, what)
                nquad += g["nq"] > 0
                key = (g["nstrips"] - (g["nq"] > 0), g["nr"])
                if key not in blocks_seen:
                    blocks_seen.add(key)
                    assert blocks_ok(*key), what
                u = geo(G, kdt, ny, nx, ncu, reserve, quad_ok=False)
                if u != g:
                    assert g["nq"] > 0, f"{what}: quad_ok changed a uniform grid"
                    assert u["nq"] == 0 and u["rows_q"] == 0, f"{what}: quad_ok = 0 must give the uniform grid"
                    check_geometry(u, cols, ny, nx, what + ", quad_ok 0")
                if per_cu == 1 and reserve:   # the narrow forms fill their CUs: they take no reserve
                    assert g == geo(G, kdt, ny, nx, ncu, 0), f"{what}: a narrow form honoured the reserve"
    assert nquad > 0, "the sweep never met quad mode on this form"


@pytest.mark.parametrize("form", list(FORMS))
def test_factored_count_agrees_with_brute_force(form):
    G, kdt, cols, per_cu = FORMS[form]
    modes = set()
    for ncu, reserve in ((8, 0), (32, 8), (256, 8), (256, 0), (304, 8), (64, 64 * per_cu + 5)):
        for ny, nx in ((16, 128), (17, 512), (40, 512), (136, 512), (1001, 512), (720, 768), (999, 768), (1001, 768), (529, 1152),
                       (353, 1280), (264, 4096), (1400, 1536), (300, 2304)):
            for quad_ok in (True, False):
                g = geo(G, kdt, ny, nx, ncu, reserve, quad_ok)
                check_geometry(g, cols, ny, nx, f"{form} {ny} x {nx}")
                cnt = pixel_counts(g, ny, nx)
                assert cnt.min() == 1 and cnt.max() == 1, f"{form} {ny} x {nx}, {ncu} CUs, reserve {reserve}: {g}"
                modes.add(g["nq"] > 0)
    assert modes == {True, False}


def test_the_restated_contract_notices_a_wrong_geometry():
    """the checks above are not vacuous: each kind of wrong geometry fails one of them"""
    g = geo(8, F64, 1001, 768, 256, 8)
    assert g["nq"] > 0
    assert not row_counts_ok(1001, g["nr"] - 7, g["rows"])          # ranges that stop short of the frame
    assert not row_counts_ok(1001, 6 * g["nq"], g["rows_q"] - 1)
    assert column_counts_ok(256, 768, True) and column_counts_ok(256, 768, False)   # a last strip of 12 live columns: either way
    assert not column_counts_ok(256, 896, True)                     # ... one of 140 live columns as a 64-lane window is not
    assert pixel_counts(dict(g, rows_q=g["rows_q"] - 1), 1001, 768).min() == 0      # quad ranges that stop short
    cnt = pixel_counts(dict(g, nq=0, rows_q=0, grid=g["nr"] * 3), 1001, 768)        # (the uniform grid of the same ranges is sound)
    assert cnt.min() == 1 and cnt.max() == 1


def test_geometry_depends_on_the_form_only():
    """not on the Legendre planes; on the group count and the ipc4d dtype only through the form"""
    for form, (G0, kdt, cols, per_cu) in FORMS.items():
        counts = range(5, 9) if G0 == 8 else range(9, 17)
        for ncu in (64, 256, 304):
            for reserve in (0, 8):
                for ny, nx in ((16, 128), (136, 512), (720, 768), (1001, 768), (1376, 512), (528, 1152), (352, 1280), (1160, 896),
                               (264, 4096), (4096, 4096), (4224, 6272)):
                    want = geo(G0, kdt, ny, nx, ncu, reserve)
                    for G in counts:
                        for planes in (4, 9, 11):
                            assert geo(G, kdt, ny, nx, ncu, reserve, planes=planes) == want, f"{form}: {G} groups, {planes} planes"


def test_configurations_without_a_form_or_frame_report_zero():
    lib = _native.load_library()
    out = (_native.C.c_int * 8)()
    assert lib.rip_chain_geometry_for(9, 8, F32, F32, 720, 768, 256, 8, 1, out) == 2
    for args in ((9, 4, F32, F32, 720, 768, 256, 8, 1), (9, 17, F32, F32, 720, 768, 256, 8, 1), (5, 8, F32, F32, 720, 768, 256, 8, 1),
                 (9, 8, F32, F64, 720, 768, 256, 8, 1), (9, 8, _native.RIP_U16, F32, 720, 768, 256, 8, 1),
                 (9, 8, F32, F32, 15, 768, 256, 8, 1), (9, 8, F32, F32, 720, 700, 256, 8, 1), (9, 8, F32, F32, 720, 0, 256, 8, 1),
                 (9, 8, F32, F32, 720, 768, 0, 8, 1)):
        assert lib.rip_chain_geometry_for(*args, out) == 0, args
    assert lib.rip_chain_geometry_for(9, 8, F32, F32, 720, 768, 256, 8, 1, None) == 0
    assert geo(8, F32, 720, 768, 256, -3) == geo(8, F32, 720, 768, 256, 0)   # (rip_set_option stores a negative reserve as 0)


# ---- known answers at the 256 CUs of an MI355X, default reserve
def mode(form, ny, nx, ncu=256, reserve=8):
    G, kdt, _cols, _per_cu = FORMS[form]
    g = geo(G, kdt, ny, nx, ncu, reserve)
    return "quad" if g["nq"] else "uniform"


def test_which_shapes_of_the_older_tests_run_quad_mode():
    """what the suite reached before this file: quad mode on the 256-column f32 form at nx = 4096 only"""
    assert geo(8, F32, 4096, 4096, 256, 8) == dict(cols=256, nstrips=17, live_last=64, nr=31, rows=133, nq=8, rows_q=128, grid=504)
    assert geo(8, F32, 4096, 4096, 256, 8, quad_ok=False) == dict(cols=256, nstrips=17, live_last=64, nr=29, rows=142, nq=0, rows_q=0,
                                                                  grid=493)
    assert mode("f32_5to8", 264, 4096) == "quad"
    for form in ("f64_5to8", "f32_9to16", "f64_9to16"):
        assert mode(form, 264, 4096) == "uniform" and mode(form, 4096, 4096) == "uniform", form
    # f64 x 16 groups at 4096 x 4096: eligible (64 live columns), loses at 256 CUs, wins at 304
    assert geo(16, F64, 4096, 4096, 256, 8)["live_last"] == 64 and mode("f64_9to16", 4096, 4096, ncu=304) == "quad"
    for form in FORMS:
        # the small 512-wide frames: eligible where the window is 256 columns (8 live columns), too short for quad mode
        for ny in (40, 136):
            assert mode(form, ny, 512) == "uniform", form
        # the seam frame: a last strip of 136 / 140 live columns
        g = geo(FORMS[form][0], FORMS[form][1], 1160, 896, 256, 8)
        assert g["live_last"] == (140 if g["cols"] == 256 else 136) and g["nq"] == 0, form
    # a 384-column window has a last strip of at most 64 live columns only where nx is a multiple of 384
    for nx in NXS:
        n = strip_count(384, nx)
        assert (n > 1 and nx - (n - 1) * 380 <= 64) == (nx % 384 == 0 and nx > 384), nx


QUAD_SHAPES = [   # the shapes tests/test_gpu_chain_geometry.py runs: form, ny, nx, live columns, nr, nq
    ("f32_5to8", 1376, 512, 8, 172, 43), ("f64_5to8", 720, 768, 8, 90, 15), ("f64_5to8", 528, 1152, 12, 66, 11),
    ("f32_9to16", 720, 768, 8, 90, 15), ("f32_9to16", 528, 1152, 12, 66, 11), ("f64_9to16", 704, 512, 8, 88, 22),
    ("f64_9to16", 544, 768, 12, 68, 17), ("f64_9to16", 352, 1280, 20, 44, 11),
]


@pytest.mark.parametrize("form,ny,nx,live,nr,nq", QUAD_SHAPES)
def test_quad_shapes_of_the_gpu_tests(form, ny, nx, live, nr, nq):
    G, kdt, cols, _per_cu = FORMS[form]
    g = geo(G, kdt, ny, nx, 256, 8)
    # ranges of 8 rows in both decompositions: ny / 8 ranges down a full strip, cols / 64 of them per quad workgroup
    assert (g["live_last"], g["nr"], g["rows"], g["nq"], g["rows_q"]) == (live, nr, 8, nq, 8), g
    assert nr == ny // 8 and nq == -(-ny // (8 * (cols // 64)))


def test_the_16_group_quad_shapes_of_the_gpu_tests():
    assert geo(16, F32, 1040, 768, 256, 8) == dict(cols=384, nstrips=3, live_last=8, nr=118, rows=9, nq=20, rows_q=9, grid=256)
    assert geo(16, F64, 1040, 512, 256, 8) == dict(cols=256, nstrips=3, live_last=8, nr=115, rows=10, nq=26, rows_q=10, grid=256)
    # (the 720 x 768 and 704 x 512 of the other counts run quad mode at 16 groups too)
    assert geo(16, F32, 720, 768, 256, 8)["nq"] == 15 and geo(16, F64, 704, 512, 256, 8)["nq"] == 22


def test_ragged_heights_on_the_384_column_forms():
    for form in ("f64_5to8", "f32_9to16"):
        G, kdt, _cols, _per_cu = FORMS[form]
        # 1001 rows: 118 ranges of 9 rows down a full strip -- 111 full ones, one of 2 rows, six empty -- and 19 quad workgroups of
        # six wave columns: the last one has four working (the fourth on 2 rows) and two empty
        g = geo(G, kdt, 1001, 768, 256, 8)
        assert g == dict(cols=384, nstrips=3, live_last=8, nr=118, rows=9, nq=19, rows_q=9, grid=255), form
        assert 1001 - 111 * 9 == 2 and 118 - 112 == 6 and 112 - 18 * 6 == 4
        # 999 rows: 111 full ranges, the last quad workgroup has three working and three empty wave columns
        g = geo(G, kdt, 999, 768, 256, 8)
        assert (g["nr"], g["rows"], g["nq"], g["rows_q"]) == (118, 9, 19, 9) and 999 == 111 * 9 and 111 - 18 * 6 == 3, form
    g = geo(11, F64, 1001, 512, 256, 8)
    assert g == dict(cols=256, nstrips=3, live_last=8, nr=114, rows=9, nq=28, rows_q=9, grid=256)


def test_the_second_pass_of_the_quad_search():
    """A reserve that leaves the first pass of the search no room (fewer than two slots): the search runs again without it.  Only
    then can a grid be in quad mode although slots - reserve <= 1; what it finds is what a reserve of 0 finds, since neither the
    second pass nor the uniform grid it competes with (slots / strips ranges when the reserve leaves none) sees the reserve."""
    slots = 2 * 256
    free = geo(8, F32, 1376, 512, 256, 0)
    assert free["nq"] == 43
    for reserve in (slots - 1, slots, slots + 5, 100000):
        assert geo(8, F32, 1376, 512, 256, reserve) == free, reserve
    # a first pass that still has room keeps the reserve: 12 slots give 2 x 5 ranges of 276 rows + 2 quad workgroups (8 x 172 rows)
    assert geo(8, F32, 1376, 512, 256, slots - 12) == dict(cols=256, nstrips=3, live_last=8, nr=5, rows=276, nq=2, rows_q=172, grid=12)
    # ... and one whose quad search loses to the uniform grid stays uniform: 4 slots, one range per strip
    assert geo(8, F32, 1376, 512, 256, slots - 4) == dict(cols=256, nstrips=3, live_last=8, nr=1, rows=1376, nq=0, rows_q=0, grid=3)
    # at this height a range is 8 rows -- the shortest the launcher makes -- with or without the default reserve; a frame of four
    # strips shows the reserve: 8 slots fewer, longer quad ranges
    assert geo(8, F32, 1376, 512, 256, 8) == free
    a, b = geo(8, F32, 1248, 768, 256, 0), geo(8, F32, 1248, 768, 256, 8)
    assert (a["nr"], a["rows"], a["nq"], a["rows_q"], a["grid"]) == (156, 8, 39, 8, 507)
    assert (b["nr"], b["rows"], b["nq"], b["rows_q"], b["grid"]) == (156, 8, 35, 9, 503) and b["grid"] <= slots - 8
