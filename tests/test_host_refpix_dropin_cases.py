"""The case table of the reference-pixel image drop-ins (refpix_dropin_cases.py) is what it claims to be: every median count it
names occurs, every parameter value meets every update form, and each value family really puts its values where the medians
are taken.  numpy only: runs without a GPU."""

import hashlib
import itertools
import warnings

import numpy as np
from conftest import assert_same_bits, load_golden

import refpix_dropin_cases as rc
from oracle import refpix as orp


def _pow2(n):
    return n & (n - 1) == 0


def test_every_named_median_count_occurs():
    row = set(itertools.chain.from_iterable(rc.row_median_counts(c) for c in rc.ROW_CASES))
    chan = {rc.chan_median_count(c) for c in rc.CHAN_CASES}
    # ctr over ny row medians: a single one, even, odd and padded, at and just over the block size, odd over two strides
    assert {1, 2, 5, 37, 1024, 1025, 2049} <= {c.ny for c in rc.ROW_CASES}
    # science medians: 8, 16, 128 and 1029 values (odd, padded, strided) -- only taken by the fit and the medians-only forms
    sci = {c.nside - 8 for c in rc.ROW_CASES if c.form in ("fit", "medians")}
    assert {8, 16, 128, 1029} <= sci
    assert {8, 128} <= row
    # windows: 512 (a channel), 480, 4, 12, 516 (one shared column), 768, 1028 (over the block size, padded)
    assert chan == {512, 480, 4, 12, 516, 768, 1028}
    counts = row | chan
    assert any(n & 1 and n > 1 for n in counts)                              # the single-middle-element branch
    assert any(not _pow2(n) for n in counts)                                  # +inf padding
    assert any(n < rc.BLOCK and not _pow2(n) for n in counts)                 # a stride loop that does not fill the block
    assert {rc.BLOCK, rc.BLOCK + 1} <= counts                                 # at and just over the block size
    assert any(n > 2 * rc.BLOCK for n in counts)                              # two full strides and a rest
    assert all(n <= rc.MAX_SORT for n in counts)


def test_every_parameter_value_meets_every_update_form():
    geo = [c for c in rc.ROW_CASES if c.family == "noise"]
    for form in rc.ROW_FORMS:
        mine = [c for c in geo if c.form == form]
        nys = {ny for ny in rc.ROW_NYS if form != "fit" or ny >= rc.FIT_MIN_NY}
        assert {c.ny for c in mine} == nys, form
        assert {c.nside for c in mine} == set(rc.ROW_NSIDES), form
        assert {(c.use_ref, c.extra) for c in mine} == set(rc.ROW_WIDTHS), form
    assert all(c.ny >= rc.FIT_MIN_NY for c in rc.ROW_CASES if c.form == "fit")
    assert all(c.form != "fit" for c in rc.ROW_CASES if c.family == "nan")    # NaN only with a given slope
    assert len({c.name for c in rc.ROW_CASES}) == len(rc.ROW_CASES)
    for c in rc.ROW_CASES:
        assert rc.row_image(c).shape == (c.ny, rc.row_width(c))
        assert rc.row_width(c) >= c.nside + (128 if c.use_ref else 0)


def test_channel_table_covers_rows_windows_and_counts():
    geo = [c for c in rc.CHAN_CASES if c.family == "noise"]
    assert {c.ny for c in geo} == set(rc.CHAN_NYS)
    assert {(c.start, c.end) for c in geo} == set(rc.CHAN_WINDOWS)
    assert {(c.n_channels, c.use_ref) for c in geo} == set(itertools.product((1, 2, 5), (False, True)))
    assert {c.extra for c in geo} == {0, 3}
    # every overlapping width runs with more than one window, so that a window sees the update of the one before it
    for win in ((0, 129), (0, 192), (0, 257)):
        assert any((c.start, c.end) == win and rc.chan_windows(c) > 1 for c in geo), win
    assert len({c.name for c in rc.CHAN_CASES}) == len(rc.CHAN_CASES)
    for c in rc.CHAN_CASES:
        assert rc.chan_image(c).shape == (c.ny, c.end + (rc.chan_windows(c) - 1) * 128 + c.extra)
    families = {"noise", "ties", "const", "zeros", "inf", "nan"}
    assert {c.family for c in rc.CHAN_CASES} == families
    assert {c.family for c in rc.ROW_CASES} == families | {"huge"}


def _middle(values):
    """the two middle elements (the same one twice for an odd count) of the sorted values"""
    s = np.sort(np.asarray(values).ravel())
    return s[(s.size - 1) // 2], s[s.size // 2]


def _row_windows(c, img):
    cols = rc.row_ref_columns(c)
    return [img[r, cols] for r in range(c.ny)]


def _chan_windows(c, img):
    out = []
    for k in range(rc.chan_windows(c)):
        sl = slice(c.start + 128 * k, c.end + 128 * k)
        out += [img[0:4, sl], img[c.ny - 4:c.ny, sl]]
    return out


def _family_windows(family):
    for c in rc.ROW_CASES:
        if c.family == family:
            yield c.name, _row_windows(c, rc.row_image(c))
    for c in rc.CHAN_CASES:
        if c.family == family:
            yield c.name, _chan_windows(c, rc.chan_image(c))


def test_tie_family_has_equal_middle_elements_and_straddled_runs():
    for name, wins in _family_windows("ties"):
        assert all(np.unique(w).size <= 3 for w in wins)
        mids = [_middle(w) for w in wins]
        assert any(lo == hi for lo, hi in mids), name
    # and a window whose middle elements straddle two runs (the mean of two different values) occurs in the family
    assert any(lo != hi for _, wins in _family_windows("ties") for lo, hi in map(_middle, wins))


def test_zero_family_has_minus_zero_middle_elements_where_numpy_gives_plus_zero():
    for name, wins in _family_windows("zeros"):
        hit = 0
        for w in wins:
            s = np.sort(w.ravel(), kind="stable")
            zeros = w.ravel()[w.ravel() == 0]
            # sort() leaves -0 and +0 in any order; the windows made for this hold no +0 at all, so the middle is -0 whatever
            # the order
            lo, hi = s[(s.size - 1) // 2], s[s.size // 2]
            if lo == 0 and hi == 0 and zeros.size and np.all(np.signbit(zeros)):
                med = np.median(w)
                assert med == 0 and not np.signbit(med), name     # np.median: +0
                hit += 1
        assert hit >= 2, name
    # pixels that are exactly -0 and +0 outside the reference windows
    for c in rc.ROW_CASES + rc.CHAN_CASES:
        if c.family == "zeros":
            img = rc.row_image(c) if isinstance(c, rc.RowCase) else rc.chan_image(c)
            z = img[img == 0]
            assert np.any(np.signbit(z)) and np.any(~np.signbit(z)), c.name
    # the oracle's medians of those cases never carry the sign
    for c in rc.ROW_CASES:
        if c.family == "zeros":
            _, ref, _, ctr, _ = rc.row_oracle(c, rc.row_image(c))
            assert np.count_nonzero(ref == 0) >= 2 * c.ny // 3 and not np.any(np.signbit(ref[ref == 0])), c.name
            assert ctr == 0 and not np.signbit(ctr), c.name
    for c in rc.CHAN_CASES:
        if c.family == "zeros":
            _, table = rc.chan_oracle(c, rc.chan_image(c))
            assert np.all(table[0, :2] == 0) and not np.any(np.signbit(table[0, :2])), c.name


def test_inf_family_medians():
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for name, wins in _family_windows("inf"):
            meds = [np.median(w) for w in wins]
            assert any(m == np.inf for m in meds), name                       # more than half +inf
            assert any(m == -np.inf for m in meds), name                      # more than half -inf
            assert any(np.isfinite(m) and np.any(w == np.inf) and np.any(w == -np.inf) for m, w in zip(meds, wins)), name


def test_nan_family_puts_one_nan_inside_a_reference_window():
    for c in rc.ROW_CASES:
        if c.family == "nan":
            img = rc.row_image(c)
            assert np.count_nonzero(np.isnan(img)) == 1
            assert sum(int(np.isnan(w).any()) for w in _row_windows(c, img)) == 1, c.name
            out, ref, _, ctr, _ = rc.row_oracle(c, img)
            assert np.isnan(ctr) and np.count_nonzero(np.isnan(ref)) == 1
            assert np.isnan(out).all() or c.form == "medians"   # the reference turns the whole image into NaN
    for c in rc.CHAN_CASES:
        if c.family == "nan":
            img = rc.chan_image(c)
            assert np.count_nonzero(np.isnan(img)) == 1
            r, col = np.argwhere(np.isnan(img))[0]
            assert r < 4 and c.start + 128 <= col < c.end + 128, c.name        # a bottom reference row of window 1
            out, table = rc.chan_oracle(c, img)
            assert np.isnan(table[1, 0]) and np.isnan(out[:, c.start + 128:c.end + 128]).all()


def test_huge_family_takes_an_odd_median_above_half_the_float_range():
    (c,) = [c for c in rc.ROW_CASES if c.family == "huge"]
    _, _, sci, _, _ = rc.row_oracle(c, rc.row_image(c))
    assert (c.nside - 8) & 1
    assert np.all(np.isfinite(sci)) and np.all(sci > np.finfo(np.float32).max / 2)   # v + v overflows, the median does not


def test_two_point_channel_step_is_the_oracle_with_another_line():
    """channel_step_two_point against the oracle on a frame whose lines both fits give exactly (medians 0 and ny - 4 apart)"""
    c = rc.CHAN_BY_NAME["const-ny13-w0_128-n2+ref+3"]
    img = rc.chan_image(c)
    want, table = rc.chan_oracle(c, img)
    got, table2 = rc.channel_step_two_point(img.copy(), c.start, c.end, rc.chan_windows(c))
    assert_same_bits(table2[:, :2], table[:, :2], "medians")
    np.testing.assert_allclose(table2[:, 2:], table[:, 2:], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-5)


def test_channel_step_n_channels_default_is_the_old_behaviour():
    """oracle.refpix.channel_step: no n_channels and n_channels = nside // 128 give the reference's own output (golden fixture)"""
    from test_oracle_golden import REFPIX_VARIANTS, _refpix_variants_base

    g = load_golden("refpix_variants")
    kw = REFPIX_VARIANTS["chan_window"][1]
    base = _refpix_variants_base(int(g["seed"]))
    for extra in ({}, {"n_channels": 32}):
        im, table = orp.channel_step(base.copy(), 4096, kw["use_ref_channel"], kw["channel_start"], kw["channel_end"], **extra)
        assert table.shape == (33, 4)
        assert hashlib.sha256(im.tobytes()).hexdigest() == str(g["chan_window_sha256"]), extra
    small = rc.chan_image(rc.CHAN_BY_NAME["noise-ny8-w0_128-n1+0"])
    _, t1 = orp.channel_step(small.copy(), 128, False)
    _, t2 = orp.channel_step(small.copy(), 4096, False, n_channels=1)
    assert_same_bits(t1, t2, "table")
