"""CPU-only: tests/darkstack_ref.py, the numpy restatement of the dark-file arithmetic, by closed forms; the proof that no input of
tests/test_gpu_darkstack.py has a borderline pixel (so that the GPU tests may compare every pixel bit for bit); and
calio.read_fits_image on files written here."""

import os
import re
from fractions import Fraction

import darkstack_cases as dc
import darkstack_ref as dr
import numpy as np
import pytest
from conftest import REPO, assert_same_bits

from romanimpreprocess_amd import _native, calio

F = np.float32


# ------------------------------------------------------------------------------------------------ the clip, closed forms
@pytest.mark.parametrize("k", [1, 2, 6, 7, 8, 40])
def test_k_equal_values_and_one_outlier(k):
    """k values v and one v + d: c = v (k >= 2), m = v + d / (k+1), s = d sqrt(k) / (k+1); the outlier goes when d > 3 s, i.e. when
    (k+1)^2 > 9 k: for k >= 7 (64 > 63) and not for k <= 6 (49 < 54).  With it gone the column is constant and keeps the rest."""
    v, d = 64.0, 16.0
    col = np.array([v] * k + [v + d], F)[:, None]
    mean, count, border = dr.sigma_clip_mean(col)
    assert not border[0]
    if (k + 1) ** 2 > 9 * k:
        assert k >= 7 and count[0] == k and mean[0] == F(v)
    else:
        assert k <= 6 and count[0] == k + 1 and mean[0] == F(v + d / (k + 1))


def test_outlier_that_falls_in_the_second_round():
    a = dc.second_round()
    assert np.all(dr.sigma_clip_mean(a, maxiters=1)[1] == 31)   # 1000 only
    mean, count, border = dr.sigma_clip_mean(a)
    assert np.all(count == 30) and not border.any()
    keep = np.sort(a, axis=0)[:30]
    assert np.all(np.abs(mean - keep.astype(np.float64).mean(axis=0)) < 1e-6)


def test_ladder_drops_its_top_value_every_round():
    a = dc.ladder()
    for rounds in range(8):
        mean, count, border = dr.sigma_clip_mean(a, maxiters=rounds)
        assert np.all(count == 16 - rounds) and not border.any()
        # the survivors are 2^0 .. 2^(15-rounds) times the pixel's scale: their sum is 2^(16-rounds) - 1
        scale = a.min(axis=0).astype(np.float64)
        assert_same_bits(mean, ((2.0 ** (16 - rounds) - 1) * scale / (16 - rounds)).astype(F), f"{rounds} rounds")
    assert np.all(dr.sigma_clip_mean(a, maxiters=5)[1] == 11)            # stopped early
    assert np.all(dr.sigma_clip_mean(a, maxiters=7)[1] == 9)
    assert np.all(dr.sigma_clip_mean(a, maxiters=16)[1] == 9)            # converged: 7 values left would need (7+1)^2 > 9 * 7


@pytest.mark.parametrize("n", [5, 6])
def test_a_chosen_median(n):
    """the centre is the MEDIAN, not the mean: values 0 .. n-2 and one far value, sigma so small that only the distance from the
    centre decides"""
    col = np.array(list(range(n - 1)) + [1000.0], F)[:, None]
    c = np.median(col)                      # 2 for n = 5; (2 + 3) / 2 = 2.5 for n = 6
    assert c == (2.0 if n == 5 else 2.5)
    s = np.std(col.astype(np.float64))
    width = 1.6 / s                         # bounds c +- 1.6: keeps the values within 1.6 of the median
    mean, count, _ = dr.sigma_clip_mean(col, sigma=width, maxiters=1)
    kept = [v for v in col[:, 0] if abs(v - c) <= 1.6]
    assert count[0] == len(kept) == (3 if n == 5 else 4)
    assert mean[0] == F(np.mean(kept))


def test_values_on_a_bound_stay_and_the_sums_behind_them_are_exact():
    a = dc.on_bound()
    mean, count, border = dr.sigma_clip_mean(a, sigma=1.0)
    assert np.all(count == 2) and not border.any()
    assert_same_bits(mean, F(0.5) * (a[0] + a[1]))
    mean, count, _ = dr.sigma_clip_mean(a, sigma=0.5)
    assert list(count) == [0, 0, 0, 2] and np.isnan(mean[:3]).all() and mean[3] == 3.0
    for x, y in a.T:   # m, the deviations and their squares are exact: no order of summation changes s
        m = Fraction(float(x)) + Fraction(float(y))
        assert Fraction((float(x) + float(y)) / 2) == m / 2
        d = float(x) - float(m / 2)
        assert Fraction(d) == Fraction(float(x)) - m / 2 and Fraction(d * d) == Fraction(d) ** 2
        assert Fraction(d * d + d * d) == 2 * Fraction(d) ** 2
    c = dc.constant()   # a constant column: n * v is exact in f64 for n = 10 and a 24-bit v, so m = v and every deviation is 0
    mean, count, border = dr.sigma_clip_mean(c)
    assert np.all(count == 10) and not border.any()
    assert_same_bits(mean, c[0])
    for v in c[0]:
        assert Fraction(float(v) * 10) == 10 * Fraction(float(v))


def test_nonfinite_values_and_zeros():
    a = dc.nonfinite()
    mean, count, _ = dr.sigma_clip_mean(a)
    assert list(count[:4]) == [0, 0, 1, 0] and np.isnan(mean[[0, 1, 3]]).all() and mean[2] == 5.0
    assert np.all(count[4:] <= np.isfinite(a[:, 4:]).sum(axis=0)) and np.isfinite(mean[4:]).all()
    z = dc.signed_zeros()
    mean, count, _ = dr.sigma_clip_mean(z)
    assert np.all(count[:5] == 16) and np.all(mean[:5] == 0) and not np.signbit(mean[:5]).any()
    assert mean[5] < 0


def test_plane_order_is_what_nanmean_does():
    a = dc.nonfinite()[:, 4:].astype(np.float64)
    a[~np.isfinite(a)] = np.nan
    tot = np.zeros(a.shape[1])
    for p in a:
        tot = tot + np.where(np.isnan(p), 0.0, p)
    assert_same_bits(np.nanmean(a, axis=0), tot / np.count_nonzero(~np.isnan(a), axis=0))


# ------------------------------------------------------------------------------------------------ no borderline pixel
def test_no_input_of_the_gpu_tests_is_borderline():
    for name, (stack, kw) in dc.clip_cases().items():
        assert not dr.sigma_clip_mean(stack, **kw)[2].any(), name
    a = dc.noisy(37, 199, 120)
    assert not dr.sigma_clip_mean(a[:20])[2].any()                      # the `n < capacity` and plane-stride cases
    nx = 64
    stack = np.stack([dr.group_means(c, dc.READS_E2E, nx) for c in dc.dark_exposures()], axis=1)
    for g in range(stack.shape[0]):
        for sigma in (3.0, 1.5):
            assert not dr.sigma_clip_mean(stack[g], sigma=sigma)[2].any(), (g, sigma)
    assert np.any(dr.sigma_clip_mean(stack[2], sigma=1.5)[1] < 5)        # at 1.5 sigma five exposures do lose values


# ------------------------------------------------------------------------------------------------ group means
def test_np_mean_is_the_sequential_f32_sum():
    for cube, reads in ((dc.cube_u16(30, 5, 140, 50), dc.READS_MIXED), (dc.cube_300(2, 24), [0, 300, 1, 300, 7, 290])):
        assert_same_bits(dr.group_means(cube, reads), dr.group_means_sequential(cube, reads))
    # and the order does show on the 300 reads: the exact mean is another number
    c = dc.cube_300(2, 24)
    assert np.any(dr.group_means(c, [0, 300])[0] != c.astype(np.float64).mean(axis=0).astype(F))
    raw = dr.to_fits_be16(c)
    assert raw.dtype == np.dtype(">i2") and np.array_equal(dr.from_fits_be16(raw), c)


def test_dark_planes_follow_numpy_promotion():
    x = (1 + np.arange(4000)).astype(F) / F(7)
    _, _, rn = dr.dark_planes(x[None], x[None], x[None], x[None], x[None], 4000)
    assert rn.dtype == F
    assert_same_bits(rn[0], (x.astype(np.float64) / np.sqrt(2.0)).astype(F))      # np.sqrt(2) is a float64 scalar: not weak
    assert np.any(rn[0] != x / F(np.sqrt(2)))                                       # a float32 division is another result


# ------------------------------------------------------------------------------------------------ the FITS reader
def test_fits_reader_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    i2 = rng.integers(-32768, 32768, (3, 5, 7)).astype(np.int16)
    f4 = rng.standard_normal((2, 9, 11)).astype(F)
    f8 = rng.standard_normal((4, 6))
    path = tmp_path / "t.fits"
    cards = [("BSCALE", 1), ("BZERO", 32768), ("OBSERVER", "it's me"), ("GAIN", 1.5), ("FLAG", False)]
    with open(path, "wb") as f:
        f.write(dc.fits_hdu(i2, cards))
        f.write(dc.fits_hdu(f4, [("EXTNAME", "NOISE"), ("DARK1", 0), ("CDS", 1)], extension=True))
        f.write(dc.fits_hdu(None, [("EXTNAME", "EMPTY")], extension=True))
        f.write(dc.fits_hdu(f8, [("EXTNAME", "AMP33"), ("M_PINK", 0.25)], extension=True, pad=False))   # a partial last block
    assert os.path.getsize(path) % 2880 == 4 * 6 * 8
    h, d = calio.read_fits_image(path, 0)
    assert isinstance(h, dict) and h["BITPIX"] == 16 and h["NAXIS3"] == 3 and h["BZERO"] == 32768 and h["OBSERVER"] == "it's me"
    assert h["GAIN"] == 1.5 and h["FLAG"] is False
    assert len(h.text) % 80 == 0 and h.text.endswith("END".ljust(80)) and h.text.startswith("SIMPLE  =")
    assert isinstance(d, np.memmap) and d.dtype == np.dtype(">i2") and d.shape == (3, 5, 7) and np.array_equal(d, i2)
    assert np.array_equal(dr.from_fits_be16(d), (i2.astype(np.int32) + 32768).astype(np.uint16))
    h1, d1 = calio.read_fits_image(path, 1)
    assert h1["EXTNAME"] == "NOISE" and d1.dtype == np.dtype(">f4") and np.array_equal(d1, f4)
    hn, dn = calio.read_fits_image(path, "noise")
    assert hn == h1 and np.array_equal(dn, f4)
    assert calio.read_fits_image(path, 2)[1] is None
    h3, d3 = calio.read_fits_image(path, "AMP33")
    assert h3["M_PINK"] == 0.25 and d3.dtype == np.dtype(">f8") and np.array_equal(d3, f8)
    assert np.array_equal(calio.read_fits_image(path, 3)[1], f8)
    with pytest.raises(KeyError):
        calio.read_fits_image(path, "NOPE")
    with pytest.raises(KeyError):
        calio.read_fits_image(path, 4)
    # a header that fills its 2880-byte block exactly (36 cards), and a truncated data block
    filler = [(f"K{i}", i) for i in range(36 - 6 - 1)]
    one = dc.fits_hdu(f4, filler)
    assert one.find(b"END     ") == 35 * 80 and len(one) == 2880 + 2880 * ((f4.nbytes + 2879) // 2880)
    p2 = tmp_path / "full.fits"
    p2.write_bytes(one)
    assert np.array_equal(calio.read_fits_image(p2)[1], f4)
    p2.write_bytes(one[:2880 + f4.nbytes - 4])
    with pytest.raises(ValueError, match="needs"):
        calio.read_fits_image(p2)
    p2.write_bytes(dc.fits_hdu(f4.astype(np.float64).astype(np.int16), [])[:2880].replace(b"BITPIX  =                   16",
                                                                                       b"BITPIX  =                   32") + b"\0" * 2880)
    with pytest.raises(ValueError, match="BITPIX"):
        calio.read_fits_image(p2)


# ------------------------------------------------------------------------------------------------ the interface
def test_new_entries_are_declared_bound_and_listed():
    hdr = open(os.path.join(REPO, "include", "romanhip.h")).read()
    host = open(os.path.join(REPO, "romanimpreprocess_amd", "csrc", "rip_host.h")).read()
    mk = open(os.path.join(REPO, "romanimpreprocess_amd", "csrc", "Makefile")).read()
    for name in ("rip_cal_group_means", "rip_cal_sigma_clip_mean", "rip_cal_dark_planes"):
        assert re.search(rf"\bint {name}\(", hdr), name
        assert name in _native.SYMBOLS
    assert "rip_cal_group_means, _sigma_clip_mean, _dark_planes" in host and "darkstack.hip" in mk
    assert "parity with astropy is unpinned" in hdr
