"""The references that ``test_gpu_post_edges.py`` holds the post-path kernels to, checked on the CPU against independent
statements of the same operations (scipy's convolution, float64 means, the reference's documented behaviour)."""

import warnings

import numpy as np
import pytest
import scipy.signal
from conftest import assert_same_bits

import post_edge_refs as refs
from oracle import post


@pytest.mark.parametrize("shape", [(37, 513), (2, 257), (300, 5), (1, 1)])
def test_build_mask_restatement_equals_per_bit_convolutions(shape):
    """oracle.post.build_mask with random growth tables over all 32 bits (PixelMask1 uses 23 bits and never bit 31) against
    maskhandling.py's own recipe: each flagged bit's layer convolved with its footprint (mode "same", zero padded)."""
    rng = np.random.default_rng(shape[1])
    for _ in range(3):
        table = refs.random_growth_table(rng)
        assert set(table.tolist()) == set(refs.GROWTHS) and table[31] != 0
        dq = refs.random_dq(rng, shape)
        want = np.zeros(shape, bool)
        for bit, g in enumerate(table):
            if g:
                layer = ((dq >> np.uint32(bit)) & np.uint32(1)).astype(np.int64)
                want |= scipy.signal.convolve(layer, refs.KERNELS[int(g)], mode="same", method="direct") > 0
        got = post.build_mask(dq, refs.table_dict(table))
        assert_same_bits(got, want, f"build_mask {shape}")
        if dq.size > 1000:
            ungrown = np.zeros(shape, bool)
            for bit, g in enumerate(table):
                if g:
                    ungrown |= (dq & np.uint32(1 << bit)) != 0
            assert ungrown.sum() < got.sum() < got.size   # the growth shows, and flagged bits of growth 0 mask nothing
            assert np.any((dq != 0) & ~got)


def test_build_mask_restatement_refuses_an_unknown_growth():
    with pytest.raises(ValueError):
        post.build_mask(np.ones((3, 3), np.uint32), {0: 3})


def test_single_pixel_footprints_have_the_documented_sizes():
    for growth, size in ((0, 0), (1, 1), (5, 5), (9, 9), (25, 25)):
        assert refs.footprint((9, 9), 4, 4, growth).sum() == size
        dq = np.zeros((9, 9), np.uint32)
        dq[4, 4] = 1 << 31
        assert_same_bits(post.build_mask(dq, {31: growth}), refs.footprint((9, 9), 4, 4, growth), f"growth {growth}")
    assert refs.footprint((6, 6), 0, 0, 25).sum() == 9 and refs.footprint((1, 7), 0, 3, 9).sum() == 3


@pytest.mark.parametrize("shape,k", refs.BIN_CASES)
@pytest.mark.parametrize("masked", [False, True])
def test_same_order_f32_bin_loop_is_within_the_bound_of_the_f64_mean(shape, k, masked):
    arr, mask = refs.bin_inputs(np.random.default_rng(k), shape)
    mask = mask if masked else None
    got = refs.bin_mean_same_order(arr, mask, k)
    mean64, meanabs = refs.bin_mean_f64(arr, mask, k)
    assert got.dtype == np.float32 and got.shape == (shape[0] // k, shape[1] // k)
    assert np.array_equal(np.isnan(got), np.isnan(mean64))
    ok = ~np.isnan(mean64)
    assert ok.sum() > 3
    assert np.all(np.abs(got.astype(np.float64) - mean64)[ok] <= refs.bin_bound(meanabs, k)[ok])
    if mask is None:   # and it is the reference's binkxk up to the summation order
        np.testing.assert_allclose(got, post.binkxk(arr, k), rtol=k * k * 2.0 ** -22, atol=1e-4)


def _quiet(f, *a, **kw):
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return f(*a, **kw)


def test_smooth_mode_restatement_on_degenerate_images():
    """What the reference's sky.smooth_mode leaves for an image without spread: sigma = 0 (or NaN) makes every weight NaN, every
    density 0, and the parabola's vertex 0 / 0."""
    const = np.full((12, 20), 3.25, np.float32)
    ctr, width = _quiet(post.smooth_mode, const)
    assert np.isnan(ctr) and width == 0.0
    holes = const.copy()
    holes[::3, ::2] = np.nan
    ctr, width = _quiet(post.smooth_mode, holes)
    assert np.isnan(ctr) and width == 0.0
    ctr, width = _quiet(post.smooth_mode, np.full((12, 20), np.nan, np.float32))
    assert np.isnan(ctr) and np.isnan(width)


@pytest.mark.parametrize("G", [1, 2, 8])
def test_endslice_restatement_without_a_border(G):
    rng = np.random.default_rng(G)
    rdq = (rng.integers(0, 256, size=(G, 5, 9))).astype(np.uint8)
    got = post.endslice(rdq, 0)
    assert got.shape == (5, 9) and got.dtype == np.int8
    assert_same_bits(got, refs.endslice_loop(rdq, 0), "endslice, nb = 0")
    assert_same_bits(post.endslice(rdq, 2), refs.endslice_loop(rdq, 2), "endslice, nb = 2")
    assert_same_bits(post.endslice(rdq, 2), got[2:-2, 2:-2], "endslice is per pixel")
    # pixel by pixel, the slow way
    for y in range(5):
        for x in range(9):
            rises = [i - 1 for i in range(1, G) if rdq[i, y, x] & 2 and not rdq[i - 1, y, x] & 2]
            assert got[y, x] == (rises[-1] if rises else -1)
