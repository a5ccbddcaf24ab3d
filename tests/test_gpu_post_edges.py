"""Every post-path kernel of ``post.hip`` (and the mask-growing copy in ``stats.hip: l2_pack_kernel``) at its edges: rows wider
than one workgroup, frame corners, every growth / order / rank / group count, special float values, refusals, and device
pointers against host arrays.  The references are numpy sorts, ``np.nanpercentile`` / ``np.nanmedian``, ``oracle/post.py`` and
explicit float64 / ``math.fsum`` sums (``post_edge_refs.py``; ``test_host_post_refs.py`` checks those on the CPU)."""

import functools
import math
import warnings

import numpy as np
import pytest
import torch
from conftest import assert_same_bits, gpu_context
from scipy.special import legendre_p

import post_edge_refs as refs
from oracle import post
from romanimpreprocess_amd.devarray import DevArray
from romanimpreprocess_amd.utils import maskhandling, sky

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NAN32 = np.float32(np.nan)


def _quiet(f, *a, **kw):
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return f(*a, **kw)


def _t(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(DEV)


def _dev(a):
    return DevArray(torch.from_numpy(np.ascontiguousarray(a)).to(DEV)).sync()


def _f32_bits(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


# =========================================================================================== 1. mask growth
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (3, 2), (6, 6), (5, 300)])
def test_single_flagged_pixel_masks_its_clipped_footprint(shape):
    ctx = gpu_context()
    n = 0
    for growth in refs.GROWTHS:
        for y, x in refs.edge_positions(shape):
            bit = (7 * n + 31) % 32   # bit 31 first, then every other bit in turn
            n += 1
            dq = np.zeros(shape, np.uint32)
            dq[y, x] = np.uint32(1 << bit)
            got = maskhandling.CombinedMask({bit: growth}).build(dq, ctx=ctx)
            want = refs.footprint(shape, y, x, growth)
            assert_same_bits(got, want, f"growth {growth} of bit {bit} at ({y}, {x}) of {shape}")
            assert_same_bits(want, post.build_mask(dq, {bit: growth}), "footprint against the restatement")
            # the same pixel flagged with a bit the table does not list masks nothing
            other = maskhandling.CombinedMask({(bit + 1) % 32: 25}).build(dq, ctx=ctx)
            assert not other.any()


@pytest.mark.parametrize("shape", [(37, 513), (2, 257), (300, 5)])
def test_random_planes_with_random_growth_tables(shape):
    rng = np.random.default_rng(shape[0])
    for _ in range(3):
        table = refs.random_growth_table(rng)
        assert set(table.tolist()) == set(refs.GROWTHS) and table[31] != 0
        dq = refs.random_dq(rng, shape)
        if dq.size > 1000:   # flagged bits of growth 0 (the 514-pixel plane has some fifteen flagged pixels in all)
            assert np.any([(dq & np.uint32(1 << b)).any() for b in np.flatnonzero(table == 0)])
        got = maskhandling.CombinedMask(refs.table_dict(table)).build(dq, ctx=gpu_context())
        assert_same_bits(got, post.build_mask(dq, refs.table_dict(table)), f"build_mask {shape}")


def test_build_mask_refuses_an_unknown_growth():
    with pytest.raises(ValueError, match="growth 3 of bit 6"):
        maskhandling.CombinedMask({6: 3}).build(np.zeros((4, 4), np.uint32), ctx=gpu_context())


@pytest.mark.parametrize("nb", [1, 4])
def test_l2_pack_grows_the_mask_on_the_trimmed_plane(nb):
    """rip_stats_l2_pack called directly on device pointers: the fully flagged border must not grow into the active region
    (the reference masks the trimmed dq plane: zero padding starts at the active edge), image / err carry a zero border."""
    ctx = gpu_context()
    ny, nx = 23, 263
    rng = np.random.default_rng(nb)
    for _ in range(2):
        table = refs.random_growth_table(rng)
        dq = np.full((ny, nx), 0xFFFFFFFF, np.uint32)
        dq[nb:-nb, nb:-nb] = refs.random_dq(rng, (ny - 2 * nb, nx - 2 * nb))
        slope, er, ep = (rng.standard_normal((ny, nx)).astype(np.float32) * s for s in (50, 3, 2))
        ins = [_t(a) for a in (slope, er, ep, dq)]
        image = torch.full((ny, nx), 7.0, dtype=torch.float32, device=DEV)
        err = torch.full((ny, nx), 7.0, dtype=torch.float32, device=DEV)
        good = torch.full((ny, nx), 7, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize(DEV)
        ctx.check(ctx.lib.rip_stats_l2_pack(ctx.h, *(t.data_ptr() for t in ins), ny, nx, nb, table.ctypes.data, image.data_ptr(),
                                            err.data_ptr(), good.data_ptr()))
        ctx.synchronize()
        act = (slice(nb, ny - nb), slice(nb, nx - nb))
        want_good = np.zeros((ny, nx), np.uint8)
        want_good[act] = ~post.build_mask(dq[act], refs.table_dict(table))
        want_image, want_err = np.zeros((ny, nx), np.float32), np.zeros((ny, nx), np.float32)
        want_image[act] = slope[act]
        want_err[act] = np.sqrt((er * er + ep * ep).astype(np.float32))[act]
        assert_same_bits(good.cpu().numpy(), want_good, f"good, nb = {nb}")
        assert_same_bits(image.cpu().numpy(), want_image, f"image, nb = {nb}")
        assert_same_bits(err.cpu().numpy(), want_err, f"err, nb = {nb}")
        assert 0.3 < want_good[act].mean() < 0.97
    bad = table.copy()
    bad[31] = 3
    with pytest.raises(ValueError):
        ctx.check(ctx.lib.rip_stats_l2_pack(ctx.h, *(t.data_ptr() for t in ins), ny, nx, nb, bad.ctypes.data, image.data_ptr(),
                                            err.data_ptr(), good.data_ptr()))


# =========================================================================================== 2. bin mean
@pytest.mark.parametrize("shape,k", refs.BIN_CASES)
@pytest.mark.parametrize("masked", [False, True])
def test_bin_mean_in_the_documented_order_and_within_the_f64_bound(shape, k, masked):
    arr, mask = refs.bin_inputs(np.random.default_rng(k), shape)
    mask = mask if masked else None
    got = sky.binkxk(arr, k, mask=mask, ctx=gpu_context())
    assert_same_bits(got, refs.bin_mean_same_order(arr, mask, k), f"bin mean {shape} k={k}: f32 row sums in row order")
    mean64, meanabs = refs.bin_mean_f64(arr, mask, k)
    assert np.array_equal(np.isnan(got), np.isnan(mean64))
    ok = ~np.isnan(mean64)
    err = np.abs(got.astype(np.float64) - mean64)[ok]
    print(f"bin mean {shape} k={k}: max |got - mean64| / bound = {np.max(err / refs.bin_bound(meanabs, k)[ok]):.3f}")
    assert np.all(err <= refs.bin_bound(meanabs, k)[ok])


def test_bin_mean_special_values_stay_in_their_block():
    k, shape = 4, (9, 1050)   # 2 x 262 blocks: the second workgroup of a row holds some of the marked ones
    arr, _ = refs.bin_inputs(np.random.default_rng(8), shape)
    mask = np.zeros(shape, bool)
    arr[1, 2] = np.nan                       # block (0, 0)
    mask[7, 1030] = True                     # block (1, 257)
    arr[3, 1043] = np.inf                    # block (0, 260)
    arr[4, 1047], arr[7, 1044] = np.inf, -np.inf   # block (1, 261)
    arr[8, 5] = np.nan                       # remainder row: ignored
    arr[2, 1049] = np.nan                    # remainder column: ignored
    for m in (None, mask):
        got = sky.binkxk(arr, k, mask=m, ctx=gpu_context())
        want_nan = np.zeros((2, 262), bool)
        want_nan[0, 0] = want_nan[1, 261] = True
        want_nan[1, 257] = m is not None
        assert np.array_equal(np.isnan(got), want_nan)
        assert got[0, 260] == np.inf
        assert_same_bits(got, refs.bin_mean_same_order(arr, m, k), "bin mean with special values")


def test_bin_mean_refuses_an_image_smaller_than_a_block():
    with pytest.raises(ValueError):
        sky.binkxk(np.zeros((3, 40), np.float32), 4, ctx=gpu_context())
    with pytest.raises(ValueError):
        sky.binkxk(np.zeros((40, 3), np.float32), 4, ctx=gpu_context())


# =========================================================================================== 3. order statistics
GEOM = dict(y0=3, x0=5, ky=5, kx=7, nby=4, nbx=6)   # on a (41, 67) image: offsets, ky != kx, rows and columns left over
SHAPE = (41, 67)


def _ref_select(a, y0, x0, ky, kx, nby, nbx, ranks):
    """counts and the requested ranks of every block from np.sort of its non-NaN values (NaN where out of range)"""
    ranks = np.asarray(ranks, np.int64).reshape(nby * nbx, -1)
    counts = np.zeros(nby * nbx, np.int64)
    vals = np.full(ranks.shape, np.nan, np.float32)
    for by in range(nby):
        for bx in range(nbx):
            blk = a[y0 + by * ky:y0 + (by + 1) * ky, x0 + bx * kx:x0 + (bx + 1) * kx].ravel()
            v = np.sort(blk[~np.isnan(blk)])
            b = by * nbx + bx
            counts[b] = v.size
            for i, r in enumerate(ranks[b]):
                if 0 <= r < v.size:
                    vals[b, i] = v[r]
    return counts, vals


def _check_select(a, geom, ranks, what):
    counts, vals = sky._select(gpu_context(), a, geom["y0"], geom["x0"], geom["ky"], geom["kx"], geom["nby"], geom["nbx"], ranks)
    want_counts, want_vals = _ref_select(a, ranks=ranks, **geom)
    assert np.array_equal(counts, want_counts), f"{what}: counts"
    assert_same_bits(vals, want_vals, what, zero_sign_ok=True)
    # counts alone (nranks = 0)
    only, none = sky._select(gpu_context(), a, geom["y0"], geom["x0"], geom["ky"], geom["kx"], geom["nby"], geom["nbx"], None)
    assert none is None and np.array_equal(only, want_counts), f"{what}: counts without ranks"
    return want_counts, want_vals


def _block_ranks(a, geom):
    """every rank 0..34 of every 5 x 7 block, then -1, count and count + 5"""
    counts, _ = _ref_select(a, ranks=np.zeros((geom["nby"] * geom["nbx"], 1)), **geom)
    every = np.tile(np.arange(35, dtype=np.int64), (counts.size, 1))
    return np.concatenate([every, np.full((counts.size, 1), -1), counts[:, None], counts[:, None] + 5], axis=1)


def _whole(shape):
    return dict(y0=0, x0=0, ky=shape[0], kx=shape[1], nby=1, nbx=1)


def _whole_ranks(a, rng):
    n = int(np.count_nonzero(~np.isnan(a)))
    fixed = [0, 1, n // 4, n // 2 - 1, n // 2, n - 2, n - 1, -1, n, n + 5]
    return np.array(fixed + list(rng.integers(0, max(n, 1), size=30)), dtype=np.int64)[None, :]


def test_every_rank_of_small_offset_blocks():
    rng = np.random.default_rng(31)
    a = rng.standard_normal(SHAPE).astype(np.float32)
    a[rng.random(SHAPE) < 0.1] = np.nan
    a[3:8, 5:12] = rng.standard_normal((5, 7)).astype(np.float32)   # one block without NaN: all 35 ranks in range
    counts, vals = _check_select(a, GEOM, _block_ranks(a, GEOM), "all ranks")
    assert counts[0] == 35 and counts.min() < 33
    assert np.isnan(vals[:, 35:]).all() and not np.isnan(vals[0, :35]).any()


SPECIALS = _f32_bits([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x80000001,
                      0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000, 0x3F800000, 0xBF800000])


def _family(name, rng, n):
    """n float32 values that stress one part of the 11 + 11 + 10 bit radix select"""
    one = 0x3F800000
    low = (one + rng.integers(0, 1000, size=n)).astype(np.uint32)           # differ in the low 10 bits only
    mid = (one | (rng.integers(0, 2048, size=n) << 10)).astype(np.uint32)   # differ in bits 10..20 only
    if name == "low10":
        return _f32_bits(low)
    if name == "mid11":
        return _f32_bits(mid)
    if name == "neg_low10":
        return _f32_bits(low | 0x80000000)
    if name == "neg_mid11":
        return _f32_bits(mid | 0x80000000)
    if name == "both_signs":
        pick = np.where(rng.random(n) < 0.5, low, mid)
        return _f32_bits(pick | (rng.integers(0, 2, size=n).astype(np.uint32) << 31))
    if name == "specials":
        return rng.permutation(np.resize(SPECIALS, n))
    if name == "all_equal":
        return np.full(n, -3.25, np.float32)
    if name == "two_values":
        return rng.permutation(np.resize(np.array([2.5, -1.0], np.float32), n))
    if name == "nan_payloads":
        v = rng.standard_normal(n).astype(np.float32).view(np.uint32)
        nan = rng.random(n) < 0.3
        v[nan] = rng.choice(np.array([0x7FC00000, 0xFFC00001, 0x7F800001, 0xFFFFFFFF], np.uint32), size=int(nan.sum()))
        return v.view(np.float32)
    if name == "only_nan":
        return _f32_bits(rng.choice(np.array([0x7FC00000, 0xFFC00001, 0x7F800001], np.uint32), size=n))
    raise KeyError(name)


FAMILIES = ["low10", "mid11", "neg_low10", "neg_mid11", "both_signs", "specials", "all_equal", "two_values", "nan_payloads",
            "only_nan"]


@pytest.mark.parametrize("family", FAMILIES)
def test_select_ranks_on_value_families(family):
    rng = np.random.default_rng(FAMILIES.index(family))
    a = np.ascontiguousarray(_family(family, rng, SHAPE[0] * SHAPE[1]).reshape(SHAPE))
    counts, vals = _check_select(a, GEOM, _block_ranks(a, GEOM), f"{family}, blocks")
    wcounts, wvals = _check_select(a, _whole(SHAPE), _whole_ranks(a, rng), f"{family}, whole image")
    if family == "only_nan":
        assert not counts.any() and not wcounts.any() and np.isnan(vals).all() and np.isnan(wvals).all()
    elif family == "nan_payloads":
        assert 0.6 * a.size < wcounts[0] < 0.8 * a.size
    else:
        assert (counts == 35).all() and wcounts[0] == a.size


@functools.lru_cache(maxsize=None)
def _big():
    """One (2100, 2048) block: 4.3 M elements, more than 1024 chunks of 4096 -- the grid-stride path of the histogram kernel and
    the block cap of the Gaussian sums.  Made once; nothing writes to it."""
    rng = np.random.default_rng(2100)
    a = rng.standard_normal((2100, 2048), dtype=np.float32)
    a[rng.random(a.shape) < 0.1] = np.nan
    a.setflags(write=False)
    v = np.sort(a[~np.isnan(a)])
    v.setflags(write=False)
    return a, v


def test_select_ranks_beyond_the_chunk_cap():
    a, v = _big()
    assert a.size > 1024 * 4096
    n = v.size
    ranks = np.array([[0, n // 4, n // 2, n - 1, n]], dtype=np.int64)
    counts, vals = sky._select(gpu_context(), a, 0, 0, a.shape[0], a.shape[1], 1, 1, ranks)
    assert counts[0] == n
    assert_same_bits(vals[0], np.array([v[0], v[n // 4], v[n // 2], v[n - 1], NAN32]), "ranks of 4.3 M elements")
    got = sky.nanpercentiles(a, (0.1, 50.0), ctx=gpu_context())
    for q, g in zip((0.1, 50.0), got):
        assert_same_bits(np.float32(g), np.float32(np.nanpercentile(a, q)), f"nanpercentile {q} of 4.3 M elements")


QS = (0, 0.1, 25, 50, 62.5, 99.9, 100)


def _percentile_inputs():
    rng = np.random.default_rng(17)
    ties = (np.round(rng.standard_normal((30, 41)) * 2) / 2).astype(np.float32)
    ties[rng.random(ties.shape) < 0.2] = np.nan
    line = rng.standard_normal(1001).astype(np.float32)
    line[::7] = np.nan
    ends = rng.standard_normal((25, 40)).astype(np.float32)
    ends[3, 3], ends[20, 7], ends[11, 11] = np.inf, -np.inf, np.nan
    two = np.array([[np.nan, 2.0, np.nan, -7.5]], np.float32)
    finite = SPECIALS[np.isfinite(SPECIALS)]
    return {
        "n=1": (np.array([[3.5]], np.float32), QS),
        "n=1 among NaN": (np.array([[np.nan], [-0.25], [np.nan]], np.float32), QS),
        "n=2": (two, QS),
        "all NaN": (np.full((3, 5), np.nan, np.float32), QS),
        "1-D": (line, QS),
        "ties": (ties, QS),
        "special values": (np.random.default_rng(4).permutation(np.resize(finite, 300)).reshape(12, 25), QS),
        "infinite ends, interior q": (ends, (0.1, 25, 50, 62.5, 99.9)),
        "infinite ends, every q": (ends, QS),
    }


@pytest.mark.parametrize("name", list(_percentile_inputs()))
def test_nanpercentiles_bit_identical_to_numpy(name):
    a, qs = _percentile_inputs()[name]
    got = _quiet(sky.nanpercentiles, a, qs, ctx=gpu_context())   # inf - inf in numpy's own interpolation warns on both sides
    assert len(got) == len(qs)
    for q, g in zip(qs, got):
        want = _quiet(np.nanpercentile, a, q)
        assert_same_bits(np.float32(g), np.float32(want), f"{name}: nanpercentile {q}", zero_sign_ok=True)
    if name == "infinite ends, interior q":
        assert np.isfinite(np.array(got[1:4], np.float32)).all()


@pytest.mark.parametrize("N", [1, 3, 8])
def test_block_nanmedians_with_offsets_and_remainders(N):
    rng = np.random.default_rng(70 + N)
    a = rng.standard_normal((70, 333)).astype(np.float32)
    a[rng.random(a.shape) < 0.2] = np.nan
    ny, nx = a.shape
    ky, kx, py, px = ny // N, nx // N, (ny % N) // 2, (nx % N) // 2
    if N > 1:
        a[py + ky:py + 2 * ky, px + 2 * kx:px + 3 * kx] = np.nan   # block (1, 2) is empty
        a[py:py + ky, px:px + kx] = 1.0   # block (0, 0) full: an even count for N = 8 (328), an odd one for N = 3 (2553)
        a[py, px] = -2.0
    inner = a[py:py + N * ky, px:px + N * kx].reshape(N, ky, N, kx)
    want = _quiet(np.nanmedian, inner, axis=(1, 3)).astype(np.float32)
    cnt = np.count_nonzero(~np.isnan(inner), axis=(1, 3))
    if N > 1:
        assert np.isnan(want[1, 2]) and (cnt % 2 == 0).any() and (cnt % 2 == 1).any()
    got = sky.block_nanmedians(a, N, ctx=gpu_context())
    assert_same_bits(got, want, f"block nan-medians, N = {N}")


def test_select_ranks_refuses_more_blocks_than_a_launch_can_index():
    """257 x 257 one-pixel blocks: one more than grid.y holds.  Before the check, the counting launch failed unnoticed, every
    count read 0 and the medians came back all NaN."""
    a = np.ones((257, 257), np.float32)
    with pytest.raises(ValueError, match="65535"):
        sky.block_nanmedians(a, 257, ctx=gpu_context())
    # nothing was launched: the context is fit for use afterwards
    got = sky.block_nanmedians(np.arange(30 * 257, dtype=np.float32).reshape(30, 257), 30, ctx=gpu_context())
    assert got.shape == (30, 30) and got[0, 0] == 11.5 and got[29, 29] == 7696.5


# =========================================================================================== 4. smoothed histogram, smooth_mode
def _gauss(arr, z, scale):
    ctx = gpu_context()
    arr = np.ascontiguousarray(arr, np.float32)
    z = np.ascontiguousarray(z, np.float64)
    out = np.full(max(z.size, 1), -1.0, np.float64)
    ctx.check(ctx.lib.rip_stage_gauss_hist(ctx.h, arr.ctypes.data, arr.size, z.ctypes.data, z.size, float(scale), out.ctypes.data))
    return out[:z.size]


def _gauss_ref(arr, z, scale):
    x = arr.astype(np.float64).ravel()
    x = x[~np.isnan(x)]
    return np.array([math.fsum(np.exp(-0.5 * ((zi - x) / scale) ** 2).tolist()) for zi in z])


def _gauss_check(arr, z, scale, what):
    """Every term is positive, so n roundings of the running sum and a few ulp between two exp implementations bound the
    relative error by (n + 16) 2^-53 (terms that underflow in one exp and not in the other are far below that)."""
    got, want = _gauss(arr, z, scale), _gauss_ref(arr, z, scale)
    rtol = (arr.size + 16) * 2.0 ** -53
    pos = want > 0
    units = np.abs(got - want)[pos] / want[pos] / 2.0 ** -53 if pos.any() else np.zeros(1)
    print(f"gauss_hist {what}: max relative error {units.max():.2f} x 2^-53 (allowed {arr.size + 16})")
    assert np.all(np.abs(got - want) <= rtol * want), f"{what}: {got} vs {want}"
    return want


def _zs(nz):
    inside = {1: [0.3], 19: list(np.linspace(-3, 3, 17)), 32: list(np.linspace(-4.1, 4.3, 28))}[nz]
    return np.array(inside + [25.0, -60.0, -25.5, 60.0][:nz - len(inside)], np.float64)


@pytest.mark.parametrize("n", [1, 255, 2049])
@pytest.mark.parametrize("nz", [1, 19, 32])
def test_gauss_hist_against_fsum(n, nz):
    """Measured on an MI355X: at most 2.0 x 2^-53 relative to the fsum reference over these nine cases (n = 1, one term and no
    sum: 1.9 x 2^-53, the device exp against numpy's), 13.8 x 2^-53 for the 4.3 M-element array below -- the device exp needs
    no more than the 16 x 2^-53 of headroom."""
    rng = np.random.default_rng(n * 100 + nz)
    arr = np.array([0.25], np.float32) if n == 1 else rng.standard_normal(n).astype(np.float32)
    if n > 1:
        arr[rng.random(n) < 0.1] = np.nan
        arr[5], arr[n - 2], arr[n // 2] = np.inf, -np.inf, 0.25   # infinite values add nothing
    z = _zs(nz)
    want = _gauss_check(arr, z, 0.7, f"n={n} nz={nz}")
    assert want[0] > 0
    if nz > 1:
        assert 0 < want[-2] < 1e-100 and want[-1] == 0   # far outside the data: tiny, and underflowed to exactly 0


def test_gauss_hist_beyond_the_block_cap():
    a, _ = _big()
    assert a.size > 2048 * 256 * 8
    _gauss_check(a, np.array([0.1, -4.5, 30.0]), 0.35, "n=4.3M nz=3")


def test_gauss_hist_refusals():
    arr = np.zeros(10, np.float32)
    with pytest.raises(ValueError):
        _gauss(arr, np.zeros(0), 1.0)
    with pytest.raises(ValueError):
        _gauss(arr, np.zeros(33), 1.0)
    with pytest.raises(ValueError):
        _gauss(arr, np.zeros(3), 0.0)
    with pytest.raises(ValueError):
        _gauss(arr, np.zeros(3), float("nan"))
    assert _gauss(arr, np.zeros(32), 1.0).tolist() == [10.0] * 32


def _bimodal(rng, shape=(60, 80)):
    a = np.where(rng.random(shape) < 0.6, rng.normal(10.0, 1.0, shape), rng.normal(14.0, 0.5, shape)).astype(np.float32)
    a[rng.random(shape) < 0.05] = np.nan
    return a


def test_smooth_mode_with_other_parameters_on_a_bimodal_image():
    a = _bimodal(np.random.default_rng(44))
    for kw in (dict(pc=20.0, pksmooth=0.3, niter=5), dict(pc=35.0, pksmooth=0.8, niter=1), {}):
        got = sky.smooth_mode(a, ctx=gpu_context(), **kw)
        want = post.smooth_mode(a, **kw)
        np.testing.assert_allclose(got, want, rtol=1e-9)
    assert 9 < want[0] < 15


def test_smooth_mode_on_degenerate_images_follows_the_reference():
    """sigma = 0 or NaN: the reference's densities are all 0, it returns a NaN mode and calibrateimage goes on with
    medsky = nan; the mirror used to die on rip_stage_gauss_hist's refusal of the scale."""
    const = np.full((12, 20), 3.25, np.float32)
    holes = const.copy()
    holes[::3, ::2] = np.nan
    nans = np.full((12, 20), np.nan, np.float32)
    for img, width in ((const, 0.0), (holes, 0.0), (nans, np.nan)):
        got = sky.smooth_mode(img, ctx=gpu_context())
        want = _quiet(post.smooth_mode, img)
        assert np.isnan(got[0]) and np.isnan(want[0])
        assert_same_bits(np.float64(got[1]), np.float64(want[1]), "width")
        assert_same_bits(np.float64(got[1]), np.float64(width), "width")
    # niter = 0 never looks at the densities: the median comes back
    assert sky.smooth_mode(const, niter=0, ctx=gpu_context()) == post.smooth_mode(const, niter=0) == (3.25, 0.0)


# =========================================================================================== 5. Legendre model, medfit
def _legendre_tables(order, n):
    return np.ascontiguousarray(np.stack([np.reshape(legendre_p(i, np.linspace(-1, 1 - 2 / n, n)), n) for i in range(order + 1)]),
                                dtype=np.float64)


def _legendre2d(arr, ny, nx, order, LPX, LPY, coef, subtract, model):
    ctx = gpu_context()
    ctx.check(ctx.lib.rip_stage_legendre2d(ctx.h, None if arr is None else arr.ctypes.data, ny, nx, order, LPX.ctypes.data,
                                           LPY.ctypes.data, coef.ctypes.data, int(subtract),
                                           None if model is None else model.ctypes.data))


@pytest.mark.parametrize("shape", [(1, 1), (1, 257), (7, 255), (33, 600)])
@pytest.mark.parametrize("order", range(9))
def test_legendre2d_every_order_and_form(order, shape):
    ny, nx = shape
    rng = np.random.default_rng(order * 1000 + nx)
    LPX, LPY = _legendre_tables(order, nx), _legendre_tables(order, ny)
    nc = (order + 1) * (order + 2) // 2
    coef = np.ascontiguousarray(rng.standard_normal(nc) * 10.0 ** rng.integers(-3, 3, size=nc))
    m64 = np.zeros(shape)
    k = 0
    for i in range(order + 1):        # oracle.post.medfit's accumulation: one product, one sum per term, in the order k
        for j in range(order + 1 - i):
            m64 += coef[k] * np.outer(LPY[j], LPX[i])
            k += 1
    assert k == nc
    want = m64.astype(np.float32)
    arr = (rng.standard_normal(shape) * 20).astype(np.float32)
    flat = arr.reshape(-1)
    for at, v in ((3, np.nan), (300, np.inf), (1500, -np.inf), (0, None), (256, None), (arr.size - 1, None)):
        flat[at % arr.size] = want.reshape(-1)[at % arr.size] if v is None else v   # None: equal to the model, result +-0
    with np.errstate(invalid="ignore"):
        want_sub = arr - want

    model = np.full(shape, 7.0, np.float32)
    _legendre2d(None, ny, nx, order, LPX, LPY, coef, 0, model)
    assert_same_bits(model, want, f"order {order} {shape}: model alone")

    work, model = arr.copy(), np.full(shape, 7.0, np.float32)
    _legendre2d(work, ny, nx, order, LPX, LPY, coef, 1, model)
    assert_same_bits(model, want, f"order {order} {shape}: model with subtraction")
    assert_same_bits(work, want_sub, f"order {order} {shape}: arr - model", zero_sign_ok=True)

    work = arr.copy()
    _legendre2d(work, ny, nx, order, LPX, LPY, coef, 1, None)
    assert_same_bits(work, want_sub, f"order {order} {shape}: arr - model, no model out", zero_sign_ok=True)
    assert work.reshape(-1)[arr.size - 1] == 0


def test_legendre2d_refusals():
    LP, coef = _legendre_tables(9, 4), np.zeros(55)
    arr, model = np.zeros((4, 4), np.float32), np.zeros((4, 4), np.float32)
    with pytest.raises(ValueError):
        _legendre2d(arr, 4, 4, 9, LP, LP, coef, 1, model)
    with pytest.raises(ValueError):
        _legendre2d(None, 4, 4, 2, LP, LP, coef, 1, model)
    with pytest.raises(ValueError):
        _legendre2d(arr, 4, 4, 2, LP, LP, coef, 0, None)
    with pytest.raises(ValueError):
        _legendre2d(arr, 4, 4, -1, LP, LP, coef, 1, model)


def _medfit_image():
    rng = np.random.default_rng(333)
    y, x = np.mgrid[0:70, 0:333]
    a = (5 + 0.01 * x - 0.02 * y + 1e-4 * x * y / 10 + rng.standard_normal((70, 333))).astype(np.float32)
    a[rng.random(a.shape) < 0.1] = np.nan
    a[23:46, 111:222] = np.nan   # the middle block of the 3 x 3 grid is empty
    return a


@pytest.mark.parametrize("order", [0, 4])
def test_medfit_on_a_coarse_grid_with_an_empty_block(order):
    a = _medfit_image()
    coef, model = sky.medfit(a, N=3, order=order, ctx=gpu_context())
    want_coef, want_model = _quiet(post.medfit, a, N=3, order=order)
    assert_same_bits(np.asarray(coef, np.float64), np.asarray(want_coef, np.float64), f"medfit coefficients, order {order}")
    assert_same_bits(model, want_model, f"medfit model, order {order}")
    work = a.copy()
    sky.medfit(work, N=3, order=order, subtract=True, ctx=gpu_context())
    assert_same_bits(work, a - want_model, "arr - model", zero_sign_ok=True)


# =========================================================================================== 6. endslice
def _rdq(rng, G, ny, nx):
    """group dq with every saturation history: the flag never set, set from group 0 on, rising once, clearing and rising again
    (per-pixel probability of the bit 0, 0.1, 0.5, 1), under other bits that toggle at random"""
    p = rng.choice([0.0, 0.1, 0.5, 1.0], size=(ny, nx))
    sat = rng.random((G, ny, nx)) < p
    other = rng.integers(0, 256, size=(G, ny, nx)).astype(np.uint8) & np.uint8(0xFD)
    return np.ascontiguousarray(other | (sat.astype(np.uint8) << 1))


@pytest.mark.parametrize("G", [1, 2, 8, 127])
@pytest.mark.parametrize("nb", [0, 1, 4])
def test_endslice_every_border_and_group_count(nb, G):
    rng = np.random.default_rng(G * 10 + nb)
    ny, nx = 3 + 2 * nb, 522 + 2 * nb   # 522 active columns: three workgroups a row, the last one partly idle
    rdq = _rdq(rng, G, ny, nx)
    if G >= 8:   # hand-made histories in the first active row
        col = rdq[:, nb, nb:nb + 5]
        col &= np.uint8(0xFD)
        col[:, 0] |= 2                                  # saturated from group 0 on: no rising edge
        col[2:4, 1] |= 2
        col[6:, 1] |= 2                                 # rises at 2, clears at 4, rises again at 6
        col[G - 1, 2] |= 2                              # rises in the last group
        col[0, 3] |= 2
        col[3, 3] |= 2                                  # set in group 0, cleared, set again in group 3 only
        col[:, 4] = np.arange(G, dtype=np.uint8) * 5 & 0xFD   # other bits toggle, never the saturation bit
    want = refs.endslice_loop(rdq, nb)
    got = sky.endslice(rdq, nb, ctx=gpu_context())
    assert got.shape == (3, 522)
    assert_same_bits(got, want, f"endslice G={G} nb={nb}")
    assert_same_bits(post.endslice(rdq, nb), want, "the restatement")
    if G >= 8:
        assert got[0, :5].tolist() == [-1, 5, G - 2, 2, -1]
    if G == 1:
        assert (got == -1).all()


def test_endslice_refuses_128_groups():
    with pytest.raises(ValueError):
        sky.endslice(np.zeros((128, 3, 3), np.uint8), 0, ctx=gpu_context())
    ctx = gpu_context()
    rdq, out = np.zeros((128, 3, 3), np.uint8), np.zeros((3, 3), np.int8)
    with pytest.raises(ValueError, match="too many groups"):
        ctx.check(ctx.lib.rip_stage_endslice(ctx.h, rdq.ctypes.data, 128, 3, 3, 0, out.ctypes.data))
    with pytest.raises(ValueError):
        sky.endslice(np.zeros((4, 8, 8), np.uint8), 4, ctx=gpu_context())   # nothing left inside the border


# =========================================================================================== 7. host arrays and device pointers
def test_device_pointers_give_the_bits_of_host_arrays():
    """The header's promise for this section, on which the noise-layer loop rests (planes that stay in HBM)."""
    ctx = gpu_context()
    a = _medfit_image()
    a[23:46, 111:222] = np.random.default_rng(1).standard_normal((23, 111)).astype(np.float32) + 5
    mask = np.random.default_rng(2).random(a.shape) < 0.01
    for k in (1, 3):
        assert_same_bits(sky.binkxk(_dev(a), k, mask=mask, ctx=ctx), sky.binkxk(a, k, mask=mask, ctx=ctx), f"binkxk {k}")
        assert_same_bits(sky.binkxk(_dev(a), k, ctx=ctx), sky.binkxk(a, k, ctx=ctx), f"binkxk {k}, no mask")
    got, want = sky.nanpercentiles(_dev(a), QS, ctx=ctx), sky.nanpercentiles(a, QS, ctx=ctx)
    assert_same_bits(np.array(got, np.float32), np.array(want, np.float32), "nanpercentiles")
    assert_same_bits(np.array(want, np.float32), np.array([np.nanpercentile(a, q) for q in QS], np.float32), "against numpy")
    flat = np.ascontiguousarray(a.reshape(-1))
    assert_same_bits(np.array(sky.nanpercentiles(_dev(flat), QS, ctx=ctx), np.float32), np.array(want, np.float32), "1-D")
    got, want = sky.smooth_mode(_dev(a), pc=30.0, ctx=ctx), sky.smooth_mode(a, pc=30.0, ctx=ctx)
    assert_same_bits(np.array(got, np.float64), np.array(want, np.float64), "smooth_mode")
    np.testing.assert_allclose(want, post.smooth_mode(a, pc=30.0), rtol=1e-9)
    for N in (3, 8):
        assert_same_bits(sky.block_nanmedians(_dev(a), N, ctx=ctx), sky.block_nanmedians(a, N, ctx=ctx), f"block medians {N}")
    for order in (0, 2, 4):
        host = a.copy()
        coef_h, _ = sky.medfit(host, N=4, order=order, subtract=True, ctx=ctx)
        dev = _dev(a)
        coef_d, none = sky.medfit(dev, N=4, order=order, subtract=True, want_model=False, ctx=ctx)
        assert none is None
        assert_same_bits(np.asarray(coef_d), np.asarray(coef_h), f"medfit coefficients, order {order}")
        assert_same_bits(dev.numpy(), host, f"arr - model in HBM, order {order}")
        _, want_model = _quiet(post.medfit, a, N=4, order=order)
        assert_same_bits(host, a - want_model, "arr - model", zero_sign_ok=True)
