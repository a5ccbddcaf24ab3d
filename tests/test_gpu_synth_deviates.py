"""The deviates that make Level-1 exposures are functions of (seed, counter): every draw of ``rip_synth_apportion`` (Poisson and
binomial), the normals of ``rip_synth_resultants`` / ``rip_synth_fill`` and the uniforms and counts of ``cr.hip`` against the
numpy restatement ``synth_deviates_ref.py`` (DESIGN.md "Shared device headers", rows 6 to 11).  The f64 samplers are pinned draw
by draw wherever the restatement is sure of its decision; the f32 sequential search of the small means must land in the
interval of counts around the f64 quantile (one value for all but the draws next to a cdf step)."""

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: both bring a HIP runtime)
from conftest import assert_same_bits, gpu_context, l1sim_golden_cal, load_golden

import synth_deviates_cases as cases
import synth_deviates_ref as ref
from romanimpreprocess_amd.from_sim import cr, sim_to_isim

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SENTINEL = -77
PINNED_MIN, UNSURE_MAX = 0.999, 0.001   # the shares test_host_synth_deviates.py finds in the reference alone


def _apportion(counts, t_reads, seed, poisson=True):
    """rip_synth_apportion on a (1, npix) frame with its own read times -> (nreads, npix) int32 numpy; the output is pre-filled
    with SENTINEL"""
    ctx = gpu_context()
    counts = np.ascontiguousarray(counts, dtype=np.float32).ravel()
    t = np.ascontiguousarray(t_reads, dtype=np.float64)
    c = torch.from_numpy(counts).to(DEV)
    out = torch.full((len(t), counts.size), SENTINEL, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    ctx.call("rip_synth_apportion", c, 1, counts.size, bool(poisson), len(t), t, seed, out)
    ctx.synchronize()
    return out.cpu().numpy()


def _equal_reads(nreads):
    return np.arange(1, nreads + 1, dtype=np.float64)   # t_reads[0] > 0: read 0 draws too


# ---- Poisson increments, means below 10: the f32 sequential search ----------------------------------------------------------------
@pytest.mark.parametrize("mean", cases.SMALL_MEANS)
def test_small_means_land_in_their_interval(mean):
    """0.05 .. 3.9 electrons per read are drawn by the first launch, 4.0 .. 9.99 by the deferred one (class 0); 1 .. 35 reads
    (whole and partial blocks of four), 1 .. 1000 pixels (less than a wave, one short of and one past a workgroup, four)"""
    draws = pinned = 0
    for nreads in cases.SMALL_NREADS:
        for npix in cases.SMALL_NPIX:
            seed = 0x5EED0000 + 64 * nreads + npix
            counts = np.full(npix, mean * nreads, dtype=np.float32)
            f = ref.PoissonFrame(counts, _equal_reads(nreads), seed)
            assert f.small.all()
            out = _apportion(counts, _equal_reads(nreads), seed)
            n = f.check(out, SENTINEL)
            assert n == f.lo.size
            draws += n
            pinned += int(np.count_nonzero(f.pinned))
            if n >= 5000:   # (99.9 % cannot be told from 100 % on fewer draws)
                assert f.pinned.mean() >= PINNED_MIN
    print("mean %g: %d draws in their interval, %d of them pinned to one value (%.4f %%)" % (mean, draws, pinned, 100.0 * pinned / draws))
    assert pinned >= PINNED_MIN * draws


@pytest.mark.parametrize("entry", cases.EXTREME_BINS, ids=lambda e: "seed%d-%06x" % (e[0], e[5]))
def test_extreme_bins_of_the_uniform(entry):
    """The uniform of a pixel does not depend on its count: the frame of a listed seed once per mean of the grid, the draw at
    the listed (pixel, read) inside its interval each time -- at least ppf(u - m), and for the top bins at most
    ppf(1 - 2^-32).  An f32 running sum that saturates below u = 1 - 2^-24 .. 1 - 5 * 2^-24 must not run on to where the terms
    underflow."""
    seed, npix, nreads, pixel, read, value = entry
    ctx = gpu_context()
    t = _equal_reads(nreads)
    u = float(ref.small_uniform(value))
    means = np.array(cases.EXTREME_MEANS)
    counts = (means * nreads).astype(np.float32)
    lam = counts.astype(np.float64) * ref.share_table(t)["w"][read]
    lo, hi = ref.small_interval(np.full(len(means), u), lam)
    c = torch.empty(npix, dtype=torch.float32, device=DEV)
    out = torch.empty((nreads, npix), dtype=torch.int32, device=DEV)
    got = np.zeros(len(means))
    for j, cj in enumerate(counts):
        c.fill_(float(cj))
        out.fill_(SENTINEL)
        torch.cuda.synchronize()
        ctx.call("rip_synth_apportion", c, 1, npix, True, nreads, t, seed, out)
        ctx.synchronize()
        col = out[:, pixel].cpu().numpy().astype(np.int64)
        assert not np.any(col == SENTINEL)
        got[j] = col[read] - (col[read - 1] if read else 0)
    bad = (got < lo) | (got > hi)
    print("seed %d, pixel %d, read %d, bin %#x: %d of %d means outside; largest draw %g (interval up to %g)"
          % (seed, pixel, read, value, np.count_nonzero(bad), len(means), got.max(), hi.max()))
    assert not bad.any(), [(float(m), float(g), float(a), float(b)) for m, g, a, b in zip(means[bad], got[bad], lo[bad], hi[bad])][:8]


# ---- Poisson increments, means of 10 and more: riprng::poisson_ptrs ---------------------------------------------------------------
@pytest.mark.parametrize("mean", cases.BIG_MEANS)
def test_rejection_branch_is_pinned(mean):
    """10 and 10.5 draw counts on both sides of the k < 16 table of the f32 pre-test, 15 mixes the two, 9e6 is past the
    pre-test's range (f64 test only).  The pre-test has no margin in the reference: the device must equal the f64 decision."""
    for nreads, npix in ((9, 1000), (2, 257)):
        counts = np.full(npix, mean * nreads, dtype=np.float32)
        f = ref.PoissonFrame(counts, _equal_reads(nreads), 0xB16 + nreads)
        assert not f.small.any() and np.all(f.lo == f.hi)
        out = _apportion(counts, _equal_reads(nreads), 0xB16 + nreads)
        n = f.check(out, SENTINEL)
        print("mean %g, %d x %d: %d draws equal the reference, %d left out" % (mean, nreads, npix, n, f.lo.size - n))
        assert n >= (1.0 - UNSURE_MAX) * f.lo.size


def test_rejection_pretest_decides_only_outside_its_error_band():
    """5e6 electrons per read, just inside the range of the f32 pre-test, where its rounding errors are largest (|d| of a few
    thousand: 1e-3 on either side of the comparison): 147 456 draws, of which a pre-test that decided inside its error band
    would get several wrong"""
    nreads, npix, mean = 36, 4096, 5.0e6
    counts = np.full(npix, mean * nreads, dtype=np.float32)
    f = ref.PoissonFrame(counts, _equal_reads(nreads), 0xE95)
    out = _apportion(counts, _equal_reads(nreads), 0xE95)
    n = f.check(out, SENTINEL)
    print("mean %g: %d draws equal the reference, %d left out" % (mean, n, f.lo.size - n))
    assert n >= (1.0 - UNSURE_MAX) * f.lo.size


def test_counts_at_and_beyond_the_clip():
    """2e9 electrons: the running sum saturates at 2e9 exactly as the output does; 3e9 is clipped to 2e9 first: the same frame"""
    t = _equal_reads(9)
    f = ref.PoissonFrame(np.full(1000, 2.0e9, dtype=np.float32), t, 0xC11F)
    assert 1.0 - f.sure.mean() <= UNSURE_MAX
    a = _apportion(np.full(1000, 2.0e9, dtype=np.float32), t, 0xC11F)
    b = _apportion(np.full(1000, 3.0e9, dtype=np.float32), t, 0xC11F)
    f.check(a, SENTINEL)
    assert np.array_equal(a, b)
    assert a.max() == 2000000000 and 100 < np.count_nonzero(a[-1] == 2000000000) < 900 and np.all(np.diff(a.astype(np.int64), axis=0) >= 0)
    whole = np.logical_and.accumulate(f.pinned, axis=0)[-1]
    assert whole.mean() > 0.98 and np.array_equal(a[-1][whole], np.minimum(f.lo.sum(axis=0), 2.0e9)[whole].astype(np.int32))


def test_negative_and_nan_counts_draw_nothing():
    counts = np.array([-5.0, np.nan, -np.inf, -0.0, 0.0, -1e30] * 50, dtype=np.float32)
    for nreads in (1, 9):
        out = _apportion(counts, _equal_reads(nreads), 3)
        assert out.shape == (nreads, counts.size) and not out.any()
    mixed = counts.copy()
    mixed[::7] = 90.0
    f = ref.PoissonFrame(mixed, _equal_reads(9), 4)
    out = _apportion(mixed, _equal_reads(9), 4)
    f.check(out, SENTINEL)
    assert not out[:, mixed != 90.0].any() and out[-1, ::7].min() > 0


# ---- unequal read spacing -------------------------------------------------------------------------------------------------------
def test_unequal_read_spacing():
    """gaps of several sizes, a repeated time and two gaps within 1e-12 of each other; pixels whose mean crosses 10 between reads
    in both directions (a PtrsPlan from an earlier share would be stale; the launch of the bright pixels takes its sequential
    search), and pixels whose largest read lies between 4 and 10 while most of their reads are below 4"""
    t = np.cumsum(cases.UNEQUAL_GAPS)
    counts = np.tile(np.array(cases.UNEQUAL_COUNTS, dtype=np.float32), 455)[:4093]
    f = ref.PoissonFrame(counts, t, 0x0E0A)
    out = _apportion(counts, t, 0x0E0A)
    n = f.check(out, SENTINEL)
    small, big = f.small, f.lam >= 10.0
    print("unequal spacing: %d draws compared (%d by search, %d by rejection), %d left out" % (n, small.sum(), big.sum(), f.lo.size - n))
    assert f.pinned[small].mean() >= PINNED_MIN and f.sure[big].mean() >= 1.0 - UNSURE_MAX
    assert np.all(out[4] == out[3])                                # the repeated time: nothing arrives
    assert np.any(small.any(axis=0) & big.any(axis=0))
    # the same frame with equal counts everywhere: a pixel's draws do not depend on its neighbours'
    for c in (35.0, 20.0):
        alone = _apportion(np.full(counts.size, c, dtype=np.float32), t, 0x0E0A)
        assert np.array_equal(alone[:, counts == c], out[:, counts == c])


# ---- frames that mix the three classes of pixels ----------------------------------------------------------------------------------
# electrons per read: below 4 (first launch), 4 .. 10 (deferred, sequential search), 10 and more (deferred, rejection)
CLASS_MEANS = ((0.3, 3.9), (4.7, 9.5), (15.0, 900.0))
_constant_frames = {}


def _constant_frame(mean, npix, nreads, seed):
    key = (mean, npix, nreads, seed)
    if key not in _constant_frames:
        _constant_frames[key] = _apportion(np.full(npix, mean * nreads, dtype=np.float32), _equal_reads(nreads), seed)
    return _constant_frames[key]


@pytest.mark.parametrize("layout,npix,nreads", [("scattered", 4093, 9), ("runs", 4093, 9), ("no_class_0", 4093, 9), ("no_class_1", 4093, 9),
                                                ("deferred_only", 4093, 9), ("scattered", 70001, 5)])
def test_mixed_frames_draw_the_same_electrons_as_constant_ones(layout, npix, nreads):
    """"the same electrons whichever kernel draws them": every pixel of a frame that mixes the classes -- scattered, in runs,
    with a class absent -- is written exactly once and equals, bit for bit, the same pixel of the frame that holds its count
    everywhere.  70001 pixels are 274 workgroups: several feed each of the 256 lists of deferred pixels."""
    seed = 0x31C5ED
    rng = np.random.default_rng(npix + nreads)
    classes = {"no_class_0": (0, 2), "no_class_1": (0, 1), "deferred_only": (1, 2)}.get(layout, (0, 1, 2))
    means = np.array([m for k in classes for m in CLASS_MEANS[k]])
    if layout == "runs":
        which = (np.arange(npix) // 300 + np.arange(npix) // 1111) % len(means)
    else:
        which = rng.integers(0, len(means), npix)
    counts = (means[which] * nreads).astype(np.float32)
    out = _apportion(counts, _equal_reads(nreads), seed)
    assert not np.any(out == SENTINEL)
    for j, m in enumerate(means):
        sel = which == j
        assert sel.any()
        assert np.array_equal(out[:, sel], _constant_frame(float(m), npix, nreads, seed)[:, sel]), (layout, float(m))
    f = ref.PoissonFrame(counts, _equal_reads(nreads), seed)
    f.check(out, SENTINEL)


# ---- given totals: riprng::binomial -----------------------------------------------------------------------------------------------
def test_binomial_shares_are_pinned():
    """totals of 0 .. 2e9, shares on both sides of one half, n q on both sides of 10 (inversion and BTRS); the last read has the
    total"""
    counts = np.repeat(np.array(cases.BINOMIAL_TOTALS, dtype=np.float32), 171)
    want, sure = ref.apportion_binomial(counts, cases.BINOMIAL_T_READS, 0xB1)
    out = _apportion(counts, cases.BINOMIAL_T_READS, 0xB1, poisson=False)
    assert not np.any(out == SENTINEL)
    assert np.array_equal(out[-1], counts.astype(np.int64)) and not out[0].any()
    differ = np.count_nonzero(out[sure] != want[sure])
    print("binomial: %d of %d values compared, %d differ" % (np.count_nonzero(sure), sure.size, differ))
    assert 1.0 - sure.mean() <= UNSURE_MAX
    assert differ == 0
    assert np.all(np.diff(out.astype(np.int64), axis=0) >= 0)


# ---- riprng::normal_f32 under the tags 0x12 .. 0x15 -------------------------------------------------------------------------------
def _close_dn(got, want, what):
    """the rule of test_injected_normals_are_philox_at_the_documented_counter: the device's f32 logf / cospif are a few ulp off
    the f64 value -- across one rounding boundary and no further, at fewer than 1 % of the samples"""
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print("%s: max |device - handed in| = %g DN, %d of %d differ" % (what, d.max(), np.count_nonzero(d), d.size))
    assert d.max() <= 1.0 and np.count_nonzero(d) < 0.01 * d.size, what


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def test_normals_are_philox_at_their_counters():
    """each entry once with device deviates and once with the reference's normals handed in as f32, on the l1sim fixture's
    calibration set; another seed per entry, so that a swapped tag or index cannot cancel"""
    g = load_golden("l1sim")
    cal, rp = l1sim_golden_cal(g)
    s = sim_to_isim.L1Synth(cal, rp, float(g["read_time"]), channelwidth=16)
    nact, npix, nchan = s.nya * s.nxa, s.ny * s.nx, s.ny * s.cw
    reads_e = torch.from_numpy(g["reads_e"]).to(s.dev)
    torch.cuda.synchronize()
    seed = 0x12131415
    dev = s.resultants(reads_e, seed, want_resultants=True, want_start=True)
    s.ctx.synchronize()
    dev = {k: v.cpu().numpy() for k, v in dev.items()}
    n_reset = ref.reset_normals(seed, nact).astype(np.float32).reshape(s.nya, s.nxa)
    n_read = ref.read_normals(seed, s.ngrp, nact).astype(np.float32).reshape(s.ngrp, s.nya, s.nxa)
    fed = s.resultants(reads_e, seed, normals_reset=n_reset, normals_read=n_read, want_resultants=True, want_start=True)
    s.ctx.synchronize()
    scale = float(np.sqrt(np.mean(fed["start_e"].cpu().numpy().astype(np.float64) ** 2)))
    assert scale > 1.0
    # 1e-5 relative; the absolute term, 1e-5 of the rms, is for the zero crossings of the cosine, where the f32 cospif is a few
    # ulp of 1 (not of its tiny result) off the f64 value: an absolute error of some 1e-7 of the rms on a deviate near zero
    np.testing.assert_allclose(dev["start_e"], fed["start_e"].cpu().numpy(), rtol=1e-5, atol=1e-5 * scale)
    _close_dn(dev["resultants"], fed["resultants"].cpu().numpy(), "resultants")
    _close_dn(dev["cube"].view(np.uint16), _u16(fed["cube"]), "cube")
    base = fed["cube"]
    for banding, seed in ((True, 0x14150001), (False, 0x14150002)):
        cube_d, cube_f = base.clone(), base.clone()
        a33_d = torch.zeros((s.ngrp, s.ny, s.cw), dtype=torch.int16, device=s.dev) if banding else None
        a33_f = torch.zeros((s.ngrp, s.ny, s.cw), dtype=torch.int16, device=s.dev) if banding else None
        torch.cuda.synchronize()
        s.fill(cube_d, a33_d, seed, banding=banding)
        s.ctx.synchronize()
        n_fill = ref.fill_normals(seed, s.ngrp, npix).astype(np.float32).reshape(s.ngrp + 1, s.ny, s.nx)
        w33 = ref.white33_normals(seed, s.ngrp, nchan).astype(np.float32).reshape(s.ngrp, s.ny, s.cw) if banding else None
        s.fill(cube_f, a33_f, seed, banding=banding, normals=n_fill, white33=w33)
        s.ctx.synchronize()
        nb = s.nb
        assert np.array_equal(_u16(cube_d)[:, nb:-nb, nb:-nb], _u16(cube_f)[:, nb:-nb, nb:-nb])   # (no normals in there)
        border = np.ones((s.ny, s.nx), bool)
        border[nb:-nb, nb:-nb] = False
        _close_dn(_u16(cube_d)[:, border], _u16(cube_f)[:, border], "reference pixels, banding %s" % banding)
        _close_dn(_u16(cube_d), _u16(cube_f), "filled cube, banding %s" % banding)
        assert np.std(_u16(cube_f)[:, border].astype(np.float64) - _u16(base)[:, border]) > 3.0   # (the comparison is not of constants)
        if banding:
            _close_dn(_u16(a33_d), _u16(a33_f), "amp33")
            assert _u16(a33_f).astype(np.float64).std() > 1.0


# ---- cr.hip -------------------------------------------------------------------------------------------------------------------------
def _tracks(par, nreads, read_time, nya, nxa, seed, counts, uniforms, capacity):
    ctx = gpu_context()
    t = torch.full((capacity, 6), float("nan"), dtype=torch.float64, device=DEV)
    o = torch.full((nreads + 1,), -1, dtype=torch.int32, device=DEV)
    c = None if counts is None else torch.from_numpy(np.asarray(counts, dtype=np.int32)).to(DEV)
    u = None if uniforms is None else torch.from_numpy(np.ascontiguousarray(uniforms, dtype=np.float64)).to(DEV)
    torch.cuda.synchronize()
    ctx.call("rip_synth_cr_tracks", par, nreads, read_time, nya, nxa, seed, c, u, capacity, t, o)
    ctx.synchronize()
    return t.cpu().numpy(), o.cpu().numpy()


def test_track_uniforms_are_philox_at_their_counter():
    """three blocks {row, 0..2, 0x21, 0x6372746b}, five u53: exact in f64, so the tracks are bit-equal"""
    nya, nxa, nreads, cap, seed = 24, 40, 6, 300, 0xC0537
    counts = [3, 0, 100, 7, 2, 150]
    par = cr.params_from({})
    got, off = _tracks(par, nreads, 3.04, nya, nxa, seed, counts, None, cap)
    want, off2 = _tracks(par, nreads, 3.04, nya, nxa, seed + 1, counts, ref.track_uniforms(seed, cap), cap)
    assert off[-1] == sum(counts) and np.array_equal(off, off2)
    assert_same_bits(got, want, "tracks")
    assert np.all(np.isfinite(got[:off[-1]])) and np.all(np.isnan(got[off[-1]:]))


@pytest.mark.parametrize("mu", [0.7, 9.5, 10.5, 40.0])
def test_track_counts_are_poisson_any(mu):
    """the number of tracks of read r: poisson_any(mu, seed, r, 0, 0x20), the sequential search in f64 below 10 and the
    transformed rejection from 10 on; 1000 reads at once"""
    nreads, read_time, seed = 1000, 3.04, 0xC0 + int(mu * 10)
    par = cr.params_from({"area": mu / (8.0 * read_time)})
    mu_lib = par.flux * par.area * read_time
    cap = int(nreads * mu * 1.5) + 1000
    _, off = _tracks(par, nreads, read_time, 8, 8, seed, None, None, cap)
    k, sure = ref.poisson_any(np.full(nreads, mu_lib), seed, np.arange(nreads), 0, ref.TAG_CR_COUNT)
    got = np.diff(off.astype(np.int64))
    assert off[0] == 0 and off[-1] < cap
    print("mu %g: %d of %d reads compared, %d differ" % (mu, np.count_nonzero(sure), nreads, np.count_nonzero(got[sure] != k[sure])))
    assert 1.0 - sure.mean() <= UNSURE_MAX
    assert np.array_equal(got[sure], k[sure])


def test_deposits_are_poisson_any():
    """a handful of tracks per mean, each inside its own pixel (length 0: the mean is dEdx * 20 * 0.5): deposit 0 of row `row`
    is poisson_any(mean, seed, row, 0, 0x22); the mean itself is read back from the device"""
    nya, nxa, nreads, per, seed = 16, 64, 4, 40, 0xDE9
    lams = (0.5, 5.0, 9.5, 10.5, 15.0, 100.0, 1.0e4)
    ctx = gpu_context()
    par = cr.params_from({})
    slot = np.arange(len(lams) * per)
    rd, pix = slot // 140, slot * 3                       # rows in the order of their reads; every track alone in its pixel
    tracks = np.stack([rd, pix // nxa, pix % nxa, np.zeros(slot.size), np.zeros(slot.size), np.array(lams)[slot // per] / 10.0], axis=1)
    offsets = np.searchsorted(rd, np.arange(nreads + 1), side="left").astype(np.int32)
    d_t = torch.from_numpy(np.concatenate([tracks, np.zeros((1, 6))])).to(DEV)
    d_o = torch.from_numpy(offsets).to(DEV)
    e = torch.zeros((nreads, nya, nxa), dtype=torch.int32, device=DEV)
    first = torch.full((nya, nxa), SENTINEL, dtype=torch.int32, device=DEV)
    lam = torch.full((nya, nxa), float("nan"), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    ctx.call("rip_synth_cr_deposit", par, nreads, nya, nxa, d_t, d_o, True, seed, e, first, lam)
    ctx.synchronize()
    e, lam = e.cpu().numpy().reshape(nreads, -1), lam.cpu().numpy().ravel()
    mean = lam[pix]
    np.testing.assert_allclose(mean, np.array(lams)[slot // per], rtol=1e-12)
    k, sure = ref.poisson_any(mean, seed, slot, 0, ref.TAG_CR_DEPOSIT)
    got = e[rd, pix] - np.where(rd > 0, e[np.maximum(rd - 1, 0), pix], 0)
    print("deposits: %d of %d compared, %d differ" % (np.count_nonzero(sure), slot.size, np.count_nonzero(got[sure] != k[sure])))
    assert np.count_nonzero(~sure) <= UNSURE_MAX * sure.size
    assert np.array_equal(got[sure], k[sure])
    assert np.array_equal(e[-1, pix], got) and np.count_nonzero(e[-1]) == np.count_nonzero(got)



def test_deposits_along_a_track_count_up_the_counter():
    """tracks that cross seven pixels each, alone in their pixels, along +i, -i and +j: deposit j of row `row`, in the order of
    the walk, is poisson_any(mean_j, seed, row, j, 0x22) -- the second counter word counts the deposits of the track.  The ends
    of a track cross a quarter of a pixel, the middle ones a whole pixel: at 9 and 10 electrons per pixel length the means of
    one track lie on both sides of 10 (5.0 / 5.6 at the ends, 10.1 / 11.2 in the middle); 0.9 and 100 stay on one side"""
    nya, nxa, nreads, seed = 32, 96, 2, 0xDE10
    ctx = gpu_context()
    par = cr.params_from({})
    cpps = (9.0, 10.0, 0.9, 100.0)                       # electrons per pixel length = dEdx * 20
    rows = []                                            # (read, i0, j0, phi, walk: the pixels in the order they are crossed)
    for n in range(8):
        j = 2 + 3 * n
        rows.append((n % 2, 4.25, float(j), 0.0, [(i, j) for i in range(4, 11)]))
        j = 40 + 3 * n
        rows.append((n % 2, 25.75, float(j), np.pi, [(i, j) for i in range(26, 19, -1)]))
        i, j0 = 14 + 2 * (n % 2), 3 + 12 * (n // 2)
        rows.append(((n // 2) % 2, float(i), j0 + 0.25, np.pi / 2, [(i, j) for j in range(j0, j0 + 7)]))
    rows.sort(key=lambda r: r[0])                        # the library wants them by read; `row` is the index after that
    tracks = np.array([[r[0], r[1], r[2], r[3], 55.0, cpps[q % 4] / 20.0] for q, r in enumerate(rows)])
    offsets = np.searchsorted(tracks[:, 0], np.arange(nreads + 1), side="left").astype(np.int32)
    d_t = torch.from_numpy(np.concatenate([tracks, np.zeros((1, 6))])).to(DEV)
    d_o = torch.from_numpy(offsets).to(DEV)
    e = torch.zeros((nreads, nya, nxa), dtype=torch.int32, device=DEV)
    first = torch.full((nya, nxa), SENTINEL, dtype=torch.int32, device=DEV)
    lam = torch.full((nya, nxa), float("nan"), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    ctx.call("rip_synth_cr_deposit", par, nreads, nya, nxa, d_t, d_o, True, seed, e, first, lam)
    ctx.synchronize()
    e, lam, first = e.cpu().numpy(), lam.cpu().numpy(), first.cpu().numpy()
    hit = np.zeros((nya, nxa), bool)
    mean, row_of, ndep, got = [], [], [], []
    for row, (rd, _, _, _, walk) in enumerate(rows):
        for j, (y, x) in enumerate(walk):
            assert not hit[y, x]                         # alone in its pixel
            hit[y, x] = True
            mean.append(lam[y, x])
            row_of.append(row)
            ndep.append(j)
            got.append(int(e[rd, y, x]) - (int(e[rd - 1, y, x]) if rd else 0))
    assert np.array_equal(first < nreads, hit) and np.array_equal(lam > 0, hit)      # the walk crossed these pixels and no others
    mean, got = np.array(mean), np.array(got)
    whole = np.array(ndep) % 6 != 0
    cpp = np.array([cpps[r % 4] for r in row_of])
    np.testing.assert_allclose(mean[whole], cpp[whole] * np.sqrt(1.25), rtol=1e-9)
    np.testing.assert_allclose(mean[~whole], cpp[~whole] * np.sqrt(0.3125), rtol=1e-9)
    assert np.any((mean > 4) & (mean < 10)) and np.any((mean >= 10) & (mean < 12))
    k, sure = ref.poisson_any(mean, seed, np.array(row_of), np.array(ndep), ref.TAG_CR_DEPOSIT)
    print("deposits along tracks: %d of %d compared, %d differ" % (np.count_nonzero(sure), got.size, np.count_nonzero(got[sure] != k[sure])))
    assert np.count_nonzero(~sure) <= UNSURE_MAX * sure.size
    assert np.array_equal(got[sure], k[sure])
    # the counter word matters to the reference: with it held at 0 the same means draw other counts
    k0, _ = ref.poisson_any(mean, seed, np.array(row_of), 0, ref.TAG_CR_DEPOSIT)
    assert np.count_nonzero(k0 != k) > got.size // 3
