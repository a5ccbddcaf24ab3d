"""Cosmic-ray hits on the device (``csrc/cr.hip``; the model is restated in DESIGN.md section 7) against the numpy reference
``cr_ref.py``: everything deterministic exactly, everything random as a distribution, then through ``L1Synth``, the
calibration chain and the many-realisations harness."""

import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: both bring a HIP runtime)
from conftest import assert_same_bits, gpu_context, l1sim_golden_cal, load_golden

import cr_ref
from romanimpreprocess_amd import pipeline, synth
from romanimpreprocess_amd.dqflags import pixel
from romanimpreprocess_amd.from_sim import cr, sim_to_isim

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
JUMP = np.uint32(pixel.JUMP_DET)


# ---- the two entries on plain arrays -------------------------------------------------------------------------------------------
def _tracks(par, nreads, read_time, nya, nxa, seed, counts, uniforms, capacity):
    """rip_synth_cr_tracks -> (tracks (capacity, 6), offsets (nreads+1,)) numpy; rows never written stay NaN"""
    ctx = gpu_context()
    t = torch.full((max(capacity, 1), 6), float("nan"), dtype=torch.float64, device=DEV)
    o = torch.full((nreads + 1,), -1, dtype=torch.int32, device=DEV)
    c = None if counts is None else torch.from_numpy(np.asarray(counts, dtype=np.int32)).to(DEV)
    u = None if uniforms is None else torch.from_numpy(np.ascontiguousarray(uniforms, dtype=np.float64)).to(DEV)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rip_synth_cr_tracks(ctx.h, C.byref(par), nreads, read_time, nya, nxa, seed, None if c is None else c.data_ptr(),
                                          None if u is None else u.data_ptr(), capacity, t.data_ptr(), o.data_ptr()))
    ctx.synchronize()
    return t.cpu().numpy(), o.cpu().numpy()


def _deposit(par, nreads, nya, nxa, tracks, poisson, seed, base=None, want_lam=False):
    """rip_synth_cr_deposit on rows sorted by read -> (reads_e, first_read, lam or None) numpy"""
    ctx = gpu_context()
    t = np.asarray(tracks, dtype=np.float64).reshape(-1, 6)
    t = t[np.argsort(t[:, 0], kind="stable")]
    offsets = np.searchsorted(t[:, 0], np.arange(nreads + 1), side="left").astype(np.int32)
    d_t = torch.from_numpy(np.concatenate([t, np.zeros((1, 6))])).to(DEV)
    d_o = torch.from_numpy(offsets).to(DEV)
    e = torch.from_numpy(np.zeros((nreads, nya, nxa), np.int32) if base is None else np.ascontiguousarray(base, dtype=np.int32)).to(DEV)
    first = torch.full((nya, nxa), -7, dtype=torch.int32, device=DEV)
    lam = torch.full((nya, nxa), float("nan"), dtype=torch.float64, device=DEV) if want_lam else None
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rip_synth_cr_deposit(ctx.h, C.byref(par), nreads, nya, nxa, d_t.data_ptr(), d_o.data_ptr(), int(poisson), seed,
                                           e.data_ptr(), first.data_ptr(), None if lam is None else lam.data_ptr()))
    ctx.synchronize()
    return e.cpu().numpy(), first.cpu().numpy(), None if lam is None else lam.cpu().numpy()


def _ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def test_tracks_from_handed_in_uniforms():
    nya, nxa, nreads, cap = 24, 40, 6, 32
    counts = [3, 0, 1, 7, 2, 5]
    rng = np.random.default_rng(11)
    u = rng.random((cap, 5))
    u[0] = [0.0, 0.0, 0.0, 0.0, 0.0]                                  # the lower ends of every range
    u[1] = [1 - 2.0 ** -53, 1 - 2.0 ** -53, 0.5, 1 - 2.0 ** -53, 1 - 2.0 ** -53]   # and the flat tails of both tables
    u[2, 3:] = [0.999999, 1e-9]
    par = cr.params_from({})
    t, off = _tracks(par, nreads, 3.04, nya, nxa, 1, counts, u, cap)
    assert off.tolist() == [0, 3, 3, 4, 11, 13, 18]
    n = off[-1]
    assert np.all(np.isnan(t[n:])) and np.all(np.isfinite(t[:n]))
    want_read = np.repeat(np.arange(nreads), counts).astype(np.float64)
    i0, j0, phi, length, dedx = cr_ref.sample(u[:n], nya, nxa)
    assert_same_bits(t[:n, 0], want_read, "read index")
    assert_same_bits(t[:n, 1], i0, "i0")
    assert_same_bits(t[:n, 2], j0, "j0")
    assert_same_bits(t[:n, 3], phi, "phi")
    print("ulps: length", _ulps(t[:n, 4], length).max(), "dEdx", _ulps(t[:n, 5], dedx).max())
    assert _ulps(t[:n, 4], length).max() <= 4 and _ulps(t[:n, 5], dedx).max() <= 4
    assert t[0, 4] == 10.0 and t[0, 5] == 10.0 and t[1, 4] <= 2000.0 and t[1, 5] <= 10000.0
    # other tables (the context's copy follows the parameters), a count that does not fit the capacity
    other = {"max_cr_len": 500.0, "slope": -2.0, "location": 300.0, "grid_size": 257}
    t2, off2 = _tracks(cr.params_from(other), nreads, 3.04, nya, nxa, 1, [4, 4, 4, 4, 4, 4], u, 10)
    assert off2.tolist() == [0, 4, 8, 10, 10, 10, 10]
    _, _, _, length2, dedx2 = cr_ref.sample(u[:10], nya, nxa, cr_ref.params(**other))
    assert _ulps(t2[:10, 4], length2).max() <= 4 and _ulps(t2[:10, 5], dedx2).max() <= 4 and np.all(t2[:10, 4] <= 500.0)
    assert t2[:10, 0].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2]
    t3, _ = _tracks(par, nreads, 3.04, nya, nxa, 1, counts, u, cap)   # and back to the first tables
    assert_same_bits(t3, t, "tracks after a change of tables and back")


def test_bad_arguments_are_refused_before_any_launch():
    par = cr.params_from({})
    with pytest.raises(ValueError):
        _tracks(par, 6, 3.04, 24, 40, 1, None, None, 0)
    with pytest.raises(ValueError):
        _tracks(par, 6, 3.04, 0, 40, 1, None, None, 8)
    with pytest.raises(ValueError):
        _tracks(cr.params_from({"grid_size": 1}), 6, 3.04, 24, 40, 1, None, None, 8)
    with pytest.raises(ValueError):
        _tracks(cr.params_from({"conversion_factor": 0.0}), 6, 3.04, 24, 40, 1, None, None, 8)
    one = np.array([[0, 1.0, 1.0, 0.0, 10.0, 100.0]])
    with pytest.raises(ValueError):
        _deposit(cr.params_from({"conversion_factor": -1.0}), 6, 24, 40, one, 0, 1)
    with pytest.raises(ValueError):
        _deposit(par, 0, 24, 40, one, 0, 1)


def test_deposit_of_the_rounded_means_matches_the_reference():
    nya, nxa, nreads = 24, 40, 6
    tracks = cr_ref.deposit_case_tracks(nya, nxa, nreads)
    ref = cr_ref.deposit(tracks, nreads, nya, nxa)
    rng = np.random.default_rng(2)
    base = np.cumsum(rng.integers(0, 50, size=(nreads, nya, nxa)), axis=0).astype(np.int32)
    e, first, lam = _deposit(cr.params_from({}), nreads, nya, nxa, tracks, 0, 9, base=base, want_lam=True)
    print("lam: largest difference", np.abs(lam - ref["lam"]).max(), "of", ref["lam"].max(), "; cpp_max", ref["cpp_max"])
    np.testing.assert_allclose(lam, ref["lam"], rtol=1e-10, atol=1e-9 * ref["cpp_max"])
    assert np.array_equal(first, ref["first_read"])
    inc = e.astype(np.int64) - base
    sure = ref["unsure"] == 0
    assert np.array_equal(inc[sure], ref["added"][sure])
    assert np.all(np.abs(inc - ref["added"]) <= ref["unsure"])
    assert ref["unsure"][-1].sum() <= 0.01 * ref["hits"]
    before = np.arange(nreads)[:, None, None] < ref["first_read"][None]
    assert np.array_equal(e[before], base[before])                    # reads before the hit, and pixels never hit
    assert np.all(np.diff(e.astype(np.int64), axis=0) >= 0)
    # the closed forms, straight from the device (pixels that no other track of the list crosses)
    checked = 0
    for k, (name, _, parts) in enumerate(cr_ref.closed_form_cases(nya, nxa)):
        cpp = tracks[k, 5] * 20.0
        for i, j, l2 in parts:
            want = cpp * np.sqrt(0.25 + l2 * l2)
            if abs(ref["lam"][i, j] - want) < 1e-9 * cpp:
                checked += 1
                assert abs(lam[i, j] - want) < 1e-9 * cpp, (name, i, j)
                assert inc[k % 4 + 1:, i, j].min() == inc[-1, i, j] == int(np.rint(want)) and first[i, j] == 1 + k % 4, (name, i, j)
    assert checked >= 15
    # without lam and without a base: the same electrons
    e0, first0, none = _deposit(cr.params_from({}), nreads, nya, nxa, tracks, 0, 10)
    assert none is None and np.array_equal(e0, inc) and np.array_equal(first0, first)


LAMBDAS = (0.5, 2.0, 5.0, 9.5, 10.5, 15.0, 30.0, 100.0, 1000.0, 1.0e4, 2.0e5)


def test_deposit_draws_poisson_deviates():
    """2000 equal tracks per mean on isolated (pixel, read) slots; each track stays inside its pixel with length 0, so its mean
    is dEdx * 20 * 0.5 electrons.  The mean is held to 5 sqrt(lambda / n) at n = 2000 per seed.  The variance bands are those
    of ``test_gpu_synth.py`` for the same generators (0.06 for the sequential search below 10, 0.02 for the transformed
    rejection); a variance estimated from 2000 deviates scatters by sqrt(2 / 2000) = 0.032 itself, wider than the band, so
    the bands are applied to the pool of 64 seeds (n = 128 000: 0.004), each of which is a 2000-track case of its own
    (measured: pool 0.9963 .. 1.0028 over the eleven means; the first seed alone 0.9735 .. 1.0533)."""
    nya, nxa, nreads, per = 64, 96, 8, 2000
    nseeds = 64
    npix = nya * nxa
    slot = np.arange(len(LAMBDAS) * per)
    which = slot // per
    rd, pix = slot // npix, slot % npix                               # 6144 slots per read
    assert rd.max() < nreads
    tracks = np.stack([rd, pix // nxa, pix % nxa, np.zeros(len(slot)), np.zeros(len(slot)), np.array(LAMBDAS)[which] / 10.0], axis=1)
    par = cr.params_from({})

    def draws(seed):
        e, first, _ = _deposit(par, nreads, nya, nxa, tracks, 1, seed)
        assert np.array_equal(first.ravel()[pix[rd == 0]], np.zeros(np.count_nonzero(rd == 0), np.int32))
        inc = np.diff(np.concatenate([np.zeros((1, nya, nxa), np.int64), e.astype(np.int64)]), axis=0)
        return e, inc.reshape(nreads, npix)[rd, pix].reshape(len(LAMBDAS), per)

    first_e, k0 = draws(100)
    again, _ = draws(100)
    other, _ = draws(101)
    assert np.array_equal(first_e, again) and not np.array_equal(first_e, other)
    pool = [k0] + [draws(100 + s)[1] for s in range(1, nseeds)]
    for s, k in enumerate(pool):
        for lam, row in zip(LAMBDAS, k):
            assert abs(row.mean() - lam) < 5 * np.sqrt(lam / per), (s, lam, row.mean())
    k = np.concatenate(pool, axis=1).astype(np.float64)
    n = k.shape[1]
    for lam, row in zip(LAMBDAS, k):
        band = 0.06 if lam < 10 else 0.02
        print(f"lambda {lam}: mean {row.mean():.6g}, variance / lambda {row.var() / lam:.5f} (n = {n}; first seed alone "
              f"{k0[LAMBDAS.index(lam)].var() / lam:.5f})")
        assert abs(row.mean() - lam) < 5 * np.sqrt(lam / n), (lam, row.mean())
        assert abs(row.var() / lam - 1) < band, (lam, row.var() / lam)
        assert np.all(row >= 0)


def test_device_sampler_has_the_distributions_of_the_model():
    from scipy import stats

    nya, nxa, nreads, mu = 64, 96, 8, 2000.0
    par = cr.params_from({"area": mu / (8.0 * 3.04)})
    cap = cr.capacity_for(par, nreads, 3.04)
    assert cap == int(nreads * mu + 10 * np.sqrt(nreads * mu) + 64)
    t, off = _tracks(par, nreads, 3.04, nya, nxa, 77, None, None, cap)
    counts = np.diff(off)
    print("tracks per read", counts.tolist())
    assert off[0] == 0 and np.all(np.abs(counts - mu) < 6 * np.sqrt(mu)) and len(set(counts.tolist())) > 1
    n = int(off[-1])
    assert n < cap and np.all(np.isnan(t[n:]))
    t = t[:n]
    assert np.array_equal(t[:, 0], np.repeat(np.arange(nreads), counts).astype(np.float64))
    assert t[:, 1].min() >= 0 and t[:, 1].max() < nya and t[:, 2].min() >= 0 and t[:, 2].max() < nxa
    cells = np.histogram2d(t[:, 1], t[:, 2], bins=(8, 8), range=((0, nya), (0, nxa)))[0].ravel()
    chi2 = np.sum((cells - n / 64.0) ** 2 / (n / 64.0))
    assert chi2 < stats.chi2.ppf(1 - 1e-6, 63), chi2
    bins = np.histogram(t[:, 3], bins=16, range=(0, 2 * np.pi))[0]
    chi2 = np.sum((bins - n / 16.0) ** 2 / (n / 16.0))
    assert chi2 < stats.chi2.ppf(1 - 1e-6, 15), chi2
    c_len, x_len, c_de, x_de = cr_ref.tables()
    p_len = stats.kstest(t[:, 4], lambda x: np.interp(x, x_len, c_len)).pvalue
    p_de = stats.kstest(t[:, 5], lambda x: np.interp(x, x_de, c_de)).pvalue
    print("kstest p: length", p_len, "dEdx", p_de)
    assert p_len > 1e-6 and p_de > 1e-6
    # the five deviates of a track are independent draws: no correlation between any two columns
    cc = np.corrcoef(t[:, 1:].T)
    assert np.max(np.abs(cc - np.eye(5))) < 6 / np.sqrt(n)
    # another seed: other tracks; the same seed: the same
    t2, off2 = _tracks(par, nreads, 3.04, nya, nxa, 78, None, None, cap)
    t3, off3 = _tracks(par, nreads, 3.04, nya, nxa, 77, None, None, cap)
    assert not np.array_equal(off2, off) and np.array_equal(off3, off) and np.array_equal(t3[:n], t)
    # the romanisim-named functions on numpy arrays
    i, j, phi, length, dedx = cr.sample_cr_params(500, nya, nxa, seed=3, ctx=gpu_context())
    assert all(a.shape == (500,) for a in (i, j, phi, length, dedx)) and i.max() < nya and j.max() < nxa
    assert 10 <= length.min() and length.max() <= 2000 and 10 <= dedx.min() and dedx.max() <= 10000 and 11 < np.median(length) < 14
    img = np.zeros((nya, nxa), dtype=np.float32)
    back = cr.simulate_crs(img, 3.04, area=6.0, seed=5, ctx=gpu_context())
    again = cr.simulate_crs(np.zeros((nya, nxa), dtype=np.float32), 3.04, area=6.0, rng=5, ctx=gpu_context())
    assert back is img and np.array_equal(img, again) and img.min() >= 0 and 100 < np.count_nonzero(img) < img.size // 2
    assert np.all(img == np.round(img)) and np.median(img[img > 0]) > 500


# ---- through L1Synth, the chain and the harness ---------------------------------------------------------------------------------
NY, NX, NB = 32, 512, 4
NYA, NXA = NY - 2 * NB, NX - 2 * NB


@pytest.fixture(scope="module")
def frame():
    rp = synth.READ_PATTERN_8
    cal = synth.make_caldir(NY, NX, read_pattern=rp, p_order=8, seed=13)
    cb = pipeline.Calibrator(ctx=gpu_context())
    s = sim_to_isim.L1Synth(cal, rp, synth.FRAME_TIME, ctx=cb.ctx)
    counts = torch.full((NYA, NXA), 300.0, dtype=torch.float32, device=s.dev)
    torch.cuda.synchronize()
    return rp, cal, cb, s, counts


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _grown(hit):
    """the pixels within one pixel (Chebyshev) of a hit: as far as the inter-pixel capacitance carries it"""
    ny, nx = hit.shape
    near = np.zeros((ny + 2, nx + 2), bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            near[dy:dy + ny, dx:dx + nx] |= hit
    return near[1:-1, 1:-1]


def test_hits_leave_the_rest_of_the_exposure_alone(frame):
    rp, cal, cb, s, counts = frame
    plain = s.make(counts, 41, poisson=True)
    assert s.last_first_read is None
    off = s.make(counts, 41, poisson=True, crparam={"area": 0})
    assert int((s.last_first_read < s.nreads).sum()) == 0
    assert np.array_equal(_u16(off[0]), _u16(plain[0])) and np.array_equal(_u16(off[1]), _u16(plain[1]))
    # the electrons: every plane minus the hit-free one is what the tracks deposit
    crparam = {"area": 0.05}
    e0 = s.apportion(counts, 41, poisson=True)
    s.ctx.synchronize()
    e0 = e0.cpu().numpy()
    e = s.apportion(counts, 41, poisson=True)
    hits = s.cosmic_rays(e, 41, crparam, poisson=False, want_lambda=True)
    s.ctx.synchronize()
    ntr = int(hits["offsets"][-1])
    tracks = hits["tracks"].cpu().numpy()[:ntr]
    assert 10 < ntr < hits["tracks"].shape[0]
    ref = cr_ref.deposit(tracks, s.nreads, NYA, NXA)
    inc = e.cpu().numpy().astype(np.int64) - e0
    assert np.all(np.abs(inc - ref["added"]) <= ref["unsure"])
    assert np.array_equal(hits["first_read"].cpu().numpy(), ref["first_read"])
    np.testing.assert_allclose(hits["lam"].cpu().numpy(), ref["lam"], rtol=1e-10, atol=1e-9 * ref["cpp_max"])
    # the exposure: the same tracks (same seed, same parameters), Poisson deposits; away from them nothing moves
    cube, a33 = s.make(counts, 41, poisson=True, crparam=crparam)
    first = s.last_first_read.cpu().numpy()
    assert np.array_equal(first, ref["first_read"])
    hit = first < s.nreads
    far = np.ones((NY, NX), bool)
    far[NB:-NB, NB:-NB] = ~_grown(hit)
    got, want = _u16(cube), _u16(plain[0])
    assert np.array_equal(got[:, far], want[:, far]) and np.array_equal(_u16(a33), _u16(plain[1]))
    changed = (got != want).any(axis=0)[NB:-NB, NB:-NB]
    assert changed[hit].mean() > 0.9 and 20 < hit.sum() < 0.05 * hit.size


THRESHOLD_E = 400.0


def test_hits_through_the_calibration_chain(frame):
    """40 isolated single-pixel hits of 100 .. 5000 electrons in reads 4 .. 25 of a flat 300-electron exposure, calibrated on the
    device: pixeldq and slope equal the oracle chain's on the same cube bit for bit, and every hit of at least THRESHOLD_E
    electrons on an otherwise unflagged pixel carries JUMP_DET.
    THRESHOLD_E = 400 was found on the CPU beforehand: exposures of this frame, scene and calibration set built with oracle/l1sim
    (numpy deviates, the fill's 1/f noise included) plus cr_ref, 40 hits per level of a ladder of 60 .. 5000 electrons, six
    exposures, calibrated by the oracle chain.  It flagged 224 of 228 hits of 300 electrons and every hit from 400 electrons up
    (229 of 229 at 400; 1372 of 1372 from 500 to 5000): 400 is the smallest level it flagged all of."""
    import oracle

    rp, cal, cb, s, counts = frame
    ladder = (100.0, 160.0, 250.0, 400.0, 600.0, 1000.0, 2000.0, 5000.0)
    rng = np.random.default_rng(8)
    slots = [(i, j) for i in range(2, NYA - 1, 3) for j in range(2, NXA - 1, 3)]
    pick = rng.permutation(len(slots))[:40]
    rows = [(int(rng.integers(4, 26)), slots[q][0] + 0.125, slots[q][1] - 0.25, 1.0, 0.0, ladder[n % len(ladder)] / 10.0)
            for n, q in enumerate(pick)]
    e = s.apportion(counts, 52, poisson=True)
    hits = s.cosmic_rays(e, 52, {}, tracks=np.array(rows), poisson=False)
    cube = s.resultants(e, 52)["cube"]
    a33 = torch.zeros((s.ngrp, NY, s.cw), dtype=torch.int16, device=s.dev)
    torch.cuda.synchronize()
    s.fill(cube, a33, 52)
    s.ctx.synchronize()
    first = hits["first_read"].cpu().numpy()
    assert sorted((r[0], int(r[1] + 0.5), int(r[2] + 0.5)) for r in rows) == sorted(
        (int(first[i, j]), i, j) for i, j in zip(*np.nonzero(first < s.nreads)))
    ramp = {"data": _u16(cube).copy(), "amp33": _u16(a33).copy(), "groupdq": np.zeros(cube.shape, np.uint8),
            "pixeldq": np.array(cal["mask"]["dq"], dtype=np.uint32), "read_pattern": rp, "frame_time": synth.FRAME_TIME}
    ref = oracle.calibrate_arrays(ramp, cal)
    cb.load_caldir(5, cal)
    try:
        got = cb.calibrate(5, ramp)
    finally:
        cb.ctx.drop_caldir(5)
    assert_same_bits(got["pixeldq"], ref["pixeldq"], "pixeldq")
    assert_same_bits(got["slope"], ref["slope"], "slope", zero_sign_ok=True)
    checked = 0
    for r, i0, j0, _, _, dedx in rows:
        y, x = int(i0 + 0.5) + NB, int(j0 + 0.5) + NB
        clean = cal["mask"]["dq"][y, x] == 0 and (ref["pixeldq"][y, x] & ~JUMP) == 0
        if clean and dedx * 10.0 >= THRESHOLD_E:
            checked += 1
            assert got["pixeldq"][y, x] & JUMP, (r, y, x, dedx * 10.0)
    assert checked >= 20


def test_make_l1_fullcal_flags_the_hit_resultants():
    g = load_golden("l1sim")
    cal, rp = l1sim_golden_cal(g)
    caldir = {k: {"roman": v} for k, v in cal.items()}
    rt = float(g["read_time"])
    crparam = {"area": 0.3}
    l1_0, dq_0 = sim_to_isim.make_l1_fullcal(g["counts"], rp, caldir, rng=17, read_time=rt)
    l1_1, dq_1 = sim_to_isim.make_l1_fullcal(g["counts"], rp, caldir, rng=17, read_time=rt, crparam=crparam)
    assert np.array_equal(dq_0, g["dq"]) and np.array_equal(dq_1 & ~JUMP, dq_0) and dq_1.dtype == np.uint32
    # the same tracks once more, by hand: same seed, same parameters
    s = sim_to_isim.L1Synth(cal, rp, rt)
    e = s.apportion(np.asarray(g["counts"], dtype=np.float32), 17)
    first = s.cosmic_rays(e, 17, crparam)["first_read"]
    s.ctx.synchronize()
    first = first.cpu().numpy()
    want = np.zeros(dq_1.shape, bool)
    r = 0
    for j, reads in enumerate(rp):          # (f): the resultant that holds the hit read, and every later one
        r += len(reads)
        want[j:] |= (first < r)[None] & ~want[j:]
    assert np.array_equal((dq_1 & JUMP) != 0, want) and 5 < want[-1].sum() < want[-1].size // 2
    assert (want[-1] & ~want[0]).any()
    far = ~_grown(want[-1])                  # the deviates of the two calls are the same: away from the hits nothing moves
    assert np.array_equal(l1_1[:, far], l1_0[:, far]) and far.any()
    assert np.median((l1_1 - l1_0)[-1][want[-1]]) > 50


def test_harness_with_cosmic_rays():
    from romanimpreprocess_amd.harness import many_realizations as mr

    rp = synth.READ_PATTERN_8
    ny, nx, nseeds = 72, 256, 4
    cal = synth.make_caldir(ny, nx, read_pattern=rp, p_order=8, seed=13)
    cb = pipeline.Calibrator(ctx=gpu_context())
    cb.load_caldir(0, cal)
    kw = dict(nseeds=nseeds, seed0=100, read_pattern=rp, device=DEV, reference_alias=False, generator="hip")
    tm0, tm1, tm2 = {}, {}, {}
    plain = mr.run(cb, 0, cal, timings=tm0, **kw)
    off = mr.run(cb, 0, cal, timings=tm1, crparam={"area": 0}, **kw)
    assert np.array_equal(plain, off) and tm0["cr_hit_pixels"] == 0 and tm1["cr_hit_pixels"] == 0
    hit = mr.run(cb, 0, cal, timings=tm2, crparam={"area": 0.2}, **kw)
    assert tm2["cr_hit_pixels"] > 0
    lost = (hit[3] < plain[3]) & (plain[3] == nseeds)
    print("hit pixels", tm2["cr_hit_pixels"], "; pixels that lost a realisation", int(lost.sum()))
    assert lost.any() and np.all(hit[3][lost] < nseeds)
    for gen in ("host", "device"):
        with pytest.raises(ValueError, match="crparam"):
            mr.run(cb, 0, cal, nseeds=1, seed0=100, read_pattern=rp, device=DEV, generator=gen, crparam={})
