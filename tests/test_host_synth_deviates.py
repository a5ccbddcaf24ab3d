"""The numpy restatement of the Level-1 deviates (``synth_deviates_ref.py``) on its own, without a GPU: its samplers have the
distributions they claim, the share of draws it pins is what the GPU tests rely on, and every listed extreme-bin seed is one."""

import numpy as np
import pytest
from scipy import stats

import synth_deviates_cases as cases
import synth_deviates_ref as ref

PINNED_MIN, UNSURE_MAX = 0.999, 0.001   # the GPU tests assert the same two shares from the same reference


def _chi2_ok(k, pmf_of, lo, hi):
    """histogram of the integers k against n * pmf on lo .. hi with both tails pooled; a range of more than 400 values in 40
    cells of about equal probability"""
    k = np.asarray(k, dtype=np.float64).ravel()
    if hi - lo > 400:
        edges = np.unique(pmf_of.dist.ppf(np.linspace(0.0, 1.0, 41)[1:-1]))          # cell j: edges[j-1] < k <= edges[j]
        cdf = np.concatenate([[0.0], pmf_of.dist.cdf(edges), [1.0]])
        obs = np.bincount(np.searchsorted(edges, k, side="left"), minlength=len(edges) + 1).astype(np.float64)
        exp = k.size * np.diff(cdf)
    else:
        ks = np.arange(lo, hi + 1)
        obs = np.concatenate([[np.sum(k < lo)], [np.sum(k == q) for q in ks], [np.sum(k > hi)]]).astype(np.float64)
        p = pmf_of(ks)
        exp = k.size * np.concatenate([[max(pmf_of.below(lo), 0.0)], p, [max(1.0 - pmf_of.below(lo) - p.sum(), 0.0)]])
    keep = exp > 0
    assert np.all(obs[~keep] == 0)
    chi2 = np.sum((obs[keep] - exp[keep]) ** 2 / exp[keep])
    limit = stats.chi2.ppf(1 - 1e-6, keep.sum() - 1)
    print("chi2 %.1f (limit %.1f, %d cells, %d draws)" % (chi2, limit, keep.sum(), k.size))
    return chi2 < limit


class _Pmf:
    def __init__(self, dist):
        self.dist = dist

    def __call__(self, ks):
        return self.dist.pmf(ks)

    def below(self, lo):
        return float(self.dist.cdf(lo - 1))


def test_poisson_ppf_is_scipys_quantile():
    rng = np.random.default_rng(3)
    for lam in (0.05, 0.3, 4.7, 9.99):
        q = np.concatenate([rng.random(2000), [0.0, 2.0 ** -24, 1 - 2.0 ** -24, ref.U_TOP], stats.poisson.cdf(np.arange(12), lam)])
        q = q[q < 1.0]
        want = np.maximum(stats.poisson.ppf(q, lam), 0.0)
        assert np.array_equal(ref.poisson_ppf(q, lam), want), lam


@pytest.mark.parametrize("mean", [0.3, 4.7, 9.5])
def test_small_mean_reference_is_poisson_and_pinned(mean):
    """the centre of the interval, ppf(u) on the 23-bit uniforms of a 4096-pixel, 9-read frame, is a Poisson sample"""
    c, t = ref.per_read(mean, 9)
    f = ref.PoissonFrame(np.full(4096, c), t, 77)
    assert f.small.all()
    k = ref.poisson_ppf(f.u, f.lam)
    assert np.all((f.lo <= k) & (k <= f.hi)) and np.all(f.hi - f.lo <= 1)
    d = stats.poisson(float(f.lam[0, 0]))
    assert _chi2_ok(k, _Pmf(d), int(d.ppf(1e-4)), int(d.ppf(1 - 1e-4)))


@pytest.mark.parametrize("mean", cases.SMALL_MEANS)
def test_small_mean_cases_pin_nearly_every_draw(mean):
    """every case on at least 5000 draws: a share of 99.9 % cannot be told from 100 % on fewer"""
    for nreads in cases.SMALL_NREADS:
        c, t = ref.per_read(mean, nreads)
        f = ref.PoissonFrame(np.full(max(1000, -(-5000 // nreads)), c), t, 1000 + nreads)
        assert f.small.all(), (mean, nreads, f.lam.max())
        share = f.pinned.mean()
        print("mean %g, %d reads, %d draws: pinned share %.5f" % (mean, nreads, f.pinned.size, share))
        assert f.pinned.size >= 5000 and share >= PINNED_MIN


@pytest.mark.parametrize("mean", [10.5, 20.0, 900.0])
def test_rejection_reference_is_poisson_and_sure(mean):
    c, t = ref.per_read(mean, 9)
    f = ref.PoissonFrame(np.full(4096, c), t, 78)
    assert not f.small.any() and np.all(f.lo == f.hi)
    d = stats.poisson(float(f.lam[0, 0]))
    assert _chi2_ok(f.lo, _Pmf(d), int(d.ppf(1e-4)), int(d.ppf(1 - 1e-4)))


@pytest.mark.parametrize("mean", cases.BIG_MEANS + (2.0e9 / 9, 3.0e9 / 9))
def test_rejection_cases_are_sure_nearly_everywhere(mean):
    c, t = ref.per_read(mean, 9)
    f = ref.PoissonFrame(np.full(1000, c), t, 79)
    assert not f.small.any()
    unsure = 1.0 - f.sure.mean()
    print("mean %g: unsure share %.5f" % (mean, unsure))
    assert unsure <= UNSURE_MAX
    assert abs(f.lo.mean() / f.lam[0, 0] - 1.0) < 6.0 / np.sqrt(f.lam[0, 0] * f.lo.size)


@pytest.mark.parametrize("n,p", [(300, 0.01), (300, 0.03), (300, 0.04), (60000, 0.3), (300, 0.97), (60000, 0.99999), (2000000000, 0.4)])
def test_binomial_reference_is_binomial_and_sure(n, p):
    """n q = 3, 9, 12, 18000 below one half; 9, 0.6 and 8e8 through the flip"""
    pix = np.arange(30000)
    k, sure = ref.binomial(n, p, 80, pix, 3, ref.TAG_SHARE)
    unsure = 1.0 - sure.mean()
    print("n %d p %g: unsure share %.5f" % (n, p, unsure))
    assert unsure <= UNSURE_MAX
    d = stats.binom(n, p)
    assert np.all((k >= 0) & (k <= n))
    assert _chi2_ok(k, _Pmf(d), int(d.ppf(1e-4)), int(d.ppf(1 - 1e-4)))


def test_binomial_frame_ends_at_the_total_and_is_sure():
    counts = np.repeat(np.array(cases.BINOMIAL_TOTALS, dtype=np.float32), 500)
    out, sure = ref.apportion_binomial(counts, cases.BINOMIAL_T_READS, 81)
    assert np.array_equal(out[-1], counts.astype(np.int64)) and np.all(out[0] == 0) and np.all(np.diff(out, axis=0) >= 0)
    assert 1.0 - sure.mean() <= UNSURE_MAX
    p = ref.share_table(cases.BINOMIAL_T_READS)["p"]
    assert p.min() == 0.0 and p.max() == 1.0 and np.any((p > 0) & (p < 0.5)) and np.any((p > 0.5) & (p < 1))
    nq = counts[None, :] * np.minimum(p, 1 - p)[:, None]
    assert np.any((nq > 0) & (nq < 10)) and np.any(nq > 10)


@pytest.mark.parametrize("mu", [0.7, 9.5, 10.5, 2000.0])
def test_poisson_any_reference_is_poisson(mu):
    k, sure = ref.poisson_any(np.full(30000, mu), 82, np.arange(30000), 0, ref.TAG_CR_COUNT)
    assert 1.0 - sure.mean() <= UNSURE_MAX
    d = stats.poisson(mu)
    assert _chi2_ok(k, _Pmf(d), int(d.ppf(1e-4)), int(d.ppf(1 - 1e-4)))


def test_normals_and_track_uniforms():
    z = ref.read_normals(83, 4, 20000)
    assert z.shape == (4, 20000) and abs(z.mean()) < 5 / np.sqrt(z.size) and abs(z.var() - 1) < 0.03
    assert stats.kstest(z.ravel(), "norm").pvalue > 1e-6
    assert np.array_equal(ref.reset_normals(83, 50), ref.normal(83, np.arange(50), 0, ref.TAG_RESET))
    assert not np.array_equal(ref.fill_normals(83, 4, 50)[:4], z[:, :50])     # another tag: other deviates
    assert ref.fill_normals(83, 4, 50).shape == (5, 50) and ref.white33_normals(83, 4, 50).shape == (4, 50)
    u = ref.track_uniforms(84, 20000)
    assert u.shape == (20000, 5) and u.min() > 0 and u.max() < 1
    for q in range(5):
        assert stats.kstest(u[:, q], "uniform").pvalue > 1e-6
    assert np.max(np.abs(np.corrcoef(u.T) - np.eye(5))) < 6 / np.sqrt(20000)


def test_unequal_spacing_case_has_what_it_claims():
    tab = ref.share_table(np.cumsum(cases.UNEQUAL_GAPS))
    w, eff = tab["w"], tab["eff"]
    assert eff[2] == 1 and w[2] != w[1] and abs(w[2] - w[1]) < 1e-12 * w[1]          # the table of read 1 serves read 2
    assert w[4] == 0.0 and 0 < 4 < len(w) - 1 and np.all(np.delete(eff, 2) == np.delete(np.arange(len(w)), 2))
    assert len(set(np.round(w, 6))) >= 6
    lam = np.array(cases.UNEQUAL_COUNTS)[:, None] * w[None, :]
    top = lam.max(axis=1)
    assert np.any(top < 4) and np.any((top >= 4) & (top < 10)) and np.any(top >= 10)
    crossing = [(row[:-1] < 10) & (row[1:] >= 10) for row in lam], [(row[:-1] >= 10) & (row[1:] < 10) for row in lam]
    assert any(c.any() for c in crossing[0]) and any(c.any() for c in crossing[1])
    straddle = (top >= 4) & (top < 10) & (np.sum(lam < 4, axis=1) > lam.shape[1] // 2)
    assert straddle.any()


def test_listed_extreme_bins_are_extreme():
    seen_words, seen_values = set(), set()
    for seed, npix, nreads, pixel, read, value in cases.EXTREME_BINS:
        bits = ref.small_bits(seed, np.arange(npix), nreads)
        assert int(bits[read, pixel]) == value, (seed, pixel, read)
        assert value in (0x7FFFFF, 0x7FFFFE, 0x7FFFFD, 0)
        seen_words.add(read & 3)
        seen_values.add(value)
        u = ref.small_uniform(value)
        assert 0.0 < u < 1.0 and float(np.float32(u)) == u
    assert seen_words == {0, 1, 2, 3} and seen_values == {0x7FFFFF, 0x7FFFFE, 0x7FFFFD, 0}
    assert any(read >= (nreads // 4) * 4 and nreads % 4 for _, _, nreads, _, read, _ in cases.EXTREME_BINS)
    means = np.array(cases.EXTREME_MEANS)
    assert len(means) >= 128 and means.min() > 0.05 and means.max() < 9.99
    # the interval of a top bin ends at the finest tail a 32-bit word can justify, that of bin 0 is the single value 0
    lo, hi = ref.small_interval(np.full(len(means), ref.small_uniform(0x7FFFFF)), means)
    assert np.array_equal(hi, np.maximum(stats.poisson.ppf(ref.U_TOP, means), 0)) and np.all(lo <= hi)
    assert np.array_equal(lo, stats.poisson.ppf(1 - 2.0 ** -24 - ref.M_SMALL, means))
    lo0, hi0 = ref.small_interval(np.full(len(means), ref.small_uniform(0)), means)
    assert np.all(lo0 == 0) and np.all(hi0 == 0)
