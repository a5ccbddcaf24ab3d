"""``tests/pearson_ref.py`` on its own (no GPU): the numpy restatement of ``pearson.hip``'s deviates must be a correct sampler of
the laws it claims before the device is held to it draw by draw (``test_gpu_pearson_deviates.py``).  Uniforms, the
Kolmogorov-Smirnov distance of 200 000 restated deviates to the analytic law of every row of the case table, the source of the
complex loggamma, the classification against the reference's goldens (types 3 and 5 among them), and the two conditions of the
replay: at most 0.1 % of the draws left out, and a recipe noise E_ref with 8 E_ref <= 1e-10."""

import mpmath
import numpy as np
import pytest
from conftest import load_golden
from scipy import special

import pearson_ref as pr
from philox_ref import MASK, block

GOLDENS = (load_golden("pearson_params"), load_golden("pearson_edges"))
KS_BOUND = 2.2     # asymptotic false-alarm rate 2 exp(-2 * 2.2^2) = 1.2e-4 a case; seeds are fixed


def golden_cases():
    return [(g, k[3:-6]) for g in GOLDENS for k in g if k.endswith("_types")]


def test_uniforms():
    elem = np.arange(4133)
    u = np.stack([pr.uniforms(pr.SEED, elem, pr.STREAMS[0], k) for k in range(16)])
    assert u.dtype == np.float64 and np.all(u > 0.0) and np.all(u < 1.0)
    assert all(np.unique(u[:, e]).size == 16 for e in range(0, 4133, 97)), "a uniform repeated within an element"
    assert np.unique(u).size == u.size
    # the layout, once by hand: block k // 2 of {element, stream * 0x9E3779B1, block, 'Pear'}, words (3, 2) then (1, 0)
    for e, k in ((5, 0), (5, 1), (4132, 6), (4132, 7)):
        w = [int(x) for x in block(pr.SEED, e, (pr.STREAMS[0] * 0x9E3779B1) & MASK, k // 2, 0x50656172)]
        hi, lo = (w[3], w[2]) if k % 2 == 0 else (w[1], w[0])
        assert u[k, e] == ((((hi << 32) | lo) >> 12) + 0.5) / 2.0**52
    # elements beyond 2^32 move the second word
    big = pr.uniforms(pr.SEED, np.array([5 + (1 << 32)], dtype=np.uint64), pr.STREAMS[0], 0)
    assert big[0] != u[0, 5]
    for stream in (pr.STREAMS[1], 8):
        assert not np.any(pr.uniforms(pr.SEED, elem, stream, 0) == u[0])
    for seed in (pr.SEED ^ 1, pr.SEED ^ (1 << 32)):
        assert not np.any(pr.uniforms(seed, elem, pr.STREAMS[0], 0) == u[0])


def test_normals_and_gammas_consume_their_own_uniforms():
    """a gamma of shape < 1 takes the boost uniform, then (u1, u2, u) per attempt; what it returns is made of the uniforms it
    reports, and the next sampler of the element starts where it stopped"""
    n = 4133
    rs = pr.Stream(pr.SEED, np.arange(n), 3)
    k = np.where(np.arange(n) % 2 == 0, 0.4, 2.5)
    val, sure, acc = pr.gamma(rs, k)
    assert np.all(np.isfinite(val)) and np.all(val > 0.0) and sure.mean() > 0.999
    assert np.array_equal(acc[0][k < 1.0], pr.uniforms(pr.SEED, np.arange(n)[k < 1.0], 3, 0))
    again = pr.gamma_value(pr.F64, k, acc[0], acc[1], acc[2])[0]
    assert np.array_equal(again, val)
    # three uniforms an attempt (two where 1 + c x <= 0), one more in front for the boost
    assert (rs.k - (k < 1.0)).min() == 3 and np.median(rs.k - (k < 1.0)) == 3
    nxt = rs.next(np.arange(n))
    assert np.array_equal(nxt, pr.uniforms(pr.SEED, np.arange(n), 3, rs.k - 1))


@pytest.mark.parametrize("row", pr.ROWS, ids=pr.row_id)
def test_the_recipe_samples_the_law_it_claims(row):
    name, I = row
    t = pr.moment_ratios(GOLDENS, name)
    d = pr.draw(*t, np.full(pr.N_LAW, I), pr.SEED, 11, detail=True)
    assert np.all(d.types == pr.ROW_TYPES[pr.ROWS.index(row)]) and np.all(np.isfinite(d.x))
    cdf = pr.analytic_cdf(d.types[0], d.par[0], d.sgn)
    ks = pr.ks_sqrt_n(d.x, cdf, pr.rounding_width(d.types[0], d.par[0], np.abs(d.x).max()))
    print("%s: sqrt(n) D = %.3f" % (pr.row_id(row), ks))
    assert ks < KS_BOUND


def test_pearson4_acceptance_is_a_quarter():
    """standard form: the hat has four times the area of the density for every parameter set"""
    for name, I in (("heavy_tail", 40.0), ("symmetric", 0.01), ("heavy_tail", 1e5)):
        _t, par = pr.classify(*pr.moment_ratios(GOLDENS, name), [I])
        rs = pr.Stream(pr.SEED, np.arange(20000), 2)
        pr.pearson4_std(rs, np.full(20000, par[0, 0]), np.full(20000, par[0, 1]))
        # attempts = first uniforms; every attempt inside (-pi/2, pi/2) takes a second one, so uniforms <= 2 attempts
        assert 20000 / rs.k.sum() * 2 >= 0.25 - 0.01 and 20000 / rs.k.sum() <= 0.25 + 0.01


def test_loggamma_source_is_good_enough():
    """scipy's complex loggamma, the independent value of Re lgamma(m + i nu / 2), against mpmath at 40 digits at every
    (m, nu) of the table: within 8 ulp of its value (of 1 below 1) -- 2e-15 at m = 2.5, 7e-9 at m = 4.8e5, where the
    restatement switches to mpmath itself"""
    seen = 0
    for name, I in pr.ROWS:
        types, par = pr.classify(*pr.moment_ratios(GOLDENS, name), [I])
        if types[0] != 4:
            continue
        m, nu = par[0, :2]
        got = special.loggamma(complex(m, 0.5 * nu)).real
        with mpmath.workdps(40):
            err = float(abs(mpmath.mpf(got) - mpmath.loggamma(mpmath.mpc(m, 0.5 * nu)).real))
        print("m %.6g nu %.6g: %.17g, off by %.3g" % (m, nu, got, err))
        assert err <= 8.0 * np.spacing(max(abs(got), 1.0))
        assert abs(pr.F64.re_lgamma_complex(m, 0.5 * nu) - got) <= 8.0 * np.spacing(max(abs(got), 1.0))
        seen += 1
    assert seen == 5


@pytest.mark.parametrize("g,name", golden_cases(), ids=[n for _g, n in golden_cases()])
def test_classification_restates_the_reference(g, name):
    """types equal, parameters to the bit (the same numpy operations in the same order); type 0 where the reference raises"""
    I = g[f"cl_{name}_I"] if f"cl_{name}_I" in g else g["cl_I"]
    types, par = pr.classify(*g[f"cl_{name}_t"], I)
    np.testing.assert_array_equal(types, g[f"cl_{name}_types"])
    np.testing.assert_array_equal(par, g[f"cl_{name}_params"])
    if f"cl_{name}_raises" in g:
        assert np.all(types[g[f"cl_{name}_raises"]] == 0)


def test_types_3_and_5_are_reached():
    e = GOLDENS[1]
    for name in ("gamma", "gamma_neg"):
        types, par = pr.classify(*e[f"cl_{name}_t"], e[f"cl_{name}_I"])
        assert np.all(types == 3)
        assert par[:, 0].min() < 1.0 < par[:, 0].max() and np.all(par[:, 3] == (1.0 if name == "gamma" else -1.0))
    for name, sign in (("inv_gamma", 1.0), ("inv_gamma_neg", -1.0), ("inv_gamma_b", 1.0)):
        types, par = pr.classify(*e[f"cl_{name}_t"], e[f"cl_{name}_I"])
        assert types[0] == 5 and par[0, 3] == sign and set(types.tolist()) >= {0, 4, 5}
    # b1 = 5, b2 = 15 = rhs2: p = 8, so a = 7, b = sigma (p - 2) sqrt(p - 3) = 30, mu = 5
    np.testing.assert_allclose(pr.classify(*e["cl_inv_gamma_t"], e["cl_inv_gamma_I"])[1][0], [7.0, 30.0, 5.0, 1.0], rtol=1e-15)
    assert (4.0 + 2.25) ** 1.5 == 15.625 and (4.0 + 5.0) ** 1.5 == 27.0


@pytest.mark.parametrize("g,name", golden_cases(), ids=[n for _g, n in golden_cases()])
def test_restated_deviates_are_finite_everywhere(g, name):
    """every intensity of every golden case, 0.01 (the clip) and 1e7, 64 draws each: finite, and exactly 0 where the type is 0"""
    I = g[f"cl_{name}_I"] if f"cl_{name}_I" in g else g["cl_I"]
    I = np.repeat(np.concatenate([I, [0.01, 1e7]]), 64)
    t = pr.moment_ratios(GOLDENS, name)
    x, _sure = pr.draw(*t, I, pr.SEED, 5)
    types, _par = pr.classify(*t, I)
    assert np.all(np.isfinite(x)) and np.all(x[types == 0] == 0.0)


@pytest.mark.parametrize("row", pr.ROWS, ids=pr.row_id)
def test_replay_conditions(row):
    """the replay's own inputs: share left out <= 0.1 %, 8 E_ref <= 1e-10 (every row, the large-m one included: its E_ref
    counts an f64 evaluation of log k)"""
    for stream in pr.STREAMS:
        d = pr.replay_case(row, stream)
        left = np.count_nonzero(~d.sure)
        print("%s stream %#x: %d of %d left out, E_ref %.3g" % (pr.row_id(row), stream, left, d.x.size, d.e_ref))
        assert left <= pr.SHARE_LEFT_OUT * d.x.size
        assert np.all(np.isfinite(d.x)) and np.all(d.scale > 0.0)
        assert 0.0 < 8.0 * d.e_ref <= pr.TOL_CAP
    assert 8.0 * d.e_ref <= pr.tolerance(row) <= pr.TOL_CAP
