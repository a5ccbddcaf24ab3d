"""The near-threshold ramps of jump_band_cases.py, held to their conditions with the oracle alone (no GPU): what makes the
comparisons of test_gpu_jump_band.py mean something.

1. Every case the GPU tests use has enough targeted differences with |rel| < 3e-6 (rel = smap / sthresh - 1 as the oracle computes
   it) on the active region, in every regime where the device takes another path: the full-ramp fit, every truncation length,
   slopes below 0 (dvardt clipped to 0), in [0, IthreshA) (no logarithm), above IthreshB; both sides of the threshold evenly; every
   difference index of the full fit.  These are conditions on the generator, not measurements.
2. The set tells a band that is too narrow from a sufficient one: a numpy emulation of the stage kernel's fast path makes wrong
   decisions with guard 0 and none with the production guard 1e-5."""

import numpy as np
import pytest

import jump_band_cases as jb


def _conditions(name, rec, jump_pars, low_slopes=True):
    c = jb.regime_counts(rec, jump_pars)
    print(f"{name}: {c}")
    assert c["full"] >= 1000, f"{name}: {c['full']} near-threshold differences of the full-ramp fit"
    for t, n in c["trunc"].items():
        assert n >= 10, f"{name}: {n} near-threshold differences of the fit truncated to {t} groups"
    for key in ("slope<0", "0<=slope<IA", "slope>IB") if low_slopes else ("slope>IB",):
        assert c[key] >= 50, f"{name}: {c[key]} near-threshold differences with {key}"
    assert 0.4 * c["near"] <= c["hits"] <= 0.6 * c["near"], f"{name}: {c['hits']} hits among {c['near']}"
    for k, n in enumerate(c["full_by_difference"]):
        assert n >= 20, f"{name}: difference {k} of the full fit is near the threshold on {n} pixels"
    return c


def _hits_are_flagged(name, rec, groupdq):
    """the record is the oracle's (the search evaluates pixels apart from their frame): a targeted hit carries JUMP_DET on its group
    in the expected flags"""
    for v in np.unique(rec["variant"][rec["k"] >= 0]):
        for k, (i, _di) in enumerate(jb.rampfit.difference_list(int(v) if v else rec["G"], rec["start"])):
            m = rec["active"] & (rec["variant"] == v) & (rec["k"] == k) & rec["hit"]
            assert np.all(groupdq[i][m] & 4), f"{name}: fit {v}, difference {k}: a hit of the record without its flag"


@pytest.mark.parametrize("name", list(jb.CHAIN_CASES))
def test_generator_conditions(name):
    G, kdt, shape, exclude_first, seed, jump_pars = jb.CHAIN_CASES[name]
    cal, ramp, ref, lines, rec = jb.near_threshold_inputs(G, kdt, shape, exclude_first, seed, jump_pars)
    _conditions(name, rec, jump_pars)
    # the negative block is not the only source of xc == IthreshA
    ia = dict(jb.rampfit.DEFAULT_JUMP_PARS, **(jump_pars or {}))["IthreshA"]
    assert np.count_nonzero(rec["active"] & (rec["k"] >= 0) & (np.abs(rec["rel"]) < jb.NEAR) & (rec["slope"] >= 0) & (rec["slope"] < ia)
                            & (ramp["rate"] > 0)) >= 50
    _hits_are_flagged(name, rec, ref["groupdq"])
    if jump_pars is jb.CROSSING:   # the threshold is <= 0 over part of the slope range, and differences near it are among the targets
        neg = rec["active"] & (rec["k"] >= 0) & (rec["sthresh"] <= 0)
        assert np.count_nonzero(neg & (np.abs(rec["rel"]) < jb.NEAR)) >= 50


@pytest.mark.parametrize("name", list(jb.FIT_CASES))
def test_generator_conditions_of_the_function_level_cases(name):
    """The same conditions.  One exemption, forced by the arithmetic: the case that tunes the GAIN cannot reach a slope <= 0, where
    dvardt = clip(slope / gain, 0) is 0 whatever the gain is, and hardly one in [0, IthreshA), where the Poisson term is too small
    for the gain to move the decision; it is not held to the counts of these two regimes (the oracle's: 0 and 12), and every
    near-threshold difference it has must have a slope above 0."""
    *_inputs, expected, rec = jb.near_threshold_fit_inputs(*jb.FIT_CASES[name])
    _hits_are_flagged(name, rec, expected[3])
    if name.endswith("gain"):
        _conditions(name, rec, None, low_slopes=False)
        near = rec["active"] & (rec["k"] >= 0) & (np.abs(rec["rel"]) < jb.NEAR)
        assert np.all(rec["slope"][near] > 0)
    else:
        _conditions(name, rec, None)


@pytest.mark.parametrize("name", list(jb.STAGE))
def test_set_tells_a_narrow_band_from_a_sufficient_one(name):
    G, kdt, shape, exclude_first, seed, jump_pars = jb.CHAIN_CASES[name]
    cal, ramp, ref, lines, rec = jb.near_threshold_inputs(G, kdt, shape, exclude_first, seed, jump_pars)
    wrong0, exact0 = jb.stage_fast_path_errors(cal, ref, rec, 0.0)
    wrong5, exact5 = jb.stage_fast_path_errors(cal, ref, rec, 1e-5)
    print(f"{name}: guard 0: {wrong0} wrong decisions ({exact0} exact evaluations); guard 1e-5: {wrong5} ({exact5})")
    assert wrong0 >= 10, f"{name}: the emulated fast path without a band makes {wrong0} wrong decisions: the set does not discriminate"
    assert wrong5 == 0, f"{name}: the emulated fast path with the production band makes {wrong5} wrong decisions"
