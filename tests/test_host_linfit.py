"""The numpy restatement of the linearity fit (``linfit_ref.py``) on its own: recovery of a known curve, the two constraints, the
case table's coverage, and the parsing of the drop-in's JSON.  No GPU."""

import copy

import numpy as np
import pytest

import linfit_cases as cases
import linfit_ref as ref

from romanimpreprocess_amd.calfiles import linearity_run

_fits = {}


def recovery(n, p):
    if (n, p) not in _fits:
        sums, counts, first, sref = cases.recovery_sums(n)
        out = ref.fit(sums, counts, first, sref, p_order=p, tframe=cases.TFRAME, nb=0, bright=0, dark=2)
        _fits[(n, p)] = (out, sums, counts, first)
    return _fits[(n, p)]


@pytest.mark.parametrize("p", sorted(cases.RECORDED_ERROR))
def test_recovery(p):
    """max |phi_fit - phi_true| over [smallest used sample, Smax] at n = 4096 against twice the value recorded in
    profiles/linearity_fit.txt (the margin is for libm and numpy versions only)"""
    out, sums, counts, first = recovery(4096, p)
    err = cases.recovery_error(out, sums, counts, first)
    print(f"order {p}: max error {err:.6f} DN_lin, recorded {cases.RECORDED_ERROR[p]}")
    assert out["dq"][0, 0] == 0 and out["cut"][0, 0] == 42 and abs(float(out["Smax"][0, 0]) - 57696.0) < 0.01
    assert err <= 2.0 * cases.RECORDED_ERROR[p]
    # the rates: 420 and 60 DN_lin/s less the dark's 0.3, and the dark itself
    np.testing.assert_allclose(out["pflat"][:, 0, 0], [419.7, 59.7], rtol=2e-6)
    np.testing.assert_allclose(out["dark"][0, 0], 0.3, rtol=1e-5)


@pytest.mark.parametrize("p", [2, 3])
def test_low_orders_cannot_recover(p):
    """a curve with a fifth-order term is out of reach of orders 2 and 3: the measure can tell a bad fit"""
    out, sums, counts, first = recovery(4096, p)
    assert cases.recovery_error(out, sums, counts, first) > 100.0


@pytest.mark.parametrize("p", [1, 2, 3, 5, 8, 10])
def test_constraints(p):
    """phi(Sref) = 0 within one f32 ulp of the largest term of the series; dphi/dS(Sref), evaluated analytically from the stored f32
    coefficients, is 1 within one f32 ulp of c_1 (every coefficient is rounded by half an ulp of its own, c_1's term dominates)"""
    out = recovery(4096, p)[0]
    c, smin, smax = out["data"][:, 0, 0], float(out["Smin"][0, 0]), float(out["Smax"][0, 0])
    h = (smax - smin) / 2.0
    z = np.array((cases.SREF - smin) / h - 1.0)
    P, _ = ref.legendre(z, max(p, 1))
    largest = max(abs(float(c[l]) * float(P[l])) for l in range(p + 1))
    value = float(ref.evaluate(c, smin, smax, cases.SREF))
    slope = float(ref.derivative(c, smin, smax, cases.SREF))
    print(f"order {p}: phi(Sref) = {value:.3e}, slope - 1 = {slope - 1.0:.3e}")
    assert abs(value) <= float(np.spacing(np.float32(largest)))
    assert abs(slope - 1.0) <= float(np.spacing(np.float32(c[1]))) / h


def test_flagged_pixels_carry_the_identity():
    sums, counts, first, sref, dark = cases.fit_inputs(3, 3)
    out = ref.fit(sums, counts, first, sref, p_order=8, nb=cases.NB, bright=0, dark=dark)
    flagged = (out["dq"] != 0) & np.isfinite(sref)
    assert flagged.any() and (out["dq"] == 0).any()
    S = out["Smin"].astype(np.float64) + 0.3 * (out["Smax"].astype(np.float64) - out["Smin"])
    with np.errstate(all="ignore"):
        phi = ref.evaluate(out["data"], out["Smin"], out["Smax"], S)
    ok = flagged & (out["Smax"] > out["Smin"])
    np.testing.assert_allclose(phi[ok], (S - sref)[ok], rtol=0, atol=0.01)
    assert not out["pflat"][:, flagged].any() and not out["ramperr"][:, flagged].any() and not out["dark"][flagged].any()
    assert np.all(out["dq"][:cases.NB] == ref.REFERENCE_PIXEL) and np.all(out["dq"][:, -cases.NB:] == ref.REFERENCE_PIXEL)
    inner = out["dq"][cases.NB:-cases.NB, cases.NB:-cases.NB]
    assert set(np.unique(inner)) <= {0, int(ref.NO_LIN_CORR)}


def test_case_table_covers_every_kind():
    """every kind of pixel the fit has a branch for occurs in the table (counted with the restatement)"""
    total = dict.fromkeys(cases.KINDS, 0)
    for nsets, tstart, p in cases.FIT_CASES:
        sums, counts, first, sref, dark = cases.fit_inputs(nsets, tstart)
        out = ref.fit(sums, counts, first, sref, p_order=p, nb=cases.NB, bright=0, dark=dark)
        for k, n in cases.kinds_of(out, sums, counts, first, sref, dark, p).items():
            total[k] += n
    print(total)
    assert not [k for k, n in total.items() if n == 0]


def test_frame_sums_restatement():
    rng = np.random.default_rng(5)
    cube = rng.integers(0, 65536, size=(5, 12, 80)).astype(np.uint16)
    stored = (cube ^ np.uint16(0x8000)).byteswap()   # FITS storage of the same samples
    a = ref.frame_sums(np.zeros((3, 6, 72), np.uint32), cube, f0=2, rows=(3, 9))
    b = ref.frame_sums(np.zeros((3, 6, 72), np.uint32), stored, f0=2, rows=(3, 9), fits_be16=True)
    assert np.array_equal(a, cube[2:, 3:9, :72]) and np.array_equal(a, b)


# ------------------------------------------------------------------------------------------ the JSON of write_linearity_config.pl
def config():
    ramp = {"FORMAT": 1, "START": 1, "NRAMP": 50, "TSTART": 3}
    return {"SCA": 7, "RAMPS": [dict(ramp, FILE="/d/99999999_SCA07_Flat_001.fits"),
                                dict(ramp, FILE="/d/99999999_SCA07_LoFlat_001.fits", NRAMP=30, START=4),
                                dict(ramp, FILE="/d/99999999_SCA07_Noise_001.fits", NRAMP=30, FORMAT=6)],
            "DARK": -1, "TFRAME": 3.15625, "P_ORDER": 8, "OUTPUT": "/d/roman_wfi_linearitylegendre_X_SCA07.asdf", "SIGN": 1,
            "SLOPECUT": 0.5, "BIAS": {"FILE": "/d/roman_wfi_dark_X_SCA07.asdf", "PATH": ["roman", "data"], "SLICE": 1},
            "NEGATIVEPAD": 500}


def test_config_as_written():
    pars = linearity_run.parse_config(config())
    assert (pars.sca, pars.dark, pars.bright, pars.p_order, pars.tframe, pars.slopecut, pars.negativepad) == (7, 2, 0, 8, 3.15625, 0.5, 500.0)
    assert pars.bias == ("/d/roman_wfi_dark_X_SCA07.asdf", ["roman", "data"], 1)
    assert [r.layout for r in pars.ramps] == ["2026_July", "2026_July", "summer2025"] and [r.tstart for r in pars.ramps] == [3] * 3
    assert pars.ramps[0].files[0] == "/d/99999999_SCA07_Flat_001.fits" and pars.ramps[0].files[-1] == "/d/99999999_SCA07_Flat_050.fits"
    assert len(pars.ramps[0].files) == 50
    assert pars.ramps[1].files[0] == "/d/99999999_SCA07_LoFlat_004.fits" and pars.ramps[1].files[-1] == "/d/99999999_SCA07_LoFlat_033.fits"


def test_dark_index_and_defaults():
    c = config()
    c["DARK"] = 0   # the first set is the dark: the bright one is the next
    pars = linearity_run.parse_config(c)
    assert (pars.dark, pars.bright) == (0, 1)
    c["DARK"] = -3
    assert linearity_run.parse_config(c).dark == 0
    del c["DARK"], c["TFRAME"], c["SIGN"]
    pars = linearity_run.parse_config(c)
    assert (pars.dark, pars.bright, pars.tframe) == (-1, 0, 3.04)


def _set(path, value):
    def change(c):
        node = c
        for k in path[:-1]:
            node = node[k]
        if value is KeyError:
            del node[path[-1]]
        else:
            node[path[-1]] = value
    return change


REFUSALS = [
    ("STOP", _set(("STOP",), 2)), ("'COLOUR'", _set(("COLOUR",), 1)), ("'NSUB'", _set(("RAMPS", 1, "NSUB"), 1)),
    ("'WHERE'", _set(("BIAS", "WHERE"), 1)), ("SIGN", _set(("SIGN",), -1)), ("P_ORDER", _set(("P_ORDER",), 0)),
    ("P_ORDER", _set(("P_ORDER",), 11)), ("SLOPECUT", _set(("SLOPECUT",), 1.0)), ("SLOPECUT", _set(("SLOPECUT",), 0.0)),
    ("RAMPS", _set(("RAMPS",), [])), ("RAMPS", _set(("RAMPS",), [config()["RAMPS"][0]] * 9)), ("DARK", _set(("DARK",), 3)),
    ("DARK", _set(("DARK",), -4)), ("FORMAT", _set(("RAMPS", 0, "FORMAT"), 2)), ("NRAMP", _set(("RAMPS", 2, "NRAMP"), 0)),
    ("NRAMP", _set(("RAMPS", 2, "NRAMP"), 65537)), ("TSTART", _set(("RAMPS", 1, "TSTART"), 0)), ("FILE", _set(("RAMPS", 1, "FILE"), "x.dat")),
    ("'TSTART'", _set(("RAMPS", 0, "TSTART"), KeyError)), ("'P_ORDER'", _set(("P_ORDER",), KeyError)), ("'BIAS'", _set(("BIAS",), KeyError)),
    ("'SLICE'", _set(("BIAS", "SLICE"), KeyError)), ("PATH", _set(("BIAS", "PATH"), "roman")), ("TFRAME", _set(("TFRAME",), 0.0)),
    ("NEGATIVEPAD", _set(("NEGATIVEPAD",), -1)), ("'OUTPUT'", _set(("OUTPUT",), KeyError)),
]


@pytest.mark.parametrize("key,change", REFUSALS, ids=[f"{i}-{k}" for i, (k, _) in enumerate(REFUSALS)])
def test_config_refusals_name_the_key(key, change):
    c = copy.deepcopy(config())
    change(c)
    with pytest.raises(ValueError, match=key):
        linearity_run.parse_config(c)


def test_only_set_cannot_be_the_dark():
    c = config()
    c["RAMPS"] = c["RAMPS"][:1]
    with pytest.raises(ValueError, match="DARK"):
        linearity_run.parse_config(c)
