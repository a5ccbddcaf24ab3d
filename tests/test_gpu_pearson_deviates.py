"""The deviates of ``csrc/pearson.hip`` against ``tests/pearson_ref.py`` (DESIGN.md "Shared device headers", row 5).

Replay: every row of ``pearson_ref.ROWS`` -- one per branch of the sampler -- draw by draw on 4133 elements and two streams.
A draw is compared wherever the restatement is sure of every decision (at most 0.1 % are not, asserted by
``test_host_pearson_ref.py``): ``|got - want| <= tol * scale``, ``scale`` the sum of the magnitudes of the terms of the last
expression and ``tol`` = 8 E_ref, the f64 noise of the recipe itself measured against mpmath (``pearson_ref.tolerance``; nothing
here is tuned on the device).  At most 7e-13, so an error of 1e-9 in ``re_lgamma_complex``, a reused uniform or a wrong
parameter shows.  Distribution: 200 000 device deviates per row against the analytic law, ``sqrt(n) D < 2.2`` -- the twin of
the host test, independent of the replay.  Finite everywhere: every intensity of every golden case.

Figures of the replay on an MI355X: ``profiles/pearson_replay.txt``."""

import numpy as np
import pytest
import torch
from conftest import gpu_context, load_golden

import pearson_ref as pr

pytestmark = pytest.mark.gpu

GOLDENS = (load_golden("pearson_params"), load_golden("pearson_edges"))
KS_BOUND = 2.2     # asymptotic false-alarm rate 2 exp(-2 * 2.2^2) = 1.2e-4 a case; seeds are fixed


def golden_cases():
    return [(g, k[3:-6]) for g in GOLDENS for k in g if k.endswith("_types")]


def stage_pearson(t, I, seed, stream):
    """(draws, types, params) of one call on host arrays"""
    ctx = gpu_context()
    I = np.ascontiguousarray(I, dtype=np.float64)
    draws, types, params = np.empty(I.size, np.float64), np.empty(I.size, np.int32), np.empty((I.size, 4), np.float64)
    ctx.check(ctx.lib.rip_stage_pearson(ctx.h, I.size, I.ctypes.data, t[0], t[1], t[2], seed, stream, draws.ctypes.data,
                                        types.ctypes.data, params.ctypes.data))
    return draws, types, params


@pytest.mark.parametrize("row", pr.ROWS, ids=pr.row_id)
def test_replay(row):
    tol = pr.tolerance(row)
    seen = []
    for stream in pr.STREAMS:
        want = pr.replay_case(row, stream)
        got, types, params = stage_pearson(want.t, np.full(pr.N_REPLAY, want.I), pr.SEED, stream)
        # the classification and the draw see the same values: those of the restatement
        np.testing.assert_array_equal(types, want.types)
        assert np.all(types == pr.ROW_TYPES[pr.ROWS.index(row)])
        np.testing.assert_array_equal(params, want.par)
        sure = want.sure
        dev = np.abs(got[sure] - want.x[sure]) / want.scale[sure]
        worst = int(np.argmax(dev))
        print("replay %s stream %#x: %d of %d left out, E_ref %.3g, tol %.3g, largest deviation %.3g (element %d: %.17g, "
              "expected %.17g); %d unsure draws differ by more" % (
                  pr.row_id(row), stream, np.count_nonzero(~sure), sure.size, want.e_ref, tol, dev[worst],
                  np.nonzero(sure)[0][worst], got[sure][worst], want.x[sure][worst],
                  np.count_nonzero(np.abs(got[~sure] - want.x[~sure]) > tol * want.scale[~sure])))
        assert np.count_nonzero(~sure) <= pr.SHARE_LEFT_OUT * sure.size
        assert np.all(np.isfinite(got))
        assert np.count_nonzero(dev > tol) == 0, "%d of %d sure draws off by more than %.3g of their scale; largest %.3g" % (
            np.count_nonzero(dev > tol), dev.size, tol, dev[worst])
        seen.append(got)
    assert not np.array_equal(seen[0], seen[1])     # (a beta of shape 1e-3 puts nine draws in ten on one f64 value)


@pytest.mark.parametrize("row", pr.ROWS, ids=pr.row_id)
def test_distribution(row):
    name, I = row
    t = pr.moment_ratios(GOLDENS, name)
    ctx = gpu_context()
    dev = torch.device("cuda", ctx.device)
    d_I = torch.full((pr.N_LAW,), I, dtype=torch.float64, device=dev)
    d_x = torch.empty(pr.N_LAW, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rip_stage_pearson(ctx.h, pr.N_LAW, d_I.data_ptr(), t[0], t[1], t[2], pr.SEED, 11, d_x.data_ptr(), None, None))
    x = d_x.cpu().numpy()
    assert np.all(np.isfinite(x))
    types, par = pr.classify(*t, [I])
    cdf = pr.analytic_cdf(types[0], par[0], 1.0 if t[1] >= 0.0 else -1.0)
    ks = pr.ks_sqrt_n(x, cdf, pr.rounding_width(types[0], par[0], np.abs(x).max()))
    print("distribution %s: sqrt(n) D = %.3f" % (pr.row_id(row), ks))
    assert ks < KS_BOUND


@pytest.mark.parametrize("g,name", golden_cases(), ids=[n for _g, n in golden_cases()])
def test_finite_everywhere(g, name):
    """every intensity of every golden case, 0.01 (the clip) and 1e7, 64 draws each: finite wherever the type is non-zero,
    exactly 0 where it is 0 -- next to the type-5 curve too, where the reference raises (``raises`` of pearson_edges)"""
    I = g[f"cl_{name}_I"] if f"cl_{name}_I" in g else g["cl_I"]
    I = np.repeat(np.concatenate([I, [0.01, 1e7]]), 64)
    t = pr.moment_ratios(GOLDENS, name)
    x, types, params = stage_pearson(t, I, pr.SEED, 5)
    want_types, _par = pr.classify(*t, I)
    bad = ~np.isfinite(x)
    assert not bad.any(), "%d deviates not finite, at intensities %s (types %s)" % (
        np.count_nonzero(bad), np.unique(I[bad])[:8], np.unique(types[bad]))
    np.testing.assert_array_equal(types, want_types)
    assert np.all(x[types == 0] == 0.0) and np.all(np.isfinite(params))
