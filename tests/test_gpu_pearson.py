"""Pseudo-Poisson noise layers (the ``O`` directives): the Pearson-family sampler on the GPU.

The distribution PARAMETERS of every pixel are pinned by goldens made with the reference's own module
(``tools/make_goldens.py pearson``: ``L1_to_L2/GalPoisson/draw_with_tilnus.py`` with its samplers replaced by recorders); the
DEVIATES come from the device's generator (the reference's scipy / numpy streams are not reproducible): their first four
moments are tested against the targets the sampler is built to match."""

import numpy as np
import pytest
import torch
from conftest import assert_same_bits, gpu_context, load_golden

from romanimpreprocess_amd.L1_to_L2.GalPoisson import draw_with_tilnus as dw

pytestmark = pytest.mark.gpu

CASES = ["poisson_like", "neg_skew", "beta_prime", "beta_prime_neg", "heavy_tail", "heavy_tail_neg", "symmetric", "light_tail",
         "ramp_fit_weights"]
# on the curves of types 3 and 5 and to either side of them (tools/make_goldens.py pearson_edges), each with its own intensities
EDGE_CASES = ["gamma", "gamma_neg", "inv_gamma", "inv_gamma_neg", "inv_gamma_b"]


@pytest.mark.parametrize("name", CASES + EDGE_CASES)
def test_types_and_parameters_match_the_reference(name):
    g = load_golden("pearson_edges" if name in EDGE_CASES else "pearson_params")
    t21, t31, t41 = g[f"cl_{name}_t"]
    types, params = dw.classify(t21, t31, t41, g[f"cl_{name}_I"] if name in EDGE_CASES else g["cl_I"], ctx=gpu_context())
    ref_t, ref_p = g[f"cl_{name}_types"], g[f"cl_{name}_params"]
    np.testing.assert_array_equal(types, ref_t)
    if name in EDGE_CASES:
        # type 3 at every intensity, type 5 at the first; type 0 where the reference raises ValueError (next to type 5)
        assert np.all(ref_t == 3) if name.startswith("gamma") else ref_t[0] == 5
        assert np.all(ref_t[g[f"cl_{name}_raises"]] == 0)
    # f64 formulas in the reference's order; powers (** 3, ** 1.5) may round differently in the last place
    np.testing.assert_allclose(params, ref_p, rtol=1e-11, atol=1e-300)


@pytest.mark.parametrize("name,I", [("poisson_like", 3.0), ("poisson_like", 400.0), ("neg_skew", 20.0), ("beta_prime", 30.0),
                                    ("beta_prime_neg", 60.0), ("heavy_tail", 40.0), ("heavy_tail_neg", 80.0), ("symmetric", 25.0),
                                    ("light_tail", 50.0), ("ramp_fit_weights", 2000.0)])
def test_moments_of_the_deviates(name, I):
    g = load_golden("pearson_params")
    t21, t31, t41 = (float(v) for v in g[f"cl_{name}_t"])
    n = 2_000_000
    x = dw.draw_from_Pearson(t21, t31, t41, np.full(n, I), rng=np.random.default_rng(5), ctx=gpu_context())
    assert np.all(np.isfinite(x))
    m2, m3, m4 = t21 * I, t31 * I, 3.0 * t21**2 * I**2 + t41 * I
    assert m4 > 0 and m2 > 0
    sd = np.sqrt(m2)
    # standard errors of the sample moments from the target moments themselves (sixth / eighth moments bounded generously)
    assert abs(np.mean(x)) < 6.0 * sd / np.sqrt(n)
    assert abs(np.var(x) / m2 - 1.0) < 6.0 * np.sqrt((m4 / m2**2 - 1.0) / n) + 1e-3
    c3 = np.mean((x - x.mean()) ** 3)
    assert abs(c3 - m3) < 0.03 * sd**3 * max(1.0, m4 / m2**2 / 3.0)
    c4 = np.mean((x - x.mean()) ** 4)
    assert abs(c4 / m4 - 1.0) < 0.06 * max(1.0, m4 / m2**2 / 3.0)
    # a different stream gives different deviates, the same arguments the same ones
    y = dw.draw_from_Pearson(t21, t31, t41, np.full(1000, I), rng=np.random.default_rng(5), ctx=gpu_context(), stream=7)
    z = dw.draw_from_Pearson(t21, t31, t41, np.full(1000, I), rng=np.random.default_rng(5), ctx=gpu_context(), stream=7)
    w = dw.draw_from_Pearson(t21, t31, t41, np.full(1000, I), rng=np.random.default_rng(5), ctx=gpu_context(), stream=8)
    assert np.array_equal(y, z) and not np.array_equal(y, w)


def test_inadmissible_and_edge_inputs():
    x = dw.draw_from_Pearson(1.0, 1.0, 1.7, np.array([1e-3, 0.0, -4.0, np.nan, 1e5]), rng=1, ctx=gpu_context())
    t, _p = dw.classify(1.0, 1.0, 1.7, np.array([1e-3, 0.0, -4.0, np.nan, 1e5]), ctx=gpu_context())
    assert t.tolist()[:4] == [0, 0, 0, 0] and t[4] == 6
    assert np.all(x[:4] == 0.0) and np.isfinite(x[4])
    assert dw.draw_from_Pearson(1.0, 1.0, 1.0, np.zeros((0,)), ctx=gpu_context()).shape == (0,)


def test_host_arrays_and_device_pointers_give_the_same_bits():
    """rip_stage_pearson takes host arrays or device pointers for I, draws, types and params (csrc/rip_host.h): the noise-layer
    loop hands it tensors that live in HBM.  4133 elements: the last block of 256 threads is partly empty."""
    g = load_golden("pearson_params")
    ctx = gpu_context()
    dev = torch.device("cuda", ctx.device)
    n, seed, stream = 4133, 20250101, 7
    for name, I in (("poisson_like", 3.0), ("neg_skew", 20.0), ("beta_prime", 30.0), ("heavy_tail", 40.0), ("light_tail", 50.0)):
        t21, t31, t41 = (float(v) for v in g[f"cl_{name}_t"])
        h_I = np.full(n, I)
        d_I = torch.from_numpy(h_I).to(dev)
        h_draw = np.empty(n, np.float64)
        d_draw = torch.empty(n, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.check(ctx.lib.rip_stage_pearson(ctx.h, n, h_I.ctypes.data, t21, t31, t41, seed, stream, h_draw.ctypes.data, None, None))
        ctx.check(ctx.lib.rip_stage_pearson(ctx.h, n, d_I.data_ptr(), t21, t31, t41, seed, stream, d_draw.data_ptr(), None, None))
        assert np.all(np.isfinite(h_draw)) and np.unique(h_draw).size > n // 2
        assert_same_bits(d_draw.cpu().numpy(), h_draw, f"{name}: draws through device pointers")
        # no draws: types and parameters only
        h_t, h_p = np.empty(n, np.int32), np.empty((n, 4), np.float64)
        d_t = torch.empty(n, dtype=torch.int32, device=dev)
        d_p = torch.empty((n, 4), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.check(ctx.lib.rip_stage_pearson(ctx.h, n, h_I.ctypes.data, t21, t31, t41, seed, stream, None, h_t.ctypes.data, h_p.ctypes.data))
        ctx.check(ctx.lib.rip_stage_pearson(ctx.h, n, d_I.data_ptr(), t21, t31, t41, seed, stream, None, d_t.data_ptr(), d_p.data_ptr()))
        assert h_t.min() == h_t.max() != 0
        assert_same_bits(d_t.cpu().numpy(), h_t, f"{name}: types through device pointers")
        assert_same_bits(d_p.cpu().numpy(), h_p, f"{name}: parameters through device pointers")
