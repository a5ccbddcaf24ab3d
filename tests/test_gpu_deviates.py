"""The device deviates are Philox-4x32-10 at the documented counters (DESIGN.md "Shared device headers"): the outputs of the
entry points that draw on the device against a numpy restatement (``philox_ref.py``) of the generator and of what each kernel
makes of its blocks."""

import numpy as np
import pytest
from conftest import gpu_context

import philox_ref
from romanimpreprocess_amd.L1_to_L2 import gen_noise_image

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15   # both halves non-zero


def test_injected_normals_are_philox_at_the_documented_counter():
    """counter {active pixel index, group, layer, 'nois'}, Box-Muller on words 0 and 1.  The device's f32 logf / cospif are a few
    ulp off the f64 value: ~1e-6 relative on |z| < 6, 0.01 DN on the product -- across one rounding boundary and no further."""
    rp = [[0], [1, 2]]
    ny, nx, nb, layer = 12, 72, 4, 3
    data = np.full((2, ny, nx), 32768, np.uint16)
    read = np.full((ny, nx), 2048.0, np.float32)
    got = gen_noise_image.inject_read_noise(data, read, rp, nb=nb, seed=SEED, layer=layer, ctx=gpu_context())
    assert np.array_equal(got[:, :nb], data[:, :nb]) and np.array_equal(got[:, :, -nb:], data[:, :, -nb:])
    z = philox_ref.injected_normals(SEED, layer, 2, (ny - 2 * nb) * (nx - 2 * nb)).reshape(2, ny - 2 * nb, nx - 2 * nb)
    want = np.rint(32768.0 + z * 2048.0 / np.sqrt([[[1.0]], [[2.0]]]))
    assert want.min() > 0 and want.max() < 65535
    diff = np.abs(got[:, nb:-nb, nb:-nb].astype(np.float64) - want)
    print("injected normals: max |got - expected| = %g DN, %d of %d differ" % (diff.max(), np.count_nonzero(diff), diff.size))
    assert diff.max() <= 1.0


@pytest.mark.parametrize("lam", [0.75, 9.5, 10.5, 900.0])
def test_resampled_poisson_is_the_documented_recipe(lam):
    """a single read, weight 1, gain 1, frame time 1: the layer is k - lam.  0.75 and 9.5 take the inversion, 10.5 and 900 the
    transformed rejection; 1000 pixels: the last workgroup is partly empty"""
    n, layer = 1000, 5
    diff = np.zeros((1, n), np.float32)
    gen_noise_image.poisson_resample(diff, np.full((1, n), lam, np.float32), np.ones((1, n), np.float32), 1.0, [[0]],
                                     np.ones((1, 1), np.float32), np.ones(1, np.uint8), np.zeros((1, n), np.int8), seed=SEED,
                                     layer=layer, ctx=gpu_context())
    k = diff[0].astype(np.float64) + lam
    ref = [philox_ref.device_poisson(lam, SEED, layer, 0, i) for i in range(n)]
    want = np.array([r[0] for r in ref])
    sure = np.array([r[1] for r in ref])
    print("lam %g: %d pixels left out, %d differ" % (lam, n - np.count_nonzero(sure), np.count_nonzero(k[sure] != want[sure])))
    assert np.count_nonzero(~sure) <= 1
    assert np.array_equal(k[sure], want[sure])


@pytest.mark.parametrize("rows,width", [(8, 8), (5, 7)])
def test_1f_frames_draw_the_documented_deviates(rows, width):
    """device deviates against the same frames from the numpy deviates: (8, 8) is the smallest length the hand-written transform
    takes, (5, 7) an odd length that goes through the library's.  The deviates agree to f32 rounding, the frame is linear in them."""
    ctx = gpu_context()
    stream = 7
    got = gen_noise_image.noise_1f_frames(3, rows=rows, width=width, seed=SEED, stream=stream, ctx=ctx)
    normals = philox_ref.pink_normals(3, rows, width, SEED, stream)
    want = gen_noise_image.noise_1f_frames(3, rows=rows, width=width, normals=normals, ctx=ctx)
    scale = np.abs(want).max()
    print("1/f frames %d x %d: max |got - want| / max |want| = %g" % (rows, width, np.abs(got - want).max() / scale))
    assert scale > 0.1
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-5 * scale)
