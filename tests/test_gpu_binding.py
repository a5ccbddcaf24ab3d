"""``Context.call`` on the GPU: the same entry fed a numpy array, a ``DevArray`` and a torch tensor; NULL; a refusal of the library."""

import numpy as np
import pytest
from conftest import assert_same_bits, gpu_context

from romanimpreprocess_amd.devarray import DevArray
from romanimpreprocess_amd.utils import sky

pytestmark = pytest.mark.gpu

NY, NX, K = 8, 12, 4


def _frame():
    a = np.random.default_rng(5).normal(100.0, 7.0, (NY, NX)).astype(np.float32)
    a[1, 9] = np.nan                      # block (0, 2)
    mask = np.zeros((NY, NX), np.uint8)
    mask[6, 2] = 1                        # block (1, 0)
    return a, mask


def _bin_mean(ctx, a, mask, kind="numpy"):
    """rip_stage_bin_mean through Context.call with every array of the given kind"""
    import torch

    if kind == "numpy":
        out = np.empty((NY // K, NX // K), np.float32)
        ctx.call("rip_stage_bin_mean", a, mask, NY, NX, K, out)
        return out
    dev = torch.device("cuda", ctx.device)
    ta, tm = torch.from_numpy(a).to(dev), None if mask is None else torch.from_numpy(mask).to(dev)
    tout = torch.empty((NY // K, NX // K), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)           # the library runs on its own stream
    wrap = DevArray if kind == "devarray" else (lambda t: t)
    ctx.call("rip_stage_bin_mean", wrap(ta), None if tm is None else wrap(tm), NY, NX, K, wrap(tout))
    return tout.cpu().numpy()


def test_numpy_devarray_and_tensor_give_the_same_bits():
    ctx = gpu_context()
    a, mask = _frame()
    ref = sky.binkxk(a, K, mask=mask, ctx=ctx)
    assert np.isnan(ref[0, 2]) and np.isnan(ref[1, 0]) and np.count_nonzero(np.isnan(ref)) == 2
    want = np.where(mask != 0, np.nan, a).reshape(NY // K, K, NX // K, K).mean(axis=(1, 3))
    # two float32 sums of 16 values of one sign in different orders: each within 15 * 2^-24 of the exact sum, plus the division
    np.testing.assert_allclose(ref, want, rtol=2 * 16 * 2.0**-24)
    for kind in ("numpy", "devarray", "tensor"):
        assert_same_bits(_bin_mean(ctx, a, mask, kind), ref, kind)


def test_null_mask_equals_an_all_zero_mask():
    ctx = gpu_context()
    a, _ = _frame()
    zero = np.zeros((NY, NX), np.uint8)
    for kind in ("numpy", "devarray", "tensor"):
        got = _bin_mean(ctx, a, None, kind)
        assert_same_bits(got, _bin_mean(ctx, a, zero, kind), kind)
        assert np.count_nonzero(np.isnan(got)) == 1 and np.isnan(got[0, 2])


def test_a_refusal_of_the_library_is_a_valueerror_with_its_message():
    ctx = gpu_context()
    a, mask = _frame()
    before = _bin_mean(ctx, a, mask)
    big = np.zeros((256, 256), np.float32)
    counts = np.zeros(256 * 256, np.int64)
    with pytest.raises(ValueError, match=r"libromanhip: select_ranks: 65536 blocks \(256 x 256\) is more than the 65535"):
        ctx.call("rip_stage_select_ranks", big, 256, 256, 0, 0, 1, 1, 256, 256, 0, None, counts, None)
    with pytest.raises(TypeError, match="rip_stage_select_ranks: parameter 'arr'"):    # refused before the library sees it
        ctx.call("rip_stage_select_ranks", big.astype(np.float64), 256, 256, 0, 0, 1, 1, 16, 16, 0, None, counts, None)
    assert ctx.call("rip_stage_select_ranks", big, 256, 256, 0, 0, 16, 16, 16, 16, 0, None, counts, None) == 0
    assert (counts[:256] == 256).all()
    assert_same_bits(_bin_mean(ctx, a, mask), before, "after the refusal")
