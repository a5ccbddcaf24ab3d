"""calfiles/_cubes.py: raw_cube, the one statement of how DarkStack.add, RampStack.add, NoiseStack.add and CorrStack.add_pair take
a cube of 16-bit samples, on numpy arrays (no GPU)."""

import numpy as np
import pytest

from romanimpreprocess_amd.calfiles._cubes import raw_cube


def test_the_two_type_errors_keep_their_text():
    for bad, name in ((np.zeros((2, 3, 4), np.float32), "float32"), (np.zeros((2, 3, 4), np.uint8), "uint8"),
                      (np.zeros((2, 3, 4), np.int32), "int32")):
        for be16 in (False, True):
            with pytest.raises(TypeError) as e:
                raw_cube(bad, be16, True)
            assert str(e.value) == f"a cube of 16-bit samples is needed, not {name}"
    for bad, text in ((np.zeros((2, 3, 4), np.int16), "<i2"), (np.zeros((2, 3, 4), ">i2"), ">i2"), (np.zeros((2, 3, 4), ">u2"), ">u2")):
        with pytest.raises(TypeError) as e:
            raw_cube(bad, False, True)
        assert str(e.value) == f"native samples must be uint16, not {text} (FITS storage: fits_be16=True)"
        assert raw_cube(bad, True, True).dtype == np.uint16   # any 16-bit integer words pass as FITS storage


def test_fits_storage_comes_back_as_a_uint16_view_of_the_same_bytes():
    be = (np.arange(24, dtype=np.int32).reshape(2, 3, 4) * 2731 - 32768).astype(">i2")
    out = raw_cube(be, True, True)
    assert out.dtype == np.uint16 and out.shape == be.shape and out.flags.c_contiguous
    assert np.shares_memory(out, be) and out.tobytes() == be.tobytes()
    native = np.arange(24, dtype=np.uint16).reshape(2, 3, 4)
    assert raw_cube(native, False, True) is native


def test_a_list_goes_through_numpy_and_is_refused_by_its_dtype():
    with pytest.raises(TypeError, match="a cube of 16-bit samples is needed, not int64"):
        raw_cube([[[1, 2], [3, 4]]], False, True)


def test_a_non_contiguous_array_is_made_contiguous():
    wide = np.arange(2 * 3 * 8, dtype=np.uint16).reshape(2, 3, 8)
    for view in (wide[:, :, ::2], wide[:, ::2], wide.transpose(0, 2, 1)):
        assert not view.flags.c_contiguous
        out = raw_cube(view, False, True)
        assert out.flags.c_contiguous and out.dtype == np.uint16 and np.array_equal(out, view)
    be = wide.astype(">i2")[:, :, 1::3]
    out = raw_cube(be, True, True)
    assert out.flags.c_contiguous and out.tobytes() == np.ascontiguousarray(be).tobytes()
    rows = wide[:, 1:]   # contiguous rows, frames apart: not C-contiguous as a whole
    assert raw_cube(rows, False, True).flags.c_contiguous


def test_the_leading_axis_is_dropped_only_where_allowed():
    four = np.arange(24, dtype=np.uint16).reshape(1, 2, 3, 4)
    out = raw_cube(four, False, True)
    assert out.shape == (2, 3, 4) and np.shares_memory(out, four)
    assert raw_cube(four, False, False).shape == (1, 2, 3, 4)        # DarkStack.add: its own shape check refuses it
    two = np.arange(24, dtype=np.uint16).reshape(2, 1, 3, 4)
    assert raw_cube(two, False, True).shape == (2, 1, 3, 4)          # only a leading axis of 1
    assert raw_cube(four[0], False, True).shape == (2, 3, 4)
    one = np.arange(12, dtype=np.uint16).reshape(1, 3, 4)
    assert raw_cube(one, False, True).shape == (1, 3, 4)             # a 3-D cube of one read keeps it
