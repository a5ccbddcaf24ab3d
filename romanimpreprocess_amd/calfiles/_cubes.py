"""The cube of raw 16-bit samples as the entries that read one take it (``rip_cal_group_means``, ``rip_cal_frame_sums``,
``rip_cal_noise_add``, ``rip_cal_corr_pair``; ``csrc/rip_samples.h`` decodes it): one statement for ``DarkStack.add``,
``RampStack.add``, ``NoiseStack.add`` and ``CorrStack.add_pair``, which keep their own shape checks."""

import numpy as np

from ..devarray import DevArray, is_dev


def raw_cube(cube, fits_be16, drop_leading):
    """``cube`` (numpy array, memory map or ``DevArray``) as contiguous 16-bit words seen as uint16: a numpy array, or a ``DevArray``
    whose producer has finished.  ``fits_be16``: the samples are FITS storage (big-endian int16 with ``BZERO = 32768``), which the
    entry un-swaps itself; otherwise they must be native uint16.  ``drop_leading``: a (1, nreads, ny, nx) cube, as
    ``frames_to_cube`` makes them, loses its first axis.  TypeError for anything but 16-bit integers."""
    dev = is_dev(cube)
    if not dev and not isinstance(cube, np.ndarray):
        cube = np.asarray(cube)
    if drop_leading and cube.ndim == 4 and cube.shape[0] == 1:
        cube = DevArray(cube.t[0], cube.dtype) if dev else cube[0]
    if cube.dtype.itemsize != 2 or cube.dtype.kind not in "iu":
        raise TypeError(f"a cube of 16-bit samples is needed, not {cube.dtype.name}")
    if not fits_be16 and (cube.dtype.kind != "u" or cube.dtype.byteorder == ">"):
        raise TypeError(f"native samples must be uint16, not {cube.dtype.str} (FITS storage: fits_be16=True)")
    if dev:
        cube.sync()
    elif not cube.flags.c_contiguous:
        cube = np.ascontiguousarray(cube)
    if cube.dtype != np.uint16:   # FITS storage: the same 16-bit words
        cube = DevArray(cube.t, np.uint16) if dev else cube.view(np.uint16)
    return cube
