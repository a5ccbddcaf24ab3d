"""Independent numpy restatement of what the reference's runs/summer2025run/convert_dark.py, convert_flt.py and convert_loflt.py do
to the frames of one exposure between reading them and writing the file (convert_flt.py:53-79; device code: csrc/rawframes.hip),
parameterised by the frame shape and by nflip, the number of leading columns that are mirrored (4096 in the scripts), and the
case tables of tests/test_gpu_rawframes.py.  tests/test_host_rawframes_ref.py holds this file against the scripts' own lines."""

import numpy as np

# ---------------------------------------------------------------------------------------------- the restatement
STORED = (0, 1, 2)   # native u16; FITS big-endian int16 with BZERO 32768; FITS big-endian int16, its bits kept


def decode(frame, stored):
    """:56, `cube[0, k, :, :] = f[0].data`: the uint16 samples of a frame given as stored (any 16-bit dtype, read as raw words)"""
    raw = np.ascontiguousarray(frame)
    if stored == 0:
        return raw.view(np.uint16).copy()
    be = raw.view(">i2")
    if stored == 1:   # astropy applies BZERO: int16 + 32768 -> uint16
        return (be.astype(np.int32) + 32768).astype(np.uint16)
    return be.astype(np.int16).astype(np.uint16)   # numpy's cast of the int16 data wraps


def encode(samples, stored):
    """the inverse: uint16 samples as a frame file holds them (stored 2: the same bits as a big-endian int16)"""
    samples = np.asarray(samples, np.uint16)
    if stored == 0:
        return samples.copy()
    if stored == 1:
        return (samples.astype(np.int32) - 32768).astype(">i2")
    return samples.view(np.int16).astype(">i2")


def orient_cube(cube, sca, nflip):
    """:59-63 on a (1, N, ny, nx) cube"""
    cube = cube.copy()
    if sca % 3 == 0:
        if nflip > 0:   # (nflip - 1 :: -1 with nflip = 0 would be -1 :: -1, the whole row)
            cube[:, :, :, :nflip] = cube[:, :, :, :nflip][:, :, :, ::-1].copy()
    else:
        cube = cube[:, :, ::-1, :]
    return np.ascontiguousarray(cube)


def orient_frame(frame, orient, nflip):
    """one frame by the `orient` code of rip_cal_raw_frame: 0 none, 1 columns 0 .. nflip-1 reversed, 2 rows reversed"""
    out = np.array(frame, copy=True)
    if orient == 1:
        out[:, :nflip] = frame[:, :nflip][:, ::-1]
    elif orient == 2:
        out = frame[::-1, :]
    return np.ascontiguousarray(out)


def nc_of(kind, N):
    """:66-68: the flat converters use 10 frames at most, convert_dark.py all"""
    return N if kind == "dark" else min(N, 10)


def slopes(cube, Nc):
    """:69-79 (convert_dark.py:66-76 with Nc = N) as written there, and :96 -- float32 (2, ny, nx)"""
    ny, nx = cube.shape[2:]
    slp = np.zeros((2, ny, nx))
    with np.errstate(all="ignore"):
        de = 0.0
        for k in range(1, Nc):
            slp[0, :, :] = slp[0, :, :] + cube[0, k, :, :] * (k - Nc / 2.0)
            de = de + (k - Nc / 2.0) ** 2
        slp[0, :, :] = slp[0, :, :] / de
        de = 0.0
        for k in range(1, Nc // 2):
            slp[1, :, :] = slp[1, :, :] + cube[0, k, :, :] * (k - (Nc // 2) / 2.0)
            de = de + (k - (Nc // 2) / 2.0) ** 2
        slp[1, :, :] = slp[1, :, :] / de
        return slp.astype(np.float32)


def exposure(frames, sca, nflip, kind):
    """(cube, slopes) of a list of uint16 frames, as the converter `kind` makes them"""
    cube = np.zeros((1, len(frames)) + frames[0].shape, dtype=np.uint16)
    for k, f in enumerate(frames):
        cube[0, k, :, :] = f
    cube = orient_cube(cube, sca, nflip)
    return cube, slopes(cube, nc_of(kind, len(frames)))


# ---------------------------------------------------------------------------------------------- case tables
# (ny, nx, nflip): wide with 8 reference-output columns; narrow, odd everything; a width that fits the wide form with an nflip
# that does not; no reference-output columns; one row of one chunk; nothing mirrored; the real row
FRAME_SHAPES = [(6, 32, 24), (5, 11, 7), (4, 32, 20), (3, 16, 16), (1, 8, 8), (7, 8, 0), (2, 4224, 4096)]
EDGE_SAMPLES = (0, 1, 32767, 32768, 65535)


def frame_samples(ny, nx, seed=0):
    """uint16 samples over the whole range with the five edge samples present (in the first row and, mirrored, the last)"""
    rng = np.random.default_rng(1000 + seed + 7 * ny + nx)
    f = rng.integers(0, 65536, (ny, nx)).astype(np.uint16)
    flat = f.reshape(-1)
    flat[:5] = EDGE_SAMPLES
    flat[-5:] = EDGE_SAMPLES
    return f


SLOPE_N = (1, 2, 3, 4, 5, 6, 7, 10, 11, 13)
SLOPE_NPIX = (1, 7, 8, 64 * 8 + 3)


def slope_cubes(N, npix, Nc):
    """name -> (1, N, 1, npix) uint16 cube: random samples; 65535 everywhere; 0 everywhere; 65535 only under the largest weight"""
    rng = np.random.default_rng(2000 + 31 * N + npix)
    peak = np.zeros((1, N, 1, npix), np.uint16)
    peak[0, Nc - 1] = 65535   # w0[k] = k - Nc / 2 is largest at k = Nc - 1 (plane 0, never read, where Nc = 1)
    return {"random": rng.integers(0, 65536, (1, N, 1, npix)).astype(np.uint16), "full": np.full((1, N, 1, npix), 65535, np.uint16),
            "zero": np.zeros((1, N, 1, npix), np.uint16), "peak": peak}


def nan_table(Nc):
    """(slp[0] is NaN, slp[1] is NaN) for Nc frames: 0 / 0 where a sum is empty or its only weight is zero"""
    return Nc <= 2, Nc <= 5
