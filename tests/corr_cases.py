"""The case table of tests/test_gpu_corr.py: pairs of small exposure cubes at the shapes where csrc/corrstat.hip can go wrong, and
the planted values of the round trips.  Every case is (nreads, ny_file, nx_file, ny, nx, nb, sy, sx, frames, maker); ``pair(name)``
builds its two native uint16 cubes, the same on every call."""

import functools

import corr_ref as ref
import numpy as np


def _noisy(rng, nreads, ny, nx, sigma=30.0):
    """a ramp of 400 DN per frame on a pedestal with Gaussian noise: the quartile rule has a width to work with"""
    t = np.arange(nreads, dtype=np.float64)[:, None, None]
    return np.clip(np.rint(6000.0 + 400.0 * t + sigma * rng.standard_normal((nreads, ny, nx))), 0, 65535).astype(np.uint16)


def gaussian(rng, c):
    return _noisy(rng, c[0], c[1], c[2]), _noisy(rng, c[0], c[1], c[2])


def extremes(rng, c):
    """0 and 65535 side by side in a checkerboard: e = +-131070 in every pixel, every product at its bound, all kept"""
    nreads, ny, nx = c[:3]
    board = (np.add.outer(np.arange(ny), np.arange(nx)) % 2).astype(np.uint16) * 65535
    a = np.empty((nreads, ny, nx), np.uint16)
    a[::2], a[1::2] = board, 65535 - board
    fa, _, _, fd = c[8]
    assert (fd - fa) % 2 == 1
    return a, (65535 - a).astype(np.uint16)


def outliers(rng, c):
    """hot pixels in the last frame of the first exposure, for 32 x 32 superpixels with a border of 4: on the corner (32, 32), the
    edge (32, 45) and the interior (40, 40) of superpixel (1, 1), on both sides of the boundaries (31 | 32, 10) and (10, 31 | 32),
    a diagonal pair across a corner (31, 31) -- and a cluster of three inside superpixel (0, 1)"""
    a, b = gaussian(rng, c)
    for y, x in ((32, 32), (32, 45), (40, 40), (31, 10), (32, 10), (10, 31), (10, 32), (31, 31), (20, 50), (20, 51), (21, 50)):
        a[c[8][3], y, x] += 5000
    b[c[8][0], 50, 20] += 3000   # and a negative one: the first frame of the second exposure
    return a, b


def constant(rng, c):
    a = np.full(c[:3], 1234, np.uint16)
    return a, a.copy()


def ties(rng, c):
    """e takes the values -1, 0, 1 only: every rank falls into a run of equal values, and q75 - q25 is 0, 1 or 2"""
    nreads, ny, nx = c[:3]
    a = np.full((nreads, ny, nx), 1000, np.uint16)
    b = a.copy()
    a[c[8][3]] += rng.integers(0, 2, size=(ny, nx)).astype(np.uint16)
    b[c[8][3]] += rng.integers(0, 2, size=(ny, nx)).astype(np.uint16)
    a[c[8][3], : ny // 2] = 1000   # the upper half: e in {-1, 0}, the median sits in the run of zeros
    return a, b


CASES = {
    # the 16-byte path and the crop of a wider file
    "crop_w8": (6, 64, 72, 64, 64, 4, 32, 32, (1, 2, 3, 5), gaussian),
    # superpixels that hold border pixels (sx % 8 == 0: one sample per lane only from a cube that is not 16-byte aligned)
    "border_inside": (5, 40, 48, 40, 48, 4, 20, 24, (1, 2, 2, 4), gaussian),
    # one sample per lane by the shape: sx % 8 != 0, an odd file width, a crop in both directions
    "lane1": (5, 42, 47, 40, 44, 4, 20, 22, (1, 3, 2, 4), gaussian),
    # the corner and edge superpixels are all border: zeros, and no fault
    "all_border": (4, 16, 16, 16, 16, 4, 4, 4, (0, 1, 2, 3), gaussian),
    # the full production tile: 128 x 128 in one workgroup
    "full_tile": (4, 128, 128, 128, 128, 4, 128, 128, (0, 1, 2, 3), gaussian),
    # superpixels of one row: no vertical or diagonal pair, m = 0 there
    "rows": (4, 8, 128, 8, 128, 1, 1, 128, (0, 1, 2, 3), gaussian),
    # e = +-131070, products beyond 32 bits, sum e^2 near 2^48
    "extremes": (4, 128, 128, 128, 128, 0, 128, 128, (0, 1, 2, 3), extremes),
    "outliers": (6, 64, 64, 64, 64, 4, 32, 32, (1, 2, 3, 5), outliers),
    "constant": (4, 32, 32, 32, 32, 4, 16, 16, (0, 2, 1, 3), constant),
    "ties": (4, 32, 40, 32, 40, 2, 16, 8, (0, 1, 1, 3), ties),
    # fa = 0 and fd the last frame; b > c
    "first_last": (7, 24, 24, 24, 24, 4, 12, 12, (0, 5, 2, 6), gaussian),
}


@functools.lru_cache(maxsize=None)
def pair(name):
    c = CASES[name]
    a, b = c[9](np.random.default_rng(sorted(CASES).index(name) + 100), c)
    a.setflags(write=False), b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restated table of a case, computed once"""
    c = CASES[name]
    a, b = pair(name)
    t = ref.pair_table(a, b, c[8], *c[3:8])
    t.setflags(write=False)
    return t


# ---- the host round trip (tests/test_host_corr.py): the planted values of the issue
PLANTED = {"g": 1.8, "aH": 0.020, "aV": 0.012, "aD": 0.003, "beta": 1.5e-6}
RATE, DARK_RATE, READ_NOISE = 600.0, 2.0, 7.0
FRAMES, TIMEREF, NREADS = (1, 7, 8, 14), 1, 16   # TIME 2 8 9 15
COLUMN = {"g": 5, "aH": 6, "aV": 7, "beta": 8, "I": 9, "aD": 10}
NSIGMA = 5.0


def config_text(target="/data/cal/07", sca=7, estart=11, eend=20, fmt=1, nbin=(32, 32), time=(2, 8, 9, 15), output=None):
    """the text ``write_solid-waffle_config.pl <target> <sca> <estart> <eend>`` prints, line by line (its print statements restated
    as data: the keys, their order and their values)"""
    lines = [f"DETECTOR: SCA{sca:02d}", "LIGHT:"]
    lines += [f"{target}/99999999_SCA{sca:02d}_Flat_{e:03d}.fits" for e in range(estart, eend + 1)]
    lines += ["DARK:"]
    lines += [f"{target}/99999999_SCA{sca:02d}_Noise_{e:03d}.fits" for e in range(estart, eend + 1)]
    lines += [f"FORMAT: {fmt}", "CHAR: Advanced 1 3 3 bfe", "TIMEREF: 1", f"NBIN: {nbin[0]} {nbin[1]}", "FULLNL: True True True",
              "NLPOLY: 3 2 16", "IPCSUB: True", "TIME: " + " ".join(str(t) for t in time),
              "OUTPUT: " + (output or f"{target}/sw-SCA{sca:02d}-E{estart:03d}"), "HOTPIX: 1000 2000 0.1 0.1"]
    return "\n".join(lines) + "\n"
