"""The case table of tests/test_gpu_visualize.py (and the host checks of its inputs): small cubes, no larger than (5, 67, 301), at
the shapes where the selection and the picture kernels take another path.  The selection kernel works in tiles of 2048 samples
by workgroups of 256 threads (waves of 64)."""

import numpy as np

FULL = (5, 67, 301)   # 100835 samples = 49 tiles + 483


def u16_cube(seed, shape=FULL):
    return np.random.default_rng(seed).integers(0, 65536, shape, dtype=np.uint16)


def f32_cube(seed, shape=FULL):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-2, 3, shape)).astype(np.float32)


def low_bits_cube(seed, shape=(3, 40, 50)):
    """float32 values that differ only in the lowest 10 bits of their keys: levels 0 and 1 each find one bin"""
    rng = np.random.default_rng(seed)
    return (np.float32(1.5).view(np.uint32) + rng.integers(0, 1024, shape).astype(np.uint32)).view(np.float32)


def zeros_cube(seed, shape=(2, 30, 70)):
    """-0, +0 and a few other values"""
    return np.random.default_rng(seed).choice(np.array([-0.0, 0.0, -1.0, 1.0, -0.0, 0.0], np.float32), shape)


def inf_cube(seed):
    c = f32_cube(seed, (3, 20, 90))
    c.flat[[5, 700, 1300, 5399]] = [np.inf, -np.inf, np.inf, -np.inf]
    return c


def nan_cube(seed):
    c = f32_cube(seed, (3, 20, 90))
    c[0, 3, 4] = c[2, 19, 89] = np.nan
    c[1, 7, 7] = -np.nan
    return c


def ranks_for(n):
    """eight ranks: the ends, the same rank twice, neighbours (what a percentile asks for) and others"""
    return [0, n - 1, n // 2, n // 2, min(n // 2 + 1, n - 1), n // 3, (7 * n) // 8, min(1, n - 1)]


# name, cube, window (x0, x1, y0, y1) inclusive, planes (g0, g1), minus
SELECT_CASES = [
    ("one sample", u16_cube(1, (2, 3, 3)), (1, 1, 1, 1), (0, 1), None),
    ("one sample f32 minus", f32_cube(2, (2, 3, 3)), (2, 2, 0, 0), (1, 2), 0),
    ("odd x0 in a u16 cube", u16_cube(3), (7, 77, 3, 40), (0, 5), None),
    ("narrower than a wave", u16_cube(4), (10, 30, 0, 0), (2, 3), None),
    ("no multiple of the tile", f32_cube(5), (3, 102, 5, 37), (0, 5), None),      # 16500 = 8 tiles + 116
    ("the whole cube u16", u16_cube(6), (0, 300, 0, 66), (0, 5), None),
    ("the whole cube f32", f32_cube(7), (0, 300, 0, 66), (0, 5), None),
    ("the whole cube u16 minus", u16_cube(8), (0, 300, 0, 66), (0, 5), 1),        # negative differences
    ("the whole cube f32 minus", f32_cube(9), (0, 300, 0, 66), (0, 5), 1),
    ("one plane minus another u16", u16_cube(10), (1, 299, 1, 65), (4, 5), 1),
    ("all equal u16", np.full((3, 40, 50), 1234, np.uint16), (0, 49, 0, 39), (0, 3), None),
    ("all equal f32", np.full((3, 40, 50), 1.5, np.float32), (0, 49, 0, 39), (0, 3), None),
    ("all equal minus itself", np.full((3, 40, 50), 77, np.uint16), (0, 49, 0, 39), (0, 3), 1),   # all +0
    ("lowest 10 key bits", low_bits_cube(11), (0, 49, 0, 39), (0, 3), None),
    ("-0 and +0", zeros_cube(12), (0, 69, 0, 29), (0, 2), None),
    ("infinities", inf_cube(13), (0, 89, 0, 19), (0, 3), None),
]

# the float32 inputs of the power-norm panels: random values over and beyond the colour range
POWER_CUBE = f32_cube(21, (3, 37, 61))
POWER_CUBE[0] = np.random.default_rng(22).uniform(-50.0, 1200.0, (37, 61)).astype(np.float32)
POWER_LIMITS = (np.float32(-12.5), np.float32(1000.25))
