"""Inputs of the dark-stack tests (tests/test_gpu_darkstack.py; tests/test_host_darkstack_ref.py proves that none of the clip
inputs has a borderline pixel, see tests/darkstack_ref.py), from seeded generators, and the writer of the small FITS files that
the reader and the make_dark_file drop-in are tested on."""

import numpy as np

# ---------------------------------------------------------------------------------------------- clip
# (planes, pixels): every plane count of the list 1, 2, 3, 4, 5, 63, 64, 65, 257, 512 (one wave's share of the planes is n / 4:
# empty shares, shares of different length, the largest column that LDS holds) and pixel counts 1, 63, 65 and 64 k + 7
CLIP_SHAPES = [(1, 65), (2, 63), (3, 1), (4, 199), (63, 65), (64, 63), (65, 199), (257, 65), (512, 199), (37, 1), (37, 63), (37, 65),
               (37, 199), (5, 65)]


def noisy(n, npix, seed, centre=1000.0, sd=5.0, frac=0.08):
    """a dark-like column per pixel: normal deviates around `centre` with a fraction of far values on both sides"""
    rng = np.random.default_rng(seed)
    a = centre + sd * rng.standard_normal((n, npix))
    hit = rng.random((n, npix)) < frac
    a = np.where(hit, a + rng.choice([-1.0, 1.0], (n, npix)) * rng.uniform(6 * sd, 60 * sd, (n, npix)), a)
    return a.astype(np.float32)


def second_round():
    """30 values within +-2 of zero, one at 8 and one at 1000: the first round removes 1000 only (s ~ 180), the second 8"""
    rng = np.random.default_rng(41)
    cols = []
    for _ in range(7):
        v = list(rng.uniform(-2, 2, 30)) + [8.0, 1000.0]
        cols.append(rng.permutation(v))
    return np.array(cols, np.float32).T.copy()


def ladder(nvals=16):
    """x_k = 2^k, k < nvals, times a power of two per pixel, in shuffled plane order: with 8 or more survivors the top value lies
    beyond median + 3 s while the next, half of it, does not, so every round removes exactly the top value: 16 -> 15 -> ... needs
    more than 5 rounds.  All values are dyadic and the sums exact."""
    rng = np.random.default_rng(42)
    cols = [rng.permutation(2.0 ** np.arange(nvals)) * 2.0 ** e for e in (-20, -3, 0, 1, 9)]
    return np.array(cols, np.float32).T.copy()


def ties():
    """few distinct values, so that the two middle values are equal or adjacent, odd and even counts (the last plane is NaN in
    every other pixel), and one far value"""
    rng = np.random.default_rng(43)
    a = rng.choice([10.0, 11.0, 12.0], (21, 70)).astype(np.float32)
    a[5] = 100.0
    a[20, ::2] = np.nan
    return a


def constant():
    a = np.empty((10, 66), np.float32)
    a[:] = (1234.5 + 0.25 * np.arange(66)).astype(np.float32)
    return a


def on_bound():
    """two planes: c = m = (a + b) / 2 and s = |a - b| / 2 exactly for dyadic a, b; with sigma = 1 both values lie ON their bounds
    (kept), with sigma = 0.5 outside (removed: nothing survives)"""
    return np.array([[1.0, -8.0, 0.5, 3.0], [3.0, -2.0, 0.75, 3.0]], np.float32)


def nonfinite():
    a = noisy(24, 70, 44)
    rng = np.random.default_rng(45)
    r = rng.random(a.shape)
    a[r < 0.05] = np.nan
    a[(r >= 0.05) & (r < 0.08)] = np.inf
    a[(r >= 0.08) & (r < 0.11)] = -np.inf
    a[:, 0] = np.nan
    a[:, 1] = np.inf
    a[:, 2] = np.nan
    a[7, 2] = 5.0          # a single finite value
    a[:, 3] = -np.inf
    a[::2, 3] = np.nan
    return a


def skewed():
    """for sigma_lower = 1.5, sigma_upper = 4"""
    rng = np.random.default_rng(46)
    return (500 + 10 * rng.standard_normal((40, 130)) + 40 * rng.random((40, 130)) ** 6).astype(np.float32)


def signed_zeros():
    rng = np.random.default_rng(47)
    a = np.round(2.0 * rng.standard_normal((16, 72)))          # many exact zeros, negative values
    a = np.where((a == 0) & (rng.random(a.shape) < 0.5), -0.0, a).astype(np.float32)
    a[:, 0] = -0.0
    a[:, 1] = 0.0
    a[:, 2] = [0.0, -0.0] * 8                                    # the two middle values are the two zeros
    a[:, 3] = [-0.0, 0.0] * 8
    a[:, 4] = [-3.0, -0.0, 0.0, 3.0] * 4
    a[:, 5] = -np.abs(a[:, 5]) - 1                               # all negative
    return a


# name -> (stack, keyword arguments of the clip)
def clip_cases():
    out = {f"n{n}_p{p}": (noisy(n, p, 100 + i), {}) for i, (n, p) in enumerate(CLIP_SHAPES)}
    out["second_round"] = (second_round(), {})
    out["ladder_5"] = (ladder(), {"maxiters": 5})
    out["ladder_16"] = (ladder(), {"maxiters": 16})
    out["ties"] = (ties(), {})
    out["constant"] = (constant(), {})
    out["on_bound_kept"] = (on_bound(), {"sigma": 1.0})
    out["on_bound_removed"] = (on_bound(), {"sigma": 0.5})
    out["nonfinite"] = (nonfinite(), {})
    out["asymmetric"] = (skewed(), {"sigma_lower": 1.5, "sigma_upper": 4.0})
    out["signed_zeros"] = (signed_zeros(), {})
    out["no_rounds"] = (noisy(9, 70, 48), {"maxiters": 0})
    return out


# ---------------------------------------------------------------------------------------------- group means
READS_MIXED = [0, 1, 1, 3, 5, 21, 24, 26]   # groups of 1, 2 and 16 reads with gaps between them


def cube_u16(nreads, ny, width, seed):
    """samples over the whole range, 0 and 65535 among them"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 65536, (nreads, ny, width)).astype(np.uint16)
    c[:, 0, 0], c[:, 0, 1] = 0, 65535
    c[::2, 1, 2], c[1::2, 1, 2] = 0, 65535
    return c


def cube_300(ny, width):
    """300 reads of 65535 / 65534: the f32 sum passes 2^24, where the order of the additions shows"""
    c = np.empty((300, ny, width), np.uint16)
    c[::2], c[1::2] = 65535, 65534
    c[:, 0, ::3] -= np.arange(300, dtype=np.uint16)[:, None] % 7
    return c


def dark_exposures(nexp=5, nreads=20, ny=36, width=70, seed=60):
    """dark-like cubes: a pedestal per pixel, a small ramp, read noise, and in a few (exposure, pixel) a step (a cosmic ray)"""
    rng = np.random.default_rng(seed)
    base = 1000 + 200 * rng.random((ny, width))
    rate = 0.5 * rng.random((ny, width))
    out = []
    for _ in range(nexp):
        c = base + rate * np.arange(nreads)[:, None, None] + 6 * rng.standard_normal((nreads, ny, width))
        hit = rng.random((ny, width)) < 0.03
        c[rng.integers(1, nreads):] += np.where(hit, 400 * rng.random((ny, width)), 0)
        out.append(np.clip(np.rint(c), 0, 65535).astype(np.uint16))
    return out


READS_E2E = [0, 1, 1, 2, 2, 6, 6, 16, 17, 20]


# ---------------------------------------------------------------------------------------------- FITS files
def _card(key, value):
    if isinstance(value, bool):
        v = "T" if value else "F"
        return f"{key:<8}= {v:>20}".ljust(80)
    if isinstance(value, str):
        q = "'" + value.replace("'", "''").ljust(8) + "'"
        return f"{key:<8}= {q}".ljust(80)
    if isinstance(value, float):
        return f"{key:<8}= {value!r:>20}".ljust(80)
    return f"{key:<8}= {value:>20d}".ljust(80)


def fits_hdu(data, cards=(), extension=False, pad=True):
    """bytes of one HDU: the mandatory cards for `data` (None: no data; int16 is written with BZERO = 32768 handling left to the
    caller's cards), `cards` (key, value) after them, END, blank padding; the data big-endian, zero-padded unless pad is False"""
    head = [_card("XTENSION", "IMAGE")] if extension else [_card("SIMPLE", True)]
    if data is None:
        head += [_card("BITPIX", 8), _card("NAXIS", 0)]
        raw = b""
    else:
        bitpix = {"i2": 16, "f4": -32, "f8": -64}[data.dtype.str[1:]]
        head += [_card("BITPIX", bitpix), _card("NAXIS", data.ndim)]
        head += [_card(f"NAXIS{i + 1}", int(n)) for i, n in enumerate(data.shape[::-1])]
        raw = data.astype(data.dtype.newbyteorder(">")).tobytes()
    if extension:
        head += [_card("PCOUNT", 0), _card("GCOUNT", 1)]
    head += [_card(k, v) for k, v in cards] + ["END".ljust(80)]
    text = "".join(head)
    text += " " * (-len(text) % 2880)
    if pad:
        raw += b"\0" * (-len(raw) % 2880)
    return text.encode("ascii") + raw


def write_dark_fits(path, cube):
    """a dark exposure as the detector software stores it: unsigned 16-bit samples as int16 with BZERO = 32768"""
    with open(path, "wb") as f:
        f.write(fits_hdu((cube.astype(np.int32) - 32768).astype(np.int16), [("BSCALE", 1), ("BZERO", 32768)]))
