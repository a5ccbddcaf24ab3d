"""Plain numpy / scipy reference of the cosmic-ray model, shared by ``test_host_cr_ref.py``
(CPU) and ``test_gpu_cosmic_rays.py`` (GPU).  Written independently of ``csrc/cr.hip``: the traversal sorts the parameters at
which the segment crosses a pixel boundary and gives every part to the pixel of its middle (the kernel walks from crossing to
crossing), the sampler is ``scipy.interpolate.interp1d`` itself.  Test infrastructure only."""

import math

import numpy as np
from scipy.interpolate import interp1d

PARAMS = dict(flux=8.0, area=16.8, conversion_factor=0.5, pixel_size=10.0, pixel_depth=5.0, min_dEdx=10.0, max_dEdx=10000.0,
              min_cr_len=10.0, max_cr_len=2000.0, grid_size=10000, location=120.0, scale=50.0, slope=-4.33)
EPS = 1e-10   # pixels: parts of a track shorter than this do not count (a track through a corner crosses one boundary)


def params(**kw):
    p = dict(PARAMS)
    p.update(kw)
    return p


# ------------------------------------------------------------------------------------------ (b) sampling
def _cdf(x, y):
    c = np.cumsum(y) - y[0]
    return c / c.max()


def tables(par=PARAMS):
    """(c_len, x_len, c_dEdx, x_dEdx).  The densities through the C library's pow / exp one element at a time: numpy's
    vectorised versions may differ from them in the last bit on some machines, and where the CDF is flat one bit of c moves
    the interpolated x by many -- the library's host code calls the C library too."""
    n = int(par["grid_size"])
    x_len = np.linspace(par["min_cr_len"], par["max_cr_len"], n)
    y_len = np.array([math.pow(v, par["slope"]) for v in x_len])
    x_de = np.linspace(par["min_dEdx"], par["max_dEdx"], n)
    s = (x_de - par["location"]) / par["scale"]
    y_de = np.array([math.exp(-(v + math.exp(-v)) / 2) for v in s])
    return _cdf(x_len, y_len), x_len, _cdf(x_de, y_de), x_de


def sample(u, n_i, n_j, par=PARAMS, tabs=None):
    """(i0, j0, phi, length, dEdx) from uniforms ``u`` (n, 5)."""
    u = np.asarray(u, dtype=np.float64).reshape(-1, 5)
    c_len, x_len, c_de, x_de = tabs or tables(par)
    return (u[:, 0] * n_i, u[:, 1] * n_j, 2 * np.pi * u[:, 2], interp1d(c_len, x_len)(u[:, 3]), interp1d(c_de, x_de)(u[:, 4]))


def moyal_cdf(x, par=PARAMS):
    """closed form of the CDF of the energy loss on its range"""
    from scipy.special import erfc

    f = lambda v: erfc(np.exp(-(np.asarray(v, dtype=np.float64) - par["location"]) / (2 * par["scale"])) / np.sqrt(2.0))   # noqa: E731
    return (f(x) - f(par["min_dEdx"])) / (f(par["max_dEdx"]) - f(par["min_dEdx"]))


def length_cdf(x, par=PARAMS):
    a = par["slope"] + 1.0
    lo, hi = par["min_cr_len"], par["max_cr_len"]
    return (np.asarray(x, dtype=np.float64) ** a - lo ** a) / (hi ** a - lo ** a)


# ------------------------------------------------------------------------------------------ (c) end point
def endpoints(i0, j0, phi, length, n_i, n_j, par=PARAMS):
    len_px = length / par["pixel_size"]
    return (np.clip(i0 + len_px * np.cos(phi), -0.5, n_i + 0.5), np.clip(j0 + len_px * np.sin(phi), -0.5, n_j + 0.5))


# ------------------------------------------------------------------------------------------ (d) traversal
def _crossings(a0, a1):
    """parameters t in (0, 1) at which a0 + t (a1 - a0) passes a half-integer"""
    if a1 == a0:
        return []
    lo, hi = min(a0, a1), max(a0, a1)
    ks = np.arange(math.floor(lo - 0.5) - 1, math.ceil(hi - 0.5) + 2)
    t = (ks + 0.5 - a0) / (a1 - a0)
    return list(t[(t > 0) & (t < 1)])


def traverse(i0, j0, i1, j1):
    """[(i, j, l2)] for every pixel that holds a part of the segment (off-image pixels included), in the order of the walk"""
    length = math.hypot(i1 - i0, j1 - j0)
    ts = np.unique(np.array([0.0, 1.0] + _crossings(i0, i1) + _crossings(j0, j1)))
    out = []
    for ta, tb in zip(ts[:-1], ts[1:]):
        seg = (tb - ta) * length
        if seg < EPS:
            continue
        tm = 0.5 * (ta + tb)
        out.append((math.floor(i0 + tm * (i1 - i0) + 0.5), math.floor(j0 + tm * (j1 - j0) + 0.5), seg))
    if not out:   # a track inside one pixel: its whole length (zero included)
        out.append((math.floor((i0 + i1) / 2 + 0.5), math.floor((j0 + j1) / 2 + 0.5), length))
    return out


def in_image_length(i0, j0, i1, j1, n_i, n_j):
    """length of the segment inside [-0.5, n_i - 0.5] x [-0.5, n_j - 0.5], by clipping the parameter range (Liang-Barsky)"""
    t0, t1 = 0.0, 1.0
    for a0, a1, n in ((i0, i1, n_i), (j0, j1, n_j)):
        d = a1 - a0
        if d == 0:
            if not (-0.5 <= a0 <= n - 0.5):
                return 0.0
            continue
        ta, tb = sorted(((-0.5 - a0) / d, (n - 0.5 - a0) / d))
        t0, t1 = max(t0, ta), min(t1, tb)
    return max(t1 - t0, 0.0) * math.hypot(i1 - i0, j1 - j0)


# ------------------------------------------------------------------------------------------ (e), (f) deposits
def deposit(tracks, nreads, n_i, n_j, par=PARAMS, half_band=1e-6):
    """What the rows ``tracks`` (n, 6: read, i0, j0, phi, length, dEdx) deposit with the rounded means (``poisson=0``):
    dict with "lam" (n_i, n_j) f64 summed means, "first_read" (n_i, n_j) i32 (nreads where no track passed), "added" (nreads,
    n_i, n_j) i64 electrons added up to each read, "unsure" (nreads, n_i, n_j) i64 how many of the deposits behind "added"
    have a mean within ``half_band`` of a half-integer (either rounding is then right), "hits" the number of deposits and
    "cpp_max" the largest electrons-per-pixel-length among the tracks."""
    lam = np.zeros((n_i, n_j))
    first = np.full((n_i, n_j), nreads, dtype=np.int32)
    added = np.zeros((nreads, n_i, n_j), dtype=np.int64)
    unsure = np.zeros((nreads, n_i, n_j), dtype=np.int64)
    ratio = par["pixel_depth"] / par["pixel_size"]
    hits, cpp_max = 0, 0.0
    for r, i0, j0, phi, length, dedx in np.asarray(tracks, dtype=np.float64).reshape(-1, 6):
        r = int(r)
        i1, j1 = endpoints(i0, j0, phi, length, n_i, n_j, par)
        cpp = dedx * par["pixel_size"] / par["conversion_factor"]
        cpp_max = max(cpp_max, cpp)
        for i, j, l2 in traverse(i0, j0, float(i1), float(j1)):
            if not (0 <= i < n_i and 0 <= j < n_j):
                continue
            mean = cpp * math.sqrt(ratio ** 2 + l2 ** 2)
            lam[i, j] += mean
            first[i, j] = min(first[i, j], r)
            added[r:, i, j] += int(np.rint(mean))
            unsure[r:, i, j] += int(abs(mean - math.floor(mean) - 0.5) <= half_band)
            hits += 1
    return {"lam": lam, "first_read": first, "added": added, "unsure": unsure, "hits": hits, "cpp_max": cpp_max}


# ------------------------------------------------------------------------------------------ the deposit test's tracks
def closed_form_cases(n_i, n_j, par=PARAMS):
    """[(name, (i0, j0, phi, length_um), [(i, j, l2) in the image])]: tracks whose parts are known without any traversal"""
    px = par["pixel_size"]
    r2 = math.sqrt(2.0)
    cases = [
        ("inside one pixel", (2.125, 3.25, 0.0, 0.25 * px), [(2, 3, 0.25)]),
        ("zero length", (7.25, 9.5, 1.0, 0.0), [(7, 10, 0.0)]),
        ("along a column", (3.0, 5.0, 0.0, 3.0 * px), [(3, 5, 0.5), (4, 5, 1.0), (5, 5, 1.0), (6, 5, 0.5)]),
        ("along a row", (9.0, 11.25, 0.5 * math.pi, 2.5 * px), [(9, 11, 0.25), (9, 12, 1.0), (9, 13, 1.0), (9, 14, 0.25)]),
        ("45 degrees through corners", (12.0, 20.0, 0.25 * math.pi, 3.0 * r2 * px),
         [(12, 20, r2 / 2), (13, 21, r2), (14, 22, r2), (15, 23, r2 / 2)]),
        ("leaves at i = -0.5", (1.0, 30.0, math.pi, 100.0 * px), [(1, 30, 0.5), (0, 30, 1.0)]),
        ("leaves at i = n_i + 0.5", (n_i - 2.0, 33.0, 0.0, 100.0 * px), [(n_i - 2, 33, 0.5), (n_i - 1, 33, 1.0)]),
        ("leaves at j = -0.5", (17.0, 1.0, 1.5 * math.pi, 100.0 * px), [(17, 1, 0.5), (17, 0, 1.0)]),
        ("leaves at j = n_j + 0.5", (19.0, n_j - 2.0, 0.5 * math.pi, 100.0 * px), [(19, n_j - 2, 0.5), (19, n_j - 1, 1.0)]),
    ]
    return cases


def deposit_case_tracks(n_i=24, n_j=40, nreads=6, par=PARAMS, seed=5):
    """The rows of the deposit test: the closed-form cases, a track over all the columns, two tracks through one pixel in one
    read and two in different reads, hits in read 0 and in the last read, and 40 random tracks drawn with numpy."""
    px = par["pixel_size"]
    rows = [(1 + k % (nreads - 2), *c[1], 150.0 + 10 * k) for k, c in enumerate(closed_form_cases(n_i, n_j, par))]
    rows.append((2, 21.3, 0.0, 0.5 * math.pi, (n_j + 5.0) * px, 97.0))                 # all 40 columns of row 21
    rows += [(3, 5.2, 25.1, 0.3, 2.0 * px, 200.0), (3, 5.4, 24.8, 2.0, 1.5 * px, 310.0)]   # pixel (5, 25) twice in read 3
    rows += [(1, 15.1, 5.2, 1.0, 1.2 * px, 180.0), (4, 15.3, 4.9, 4.0, 0.9 * px, 90.0)]   # pixel (15, 5) in reads 1 and 4
    rows += [(0, 22.5, 7.7, 5.0, 2.2 * px, 130.0), (nreads - 1, 10.6, 36.2, 2.5, 3.1 * px, 75.0)]   # first and last read
    rng = np.random.default_rng(seed)
    i0, j0, phi, length, dedx = sample(rng.random((40, 5)), n_i, n_j, par)
    rows += list(zip(rng.integers(0, nreads, 40), i0, j0, phi, length, dedx))
    return np.array(rows, dtype=np.float64)
