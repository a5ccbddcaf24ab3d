"""Seeded inputs at the edges of the Level-1 synthesis arithmetic (synth.hip: reset_kernel, resultants_kernel,
zero_border_kernel, fill_kernel, amp33_kernel, extract_ref_kernel; invlin.hip: invlin_kernel) with their expectations from
oracle/l1sim.py and oracle/linearity.py -- numpy, every deviate handed in.  numpy only; used by test_gpu_synth_edges.py (the
kernels against these expectations, bit for bit) and by test_host_synth_edge_cases.py (the cases hold what they claim).

Every case is built once per process and shared read-only (its arrays are not writable)."""

import functools

import numpy as np

from oracle import l1sim, linearity
from romanimpreprocess_amd import synth

F4, F8 = np.float32, np.float64
READ_TIME = 3.04
PATTERN_ONE = [[0], [1]]                                          # groups of one read
PATTERN_FIVE = [[0], [1, 2], [3, 4, 5], [6, 7, 8, 9], [10]]       # uneven: 1, 2, 3, 4, 1 reads
PATTERNS = {"one": PATTERN_ONE, "five": PATTERN_FIVE, "six": synth.READ_PATTERN_6}
GARBAGE = 0xA5A5    # what the output buffers hold before a call


def border_rule(nyc):
    """the border oracle.linearity.il_apply cuts the full-frame linearity arrays by, from the active height"""
    return (8192 - nyc // 2) % 16


def freeze(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def make_cal(ny, nx, nb, rp, nplanes, gain_dtype=F4, ipc_dtype=F4, with_biascorr=True, seed=77, bias_amplitude=1.5):
    """synth.make_caldir with `nplanes` coefficient planes (2: planes 0..1 of a p_order = 2 set, a linear series);
    ipc_dtype None: no ipc4d"""
    cal = synth.make_caldir(ny, nx, read_pattern=rp, p_order=max(nplanes - 1, 2), seed=seed, gain_dtype=gain_dtype,
                            ipc_dtype=ipc_dtype or F4, nb=nb, with_biascorr=with_biascorr, bias_amplitude=bias_amplitude)
    if ipc_dtype is None:
        del cal["ipc4d"]
    lin = cal["linearitylegendre"]
    lin["data"] = np.ascontiguousarray(lin["data"][:nplanes])
    assert lin["data"].shape[0] == nplanes
    return cal


def ordinary_ramps(rng, rp, nya, nxa):
    """(counts f4, reads_e i4 (nreads, nya, nxa), normals_reset, normals_read): binomial ramps of 100 .. 40000 electrons"""
    counts = rng.poisson(rng.uniform(100, 40000, size=(nya, nxa))).astype(F4)
    tij = l1sim.read_pattern_to_tij(rp, READ_TIME)
    reads_e = l1sim.binomial_shares(counts, tij, rng)
    n_reset = rng.standard_normal((nya, nxa)).astype(F4)
    n_read = rng.standard_normal((len(rp), nya, nxa)).astype(F4)
    return counts, reads_e, n_reset, n_read


# ---- 2. rip_synth_resultants: instantiations and geometry ------------------------------------------------------------------------
# (ny, nx, nb): 32 active columns (narrower than a workgroup); odd rows, 264 active columns (a full workgroup and one of 8 lanes);
# a border of 2; no border
GEOMETRIES = ((32, 40, 4), (33, 272, 4), (32, 264, 2), (32, 520, 0))


def _res_table():
    pairs = ((F8, F8), (F4, F4), (F8, F4), (F4, F8))   # (gain, ipc4d)
    pats = ("one", "five", "six")
    rows = []
    for n in range(2, 18):
        k = n - 2
        g, kd = (F8, F8) if n == 17 else pairs[k % 4]
        rows.append((n, g, kd, (k // 4 + k) % 4, pats[k % 3], (k // 2) % 2 == 0))
    rows.append((5, F4, None, 1, "five", False))    # null ipc4d
    rows.append((12, F8, None, 3, "six", True))
    return tuple(rows)


# (coefficient planes, gain dtype, ipc4d dtype or None, index into GEOMETRIES, key of PATTERNS, with biascorr)
RES_TABLE = _res_table()


def res_id(i):
    n, g, k, geom, pat, bias = RES_TABLE[i]
    ny, nx, nb = GEOMETRIES[geom]
    return (f"np{n}-g{np.dtype(g).itemsize * 8}-k{np.dtype(k).itemsize * 8 if k else 'none'}-{ny}x{nx}b{nb}-{pat}-"
            f"{'bias' if bias else 'nobias'}")


@functools.lru_cache(maxsize=None)
def resultants_case(i):
    n, gdt, kdt, geom, pat, bias = RES_TABLE[i]
    ny, nx, nb = GEOMETRIES[geom]
    rp = PATTERNS[pat]
    cal = make_cal(ny, nx, nb, rp, n, gdt, kdt, with_biascorr=bias, seed=300 + i)
    rng = np.random.default_rng(500 + i)
    counts, reads_e, n_reset, n_read = ordinary_ramps(rng, rp, ny - 2 * nb, nx - 2 * nb)
    want, start, pre = l1sim.make_l1_fullcal(counts, rp, cal, READ_TIME, n_reset, reads_e, n_read, nb=nb, unrounded=True)
    return freeze({"cal": cal, "rp": rp, "ny": ny, "nx": nx, "nb": nb, "reads_e": reads_e, "n_reset": n_reset, "n_read": n_read,
                   "want": want, "start": start, "pre": pre, "cube": l1sim.embed(want, ny, nx, nb=nb)})


# ---- 3. planted read sequences: the warm bisection against cold evaluation -------------------------------------------------------
WARM_FRAME = (32, 272, 4)     # 24 x 264 active pixels: four full waves and one of 8 lanes in a row
WARM_ROW, WARM_COL0, WARM_STRIDE = 10, 6, 13
WARM_KINDS = ("constant", "plus_one") + tuple(f"jump_{r}" for r in range(1, 11)) + \
             ("fall_back", "zeros", "full", "negative", "alternate")
# (gain dtype, ipc4d dtype or None, coefficient planes)
WARM_VARIANTS = ((F4, F4, 9), (F8, None, 4), (F8, F8, 17))
FULL = 2 * 10**9


def planted_sequence(kind, nreads=11):
    """electrons up to every read, i4"""
    r = np.arange(nreads)
    if kind == "constant":
        seq = np.full(nreads, 30000)
    elif kind == "plus_one":
        seq = 20000 + r
    elif kind.startswith("jump_"):
        seq = 1000 * r + 300000 * (r >= int(kind[5:]))
    elif kind == "fall_back":
        seq = 5000 + 100 * r + 300000 * (r == 5)
    elif kind == "zeros":
        seq = 0 * r
    elif kind == "full":
        seq = np.full(nreads, FULL)
    elif kind == "negative":
        seq = np.full(nreads, -50000)
    elif kind == "alternate":
        seq = np.where(r % 2 == 0, 0, FULL)
    else:
        raise KeyError(kind)
    return seq.astype(np.int32)


def warm_plants():
    """[(kind, row, column)] in active coordinates: every kind along WARM_ROW, 13 columns apart (so every wave of the row mixes
    planted and ordinary lanes), and two more in the workgroup of 8 lanes.  A "constant" pixel stands in a 3 x 3 block of
    constant pixels: with an ipc4d its neighbours enter its target, which must not move either."""
    plants = [(k, WARM_ROW, WARM_COL0 + WARM_STRIDE * i) for i, k in enumerate(WARM_KINDS)]
    return plants + [("constant", 14, 259), ("alternate", WARM_ROW, 262)]


@functools.lru_cache(maxsize=None)
def warm_case(v):
    gdt, kdt, n = WARM_VARIANTS[v]
    ny, nx, nb = WARM_FRAME
    rp = PATTERN_FIVE
    cal = make_cal(ny, nx, nb, rp, n, gdt, kdt, seed=700 + v)
    rng = np.random.default_rng(710 + v)
    counts, reads_e, n_reset, n_read = ordinary_ramps(rng, rp, ny - 2 * nb, nx - 2 * nb)
    for kind, y, x in warm_plants():
        if kind == "constant":
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    reads_e[:, y + dy, x + dx] = 30000 + 1000 * (3 * dy + dx)
        reads_e[:, y, x] = planted_sequence(kind, reads_e.shape[0])
    want, start = l1sim.make_l1_fullcal(counts, rp, cal, READ_TIME, n_reset, reads_e, n_read, nb=nb)
    return freeze({"cal": cal, "rp": rp, "ny": ny, "nx": nx, "nb": nb, "reads_e": reads_e, "n_reset": n_reset, "n_read": n_read,
                   "want": want, "start": start, "cube": l1sim.embed(want, ny, nx, nb=nb)})


def per_read_dn(case):
    """(nreads, nya, nxa): the raw DN of every read as the oracle's model gives it, each read on its own"""
    cal = case["cal"]
    lin = cal["linearitylegendre"]
    kern = cal["ipc4d"]["data"] if "ipc4d" in cal else None
    return np.stack([linearity.il_apply(e, kern, cal["gain"]["data"], lin["data"], lin["Smin"], lin["Smax"], lin["Sref"],
                                        start_e=case["start"], electrons=True) for e in case["reads_e"]])


# ---- 4. rounding ties and the u16 clip in resultants_kernel ----------------------------------------------------------------------
TIE_FRAME = (32, 272, 4)
TIE_ROW, TIE_COLS = 6, np.arange(20, 80)            # 60 pixels of one row, in every group
CLIP_ROW, CLIP_COLS = 12, np.arange(30, 36)         # biascorr + 70000 on the even ones, - 70000 on the odd ones
BRIGHT = ((18, 40, 3.0e5), (18, 100, 1.0e6), (18, 200, 2.0e9))   # (row, column, counts)
TIE_VARIANTS = ((F4, F4, 9), (F8, F8, 5))


@functools.lru_cache(maxsize=None)
def tie_clip_case(v):
    gdt, kdt, n = TIE_VARIANTS[v]
    ny, nx, nb = TIE_FRAME
    rp = PATTERN_FIVE
    cal = make_cal(ny, nx, nb, rp, n, gdt, kdt, seed=800 + v)
    rng = np.random.default_rng(810 + v)
    nya, nxa = ny - 2 * nb, nx - 2 * nb
    counts = rng.poisson(rng.uniform(100, 40000, size=(nya, nxa))).astype(F4)
    for y, x, c in BRIGHT:
        counts[y, x] = c
    tij = l1sim.read_pattern_to_tij(rp, READ_TIME)
    reads_e = l1sim.binomial_shares(counts, tij, rng)
    n_reset = rng.standard_normal((nya, nxa)).astype(F4)
    n_read = rng.standard_normal((len(rp), nya, nxa)).astype(F4)
    bc = cal["biascorr"]["data"]
    bc[:, TIE_ROW, TIE_COLS] = 0.0
    _, _, pre0 = l1sim.make_l1_fullcal(counts, rp, cal, READ_TIME, n_reset, reads_e, n_read, nb=nb, unrounded=True)
    pre0 = pre0[:, TIE_ROW, TIE_COLS].astype(F8)
    k = 2.0 * np.floor(pre0 / 2.0) + (np.arange(TIE_COLS.size) % 2)[None]     # alternately even and odd
    bc[:, TIE_ROW, TIE_COLS] = (k + 0.5 - pre0).astype(F4)
    bc[:, CLIP_ROW, CLIP_COLS] = np.where(CLIP_COLS % 2 == 0, 70000.0, -70000.0).astype(F4)[None]
    want, start, pre = l1sim.make_l1_fullcal(counts, rp, cal, READ_TIME, n_reset, reads_e, n_read, nb=nb, unrounded=True)
    return freeze({"cal": cal, "rp": rp, "ny": ny, "nx": nx, "nb": nb, "reads_e": reads_e, "n_reset": n_reset, "n_read": n_read,
                   "want": want, "start": start, "pre": pre, "tie_k": k, "cube": l1sim.embed(want, ny, nx, nb=nb)})


# ---- 5. rip_synth_fill -----------------------------------------------------------------------------------------------------------
# (ny, nx, channel width, nb): 2 channels (L1Synth's default width), 32 channels (the fixture's layout), 3 channels, a border of 2
FILL_GEOMETRIES = ((32, 256, 128, 4), (32, 512, 16, 4), (33, 384, 128, 4), (32, 256, 128, 2))
FILL_CALLS = ("no_banding", "banding", "banding_no_amp33")
EDGE_DARKS = (-5.0, 0.5, 1.5, 2.5, 65534.5, 65535.5, 70000.0)     # the value of a border pixel before rounding and clipping
EDGE_WANT = (0, 0, 2, 2, 65534, 65535, 65535)                     # round-half-even, then the clip
AMP33_MEDS = (-1.5, -0.5, 0.4, 65535.9, 65536.2, 131073.7)        # the level of a reference-output pixel
AMP33_WANT = (65535, 0, 0, 65535, 0, 1)                           # towards zero, modulo 2^16
AMP33_ROW = 2


def edge_pixels(ny, nx, cw):
    """[(y, x, index into EDGE_DARKS)]: border pixels of row 1 in channel 0 and in channel 1 (an odd one: mirrored), and of the
    first and the last column in interior rows"""
    px = [(1, 3 + 2 * i, i) for i in range(7)] + [(1, cw + 1 + 2 * i, i) for i in range(7)]
    return px + [(10 + i, 0 if i % 2 == 0 else nx - 1, i) for i in range(7)]


def amp33_pixels():
    return [(AMP33_ROW, 1 + 2 * i, i) for i in range(len(AMP33_MEDS))]


def _frame_column(x, cw):
    ch, xc = divmod(x, cw)
    return ch, (cw - 1 - xc if ch % 2 else xc)


def fill_inputs(g):
    ny, nx, cw, nb = FILL_GEOMETRIES[g]
    rp = PATTERN_FIVE
    ngrp, nch = len(rp), nx // cw
    cal = make_cal(ny, nx, nb, rp, 4, seed=900 + g)
    rng = np.random.default_rng(910 + g)
    a33 = cal["read"]["amp33"]
    a33["med"] = np.ascontiguousarray(a33["med"][:, :cw])
    a33["std"] = np.ascontiguousarray(a33["std"][:, :cw])
    cube = rng.integers(0, 65536, size=(ngrp, ny, nx)).astype(np.uint16)
    cube[:, nb + 1, nb + 1], cube[:, nb + 1, nb + 2] = 0, 65535                 # the ends of the range in the active region too
    normals = rng.standard_normal((ngrp + 1, ny, nx)).astype(F4)
    frames = (3.0 * rng.standard_normal((ngrp, nch + 2, ny, cw))).astype(F4)
    white33 = rng.standard_normal((ngrp, ny, cw)).astype(F4)
    for y, x, i in edge_pixels(ny, nx, cw):
        ch, xs = _frame_column(x, cw)
        normals[:, y, x] = 0.0
        cal["dark"]["data"][:, y, x] = EDGE_DARKS[i]
        frames[:, 0, y, xs] = 0.0
        frames[:, 1 + ch, y, xs] = 0.0
    for y, xc, i in amp33_pixels():
        a33["med"][y, xc], a33["std"][y, xc] = AMP33_MEDS[i], 0.0
        frames[:, 0, y, xc] = 0.0
        frames[:, nch + 1, y, xc] = 0.0
    return cal, rp, cube, normals, frames, white33


def _fill_expect(cal, rp, cube, normals, frames, white33, nb, cw, with_amp33):
    ngrp, ny, _ = cube.shape
    im = cube.copy()
    amp33 = np.full((ngrp, ny, cw), GARBAGE, np.uint16) if with_amp33 else None
    l1sim.fill_in_refdata_and_1f(im, cal, l1sim.read_pattern_to_tij(rp, READ_TIME), normals, frames=frames, white33=white33,
                                 amp33=amp33, nb=nb, channelwidth=cw)
    return im, amp33


@functools.lru_cache(maxsize=None)
def fill_case(g, call):
    """`amp33_in` / `amp33_want`: None where the call hands in no reference output; without banding the reference output is
    handed in and must stay as it was"""
    ny, nx, cw, nb = FILL_GEOMETRIES[g]
    cal, rp, cube, normals, frames, white33 = fill_inputs(g)
    banding = call != "no_banding"
    with_amp33 = call != "banding_no_amp33"
    im, amp33 = _fill_expect(cal, rp, cube, normals, frames if banding else None, white33, nb, cw, with_amp33)
    return freeze({"cal": cal, "rp": rp, "ny": ny, "nx": nx, "cw": cw, "nb": nb, "banding": banding, "cube_in": cube,
                   "normals": normals, "frames": frames if banding else None, "white33": white33 if banding else None,
                   "with_amp33": with_amp33, "cube_want": im, "amp33_want": amp33})


MIRROR_STEP = 100.0   # the ramp planted along a channel's columns, per column, in units of the 1/f frames


@functools.lru_cache(maxsize=None)
def fill_mirror_case():
    """A flat exposure (every pixel 20000, no white noise) with the SAME ramp along the columns in the frames of channels 0
    and 1 and nothing in the common frame: channel 1 must come out as the mirror image of channel 0."""
    ny, nx, cw, nb = FILL_GEOMETRIES[0]
    rp = PATTERN_FIVE
    ngrp, nch = len(rp), nx // cw
    cal = make_cal(ny, nx, nb, rp, 4, seed=950)
    cal["dark"]["data"][:] = 20000.0
    cube = np.full((ngrp, ny, nx), 20000, np.uint16)
    normals = np.zeros((ngrp + 1, ny, nx), F4)
    frames = np.zeros((ngrp, nch + 2, ny, cw), F4)
    frames[:, 1:1 + nch] = (MIRROR_STEP * np.arange(cw, dtype=F4))[None, None, None, :]
    white33 = np.zeros((ngrp, ny, cw), F4)
    im, amp33 = _fill_expect(cal, rp, cube, normals, frames, white33, nb, cw, True)
    return freeze({"cal": cal, "rp": rp, "ny": ny, "nx": nx, "cw": cw, "nb": nb, "banding": True, "cube_in": cube,
                   "normals": normals, "frames": frames, "white33": white33, "with_amp33": True, "cube_want": im,
                   "amp33_want": amp33})


# ---- 6. rip_synth_extract_ref ----------------------------------------------------------------------------------------------------
EXTRACT_N = (1, 255, 256, 257, 1000)
EXTRACT_NGRP = (1, 2, 5)
EXTRACT_OFFSETS = (0, 1000, 65535)
EXTRACT_PAIRS = ((65535, 0), (0, 65535), (0, 0), (65535, 65535))   # (first resultant, every later one)


def extract_pair_of(p, n, ngrp, offset):
    """which of EXTRACT_PAIRS pixel p < 4 holds (one pixel: the pairs take turns over the cases)"""
    return p if n >= 4 else (p + ngrp + EXTRACT_OFFSETS.index(offset)) % 4


@functools.lru_cache(maxsize=None)
def extract_case(n, ngrp, offset):
    rng = np.random.default_rng([n, ngrp, offset])
    data = rng.integers(0, 65536, size=(ngrp, n)).astype(np.uint16)
    for p in range(min(n, 4)):
        first, later = EXTRACT_PAIRS[extract_pair_of(p, n, ngrp, offset)]
        data[0, p] = first
        data[1:, p] = later
    ref, rest = l1sim.extract_ref(data, offset)
    return freeze({"data": data, "ref": ref, "rest": rest})


# ---- 7. rip_stage_invlinearity ---------------------------------------------------------------------------------------------------
INVLIN_SHAPE = (7, 37)
INVLIN_ROWS = ((1, 0.0), (2, 0.5), (3, -0.5))    # (row, z): the targets of the row are the series values at z
INVLIN_INF_ROW = 4                               # + inf in its first 18 columns, - inf in the others


@functools.lru_cache(maxsize=None)
def invlin_case(nplanes, dtype):
    ny, nx = INVLIN_SHAPE
    dtype = np.dtype(dtype).type
    lin = make_cal(ny, nx, 0, PATTERN_ONE, nplanes, seed=1000 + nplanes)["linearitylegendre"]
    coefs, smin, smax = lin["data"], lin["Smin"], lin["Smax"]
    rng = np.random.default_rng(1100 + nplanes)
    target = rng.uniform(-2000.0, 70000.0, size=(ny, nx)).astype(dtype)
    for row, z0 in INVLIN_ROWS:
        phi, _ = linearity.legendre_series(np.full(nx, z0, dtype), coefs[:, row], linextrap=False)
        target[row] = phi          # f4 -> dtype: exact
    target[INVLIN_INF_ROW, :18], target[INVLIN_INF_ROW, 18:] = np.inf, -np.inf
    S, ex = linearity.invlinearity(target, coefs, smin, smax)
    lo, _ = linearity.legendre_series(np.full((ny, nx), -1.0, dtype), coefs, linextrap=False)
    hi, _ = linearity.legendre_series(np.full((ny, nx), 1.0, dtype), coefs, linextrap=False)
    return freeze({"target": target, "coefs": coefs, "Smin": smin, "Smax": smax, "S": S, "ex": ex, "phi_lo": lo, "phi_hi": hi})
