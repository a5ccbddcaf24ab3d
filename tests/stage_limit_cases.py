"""Seeded inputs at the ends of the stage kernels' domain: ramps of 17 to 64 groups, Legendre sets of 1 to 32 planes, IPC
frames whose active edge falls on tile seams and on the frame edge.  numpy only; used by test_gpu_stage_limits.py (the HIP
stage kernels against oracle/) and by test_host_stage_limits.py (the preconditions of these cases and independent checks of
the oracle at these shapes)."""

import numpy as np

import golden_cases as gc
from oracle import rampfit as orf
from romanimpreprocess_amd import synth
from romanimpreprocess_amd.dqflags import pixel

SAT, JUMP = 2, 4
NB = 4

# ---- long ramps -----------------------------------------------------------------------------------------------------------
# the last and the first count on each side of the 48 KiB steps of rampfit_kernel's (32 | 33) and jumpdetect_kernel's (48 | 49)
# dynamic LDS, the first count past the fused forms (17) and the limit RIP_MAX_GROUPS (64)
LONG_COUNTS = (17, 32, 33, 48, 49, 64)
STAIR_ROWS = slice(6, None, 3)   # rampfit_case: pixel (r, 8 + c), r in rows 6::3, first saturates at group c (c == G: never)
STAIR_COL0 = 8
PLANT_ROW = 6                    # the staircase row whose pixels get a planted step


def long_read_pattern(G):
    return [[0]] + [[1 + 2 * i, 2 + 2 * i] for i in range(G - 1)]


def long_frame(G):
    """the smallest frame that holds the whole staircase in its active region (nx >= G + 13: column 8 + G is the last active
    one) and the fixed pixels of rampfit_case (up to row 20 and column 32, active: ny >= 24 for a border of 4, nx >= 37)"""
    return 24, max(G + 13, 40)


def planted_steps(G, start):
    """[(first-saturation group c, group of the step)]: staircase pixels of PLANT_ROW that get a 3000 DN step inside the
    groups their truncated fit covers -- the longest, a middle and the shortest truncated variant, and the never-saturated
    pixel (c == G) for the full ramp"""
    return [(G, G // 2), (G - 1, G - 3), (G // 2 + 1, G // 4 + 1), (3 + start, 1 + start)]


def long_ramp_case(G, gain_dtype=np.float32, exclude_first=True):
    """golden_cases.rampfit_case on long_frame(G), with one change to its saturation staircase: on the staircase pixels the
    staircase alone decides the saturation flags (the random saturation of the frame's right half, which this narrow frame
    lays over the staircase, is taken off them), so that every group 0..G-1 is the first saturated one of some active pixel
    and column 8 + G never saturates: every truncated variant is fitted somewhere.  Plus the planted steps above.
    Returns the arrays of rampfit_case and meta (with K and nborder) as fitting.ramp_fit and oracle.rampfit take it."""
    rp = long_read_pattern(G)
    ny, nx = long_frame(G)
    start = 1 if exclude_first else 0
    c = gc.rampfit_case(rp, 900 + G, exclude_first=exclude_first, gain_dtype=gain_dtype, cr_frac=0.03, shape=(ny, nx))
    gdq = c["groupdq"]
    for col in range(G + 1):
        gdq[:, STAIR_ROWS, STAIR_COL0 + col] &= np.uint8(~SAT & 0xFF)
        gdq[col:, STAIR_ROWS, STAIR_COL0 + col] |= np.uint8(SAT)
    for first_sat, at in planted_steps(G, start):
        c["data"][at:, PLANT_ROW, STAIR_COL0 + first_sat] += np.float32(3000.0)
    meta = orf.ma_table_meta(rp, synth.FRAME_TIME)
    meta["nborder"] = NB
    meta["K"] = orf.construct_weights(0.4 / 1.8 / 6.5**2, meta, exclude_first=exclude_first)
    c["meta"], c["read_pattern"], c["exclude_first"] = meta, rp, exclude_first
    return c


def first_saturation(groupdq):
    """per pixel the first group that carries SATURATED, G where none does"""
    sat = (groupdq & SAT) != 0
    return np.where(sat.any(axis=0), np.argmax(sat, axis=0), groupdq.shape[0])


# ---- Legendre sets --------------------------------------------------------------------------------------------------------
LIN_PLANES = (1, 2, 3, 5, 31, 32)
LIN_SHAPE = (24, 40)
LIN_GROUPS = 4
PLANT_GROUPS = (0, 2)
# kind -> (which bound, intended to be in range).  "at": S is the bound itself, z = -+1 exactly.  "ulp": the next f32 beyond the
# bound; S is outside [Smin, Smax] but z, rounded, may still be -+1 (at Smin it always is: 2 ulp(Smin) / span is below half an
# ulp of 1) -- the rounding of z decides, so the intent is only that |z| stays within 2 eps of 1.  "last": the f32 farthest
# beyond the bound whose z is still -+1; "cross": its successor, the first S that is out of range.
PLANT_KINDS = ("at_min", "ulp_min", "last_min", "cross_min", "at_max", "ulp_max", "last_max", "cross_max")


def z_of(S, Smin, Smax):
    """z of oracle.linearity.multilin, in the dtype of the inputs"""
    return -1 + 2 * (S - Smin) / (Smax - Smin)


def _crossing(smin, smax, upper):
    """(last, cross): the adjacent f32 values of S beyond the bound between which |z| goes above 1"""
    toward = np.float32(np.inf if upper else -np.inf)
    s = smax if upper else smin
    for _ in range(64):
        nxt = np.nextafter(s, toward)
        if abs(z_of(nxt, smin, smax)) > 1:
            return s, nxt
        s = nxt
    raise AssertionError("no crossing within 64 ulp of the bound")


def legendre_case(nplanes, seed=None):
    """Coefficient stacks built directly (synth.make_caldir cannot make fewer than 3 planes): plane 0 ~ 3e4, plane 1 ~ 3e4,
    plane L >= 2 ~ N(0, 200 / L^2); Smin, Smax, Sref per pixel; a few pixels of lin_dq carry NO_LIN_CORR or REFERENCE_PIXEL
    (phi = S - Sref there).  The cube: LIN_GROUPS groups on LIN_SHAPE drawn in [Smin - 400, Smax + 400], plus the planted
    samples `plants`: [(group, y, x, kind)], every kind of PLANT_KINDS in every group of PLANT_GROUPS, on clean pixels."""
    ny, nx = LIN_SHAPE
    rng = np.random.default_rng(7000 + nplanes if seed is None else seed)
    coefs = np.zeros((nplanes, ny, nx), np.float32)
    coefs[0] = 3.0e4 + 300.0 * rng.normal(size=(ny, nx))
    if nplanes > 1:
        coefs[1] = 3.0e4 + 300.0 * rng.normal(size=(ny, nx))
    for L in range(2, nplanes):
        coefs[L] = (200.0 / L**2) * rng.normal(size=(ny, nx))
    Smin = (5000 + 500 * rng.uniform(size=(ny, nx))).astype(np.float32)
    Smax = (56000 + 8000 * rng.uniform(size=(ny, nx))).astype(np.float32)
    Sref = (Smin + 300 + 100 * rng.uniform(size=(ny, nx))).astype(np.float32)
    lin_dq = np.zeros((ny, nx), np.uint32)
    lin_dq[rng.uniform(size=(ny, nx)) < 0.02] |= np.uint32(pixel.NO_LIN_CORR)
    lin_dq[rng.uniform(size=(ny, nx)) < 0.02] |= np.uint32(pixel.REFERENCE_PIXEL)
    lin_dq[3, 5] |= np.uint32(pixel.NO_LIN_CORR)
    lin_dq[4, 7] |= np.uint32(pixel.REFERENCE_PIXEL)
    lin_dq[5, 9] |= np.uint32(pixel.HOT)          # a flag that does not switch the branch
    S = (Smin - 400 + (Smax - Smin + 800) * rng.uniform(size=(LIN_GROUPS, ny, nx))).astype(np.float32)
    attempt = np.where(rng.uniform(size=S.shape) < 0.8, np.uint8(2), np.uint8(0))
    clean = np.argwhere(lin_dq == 0)
    plants = []
    at = 0
    for g in PLANT_GROUPS:
        for kind in PLANT_KINDS:
            y, x = (int(v) for v in clean[7 * at + 3])
            at += 1
            upper = kind.endswith("max")
            lo, hi = Smin[y, x], Smax[y, x]
            bound = hi if upper else lo
            last, cross = _crossing(lo, hi, upper)
            S[g, y, x] = {"at": bound, "ulp": np.nextafter(bound, np.float32(np.inf if upper else -np.inf)), "last": last,
                          "cross": cross}[kind.split("_")[0]]
            attempt[g, y, x] = 2
            plants.append((g, y, x, kind))
    return {"S": S, "coefs": coefs, "Smin": Smin, "Smax": Smax, "Sref": Sref, "lin_dq": lin_dq, "attempt_corr": attempt,
            "plants": plants}


def lin_file(c):
    return {"roman": {"data": c["coefs"], "Smin": c["Smin"], "Smax": c["Smax"], "Sref": c["Sref"], "dq": c["lin_dq"]}}


# ---- IPC geometries -------------------------------------------------------------------------------------------------------
# (ny, nx, nb): where the edge of the active region falls against the 64 x 16 tiles of ipc_cube_kernel
IPC_FRAMES = (
    (16, 64, 0),     # one tile: active edge, tile edge and frame edge coincide
    (32, 128, 0),    # interior seams; the ring of the outer tiles at coordinates -1 and ny
    (17, 65, 0),     # tiles of one row and of one column
    (12, 20, 4),     # the frame is smaller than a tile
    (48, 144, 8),    # a border other than 4
    (40, 72, 15),    # the widest border the rule (8192 + (nx - nxa) // 2) % 16 allows
)
IPC_MIXED = ((32, 128, 0), (12, 20, 4))   # the frames that run every (kernel dtype) x (gain none / f32 / f64)
IPC_GROUPS = 2


def ipc_kernel_stack(nya, nxa, dtype, rng):
    """per-pixel random 3 x 3 stack: neighbours 0.01 .. 0.02 with a few exact zeros, centre ~ 0.94"""
    K = rng.uniform(0.01, 0.02, size=(3, 3, nya, nxa))
    K[rng.uniform(size=K.shape) < 0.03] = 0.0
    K[1, 1] = 0.94 + 0.005 * rng.normal(size=(nya, nxa))
    return K.astype(dtype)


def ipc_geometry_case(ny, nx, nb, kernel_dtype=np.float32, gain_dtype=None):
    """cube f32 (IPC_GROUPS, ny, nx) with the values and rare spikes of golden_cases.ipc_case, the kernel stack cut to the
    active region (oracle.ipc.border_of gives nb back), the full-frame gain in `gain_dtype` (None: no gain)"""
    code = {None: 0, np.float32: 1, np.float64: 2}[gain_dtype] + (3 if kernel_dtype == np.float64 else 0)
    rng = np.random.default_rng([ny, nx, nb, code])
    G = IPC_GROUPS
    cube = (rng.uniform(-50, 3000, size=(G, ny, nx)) + 20000 * (rng.uniform(size=(G, ny, nx)) < 0.01)).astype(np.float32)
    K = ipc_kernel_stack(ny - 2 * nb, nx - 2 * nb, kernel_dtype, rng)
    gain = None if gain_dtype is None else np.clip(1.5 + 0.03 * rng.normal(size=(ny, nx)), 1.4, 1.6).astype(gain_dtype)
    return {"cube": cube, "K": K, "gain": gain, "nb": nb}


def ipc_image_case(ny, nx, image_dtype, kernel_dtype=np.float32, gain_dtype=None):
    """one image in `image_dtype` with its (3, 3, ny, nx) stack (and gain): the operands of ipc_fwd / ipc_rev"""
    rng = np.random.default_rng([ny, nx, 77, np.dtype(image_dtype).itemsize, np.dtype(kernel_dtype).itemsize])
    img = (rng.uniform(-50, 3000, size=(ny, nx)) + 20000 * (rng.uniform(size=(ny, nx)) < 0.01)).astype(image_dtype)
    K = ipc_kernel_stack(ny, nx, kernel_dtype, rng)
    gain = None if gain_dtype is None else np.clip(1.5 + 0.03 * rng.normal(size=(ny, nx)), 1.4, 1.6).astype(gain_dtype)
    return {"image": img, "K": K, "gain": gain}


# ---- the oracle's results on the long ramps, computed once per process and shared (read-only) ---------------------------------
_FIT_CACHE = {}


def oracle_ramp_fit(G, gain64=False, exclude_first=True):
    """oracle.rampfit.ramp_fit on long_ramp_case: dict(case, slope, err_read, err_poisson, groupdq, pixeldq, seconds).  The
    arrays are shared between the tests that ask for the same case: nobody writes to them."""
    import time

    key = (G, bool(gain64), bool(exclude_first))
    if key not in _FIT_CACHE:
        c = long_ramp_case(G, np.float64 if gain64 else np.float32, exclude_first)
        rdq, pdq = c["groupdq"].copy(), c["pixeldq"].copy()
        t0 = time.perf_counter()
        with np.errstate(all="ignore"):
            s, er, ep = orf.ramp_fit(c["data"], rdq, pdq, c["gain"], c["read"], c["meta"], exclude_first)
        res = {"case": c, "slope": s, "err_read": er, "err_poisson": ep, "groupdq": rdq, "pixeldq": pdq,
               "seconds": time.perf_counter() - t0}
        for v in list(res.values()) + list(c.values()) + list(c["meta"].values()):   # gain, read and meta's K among them
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _FIT_CACHE[key] = res
    return _FIT_CACHE[key]


def new_jumps(res):
    """(G, ny, nx) bool: JUMP_DET in the oracle's group flags that the input did not carry"""
    return ((res["groupdq"] & JUMP) != 0) & ((res["case"]["groupdq"] & JUMP) == 0)


def assert_long_ramp_conditions(res, need_truncated):
    """what makes a comparison on this case mean something, asked of the ORACLE's output: every group 0..G-1 is the first
    saturated one of an active pixel and one active pixel never saturates; the oracle raised new JUMP_DET flags -- among them
    the planted step of the never-saturated staircase pixel -- and, where `need_truncated`, the planted steps inside the longest,
    a middle and the shortest truncated variant"""
    c = res["case"]
    G = c["data"].shape[0]
    start = 1 if c["exclude_first"] else 0
    act = (slice(NB, -NB), slice(NB, -NB))
    fs = first_saturation(c["groupdq"])[act]
    missing = [g for g in range(G + 1) if not np.any(fs == g)]
    assert not missing, f"no active pixel first saturates at group(s) {missing} (G = never)"
    nj = new_jumps(res)
    assert np.count_nonzero(nj[(slice(None),) + act]) > 0, "the oracle raised no new JUMP_DET"
    for first_sat, at in planted_steps(G, start):
        if first_sat < G and not need_truncated:
            continue
        assert nj[at - 1, PLANT_ROW, STAIR_COL0 + first_sat], \
            f"planted step into group {at} of the pixel that first saturates at {first_sat}: not flagged by the oracle"
