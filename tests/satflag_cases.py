"""Planted inputs for dq-init + saturation flagging (misc.hip: sat_exceed_kernel / sat_flags_kernel) at every edge of the kernel
pair: the four pixels of a thread, the 64-bit word of group bits, the 3 x 3 OR at the frame edges and at the seam between two
256-thread blocks, the time logic (skip, backup, stickiness), every kind of threshold, f32 cubes with non-finite samples and the
f64 read-pattern rule.  numpy only; used by test_host_satflag_cases.py (what the cases hold, and two further statements of the
rule beside oracle/saturation.py) and by test_gpu_satflag.py (the kernels against oracle/saturation.py, through rip_calibrate).

Every case is deterministic.  A seeded draw fills the cube with a quiet background far below the default threshold of 60000; a
plant first sets the whole ramp of its pixel to QUIET and then writes its samples, threshold and saturation dq.  Each plant
declares `first`: the first group >= skip in which its own pixel exceeds its own threshold while it is checked (None: never).
From the plants alone `expected_sat` states the flags of the whole case, which the restatement and the scalar loop must give.

What the device takes (and what it refuses by name), for the GPU module:
  * every frame here is accepted by the CALDIR upload (16 x 16 is its minimum) and by a ramp-fit-only call;
  * a plan needs 2 groups, and 3 with the first group excluded ("plan: 1 groups unsupported"): the cases of 2 groups run with
    exclude_first=False, and the cases of 1 group reach no kernel through rip_calibrate -- they are held to the two numpy
    statements, and the GPU module asserts that refusal by name (`runs_on_device`)."""

import math

import numpy as np

from oracle import saturation

SAT, DNU = 2, 1
NO_SAT_CHECK = 1 << 21
REFERENCE_PIXEL = 1 << 31
DEFAULT_THR = np.float32(60000.0)
QUIET = 100
FLT_MAX = np.finfo(np.float32).max
F32, F64 = np.float32, np.float64
RULE_LENS = (1, 1, 2, 3, 4, 5, 6, 1)


def plan_pattern(G):
    """consecutive reads in groups of 1, 1, 2, 3, 4, 5, 6, 1 reads (repeating): group 0 is the read 0 alone (dilution 0/0 = NaN),
    groups 1 and 7 hold one read (factor exactly 1), groups 2 to 6 hold 2 to 6 reads"""
    rp, at = [], 0
    for g in range(G):
        n = RULE_LENS[g % 8]
        rp.append(list(range(at, at + n)))
        at += n
    return rp


def footprint(ny, nx, y, x):
    """the clipped 3 x 3 neighbourhood of (y, x) as a mask"""
    m = np.zeros((ny, nx), bool)
    m[max(y - 1, 0):min(y + 2, ny), max(x - 1, 0):min(x + 2, nx)] = True
    return m


class Case:
    def __init__(self, name, ny, nx, G, dtype=np.uint16, skip=1, backups=None, rule=False, exclude_first=True, seed=0):
        self.name, self.ny, self.nx, self.G, self.dtype = name, ny, nx, G, np.dtype(dtype)
        self.skip, self.rule = skip, rule
        self.backups = tuple(sorted({0, 1, 2, max(G - 1, 0), G, G + 6})) if backups is None else tuple(backups)
        self.exclude_first = exclude_first and G >= 3     # (a plan of 2 groups cannot exclude the first)
        self.rp = plan_pattern(G)
        rng = np.random.default_rng([ny, nx, G, seed])
        bg = rng.integers(150, 2000, size=(G, ny, nx))
        self.data = bg.astype(np.uint16) if self.dtype == np.uint16 else (bg + 0.25).astype(F32)
        self.thr = np.full((ny, nx), DEFAULT_THR, F32)
        self.sdq = np.zeros((ny, nx), np.uint32)
        self.groupdq = None
        self.pixeldq = np.zeros((ny, nx), np.uint32)
        self.plants = []

    @property
    def runs_on_device(self):
        return self.G >= 2

    @property
    def read_pattern(self):
        """what the restatement gets: the pattern where the read-pattern rule is on, else None"""
        return self.rp if self.rule else None

    def plant(self, kinds, y, x, samples, first, thr=5000.0, sdq=0, where=None, alt=None):
        """samples: {group: value}.  alt: edits [(array name, index, value)] that flip the decision of an unflagged plant"""
        assert not any(p["y"] == y and p["x"] == x for p in self.plants), f"{self.name}: two plants at ({y}, {x})"
        self.data[:, y, x] = QUIET
        for g, v in samples.items():
            self.data[g, y, x] = v
        self.thr[y, x] = thr
        self.sdq[y, x] = sdq
        kinds = (kinds,) if isinstance(kinds, str) else tuple(kinds)
        self.plants.append({"kinds": kinds, "y": y, "x": x, "first": first, "where": where, "alt": alt})

    def removal(self, p):
        """the edits that take plant p out again"""
        y, x = p["y"], p["x"]
        return [("data", (slice(None), y, x), QUIET), ("thr", (y, x), DEFAULT_THR), ("sdq", (y, x), 0)]

    def edited(self, edits):
        """a copy of the case (without its plants' records) with the edits applied"""
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.data, c.thr, c.sdq = self.data.copy(), self.thr.copy(), self.sdq.copy()
        for name, idx, v in edits:
            getattr(c, name)[idx] = v
        return c

    def kinds(self):
        return {k for p in self.plants for k in p["kinds"]}


def expected_first(case):
    """per pixel the first group of the earliest plant whose footprint covers it, G where none does"""
    first = np.full((case.ny, case.nx), case.G, np.int64)
    for p in case.plants:
        if p["first"] is not None:
            m = footprint(case.ny, case.nx, p["y"], p["x"])
            first[m] = np.minimum(first[m], p["first"])
    return first


def expected_sat(case, backup):
    """(G, ny, nx) bool from the plants alone: a footprint pixel is saturated from max(skip, first - backup) on"""
    first = expected_first(case)
    g = np.arange(case.G)[:, None, None]
    return (first[None] < case.G) & (g >= np.maximum(case.skip, first[None] - backup))


def flag_host(case, backup, groupdq="case"):
    """oracle.saturation.flag_saturation on the case: (groupdq, pixeldq) with the given flags kept"""
    given = case.groupdq if isinstance(groupdq, str) else groupdq
    h = {"data": case.data, "groupdq": np.zeros(case.data.shape, np.uint8) if given is None else given.copy(),
         "pixeldq": case.pixeldq.copy()}
    with np.errstate(all="ignore"):
        saturation.flag_saturation(h, case.thr, backup=backup, skip_firstn=case.skip, n_pix_grow_sat=1, sat_dq=case.sdq,
                                   read_pattern=case.read_pattern)
    return h["groupdq"], h["pixeldq"]


# ---- positions ---------------------------------------------------------------------------------------------------------------
def position_spots(ny, nx):
    """[(y, x, where, kind)]: lone plants whose footprints do not touch (ny >= 16, nx >= 16)"""
    spots = [(0, 0, "corner", "pos_corner"), (0, nx - 1, "corner", "pos_corner"), (ny - 1, 0, "corner", "pos_corner"),
             (ny - 1, nx - 1, "corner", "pos_corner"),
             (0, 7, "edge", "pos_edge"), (ny - 1, 8, "edge", "pos_edge"), (7, 0, "edge", "pos_edge"), (8, nx - 1, "edge", "pos_edge"),
             (4, 4, "interior", "pos_interior_x0"), (4, 11, "interior", "pos_interior_x3"),
             (11, 5, "interior", "pos_interior_x1"), (11, 10, "interior", "pos_interior_x2")]
    if nx > 1024:   # the last pixel of the first 256-thread block of a row and the first pixel of the second
        spots += [(5, 1023, "interior", "pos_block_seam_1023"), (12, 1024, "interior", "pos_block_seam_1024")]
    for y, x, _, kind in spots:
        assert x % 4 == int(kind[-1]) if kind.startswith("pos_interior") else True
    return spots


def positions_case(name, ny, nx, G, skip, groups=None, **kw):
    """a lone plant on every spot, each exceeding in ONE group only (stickiness carries it on); the groups rotate through
    `groups` (default: every group from skip on).  With skip == G nothing is checked and every plant sits below skip."""
    c = Case(name, ny, nx, G, skip=skip, **kw)
    groups = [g for g in (range(skip, G) if groups is None else groups) if skip <= g < G]
    for i, (y, x, where, kind) in enumerate(position_spots(ny, nx)):
        if not groups:
            c.plant((kind, "nothing_checked"), y, x, {G - 1: 65535}, None, where=where)
            continue
        g = groups[i % len(groups)]
        kinds = [kind, f"first_at_{g}"]
        if g == skip:
            kinds.append("at_skip_only")
        if g == G - 1:
            kinds.append("last_group_only")
        c.plant(kinds, y, x, {g: 5000 + g}, g, where=where)
    if 0 < skip < G:   # exceeds in the last group below skip and never again
        c.plant("below_skip_only", 8, 8, {skip - 1: 6000}, None, alt=[("data", (skip, 8, 8), 6000)])
    return c


def pairs_case():
    """adjacent plants whose first groups differ: where the footprints overlap the earlier group wins"""
    c = Case("pairs_16x20_g8", 16, 20, 8, skip=1)
    c.plant("pair_same_thread", 5, 5, {4: 5001}, 4)
    c.plant("pair_same_thread", 5, 6, {2: 5001}, 2)
    c.plant("pair_neighbour_threads", 11, 7, {5: 5001}, 5)
    c.plant("pair_neighbour_threads", 11, 8, {3: 5001}, 3)
    c.plant("pair_rows", 4, 14, {6: 5001}, 6)
    c.plant("pair_rows", 5, 14, {2: 5001}, 2)
    c.plant("pair_diagonal_across_threads", 13, 15, {7: 5001}, 7)
    c.plant("pair_diagonal_across_threads", 14, 16, {1: 5001}, 1)
    return c


# ---- thresholds --------------------------------------------------------------------------------------------------------------
def _grid(ny=16, nx=16):
    """spots three apart: lone footprints"""
    return [(y, x) for y in range(1, ny - 1, 3) for x in range(1, nx - 1, 3)]


def thresholds_u16_case():
    c = Case("thresholds_u16", 16, 16, 4, skip=1, backups=(0, 1))
    at = iter(_grid())
    other = (1 << 20) | (1 << 11) | 1   # bits of a saturation dq that say nothing about the check

    def pair(kind, thr, hit, miss, g=2):
        """sample `hit` flags, `miss` (one unit lower) does not"""
        y, x = next(at)
        c.plant(kind, y, x, {g: hit}, g, thr=thr)
        y, x = next(at)
        c.plant(kind + "_below", y, x, {g: miss}, None, thr=thr, alt=[("data", (g, y, x), hit)])

    pair("thr_equal", 5000.0, 5000, 4999)
    pair("thr_half", 1000.5, 1001, 1000)
    pair("thr_65535", 65535.0, 65535, 65534, g=3)
    y, x = next(at)
    c.data[:, y, x] = 0    # (set again by plant; the samples are 0 everywhere)
    c.plant("thr_zero", y, x, {g: 0 for g in range(4)}, 1, thr=0.0)
    y, x = next(at)
    c.plant("thr_negative", y, x, {}, 1, thr=-3.5)
    for kind, thr in (("thr_65535_5", 65535.5), ("thr_65536", 65536.0)):    # never reached by u16
        y, x = next(at)
        c.plant(kind, y, x, {2: 65535}, None, thr=thr, alt=[("thr", (y, x), 65535.0)])
    for kind, thr in (("thr_nan", np.nan), ("thr_pinf", np.inf), ("thr_ninf", -np.inf)):
        y, x = next(at)
        c.plant(kind, y, x, {1: 65535, 2: 65535, 3: 65535}, None, thr=thr, alt=[("thr", (y, x), 65535.0)])
    y, x = next(at)
    c.plant("nocheck_alone", y, x, {2: 65535}, None, thr=1000.0, sdq=NO_SAT_CHECK, alt=[("sdq", (y, x), 0)])
    y, x = next(at)
    c.plant("nocheck_with_bits", y, x, {2: 65535}, None, thr=1000.0, sdq=NO_SAT_CHECK | other, alt=[("sdq", (y, x), other)])
    y, x = next(at)
    c.plant("bits_without_nocheck", y, x, {2: 65535}, 2, thr=1000.0, sdq=other | (1 << 22) | (1 << 31))
    return c


def thresholds_f32_case():
    """the largest finite thresholds (np.isfinite draws the line at FLT_MAX), reached only by f32 data"""
    c = Case("thresholds_f32", 16, 16, 4, dtype=F32, skip=1, backups=(0, 1))
    at = iter(_grid())
    below = np.nextafter(FLT_MAX, F32(0))
    big = F32(3.401e38)
    assert F32(3.4e38) < big < below < FLT_MAX
    y, x = next(at)
    c.plant("thr_below_fltmax", y, x, {2: FLT_MAX}, 2, thr=below)
    y, x = next(at)
    c.plant("thr_below_fltmax_miss", y, x, {2: np.nextafter(below, F32(0))}, None, thr=below, alt=[("data", (2, y, x), below)])
    y, x = next(at)
    c.plant("thr_3401e38", y, x, {3: FLT_MAX}, 3, thr=big)
    y, x = next(at)
    c.plant("thr_3401e38_miss", y, x, {3: F32(3.4e38)}, None, thr=big, alt=[("data", (3, y, x), big)])
    y, x = next(at)
    c.plant("thr_fltmax", y, x, {1: FLT_MAX}, 1, thr=FLT_MAX)
    y, x = next(at)
    c.plant("thr_fltmax_miss", y, x, {1: below}, None, thr=FLT_MAX, alt=[("data", (1, y, x), FLT_MAX)])
    y, x = next(at)
    c.plant("thr_fltmax_pinf_sample", y, x, {2: np.inf}, 2, thr=FLT_MAX)
    y, x = next(at)
    c.plant("thr_neg_fltmax", y, x, {}, 1, thr=-FLT_MAX)     # checked, and every sample exceeds it
    return c


def _unchecked():
    """(name, threshold, saturation dq) of the ways a pixel is not checked"""
    return (("nan_thr", np.nan, 0), ("pinf_thr", np.inf, 0), ("ninf_thr", -np.inf, 0), ("nocheck", 1000.0, NO_SAT_CHECK))


def samples_f32_case(rule):
    """f32 cubes: non-finite, negative and large samples at checked pixels, and the same at pixels that are not checked
    (an infinite sample there must not be flagged: the comparison is masked, it does not meet a sentinel)"""
    c = Case("samples_f32_rule" if rule else "samples_f32", 16, 24, 8, dtype=F32, skip=1, backups=(0, 1), rule=rule)
    at = iter(_grid(16, 24))
    # (with the rule on: group 3 holds 3 reads, factor 5/6; group 1 one read, factor 1)
    for g in (3, 1) if rule else (3,):
        y, x = next(at)
        c.plant("f32_nan_checked", y, x, {g: np.nan}, None, thr=50000.0, alt=[("data", (g, y, x), 50000.0)])
        y, x = next(at)
        c.plant("f32_pinf_checked", y, x, {g: np.inf}, g, thr=50000.0)
        y, x = next(at)
        c.plant("f32_ninf_checked", y, x, {g: -np.inf}, None, thr=50000.0, alt=[("data", (g, y, x), 50000.0)])
        for name, thr, sdq in _unchecked():
            y, x = next(at)
            c.plant(f"f32_pinf_at_{name}", y, x, {g: np.inf}, None, thr=thr, sdq=sdq, alt=[("thr", (y, x), 50000.0), ("sdq", (y, x), 0)])
    y, x = next(at)
    c.plant("f32_nan_at_nocheck", y, x, {2: np.nan, 3: -np.inf, 4: 1e38}, None, thr=np.nan, sdq=NO_SAT_CHECK,
            alt=[("thr", (y, x), 50000.0), ("sdq", (y, x), 0)])
    if not rule:
        c.data[:, 13, :] = -20.0    # a row of negative samples under negative thresholds
        for x, (kind, v, first) in zip((1, 4, 7), (("f32_negative_hit", -5.0, 2), ("f32_negative_equal", -10.0, 2), ("f32_negative_miss", -11.0, None))):
            c.plant(kind, 13, x, {2: v}, first, thr=-10.0, alt=None if first is not None else [("data", (2, 13, x), -10.0)])
            c.data[[0, 1, 3, 4, 5, 6, 7], 13, x] = -20.0
        c.plant("f32_above_65535_hit", 13, 10, {5: 70000.0}, 5, thr=69999.5)
        c.plant("f32_above_65535_miss", 13, 13, {5: 69999.0}, None, thr=69999.5, alt=[("data", (5, 13, 13), 70000.0)])
        c.plant("f32_1e30", 13, 16, {6: 1e30}, 6, thr=65536.0)
    return c


# ---- the read-pattern rule ---------------------------------------------------------------------------------------------------
def _next_f32(v, steps):
    v = F32(v)
    for _ in range(abs(steps)):
        v = np.nextafter(v, F32(np.inf if steps > 0 else -np.inf))
    return v


def u16_product_disagreement(f):
    """(threshold T, integer sample n): n >= f64(T) * f (the rule) and n >= f32(T) * f32(f) decide differently"""
    for n in range(20000, 24000):
        for k in range(-6, 7):
            T = _next_f32(n / f, k)
            p64 = F64(T) * F64(f)
            p32 = F64(T * F32(f))
            if (n >= p64) != (n >= p32):
                return T, n, bool(n >= p64)
    raise AssertionError("no threshold found at which the f32 product decides the other way")


def rule_u16_case():
    c = Case("rule_u16", 16, 16, 8, skip=0, backups=(0, 1), rule=True)
    dil = saturation.read_pattern_dilution(c.rp)
    assert np.isnan(dil[0]) and dil[1] == 1.0 and dil[7] == 1.0 and [len(r) for r in c.rp] == list(RULE_LENS)
    at = iter(_grid())
    y, x = next(at)
    c.plant("rule_read0_alone", y, x, {0: 65535}, None, thr=1000.0, alt=[("data", (0, y, x), QUIET), ("data", (1, y, x), 65535)])
    for g in (1, 7):
        y, x = next(at)
        c.plant("rule_single_read", y, x, {g: 3000}, g, thr=3000.0)
        y, x = next(at)
        c.plant("rule_single_read_below", y, x, {g: 2999}, None, thr=3000.0, alt=[("data", (g, y, x), 3000)])
    for g in range(2, 7):
        T = F32(20000.3 + 1000.0 * g)
        n = math.ceil(F64(T) * dil[g])
        assert n - 1 < F64(T) * dil[g] <= n < F64(T)    # below the undiluted threshold: only the rule flags it
        y, x = next(at)
        c.plant(f"rule_reads_{len(c.rp[g])}", y, x, {g: n}, g, thr=T)
        y, x = next(at)
        c.plant(f"rule_reads_{len(c.rp[g])}_below", y, x, {g: n - 1}, None, thr=T, alt=[("data", (g, y, x), n)])
    T, n, hit = u16_product_disagreement(dil[2])
    y, x = next(at)
    c.plant("rule_f32_product_differs", y, x, {2: n}, 2 if hit else None, thr=T,
            alt=None if hit else [("data", (2, y, x), n + 1)])
    return c


def f32_neighbours(p64):
    """(lo, hi): the largest f32 < p64 and the smallest f32 >= p64"""
    c = F32(p64)
    if F64(c) >= p64:
        return np.nextafter(c, F32(-np.inf)), c
    return c, np.nextafter(c, F32(np.inf))


def rule_f32_case():
    """f32 cube, non-integer thresholds: samples at the two f32 neighbours of the f64 product; at least one threshold at which
    f32(T) * f32(f) lands on the other side of one of them"""
    c = Case("rule_f32", 16, 16, 8, dtype=F32, skip=1, backups=(0, 1), rule=True)
    dil = saturation.read_pattern_dilution(c.rp)
    at = iter(_grid())
    differs = 0
    for g in range(2, 7):
        for i in range(200):     # the first threshold of this group at which the f32 product would decide the other way
            T = _next_f32(30000.37 + 777.1 * g, 3 * i)
            lo, hi = f32_neighbours(F64(T) * dil[g])
            p32 = T * F32(dil[g])
            wrong = (lo >= p32) or not (hi >= p32)
            if wrong:
                break
        differs += bool(wrong)
        assert F64(lo) < F64(T) * dil[g] <= F64(hi) and np.nextafter(lo, F32(np.inf)) == hi
        kinds = [f"rule_f32cube_reads_{len(c.rp[g])}"] + (["rule_f32cube_product_differs"] if wrong else [])
        y, x = next(at)
        c.plant(kinds, y, x, {g: hi}, g, thr=T)
        y, x = next(at)
        c.plant([k + "_below" for k in kinds], y, x, {g: lo}, None, thr=T, alt=[("data", (g, y, x), hi)])
    assert differs >= 1
    for g in (1, 7):
        y, x = next(at)
        c.plant("rule_f32cube_single_read", y, x, {g: F32(3000.25)}, g, thr=3000.25)
        y, x = next(at)
        c.plant("rule_f32cube_single_read_below", y, x, {g: np.nextafter(F32(3000.25), F32(0))}, None, thr=3000.25,
                alt=[("data", (g, y, x), F32(3000.25))])
    return c


# ---- given flags -------------------------------------------------------------------------------------------------------------
GIVEN_GROUP_BITS = (1, 4, 128)
MASK_BITS = (1 << 10, 1 << 11, 1 << 12)     # DEAD, HOT, WARM


def given_flags_case(given, exclude_first):
    """the positions of a 16 x 16 frame at skip 2 under a mask pixeldq (the reference border of 4 with bit 31, bit 31 on one
    active pixel, DEAD / HOT / WARM pixels) and, where `given`, a groupdq that carries bits 1, 4 and 128 on some groups and
    SATURATED on groups below skip: on the planted pixel (4, 4), whose pixeldq gets the bit from its own plant as well, and on
    the reference pixel (2, 12), whose pixeldq the ramp fit leaves alone"""
    c = positions_case(f"given_{'groupdq' if given else 'none'}_start{int(exclude_first)}", 16, 16, 8, 2, backups=(0, 1, 7),
                       exclude_first=exclude_first, seed=5)
    y, x = np.mgrid[0:16, 0:16]
    c.pixeldq[:] = np.where((y < 4) | (y >= 12) | (x < 4) | (x >= 12), np.uint32(REFERENCE_PIXEL), np.uint32(0))
    c.pixeldq[6, 6] |= np.uint32(REFERENCE_PIXEL)
    for i, bit in enumerate(MASK_BITS):
        c.pixeldq[(3 * y + 5 * x) % 17 == i] |= np.uint32(bit)
    if given:
        g = np.arange(8)[:, None, None]
        q = np.zeros((8, 16, 16), np.uint8)
        q[(y + x + g) % 5 == 0] |= 1
        q[(3 * y + x + 2 * g) % 7 == 0] |= 4
        q[(y + 2 * x + 3 * g) % 11 == 0] |= 128
        q[0, 4, 4] |= SAT
        q[1, 4, 4] |= SAT
        q[1, 2, 12] |= SAT
        c.groupdq = q
    return c


# ---- the table ---------------------------------------------------------------------------------------------------------------
def _skips(G):
    return sorted({s for s in (0, 1, 2, G - 1, G) if 0 <= s <= G})


def build_cases():
    cases = []
    for G in (1, 2, 3):
        for skip in _skips(G):
            cases.append(positions_case(f"pos_16x16_g{G}_skip{skip}", 16, 16, G, skip))
    for skip in _skips(8):
        cases.append(positions_case(f"pos_16x20_g8_skip{skip}", 16, 20, 8, skip))
    cases.append(positions_case("pos_24x1032_g8_skip1", 24, 1032, 8, 1))
    for G in (31, 32, 33, 63, 64):
        for skip in (1, G - 1, G) + ((0,) if G == 64 else ()):
            cases.append(positions_case(f"pos_16x16_g{G}_skip{skip}", 16, 16, G, skip, groups=(skip, 30, 31, 32, 62, 63)))
    cases += [pairs_case(), thresholds_u16_case(), thresholds_f32_case(), samples_f32_case(False), samples_f32_case(True),
              rule_u16_case(), rule_f32_case()]
    cases += [given_flags_case(given, ef) for given in (True, False) for ef in (True, False)]
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return cases


_CASES = None


def cases():
    """the table, built once per process and shared: nobody writes to its arrays"""
    global _CASES
    if _CASES is None:
        _CASES = build_cases()
        for c in _CASES:
            for a in (c.data, c.thr, c.sdq, c.pixeldq, c.groupdq):
                if a is not None:
                    a.setflags(write=False)
    return _CASES


def case_names():
    return [c.name for c in cases()]


def case(name):
    return next(c for c in cases() if c.name == name)


# every class of the issue's list, by the kind a plant carries (asked of the table by test_host_satflag_cases.py)
REQUIRED_KINDS = (
    ["pos_corner", "pos_edge", "pos_interior_x0", "pos_interior_x1", "pos_interior_x2", "pos_interior_x3", "pos_block_seam_1023",
     "pos_block_seam_1024", "pair_same_thread", "pair_neighbour_threads", "below_skip_only", "at_skip_only", "last_group_only",
     "nothing_checked", "first_at_30", "first_at_31", "first_at_32", "first_at_62", "first_at_63",
     "thr_equal", "thr_equal_below", "thr_half", "thr_half_below", "thr_zero", "thr_negative", "thr_65535", "thr_65535_below",
     "thr_65535_5", "thr_65536", "thr_nan", "thr_pinf", "thr_ninf", "nocheck_alone", "nocheck_with_bits", "bits_without_nocheck",
     "thr_below_fltmax", "thr_3401e38", "f32_nan_checked", "f32_pinf_checked", "f32_ninf_checked", "f32_negative_hit",
     "f32_negative_miss", "f32_above_65535_hit", "f32_above_65535_miss", "f32_nan_at_nocheck",
     "rule_read0_alone", "rule_single_read", "rule_single_read_below", "rule_f32_product_differs",
     "rule_f32cube_product_differs", "rule_f32cube_product_differs_below"]
    + [f"f32_pinf_at_{n}" for n, _, _ in _unchecked()]
    + [f"rule_reads_{n}{s}" for n in range(2, 7) for s in ("", "_below")]
    + [f"rule_f32cube_reads_{n}{s}" for n in range(2, 7) for s in ("", "_below")])


# ---- flat and gain preparation (misc.hip: flat_prepare_kernel, in front of the IPC deconvolution of get_flat) -----------------
NO_FLAT_FIELD, NO_GAIN_VALUE = 1 << 18, 1 << 19
FLAT_FRAMES = ((9, 11, 4), (16, 16, 4), (19, 23, 4), (12, 300, 1))    # (ny, nx, nb): one block of 256 threads exactly, and frames that are no multiple of it
_UP, _DOWN = F32(np.inf), F32(-np.inf)
_TENTH = F32(0.1)
FLAT_PLANTS = (("flat_below_tenth", np.nextafter(_TENTH, _DOWN)), ("flat_tenth", _TENTH), ("flat_nan", F32(np.nan)),
               ("flat_above_tenth", np.nextafter(_TENTH, _UP)), ("flat_below_ten", np.nextafter(F32(10), _DOWN)),
               ("flat_ten", F32(10)), ("flat_above_ten", np.nextafter(F32(10), _UP)), ("flat_zero", F32(0.0)),
               ("flat_minus_zero", F32(-0.0)), ("flat_negative", F32(-2.5)), ("flat_denormal", F32(1e-40)),
               ("flat_pinf", F32(np.inf)), ("flat_ninf", F32(-np.inf)))


def gain_plants(dtype):
    """f32: f32(0.1) and its neighbours.  f64: 0.1, f64(f32(0.1)) -- above 0.1: not flagged -- and the neighbours of 0.1"""
    if np.dtype(dtype) == np.dtype(F32):
        edge = (("gain_below_tenth", np.nextafter(_TENTH, _DOWN)), ("gain_tenth", _TENTH), ("gain_above_tenth", np.nextafter(_TENTH, _UP)))
    else:
        edge = (("gain_below_tenth", np.nextafter(F64(0.1), -np.inf)), ("gain_tenth", F64(0.1)), ("gain_f32_tenth", F64(_TENTH)),
                ("gain_above_tenth", np.nextafter(F64(0.1), np.inf)))
    return edge + (("gain_zero", 0.0), ("gain_negative", -1.5), ("gain_nan", np.nan), ("gain_pinf", np.inf))


def flat_case(ny, nx, nb, gain_dtype, ipc_dtype):
    """flat (f32), gain and ipc4d stack of a frame with the plants above in the active region, as many as it holds (the first
    three on the active region of 1 x 3, which a NaN would fill: a flagged flat, a flagged and clipped gain, f32(0.1)): on a lattice
    six apart where that fits (`isolated`: no plant within the reach of another), else closer.  The border holds sick values
    of both arrays, which must never be read.  `plants`: [(kind, y, x, value)]."""
    rng = np.random.default_rng([ny, nx, nb, np.dtype(gain_dtype).itemsize, np.dtype(ipc_dtype).itemsize])
    flat = rng.uniform(0.8, 1.2, size=(ny, nx)).astype(F32)
    gain = rng.uniform(1.4, 1.6, size=(ny, nx)).astype(gain_dtype)
    nya, nxa = ny - 2 * nb, nx - 2 * nb
    K = rng.uniform(0.01, 0.02, size=(3, 3, nya, nxa))
    K[rng.uniform(size=K.shape) < 0.03] = 0.0
    K[1, 1] = 0.94 + 0.005 * rng.normal(size=(nya, nxa))
    K = K.astype(ipc_dtype)
    fl, gn = list(FLAT_PLANTS), list(gain_plants(gain_dtype))
    want = [v for pair in zip(fl, gn) for v in pair] + fl[len(gn):] + gn[len(fl):]     # interleaved: a small frame gets both
    for s in (6, 3, 2, 1):
        spots = [(y, x) for y in range(nb, ny - nb, s) for x in range(nb, nx - nb, s)]
        if len(spots) >= len(want):
            break
    border = np.ones((ny, nx), bool)
    border[nb:ny - nb, nb:nx - nb] = False
    sick_flat = np.array([np.nan, -1.0, 0.0, np.inf, 50.0, 0.05], F32)
    sick_gain = np.array([0.0, np.nan, -np.inf, 0.05, -3.0], gain_dtype)
    flat[border] = sick_flat[np.arange(np.count_nonzero(border)) % len(sick_flat)]
    gain[border] = sick_gain[np.arange(np.count_nonzero(border)) % len(sick_gain)]
    plants = []
    for (kind, v), (y, x) in zip(want, spots):
        (flat if kind.startswith("flat") else gain)[y, x] = v
        plants.append((kind, y, x, v))
    pdq = np.where(border, np.uint32(REFERENCE_PIXEL), np.uint32(0))
    pdq[(np.add.outer(np.arange(ny), 2 * np.arange(nx)) % 9) == 0] |= np.uint32(1 << 11)
    return {"flat": flat, "gain": gain, "K": K, "nb": nb, "plants": plants, "complete": len(plants) == len(want), "isolated": s == 6,
            "border": border, "pixeldq": pdq}


def flat_plant_flags(c):
    """(ny, nx) u32 from the plants alone, by the scalar rules: NO_FLAT_FIELD where the flat is below f32(0.1) or above 10 (a
    NaN is neither), NO_GAIN_VALUE where the gain is <= 0.1 in its own dtype (a NaN is not)"""
    out = np.zeros(c["flat"].shape, np.uint32)
    tenth = float(_TENTH) if c["gain"].dtype == np.dtype(F32) else 0.1
    for kind, y, x, v in c["plants"]:
        v = float(v)
        if kind.startswith("flat") and (v < float(_TENTH) or v > 10.0):
            out[y, x] |= np.uint32(NO_FLAT_FIELD)
        if kind.startswith("gain") and v <= tenth:
            out[y, x] |= np.uint32(NO_GAIN_VALUE)
    return out
