"""Plain numpy / f64 restatement of the deviates of ``csrc/pearson.hip`` (DESIGN.md "Shared device headers", row 5): the 52-bit
uniforms of ``PxRng``, its Box-Muller normal and Marsaglia-Tsang gamma, the Pearson IV rejection sampler on the angle, the
reference's classification and parameter formulas (``draw_with_tilnus.py:43-97`` and the ``solve_*`` functions, f64, operation
for operation) and the affine map of every type as ``pearson_kernel`` writes it.  Built on ``philox_ref.block``; shared by
``test_host_pearson_ref.py`` (CPU) and ``test_gpu_pearson_deviates.py`` (GPU).  Test infrastructure only.

``draw`` returns ``(x, sure)`` in the manner of ``synth_deviates_ref``: ``sure`` is False where a uniform lies within 1e-9 of
a decision of the sampler (the squeeze and the log test of the gamma, ``v <= 0``, ``|x|`` against pi/2 and the acceptance of
Pearson IV; the two log tests get 8 ulp of their largest term on top), where the device's own log / pow / cos may decide the
other way.  The branches of the Pearson IV hat (``4 u`` against 1, 2, 3) are exact in f64 on both sides and get no margin.

The normalisation of Pearson IV, ``log k``, is NOT the kernel's recurrence + Stirling series: it comes from
``scipy.special.loggamma`` of the complex argument (``mpmath.loggamma`` from m = 1000 on, where the f64 terms of ``log k`` pass
1e4 and their rounding noise 1e-12), so that the replay holds ``re_lgamma_complex`` to an independent value.

Every value function takes a backend, ``F64`` (numpy) or ``MP`` (mpmath, 40 digits, on object arrays): ``recipe_noise`` runs
the accepted candidates of a draw through both and returns the largest scaled difference, the f64 noise of the recipe itself,
from which the tests take their tolerance."""

import functools
import math

import mpmath
import numpy as np
from scipy import special, stats

from philox_ref import MASK, block

TAG_PEARSON = 0x50656172
STREAM_MUL = 0x9E3779B1
MARGIN = 1e-9                 # the band around an f64 decision (philox_ref.device_poisson's)
HALF_PI = 1.57079632679489661923
LOG2, LOGPI = 0.69314718055994530942, 1.14472988584940017414
SCIPY_LOGGAMMA_BELOW = 1000.0
MP_DIGITS = 40


# ------------------------------------------------------------------------------------------ PxRng
def uniforms(seed, elem, stream, k):
    """The k-th uniform (k = 0, 1, ...; scalar or one per element) of every element: block k // 2 of the counter {element,
    (element >> 32) ^ stream * 0x9E3779B1, block, 0x50656172}, words (3, 2) for even k and (1, 0) for odd k as (hi, lo);
    ``bits = ((hi << 32) | lo) >> 12``, ``(bits + 0.5) * 2^-52``.  Exact in f64, in (0, 1)."""
    elem, k = np.broadcast_arrays(np.asarray(elem, dtype=np.uint64), np.asarray(k, dtype=np.uint64))
    c1 = (elem >> np.uint64(32)) ^ np.uint64((int(stream) * STREAM_MUL) & MASK)
    blk = block(seed, elem, c1, k >> np.uint64(1), TAG_PEARSON)
    even = (k & np.uint64(1)) == 0
    hi = np.where(even, blk[..., 3], blk[..., 1])
    lo = np.where(even, blk[..., 2], blk[..., 0])
    bits = ((hi << np.uint64(32)) | lo) >> np.uint64(12)
    return (bits.astype(np.float64) + 0.5) * (1.0 / 4503599627370496.0)


class Stream:
    """the uniforms of a set of elements, every element counting its own"""

    def __init__(self, seed, elem, stream):
        self.seed, self.stream = int(seed), int(stream)
        self.elem = np.asarray(elem, dtype=np.uint64).ravel()
        self.k = np.zeros(self.elem.size, dtype=np.int64)

    def next(self, idx):
        u = uniforms(self.seed, self.elem[idx], self.stream, self.k[idx])
        self.k[idx] += 1
        return u


# ------------------------------------------------------------------------------------------ the two arithmetics
def _cospi2_f64(u):
    """cos(2 pi u) as cospi(2 u) gives it: the argument reduced exactly, then cos or sin of at most pi / 4"""
    t = 2.0 * np.asarray(u, dtype=np.float64)
    n = np.rint(t)
    r = np.abs(t - n)                                        # exact, in [0, 1/2]
    c = np.where(r <= 0.25, np.cos(np.pi * r), np.sin(np.pi * (0.5 - r)))
    return np.where(n.astype(np.int64) & 1, -c, c)


class F64:
    name = "f64"
    arr = staticmethod(lambda x: np.asarray(x, dtype=np.float64))
    log, exp, sqrt, cos, tan = np.log, np.exp, np.sqrt, np.cos, np.tan
    atan2, hypot, pow = np.arctan2, np.hypot, np.power
    cospi2 = staticmethod(_cospi2_f64)
    lgamma = staticmethod(special.gammaln)

    @staticmethod
    def re_lgamma_complex(x, y):
        x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
        out = np.empty(x.shape)
        for i in np.ndindex(x.shape):
            if x[i] < SCIPY_LOGGAMMA_BELOW:
                out[i] = special.loggamma(complex(x[i], y[i])).real
            else:
                with mpmath.workdps(MP_DIGITS):
                    out[i] = float(mpmath.loggamma(mpmath.mpc(float(x[i]), float(y[i]))).real)
        return out


class F64S(F64):
    """f64 throughout: scipy's loggamma at every m (what an f64 implementation of the recipe can know about log k)"""
    name = "f64, scipy loggamma"

    @staticmethod
    def re_lgamma_complex(x, y):
        return special.loggamma(np.asarray(x, dtype=np.float64) + 1j * np.asarray(y, dtype=np.float64)).real


def _mpfunc(f, nin=1):
    uf = np.frompyfunc(f, nin, 1)
    return lambda *a: uf(*a)


class MP:
    name = "mpmath"
    arr = staticmethod(lambda x: np.frompyfunc(mpmath.mpf, 1, 1)(np.asarray(x, dtype=np.float64)))
    log, exp, sqrt, cos, tan = (_mpfunc(f) for f in (mpmath.log, mpmath.exp, mpmath.sqrt, mpmath.cos, mpmath.tan))
    atan2, hypot, pow = (_mpfunc(f, 2) for f in (mpmath.atan2, mpmath.hypot, mpmath.power))
    cospi2 = staticmethod(_mpfunc(lambda u: mpmath.cospi(2 * u)))
    lgamma = staticmethod(_mpfunc(mpmath.loggamma))
    re_lgamma_complex = staticmethod(_mpfunc(lambda x, y: mpmath.loggamma(mpmath.mpc(x, y)).real, 2))


# ------------------------------------------------------------------------------------------ normal and gamma
def normal_value(B, u1, u2):
    """Box-Muller of PxRng::normal: sqrt(-2 log u1) * cospi(2 u2)"""
    return B.sqrt(-2.0 * B.log(u1)) * B.cospi2(u2)


def normal(rs, idx):
    return normal_value(F64, rs.next(idx), rs.next(idx))


def squeeze(x):
    return 1.0 - 0.0331 * (x * x) * (x * x)


def gamma_value(B, k, ub, u1, u2):
    """The candidate of PxRng::gamma(k) made from the boost uniform ``ub`` (shape below 1) and the normal's (u1, u2):
    (value, x, 1 + c x, v, d).  ``k`` f64; the uniforms in the backend's numbers."""
    k = np.asarray(k, dtype=np.float64)
    lt = k < 1.0
    inv = 1.0 / B.arr(np.where(lt, k, 1.0))
    boost = np.where(lt, B.pow(ub, inv), B.arr(np.ones(k.shape)))
    d = B.arr(np.where(lt, k + 1.0, k)) - 1.0 / 3.0
    c = 1.0 / B.sqrt(9.0 * d)
    x = normal_value(B, u1, u2)
    v1 = 1.0 + c * x
    v = v1 * v1 * v1
    return boost * d * v, x, v1, v, d


def gamma(rs, k, idx=None):
    """(value, sure, acc) of ``PxRng::gamma(k)`` for the elements ``idx`` of the stream (k one per element of idx): the boost
    uniform first where k < 1, then per attempt the normal's two uniforms and, where 1 + c x > 0, the acceptance uniform.
    ``acc`` holds the uniforms (ub, u1, u2) of the accepted candidate."""
    k = np.asarray(k, dtype=np.float64).ravel()
    idx = np.arange(k.size) if idx is None else np.asarray(idx)
    n = k.size
    lt = k < 1.0
    ub = np.full(n, 0.5)
    ub[lt] = rs.next(idx[lt])
    val, sure = np.full(n, np.nan), np.ones(n, dtype=bool)
    acc = np.full((3, n), 0.5)
    acc[0] = ub
    pending = np.isfinite(k) & (k > 0.0)
    for _attempt in range(1000):
        j = np.nonzero(pending)[0]
        if j.size == 0:
            break
        u1, u2 = rs.next(idx[j]), rs.next(idx[j])
        with np.errstate(invalid="ignore", divide="ignore"):
            value, x, v1, v, d = gamma_value(F64, k[j], ub[j], u1, u2)
        s = np.abs(v1) >= MARGIN                                   # v <= 0
        pos = v1 > 0.0
        p = np.nonzero(pos)[0]
        u = rs.next(idx[j[p]])
        xp, vp, dp = x[p], v[p], d[p]
        sq = squeeze(xp)
        s_sq = np.abs(u - sq) >= MARGIN                            # the squeeze
        acc1 = u < sq
        lhs, lv = np.log(u), np.log(vp)
        rhs = 0.5 * xp * xp + dp * (1.0 - vp + lv)
        # the log test: the device's log(u), log(v) and the sum are a few ulp of the largest term off these
        band = MARGIN + 8.0 * np.spacing(np.maximum(np.maximum(np.abs(lhs), 0.5 * xp * xp), dp * np.maximum(np.maximum(1.0, vp), np.abs(lv))))
        s_log = np.abs(lhs - rhs) >= band
        s[p] &= s_sq & (acc1 | s_log)
        ok = np.zeros(j.size, dtype=bool)
        ok[p] = acc1 | (lhs < rhs)
        sure[j] &= s
        a = j[ok]
        val[a] = value[ok]
        acc[1, a], acc[2, a] = u1[ok], u2[ok]
        pending[a] = False
    return val, sure, acc


# ------------------------------------------------------------------------------------------ Pearson IV, standard form
def p4_constants(B, m, nu):
    """(b, M, r_const, rc) of ``pearson4_std``; ``log k`` from the backend's complex loggamma"""
    m, nu = B.arr(m), B.arr(nu)
    b = 2.0 * m - 2.0
    M = B.atan2(-nu, b)
    cosM = b / B.hypot(b, nu)
    r_const = b * B.log(cosM) - nu * M
    logk = (2.0 * m - 2.0) * LOG2 + 2.0 * B.re_lgamma_complex(m, 0.5 * nu) - (LOGPI + B.lgamma(2.0 * m - 1.0))
    return b, M, r_const, B.exp(-r_const - logk)


def p4_hat(B, u):
    """(z, x, s) from the first uniform of an attempt: the four branches of the hat.  4 u, x - 2 and x - 1 are exact in f64,
    so the branches are taken in f64 for either backend."""
    x = 4.0 * np.asarray(u, dtype=np.float64)
    s = x > 2.0
    x = np.where(s, x - 2.0, x)
    tail = x > 1.0
    l = B.log(B.arr(np.where(tail, x - 1.0, 1.0)))
    return np.where(tail, l, B.arr(np.zeros(x.shape))), np.where(tail, 1.0 - l, B.arr(x)), s


def p4_angle(B, M, rc, u):
    z, x, s = p4_hat(B, u)
    return z, np.where(s, M + rc * x, M - rc * x), x


def pearson4_std(rs, m, nu, idx=None):
    """(tan of the accepted angle, sure, acc, scale) of ``pearson4_std(g, m, nu)``: per attempt one uniform for the angle and,
    where |angle| < pi / 2, one for the acceptance.  ``acc`` is the first uniform of the accepted attempt; ``scale`` the
    magnitude against which the value is compared: |tan| + (1 + tan^2) (|M| + |rc x|), the terms of the angle seen through
    the tangent's slope."""
    m, nu = (np.asarray(v, dtype=np.float64).ravel() for v in np.broadcast_arrays(m, nu))
    idx = np.arange(m.size) if idx is None else np.asarray(idx)
    n = m.size
    pairs, inv = np.unique(np.stack([m, nu], axis=1), axis=0, return_inverse=True)
    inv = np.ravel(inv)
    b, M, r_const, rc = (c[inv] for c in p4_constants(F64, pairs[:, 0], pairs[:, 1]))
    val, sure, acc, scale = np.full(n, np.nan), np.ones(n, dtype=bool), np.full(n, 0.5), np.ones(n)
    pending = np.isfinite(rc)
    for _attempt in range(10000):
        j = np.nonzero(pending)[0]
        if j.size == 0:
            break
        u = rs.next(idx[j])
        z, ang, xh = p4_angle(F64, M[j], rc[j], u)
        s = np.abs(np.abs(ang) - HALF_PI) >= MARGIN                # |x| against pi / 2
        p = np.nonzero(np.abs(ang) < HALF_PI)[0]
        jp, ap = j[p], ang[p]
        lhs = z[p] + np.log(rs.next(idx[jp]))
        t1, t2 = b[jp] * np.log(np.cos(ap)), nu[jp] * ap
        rhs = t1 - t2 - r_const[jp]
        band = MARGIN + 8.0 * np.spacing(np.maximum(np.maximum(np.abs(t1), np.abs(t2)), np.maximum(np.abs(r_const[jp]), np.abs(lhs))))
        s[p] &= np.abs(lhs - rhs) >= band                          # the acceptance
        ok = np.zeros(j.size, dtype=bool)
        ok[p] = ~(lhs > rhs)
        sure[j] &= s
        a = j[ok]
        t = np.tan(ang[ok])
        val[a], acc[a] = t, u[ok]
        scale[a] = np.abs(t) + (1.0 + t * t) * (np.abs(M[a]) + np.abs(rc[a] * xh[ok]))
        pending[a] = False
    return val, sure, acc, scale


def p4_value(B, m, nu, u):
    """tan of the angle that the first uniform ``u`` of an accepted attempt gives"""
    _b, M, _r, rc = p4_constants(B, m, nu)
    return B.tan(p4_angle(B, M, rc, u)[1])


# ------------------------------------------------------------------------------------------ classification and parameters
def classify(t21, t31, t41, I):
    """(types int32, params (n, 4)) in the layout of ``rip_stage_pearson``: the reference's f64 formulas, operation for
    operation.  Type 0 where the reference leaves the element alone or raises: outside the admissible region, type 4 with
    r <= 1 or inner <= 0, type 6 with shapes that scipy.stats.betaprime refuses (not positive, or NaN)."""
    t21, t31, t41 = float(t21), float(t31), float(t41)
    I = np.clip(np.asarray(I, dtype=np.float64).ravel(), 0.01, None)
    par = np.zeros((I.size, 4))
    with np.errstate(all="ignore"):
        t42 = 3 * t21**2
        b1 = t31**2 / (t21**3 * I)
        b2 = (t42 * I + t41) / (t21**2 * I)
        base = (b2 > 0) & (b1 >= 0) & (b2 > b1 + 1) & (b2 > 0.75 * b1)
        rhs1 = 1.5 * b1 + 3
        rhs2 = (48 + 39 * b1 + 6 * (4 + b1) ** 1.5) / (32 - b1)
        ty1, ty3 = base & (b2 < rhs1), base & (b2 == rhs1)
        ty5 = base & (b2 == rhs2) & ~ty3
        ty6 = base & (b2 > rhs1) & (b2 < rhs2)
        ty4 = base & (b2 > rhs2) & (b1 < 32)
        # type 1: analytic_u_v_from_betas, ab_from_u_v, central_moments_beta
        u = 3 * (b1 - b2 + 1) / ((b2 - 3) - 1.5 * b1)
        v = b1 * (u + 2) ** 2 / (4 * (u + 1))
        s = np.sqrt(v / (v + 4))
        ap, bp = 0.5 * u * (1 + s), 0.5 * u * (1 - s)
        cond = ap > bp if t31 < 0 else ap < bp
        a, b = np.where(cond, ap, bp), np.where(cond, bp, ap)
        var = a * b / ((a + b) ** 2 * (a + b + 1))
        par[ty1] = np.stack([a, b, a / (a + b), np.sqrt((t21 * I) / var)], axis=1)[ty1]
        # type 3
        scale = abs(t31) / (2.0 * t21)
        shape = 4.0 * t21**3 * I / t31**2
        par[ty3] = np.stack([shape, np.full(I.size, scale), shape * scale, np.full(I.size, 1.0 if t31 > 0 else -1.0)], axis=1)[ty3]
        # type 5: solve_pearson5_parameters_vec
        sq = np.sqrt(4.0 + b1)
        pp, pm = 4.0 * (1 + 2 / b1 + sq / b1), 4.0 * (1 + 2 / b1 - sq / b1)
        p = np.where(pp > 4.0, pp, pm)
        g5 = np.sqrt(t21 * I) * (p - 2) * np.sqrt(p - 3)
        par[ty5] = np.stack([p - 1.0, g5, g5 / (p - 1.0 - 1.0), np.full(I.size, 1.0 if t31 >= 0 else -1.0)], axis=1)[ty5]
        # type 6: solve_pearson6_params
        r = 6 * (b2 - b1 - 1) / (3 * b1 - 2 * b2 + 6)
        eps = r**2 / (4 + (b1 / 4) * (r + 2) ** 2 / (r + 1))
        dd = np.sqrt(r**2 - 4 * eps)
        q1, q2 = (2 - r + dd) / 2, (r - 2 + dd) / 2
        alpha, beta = q2 + 1, q1 - q2 - 1
        var1 = alpha * (alpha + beta - 1) / ((beta - 2) * (beta - 1) ** 2)
        sc = np.sqrt(t21 * I / var1)
        ok6 = (alpha > 0) & (beta > 0)
        par[ty6 & ok6] = np.stack([alpha, beta, sc, sc * (alpha / (beta - 1))], axis=1)[ty6 & ok6]
        # type 4: random_from_type4
        r = 6 * (b2 - b1 - 1) / (2 * b2 - 3 * b1 - 6)
        inner = 16 * (r - 1) - b1 * (r - 2) ** 2
        ok4 = (r > 1) & (inner > 0)
        nu = (-1.0 if t31 >= 0 else 1.0) * (r * (r - 2) * np.sqrt(b1) / np.sqrt(inner))
        a4 = np.sqrt(t21 * I * inner) / 4
        m = r / 2 + 1
        par[ty4 & ok4] = np.stack([m, nu, a4, a4 * nu / (2 * (m - 1))], axis=1)[ty4 & ok4]
    types = np.zeros(I.size, dtype=np.int32)
    for code, sel in ((1, ty1), (3, ty3), (5, ty5), (6, ty6 & ok6), (4, ty4 & ok4)):
        types[sel] = code
    return types, par


# ------------------------------------------------------------------------------------------ pearson_kernel
class Draw:
    """What ``draw`` keeps: ``x`` and ``sure``; ``types`` and ``par``; ``scale``, the sum of the magnitudes of the terms of
    the last expression of every element; ``acc``, the uniforms of the accepted candidates (``recipe_noise`` evaluates them
    again)."""


def _final(B, types, par, sgn, g):
    """the affine maps of pearson_kernel on the sampler values ``g`` (two rows: ga, gb) -> (x, scale)"""
    p0, p1, p2, p3 = (par[:, i] for i in range(4))
    x, scale = B.arr(np.zeros(types.size)), np.ones(types.size)
    ga, gb = g
    for code in (1, 3, 4, 5, 6):
        s = types == code
        if not s.any():
            continue
        if code == 1:
            frac = ga[s] / (ga[s] + gb[s])
            x[s] = p3[s] * (frac - p2[s])
            # scale: |par3| (|frac| + |mean|)
            scale[s] = np.abs(p3[s]) * (np.abs(frac) + np.abs(p2[s])).astype(np.float64)
        elif code == 3:
            x[s] = p3[s] * (p1[s] * ga[s] - p2[s])
            # scale: |scale g| + |shift|
            scale[s] = np.abs(p1[s] * ga[s]).astype(np.float64) + np.abs(p2[s])
        elif code == 4:
            x[s] = p2[s] * ga[s] + p3[s]
            # scale: |a| (|tan| + (1 + tan^2) (|M| + |rc x|)) + |lambda|; the bracket comes from pearson4_std in gb
            scale[s] = np.abs(p2[s]) * gb[s].astype(np.float64) + np.abs(p3[s])
        elif code == 5:
            x[s] = p3[s] * (p1[s] / ga[s] - p2[s])
            # scale: |b / g| + |mu|
            scale[s] = np.abs(p1[s] / ga[s]).astype(np.float64) + np.abs(p2[s])
        else:
            q = ga[s] / gb[s]
            x[s] = sgn * (p2[s] * q - p3[s])
            # scale: |scale ga / gb| + |shift|
            scale[s] = np.abs(p2[s] * q).astype(np.float64) + np.abs(p3[s])
    return x, scale


def draw(t21, t31, t41, I, seed, stream, elem=None, detail=False):
    """(x, sure) of ``rip_stage_pearson(n, I, t21, t31, t41, seed, stream, draws)``; element i of the call is ``elem[i]``
    (default 0 .. n - 1).  With ``detail`` the whole ``Draw``."""
    I = np.asarray(I, dtype=np.float64).ravel()
    n = I.size
    types, par = classify(t21, t31, t41, I)
    rs = Stream(seed, np.arange(n) if elem is None else elem, stream)
    ga, gb, sure = np.ones(n), np.ones(n), np.ones(n, dtype=bool)
    acc = np.full((2, 3, n), 0.5)
    for code in (1, 3, 5, 6):
        idx = np.nonzero(types == code)[0]
        if idx.size == 0:
            continue
        ga[idx], s, acc[0][:, idx] = gamma(rs, par[idx, 0], idx)
        sure[idx] &= s
        if code in (1, 6):
            gb[idx], s, acc[1][:, idx] = gamma(rs, par[idx, 1], idx)
            sure[idx] &= s
    idx = np.nonzero(types == 4)[0]
    if idx.size:
        ga[idx], s, acc[0][0, idx], gb[idx] = pearson4_std(rs, par[idx, 0], par[idx, 1], idx)
        sure[idx] &= s
    sgn = 1.0 if float(t31) >= 0.0 else -1.0
    with np.errstate(invalid="ignore", divide="ignore"):
        x, scale = _final(F64, types, par, sgn, (ga, gb))
    if not detail:
        return x, sure
    d = Draw()
    d.x, d.sure, d.types, d.par, d.scale, d.acc, d.sgn, d.p4_bracket = x, sure, types, par, scale, acc, sgn, gb
    return d


def recipe_noise(d, sel=None, f64_logk=False):
    """E_ref of a ``Draw``: its accepted candidates evaluated once more with mpmath at 40 digits (same uniforms, same
    parameters, same decisions) and the largest |x_f64 - x_mp| / scale over the sure draws (of ``sel``).  ``f64_logk``: the
    Pearson IV values are evaluated a third time in f64 with scipy's loggamma at every m, and their distance from the mpmath
    values counts as well: the noise of a recipe whose log k is a difference of f64 terms (``LARGE_M``)."""
    keep = d.sure & np.isfinite(d.x) & (d.types != 0)
    if sel is not None:
        mask = np.zeros(keep.size, dtype=bool)
        mask[sel] = True
        keep &= mask
    j = np.nonzero(keep)[0]
    if j.size == 0:
        return 0.0
    with mpmath.workdps(MP_DIGITS):
        types, par = d.types[j], d.par[j]
        ga, gb = MP.arr(np.ones(j.size)), MP.arr(np.ones(j.size))
        for code in (1, 3, 5, 6):
            s = types == code
            if not s.any():
                continue
            a = d.acc[0][:, j[s]]
            ga[s] = gamma_value(MP, par[s, 0], MP.arr(a[0]), MP.arr(a[1]), MP.arr(a[2]))[0]
            if code in (1, 6):
                a = d.acc[1][:, j[s]]
                gb[s] = gamma_value(MP, par[s, 1], MP.arr(a[0]), MP.arr(a[1]), MP.arr(a[2]))[0]
        s = types == 4
        if s.any():
            pairs, inv = np.unique(par[s, :2], axis=0, return_inverse=True)
            inv = np.ravel(inv)
            _b, M, _r, rc = (c[inv] for c in p4_constants(MP, pairs[:, 0], pairs[:, 1]))
            ga[s] = MP.tan(p4_angle(MP, M, rc, d.acc[0][0, j[s]])[1])
            gb[s] = MP.arr(d.p4_bracket[j[s]])
        x_mp, _scale = _final(MP, types, MP.arr(par), d.sgn, (ga, gb))
        diff = np.array([float(abs(mpmath.mpf(float(a)) - b)) for a, b in zip(d.x[j], x_mp)])
        if f64_logk and s.any():
            t = p4_value(F64S, par[s, 0], par[s, 1], d.acc[0][0, j[s]])
            xs = par[s, 2] * t + par[s, 3]
            diff[s] = np.maximum(diff[s], [float(abs(mpmath.mpf(float(a)) - b)) for a, b in zip(xs, x_mp[s])])
    return float(np.max(diff / d.scale[j]))


# ------------------------------------------------------------------------------------------ the analytic laws
def _p4_angle_cdf(m, nu, npts=400001):
    """(theta grid, cdf on it) of the density ~ cos^(2m-2) theta exp(-nu theta) on (-pi/2, pi/2): evaluated in logs relative
    to its mode atan2(-nu, 2m - 2), integrated by the trapezoid rule on +-40 widths (1 / sqrt(-second derivative) =
    cos M / sqrt(2m - 2)) around the mode and normalised numerically -- no gamma function"""
    b = 2.0 * m - 2.0
    M = math.atan2(-nu, b)
    w = math.cos(M) / math.sqrt(b)
    th = np.linspace(max(-HALF_PI, M - 40.0 * w), min(HALF_PI, M + 40.0 * w), npts)
    with np.errstate(divide="ignore"):
        logf = b * (np.log(np.cos(th)) - math.log(math.cos(M))) - nu * (th - M)
    f = np.exp(logf)
    f[~np.isfinite(f)] = 0.0
    c = np.concatenate([[0.0], np.cumsum(0.5 * (f[1:] + f[:-1]) * np.diff(th))])
    return th, c / c[-1]


def analytic_cdf(ptype, par, sgn):
    """F(x) of the deviate of one element of type ``ptype`` with the parameters ``par`` (layout of rip_stage_pearson; ``sgn``
    = +1 where tilnu_31 >= 0, used by type 6), from scipy.stats' beta, gamma, invgamma and betaprime; Pearson IV by numerical
    integration on the angle"""
    p0, p1, p2, p3 = (float(v) for v in par)

    def signed(dist, y_of_x, sign):
        return (lambda x: dist.cdf(y_of_x(x))) if sign > 0 else (lambda x: dist.sf(y_of_x(-x)))

    if ptype == 1:
        return lambda x: stats.beta.cdf(x / p3 + p2, p0, p1)
    if ptype == 3:              # x = sign (scale g - shift)
        return signed(stats.gamma(p0), lambda x: (x + p2) / p1, p3)
    if ptype == 5:              # x = sign (b / g - mu)
        return signed(stats.invgamma(p0, scale=p1), lambda x: x + p2, p3)
    if ptype == 6:              # x = sgn (scale ga / gb - shift)
        return signed(stats.betaprime(p0, p1), lambda x: (x + p3) / p2, sgn)
    if ptype == 4:              # x = a tan(theta) + lambda
        th, c = _p4_angle_cdf(p0, p1)
        return lambda x: np.interp(np.arctan((x - p3) / p2), th, c, left=0.0, right=1.0)
    raise ValueError("no law for type %r" % (ptype,))


def ks_sqrt_n(x, cdf, delta=0.0):
    """sqrt(n) D of the sample ``x`` against ``cdf``.  ``delta``: half-width of the rounding of x (one f64 value stands for
    every real number that rounds to it: where the law piles mass of several per cent inside a single rounding interval, as
    the beta of shape 1e-3 does at its lower end, the empirical step is compared with F at the ends of the interval)."""
    x = np.sort(np.asarray(x, dtype=np.float64))
    n = x.size
    i = np.arange(1, n + 1)
    d = max(np.max(i / n - cdf(x + delta)), np.max(cdf(x - delta) - (i - 1) / n))
    return math.sqrt(n) * d


# ------------------------------------------------------------------------------------------ the cases of the tests
SEED = 0x9E3779B97F4A7C15     # both halves non-zero (test_gpu_deviates.SEED)
STREAMS = (7, 7 + (1 << 28))  # stream * 0x9E3779B1 mod 2^32 of the two differ by 2^28: in the four high bits only
N_REPLAY, N_LAW = 4133, 200000
SHARE_LEFT_OUT = 1e-3         # at most 0.1 % of the draws of a case may be unsure
TOL_CAP = 1e-10               # 8 E_ref of every replay case stays below this: an error of 1e-9 in log k is seen

# one row per branch of the sampler: (golden case, intensity)
ROWS = [
    ("light_tail", 50.0),                                   # type 1, both shapes > 1
    ("poisson_like", 0.3), ("poisson_like", 0.01),          # type 1, shapes < 1: the boost, pow underflowing to 0
    ("neg_skew", 20.0),                                     # type 1, a and b swapped for negative skew
    ("gamma", 0.25), ("gamma", 100.0), ("gamma_neg", 16.0),  # type 3: shape < 1 and > 1, sign
    ("inv_gamma", 5.0), ("inv_gamma_neg", 5.0),             # type 5
    ("beta_prime", 30.0), ("beta_prime_neg", 60.0),         # type 6, sign
    ("heavy_tail", 40.0), ("heavy_tail_neg", 80.0),         # type 4, nu of both signs
    ("symmetric", 25.0), ("symmetric", 0.01),               # type 4, nu = 0; m = 2.5 (ten steps of the device's recurrence)
    ("heavy_tail", 1e5),                                    # type 4, m = 4.8e5: cancellation in log k
]
ROW_TYPES = [1, 1, 1, 1, 3, 3, 3, 5, 5, 6, 6, 4, 4, 4, 4, 4]
# log k of this row is a difference of f64 terms near 1e7 (half an ulp of them: 1e-9) on the device as in any f64 evaluation:
# by its nature the row cannot be held to TOL_CAP.  Its E_ref counts the f64 evaluation of log k (recipe_noise(f64_logk=True));
# the restatement itself draws with mpmath's log k.
LARGE_M = ("heavy_tail", 1e5)


def row_id(row):
    return "%s-%g" % row


def moment_ratios(goldens, name):
    """(t21, t31, t41) of a golden case; ``goldens``: the dicts of pearson_params and pearson_edges"""
    for g in goldens:
        if f"cl_{name}_t" in g:
            return tuple(float(v) for v in g[f"cl_{name}_t"])
    raise KeyError(name)


def rounding_width(ptype, par, xmax):
    """8 ulp of the largest term of the last expression at |x| = xmax: the ``delta`` of ``ks_sqrt_n``"""
    shift = {1: abs(par[3] * par[2]), 3: abs(par[2]), 4: abs(par[3]), 5: abs(par[2]), 6: abs(par[3])}[int(ptype)]
    return 8.0 * float(np.spacing(shift + xmax))


@functools.lru_cache(maxsize=None)
def replay_case(row, stream):
    """The ``Draw`` of a row of the table as the replay takes it (N_REPLAY elements of one intensity, SEED), with ``e_ref``
    (``recipe_noise``).  Computed once a process; callers leave it unchanged."""
    from conftest import load_golden

    name, I = row
    t = moment_ratios((load_golden("pearson_params"), load_golden("pearson_edges")), name)
    d = draw(*t, np.full(N_REPLAY, I), SEED, stream, detail=True)
    d.t, d.I = t, I
    d.e_ref = recipe_noise(d, f64_logk=(row == LARGE_M))
    return d


@functools.lru_cache(maxsize=None)
def tolerance(row):
    """tol of |got - want| <= tol * scale: 8 E_ref, E_ref the largest of the rows of the same Pearson type and both streams
    (the device's f64 log, pow, cospi, cos, tan, atan2, exp and lgamma are good to a few ulp where numpy's are within one).
    The large-m row is on its own: its E_ref is its own, and it does not count towards type 4's."""
    if row == LARGE_M:
        rows = [row]
    else:
        rows = [r for r, ty in zip(ROWS, ROW_TYPES) if ty == ROW_TYPES[ROWS.index(row)] and r != LARGE_M]
    return 8.0 * max(replay_case(r, stream).e_ref for r in rows for stream in STREAMS)
