"""numpy restatement of csrc/noisestat.hip and of calfiles/noisestack.py: the integer accumulators and row sums of a dark exposure
(``add``), the f64 moment tables in exposure order (``tables_add``), the per-pixel planes operation by operation (``planes``) and
the noise parameters (``params``), working from cubes directly.  ``make_darks`` is a small generator of raw dark frames after
the noise model of the reference's ``from_sim/sim_to_isim.py`` :340-399 with single-read groups: bias, reset noise, dark current,
white read noise, ``u_pink`` / ``c_pink`` 1/f noise with the flip of the odd channels, the reference output's terms -- and
alternating column noise, added before the samples are rounded.  The estimator is that generator's inverse."""

import numpy as np

MAX_SCALE = 6
G = 8.0 * np.log(2.0)
PLANES = ("DARK1", "DARK1ERR", "DARK2", "DARK2ERR", "CDS", "RESET")
ACC = (("a0", np.uint32), ("a1", np.uint64), ("b0", np.int32), ("b1", np.uint64), ("s0", np.int64), ("s1", np.uint64),
       ("c0", np.int32), ("c1", np.uint64))
TABLES = ("h1", "h2", "t1", "t2", "ht", "q1", "q2")


def scales(ny):
    """J = min(6, floor(log2(ny / 64)))"""
    J = 0
    while 64 << (J + 1) <= ny and J < MAX_SCALE:
        J += 1
    return J if ny >= 128 else -1


def new_acc(ny, C, cw, ref_out):
    acc = {k: np.zeros((ny, (C + bool(ref_out)) * cw), t) for k, t in ACC}
    acc["m33"] = np.zeros((ny, cw), np.uint32) if ref_out else None
    return acc


def add(acc, cube, C, cw, ref_out, f0, n):
    """one exposure (nreads, ny, width) of uint16 samples into ``acc``; returns its row sums (n, ny, nch, 2) uint32"""
    nch = C + bool(ref_out)
    x = cube[f0:f0 + n, :, :nch * cw].astype(np.int64)
    d = x[1:] - x[:-1]
    S = np.zeros(x.shape[1:], np.int64)
    for i in range(n):
        S += (2 * i - (n - 1)) * x[i]
    for key, v in (("a0", x[0]), ("a1", x[0] ** 2), ("b0", d[0]), ("b1", d[0] ** 2), ("s0", S), ("s1", S ** 2), ("c0", x[-1] - x[0]),
                   ("c1", (d ** 2).sum(0))):
        assert v.min() >= 0 or key in ("b0", "s0", "c0")
        acc[key] += v.astype(acc[key].dtype)
    if ref_out:
        acc["m33"] += x[:, :, C * cw:].sum(0).astype(np.uint32)
    ny = x.shape[1]
    return x.reshape(n, ny, nch, cw // 2, 2).sum(3).astype(np.uint32)


def new_tables(n, ny, C, ref_out):
    nch, J = C + bool(ref_out), scales(ny)
    nbt = sum(ny >> (j + 1) for j in range(J + 1))
    t = {"h1": (n - 1, nbt, nch), "h2": (n - 1, nbt, nch), "t1": (n - 1, nbt), "t2": (n - 1, nbt), "ht": (n - 1, nbt), "q1": (n - 1, nch),
         "q2": (n - 1, nch)}
    return {k: np.zeros(s) if (k != "ht" or ref_out) else None for k, s in t.items()}


def haar(rowsum, C):
    """(H (n-1, nbt, nch), T (n-1, nbt), Q (n-1, nch)) of one exposure's row sums, int64"""
    rs = rowsum.astype(np.int64)
    n, ny, nch, _ = rs.shape
    D = rs[1:].sum(-1) - rs[:-1].sum(-1)
    parts = []
    for j in range(scales(ny) + 1):
        w, nb = 1 << j, ny >> (j + 1)
        blocks = D[:, :nb * 2 * w].reshape(n - 1, nb, 2, w, nch).sum(3)
        parts.append(blocks[:, :, 0] - blocks[:, :, 1])
    H = np.concatenate(parts, axis=1)
    Q = ((rs[1:, :, :, 0] - rs[:-1, :, :, 0]) - (rs[1:, :, :, 1] - rs[:-1, :, :, 1])).sum(1)
    return H, H[:, :, :C].sum(-1), Q


def tables_add(tab, rowsum, C):
    """what rip_cal_noise_rowstats adds for one exposure: every term f64(int) * f64(int), added with one rounding"""
    H, T, Q = (a.astype(np.float64) for a in haar(rowsum, C))
    tab["h1"] = tab["h1"] + H
    tab["h2"] = tab["h2"] + H * H
    tab["t1"] = tab["t1"] + T
    tab["t2"] = tab["t2"] + T * T
    if tab["ht"] is not None:
        tab["ht"] = tab["ht"] + H[:, :, C] * T
    tab["q1"] = tab["q1"] + Q
    tab["q2"] = tab["q2"] + Q * Q


def _var(q, s, m):
    v = (q - s * s / m) / (m - 1.0)
    return np.where(v > 0.0, v, 0.0)


def planes(acc, N, n, C, cw, ref_out, tframe=3.04):
    """(planes (6, ny, C*cw) float32, amp33 (2, ny, cw) float32 or None): rip_cal_noise_planes, the same f64 operations in the same
    order, each result rounded once"""
    f = {k: acc[k].astype(np.float64) for k, _ in ACC}
    dN, ntot, nn, tframe = float(N), float(N * (n - 1)), float(n * (n * n - 1)), float(tframe)
    cds = np.sqrt(_var(f["c1"], f["c0"], ntot)).astype(np.float32)
    nx = C * cw
    sci = {k: v[:, :nx] for k, v in f.items()}
    out = np.empty((6,) + sci["a0"].shape, np.float32)
    out[0] = sci["b0"] / (dN * tframe)
    out[1] = np.sqrt(_var(sci["b1"], sci["b0"], dN) / dN) / tframe
    out[2] = (6.0 * sci["s0"]) / ((dN * nn) * tframe)
    out[3] = (6.0 * np.sqrt(_var(sci["s1"], sci["s0"], dN) / dN)) / (nn * tframe)
    out[4] = cds[:, :nx]
    out[5] = np.sqrt(_var(sci["a1"], sci["a0"], dN))
    amp33 = None
    if ref_out:
        amp33 = np.empty((2,) + acc["m33"].shape, np.float32)
        amp33[0] = acc["m33"].astype(np.float64) / (dN * float(n))
        amp33[1] = cds[:, nx:].astype(np.float64) / np.sqrt(2.0)
    return out, amp33


def _cov(sab, sa, sb, N):
    return (sab - sa * sb / N) / (N - 1.0)


def _intercept(y):
    """a of the least-squares line y_j = a + w 2^-j"""
    x = 0.5 ** np.arange(len(y))
    A = np.stack([np.ones_like(x), x], axis=1)
    return float(np.linalg.lstsq(A, np.asarray(y, float), rcond=None)[0][0])


def params(tab, N, n, ny, C, cw, vbar):
    """ACN, C_PINK, U_PINK (and M_PINK, RU_PINK where the tables hold the reference output), scale by scale"""
    N = float(N)
    J = scales(ny)
    V, X, V33, E = [], [], [], []
    at = 0
    for j in range(J + 1):
        nb, norm = ny >> (j + 1), float(cw << j)
        sl = slice(at, at + nb)
        at += nb
        varh = _cov(tab["h2"][:, sl], tab["h1"][:, sl], tab["h1"][:, sl], N) / norm ** 2      # (K, nb, nch)
        vart = _cov(tab["t2"][:, sl], tab["t1"][:, sl], tab["t1"][:, sl], N) / norm ** 2      # (K, nb)
        V.append(varh[:, :, :C].mean())
        X.append(((vart - varh[:, :, :C].sum(-1)) / (C * (C - 1))).mean() if C > 1 else 0.0)
        if tab["ht"] is not None:
            V33.append(varh[:, :, C].mean())
            E.append((_cov(tab["ht"][:, sl], tab["h1"][:, sl, C], tab["t1"][:, sl], N) / norm ** 2 / C).mean())
    V, X = np.array(V), np.array(X)
    xm = X.mean()
    out = {"C_PINK": float(np.sqrt(max(xm, 0.0) / G)), "U_PINK": float(np.sqrt(max(_intercept(V - X) / G, 0.0)))}
    if tab["ht"] is not None:
        m = float(np.mean(E) / xm) if xm > 0 else 0.0
        out["M_PINK"] = m
        out["RU_PINK"] = float(np.sqrt(max(_intercept(V33) / G - m * m * out["C_PINK"] ** 2, 0.0)))
    area = float(ny * cw)
    varq = _cov(tab["q2"][:, :C], tab["q1"][:, :C], tab["q1"][:, :C], N) * (2.0 / area) ** 2
    out["ACN"] = float(np.sqrt(max((varq.mean() - 4.0 * vbar / area) / 8.0, 0.0)))
    return out


def summarize(cubes, C, cw, ref_out, f0, n, tframe=3.04):
    """the whole restatement over a list of uint16 cubes: (acc, row sums per exposure, tables, planes, amp33, parameters)"""
    ny = cubes[0].shape[1]
    acc, tab, rows = new_acc(ny, C, cw, ref_out), new_tables(n, ny, C, ref_out), []
    for c in cubes:
        rows.append(add(acc, c, C, cw, ref_out, f0, n))
        tables_add(tab, rows[-1], C)
    N = len(cubes)
    pl, a33 = planes(acc, N, n, C, cw, ref_out, tframe)
    vbar = float(np.mean(pl[4].astype(np.float64) ** 2))
    return acc, rows, tab, pl, a33, params(tab, N, n, ny, C, cw, vbar)


# ---------------------------------------------------------------------------------------------------- the generator
def pink_frame(rng, ny, cw):
    """an (ny, cw) block of noise with S(f) = 1/f along the read-out order: the first half of a series of 2 ny cw samples"""
    m = 2 * ny * cw
    z = rng.standard_normal(2 * m)
    f = np.arange(m, dtype=np.float64)
    f[m // 2:] -= m
    amp = np.zeros(m)
    amp[1:] = 1.0 / np.sqrt(np.abs(f[1:]))
    series = np.fft.fft((z[:m] + 1j * z[m:]) * amp).real[:m // 2] / np.sqrt(2.0)
    return (series - series.mean()).reshape(ny, cw)


def make_darks(seed, N, nreads, ny, C, cw, ref_out=True, c_pink=1.5, u_pink=1.0, m_pink=0.8, ru_pink=1.2, read=5.0, white33=4.0,
               acn=0.0, reset=20.0, bias=8000.0, dark=1.5, med33=6000.0):
    """N dark exposures (nreads, ny, (C + ref_out) * cw) uint16: per exposure a reset offset per pixel, per frame the dark signal
    ``dark`` DN/frame, white noise ``read``, per channel ``u_pink`` 1/f noise plus the frame's common ``c_pink`` 1/f noise (odd
    channels read backwards), alternating column noise of amplitude ``acn`` (+a on even, -a on odd columns, a ~ N(0, acn^2) per
    channel and frame), and in the reference output ``med33`` + white ``white33`` + ``ru_pink`` 1/f + ``m_pink`` x the common noise."""
    rng = np.random.default_rng(seed)
    nch = C + bool(ref_out)
    sign = np.where(np.arange(cw) % 2 == 0, 1.0, -1.0)
    cubes = []
    for _ in range(N):
        base = bias + reset * rng.standard_normal((ny, C * cw))
        cube = np.empty((nreads, ny, nch * cw), np.uint16)
        for i in range(nreads):
            fr = np.empty((ny, nch * cw))
            fr[:, :C * cw] = base + dark * i + read * rng.standard_normal((ny, C * cw))
            common = c_pink * pink_frame(rng, ny, cw)
            for ch in range(C):
                p = u_pink * pink_frame(rng, ny, cw) + common
                fr[:, ch * cw:(ch + 1) * cw] += (p[:, ::-1] if ch % 2 else p) + acn * rng.standard_normal() * sign
            if ref_out:
                fr[:, C * cw:] = med33 + white33 * rng.standard_normal((ny, cw)) + ru_pink * pink_frame(rng, ny, cw) + m_pink * common
            cube[i] = np.clip(np.round(fr), 0, 65535).astype(np.uint16)
        cubes.append(cube)
    return cubes


# ---------------------------------------------------------------------------------------------------- the round-trip case
PLANTED = {"C_PINK": 1.5, "U_PINK": 1.0, "M_PINK": 0.8, "RU_PINK": 1.2}
ACN, ACN_TOL = 0.6, 0.0625   # 4 x the standard deviation of the restatement's ACN over six seeds (profiles/noise_run.txt)
CASE = dict(seed=1, N=16, nreads=8, ny=256, C=8, cw=16)
_MADE = {}


def round_trip_case():
    """(cubes, ``summarize`` of them) of the round-trip case, made once and shared by the host and the device tests"""
    if not _MADE:
        c = CASE
        cubes = make_darks(c["seed"], c["N"], c["nreads"], c["ny"], c["C"], c["cw"], ref_out=True, acn=ACN, read=5.0, white33=4.0,
                           **{k.lower(): v for k, v in PLANTED.items()})
        _MADE["cubes"], _MADE["sum"] = cubes, summarize(cubes, c["C"], c["cw"], True, 0, c["nreads"])
    return _MADE["cubes"], _MADE["sum"]
