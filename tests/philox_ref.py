"""Plain numpy reference of the device generators' documented recipes (DESIGN.md "Shared device headers"): Philox-4x32-10 on
uint64 arrays and, in f64, the deviates ``csrc/noise.hip`` and ``csrc/pink.hip`` make from its blocks.  Shared by
``test_host_philox_ref.py`` (CPU: the Random123 known-answer vectors) and ``test_gpu_deviates.py`` (GPU).  Test infrastructure
only."""

import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # the round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # the Weyl increments of the key
MASK = 0xFFFFFFFF

TAG_NOISE, TAG_POIS, TAG_PTRS, TAG_PINK = 0x6E6F6973, 0x706F6973, 0x70747273, 0x70696E6B


def philox4x32(counter, key0, key1, rounds=10):
    """``counter`` (..., 4) of 32-bit words -> the block (..., 4) as uint64 (values below 2^32)."""
    c = np.array(counter, dtype=np.uint64) & np.uint64(MASK)
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = int(key0) & MASK, int(key1) & MASK
    for _ in range(rounds):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2       # 32 x 32 -> 64 bits: no overflow
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & np.uint64(MASK), n2, p0 & np.uint64(MASK)
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack([c0, c1, c2, c3], axis=-1)


def block(seed, a, b, c, d):
    """Blocks of the library's keying: key = (low, high) half of the 64-bit seed; a, b, c, d broadcast."""
    a, b, c, d = np.broadcast_arrays(*(np.asarray(x, dtype=np.uint64) & np.uint64(MASK) for x in (a, b, c, d)))
    return philox4x32(np.stack([a, b, c, d], axis=-1), seed & MASK, (seed >> 32) & MASK)


def u24(w):
    """(0, 1) uniform from the top 24 bits of a word (exact in f32, hence in f64)"""
    return ((w >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0


def box_muller(w0, w1):
    return np.sqrt(-2.0 * np.log(u24(w0))) * np.cos(2.0 * np.pi * u24(w1))


def injected_normals(seed, layer, ngrp, nact):
    """(ngrp, nact) f64: the normal of noise_inject_kernel at counter {active pixel index, group, layer, 'nois'}, words 0 and 1."""
    blk = block(seed, np.arange(nact)[None, :], np.arange(ngrp)[:, None], layer, TAG_NOISE)
    return box_muller(blk[..., 0], blk[..., 1])


# ------------------------------------------------------------------------------------------ device_poisson of noise.hip
def device_poisson(lam, seed, layer, isamp, pix, margin=1e-9):
    """(k, sure): device_poisson step for step in f64; sure = False when a uniform of this pixel lies within ``margin`` of a
    decision boundary (a step of the running cdf; vr, the 0.07 / 0.013 squeeze limits, v = us and the log test), where the
    device's exp / log / lgamma may decide the other way."""
    if not lam > 0.0:
        return 0.0, True
    if lam < 10.0:
        c = [int(x) for x in block(seed, pix, isamp, layer, TAG_POIS)]
        u = (float((c[0] << 16) | (c[1] >> 16)) + 0.5) / 281474976710656.0
        p = math.exp(-lam)
        cdf, k, sure = p, 0, True
        while True:
            sure = sure and abs(u - cdf) >= margin
            if not (u > cdf and k < 200):
                return float(k), sure
            k += 1
            p *= lam / k
            cdf += p
    slam, loglam = math.sqrt(lam), math.log(lam)
    b = 0.931 + 2.53 * slam
    a = -0.059 + 0.02483 * b
    inv_alpha = 1.1239 + 1.1328 / (b - 3.4)
    vr = 0.9277 - 3.6224 / (b - 2.0)
    sure = True
    for attempt in range(64):
        c = [int(x) for x in block(seed, pix, isamp, layer ^ (attempt << 16), TAG_PTRS)]
        u = (c[0] + 0.5) / 4294967296.0 - 0.5
        v = (c[1] + 0.5) / 4294967296.0
        us = 0.5 - abs(u)
        k = math.floor((2.0 * a / us + b) * u + lam + 0.43)
        sure = sure and abs(us - 0.07) >= margin and abs(v - vr) >= margin
        if us >= 0.07 and v <= vr:
            return float(k), sure
        sure = sure and abs(us - 0.013) >= margin and abs(v - us) >= margin
        if k < 0 or (us < 0.013 and v > us):
            continue
        lhs = math.log(v) + math.log(inv_alpha) - math.log(a / (us * us) + b)
        rhs = -lam + k * loglam - math.lgamma(k + 1.0)
        sure = sure and abs(lhs - rhs) >= margin
        if lhs <= rhs:
            return float(k), sure
    return math.floor(lam + 0.5), sure


# ------------------------------------------------------------------------------------------ the 1/f frames of pink.hip
def box_muller_64(w0, w1):
    """(a, b) of pink.hip's box_muller_64: a 40-bit uniform for the radius, the low 24 bits of w1 for the angle"""
    u1 = (((w0 << np.uint64(8)) | (w1 >> np.uint64(24))).astype(np.float64) + 0.5) / 1099511627776.0
    u2 = ((w1 & np.uint64(0xFFFFFF)).astype(np.float64) + 0.5) / 16777216.0
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)


def pink_normals(nframes, rows, width, seed, stream):
    """(nframes, 4*rows*width) f64: the deviates (n_0 .. n_{2L-1}) the device generator uses for each frame.  Counter
    {j, (j >> 32) ^ f, stream id, 'pink'} for j = 0 .. L/2: words 0, 1 make (n_j, n_{L+j}), words 2, 3 the pair at L - j
    (0 < j < L/2).  Frames come in blocks of max(1, 2^30 / (16 L)): frame F of the call has f = F mod block and the stream id
    ``stream`` + F - f (pink_fill_kernel).  Deviates the frame never uses stay 0."""
    L = 2 * rows * width
    half = L // 2
    fblock = max(1, (1 << 30) // (L * 16))
    out = np.zeros((nframes, 2 * L))
    j = np.arange(half + 1)
    inner = (j > 0) & (j < half)
    for F in range(nframes):
        f = F % fblock
        blk = block(seed, j, (j >> 32) ^ f, stream + F - f, TAG_PINK)
        a, b = box_muller_64(blk[:, 0], blk[:, 1])
        out[F, j], out[F, L + j] = a, b
        a2, b2 = box_muller_64(blk[inner, 2], blk[inner, 3])
        out[F, L - j[inner]], out[F, 2 * L - j[inner]] = a2, b2
    return out
