"""Plain numpy references and input generators shared by ``test_gpu_post_edges.py`` (GPU) and ``test_host_post_refs.py``
(CPU): what the post-path kernels of ``post.hip`` compute, written out the slow way.  Test infrastructure only."""

import numpy as np

GROWTHS = (0, 1, 5, 9, 25)

# the four grown footprints as convolution kernels (maskhandling.py:82-117)
KERNELS = {
    1: np.ones((1, 1), np.int64),
    5: np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], np.int64),
    9: np.ones((3, 3), np.int64),
    25: np.ones((5, 5), np.int64),
}


# ------------------------------------------------------------------------------------------ mask growth
def footprint(shape, y, x, growth):
    """The pixels one flagged pixel at (y, x) masks under ``growth``, clipped to the frame."""
    out = np.zeros(shape, bool)
    if growth == 0:
        return out
    reach = {1: 0, 5: 1, 9: 1, 25: 2}[growth]
    for dy in range(-reach, reach + 1):
        for dx in range(-reach, reach + 1):
            if growth == 5 and abs(dy) + abs(dx) > 1:
                continue
            if 0 <= y + dy < shape[0] and 0 <= x + dx < shape[1]:
                out[y + dy, x + dx] = True
    return out


def edge_positions(shape):
    """Corners, edge middles, one pixel in from each edge and the interior of a frame (duplicates on small frames dropped)."""
    ny, nx = shape
    ys = sorted({0, 1, ny // 2, ny - 2, ny - 1} & set(range(ny)))
    xs = sorted({0, 1, nx // 2, nx - 2, nx - 1} & set(range(nx)))
    return [(y, x) for y in ys for x in xs]


def random_growth_table(rng):
    """growth[32] over all bits: every growth value appears, bit 31 is grown, and some bits carry growth 0."""
    table = rng.choice(GROWTHS, size=32)
    table[rng.permutation(31)[:10]] = (0, 0, 0, 1, 1, 5, 5, 9, 9, 25)
    table[31] = rng.choice((5, 9, 25))
    return table.astype(np.uint8)


def random_dq(rng, shape, frac=0.03):
    """~``frac`` of the pixels flagged with one random bit (so that each growth shows on its own), a tenth of those with a
    second one; every bit 0..31 occurs on the larger planes."""
    one = np.left_shift(np.uint32(1), rng.integers(0, 32, size=shape).astype(np.uint32))
    two = np.left_shift(np.uint32(1), rng.integers(0, 32, size=shape).astype(np.uint32))
    r = rng.random(shape)
    return (np.where(r < frac, one, np.uint32(0)) | np.where(r < frac / 10, two, np.uint32(0))).astype(np.uint32)


def table_dict(table):
    return {bit: int(g) for bit, g in enumerate(table)}


# ------------------------------------------------------------------------------------------ bin mean
def bin_inputs(rng, shape, masked=0.004):
    arr = (rng.standard_normal(shape) * 100 + 30).astype(np.float32)
    return arr, rng.random(shape) < masked


def bin_mean_same_order(arr, mask, k):
    """include/romanhip.h's order in float32: the k values of a block row summed left to right, the k row sums summed top to
    bottom, divided by f32(k*k); a masked pixel counts as NaN."""
    ny, nx = arr.shape
    nyo, nxo = ny // k, nx // k
    v = arr.astype(np.float32)
    if mask is not None:
        v = np.where(mask, np.float32(np.nan), v)
    v = v[:nyo * k, :nxo * k].reshape(nyo, k, nxo, k)
    s = np.zeros((nyo, nxo), np.float32)
    with np.errstate(invalid="ignore"):
        for a in range(k):
            t = np.zeros((nyo, nxo), np.float32)
            for b in range(k):
                t = t + v[:, a, :, b]
            s = s + t
        return s / np.float32(k * k)


def bin_mean_f64(arr, mask, k):
    """(block means, block means of |v|) in float64"""
    ny, nx = arr.shape
    nyo, nxo = ny // k, nx // k
    v = arr.astype(np.float64)
    if mask is not None:
        v = np.where(mask, np.nan, v)
    v = v[:nyo * k, :nxo * k].reshape(nyo, k, nxo, k)
    with np.errstate(invalid="ignore"):
        return v.mean(axis=(1, 3)), np.abs(v).mean(axis=(1, 3))


def bin_bound(meanabs, k):
    """k*k roundings of 2^-24 relative to the block's mean |v|: k*k - 1 additions and the division"""
    return k * k * 2.0 ** -24 * meanabs


BIN_CASES = [((9, 1030), 4), ((5, 300), 1), ((23, 29), 7), ((7, 523), 2), ((10, 800), 3)]


# ------------------------------------------------------------------------------------------ endslice
def endslice_loop(rdq, nb):
    """gen_cal_image.py:697-712 group by group: iend - 1 of the last group where the saturation bit rises, -1 if none."""
    G, ny, nx = rdq.shape
    sat = (rdq[:, nb:ny - nb, nb:nx - nb] & np.uint8(2)) != 0
    out = np.full(sat.shape[1:], -1, np.int8)
    for iend in range(1, G):
        out[sat[iend] & ~sat[iend - 1]] = iend - 1
    return out
