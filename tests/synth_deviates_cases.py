"""Seeds whose small-mean uniform (``synth.hip``, counter {pixel, r & ~3, 0x10, 0x706f6934}, word r & 3, >> 9) falls into an
extreme bin of the 23-bit grid: the three highest values and 0.  Found once with ``synth_deviates_ref.small_bits`` by scanning
seeds 1 .. 1199 of a 4096-pixel, 9-read call (every hit of that scan is listed); ``test_host_synth_deviates.py`` verifies each
entry, ``test_gpu_synth_deviates.py`` draws them on the device at a grid of means.  All four word positions occur, and read 8
lies in the last, partial block of four."""

# (seed, npix, nreads, pixel, read, 23-bit value)
EXTREME_BINS = (
    (256, 4096, 9, 1672, 1, 0),
    (296, 4096, 9, 1610, 8, 0x7FFFFE),
    (335, 4096, 9, 909, 3, 0x7FFFFF),
    (376, 4096, 9, 3187, 3, 0x7FFFFF),
    (414, 4096, 9, 2566, 0, 0),
    (476, 4096, 9, 1965, 7, 0),
    (525, 4096, 9, 1769, 2, 0),
    (631, 4096, 9, 605, 1, 0x7FFFFE),
    (649, 4096, 9, 1541, 6, 0x7FFFFD),
    (695, 4096, 9, 3140, 0, 0),
    (713, 4096, 9, 1724, 8, 0x7FFFFE),
    (809, 4096, 9, 532, 6, 0x7FFFFF),
    (827, 4096, 9, 2321, 6, 0x7FFFFF),
    (881, 4096, 9, 1129, 4, 0),
    (890, 4096, 9, 2837, 0, 0),
    (967, 4096, 9, 3981, 1, 0),
    (995, 4096, 9, 929, 7, 0),
)

# the means per read of the extreme-bin test: 160 values strictly inside (0.05, 9.99) -- which means an f32 running sum
# saturates at depends on the device's exponential, so the grid is dense
EXTREME_MEANS = tuple(0.05 + (9.99 - 0.05) * (j + 0.5) / 160.0 for j in range(160))

# means per read of the pinned small-mean test: 0.05 .. 3.9 are drawn by the first launch, 4.0 .. 9.99 by the deferred one
SMALL_MEANS = (0.05, 0.3, 3.9, 4.0, 4.7, 9.5, 9.99)
SMALL_NREADS = (1, 5, 9, 35)
SMALL_NPIX = (1, 255, 257, 1000)

# means per read of the rejection branch; the last is beyond the 8e6 limit of the f32 pre-test (f64 test only)
BIG_MEANS = (10.0, 10.5, 15.0, 20.0, 900.0, 1.0e5, 9.0e6)

# unequal read spacing: gaps of several sizes, a repeated time (share 0 in the middle) and two neighbouring gaps that differ by
# less than 1e-12 relative (the kernel keeps the first one's table for the second)
UNEQUAL_GAPS = (0.5, 1.0, 1.0 + 2.0 ** -41, 4.0, 0.0, 0.25, 4.0, 1.0, 0.125, 2.0)
# counts for it (the largest share is 4 / 13.875): 13 stays below 4 a read everywhere (first launch); 15 and 20 pass 4 in the two
# long reads only (deferred, sequential search); 34 peaks at 9.8; 35 and 40 cross 10 in the two long reads and come back below
# (rejection sampler and sequential search by turns in the launch of the bright pixels); 200 and 5000 are above 10 in most reads
# and below in the short ones; 0.7 is the sky
UNEQUAL_COUNTS = (13.0, 15.0, 20.0, 34.0, 35.0, 40.0, 200.0, 5000.0, 0.7)

# given totals (binomial shares): read 0 at t = 0 takes nothing, shares on both sides of 0.5 and a last share of 1
BINOMIAL_TOTALS = (0.0, 1.0, 7.0, 300.0, 60000.0, 2.0e9)
BINOMIAL_T_READS = (0.0, 1.0, 1.25, 5.0, 5.0, 9.0, 30.0, 31.0)
