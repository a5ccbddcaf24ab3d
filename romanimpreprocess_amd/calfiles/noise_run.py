"""Drop-in for the ``solid_waffle.noise_run`` line of the reference's ``runs/2026_July/make_sca_files_2026Jul.job`` (line 76): the
noise summary of a set of dark exposures, computed on the GPU and written as the file ``make_dark_file`` reads.

    python -m romanimpreprocess_amd.calfiles.noise_run -f 1 -i <first noise file> -o <noise summary> -n 100 -t 3 -cd 5.0 -rh 7 -tn 34 -ro

``-f``: the input format, only 1 (the 2026_July cubes: the primary HDU holds the unsigned 16-bit samples); ``-i``: the first
exposure, its ``001.fits`` counted up as ``make_dark_file.noise_files`` does; ``-o``: the summary; ``-n``: the number of exposures
(fewer found: an error); ``-t``: the first frame used, counted from 1; ``-tn``: the number of frames used; ``-ro``: the cubes carry the
reference output behind the science columns and the ``AMP33`` extension is written; ``-cd`` and ``-rh`` are recorded as the cards
``CDSCUT`` and ``ROWOVER`` and have no other effect (nothing is clipped: DESIGN.md section 7); ``--tframe``: the frame time in
seconds, default 3.04.  Every exposure is read once.  solid-waffle's source is not part of the reference: the estimator is the
one of ``noisestack.py``, parity with solid-waffle is unpinned.
"""

import argparse
import sys

from .. import calio, pars
from . import make_dark_file
from .noisestack import MAX_EXPOSURES, MAX_FRAMES, NoiseStack, check_geometry

FORMATS = (1,)


def parser():
    p = argparse.ArgumentParser(prog="noise_run", allow_abbrev=False, description="noise summary of a dark set")
    p.add_argument("-f", dest="format", type=int, required=True, help="input format (only 1)")
    p.add_argument("-i", dest="first", required=True, help="first noise file, ...001.fits")
    p.add_argument("-o", dest="out", required=True, help="noise summary to write")
    p.add_argument("-n", dest="ndark", type=int, required=True, help="number of dark exposures")
    p.add_argument("-t", dest="tstart", type=int, default=1, help="first frame used, counted from 1")
    p.add_argument("-tn", dest="nframe", type=int, required=True, help="number of frames used")
    p.add_argument("-cd", dest="cdscut", type=float, default=5.0, help="recorded as CDSCUT only")
    p.add_argument("-rh", dest="rowover", type=int, default=7, help="recorded as ROWOVER only")
    p.add_argument("-ro", dest="ref_out", action="store_true", help="the cubes carry the reference output")
    p.add_argument("--tframe", type=float, default=3.04, help="frame time in seconds")
    return p


def parse(argv):
    """the job's line as a namespace; ValueError naming the option for what is not supported"""
    a = parser().parse_args(argv)
    if a.format not in FORMATS:
        raise ValueError(f"-f {a.format}: only format 1 (the 2026_July cubes) is supported")
    if not 2 <= a.ndark <= MAX_EXPOSURES:
        raise ValueError(f"-n {a.ndark} exposures (2..{MAX_EXPOSURES} supported)")
    if a.tstart < 1:
        raise ValueError(f"-t {a.tstart}: frames are counted from 1")
    if not 2 <= a.nframe <= MAX_FRAMES:
        raise ValueError(f"-tn {a.nframe} frames (2..{MAX_FRAMES} supported)")
    if not a.tframe > 0:
        raise ValueError(f"--tframe {a.tframe} (positive)")
    return a


def geometry(width, nside=pars.nside, cw=pars.channelwidth):
    """(C, cw) of frames ``width`` columns wide: the channels of ``cw`` columns within the first ``nside`` columns"""
    return min(int(nside), int(width)) // int(cw), int(cw)


class Feeder:
    """Takes the exposures of one pass over a dark set: ``feed(cube, fits_be16)`` makes the ``NoiseStack`` from the first cube's
    shape and adds every cube to it (``make_dark_file.run`` hands it the cubes that feed its ``DarkStack``); ``finish()`` is
    the ``NoiseSummary``."""

    def __init__(self, tstart, nframe, ref_out, tframe=3.04, nside=pars.nside, cw=pars.channelwidth, ndark=None, ctx=None):
        self.tstart, self.nframe, self.ref_out, self.tframe = int(tstart), int(nframe), bool(ref_out), float(tframe)
        self.nside, self.cw, self.ndark, self.ctx, self.stack = int(nside), int(cw), ndark, ctx, None

    def feed(self, cube, fits_be16):
        if self.stack is None:
            nreads, ny, width = cube.shape
            C, cw = geometry(width, self.nside, self.cw)
            check_geometry(ny, width, C, cw, self.tstart - 1, self.nframe, self.ref_out)
            if self.tstart - 1 + self.nframe > nreads:
                raise ValueError(f"-t {self.tstart} and -tn {self.nframe} ask for the frames {self.tstart}.."
                                 f"{self.tstart - 1 + self.nframe} of a cube of {nreads}")
            self.stack = NoiseStack(ny, width, C, cw, self.tstart - 1, self.nframe, self.ref_out, ctx=self.ctx)
        if self.ndark is None or self.stack.count < self.ndark:
            self.stack.add(cube, fits_be16=fits_be16)

    def finish(self):
        if self.stack is None:
            raise FileNotFoundError("no dark exposure")
        return self.stack.finish(self.tframe)


def summarize(files, tstart, nframe, ref_out, tframe=3.04, nside=pars.nside, cw=pars.channelwidth, layout="2026_July", ctx=None):
    """The ``NoiseSummary`` of ``files`` (paths, or ``DevArray`` cubes as ``make_dark_file.dark_data`` takes them), each read once."""
    from ..devarray import is_dev

    feeder = Feeder(tstart, nframe, ref_out, tframe, nside, cw, ctx=ctx)
    for f in files:
        dev = is_dev(f)
        feeder.feed(make_dark_file._dev_cube(f) if dev else make_dark_file._open_dark(f, layout), not dev)
    return feeder.finish()


def run(argv, nside=pars.nside, cw=pars.channelwidth, ctx=None):
    """Write the summary of the job's line ``argv``; returns the ``NoiseSummary``."""
    a = parse(argv)
    files = make_dark_file.noise_files(a.first)[:a.ndark]
    if len(files) < a.ndark:
        raise FileNotFoundError(f"-n {a.ndark}: only {len(files)} exposures from {a.first[:-8]}001.fits on")
    s = summarize(files, a.tstart, a.nframe, a.ref_out, a.tframe, nside=nside, cw=cw, ctx=ctx)
    write(a.out, s, a.cdscut, a.rowover, ctx=ctx)
    return s


def write(path, summary, cdscut=5.0, rowover=7, ctx=None):
    calio.write_fits(path, summary.hdus([("CDSCUT", float(cdscut)), ("ROWOVER", int(rowover))]), ctx=ctx)


if __name__ == "__main__":
    print(run(sys.argv[1:]).params)
