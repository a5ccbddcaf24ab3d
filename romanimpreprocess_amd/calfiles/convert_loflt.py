"""Drop-in for the reference's ``runs/summer2025run/convert_loflt.py`` (low-intensity flat conversion script), on the GPU
(``convert_frames.convert("loflt", ...)``).

    python -m romanimpreprocess_amd.calfiles.convert_loflt <input directory> <Number of frames> <output directory> <sca>
"""

import sys

from . import convert_frames


def run(indir, N, outdir, sca, **kw):
    """``convert_frames.convert("loflt", indir, N, outdir, sca, ...)``: the files written"""
    return convert_frames.convert("loflt", indir, N, outdir, sca, **kw)


if __name__ == "__main__":
    convert_frames.main("loflt", sys.argv)
