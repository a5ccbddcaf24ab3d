"""Drop-in for the reference's ``runs/summer2025run/convert_dark.py`` (dark conversion script), on the GPU
(``convert_frames.convert("dark", ...)``).

    python -m romanimpreprocess_amd.calfiles.convert_dark <input directory> <Number of frames> <output directory> <sca>
"""

import sys

from . import convert_frames


def run(indir, N, outdir, sca, **kw):
    """``convert_frames.convert("dark", indir, N, outdir, sca, ...)``: the files written"""
    return convert_frames.convert("dark", indir, N, outdir, sca, **kw)


if __name__ == "__main__":
    convert_frames.main("dark", sys.argv)
