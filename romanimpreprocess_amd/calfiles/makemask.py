"""Drop-in for the reference's ``runs/2026_July/makemask.py``: the mask file of a CALDIR set, computed on the GPU.

    python -m romanimpreprocess_amd.calfiles.makemask <mask file to write> <sca>

The ``linearitylegendre``, ``dark`` and ``gain`` files are found by replacing ``_mask_`` in the output's name; the tree has the
script's layout and metadata keys and the script's one line (the p-flat's median) is printed.  The frame is the files' own (the
script hard-codes 4096 x 4096), the reference-pixel border 4 as there.
"""

import sys
from datetime import datetime, timezone

import numpy as np

from .. import calio
from ..utils import sky
from . import NBORDER, derive_mask


def run(outfile, sca, ctx=None):
    """Write the mask file ``outfile``; returns its path."""
    sca = int(sca)
    lin = calio.roman_branch(outfile.replace("_mask_", "_linearitylegendre_"))
    dark = calio.roman_branch(outfile.replace("_mask_", "_dark_"))
    gain = calio.roman_branch(outfile.replace("_mask_", "_gain_"))
    pflat = np.ascontiguousarray(np.asarray(lin["pflat"])[0])
    print(sky.median(pflat, ctx=ctx))
    dq = derive_mask(lin["dq"], pflat, dark["dark_slope"], gain["dq"], nb=NBORDER, ctx=ctx)
    tree = {
        "roman": {
            "meta": {
                "author": "makemask.py",
                "description": "makemask.py",
                "instrument": {"detector": f"WFI{sca:02d}", "name": "WFI"},
                "origin": "PIT - romanimpreprocess",
                "date": datetime.now(timezone.utc).isoformat(),
                "pedigree": "DUMMY",
                "reftype": "PFLAT",
                "telescope": "ROMAN",
                "useafter": "!time/time-1.2.0 2020-01-01T00:00:00.000",
            },
            "dq": dq,
        },
    }
    calio.write_asdf(outfile, tree)
    return outfile


if __name__ == "__main__":
    run(sys.argv[1], int(sys.argv[2]))
