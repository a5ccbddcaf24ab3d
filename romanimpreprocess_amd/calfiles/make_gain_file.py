"""Drop-in for the reference's ``runs/2026_July/make_gain_file.py`` (the same script in ``runs/summer2025run``): the ``gain`` and
``ipc4d`` files of a CALDIR set from solid-waffle's superpixel summaries, expanded on the GPU.

    python -m romanimpreprocess_amd.calfiles.make_gain_file <summaries> <sca> <outfile>

Same conventions: ``summaries`` is a text file of summary-file paths, each read with ``np.loadtxt``; the configuration file of
a summary is its path minus the last 11 characters plus ``config.txt``, and all of them go into ``notes.solid_waffle_config``,
each behind a ``# <name>`` line; the ipc4d file's name is ``outfile``'s with ``_gain_`` replaced (in the file name, not in the
directory); the two trees have the script's layout and metadata keys (``reftype`` ``GAIN`` and ``IPC4D``) and the script's lines
are printed.  The ipc4d flags are all zero, as the script's are.  ``ipc_dtype=np.float32`` writes the
kernel rounded once to float32, which the fused chain reads in its faster form; float64 is what the script writes.
The two ``_asdf_data.fits`` display dumps of the script are written too (``calio.write_fits``): the gain plane, and ipc4d laid out as
a (3 ny, 3 nx) image by the script's transpose (made on the host: it is a display file), each behind an empty primary HDU.
"""

import sys
from datetime import datetime, timezone
from os.path import split as pathsplit

import numpy as np

from .. import calio, pars
from . import NBORDER, derive_gain_ipc4d, summary_means


def _meta(sca, reftype):
    return {
        "author": "make_gain_file.py",
        "description": "make_gain_file.py",
        "instrument": {"detector": f"WFI{sca:02d}", "name": "WFI"},
        "origin": "PIT - romanimpreprocess",
        "date": datetime.now(timezone.utc).isoformat(),
        "pedigree": "DUMMY",
        "reftype": reftype,
        "telescope": "ROMAN",
        "useafter": "!time/time-1.2.0 2020-01-01T00:00:00.000",
    }


def ipc4d_path(outfile):
    """``make_gain_file.py:178-179``"""
    head, tail = pathsplit(outfile)
    return head + "/" + tail.replace("_gain_", "_ipc4d_")


def run(summaries, sca, outfile, *, ipc_dtype=np.float64, shape=None, ctx=None):
    """Write the gain file ``outfile`` and its ``_ipc4d_`` sibling; returns their two paths.  ``shape``: the frame, where it is
    not the H4RG's ``(pars.nside, pars.nside)`` the script hard-codes."""
    sca = int(sca)
    ny, nx = (pars.nside, pars.nside) if shape is None else (int(shape[0]), int(shape[1]))
    with open(summaries) as f:
        infiles = [line.rstrip() for line in f.readlines()]
    tables = []
    for name in infiles:
        print(name)
        tables.append(np.loadtxt(name))
    means, good, tmean = summary_means(np.stack(tables))
    nsy, nsx = good.shape
    print("superpixels", nsx, nsy)
    print("repeat", nx // nsx, ny // nsy)
    print(good.ravel(), "-->", np.count_nonzero(good), "good pixels")
    print("mean values", tmean)

    config_lines = []
    for name in infiles:
        iq = name[:-11] + "config.txt"
        config_lines.append("# " + iq)
        with open(iq) as f:
            config_lines.extend([s.rstrip() for s in f.readlines()])
    config_lines = "\n".join(config_lines)
    print("--")
    print(config_lines)
    print("--")

    gain, gain_dq, kernel, kernel_dq = derive_gain_ipc4d(means, good, shape=(ny, nx), nb=NBORDER, ipc_dtype=ipc_dtype, ctx=ctx)
    calio.write_asdf(outfile, {"roman": {"meta": _meta(sca, "GAIN"), "data": gain, "dq": gain_dq},
                               "notes": {"solid_waffle_config": config_lines}})
    calio.write_fits(outfile[:-5] + "_asdf_data.fits", [None, gain], ctx=ctx)   # (make_gain_file.py:114-119)
    outfile2 = ipc4d_path(outfile)
    calio.write_asdf(outfile2, {"roman": {"meta": _meta(sca, "IPC4D"), "data": kernel, "dq": kernel_dq},
                                "notes": {"solid_waffle_config": config_lines}})
    tiled = np.ascontiguousarray(np.transpose(kernel, axes=(0, 2, 1, 3))).reshape(3 * kernel.shape[2], 3 * kernel.shape[3])
    calio.write_fits(outfile2[:-5] + "_asdf_data.fits", [None, tiled], ctx=ctx)   # (make_gain_file.py:202-209)
    return outfile, outfile2


if __name__ == "__main__":
    run(sys.argv[1], int(sys.argv[2]), sys.argv[3])
