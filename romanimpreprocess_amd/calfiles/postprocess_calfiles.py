"""Drop-in for the reference's ``runs/2026_July/postprocess_calfiles.py``: p-flat, saturation and bias-correction files from a
``linearitylegendre`` file and its ``gain`` and ``dark`` siblings, computed on the GPU.

    python -m romanimpreprocess_amd.calfiles.postprocess_calfiles <linearitylegendre file> <sca> <read pattern name>

Same conventions: the siblings and the outputs are found by replacing ``_linearitylegendre_`` in the file name,
``settings_<read pattern name>.yaml`` (``READS``) and ``linearity_pars_<sca>.json`` (``TFRAME``, ``BIAS/SLICE``) are read from the
working directory, the three trees have the script's layout and metadata keys (``t0`` and ``t0_comment`` included) and the same
lines are printed.  The script's last statements, which dump biascorr and the predicted dark as one (2 ngrp, ny, nx) float32 cube
to ``<biascorr>_asdf_to.fits``, are mirrored through ``calio.write_fits``.
"""

import json
import sys
from datetime import datetime, timezone

import numpy as np
import yaml

from .. import calio
from . import BFRAME, NBORDER, TFRAME, derive_biascorr, derive_pflat, derive_saturation, parse_reads


def _meta(sca, reftype):
    return {
        "author": "postprocess_calfiles.py",
        "description": "postprocess_calfiles.py",
        "instrument": {"detector": f"WFI{sca:02d}", "name": "WFI"},
        "origin": "PIT - romanimpreprocess",
        "date": datetime.now(timezone.utc).isoformat(),
        "pedigree": "DUMMY",
        "reftype": reftype,
        "telescope": "ROMAN",
        "useafter": "!time/time-1.2.0 2020-01-01T00:00:00.000",
    }


def frame_pars(lpars):
    """(tframe, bframe) of a ``linearity_pars_<sca>.json`` dict (``postprocess_calfiles.py:106-112``)."""
    tframe, bframe = TFRAME, BFRAME
    if "TFRAME" in lpars:
        tframe = float(lpars["TFRAME"])
    if "BIAS" in lpars and "SLICE" in lpars["BIAS"]:
        bframe = int(lpars["BIAS"]["SLICE"])
    return tframe, bframe


def run(infile, sca, readpatternname=None, *, reads=None, lpars=None, ctx=None):
    """Write the ``_pflat_``, ``_saturation_`` and ``_biascorr_`` siblings of ``infile``; returns their three paths.  ``reads`` (the
    flat ``READS`` list) and ``lpars`` (the json's dict) replace the two files of the working directory."""
    sca = int(sca)
    if reads is None:
        with open("settings_" + readpatternname + ".yaml") as f:
            reads = yaml.safe_load(f)["READS"]
    if lpars is None:
        with open(f"linearity_pars_{sca:02d}.json") as f:
            lpars = json.load(f)
    tframe, bframe = frame_pars(lpars)
    lin = calio.roman_branch(infile)
    gain = calio.roman_branch(infile.replace("_linearitylegendre_", "_gain_"))
    dark = calio.roman_branch(infile.replace("_linearitylegendre_", "_dark_"))
    nb = NBORDER

    # p-flat
    outfile_flat = infile.replace("_linearitylegendre_", "_pflat_")
    pflat, dq, coefs = derive_pflat(np.asarray(lin["pflat"])[0], gain["data"], ctx=ctx)
    print(coefs)
    calio.write_asdf(outfile_flat, {"roman": {"meta": _meta(sca, "PFLAT"), "data": pflat, "dq": dq}, "notes": {"src": infile}})
    print("Pflat quality -->", np.count_nonzero(dq[nb:-nb, nb:-nb]), "science pixels flagged.")
    print("deciles -->", [np.round(np.percentile(pflat, 10 * i), 5) for i in range(1, 10)])

    # saturation
    outfile_sat = infile.replace("_linearitylegendre_", "_saturation_")
    sat, sdq = derive_saturation(lin["Smax"], lin["Sref"], ctx=ctx)
    print("saturation deciles -->", [np.percentile(sat, 10 * i) for i in range(1, 10)])
    calio.write_asdf(outfile_sat, {"roman": {"meta": _meta(sca, "SATURATION"), "data": sat, "dq": sdq}, "notes": {"src": infile}})

    # bias correction: the dark image minus the dark current run forward in time
    rd, ngrp, xref = parse_reads(reads, bframe)
    print("-----", xref)
    for j in range(ngrp):
        print("::", j, int(rd[2 * j]), int(rd[2 * j + 1]))
    bias_corr, t0, pred = derive_biascorr(dark["dark_slope"], dark["data"], lin["data"], lin["Smin"], lin["Smax"], reads, tframe=tframe,
                                          bframe=bframe, nb=nb, want_pred=True, ctx=ctx)
    print("-->")
    print(np.asarray(dark["data"])[:, nb:-nb, nb:-nb][:, :4, :4])
    print("-->")
    print(pred[:, :4, :4])
    outfile_biascorr = infile.replace("_linearitylegendre_", "_biascorr_")
    calio.write_asdf(outfile_biascorr, {"roman": {
        "meta": _meta(sca, "BIASCORR"), "data": bias_corr, "t0": t0,
        "t0_comment": "number of seconds after reset used to define Sref, corresponding to 0 DN_lin"}})
    # (postprocess_calfiles.py:169-172)
    calio.write_fits(outfile_biascorr[:-5] + "_asdf_to.fits", [np.concatenate([bias_corr, pred]).astype(np.float32, copy=False)], ctx=ctx)
    return outfile_flat, outfile_sat, outfile_biascorr


if __name__ == "__main__":
    run(sys.argv[1], int(sys.argv[2]), sys.argv[3])
