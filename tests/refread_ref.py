"""Exposures stored with the reference read subtracted: the numpy decode the device is tested against, and the inputs the tests
of the stage entry and of the chain share.  A plain module: no fixtures, no test."""

from functools import lru_cache

import numpy as np

import oracle
from oracle import l1sim
from romanimpreprocess_amd import synth

# the stored read pattern of the chain tests: 8 groups in the exposure, 7 after the reference read has left
READ_PATTERN = [[0], [1], [2, 3], [4, 5, 6], [7, 8, 9, 10, 11], [12, 13], [14], [15, 16, 17, 18]]
NY, NX = 48, 256


def decode(enc, ref, offset):
    """the inverse of EXTRACT_REF on (ngrp, ...) u16 samples: (decoded u16, number of samples the clip changed)"""
    v = enc.astype(np.int64) + ref.astype(np.int64)[None] - int(offset)
    out = np.clip(v, 0, 65535)
    return out.astype(np.uint16), int(np.count_nonzero(out != v))


def encode_ramp(ramp, offset):
    """(the ramp as EXTRACT_REF stores it, the number of samples the encoder clipped): data, amp33, groupdq and the read pattern
    lose their first group, ``reference_read`` / ``reference_amp33`` / ``data_encoding_offset`` join"""
    ref, rest = l1sim.extract_ref(ramp["data"], offset)
    ref33, rest33 = l1sim.extract_ref(ramp["amp33"], offset)
    clipped = 0
    for stored, first, full in ((rest, ref, ramp["data"]), (rest33, ref33, ramp["amp33"])):
        exact = full[1:].astype(np.int64) - (first.astype(np.int64)[None] - offset)
        clipped += int(np.count_nonzero(exact != stored))
    enc = dict(plain_ramp(ramp), data=rest, amp33=rest33, reference_read=ref, reference_amp33=ref33, data_encoding_offset=offset)
    return enc, clipped


def plain_ramp(ramp):
    """the same exposure without its first group, not encoded"""
    return dict(ramp, data=np.ascontiguousarray(ramp["data"][1:]), amp33=np.ascontiguousarray(ramp["amp33"][1:]),
                groupdq=np.ascontiguousarray(ramp["groupdq"][1:]), read_pattern=ramp["read_pattern"][1:])


@lru_cache(maxsize=2)
def chain_inputs(k64):
    """CALDIR set (8 groups), the full ramp, its 7-group plain form, and the oracle's result for the plain form on that set
    (first group included in the fit: nothing is left to exclude)"""
    cal = synth.make_caldir(NY, NX, read_pattern=READ_PATTERN, p_order=3, seed=31, bias_amplitude=2.0, bad_lin_frac=0.005,
                            ipc_dtype=np.float64 if k64 else np.float32)
    ramp = synth.make_ramp(cal, read_pattern=READ_PATTERN, seed=32, cr_frac=0.05, saturation_backup=0)
    plain = plain_ramp(ramp)
    with np.errstate(all="ignore"):
        ref = oracle.calibrate_arrays(plain, cal, exclude_first=False)
    return cal, ramp, plain, ref
