"""Exposures stored with the reference read subtracted, the parts that need no GPU: the C-ABI additions and their ctypes mirror,
the driver's reading of such a tree, the noise driver's choice of back end, and the numpy decode the GPU tests compare with."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from conftest import REPO, assert_same_bits
from refread_ref import READ_PATTERN, decode, encode_ramp

from oracle import l1sim
from romanimpreprocess_amd import _native, synth
from romanimpreprocess_amd.from_sim import sim_to_isim
from romanimpreprocess_amd.L1_to_L2 import gen_cal_image, gen_noise_image


def test_entry_is_declared_and_bound():
    hdr = open(os.path.join(REPO, "include", "romanhip.h")).read()
    assert re.search(r"\bint rip_stage_decode_reference_read\s*\(", hdr)
    assert "rip_stage_decode_reference_read" in _native.SYMBOLS
    lib = _native.load_library()
    assert hasattr(lib, "rip_stage_decode_reference_read")
    assert lib.rip_version() == 100


def test_new_ramp_fields_match_the_header(tmp_path):
    """sizeof / offsetof of the three trailing fields of rip_ramp_desc as gcc sees them == the ctypes mirror; they follow
    or_first_group, so that a descriptor of an older caller, zeroed, reads as a plain ramp"""
    fields = ["or_first_group", "reference_read", "reference_amp33", "data_encoding_offset"]
    src = tmp_path / "abi.c"
    body = 'printf("size %zu\\n", sizeof(rip_ramp_desc));\n' + "".join(
        f'printf("{f} %zu %zu\\n", offsetof(rip_ramp_desc, {f}), sizeof(((rip_ramp_desc *)0)->{f}));\n' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "romanhip.h"\nint main(void){\n' + body + "return 0;}\n")
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = {line.split()[0]: [int(x) for x in line.split()[1:]] for line in subprocess.check_output([str(exe)], text=True).splitlines()}
    assert got["size"] == [C.sizeof(_native.RampDesc)]
    for f in fields:
        d = getattr(_native.RampDesc, f)
        assert got[f] == [d.offset, d.size], f
    offsets = [got[f][0] for f in fields]
    assert offsets == sorted(offsets) and [name for name, _ in _native.RampDesc._fields_][-3:] == fields[1:]


def test_numpy_decode_inverts_the_encoder():
    """decode o encode is the identity where the encoder did not clip; where it did, the decoded sample stays inside 0..65535 (no
    count); pieces that do not belong together are counted"""
    rng = np.random.default_rng(3)
    data = rng.integers(0, 65536, size=(4, 9, 11), dtype=np.uint16)
    for offset in (0, 1000, 65535, -5):
        ref, rest = l1sim.extract_ref(data, offset)
        out, bad = decode(rest, ref, offset)
        exact = data[1:].astype(np.int64) - (data[0].astype(np.int64) - offset)
        kept = (exact >= 0) & (exact <= 65535)
        assert bad == 0 and np.array_equal(out[kept], data[1:][kept]) and np.count_nonzero(~kept) > 0
        assert np.all(out[exact < 0] >= data[1:][exact < 0]) and np.all(out[exact > 65535] <= data[1:][exact > 65535])
    out, bad = decode(np.zeros((2, 5), np.uint16), np.zeros(5, np.uint16), 70000)
    assert bad == 10 and not out.any()


def l1_tree():
    cal = synth.make_caldir(24, 128, read_pattern=READ_PATTERN, p_order=3, seed=5)
    ramp = synth.make_ramp(cal, read_pattern=READ_PATTERN, seed=6)
    return {"data": ramp["data"], "amp33": ramp["amp33"],
            "meta": {"exposure": {"frame_time": synth.FRAME_TIME, "read_pattern": [list(g) for g in READ_PATTERN]},
                     "instrument": {"detector": "WFI04"}}}, ramp


def test_initializationstep_reads_an_encoded_tree():
    tree, ramp = l1_tree()
    sim_to_isim.extract_ref(tree, {"EXTRACT_REF": {"data_encoding_offset": 4000}})
    want, clipped = encode_ramp(ramp, 4000)
    assert clipped == 0
    got, meta = gen_cal_image.initializationstep({"IN": tree, "EXCLUDE_FIRST": False}, {}, None)
    assert got["data_encoding_offset"] == 4000
    assert_same_bits(got["reference_read"], want["reference_read"], "reference_read")
    assert_same_bits(got["reference_amp33"], want["reference_amp33"], "reference_amp33")
    assert_same_bits(got["data"], want["data"], "data as stored")
    assert got["data"].shape[0] == 7 and len(meta["read_pattern"]) == 7 and got["groupdq"].shape == got["data"].shape
    # amp33 not encoded: the key is there and says so
    del tree["reference_amp33"]
    got, _ = gen_cal_image.initializationstep({"IN": tree, "EXCLUDE_FIRST": False}, {}, None)
    assert got["reference_amp33"] is None and got["reference_read"] is not None
    # a plain tree yields none of the three
    plain, _ = l1_tree()
    got, _ = gen_cal_image.initializationstep({"IN": plain}, {}, None)
    assert not {"reference_read", "reference_amp33", "data_encoding_offset"} & set(got)


def test_initializationstep_wants_the_offset():
    tree, _ = l1_tree()
    sim_to_isim.extract_ref(tree, {"EXTRACT_REF": {"data_encoding_offset": 4000}})
    del tree["meta"]["instrument"]["data_encoding_offset"]
    with pytest.raises(ValueError, match="data_encoding_offset"):
        gen_cal_image.initializationstep({"IN": tree}, {}, None)
    del tree["meta"]["instrument"]
    with pytest.raises(ValueError, match="data_encoding_offset"):
        gen_cal_image.initializationstep({"IN": tree}, {}, None)


def test_noise_layers_of_an_encoded_exposure_stay_on_the_host():
    tree, _ = l1_tree()
    config = {"IN": {"roman": tree}, "CALDIR": {"saturation": "x"}, "NOISE": {"LAYER": []}}
    assert gen_noise_image._device_path_applies(config, None)
    sim_to_isim.extract_ref(tree, {"EXTRACT_REF": {"data_encoding_offset": 1000}})
    assert not gen_noise_image._device_path_applies(config, None)
    assert not gen_noise_image._device_path_applies(dict(config, IN=tree), None)
    # IN a path: the driver hands over the tree it has read
    assert not gen_noise_image._device_path_applies(dict(config, IN="l1.asdf"), None, {"roman": tree})
    assert gen_noise_image._device_path_applies(dict(config, IN="l1.asdf"), None, {"roman": l1_tree()[0]})
