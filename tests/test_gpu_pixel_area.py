"""The pixel-area map on the GPU (rip_stage_pixel_area) and the FITSWCS path of calibrateimage and the noise layers."""

import ctypes as C

import numpy as np
import pytest
import torch  # before libromanhip is loaded: torch brings its own copy of the HIP runtime, and the first one loaded must be the one both use
import wcs_area_ref as ref
from conftest import assert_same_bits, gpu_context

import oracle
from oracle import saturation
from romanimpreprocess_amd import _native, calio, pars, pipeline, synth
from romanimpreprocess_amd.L1_to_L2 import gen_cal_image, gen_noise_image
from romanimpreprocess_amd.utils import coordutils
from romanimpreprocess_amd.utils.coordutils import FitsWCS

pytestmark = pytest.mark.gpu

SIP3 = {"A_1_1": -1.0e-6, "A_2_0": 3.0e-6, "A_0_2": 2.0e-6, "B_0_2": 1.4e-5, "B_1_1": -1.0e-5, "A_0_3": 1.0e-9, "B_2_1": -2.0e-9}


def _wcs(cards):
    return FitsWCS(calio.parse_fits_header(ref.header_text(cards)))


def _max_rel(a, b):
    return float(np.max(np.abs(a / b - 1.0)))


def caldir_files(tmp_path, cal, npz_biascorr=True):
    """the CALDIR set as files (the recipe of test_calibrateimage_files_end_to_end)"""
    caldir = {}
    names = {"dark": "dark", "read": "read", "gain": "gain", "linearitylegendre": "linearitylegendre", "ipc4d": "ipc4d",
             "flat": "pflat", "biascorr": "biascorr", "mask": "mask", "saturation": "saturation"}
    for key, fname in names.items():
        npz = npz_biascorr and key == "biascorr"
        path = tmp_path / f"roman_wfi_{fname}_TEST_SCA04.{'npz' if npz else 'asdf'}"
        if npz:
            calio.save_npz_tree(str(path), {"roman": cal[key]})
        else:
            calio.write_asdf(str(path), {"roman": cal[key]})
        caldir[key] = str(path)
    return caldir


@pytest.mark.parametrize("proj", ["TAN", "STG", "ZEA", "ARC", "SIN"])
def test_device_map_matches_the_restatement(proj):
    ctx = gpu_context()
    worst = 0.0
    for crval2 in (83.0, -20.0, 0.0):
        for sip in (None, SIP3):
            for ny, nx in ((1, 1), (2, 3), (37, 53), (256, 256)):
                w = _wcs(ref.simple_cards(proj, crval2, 0.11 / 3600, max(ny, nx), sip=sip, rot_deg=30.0))
                got = coordutils.pixelarea_map(w, ny, nx, ctx=ctx)
                assert got.shape == (ny, nx) and got.dtype == np.float64
                worst = max(worst, _max_rel(got, ref.pixel_area(w, ny, nx)))
    print(proj, "device vs restatement, max relative difference", worst)
    assert worst <= 1e-8


def test_workflow_header_full_frame():
    """the reference workflow test's TAN-SIP header at 4096 x 4096: restatement, analytic Jacobian, AreaFactor range"""
    ctx = gpu_context()
    w = _wcs(ref.WORKFLOW_CARDS)
    N = pars.nside
    got = coordutils.pixelarea_map(w, N, N, scale=pars.Omega_ideal, ctx=ctx)
    d_ref = _max_rel(got, ref.pixel_area(w, N, N, scale=pars.Omega_ideal))
    d_ana = _max_rel(got, ref.analytic_area(w, N, N, scale=pars.Omega_ideal))
    print("4096^2 workflow header: vs restatement", d_ref, "vs analytic", d_ana, "AreaFactor", got.min(), got.max())
    assert d_ref <= 1e-8 and d_ana <= 1e-8
    assert 0.93 < got.min() < 0.94 and 1.06 < got.max() < 1.07


def test_host_and_device_outputs_are_identical():
    ctx = gpu_context()
    w = _wcs(ref.simple_cards("STG", -83.0, 1.0 / 3600, 300, sip=SIP3, rot_deg=-12.0))
    a = coordutils.pixelarea_map(w, 300, 301, scale=2.5, ctx=ctx)
    b = coordutils.pixelarea_map(w, 300, 301, scale=2.5, ctx=ctx)
    t = coordutils.pixelarea_map(w, 300, 301, scale=2.5, device=True, ctx=ctx)
    assert t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (300, 301)
    assert_same_bits(a, b, "two host calls")
    assert_same_bits(t.cpu().numpy(), a, "device vs host output")
    cb = pipeline.Calibrator(ctx=ctx)
    af = cb.area_factor(w, 40, 50)
    assert not af.flags.writeable and cb.area_factor(w, 40, 50) is af
    assert_same_bits(af, coordutils.pixelarea_map(w, 40, 50, scale=pars.Omega_ideal, ctx=ctx), "Calibrator.area_factor")


def test_bad_descriptors_are_refused():
    ctx = gpu_context()
    good = _wcs(ref.WORKFLOW_CARDS).desc()
    out = np.zeros((4, 4))

    def call(d, ny=4, nx=4, scale=1.0, loc=_native.RIP_HOST):
        rc = ctx.lib.rip_stage_pixel_area(ctx.h, C.byref(d), ny, nx, scale, loc, out.ctypes.data)
        return rc, ctx.lib.rip_last_error(ctx.h).decode()

    for field, value, word in (("projection", 5, "projection"), ("projection", -1, "projection"),
                               ("sip_order", 10, "SIP order"), ("sip_order", -1, "SIP order"), ("lonpole", float("nan"), "finite")):
        d = _native.WcsDesc.from_buffer_copy(good)
        setattr(d, field, value)
        rc, msg = call(d)
        assert rc == -1, (field, value)   # RIP_EINVAL
        assert word in msg, msg
    for kw, word in ((dict(ny=0), "bad arguments"), (dict(nx=-3), "bad arguments"), (dict(scale=0.0), "scale"),
                     (dict(scale=-1.0), "scale"), (dict(loc=7), "bad arguments")):
        rc, msg = call(_native.WcsDesc.from_buffer_copy(good), **kw)
        assert rc == -1 and word in msg, (kw, msg)
    with pytest.raises(ValueError, match="scale"):
        coordutils.pixelarea_map(_wcs(ref.WORKFLOW_CARDS), 4, 4, scale=0.0, ctx=ctx)


# ---- calibrateimage with FITSWCS

STRONG_SIP = [("CTYPE1", "RA---TAN-SIP"), ("CTYPE2", "DEC--TAN-SIP"), ("CRPIX1", 127.5), ("CRPIX2", 23.5),
              ("CD1_1", -3.0555555555555554e-05), ("CD1_2", 0.0), ("CD2_1", 0.0), ("CD2_2", 3.0555555555555554e-05),
              ("CRVAL1", 37.0), ("CRVAL2", -20.0), ("LONPOLE", 215.0),
              ("A_ORDER", 2), ("A_2_0", 1.0e-4), ("A_1_1", -2.0e-5), ("B_ORDER", 2), ("B_0_2", 1.0e-4), ("B_1_1", 1.0e-4),
              "COMMENT truth wcs from sim_to_isim"]


def test_calibrateimage_with_fitswcs(tmp_path):
    rp = synth.READ_PATTERN_6
    ny, nx = 48, 256
    cal = synth.make_caldir(ny, nx, read_pattern=rp, p_order=3, seed=31, bias_amplitude=1.0)
    ramp = synth.make_ramp(cal, read_pattern=rp, seed=32, cr_frac=0.02)
    caldir = caldir_files(tmp_path, cal)
    l1 = {"roman": {"data": ramp["data"], "amp33": ramp["amp33"],
                    "meta": {"exposure": {"frame_time": synth.FRAME_TIME, "read_pattern": rp},
                             "instrument": {"detector": "WFI04"}}}}
    calio.write_asdf(str(tmp_path / "l1.asdf"), l1)
    wcs_path = tmp_path / "l1_asdf_wcshead.txt"
    wcs_path.write_text(ref.header_text(STRONG_SIP))
    base = {"IN": str(tmp_path / "l1.asdf"), "CALDIR": caldir, "JUMP_DETECT_PARS": {"SthreshA": 5.0, "IthreshB": 800.0}}
    cb = pipeline.Calibrator(ctx=gpu_context())

    def run(name, **extra):
        cfg = dict(base, OUT=str(tmp_path / f"{name}.asdf"), **extra)
        gen_cal_image.calibrateimage(cfg, verbose=False, calibrator=cb)
        return calio.read_asdf(cfg["OUT"])

    A = coordutils.pixelarea_map(FitsWCS.from_file(str(wcs_path)), ny, nx, scale=pars.Omega_ideal, ctx=gpu_context())
    print("AreaFactor of the test frame", A.min(), A.max())
    assert A.max() / A.min() > 1.01
    calio.write_asdf(str(tmp_path / "area.asdf"), {"roman": {"data": A}})
    other = 1.0 + 0.01 * np.cos(np.arange(ny * nx, dtype=np.float64).reshape(ny, nx) / 50.0)
    calio.write_asdf(str(tmp_path / "area_other.asdf"), {"roman": {"data": other}})

    with_wcs = run("l2_wcs", FITSWCS=str(wcs_path))
    with_file = run("l2_area", AREAFACTOR=str(tmp_path / "area.asdf"))
    plain = run("l2_plain")
    both = run("l2_both", FITSWCS=str(wcs_path), AREAFACTOR=str(tmp_path / "area_other.asdf"))
    file_only = run("l2_other", AREAFACTOR=str(tmp_path / "area_other.asdf"))
    for k in ("data", "dq", "var_poisson", "var_rnoise", "err", "data_withsky"):
        assert_same_bits(np.asarray(with_wcs["roman"][k]), np.asarray(with_file["roman"][k]), f"FITSWCS vs AREAFACTOR: {k}")
        assert_same_bits(np.asarray(both["roman"][k]), np.asarray(file_only["roman"][k]), f"AREAFACTOR takes precedence: {k}")
    assert "acquired flat field" in with_wcs["processinfo"]["log"] and "50%ile" in with_wcs["processinfo"]["log"]

    # the oracle chain with the same AreaFactor
    r0 = {"data": ramp["data"], "amp33": ramp["amp33"], "groupdq": np.zeros(ramp["data"].shape, np.uint8),
          "pixeldq": cal["mask"]["dq"].copy(), "read_pattern": rp, "frame_time": synth.FRAME_TIME}
    r0["groupdq"][0] |= 1
    saturation.flag_saturation(r0, cal["saturation"]["data"], backup=1, skip_firstn=1, sat_dq=cal["saturation"]["dq"],
                               read_pattern=rp)
    want = oracle.calibrate_arrays(r0, cal, jump_pars=base["JUMP_DETECT_PARS"], area_factor=A)
    act = (slice(4, -4), slice(4, -4))
    slope = np.asarray(with_wcs["roman"]["data"])
    assert_same_bits(with_wcs["roman"]["dq"], want["pixeldq"][act], "L2 dq")
    np.testing.assert_allclose(slope, want["slope"][act], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(with_wcs["roman"]["var_poisson"], want["err_poisson"][act] ** 2, rtol=3e-5, atol=1e-12)
    # ... and the map is not a no-op
    assert not np.allclose(slope, np.asarray(plain["roman"]["data"]), rtol=1e-5, atol=1e-7)


# ---- noise layers with FITSWCS


def test_noise_layers_with_fitswcs(tmp_path):
    rp = synth.READ_PATTERN_8
    ny, nx = 72, 256
    cal = synth.make_caldir(ny, nx, read_pattern=rp, p_order=3, seed=31, bias_amplitude=1.0)
    ramp = synth.make_ramp(cal, read_pattern=rp, seed=32, cr_frac=0.0)
    caldir = caldir_files(tmp_path, cal, npz_biascorr=False)
    l1 = {"roman": {"data": ramp["data"], "amp33": ramp["amp33"],
                    "meta": {"exposure": {"frame_time": synth.FRAME_TIME, "read_pattern": rp},
                             "instrument": {"detector": "WFI04"}}}}
    calio.write_asdf(str(tmp_path / "l1.asdf"), l1)
    wcs_path = tmp_path / "l1_asdf_wcshead.txt"
    wcs_path.write_text(ref.header_text(STRONG_SIP))
    noise = {"LAYER": ["Ra", "R", "RaS2", "Raz2", "Ccomment", "Pr", "Pb2r", "OS2"], "TEMP": str(tmp_path / "tmp.asdf"), "SEED": 11,
             "OUT": str(tmp_path / "noise.asdf")}
    config = {"IN": str(tmp_path / "l1.asdf"), "OUT": str(tmp_path / "l2.asdf"), "CALDIR": caldir, "SLICEOUT": True,
              "NOISE": noise, "NOISE_PRECISION": 32, "FITSWCS": str(wcs_path)}
    cb = pipeline.Calibrator(ctx=gpu_context())
    gen_cal_image.calibrateimage(config, verbose=False, calibrator=cb)
    assert gen_noise_image._device_path_applies(config, None)
    dev_loop = gen_noise_image.make_noise_cube(config)
    host_loop = gen_noise_image.make_noise_cube(dict(config, NOISE=dict(noise, DEVICE_RESIDENT=False)))
    assert_same_bits(host_loop, dev_loop, "host-array layer loop vs the HBM-resident one, FITSWCS")

    # a read-noise layer is a difference of two slopes divided by the same f32(flat / AreaFactor): it scales with AreaFactor
    plain = {k: v for k, v in config.items() if k != "FITSWCS"}
    plain["OUT"] = str(tmp_path / "l2_plain.asdf")
    gen_cal_image.calibrateimage(plain, verbose=False, calibrator=cb)
    one = dict(noise, LAYER=["Ra"])
    lw = gen_noise_image.make_noise_cube(dict(config, NOISE=one))[0]
    lp = gen_noise_image.make_noise_cube(dict(plain, NOISE=one))[0]
    A = cb.area_factor(FitsWCS.from_file(str(wcs_path)), ny, nx)[4:-4, 4:-4]
    l2p = calio.read_asdf(plain["OUT"])["roman"]
    good = (np.asarray(l2p["dq"]) == 0) & np.isfinite(lp)
    s = np.std(lp[good])
    # f32 rounding of the two slopes the layer is the difference of: ~1e-7 of the slope itself
    assert np.all(np.abs(lw[good] - lp[good] * A[good]) < 1e-3 * s + 1e-6 * np.abs(np.asarray(l2p["data"])[good]))
    assert np.max(np.abs(lw[good] - lp[good])) > 5e-3 * s
