"""Gain and ipc4d files on the device (csrc/gainfile.hip, calfiles.derive_gain_ipc4d, calfiles/make_gain_file.py) against the
fixtures the reference's own make_gain_file.py produced on the tables of tests/gainfile_cases.py, and against the closed-form
restatement tests/gainfile_ref.py where no fixture exists (non-square frames, strips of the full frame).  Everything is
compared bit for bit.  The frames walk the kernel's store paths: 16 bytes per lane (active width a multiple of 4, or of 2 for
float64), 8 bytes (float32 on a width of 4k + 2) and single values (odd widths)."""

import contextlib
import io

import gainfile_cases as gc
import gainfile_ref as gr
import numpy as np
import pytest
from conftest import assert_same_bits, gpu_context, load_golden

from romanimpreprocess_amd import _native, calfiles, calio, pipeline, synth
from romanimpreprocess_amd.calfiles import make_gain_file
from romanimpreprocess_amd.devarray import DevArray

pytestmark = pytest.mark.gpu

OUTPUTS = ("gain", "gain_dq", "kernel", "kernel_dq")


def fixture(name):
    g = load_golden(name)
    n = int(g["nside"])
    return g, {e: g["mean_" + e] for e in gr.NAMES}, g["good"], (n, n)


def check_all(got, want, what):
    assert len(got) == len(want) == 4
    for o, a, b in zip(OUTPUTS, got, want):
        assert_same_bits(a.numpy() if isinstance(a, DevArray) else a, b, f"{what} {o}")


def random_tables(seed, nsy, nsx, bad=()):
    rng = np.random.default_rng(seed)
    u = rng.random((4, nsy, nsx))
    means = {"g": 1.4 + 0.3 * u[0], "aH": 0.012 + 0.006 * u[1], "aV": 0.015 + 0.007 * u[2], "aD": 0.0011 + 0.0009 * u[3]}
    good = np.ones((nsy, nsx), bool)
    for b in bad:
        good[b] = False
    return means, good


@pytest.mark.parametrize("name", list(gc.CASES))
@pytest.mark.parametrize("on_device", [False, True])
def test_against_the_reference_fixture(name, on_device):
    g, means, good, shape = fixture(name)
    ctx = gpu_context()
    want = (g["gain"], g["gain_dq"], g["kernel"], g["kernel_dq"])
    got = calfiles.derive_gain_ipc4d(means, good, shape=shape, nb=gc.NB, on_device=on_device, ctx=ctx)
    assert all(isinstance(a, DevArray if on_device else np.ndarray) for a in got)
    check_all(got, want, name)
    got32 = calfiles.derive_gain_ipc4d(means, good, shape=shape, nb=gc.NB, ipc_dtype=np.float32, on_device=on_device, ctx=ctx)
    check_all(got32, want[:2] + (g["kernel"].astype(np.float32), want[3]), f"{name} float32")
    # the values the planes are made of, spelled out once more: zero edges, flagged border, no ipc4d flag
    K = got[2].numpy() if on_device else got[2]
    assert (K[0, :, 0] == 0).all() and (K[2, :, -1] == 0).all() and (K[:, 0, :, 0] == 0).all() and (K[:, 2, :, -1] == 0).all()
    dq = got[1].numpy() if on_device else got[1]
    assert (dq[:4] == 2**19).all() and (dq[-4:] == 2**19).all() and (dq[:, :4] == 2**19).all() and (dq[:, -4:] == 2**19).all()
    assert not (got[3].numpy() if on_device else got[3]).any()


@pytest.mark.parametrize("name", list(gc.CASES))
@pytest.mark.parametrize("ipc_dtype", [np.float64, np.float32])
def test_each_output_skipped_in_turn(name, ipc_dtype):
    g, means, good, shape = fixture(name)
    ctx = gpu_context()
    want = dict(zip(OUTPUTS, (g["gain"], g["gain_dq"], g["kernel"].astype(ipc_dtype), g["kernel_dq"])))
    for skip in OUTPUTS:
        for on_device in (False, True):
            got = dict(zip(OUTPUTS, calfiles.derive_gain_ipc4d(means, good, shape=shape, nb=gc.NB, ipc_dtype=ipc_dtype, on_device=on_device,
                                                               ctx=ctx, outputs=tuple(o for o in OUTPUTS if o != skip))))
            assert got[skip] is None
            for o in OUTPUTS:
                if o != skip:
                    a = got[o]
                    assert_same_bits(a.numpy() if on_device else a, want[o], f"{name} {o} without {skip}")
    only = calfiles.derive_gain_ipc4d(means, good, shape=shape, nb=gc.NB, ipc_dtype=ipc_dtype, ctx=ctx, outputs=("kernel_dq",))
    assert only[:3] == (None, None, None) and not only[3].any() and only[3].shape == want["kernel_dq"].shape


# frame, superpixel table, superpixels without data, border: non-square frames; one pixel column per superpixel; superpixels
# smaller than the border (whole superpixels of reference pixels) on an active width of 4k + 2; no border at all
NONSQUARE = {
    "44x140 2x5": ((44, 140), (2, 5), [(1, 3)], 4),
    "16x128 rx=1": ((16, 128), (4, 128), [(2, 0), (1, 77), (3, 127)], 4),
    "24x50 rx=2": ((24, 50), (8, 25), [(0, 0), (4, 12), (7, 24)], 4),
    "27x35 odd": ((27, 35), (9, 7), [(3, 3)], 4),
    "12x24 nb=0": ((12, 24), (3, 4), [(0, 0)], 0),
    "20x2064 several workgroups a row": ((20, 2064), (2, 8), [(1, 7)], 4),
}


@pytest.mark.parametrize("case", list(NONSQUARE))
def test_non_square_frames_against_the_restatement(case):
    shape, (nsy, nsx), bad, nb = NONSQUARE[case]
    means, good = random_tables(500 + len(case), nsy, nsx, bad)
    means["aD"][0, 0] = -0.0004
    ctx = gpu_context()
    for ipc_dtype in (np.float64, np.float32):
        want = gr.derive(means, good, shape, nb=nb, ipc_dtype=ipc_dtype)
        check_all(calfiles.derive_gain_ipc4d(means, good, shape=shape, nb=nb, ipc_dtype=ipc_dtype, ctx=ctx), want, f"{case} host")
        check_all(calfiles.derive_gain_ipc4d(means, good, shape=shape, nb=nb, ipc_dtype=ipc_dtype, on_device=True, ctx=ctx), want,
                  f"{case} device")


def test_all_zero_tables_give_positive_zero_sums():
    """alphas of -0.0: every off-centre value is -0.0 or +0.0, and the centre is 1.0 - (+0.0) as numpy's sum leaves it"""
    means, good = random_tables(7, 2, 2)
    for e in ("aH", "aV", "aD"):
        means[e][:] = -0.0
    want = gr.derive(means, good, (16, 20))
    got = calfiles.derive_gain_ipc4d(means, good, shape=(16, 20), ctx=gpu_context())
    check_all(got, want, "negative zeros")
    assert np.signbit(got[2][0, 1, 1:]).all() and (got[2][1, 1] == 1.0).all()


@pytest.mark.parametrize("ipc_dtype", [np.float64, np.float32])
def test_full_frame_strips(ipc_dtype):
    """4096 x 4096 with 32 x 32 superpixels, resident: strips copied back against the restatement evaluated for those rows --
    the first and last 8 active rows, 4 rows either side of two superpixel seams, and the first and last 8 columns (and the
    columns around two seams) of 64 other rows."""
    import torch

    n, nb = 4096, 4
    means, good = random_tables(77, 32, 32, bad=[(0, 0), (17, 5), (31, 31)])
    ctx = gpu_context()
    gain, gain_dq, K, kdq = calfiles.derive_gain_ipc4d(means, good, shape=(n, n), nb=nb, ipc_dtype=ipc_dtype, on_device=True, ctx=ctx)
    na = n - 2 * nb
    assert K.shape == (3, 3, na, na) and K.dtype == np.dtype(ipc_dtype) and kdq.shape == (na, na)
    seam1, seam2 = 128 - nb, 2048 - nb   # first active row of the superpixel rows 1 and 16
    rows = np.r_[0:8, na - 8:na, seam1 - 4:seam1 + 4, seam2 - 4:seam2 + 4]
    got = K.t[:, :, torch.as_tensor(rows, device=K.t.device)].cpu().numpy()
    assert_same_bits(got, gr.ipc4d(means, (n, n), nb, ipc_dtype, rows=rows), "whole rows")
    others = np.arange(64) * 61 + 200   # 64 rows spread over the frame, none of the above
    cols = np.r_[0:8, na - 8:na, seam1 - 4:seam1 + 4, seam2 - 4:seam2 + 4]
    sub = K.t[:, :, torch.as_tensor(others, device=K.t.device)][..., torch.as_tensor(cols, device=K.t.device)].cpu().numpy()
    want = gr.ipc4d(means, (n, n), nb, ipc_dtype, rows=others)[..., cols]
    assert_same_bits(sub, want, "columns of other rows")
    for strip in (got, sub):   # charge is conserved: the nine planes sum to 1
        total = strip.astype(np.float64).sum(axis=(0, 1))
        assert np.abs(total - 1.0).max() <= 2 * np.finfo(ipc_dtype).eps
    assert not bool(kdq.t.any())
    g_ref, dq_ref = gr.gain_planes(means, good, (n, n), nb)
    assert_same_bits(gain.numpy(), g_ref, "full-frame gain")
    assert_same_bits(gain_dq.numpy(), dq_ref, "full-frame gain dq")


def test_refusals_leave_the_context_usable():
    g, means, good, shape = fixture("gainfile_odd")
    ctx = gpu_context()
    want = (g["gain"], g["gain_dq"], g["kernel"], g["kernel_dq"])

    def call(means=means, good=good, **kw):
        kw = dict(dict(shape=shape, nb=gc.NB, ctx=ctx), **kw)
        return calfiles.derive_gain_ipc4d(means, good, **kw)

    none = {e: np.zeros((0, 3)) for e in gr.NAMES}
    bad = {
        "no superpixel row": (dict(means=none, good=np.zeros((0, 3), bool)), "a table of 0 x 3 superpixels"),
        "no superpixel column": (dict(means={e: np.zeros((5, 0)) for e in gr.NAMES}, good=np.zeros((5, 0), bool)), "a table of 5 x 0"),
        "rows not tiled": (dict(shape=(46, 45)), "do not tile a 46 x 45 frame"),
        "columns not tiled": (dict(shape=(45, 44)), "do not tile a 45 x 44 frame"),
        "border eats the frame": (dict(nb=23), "no active pixel"),
        "negative border": (dict(nb=-1), "no active pixel"),
        "float16 kernel": (dict(ipc_dtype=np.float16), "neither RIP_F32 nor RIP_F64"),
        "nothing wanted": (dict(outputs=()), "every output is NULL"),
    }
    for what, (kw, text) in bad.items():
        with pytest.raises(ValueError, match=text):
            call(**kw)
        assert text in ctx.lib.rip_last_error(ctx.h).decode(), what
        check_all(call(), want, f"a valid call after '{what}'")
    # the dtype code at the C interface itself
    t = np.ascontiguousarray([means[e] for e in gr.NAMES])
    gd = good.astype(np.uint8)
    out = np.empty((3, 3, 37, 37))
    rc = ctx.lib.rip_cal_gain_ipc4d(ctx.h, t.ctypes.data, gd.ctypes.data, 5, 3, 45, 45, 4, _native.RIP_HOST, None, None, out.ctypes.data,
                                    _native.RIP_U16, None)
    assert rc == -1 and "neither RIP_F32 nor RIP_F64" in ctx.lib.rip_last_error(ctx.h).decode()
    check_all(call(), want, "a valid call after a refused dtype code")


def test_drop_in_files(tmp_path):
    """make_gain_file.run on the gainfile_even tables written as the text files the script reads: names, trees, dtypes, notes,
    printed lines and bits"""
    name, sca = "gainfile_even", 7
    g, means, good, shape = fixture(name)
    ctx = gpu_context()
    listfile, paths, notes = gc.write_summaries(str(tmp_path), name)
    (tmp_path / "with_gain_dir").mkdir()
    outfile = str(tmp_path / "with_gain_dir" / "roman_wfi_gain_TEST_SCA07.asdf")
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        files = make_gain_file.run(listfile, sca, outfile, shape=shape, ctx=ctx)
    assert files == (outfile, str(tmp_path / "with_gain_dir") + "/roman_wfi_ipc4d_TEST_SCA07.asdf")   # the directory keeps its name
    lines = out.getvalue().split("\n")
    assert lines[:3] == paths and lines[3:5] == ["superpixels 4 10", "repeat 35 14"]
    text = out.getvalue()
    tmean = dict(zip(gr.NAMES, g["tmean"]))
    assert "--> 39 good pixels\n" in text and f"mean values {tmean}\n" in text and f"--\n{notes}\n--\n" in text
    gt, kt = (calio.read_asdf(p) for p in files)
    for tree, reftype in ((gt, "GAIN"), (kt, "IPC4D")):
        assert set(tree) >= {"roman", "notes"} and set(tree["roman"]) == {"meta", "data", "dq"}
        meta = tree["roman"]["meta"]
        assert meta["reftype"] == reftype and meta["instrument"] == {"detector": "WFI07", "name": "WFI"}
        assert meta["author"] == meta["description"] == "make_gain_file.py"
        assert set(meta) == {"author", "description", "instrument", "origin", "date", "pedigree", "reftype", "telescope", "useafter"}
        assert tree["notes"] == {"solid_waffle_config": notes}
    want = calfiles.derive_gain_ipc4d(means, good, shape=shape, ctx=ctx)
    check_all((gt["roman"]["data"], gt["roman"]["dq"], kt["roman"]["data"], kt["roman"]["dq"]), want, "files")
    check_all(want, (g["gain"], g["gain_dq"], g["kernel"], g["kernel_dq"]), "fixture")
    assert gt["roman"]["data"].dtype == np.float32 and gt["roman"]["data"].shape == shape and gt["roman"]["dq"].dtype == np.uint32
    assert kt["roman"]["data"].dtype == np.float64 and kt["roman"]["data"].shape == (3, 3, 132, 132)
    assert kt["roman"]["dq"].dtype == np.uint32 and kt["roman"]["dq"].shape == (132, 132)
    # the float32 option writes the kernel rounded once
    with contextlib.redirect_stdout(io.StringIO()):
        f32 = make_gain_file.run(listfile, sca, str(tmp_path / "f32_gain_X.asdf"), ipc_dtype=np.float32, shape=shape, ctx=ctx)
    assert_same_bits(calio.read_asdf(f32[1])["roman"]["data"], g["kernel"].astype(np.float32), "float32 file")
    # the script's frame is the H4RG's: these tables do not tile it, which is refused by name
    with contextlib.redirect_stdout(io.StringIO()), pytest.raises(ValueError, match="do not tile a 4096 x 4096 frame"):
        make_gain_file.run(listfile, sca, str(tmp_path / "full_gain_X.asdf"), ctx=ctx)


@pytest.mark.parametrize("ipc_dtype", [np.float64, np.float32])
def test_derived_files_serve_calibrateimage(tmp_path, ipc_dtype):
    """a 48 x 256 synthetic CALDIR whose gain and ipc4d files are derived at that shape from summary files"""
    from romanimpreprocess_amd.L1_to_L2 import gen_cal_image

    ctx = gpu_context()
    rp = synth.READ_PATTERN_6
    ny, nx, sca, p_order = 48, 256, 4, 3
    cal = synth.make_caldir(ny, nx, read_pattern=rp, p_order=p_order, seed=41)
    stem = str(tmp_path / "roman_wfi_{}_TEST_SCA04.asdf")
    for key in ("dark", "read", "linearitylegendre", "biascorr", "mask", "saturation", "flat"):
        calio.write_asdf(stem.format(key), {"roman": cal[key]})
    nsy, nsx = 4, 8
    means, good = random_tables(91, nsy, nsx, bad=[(2, 5)])
    sy, sx = np.divmod(np.arange(nsy * nsx), nsx)
    table = np.zeros((nsy * nsx, gc.NCOL))
    table[:, 0], table[:, 1], table[:, 2] = sx, sy, np.where(good.ravel(), 500, 0)
    for e in gr.NAMES:
        table[:, gr.COLS[e]] = means[e].ravel()
    np.savetxt(str(tmp_path / "sw_summary.txt"), table, fmt="%.17e")
    (tmp_path / "sw_config.txt").write_text("DETECTOR: SCA04\n")
    (tmp_path / "list.txt").write_text(str(tmp_path / "sw_summary.txt") + "\n")
    with contextlib.redirect_stdout(io.StringIO()):
        gfile, kfile = make_gain_file.run(str(tmp_path / "list.txt"), sca, stem.format("gain"), ipc_dtype=ipc_dtype, shape=(ny, nx), ctx=ctx)
    assert kfile == stem.format("ipc4d")
    m2, g2, _ = gr.summary_means(table[None])
    want = gr.derive(m2, g2, (ny, nx), ipc_dtype=ipc_dtype)
    gt, kt = calio.read_asdf(gfile)["roman"], calio.read_asdf(kfile)["roman"]
    check_all((gt["data"], gt["dq"], kt["data"], kt["dq"]), want, "derived files")
    code = {np.float32: _native.RIP_F32, np.float64: _native.RIP_F64}[ipc_dtype]
    assert _native.chain_form_for(p_order + 1, len(rp), code, _native.RIP_F32) == 2   # the fused form serves these dtypes

    ramp = synth.make_ramp(cal, read_pattern=rp, seed=42, cr_frac=0.02)
    calio.write_asdf(str(tmp_path / "l1.asdf"), {"roman": {"data": ramp["data"], "amp33": ramp["amp33"], "meta": {
        "exposure": {"frame_time": synth.FRAME_TIME, "read_pattern": rp}, "instrument": {"detector": "WFI04"}}}})
    caldir = {k: stem.format(k) for k in ("dark", "read", "gain", "linearitylegendre", "ipc4d", "biascorr", "mask", "saturation", "flat")}
    config = {"IN": str(tmp_path / "l1.asdf"), "OUT": str(tmp_path / "l2.asdf"), "CALDIR": caldir,
              "JUMP_DETECT_PARS": {"SthreshA": 5.0, "IthreshB": 800.0}}
    gen_cal_image.calibrateimage(config, verbose=False, calibrator=pipeline.Calibrator(ctx=ctx))
    l2 = calio.read_asdf(config["OUT"])["roman"]
    assert l2["data"].shape == (ny - 8, nx - 8) and l2["data"].dtype == np.float32 and np.isfinite(l2["data"]).mean() > 0.9
