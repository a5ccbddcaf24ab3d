"""The linearitylegendre derivation on the device (csrc/linfit.hip, romanimpreprocess_amd/calfiles/linfit.py, linearity_run.py)
against tests/linfit_ref.py: the frame sums exactly, every plane of the fit bit for bit (floats as bit patterns) on the table of
tests/linfit_cases.py, whose coverage tests/test_host_linfit.py counts with the restatement."""

import ctypes as C
import json

import calfiles_ref as cr
import linfit_cases as cases
import linfit_ref as ref
import numpy as np
import pytest
from conftest import assert_same_bits, gpu_context

from romanimpreprocess_amd import _native, calfiles, calio
from romanimpreprocess_amd.calfiles import RampStack, derive_linearity, linearity_run
from romanimpreprocess_amd.devarray import DevArray, is_dev, to_device
from romanimpreprocess_amd.utils import ipc_linearity

pytestmark = pytest.mark.gpu

PLANES = ("data", "Smin", "Smax", "dq", "pflat", "dark", "ramperr", "cut")
_REF = {}


def fit_ref(nsets, tstart, p):
    if (nsets, tstart, p) not in _REF:
        sums, counts, first, sref, dark = cases.fit_inputs(nsets, tstart)
        _REF[(nsets, tstart, p)] = ref.fit(sums, counts, first, sref, p_order=p, nb=cases.NB, bright=0, dark=dark)
    return _REF[(nsets, tstart, p)]


def fit_dev(nsets, tstart, p, **kw):
    sums, counts, first, sref, dark = cases.fit_inputs(nsets, tstart)
    return derive_linearity(list(zip(sums, counts)), sref, p_order=p, tstart=tstart, dark=None if dark < 0 else dark, nb=cases.NB,
                            ctx=gpu_context(), **kw)


def same_planes(got, want, what):
    for k in PLANES:
        assert_same_bits(got[k].numpy() if is_dev(got[k]) else got[k], want[k], f"{what} {k}")


def dev16(a):
    """a cube of 16-bit words in HBM under the dtype of its samples (uint16, or int16 for FITS storage)"""
    import torch

    return DevArray(torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda(), np.uint16 if a.dtype == np.uint16 else np.int16)


def cube(seed, nreads, ny, width):
    a = np.random.default_rng(seed).integers(0, 65536, size=(nreads, ny, width)).astype(np.uint16)
    a[0, 0, :4] = a[-1, -1, -4:] = (0, 32767, 32768, 65535)
    a[:, 5, 8:12] = (0, 32767, 32768, 65535)
    return a


def stored(a):
    """the FITS storage of unsigned samples: big-endian int16 with BZERO 32768"""
    return (a.astype(np.int32) - 32768).astype(">i2")


# ------------------------------------------------------------------------------------------------ frame sums
@pytest.mark.parametrize("nx,width", [(72, 80), (64, 64), (70, 80), (13, 13)])
@pytest.mark.parametrize("on_device", [False, True])
def test_frame_sums(nx, width, on_device):
    """a crop with a partial wave (72 of 80), aligned rows (64), rows of sums off the 16-byte grid (70: element-wise stores of
    full and partial vectors), a width that takes the one-pixel kernel (13); native and FITS-storage samples; a row band; three
    exposures in two orders: the words of cube.astype(uint32).sum"""
    ctx = gpu_context()
    cubes = [cube(10 + j, 5, 12, width) for j in range(3)]
    for rows in (None, (3, 9)):
        y0, y1 = rows or (0, 12)
        want = sum(c[:, y0:y1, :nx].astype(np.uint32) for c in cubes)
        for order in ((0, 1, 2), (2, 0, 1)):
            for be in (False, True):
                st = RampStack(5, 12, nx, ctx=ctx, rows=rows)
                for j in order:
                    c = stored(cubes[j]) if be else cubes[j]
                    st.add(dev16(c) if on_device else c, fits_be16=be)
                assert st.count == 3
                assert_same_bits(st.sums.numpy(), want, f"rows {rows} order {order} be16 {be}")


@pytest.mark.parametrize("f0", [0, 2])
@pytest.mark.parametrize("location", ["host", "device", "device off the 16-byte grid"])
def test_frame_sums_entry(f0, location):
    """the C entry: the frames from f0 on, (1, N, ny, nx) cubes through the Python layer, a device cube whose first sample is not
    on a 16-byte boundary (the one-pixel kernel), sums that are added to"""
    import torch

    ctx = gpu_context()
    a = cube(3, 5, 12, 80)
    sums = to_device(np.full((5 - f0, 6, 72), 7, np.uint32))
    if location == "host":
        arg, where = a, _native.RIP_HOST
    else:
        off = 1 if "off" in location else 0
        flat = torch.zeros(a.size + 8, dtype=torch.int16, device="cuda")
        flat[off:off + a.size] = torch.from_numpy(a.view(np.int16).reshape(-1)).cuda()
        arg, where = DevArray(flat[off:off + a.size], np.uint16), _native.RIP_DEVICE
        assert (arg.ctypes.data % 16 != 0) == bool(off)
    ctx.call("rip_cal_frame_sums", arg, where, 5, 12, 80, 3, 6, 72, f0, 0, sums, 0)
    assert_same_bits(sums.numpy(), a[f0:, 3:9, :72].astype(np.uint32) + np.uint32(7))
    st = RampStack(5, 12, 72, ctx=ctx)
    st.add(a[None] if location == "host" else dev16(a[None]))
    assert_same_bits(st.sums.numpy(), a[:, :, :72].astype(np.uint32))


def test_frame_sums_refusals():
    ctx = gpu_context()
    a = cube(1, 5, 12, 80)
    sums = to_device(np.zeros((5, 12, 72), np.uint32))

    def call(nreads=5, ny_file=12, nx_file=80, y0=0, ny=12, nx=72, f0=0, count=0, where=_native.RIP_HOST):
        ctx.call("rip_cal_frame_sums", a, where, nreads, ny_file, nx_file, y0, ny, nx, f0, 0, sums, count)

    for kw, text in (({"count": 65536}, "exposure 65537"), ({"count": -1}, "exposure"), ({"nx": 81}, "81 columns"), ({"y0": 7}, "rows 7"),
                     ({"y0": -1}, "rows -1"), ({"ny": 13}, "rows 0"), ({"f0": 5}, "first frame 5"), ({"f0": -1}, "first frame -1"),
                     ({"where": 9}, "location 9")):
        with pytest.raises(ValueError, match=text):
            call(**kw)
    assert not sums.numpy().any()   # a refused call has written nothing
    call(count=65535)   # the last exposure a set can take
    assert_same_bits(sums.numpy(), a[:, :, :72].astype(np.uint32))
    st = RampStack(5, 12, 72, ctx=ctx)
    with pytest.raises(ValueError):
        st.add(a[:4])
    with pytest.raises(TypeError):
        st.add(a.astype(np.float32))
    with pytest.raises(TypeError):
        st.add(stored(a))   # FITS storage without saying so
    assert st.count == 0 and not st.sums.numpy().any()


# ------------------------------------------------------------------------------------------------ the fit
@pytest.mark.parametrize("nsets,tstart,p", cases.FIT_CASES)
def test_fit_equals_the_restatement(nsets, tstart, p):
    """orders 1, 2, 3, 8, 10; one set (no dark), two and three; TSTART 1 and 3; set lengths 5, 12, 7: every plane bit for bit"""
    same_planes(fit_dev(nsets, tstart, p), fit_ref(nsets, tstart, p), f"{nsets} sets, TSTART {tstart}, order {p}:")


def test_fit_table_covers_every_kind():
    total = dict.fromkeys(cases.KINDS, 0)
    for nsets, tstart, p in cases.FIT_CASES:
        sums, counts, first, sref, dark = cases.fit_inputs(nsets, tstart)
        for k, n in cases.kinds_of(fit_ref(nsets, tstart, p), sums, counts, first, sref, dark, p).items():
            total[k] += n
    print(total)
    assert not [k for k, n in total.items() if n == 0]


def test_fit_is_deterministic():
    a, b = fit_dev(3, 3, 8), fit_dev(3, 3, 8)
    same_planes(a, {k: b[k].numpy() for k in PLANES}, "second call:")


def test_fit_of_a_row_band():
    """the stacks and Sref of rows 3..9: the planes of those rows of the whole frame, the border taken from the frame"""
    sums, counts, first, sref, dark = cases.fit_inputs(3, 3)
    got = derive_linearity([(s[:, 3:9], c) for s, c in zip(sums, counts)], sref[3:9], p_order=8, tstart=3, dark=dark, nb=cases.NB,
                           rows=(3, cases.NY), ctx=gpu_context())
    want = fit_ref(3, 3, 8)
    same_planes(got, {k: np.ascontiguousarray(want[k][..., 3:9, :]) for k in PLANES}, "rows 3..9:")
    top = derive_linearity([(s[:, :3], c) for s, c in zip(sums, counts)], sref[:3], p_order=8, tstart=3, dark=dark, nb=cases.NB,
                           rows=(0, cases.NY), ctx=gpu_context())
    assert_same_bits(top["dq"].numpy(), want["dq"][:3])


@pytest.mark.parametrize("p", sorted(cases.RECORDED_ERROR))
def test_recovery_on_the_device(p):
    """the host recovery case at n = 4096, sums handed in directly: the same recorded bound, and the restatement's bits"""
    sums, counts, first, sref = cases.recovery_sums(4096)
    got = derive_linearity(list(zip(sums, counts)), sref, p_order=p, tframe=cases.TFRAME, tstart=cases.TSTART, dark=-1, nb=0,
                           ctx=gpu_context())
    out = {k: got[k].numpy() for k in PLANES}
    err = cases.recovery_error(out, sums, counts, first)
    print(f"order {p}: max error {err:.6f} DN_lin, recorded {cases.RECORDED_ERROR[p]}")
    assert out["dq"][0, 0] == 0 and out["cut"][0, 0] == 42
    assert err <= 2.0 * cases.RECORDED_ERROR[p]
    same_planes(out, ref.fit(sums, counts, first, sref, p_order=p, tframe=cases.TFRAME, nb=0, bright=0, dark=2), f"order {p}:")


def test_fit_refusals_name_the_key():
    ctx = gpu_context()
    sums, counts, first, sref, dark = cases.fit_inputs(3, 3)
    stacks = list(zip(sums, counts))
    for kw, text in (({"p_order": 0}, "P_ORDER 0"), ({"p_order": 11}, "P_ORDER 11"), ({"sign": -1}, "SIGN -1"), ({"slopecut": 0.0}, "SLOPECUT"),
                     ({"slopecut": 1.0}, "SLOPECUT"), ({"slopecut": float("nan")}, "SLOPECUT"), ({"dark": 3}, "DARK 3"),
                     ({"dark": -4}, "DARK -4"), ({"bright": 3}, "bright set 3"), ({"bright": 2}, "bright set 2"),
                     ({"tstart": 5}, "TSTART 5"), ({"tstart": (1, 12, 1)}, "TSTART 12"), ({"tstart": 0}, "TSTART 0"),
                     ({"tframe": 0.0}, "TFRAME"), ({"negativepad": -1.0}, "NEGATIVEPAD")):
        with pytest.raises(ValueError, match=text):
            derive_linearity(stacks, sref, **{"ctx": ctx, "dark": dark, **kw})
    with pytest.raises(ValueError, match="RAMPS holds 9 sets"):
        derive_linearity(stacks * 3, sref, ctx=ctx)
    with pytest.raises(ValueError, match="NRAMP 65537"):
        derive_linearity([(sums[0], 65537)], sref, dark=None, ctx=ctx)
    # the entry itself: nine sets, an index outside them
    d = {k: to_device(v) for k, v in fit_ref(3, 3, 8).items() if k in PLANES}
    s9 = [to_device(sums[0])] * 9
    ptrs = (C.c_void_p * 9)(*[a.ctypes.data for a in s9])
    tables = [np.full(9, 3, np.int32), np.zeros(9, np.int32), np.full(9, 5, np.int32)]

    def entry(nsets, dark):
        ctx.call("rip_cal_linearity_fit", nsets, ptrs, *tables, to_device(sref), cases.NY, cases.NX, 0, cases.NY, 2, 8, 1, 3.04, 0.5,
                 500.0, 0, dark, d["data"], d["Smin"], d["Smax"], d["dq"], d["pflat"], d["dark"], d["ramperr"], d["cut"])

    with pytest.raises(ValueError, match="RAMPS holds 9 sets"):
        entry(9, -1)
    with pytest.raises(ValueError, match="DARK -2"):
        entry(3, -2)
    with pytest.raises(TypeError):
        derive_linearity([(sums[0].astype(np.int64), 3)], sref, dark=None, ctx=ctx)


# ------------------------------------------------------------------------------------------------ the planes go on in HBM
def test_planes_feed_the_derived_files():
    """derive_saturation and derive_mask on the DevArray planes of derive_linearity: what the numpy planes give"""
    ctx = gpu_context()
    out = fit_dev(3, 3, 8)
    want = fit_ref(3, 3, 8)
    sref = cases.fit_inputs(3, 3)[3]
    sat, sdq = calfiles.derive_saturation(out["Smax"], out["Sref"], ctx=ctx)
    assert is_dev(sat) and is_dev(sdq)
    rsat, rsdq = calfiles.derive_saturation(want["Smax"], sref, ctx=ctx)
    assert_same_bits(sat.numpy(), rsat)
    assert_same_bits(sdq.numpy(), rsdq)
    rng = np.random.default_rng(2)
    dark_slope = rng.uniform(0.0, 20.0, size=sref.shape).astype(np.float32)
    gain_dq = (rng.uniform(size=sref.shape) < 0.05).astype(np.uint32) << 19
    pf0 = DevArray(out["pflat"].t[0])
    mask = calfiles.derive_mask(out["dq"], pf0, to_device(dark_slope), to_device(gain_dq), nb=cases.NB, ctx=ctx)
    assert is_dev(mask)
    assert_same_bits(mask.numpy(), calfiles.derive_mask(want["dq"], want["pflat"][0], dark_slope, gain_dq, nb=cases.NB, ctx=ctx))
    assert_same_bits(mask.numpy(), cr.mask(want["dq"], want["pflat"][0], dark_slope, gain_dq, nb=cases.NB))


# ------------------------------------------------------------------------------------------------ the drop-in
def test_linearity_run(tmp_path, capsys):
    """three tiny sets as FITS files (the dark one in the summer2025 layout, 80 columns wide of which 72 are used), the JSON as
    write_linearity_config.pl writes it: the tree's keys, dtypes and shapes, the restatement's bits, and phi(Sref) = 0"""
    ctx = gpu_context()
    sets, sref = cases.exposures(3, 1, width=80)
    names = ("Flat", "LoFlat", "Noise")
    for k, cubes in enumerate(sets):
        for e, c in enumerate(cubes):
            path = str(tmp_path / f"99999999_SCA07_{names[k]}_{e + 1:03d}.fits")
            calio.write_fits(path, [None, np.ascontiguousarray(c[None])] if k == 2 else [c], ctx=ctx)
    calio.write_asdf(str(tmp_path / "roman_wfi_dark_T_SCA07.asdf"),
                     {"roman": {"data": np.stack([np.zeros_like(sref), sref])}})
    cfg = {"SCA": 7, "RAMPS": [{"FORMAT": 6 if k == 2 else 1, "FILE": str(tmp_path / f"99999999_SCA07_{names[k]}_001.fits"), "START": 1,
                                "NRAMP": len(sets[k]), "TSTART": 1} for k in range(3)],
           "DARK": -1, "TFRAME": 3.15625, "P_ORDER": 3, "OUTPUT": str(tmp_path / "roman_wfi_linearitylegendre_T_SCA07.asdf"), "SIGN": 1,
           "SLOPECUT": 0.5, "BIAS": {"FILE": str(tmp_path / "roman_wfi_dark_T_SCA07.asdf"), "PATH": ["roman", "data"], "SLICE": 1},
           "NEGATIVEPAD": 500}
    with open(tmp_path / "linearity_pars_07.json", "w") as f:
        json.dump(cfg, f, indent=0)
    outfile, dump = linearity_run.run(str(tmp_path / "linearity_pars_07.json"), nside=cases.NX, nb=cases.NB, ctx=ctx)
    capsys.readouterr()
    tree = calio.read_asdf(outfile)["roman"]
    ny, nx = cases.NY, cases.NX
    schema = {"data": (np.float32, (4, ny, nx)), "dq": (np.uint32, (ny, nx)), "Smin": (np.float32, (ny, nx)), "Smax": (np.float32, (ny, nx)),
              "Sref": (np.float32, (ny, nx)), "dark": (np.float32, (ny, nx)), "pflat": (np.float32, (2, ny, nx)),
              "ramperr": (np.uint16, (3, ny, nx))}
    assert set(tree) == set(schema) | {"meta"} and tree["meta"]["reftype"] == "LINEARITYLEGENDRE"
    assert tree["meta"]["instrument"]["detector"] == "WFI07"
    for k, (dt, shape) in schema.items():
        assert tree[k].dtype == dt and tree[k].shape == shape, k
    sums = [sum(c[:, :, :nx].astype(np.uint32) for c in cubes) for cubes in sets]
    want = ref.fit(sums, [len(c) for c in sets], [0, 0, 0], sref, p_order=3, tframe=3.15625, nb=cases.NB, bright=0, dark=2)
    for k in schema:
        assert_same_bits(np.asarray(tree[k]), sref if k == "Sref" else want[k], k)
    # two row bands give the same file
    cfg["OUTPUT"] = str(tmp_path / "banded.asdf")
    linearity_run.run(cfg, nside=cases.NX, nb=cases.NB, band_rows=7, ctx=ctx)
    capsys.readouterr()
    banded = calio.read_asdf(cfg["OUTPUT"])["roman"]
    for k in schema:
        assert_same_bits(np.asarray(banded[k]), np.asarray(tree[k]), f"banded {k}")
    # the dump of data, and the consumer's view: the linearised signal at Sref (as test_workflow.py:253-263 looks at a file)
    hdr, d = calio.read_fits_image(dump, 0)
    assert hdr["BITPIX"] == -32 and np.array_equal(np.asarray(d).astype(np.float32).view(np.uint32), tree["data"].view(np.uint32))
    good = tree["dq"] == 0
    assert np.count_nonzero(good) > 100
    sr = np.where(np.isfinite(sref), sref, 0).astype(np.float32)
    s0, _ = ipc_linearity.linearity(sr, outfile, ctx=ctx)
    # "0" as a float32 series gives it: p + 1 terms, each rounded, and z = 2 (S - Smin) / (Smax - Smin) - 1 a few ulp off, which
    # P_l turns into at most l (l + 1) / 2 times as much: (p + 1) (1 + p (p + 1)) ulp of the largest coefficient bound the sum
    bound = (3 + 1) * (1 + 3 * 4) * np.spacing(np.abs(tree["data"]).max(axis=0).astype(np.float32))
    print("phi(Sref): largest", np.abs(s0[good]).max(), "largest share of its bound", (np.abs(s0[good]) / bound[good]).max())
    assert np.all(np.abs(s0[good]) <= bound[good])
