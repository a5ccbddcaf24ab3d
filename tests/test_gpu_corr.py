"""The pair statistics on the device (csrc/corrstat.hip, calfiles/corrstack.py, calfiles/correlation_run.py) against the numpy
restatement tests/corr_ref.py: every int64 of the table equal, at the shapes of tests/corr_cases.py; every refusal before a
launch; and one round trip through the package's own generator (L1Synth), whose planted gain and couplings come back within
five standard errors formed from the planted values (corr_ref.standard_errors)."""

import contextlib
import io

import corr_cases as cc
import corr_ref as ref
import darkstack_cases as dc
import numpy as np
import pytest
from conftest import gpu_context

from romanimpreprocess_amd import _native, calio
from romanimpreprocess_amd.calfiles import CorrStack, correlation_run, derive_gain_ipc4d, solve_summary
from romanimpreprocess_amd.calfiles.corrstack import frame_times
from romanimpreprocess_amd.devarray import DevArray
from romanimpreprocess_amd.from_sim import sim_to_isim

pytestmark = pytest.mark.gpu


def dev16(a, offset=0):
    """a cube of 16-bit words in HBM under the dtype of its samples, its first sample ``offset`` samples off the allocation"""
    import torch

    flat = torch.zeros(a.size + 8, dtype=torch.int16, device="cuda")
    flat[offset:offset + a.size] = torch.from_numpy(np.array(a, order="C").view(np.int16).reshape(-1)).cuda()   # (a writable copy)
    arr = DevArray(flat[offset:offset + a.size].view(a.shape), np.uint16 if a.dtype == np.uint16 else np.int16)
    assert (arr.ctypes.data % 16 == 0) == (offset % 8 == 0)
    return arr


def same_table(got, want, what):
    assert got.dtype == np.int64 and got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} words differ; first at (iy, ix, slot) {tuple(bad[0])}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


def device_table(name, cubes=None, fits_be16=False):
    c = cc.CASES[name]
    a, b = cc.pair(name) if cubes is None else cubes
    st = CorrStack(c[8], c[3], c[4], (c[4] // c[7], c[3] // c[6]), nb=c[5], ctx=gpu_context())
    out = st.add_pair(a, b, fits_be16=fits_be16)
    assert st.count == 1 and st.table().shape == (1, c[3] // c[6], c[4] // c[7], 25) and np.array_equal(st.table()[0], out)
    return out


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_table_equals_the_restatement(name):
    want = cc.expected(name)
    same_table(device_table(name), want, name)
    # what the case is there for
    if name == "all_border":
        assert not want[0].any() and not want[:, 0].any() and not want[3].any() and not want[:, 3].any() and want[1, 1, 0] > 0
    if name == "rows":
        assert not want[0].any() and not want[7].any() and (want[1:7, 0, 3] > 100).all() and not want[1:7, 0, 7:19].any()
    if name == "extremes":
        assert want[0, 0, 0] == 16384 and want[0, 0, 2] == 16384 * 131070**2 > 2**47 and want[0, 0, 6] == -(128 * 127) * 131070**2
        assert want[0, 0, 22] == -131070 and want[0, 0, 24] == 131070
    if name == "outliers":   # 3, 4, 2 and 3 outliers in the four superpixels, none kept
        assert np.array_equal(want[..., 0], 28 * 28 - np.array([[3, 4], [2, 3]]))
        # superpixel (1, 1), shift (0, 1): the corner pixel loses one pair, the edge and the interior pixel two each
        assert want[1, 1, 3] == 28 * 27 - 5
        # two hot neighbours would give a product of 2.5e7: no sum holds one
        assert np.abs(want[..., [6, 10, 14, 18]]).max() < 1e6
    if name == "constant":
        assert (want[..., 0] == 12 * 12).all() and (want[..., 3] == 12 * 11).all() and (want[..., 15] == 11 * 11).all()
        assert not want[..., [1, 2, 4, 5, 6, 19, 20, 21, 22, 23, 24]].any()
    if name == "ties":   # some superpixels have q75 = q25 and keep only the pixels at the median
        assert set(np.unique(want[..., 22:])) <= {-1, 0, 1} and want[..., 0].min() < 50 < 100 < want[..., 0].max()


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("fits", [False, True])
def test_host_and_hbm_cubes_native_and_fits_storage(device, fits):
    name = "crop_w8"
    a, b = cc.pair(name)
    if fits:
        a, b = ref.to_fits_storage(a), ref.to_fits_storage(b)
        assert np.array_equal(ref.native(a, True), cc.pair(name)[0])
    if device:
        a, b = dev16(a), dev16(b)
    same_table(device_table(name, (a, b), fits), cc.expected(name), f"device {device} fits {fits}")


def test_one_cube_in_host_memory_and_one_in_hbm_and_a_leading_axis():
    name = "crop_w8"
    a, b = cc.pair(name)
    same_table(device_table(name, (a[None], dev16(b))), cc.expected(name), "host + HBM")
    same_table(device_table(name, (dev16(a), b)), cc.expected(name), "HBM + host")


@pytest.mark.parametrize("name", ["border_inside", "crop_w8"])
def test_one_sample_per_lane_from_a_cube_that_is_not_aligned(name):
    a, b = cc.pair(name)
    same_table(device_table(name, (dev16(a, 1), dev16(b, 1))), cc.expected(name), "both off by one sample")
    same_table(device_table(name, (dev16(a), dev16(b, 3))), cc.expected(name), "the second off by three")


def test_every_refusal_by_name_before_any_launch():
    ctx = gpu_context()
    a, b = cc.pair("crop_w8")
    table = np.full((2, 2, 25), -7, np.int64)
    ok = dict(cube1=a, location1=_native.RIP_HOST, cube2=b, location2=_native.RIP_HOST, nreads=6, ny_file=64, nx_file=72, fits_be16=0,
              fa=1, fb=2, fc=3, fd=5, ny=64, nx=64, nb=4, sy=32, sx=32, table=table, table_location=_native.RIP_HOST)
    for kw, text in (({"cube1": None}, "NULL"), ({"cube2": None}, "NULL"), ({"table": None}, "NULL"), ({"location1": 7}, "location1 7"),
                     ({"location2": 9}, "location2 9"), ({"table_location": 5}, "table_location 5"), ({"nreads": 0}, r"\(0,64,72\) cube"),
                     ({"fd": 6}, "TIME 2 3 4 7 .*outside a cube of 6"), ({"fa": -1}, "TIME 0 3 4 6"), ({"nreads": 5}, "TIME 2 3 4 6 .*cube of 5"),
                     ({"fb": 1}, "TIME 2 2 4 6"), ({"fc": 5}, "TIME 2 3 6 6"), ({"fa": 5, "fb": 5, "fd": 4}, "TIME 6 6 4 5"),
                     ({"fa": 4, "fb": 5, "fc": 1, "fd": 2}, "TIME 5 6 2 3"), ({"ny": 65}, r"frame of \(65,64\)"), ({"nx": 80}, r"frame of \(64,80\)"),
                     ({"ny": 0}, r"frame of \(0,64\)"), ({"nb": -1}, "border of -1"), ({"sy": 24}, r"NBIN: superpixels of \(24,32\)"),
                     ({"sx": 0}, r"NBIN: superpixels of \(32,0\)"), ({"sx": 48}, r"NBIN: superpixels of \(32,48\)")):
        with pytest.raises(ValueError, match=text):
            ctx.call("rip_cal_corr_pair", *dict(ok, **kw).values())
        assert (table == -7).all(), kw   # nothing was launched or copied
    # a superpixel above 16384 pixels: 128 x 136
    big = np.zeros((4, 128, 136), np.uint16)
    with pytest.raises(ValueError, match=r"NBIN: a superpixel of \(128,136\) has 17408 pixels \(at most 16384"):
        ctx.call("rip_cal_corr_pair", *dict(ok, cube1=big, cube2=big, nreads=4, ny_file=128, nx_file=136, fa=0, fb=1, fc=2, fd=3, ny=128, nx=136,
                                            sy=128, sx=136).values())
    assert (table == -7).all()
    ctx.call("rip_cal_corr_pair", *ok.values())
    same_table(table, cc.expected("crop_w8"), "the call that is in order")
    # the Python layer
    for kw, text in (({"frames": (1, 1, 3, 5)}, "TIME 2 2 4 6"), ({"nbin": (3, 2)}, "NBIN 3 2"), ({"nbin": (1, 1), "ny": 256, "nx": 256}, "NBIN 1 1")):
        with pytest.raises(ValueError, match=text):
            CorrStack(**dict(dict(frames=(1, 2, 3, 5), ny=64, nx=64, nbin=(2, 2), nb=4, ctx=ctx), **kw))
    st = CorrStack((1, 2, 3, 5), 64, 64, (2, 2), ctx=ctx)
    with pytest.raises(ValueError, match="pair are"):
        st.add_pair(a, b[:5])
    with pytest.raises(TypeError, match="16-bit"):
        st.add_pair(a.astype(np.float32), b)
    with pytest.raises(TypeError, match="fits_be16"):
        st.add_pair(ref.to_fits_storage(a), b)
    with pytest.raises(ValueError, match="TIME 2 3 4 6 .*cube of 5"):
        st.add_pair(a[:5], b[:5])
    with pytest.raises(ValueError, match=r"frame of \(64,64\)"):   # a file smaller than the frame, by the library
        st.add_pair(a[:, :60], b[:, :60])
    assert st.count == 0 and st.table().shape == (0, 2, 2, 25)


# ------------------------------------------------------------------------------------------------ the round trip
NY = NX = 256
NB = 4
G = np.array([[1.8, 1.5], [1.6, 2.0]])
AH = np.array([[0.030, 0.006], [0.015, 0.020]])   # (0, 0) and (0, 1) swap alphaH and alphaV: a transposed shift fails
AV = np.array([[0.006, 0.030], [0.010, 0.014]])
AD = np.full((2, 2), 0.003)
KAPPA, SREF, SMIN, SMAX = 4.0e-6, 5000.0, 2000.0, 14000.0
READ_NOISE = 7.0
RATE, DARK_RATE = 600.0, 2.0


def planted_caldir(ctx):
    """the CALDIR arrays of L1Synth from the planted superpixel table: gain and ipc4d by derive_gain_ipc4d, an order-2 linearity
    phi(S) = (S - Sref) + kappa (S - Sref)^2 written in Legendre polynomials of z = (S - Smin) / h - 1, h = (Smax - Smin) / 2:
    with d = Smin + h - Sref, phi = (d + kappa d^2 + kappa h^2 / 3) P0 + (h + 2 kappa h d) P1 + (2 kappa h^2 / 3) P2"""
    means = {"g": G, "aH": AH, "aV": AV, "aD": AD}
    gain, _, kernel, _ = derive_gain_ipc4d(means, np.ones((2, 2), bool), shape=(NY, NX), nb=NB, ctx=ctx)
    h = (SMAX - SMIN) / 2.0
    d = SMIN + h - SREF
    coef = (d + KAPPA * d * d + KAPPA * h * h / 3.0, h + 2.0 * KAPPA * h * d, 2.0 * KAPPA * h * h / 3.0)
    plane = lambda v, dt=np.float32: np.full((NY, NX), v, dt)   # noqa: E731
    return {"gain": {"data": gain}, "ipc4d": {"data": kernel},
            "read": {"data": plane(READ_NOISE), "resetnoise": plane(0.0)},
            "dark": {"data": np.zeros((cc.NREADS, NY, NX), np.float32), "dark_slope": plane(0.0)},
            "linearitylegendre": {"data": np.stack([plane(c) for c in coef]), "Smin": plane(SMIN), "Smax": plane(SMAX), "Sref": plane(SREF),
                                  "dq": plane(0, np.uint32)}}


@pytest.fixture(scope="module")
def exposures():
    """10 light and 10 dark exposures of the planted set from L1Synth.make, uint16 DevArray cubes (16, 256, 256)"""
    ctx = gpu_context()
    l_max = RATE * (cc.NREADS - 1) / G.min()
    assert KAPPA * l_max <= 0.03   # the neglected second-order terms, at most 4 (kappa L)^2, stay below one standard error
    synth = sim_to_isim.L1Synth(planted_caldir(ctx), [[k] for k in range(cc.NREADS)], 3.04, ctx=ctx, nb=NB)
    out = []
    for rate, seed0 in ((RATE, 1000), (DARK_RATE, 2000)):
        counts = np.full((NY - 2 * NB, NX - 2 * NB), rate * (cc.NREADS - 1), np.float32)
        out.append([DevArray(synth.make(counts, seed0 + j, poisson=True, banding=False)[0], np.uint16) for j in range(10)])
    return out


def stacked(exposures):
    ctx = gpu_context()
    tabs = []
    for cubes in exposures:
        st = CorrStack(cc.FRAMES, NY, NX, (2, 2), nb=NB, ctx=ctx)
        for j in range(0, 10, 2):
            st.add_pair(cubes[j], cubes[j + 1])
        tabs.append(st.table())
    return tabs


def superpixel_errors(light, iy, ix):
    times = frame_times(cc.FRAMES, cc.TIMEREF)
    g, aH, aV, aD = G[iy, ix], AH[iy, ix], AV[iy, ix], AD[iy, ix]
    mom = [ref.expected_moments(r, g, aH, aV, aD, KAPPA / g, READ_NOISE, times) for r in (RATE, DARK_RATE)]
    n = int(light[:, iy, ix, 0].sum())
    m = [int(light[:, iy, ix, 3 + 4 * s].sum()) for s in range(4)]
    return ref.standard_errors(solve_summary, mom[0], mom[1], n, m, cc.FRAMES, cc.TIMEREF)


def test_round_trip_through_the_generator(exposures, tmp_path):
    ctx = gpu_context()
    light, dark = stacked(exposures)
    # the device table of the generator's cubes is the restatement's too
    same_table(light[0], ref.pair_table(exposures[0][0].numpy(), exposures[0][1].numpy(), cc.FRAMES, NY, NX, NB, 128, 128), "first light pair")
    table = solve_summary(light, dark, cc.FRAMES, cc.TIMEREF)
    assert table.shape == (4, 11)
    ses = {}
    for iy in range(2):
        for ix in range(2):
            row = table[iy * 2 + ix]
            ideal, se = superpixel_errors(light, iy, ix)
            ses[iy, ix] = se
            assert row[0] == ix and row[1] == iy and row[2] > 0.99 * 124 * 124
            print(f"superpixel ({iy},{ix}): beta {row[8]:.4g} (kappa / g = {KAPPA / G[iy, ix]:.4g}), I {row[9]:.5g}")
            for name, col, want in (("g", 5, G), ("aH", 6, AH), ("aV", 7, AV), ("aD", 10, AD)):
                print(f"  {name}: got {row[col]:.6g}, planted {want[iy, ix]:.6g}, se {se[col]:.3g}, off by {(row[col] - want[iy, ix]) / se[col]:+.2f} se")
                assert abs(row[col] - want[iy, ix]) <= cc.NSIGMA * se[col], (name, iy, ix)
    # a transposed shift or a swapped row order would land more than five standard errors off
    assert abs(AH[0, 0] - AV[0, 0]) > 2 * cc.NSIGMA * ses[0, 0][6] and abs(G[0, 0] - G[0, 1]) > 2 * cc.NSIGMA * ses[0, 0][5]

    # the job's lines 48-71 on FITS files written from those cubes
    text = cc.config_text(target=str(tmp_path), sca=7, estart=1, eend=10, nbin=(2, 2), output=str(tmp_path / "sw-SCA07-E001"))
    cfg = correlation_run.parse_config(text)
    for files, cubes in ((cfg.light, exposures[0]), (cfg.dark, exposures[1])):
        for path, cube in zip(files, cubes):
            dc.write_dark_fits(path, cube.numpy())
    (tmp_path / "config1_07.txt").write_text(text)
    outfile = str(tmp_path / "roman_wfi_gain_T_SCA07.asdf")
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        files = correlation_run.gain_from_flats([str(tmp_path / "config1_07.txt")], 7, outfile, ctx=ctx, nside=NX, nb=NB)
    assert files == (outfile, str(tmp_path / "roman_wfi_ipc4d_T_SCA07.asdf"))
    for key in ("CHAR", "FULLNL", "NLPOLY", "IPCSUB", "HOTPIX"):
        assert f"{key}: " in log.getvalue() and "not acted on" in log.getvalue()
    back = np.loadtxt(str(tmp_path / "sw-SCA07-E001_summary.txt"))
    assert np.array_equal(back, table)   # files in FITS storage and cubes in HBM: the same sums, the same table
    assert (tmp_path / "sw-SCA07-E001_config.txt").read_text() == text
    tree = calio.roman_branch(outfile)
    gain = np.asarray(tree["data"])
    assert gain.shape == (NY, NX) and not gain[:NB].any() and not gain[:, -NB:].any()
    for iy in range(2):
        for ix in range(2):
            block = gain[max(iy * 128, NB):min((iy + 1) * 128, NY - NB), max(ix * 128, NB):min((ix + 1) * 128, NX - NB)]
            assert (block == np.float32(table[iy * 2 + ix, 5])).all()
            assert abs(float(block[0, 0]) - G[iy, ix]) <= cc.NSIGMA * ses[iy, ix][5]
    kernel = np.asarray(calio.roman_branch(files[1])["data"])
    assert kernel.shape == (3, 3, NY - 2 * NB, NX - 2 * NB) and kernel[1, 2, 50, 50] == np.float64(np.float32(table[0, 6]))
