"""The noise summary on the device (csrc/noisestat.hip, calfiles/noisestack.py, calfiles/noise_run.py) against its numpy restatement
tests/noise_run_ref.py: accumulators, row sums, moment tables and planes bit for bit (floats as bit patterns); the parameters at
1e-9 relative (the same tables through two numpy expressions differ by reordering only; sampling error is six orders above that);
the planted parameters of the round-trip case within the 10 % (ACN: 0.0625 DN) of tests/test_host_noise_run.py."""

import contextlib
import io

import darkstack_cases as dc
import noise_run_ref as ref
import numpy as np
import pytest
from conftest import assert_same_bits, gpu_context

from romanimpreprocess_amd import _native, calio
from romanimpreprocess_amd.calfiles import NoiseStack, make_dark_file, noise_run
from romanimpreprocess_amd.devarray import DevArray, to_device
from romanimpreprocess_amd.from_sim import sim_to_isim

pytestmark = pytest.mark.gpu

ACC = [k for k, _ in ref.ACC] + ["m33"]


def cubes_u16(seed, N, nreads, ny, width):
    """random samples over the whole range with the extremes planted: next to each other in a row and in consecutive frames"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(N):
        a = rng.integers(0, 65536, size=(nreads, ny, width)).astype(np.uint16)
        a[:, 3, 8:12] = (0, 32767, 32768, 65535)
        a[::2, 5, :4], a[1::2, 5, :4] = 0, 65535
        a[::2, 6, :4], a[1::2, 6, :4] = 65535, 0
        out.append(a)
    return out


def stored(a):
    """the FITS storage of unsigned samples: big-endian int16 with BZERO 32768"""
    return (a.astype(np.int32) - 32768).astype(">i2")


def dev16(a, offset=0):
    """a cube of 16-bit words in HBM under the dtype of its samples, its first sample ``offset`` samples off the allocation"""
    import torch

    flat = torch.zeros(a.size + 8, dtype=torch.int16, device="cuda")
    flat[offset:offset + a.size] = torch.from_numpy(np.ascontiguousarray(a).view(np.int16).reshape(-1)).cuda()
    arr = DevArray(flat[offset:offset + a.size].view(a.shape), np.uint16 if a.dtype == np.uint16 else np.int16)
    assert (arr.ctypes.data % 16 == 0) == (offset % 8 == 0)
    return arr


def words(stack):
    """every accumulator and table of a NoiseStack as numpy arrays"""
    out = {k: None if stack.acc[k] is None else stack.acc[k].numpy() for k in ACC}
    out.update({k: None if v is None else v.numpy() for k, v in stack.tables.items()})
    return out


def same_words(got, acc, tab, what):
    for k in ACC:
        if acc[k] is None:
            assert got[k] is None
        else:
            assert_same_bits(got[k], acc[k], f"{what} {k}")
    for k in ref.TABLES:
        if tab[k] is None:
            assert got[k] is None
        else:
            assert_same_bits(got[k], tab[k], f"{what} table {k}")


def run_both(cubes, C, cw, ref_out, f0, n, feed, tframe=3.04, params=True):
    """the cubes through a NoiseStack (``feed(cube)``: what add() gets, fits_be16) and through the restatement, everything compared"""
    ctx = gpu_context()
    nreads, ny, width = cubes[0].shape
    acc, rows, tab, pl, a33, want = ref.summarize(cubes, C, cw, ref_out, f0, n, tframe)
    st = NoiseStack(ny, width, C, cw, f0, n, ref_out, ctx=ctx)
    for j, c in enumerate(cubes):
        arg, be = feed(c)
        st.add(arg, fits_be16=be)
        assert_same_bits(st.rowsum.numpy(), rows[j], f"rowsum of exposure {j}")
    assert st.count == len(cubes)
    same_words(words(st), acc, tab, "stack")
    s = st.finish(tframe)
    assert_same_bits(s.planes.numpy(), pl, "planes")
    if ref_out:
        assert_same_bits(s.amp33.numpy(), a33, "amp33")
    else:
        assert s.amp33 is None and sorted(s.params) == ["ACN", "C_PINK", "U_PINK"]
    if params:
        assert s.params.keys() == want.keys()
        for k in want:
            print(k, s.params[k], want[k])
            assert s.params[k] == pytest.approx(want[k], rel=1e-9), k
    return st, s


# ------------------------------------------------------------------------------------------------ 1. host arrays, one pixel per lane
def test_host_arrays_one_pixel_form():
    """ny 128, 4 channels of 16 and the reference output (80 columns) of frames 83 wide: rows off the 16-byte grid"""
    cubes = cubes_u16(5, 3, 6, 128, 83)
    run_both(cubes, 4, 16, True, 1, 5, lambda c: (c, False))
    run_both(cubes, 4, 16, True, 1, 5, lambda c: (c[None], False))   # (1, N, ny, nx) cubes


# ------------------------------------------------------------------------------------------------ 2. the 8-pixel form
def test_eight_pixel_form_and_the_same_cube_off_the_grid():
    """ny 256, 2 channels of 128 and the reference output, FITS storage in HBM: 8 pixels per lane; the same cubes one sample off
    the 16-byte grid take the one-pixel form and give the same words; so do host arrays (staged: aligned)"""
    cubes = cubes_u16(6, 2, 4, 256, 384)
    a, sa = run_both(cubes, 2, 128, True, 1, 3, lambda c: (dev16(stored(c)), True))
    b, sb = run_both(cubes, 2, 128, True, 1, 3, lambda c: (dev16(stored(c), offset=1), True))
    c, sc = run_both(cubes, 2, 128, True, 1, 3, lambda c: (stored(c), True))
    wa, wb, wc = words(a), words(b), words(c)
    for k in wa:
        assert_same_bits(wa[k], wb[k], k)
        assert_same_bits(wa[k], wc[k], k)
    assert_same_bits(sa.planes.numpy(), sb.planes.numpy())
    assert sa.params == sb.params == sc.params


# ------------------------------------------------------------------------------------------------ 3. no reference output
def test_no_reference_output_and_a_wider_file():
    cubes = cubes_u16(7, 3, 5, 128, 64 + 3)
    _, s = run_both(cubes, 4, 16, False, 0, 5, lambda c: (to_device(c), False))
    hdus = s.hdus()
    assert len(hdus) == 2 and hdus[0] is None and [k for k, _ in hdus[1]["cards"][:6]] == list(ref.PLANES)
    # 8 pixels per lane where the file allows it: 72 columns wide, 8 channels of 8, the last 8 columns unused
    run_both(cubes_u16(8, 2, 3, 130, 72), 8, 8, False, 1, 2, lambda c: (to_device(c), False))


# ------------------------------------------------------------------------------------------------ 4. the accumulators at their bounds
def test_accumulators_at_their_bounds():
    """n = 64 frames, 512 exposures, ny 128, one channel of 2 columns.  Rows by y % 4: samples alternating 0 / 65535 from frame to
    frame (every d^2 at its largest: c1), the same starting at 65535 (a0, a1, b1), 32 frames of 0 then 32 of 65535 (the largest S:
    s0, s1) and the reverse.  Nothing wraps: the words are those of Python's integers."""
    n, N = 64, 512
    cube = np.zeros((n, 128, 2), np.uint16)
    cube[1::2, 0::4], cube[0::2, 1::4], cube[32:, 2::4], cube[:32, 3::4] = 65535, 65535, 65535, 65535
    ctx = gpu_context()
    st = NoiseStack(128, 2, 1, 2, 0, n, False, ctx=ctx)
    dev = to_device(cube)
    acc, tab = ref.new_acc(128, 1, 2, False), ref.new_tables(n, 128, 1, False)
    for _ in range(N):
        st.add(dev)
        ref.tables_add(tab, ref.add(acc, cube, 1, 2, False, 0, n), 1)
    got = words(st)
    same_words(got, acc, tab, "bounds")
    S = sum((2 * i - (n - 1)) * 65535 for i in range(32, n))
    assert S == 65535 * n * n // 4 and N * S * S < 1 << 64
    for y, want in ((0, {"a0": 0, "c1": N * 63 * 65535 ** 2, "b0": N * 65535, "c0": N * 65535}),
                    (1, {"a0": N * 65535, "a1": N * 65535 ** 2, "b1": N * 65535 ** 2, "b0": -N * 65535, "c0": -N * 65535}),
                    (2, {"s0": N * S, "s1": N * S * S, "c1": N * 65535 ** 2}), (3, {"s0": -N * S, "s1": N * S * S})):
        for k, v in want.items():
            assert int(got[k][y, 0]) == v and int(got[k][y + 4, 1]) == v, (y, k)
    with pytest.raises(ValueError, match="exposure 513"):
        st.add(dev)
    same_words(words(st), acc, tab, "after the refused exposure")
    pl, _ = ref.planes(acc, N, n, 1, 2, False)
    assert_same_bits(st.finish().planes.numpy(), pl, "planes at the bounds")


# ------------------------------------------------------------------------------------------------ 5. the round trip
def test_round_trip_on_the_device():
    cubes, _ = ref.round_trip_case()
    c = ref.CASE
    _, s = run_both(cubes, c["C"], c["cw"], True, 0, c["nreads"], lambda a: (to_device(a), False))
    for k, want in ref.PLANTED.items():
        assert abs(s.params[k] / want - 1) < 0.10, (k, s.params[k])
    assert abs(s.params["ACN"] - ref.ACN) < ref.ACN_TOL


# ------------------------------------------------------------------------------------------------ 6. end to end
class _Clock:
    """make_dark_file stamps its trees with the time of day: one instant for both runs"""

    @staticmethod
    def now(tz=None):
        from datetime import datetime, timezone

        return datetime(2026, 7, 1, 12, 0, 0, tzinfo=timezone.utc)


@pytest.mark.parametrize("ref_out", [True, False])
def test_summary_file_dark_and_read_files_and_the_generator(tmp_path, monkeypatch, ref_out):
    """noise_run writes the summary, make_dark_file.run writes dark and read from it, L1Synth is built from that read file;
    run(noise_out=None) makes the summary in its own pass and gives byte-identical dark and read files"""
    ctx = gpu_context()
    N, nreads, ny, C, cw = 4, 8, 128, 4, 16
    nside = C * cw
    cubes = ref.make_darks(9, N, nreads, ny, C, cw, ref_out=True, acn=0.3)
    if not ref_out:
        cubes = [np.ascontiguousarray(c[:, :, :nside + 3]) for c in cubes]   # 3 columns that are no channel
    for j, c in enumerate(cubes):
        dc.write_dark_fits(tmp_path / f"99_SCA07_Noise_{j + 1:03d}.fits", c)
    first, out = str(tmp_path / "99_SCA07_Noise_001.fits"), str(tmp_path / "noise_SCA07.fits")
    opts = ["-f", "1", "-o", out, "-n", str(N), "-t", "3", "-cd", "5.0", "-rh", "7", "-tn", "6"] + (["-ro"] if ref_out else [])
    s = noise_run.run(["-i", first] + opts, nside=nside, cw=cw, ctx=ctx)
    _, _, _, pl, a33, want = ref.summarize(cubes, C, cw, ref_out, 2, 6)
    head, data = calio.read_fits_image(out, 1)
    assert_same_bits(np.asarray(data, np.float32), pl, "the file's planes")
    assert [head[k] for k in ref.PLANES] == list(range(6)) and head["NDARK"] == N and head["TSTART"] == 3 and head["NFRAME"] == 6
    assert head["TFRAME"] == 3.04 and head["CDSCUT"] == 5.0 and head["ROWOVER"] == 7
    for k in ("ACN", "C_PINK", "U_PINK"):
        assert head[k] == s.params[k] == pytest.approx(want[k], rel=1e-9)
    if ref_out:
        h33, d33 = calio.read_fits_image(out, "AMP33")
        assert_same_bits(np.asarray(d33, np.float32), a33, "AMP33")
        assert h33["M_PINK"] == s.params["M_PINK"] and h33["RU_PINK"] == pytest.approx(want["RU_PINK"], rel=1e-9)
    else:
        with pytest.raises(KeyError):
            calio.read_fits_image(out, "AMP33")
    monkeypatch.setattr(make_dark_file, "datetime", _Clock)
    reads = [0, 1, 1, 3, 4, 8]
    kw = dict(reads=reads, nside=nside, ctx=ctx)
    with contextlib.redirect_stdout(io.StringIO()):
        files = make_dark_file.run("p", first, out, 7, str(tmp_path / "a_dark_X.asdf"), **kw)
        same = make_dark_file.run("p", first, None, 7, str(tmp_path / "b_dark_X.asdf"), noise_args=[str(tmp_path / "b.fits") if o == out else o
                                                                                                      for o in opts], channelwidth=cw, **kw)
    for a, b in zip(files, same):
        assert open(a, "rb").read() == open(b, "rb").read(), (a, b)
    assert open(out, "rb").read() == open(tmp_path / "b.fits", "rb").read()
    dark, read = calio.roman_branch(files[0]), calio.roman_branch(files[1])
    assert_same_bits(np.asarray(read["data"]), (pl[4].astype(np.float64) / np.sqrt(2.0)).astype(np.float32)[:, :nside], "read noise")
    assert_same_bits(np.asarray(read["resetnoise"]), pl[5][:, :nside], "reset noise")
    assert float(read["anc"]["U_PINK"]) == s.params["U_PINK"] and float(read["anc"]["C_PINK"]) == s.params["C_PINK"]
    assert bool(read["amp33"]["valid"]) == ref_out
    if ref_out:
        assert_same_bits(np.asarray(read["amp33"]["med"]), a33[0], "amp33 med")
        assert_same_bits(np.asarray(read["amp33"]["std"]), a33[1], "amp33 std")
        assert float(read["amp33"]["M_PINK"]) == s.params["M_PINK"]
    else:   # make_dark_file's placeholder
        assert np.asarray(read["amp33"]["med"]).shape == (4096, 128) and not np.asarray(read["amp33"]["std"]).any()
    # the generator takes its parameters from that read file
    cal = {"gain": {"data": np.full((ny, nside), 1.5, np.float32)}, "read": read,
           "dark": {"data": np.asarray(dark["data"]), "dark_slope": np.asarray(dark["dark_slope"])}}
    synth = sim_to_isim.L1Synth(cal, [[0], [1, 2], [4, 5, 6, 7]], 3.04, ctx=ctx, channelwidth=cw)
    assert synth.desc.u_pink == s.params["U_PINK"] and synth.desc.c_pink == s.params["C_PINK"]
    assert synth.desc.amp33_valid == int(ref_out) and (not ref_out or synth.desc.ru_pink == s.params["RU_PINK"])


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_every_refusal_by_name_before_any_launch():
    ctx = gpu_context()
    cube = cubes_u16(1, 1, 6, 128, 83)[0]
    st = NoiseStack(128, 83, 4, 16, 1, 5, True, ctx=ctx)
    a, t = st.acc, st.tables
    ok = dict(cube=cube, location=_native.RIP_HOST, nreads=6, ny=128, nx_file=83, C=4, cw=16, ref_out=1, f0=1, n=5, fits_be16=0, count=0,
              a0=a["a0"], a1=a["a1"], b0=a["b0"], b1=a["b1"], s0=a["s0"], s1=a["s1"], c0=a["c0"], c1=a["c1"], m33=a["m33"],
              rowsum=st.rowsum)
    for kw, text in (({"n": 1}, "-tn 1"), ({"n": 65}, "-tn 65"), ({"count": 512}, "exposure 513"), ({"count": -1}, "exposure 0"),
                     ({"n": 6}, "-tn 6"), ({"f0": 2}, "-tn 5"), ({"f0": -1}, "-t 0"), ({"cw": 15}, "channel width 15"),
                     ({"cw": 258}, "channel width 258"), ({"ny": 127}, "127 rows"), ({"nx_file": 79}, "frame of 79"), ({"C": 5}, "5 channels"),
                     ({"C": 0}, "0 channels"), ({"location": 7}, "location 7"), ({"cube": None}, "NULL"), ({"s1": None}, "NULL"),
                     ({"m33": None}, "NULL"), ({"rowsum": None}, "NULL")):
        with pytest.raises(ValueError, match=text):
            ctx.call("rip_cal_noise_add", *dict(ok, **kw).values())
    rs = ok["rowsum"]
    tabs = [t[k] for k in ref.TABLES]
    for args, text in (((rs, 1, 128, 4, 1), "-tn 1"), ((rs, 5, 127, 4, 1), "127 rows"), ((rs, 5, 128, 0, 1), "0 channels"),
                       ((None, 5, 128, 4, 1), "NULL")):
        with pytest.raises(ValueError, match=text):
            ctx.call("rip_cal_noise_rowstats", *args, *tabs)
    with pytest.raises(ValueError, match="NULL"):
        ctx.call("rip_cal_noise_rowstats", rs, 5, 128, 4, 1, *tabs[:4], None, *tabs[5:])
    got = words(st)
    assert not st.rowsum.numpy().any() and all(not v.any() for v in got.values())   # nothing was launched
    out = to_device(np.zeros((6, 128, 64), np.float32))
    a33 = to_device(np.zeros((2, 128, 16), np.float32))
    pk = dict(a0=a["a0"], a1=a["a1"], b0=a["b0"], b1=a["b1"], s0=a["s0"], s1=a["s1"], c0=a["c0"], c1=a["c1"], m33=a["m33"], nexp=2, n=5,
              ny=128, C=4, cw=16, ref_out=1, tframe=3.04, location=_native.RIP_DEVICE, planes=out, amp33=a33)
    for kw, text in (({"nexp": 1}, "-n 1"), ({"nexp": 513}, "-n 513"), ({"n": 1}, "-tn 1"), ({"tframe": 0.0}, "tframe 0"),
                     ({"location": 5}, "location 5"), ({"planes": None}, "NULL"), ({"amp33": None}, "NULL"), ({"c1": None}, "NULL")):
        with pytest.raises(ValueError, match=text):
            ctx.call("rip_cal_noise_planes", *dict(pk, **kw).values())
    assert not out.numpy().any()
    with pytest.raises(ValueError, match="-n 0"):   # a summary needs two exposures
        st.finish()
    # the Python layer
    for kw, text in (({"n": 65}, "-tn 65"), ({"cw": 15}, "channel width 15"), ({"ny": 100}, "100 rows"), ({"nx_file": 70}, "frame of 70")):
        with pytest.raises(ValueError, match=text):
            NoiseStack(**dict(dict(ny=128, nx_file=83, C=4, cw=16, f0=1, n=5, ref_out=True, ctx=ctx), **kw))
    with pytest.raises(ValueError, match="cube is needed"):
        st.add(cube[:, :100])
    with pytest.raises(TypeError, match="16-bit"):
        st.add(cube.astype(np.float32))
    with pytest.raises(TypeError, match="fits_be16"):
        st.add(stored(cube))
    with pytest.raises(ValueError, match="-tn 5"):   # a cube with too few frames, by the library
        st.add(cube[:5])
    assert st.count == 0
