"""Every launch-geometry branch of the fused kernel (chain2_form.h: chain2_geometry; the prologue of chain2_kernel.h) on every form,
against the CPU oracle, the stage kernels and the uniform grid, bit for bit.

The launcher cuts a frame into column strips and row ranges in one of two ways: the UNIFORM grid (every strip the same row ranges)
or QUAD mode (a last strip of at most 64 live columns is covered by workgroups whose cols / 64 wave columns are 64-column windows
on a row range each: another index path of the kernel).  Which one runs depends on the form, the frame and the CU count, so every
case here
  (a) asks ``rip_chain_geometry_for`` for a shape with the property it is after -- the listed shape where the device has the 256 CUs
      the shapes were designed for, else the first height up to 1600 rows that has it; the case FAILS when there is none -- and
      asserts through ``rip_last_chain_geometry`` that the launch really took that geometry;
  (b) compares the fused kernel with the oracle, bit for bit;
  (c) compares it with the stage kernels and with the fused kernel on the uniform grid (option "chain_quad" = 0), bit for bit.
At 512 / 768 columns the quad strip emits two science columns and the four reference columns, which random sources never
saturate: a band of bright rates over the last science columns (200 .. 60000 DN/s down the rows) and a cosmic-ray fraction of 5 %
put jumps and first saturations at every group there, and every case checks the ORACLE's output for them before any GPU call."""

import numpy as np
import pytest
import torch  # before libromanhip is loaded: torch brings its own copy of the HIP runtime, and the first one loaded must be the one both use
from chain_support import (F32, F64, assert_equal_outputs, assert_oracle, band_conditions, calibrate_resident, chain_context, device_cus,
                           device_outputs, find_height, geometry, inputs, is_quad, loaded, make_band_ramp, outputs_to_numpy,
                           quad_columns, ramp_to_dev)

from romanimpreprocess_amd import _native, pipeline, synth

pytestmark = pytest.mark.gpu

SLOT = 7


def last_rows(ny, rows):
    """rows of the last non-empty range"""
    return ny - (-(-ny // rows) - 1) * rows


# ---- one case: (a) the branch, (b) the oracle, (c) stage kernels and the uniform grid
KEYS = ("cube", "groupdq", "pixeldq", "slope", "err_read", "err_poisson")


def run_case(G, kdt, ny, nx, p, exclude_first, want, want_uniform=None, reserves=None):
    """`want(g)` / `want_uniform(g)`: the property the geometry of the default / the chain_quad = 0 launch must have;
    `reserves`: the values of "chain_reserve" the fused kernel runs with (None: the library's default alone)"""
    ncu = device_cus()
    rp, cal, ramp, ref, lines = inputs(G, kdt == F64, ny, nx, p, exclude_first)
    g0 = geometry(G, kdt, ny, nx, ncu)
    band_conditions(ref, G, quad_columns(g0, nx) if g0["nq"] else slice(nx - 28, nx - 4))
    ctx = chain_context()
    reserves = reserves or (ctx.get_option("chain_reserve"),)
    kw = dict(exclude_first=exclude_first, want_cube=True, channel_lines=lines)
    with loaded(pipeline.Calibrator(ctx=ctx), SLOT, cal) as cb:
        seen = []
        for reserve in reserves:
            with ctx.options(chain_reserve=reserve):
                fused = cb.calibrate(SLOT, ramp, **kw)
            assert ctx.last_chain_form() == 2, "the fused kernel did not run"
            g = ctx.last_chain_geometry()
            assert g == geometry(G, kdt, ny, nx, ncu, reserve), "the launch and the query disagree"
            assert g == cb.chain_geometry_for(SLOT, G, ncu, reserve)
            assert want(g), f"not the intended branch: {g}"
            seen.append(g)
            assert_oracle(fused, ref, f"reserve {reserve}", cube=True)
        with ctx.options(chain_quad=0):
            uniform = cb.calibrate(SLOT, ramp, **kw)
        assert ctx.last_chain_form() == 2
        u = ctx.last_chain_geometry()
        assert u == geometry(G, kdt, ny, nx, ncu, quad_ok=False) and u["nq"] == 0 and u["rows_q"] == 0, u
        assert want_uniform is None or want_uniform(u), f"not the intended uniform grid: {u}"
        with ctx.options(chain2=0):
            stages = cb.calibrate(SLOT, ramp, **kw)
        assert ctx.last_chain_form() == 0
        assert ctx.last_chain_geometry() == dict.fromkeys(_native.GEOMETRY_FIELDS, 0)
    assert_equal_outputs(fused, stages, "fused vs stage kernels", keys=KEYS)
    assert_equal_outputs(fused, uniform, "fused vs fused on the uniform grid", keys=KEYS)
    return seen


# ---- 1. quad mode on every form
# form, groups, shape at 256 CUs, live columns of the last strip; Legendre orders and starts rotate down the rows.  The two 16-group
# cases are 1040 rows tall, not the 720 / 704 of their neighbours: the band repeats every 97 rows and the last two groups of the read
# pattern lie 1.5 reads apart, so at 720 x 768 and 704 x 512 the oracle shows 9 pixels that first saturate at group 15 on the two
# science columns of the quad strip -- one short of what band_conditions asks; at 1040 rows it shows 17 and 18 (ranges of 9 and 10
# rows there, where the others have 8).
QUAD = [
    (6, F64, 720, 768, 8), (7, F64, 720, 768, 8),            # f64 ipc4d, 5-8 groups: 384 columns, six (K rings of 6 and 7 differ)
    (8, F64, 528, 1152, 12),
    (9, F32, 720, 768, 8), (16, F32, 1040, 768, 8),          # f32 ipc4d, 9-16 groups: 384 columns, six, no rings
    (12, F32, 528, 1152, 12),
    (11, F64, 704, 512, 8), (16, F64, 1040, 512, 8),         # f64 ipc4d, 9-16 groups: 256 columns, four, no rings
    (10, F64, 544, 768, 12),
    (13, F64, 352, 1280, 20),
    (5, F32, 1376, 512, 8), (8, F32, 1376, 512, 8),          # f32 ipc4d, 5-8 groups: 256 columns, four wave columns
]
_ORDERS = (3, 8, 10)


def _quad_cases():
    return [pytest.param(G, kdt, ny, nx, live, _ORDERS[i % 3], bool(i % 2),
                         id=f"g{G}_{'k64' if kdt == F64 else 'f32'}_{ny}x{nx}_np{_ORDERS[i % 3] + 1}_start{i % 2}")
            for i, (G, kdt, ny, nx, live) in enumerate(QUAD)]


@pytest.mark.parametrize("G,kdt,ny0,nx,live,p,exclude_first", _quad_cases())
def test_quad_mode_on_every_form(G, kdt, ny0, nx, live, p, exclude_first):
    ncu = device_cus()
    ny = find_height(ny0, 8, lambda ny: is_quad(geometry(G, kdt, ny, nx, ncu), live), f"quad mode at nx = {nx}")
    (g,) = run_case(G, kdt, ny, nx, p, exclude_first, lambda g: is_quad(g, live))
    assert g["cols"] // 64 == (4 if g["cols"] == 256 else 6)


# ---- 2. the reserve
def test_reserve_changes_the_geometry_not_the_bits():
    """f32 ipc4d x 8 groups (the only form that takes a reserve) in quad mode with no reserve, the default, a reserve that leaves a
    dozen slots (long ranges: 5 x 276 rows, quad 8 x 172 at 256 CUs) and one larger than the slot count, which the quad search
    meets in its SECOND pass (without the reserve).  What that pass finds is the geometry of reserve 0 -- neither it nor the
    uniform grid it competes with sees a reserve that leaves no slot -- so the second pass shows as quad mode at a reserve that
    leaves the first pass fewer than two slots."""
    G, kdt, nx = 8, F32, 512
    ncu = device_cus()
    slots = 2 * ncu
    default_reserve = _native.option_table()["chain_reserve"][0]
    reserves = (0, default_reserve, slots - 12, slots + 5)
    ny = find_height(1376, 8, lambda ny: all(is_quad(geometry(G, kdt, ny, nx, ncu, r), 8) for r in reserves), "quad mode at every reserve")
    p, exclude_first = _quad_cases()[-1].values[5:]   # (the inputs of the case above)
    seen = run_case(G, kdt, ny, nx, p, exclude_first, lambda g: is_quad(g, 8), reserves=reserves)
    assert seen[3] == seen[0], "the second pass searches without the reserve"
    assert seen[2] != seen[0] and seen[2]["grid"] <= 12 and seen[2]["rows"] > seen[0]["rows"] and seen[2]["rows_q"] > seen[0]["rows_q"]
    assert seen[1]["grid"] <= slots - default_reserve


# ---- 3. ragged rows: heights that are no multiple of the range length
RAGGED_FORMS = [(8, F64, 768), (10, F32, 768), (11, F64, 512)]


def quad_tail(g, ny):
    """(rows of the last quad range, wave columns of the last WORKING quad workgroup that work, empty trailing full-strip ranges)"""
    wc = g["cols"] // 64
    nranges = -(-ny // g["rows_q"])
    return last_rows(ny, g["rows_q"]), nranges - (-(-nranges // wc) - 1) * wc, g["nr"] - -(-ny // g["rows"])


def _ragged_property(kind, wc):
    """kind -> (property of the default launch's geometry, of the chain_quad = 0 launch's, or None) as functions of (g, ny)"""
    mixed = lambda g, ny: 0 < quad_tail(g, ny)[1] < wc          # noqa: E731  (working and empty wave columns share barriers)
    if kind == "last2_mixed_empty":   # 1001 rows on the 384-column forms: a last range of 2 rows, wholly empty ranges, a mixed workgroup
        return (lambda g, ny: is_quad(g) and quad_tail(g, ny)[0] == 2 and mixed(g, ny) and quad_tail(g, ny)[2] > 0), None
    if kind == "full_mixed":          # 999 rows: a full last range, a mixed workgroup
        return (lambda g, ny: is_quad(g) and quad_tail(g, ny)[0] == g["rows_q"] and mixed(g, ny)), None
    if kind == "last1_uniform3":      # a last range of 1 row in quad mode, of 3 rows on the uniform grid of the same frame
        return (lambda g, ny: is_quad(g) and quad_tail(g, ny)[0] == 1), (lambda u, ny: last_rows(ny, u["rows"]) == 3)
    if kind == "last3_uniform1":
        return (lambda g, ny: is_quad(g) and quad_tail(g, ny)[0] == 3), (lambda u, ny: last_rows(ny, u["rows"]) == 1)
    raise ValueError(kind)


RAGGED = [("last2_mixed_empty", 1001), ("full_mixed", 999), ("last1_uniform3", 793), ("last3_uniform1", 811)]


@pytest.mark.parametrize("kind,ny0", RAGGED, ids=[k for k, _ in RAGGED])
@pytest.mark.parametrize("G,kdt,nx", RAGGED_FORMS, ids=[f"g{g}_{'k64' if k == F64 else 'f32'}_nx{nx}" for g, k, nx in RAGGED_FORMS])
def test_ragged_row_ranges(G, kdt, nx, kind, ny0):
    ncu = device_cus()
    wc = geometry(G, kdt, 1001, nx, ncu)["cols"] // 64
    want, want_u = _ragged_property(kind, wc)

    def has(ny):
        g, u = geometry(G, kdt, ny, nx, ncu), geometry(G, kdt, ny, nx, ncu, quad_ok=False)
        return g is not None and want(g, ny) and (want_u is None or want_u(u, ny))

    ny = find_height(ny0, 1, has, f"{kind} at nx = {nx}", lo=600)   # (several periods of the band)
    run_case(G, kdt, ny, nx, 8, True, lambda g: want(g, ny), None if want_u is None else (lambda u: want_u(u, ny)))


def test_uniform_grid_with_a_last_range_of_one_row():
    """a last strip of 136 live columns: no quad mode at any height; wholly empty ranges too where the search finds them"""
    G, kdt, nx = 8, F64, 896
    ncu = device_cus()
    uniform1 = lambda g, ny: g is not None and g["nq"] == 0 and g["live_last"] > 64 and last_rows(ny, g["rows"]) == 1   # noqa: E731
    ny = find_height(601, 1, lambda ny: uniform1(geometry(G, kdt, ny, nx, ncu), ny), "a uniform grid with a last range of 1 row", lo=600)
    run_case(G, kdt, ny, nx, 8, True, lambda g: uniform1(g, ny))


# ---- 4. the batch and the device-resident entry points in quad mode
def _entry_inputs():
    G, kdt, nx = 8, F64, 768
    ncu = device_cus()
    ny = find_height(720, 8, lambda ny: is_quad(geometry(G, kdt, ny, nx, ncu), 8), "quad mode at nx = 768")
    rp, cal, ramp, ref, _lines = inputs(G, True, ny, nx, 8, True)
    band_conditions(ref, G, quad_columns(geometry(G, kdt, ny, nx, ncu), nx))
    return G, ny, nx, rp, cal, ramp


def test_batch_equals_single_calls_in_quad_mode():
    G, ny, nx, rp, cal, ramp = _entry_inputs()
    ramps = [ramp, make_band_ramp(cal, rp, ny, nx, 57)]
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), SLOT, cal) as cb:
        singles = []
        for r in ramps:
            singles.append(cb.calibrate(SLOT, r))
            assert ctx.last_chain_form() == 2 and is_quad(ctx.last_chain_geometry(), 8)
        many = cb.calibrate_many(SLOT, ramps, want_groupdq=True)
        assert ctx.last_chain_form() == 2 and is_quad(ctx.last_chain_geometry(), 8)
    assert len(many) == 2
    for i, (a, b) in enumerate(zip(many, singles)):
        assert_equal_outputs(a, b, f"ramp {i}")
    assert not np.array_equal(singles[0]["slope"], singles[1]["slope"])


def test_device_resident_calls_equal_host_call_in_quad_mode():
    G, ny, nx, rp, cal, ramp = _entry_inputs()
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), SLOT, cal) as cb:
        host = cb.calibrate(SLOT, ramp)
        assert ctx.last_chain_form() == 2 and is_quad(ctx.last_chain_geometry(), 8)
        pid, _meta = cb.plan_for(rp, synth.FRAME_TIME)
        t, o = ramp_to_dev(ramp), device_outputs(G, ny, nx)
        torch.cuda.synchronize()
        for _ in range(2):   # back to back: the second call's pre-pass is queued while the first call's kernel runs
            calibrate_resident(cb, SLOT, pid, G, t, o)
        cb.synchronize()
        assert ctx.last_chain_form() == 2 and is_quad(ctx.last_chain_geometry(), 8)
        got = outputs_to_numpy(o)
    assert_equal_outputs(got, host, "device-resident against host call")
