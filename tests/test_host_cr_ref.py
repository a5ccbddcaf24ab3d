"""CPU-only tests of the cosmic-ray model's numpy reference (``cr_ref.py``) against closed forms, and of the host side of the two
library entries (``rip_synth_cr_tracks``, ``rip_synth_cr_deposit``): struct layout, exported symbols, parameter mapping."""

import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
from conftest import REPO

import cr_ref
from romanimpreprocess_amd import _native

N_I, N_J = 24, 40


def _as_dict(parts):
    out = {}
    for i, j, l2 in parts:
        assert (i, j) not in out, "a pixel listed twice"
        out[(i, j)] = l2
    return out


@pytest.mark.parametrize("case", cr_ref.closed_form_cases(N_I, N_J), ids=lambda c: c[0].replace(" ", "_"))
def test_traversal_matches_the_closed_forms(case):
    """inside one pixel, zero length, along a row and a column, 45 degrees through pixel corners, out of each of the four sides"""
    _, (i0, j0, phi, length), want = case
    i1, j1 = cr_ref.endpoints(i0, j0, phi, length, N_I, N_J)
    assert -0.5 <= i1 <= N_I + 0.5 and -0.5 <= j1 <= N_J + 0.5
    got = _as_dict(p for p in cr_ref.traverse(i0, j0, float(i1), float(j1)) if 0 <= p[0] < N_I and 0 <= p[1] < N_J)
    assert set(got) == {(i, j) for i, j, _ in want}
    for i, j, l2 in want:
        assert abs(got[(i, j)] - l2) < 1e-12, (i, j, got[(i, j)], l2)


def test_exact_corners_give_no_slivers():
    """end points handed in exactly: the i and j crossings coincide bit for bit and only the diagonal pixels are crossed"""
    got = cr_ref.traverse(2.0, 3.0, 6.0, 7.0)
    r2 = math.sqrt(2.0)
    assert [(i, j) for i, j, _ in got] == [(2, 3), (3, 4), (4, 5), (5, 6), (6, 7)]
    assert np.allclose([l2 for _, _, l2 in got], [r2 / 2, r2, r2, r2, r2 / 2], rtol=0, atol=1e-14)
    # the same diagonal walked backwards
    back = cr_ref.traverse(6.0, 7.0, 2.0, 3.0)
    assert [(i, j) for i, j, _ in back] == [(6, 7), (5, 6), (4, 5), (3, 4), (2, 3)]


def test_parts_sum_to_the_length_inside_the_image():
    rng = np.random.default_rng(3)
    n = 300
    i0, j0 = rng.uniform(0, N_I, n), rng.uniform(0, N_J, n)
    phi, length = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 600.0, n)
    i1, j1 = cr_ref.endpoints(i0, j0, phi, length, N_I, N_J)
    for k in range(n):
        parts = cr_ref.traverse(i0[k], j0[k], i1[k], j1[k])
        assert abs(sum(p[2] for p in parts) - math.hypot(i1[k] - i0[k], j1[k] - j0[k])) < 1e-11
        inside = sum(p[2] for p in parts if 0 <= p[0] < N_I and 0 <= p[1] < N_J)
        assert abs(inside - cr_ref.in_image_length(i0[k], j0[k], i1[k], j1[k], N_I, N_J)) < 1e-10 * len(parts) + 1e-11, k
        assert len({(p[0], p[1]) for p in parts}) == len(parts)   # a straight line enters a pixel once


def test_sampler_medians_match_the_tables_and_the_closed_forms():
    par = cr_ref.PARAMS
    c_len, x_len, c_de, x_de = tabs = cr_ref.tables()
    for c in (c_len, c_de):
        assert c[0] == 0.0 and c[-1] == 1.0 and np.all(np.diff(c) >= 0)
    _, _, _, length, dedx = cr_ref.sample([[0.1, 0.2, 0.3, 0.5, 0.5]], N_I, N_J, tabs=tabs)
    # the interpolated median sits in the table segment that brackets 0.5 ...
    for med, c, x in ((length[0], c_len, x_len), (dedx[0], c_de, x_de)):
        k = np.searchsorted(x, med, side="right") - 1
        assert c[k] <= 0.5 <= c[k + 1] and x[k] <= med <= x[k + 1]
    # ... and within a grid step of the continuous distribution's (the table is a left Riemann sum)
    a = par["slope"] + 1.0
    lo, hi = par["min_cr_len"], par["max_cr_len"]
    med_len = (lo ** a + 0.5 * (hi ** a - lo ** a)) ** (1.0 / a)
    assert abs(length[0] - med_len) < x_len[1] - x_len[0]
    assert abs(float(cr_ref.moyal_cdf(dedx[0])) - 0.5) < 0.01 and abs(float(cr_ref.length_cdf(length[0])) - 0.5) < 0.05
    # ends of the range
    i0, j0, phi, length, dedx = cr_ref.sample([[0.0, 0.5, 0.25, 0.0, 1.0]], N_I, N_J, tabs=tabs)
    assert i0[0] == 0.0 and j0[0] == 0.5 * N_J and phi[0] == 0.5 * np.pi and length[0] == lo and dedx[0] == par["max_dEdx"]


def test_deposit_case_keeps_its_roundings_decided():
    """the tracks of the GPU deposit test: at most 1 % of their deposits may have a mean within 1e-6 of a half-integer (there the
    test only asks for agreement within 1), and they do cover what they are meant to cover"""
    nreads = 6
    tracks = cr_ref.deposit_case_tracks(N_I, N_J, nreads)
    assert 56 <= len(tracks) <= 64
    ref = cr_ref.deposit(tracks, nreads, N_I, N_J)
    unsure_hits = int(ref["unsure"][-1].sum())
    assert unsure_hits <= 0.01 * ref["hits"], (unsure_hits, ref["hits"])
    first = ref["first_read"]
    assert (first == 0).any() and (first == nreads - 1).any() and (first == nreads).any()
    assert np.all(first[21] < nreads)                         # the track over every column of row 21
    assert first[5, 25] == 3 and first[15, 5] == 1            # two tracks in one read; in two reads
    assert ref["added"][0, 15, 5] == 0 and ref["added"][1, 15, 5] > 0 and ref["added"][4, 15, 5] > ref["added"][3, 15, 5]
    assert np.all(np.diff(ref["added"], axis=0) >= 0)
    # a closed form among them: 10 dEdx electrons per unit of l3 = sqrt(0.25 + l2^2)
    name, (i0, j0, _, _), parts = cr_ref.closed_form_cases(N_I, N_J)[2]
    assert name == "along a column"
    dedx = tracks[2, 5]
    for i, j, l2 in parts:
        assert abs(ref["lam"][i, j] - dedx * 20.0 * math.sqrt(0.25 + l2 * l2)) < 1e-9


def test_cr_params_layout_matches_the_header(tmp_path):
    """sizeof/offsetof of rip_cr_params as gcc sees it == the ctypes mirror"""
    fields = [f for f, _ in _native.CrParams._fields_]
    body = 'printf("size %zu\\n", sizeof(rip_cr_params));\n' + "".join(
        f'printf("{f} %zu\\n", offsetof(rip_cr_params, {f}));\n' for f in fields)
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "romanhip.h"\nint main(void){\n' + body + "return 0;}\n")
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(_native.CrParams) == 13 * 8
    for f in fields:
        assert int(got[f]) == getattr(_native.CrParams, f).offset, f


def test_library_exports_the_two_entries():
    lib = _native.load_library()
    for name in ("rip_synth_cr_tracks", "rip_synth_cr_deposit"):
        assert name in _native.SYMBOLS and hasattr(lib, name)
    assert lib.rip_version() == 100   # additions: the version stays


def test_parameter_keywords_map_onto_the_struct():
    from romanimpreprocess_amd.from_sim import cr

    p = cr.params_from({})
    assert {k: getattr(p, f) for k, (f, _) in cr.DEFAULTS.items()} == cr_ref.PARAMS
    p = cr.params_from({"area": 0, "max_cr_len": 500, "grid_size": 64})
    assert (p.area, p.max_len, p.grid_size, p.flux) == (0.0, 500.0, 64, 8.0)
    with pytest.raises(TypeError, match="unknown"):
        cr.params_from({"fluxx": 1})
    assert cr.capacity_for(cr.params_from(None), 35, 3.04) == int(35 * 408.576 + 10 * math.sqrt(35 * 408.576) + 64)
