"""The short exact forms of csrc/short_forms.h -- the one-correction quotient (div_rcp, div_rcp2) and the short hypot -- on the host:
tests/host/short_forms_check.cpp includes the header the device code calls, is built here with the host compiler (one rounding per
operation: -ffp-contract=off, fmaf / fma from the C library or the CPU) and compares

  * rip_div_rcp1(a, b, RN(1/b)) with a / b for every one of the 2^23 numerator mantissas at three exponents (the two ends of the
    numerators' range and 1) and about a thousand divisors: 1, the smallest and largest mantissas, all ones and one-off -- the
    cases the argument in the header leaves to enumeration --, the edges of rcp_safe, rip_mid_range, rip_mid36 and of the gain's
    clip, and 1000 seeded ones;
  * rip_hypot_short with (float)sqrt((double)a*a + (double)b*b) on 400 thousand seeded pairs and 1.4 million pairs whose root lies
    within a few f64 steps of an f32 rounding midpoint, on both sides of it, under reciprocal-root estimates with a relative error
    of up to 2^-20 (the hardware's is 2^-23): where the form accepts, the same bits; it turns a pair away only outside its range
    or inside its guard band; the refined f64 root within the 8 steps the header's bound allows (seen: 1)."""

import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "short_forms_check.cpp")


def host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        path = shutil.which(name) if name else None
        if path:
            return path
    raise AssertionError("no host C++ compiler (CXX, c++, g++, clang++)")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("short_forms") / "short_forms_check")
    flags = ["-O3", "-std=c++17", "-ffp-contract=off", "-pthread", "-Wall"]
    cxx = host_compiler()
    # the CPU's own fma and vector units where the compiler knows them (the quotient loop is 2.6e10 divisions); plain code otherwise
    native = subprocess.run([cxx, "-march=native", *flags, SRC, "-o", exe], capture_output=True, text=True)
    if native.returncode != 0:
        subprocess.run([cxx, *flags, SRC, "-o", exe], check=True)
    return exe


def test_short_forms_on_the_host(program):
    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    run = subprocess.run([program, str(threads)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("OK"), run.stdout[-4000:] + run.stderr[-2000:]
    assert " 0 mismatches" in run.stdout and " 0 failures" in run.stdout
