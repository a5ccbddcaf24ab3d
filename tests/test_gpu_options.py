"""rip_set_option / rip_get_option / rip_reset_options and Context.options() on a context: values only, no kernel is launched."""

import pytest
import torch  # noqa: F401  before libromanhip is loaded: torch brings its own copy of the HIP runtime, and the first one loaded must be the one both use
from conftest import gpu_context

from romanimpreprocess_amd import _native

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = -2**31, 2**31 - 1


def int_options():
    """name -> (default, lowest, highest) of the integer options; "guard_band" is the f64 one"""
    return {name: row for name, row in _native.option_table().items() if name != "guard_band"}


def defaults():
    return {**{name: row[0] for name, row in int_options().items()}, "guard_band": 1e-5}


@pytest.fixture
def ctx():
    c = gpu_context()
    c.reset_options()
    yield c
    c.reset_options()


def values(c):
    return {**{name: c.get_option(name) for name in int_options()}, "guard_band": c.get_option_f64("guard_band")}


def test_reset_gives_the_table_defaults(ctx):
    assert values(ctx) == defaults()


def test_set_get_round_trip_at_both_ends(ctx):
    for name, (_default, lo, hi) in int_options().items():
        for v in (lo, hi) + ((-1, 0, 1) if name == "overlap" else ()):
            ctx.set_option(name, v)
            assert ctx.get_option(name) == v, f"{name} = {v}"
    for v in (0.0, 1e-5, float("inf")):
        ctx.set_option_f64("guard_band", v)
        assert ctx.get_option_f64("guard_band") == v


def test_one_step_outside_a_bounded_range_is_refused(ctx):
    bounded = 0
    for name, (_default, lo, hi) in int_options().items():
        # an end at INT_MIN / INT_MAX is no bound; chain_reserve clamps below its lowest value instead of refusing
        outside = [lo - 1] * (lo > INT_MIN and name != "chain_reserve") + [hi + 1] * (hi < INT_MAX)
        for v in outside:
            before = ctx.get_option(name)
            with pytest.raises(ValueError, match=name):
                ctx.set_option(name, v)
            assert ctx.get_option(name) == before
            bounded += 1
    assert bounded == 6   # prepass_form, prepass_gate and overlap, both ends
    for v in (-1e-9, float("nan")):
        with pytest.raises(ValueError, match="guard_band"):
            ctx.set_option_f64("guard_band", v)
        assert ctx.get_option_f64("guard_band") == 1e-5


def test_chain_reserve_clamps_negatives_to_zero(ctx):
    ctx.set_option("chain_reserve", -3)
    assert ctx.get_option("chain_reserve") == 0


def test_unknown_names_raise(ctx):
    for call in (lambda: ctx.set_option("no_such_option", 1), lambda: ctx.get_option("no_such_option"),
                 lambda: ctx.set_option_f64("no_such_option", 1.0), lambda: ctx.get_option_f64("no_such_option"),
                 lambda: ctx.set_option("guard_band", 1), lambda: ctx.get_option_f64("fused")):   # (each kind has its own calls)
        with pytest.raises(ValueError, match="unknown option"):
            call()
    assert values(ctx) == defaults()


def test_options_restores_on_exit_and_on_an_exception(ctx):
    ctx.set_option("overlap", 1)
    start = values(ctx)
    with ctx.options(fused=0, overlap=0, chain_reserve=3, guard_band=float("inf")):
        assert (ctx.get_option("fused"), ctx.get_option("overlap"), ctx.get_option("chain_reserve")) == (0, 0, 3)
        assert ctx.get_option_f64("guard_band") == float("inf")
    assert values(ctx) == start
    with pytest.raises(RuntimeError, match="the body"):
        with ctx.options(skip_first=0, prepass_gate=100):
            assert ctx.get_option("prepass_gate") == 100
            raise RuntimeError("the body")
    assert values(ctx) == start
    with pytest.raises(ValueError, match="prepass_form"):   # a refused value: what was set before it goes back too
        with ctx.options(chain2=0, prepass_form=7):
            pass
    assert values(ctx) == start


def test_reset_after_setting_everything(ctx):
    for name, (default, lo, hi) in int_options().items():
        ctx.set_option(name, hi if default != hi else lo)
    ctx.set_option_f64("guard_band", 0.5)
    assert all(values(ctx)[name] != defaults()[name] for name in defaults())
    ctx.reset_options()
    assert values(ctx) == defaults()
