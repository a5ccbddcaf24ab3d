"""The library's option table as the binding sees it (rip_option_info): no GPU."""

from romanimpreprocess_amd import _native

NAMES = {"fused", "chain2", "chain_quad", "skip_first", "chain_reserve", "prepass_form", "prepass_gate", "pink_form", "overlap",
         "chain_dbg", "guard_band"}


def test_option_table_lists_the_eleven_options():
    assert set(_native.option_table()) == NAMES and len(_native.option_table()) == 11


def test_every_default_lies_inside_its_range():
    for name, (default, lo, hi) in _native.option_table().items():
        assert lo <= default <= hi, f"{name}: default {default} outside {lo} .. {hi}"


def test_reserve_none_is_the_default_of_chain_reserve():
    default = _native.option_table()["chain_reserve"][0]
    args = (9, 8, _native.RIP_F32, 64, 512, 256)   # one 8-group f32 frame of 64 x 512 on 256 compute units
    g = _native.chain_geometry_for(*args, reserve=None)
    assert g is not None and g == _native.chain_geometry_for(*args, reserve=default)
