"""rip_chain_form_for: which (Legendre planes, group count, ipc4d dtype, gain dtype) have a fused-kernel form.  No GPU needed:
the library loads without one."""

import pytest

from romanimpreprocess_amd import _native

F32, F64 = _native.RIP_F32, _native.RIP_F64


@pytest.mark.parametrize("ipc_dtype", [F32, F64])
@pytest.mark.parametrize("planes", [4, 9, 11])
def test_every_group_count_from_5_to_16_has_a_fused_form(planes, ipc_dtype):
    for G in range(5, 17):
        assert _native.chain_form_for(planes, G, ipc_dtype, F32) == 2, f"{planes} planes, {G} groups"


@pytest.mark.parametrize("ipc_dtype", [F32, F64])
def test_configurations_without_a_form_report_the_stage_kernels(ipc_dtype):
    lib = _native.load_library()
    for G in (2, 3, 4, 17, 64):
        for planes in (4, 9, 11):
            assert lib.rip_chain_form_for(planes, G, ipc_dtype, F32) == 0, f"{G} groups"
    for G in range(5, 17):
        for planes in (5, 10):
            assert lib.rip_chain_form_for(planes, G, ipc_dtype, F32) == 0, f"{planes} planes"
        for planes in (4, 9, 11):
            assert lib.rip_chain_form_for(planes, G, ipc_dtype, F64) == 0, "f64 gain"


def test_unknown_dtype_codes_report_the_stage_kernels():
    lib = _native.load_library()
    assert lib.rip_chain_form_for(9, 8, _native.RIP_U16, F32) == 0
    assert lib.rip_chain_form_for(9, 8, F32, _native.RIP_U16) == 0
