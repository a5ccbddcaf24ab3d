"""The Python binding is read from include/romanhip.h (romanimpreprocess_amd/_header.py): gcc is the judge of what the parser
made of the header, and ``_native.marshal`` is tried without a GPU."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from conftest import REPO

from romanimpreprocess_amd import _header, _native

INCLUDE = os.path.join(REPO, "include")
FLOATS = (C.c_float, C.c_double)


def _header_text():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(INCLUDE, "romanhip.h")).read(), flags=re.S)


def _gcc_prints(tmp_path, body, top=""):
    """the lines a C program with ``body`` in main() prints, as lists of words"""
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "romanhip.h"\n' + top + "\nint main(void){\n" + body
                   + "return 0;}\n")
    subprocess.check_call(["gcc", "-Werror=incompatible-pointer-types", "-I", INCLUDE, str(src), "-o", str(exe)])
    return [line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()]


def test_every_constant_equals_the_compilers(tmp_path):
    consts = _native.HEADER.constants
    # nothing the header names is missing from the parse: every RIP_<CAPITALS> word outside the comments is a constant
    named = set(re.findall(r"\bRIP_[A-Z0-9_]+\b", _header_text()))
    assert named == set(consts), named ^ set(consts)
    got = _gcc_prints(tmp_path, "".join(f'printf("{k} %lld\\n", (long long)({k}));\n' for k in consts))
    assert {k: int(v) for k, v in got} == consts
    for k, v in consts.items():   # the module attributes are these values
        assert getattr(_native, k) == v
        if k.startswith(("RIP_STAGE_", "RIP_BIAS_")):
            assert getattr(_native, k[4:]) == v
    assert _native.STAGE_ALL == 0x7F and _native.RIP_SIP_MAX_ORDER == 9 and _native.RIP_MAX_GROUPS == 64


def _scalar_facts(ctype):
    """[size, signed, float] of a ctypes scalar, as the C program prints them"""
    return [C.sizeof(ctype), 1 if ctype in FLOATS else int(ctype(-1).value < 0), int(ctype in FLOATS)]


def test_every_prototype_matches_the_compilers(tmp_path):
    """Per parameter and return type, from the type text of the header: sizeof, signedness and floatness as gcc sees them equal
    those of the ctypes type in SYMBOLS; a function pointer made of the parsed parameter types must take the declared function
    (gcc refuses another count or another pointer type)."""
    protos = _native.PROTOTYPES
    declared = set(re.findall(r"\b(rip_[a-z0-9_]+)\s*\(", _header_text()))
    assert declared == set(protos) == set(_native.SYMBOLS)
    top, body, want = [], [], {}
    for name, p in protos.items():
        res, args = _native.SYMBOLS[name]
        assert len(args) == len(p.params) and res is p.restype
        top.append(f"static {p.rettext} (*const probe_{name})({', '.join(q.ctext for q in p.params) or 'void'}) = {name};\n")
        entries = [(f"{i}:{q.name}", q.ctext, q.depth, args[i]) for i, q in enumerate(p.params)]
        if p.rettext != "void":
            entries.append(("return", p.rettext, p.rettext.count("*"), res))
        for tag, ctext, depth, ctype in entries:
            key = f"{name}/{tag}"
            if depth:
                body.append(f'printf("{key} %zu\\n", sizeof({ctext}));\n')
                want[key] = [C.sizeof(ctype)]
            else:
                body.append(f'printf("{key} %zu %d %d\\n", sizeof({ctext}), ({ctext})-1 < ({ctext})0, ({ctext})0.5 != ({ctext})0);\n')
                want[key] = _scalar_facts(ctype)
    src = tmp_path / "protos.c"   # compiled only: the function pointers need no library
    src.write_text('#include <stddef.h>\n#include "romanhip.h"\n' + "".join(top))
    subprocess.check_call(["gcc", "-c", "-Werror", "-Wall", "-Wno-unused-variable", "-Wno-unused-const-variable", "-I", INCLUDE,
                           str(src), "-o", str(tmp_path / "protos.o")])
    got = {k: [int(v) for v in rest] for k, *rest in _gcc_prints(tmp_path, "".join(body))}
    assert got.keys() == want.keys()
    for key in want:
        assert got[key] == want[key], f"{key}: gcc {got[key]}, ctypes {want[key]}"
    # the rule for pointers
    a = dict(zip((q.name for q in protos["rip_option_info"].params), _native.SYMBOLS["rip_option_info"][1]))
    assert a["name"] == C.POINTER(C.c_char_p) and a["def"] is C.c_void_p and a["index"] is C.c_int
    assert _native.SYMBOLS["rip_set_option"][1] == [C.c_void_p, C.c_char_p, C.c_int]
    assert _native.SYMBOLS["rip_calibrate"][1][4:] == [C.POINTER(_native.RampDesc), C.POINTER(_native.Outputs)]
    assert _native.SYMBOLS["rip_last_error"] == (C.c_char_p, [C.c_void_p]) and _native.SYMBOLS["rip_ctx_destroy"][0] is None
    assert _native.SYMBOLS["rip_host_alloc"] == (C.c_void_p, [C.c_void_p, C.c_size_t])
    elems = {q.name: q.elem for q in protos["rip_stage_select_ranks"].params}
    assert elems["arr"] == "float" and elems["ranks"] == "int64_t" and elems["ctx"] == "rip_ctx" and elems["ny"] is None
    assert [q.elem for q in protos["rip_stage_build_mask"].params if q.name == "grow"] == ["uint8_t"]   # an array parameter


# ---- marshal ---------------------------------------------------------------------------------------------------------------
def _bin_mean_args(**over):
    a = np.arange(96, dtype=np.float32).reshape(8, 12)
    args = dict(ctx=None, arr=a, mask=np.zeros((8, 12), np.uint8), ny=8, nx=12, k=4, out=np.empty((2, 3), np.float32))
    args.update(over)
    return args


def test_marshal_passes_what_the_header_declares():
    args = _bin_mean_args()
    got = _native.marshal("rip_stage_bin_mean", tuple(args.values()))
    assert got == [None, args["arr"].ctypes.data, args["mask"].ctypes.data, 8, 12, 4, args["out"].ctypes.data]
    assert all(type(v) is int for v in got[1:])
    # None is NULL, a bool mask goes where uint8_t is declared, an int is an address, numpy and bool scalars are scalars
    m = np.zeros((8, 12), bool)
    got = _native.marshal("rip_stage_bin_mean", tuple(_bin_mean_args(mask=m, ny=np.int64(8), k=np.int32(4)).values()))
    assert got[2] == m.ctypes.data and got[3:6] == [8, 12, 4] and all(type(v) is int for v in got[3:6])
    assert _native.marshal("rip_stage_bin_mean", tuple(_bin_mean_args(mask=None).values()))[2] is None
    assert _native.marshal("rip_stage_bin_mean", tuple(_bin_mean_args(arr=0x7F0000001000).values()))[1] == 0x7F0000001000
    assert _native.marshal("rip_profile_enable", (None, True)) == [None, 1]
    # by C type: double and float parameters become float, size_t / uint64_t stay int
    got = _native.marshal("rip_stage_gauss_hist", (None, None, 5, None, np.int64(3), np.float32(0.5), None))
    assert got == [None, None, 5, None, 3, 0.5] + [None] and type(got[5]) is float and type(got[4]) is int
    # void * takes any dtype; ctypes objects go through, a struct by reference; text for const char *
    k64 = np.zeros((3, 3, 2, 2), np.float64)
    assert _native.marshal("rip_stage_correct_cube", (None, None, 1, 2, 2, 0, k64, 1, None, 0))[6] == k64.ctypes.data
    n, out8 = C.c_int(0), (C.c_int * 8)()
    ref = C.byref(n)
    assert _native.marshal("rip_last_prepass_gate", (None, ref))[1] is ref
    assert _native.marshal("rip_last_chain_geometry", (None, out8))[1] is out8
    d = _native.PlanDesc()
    by = _native.marshal("rip_plan_desc_first_weight_zero", (d,))[0]
    assert type(by) is type(ref) and not isinstance(by, C.Structure)
    assert _native.marshal("rip_set_option", (None, "fused", 0))[1] == b"fused"


@pytest.mark.parametrize("over, words", [
    (dict(arr=np.zeros((8, 12), np.float64)), ("'arr'", "float32", "float64")),
    (dict(arr=np.zeros((8, 24), np.float32)[:, ::2]), ("'arr'", "non-contiguous")),
    (dict(mask=np.zeros((8, 12), np.int32)), ("'mask'", "uint8", "int32")),
    (dict(ny=np.zeros(3, np.int32)), ("'ny'", "scalar")),
    (dict(k=[4]), ("'k'", "scalar")),
    (dict(out=[1.0, 2.0]), ("'out'", "list")),
])
def test_marshal_refuses_what_the_header_does_not_declare(over, words):
    with pytest.raises(TypeError) as e:
        _native.marshal("rip_stage_bin_mean", tuple(_bin_mean_args(**over).values()))
    assert "rip_stage_bin_mean" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)


def test_marshal_counts_the_arguments():
    with pytest.raises(TypeError, match=r"rip_stage_bin_mean takes 7 arguments \(ctx, arr, mask, ny, nx, k, out\), got 6"):
        _native.marshal("rip_stage_bin_mean", tuple(_bin_mean_args().values())[:-1])


def test_marshal_checks_torch_tensors_by_width_and_kind():
    import torch

    a, m = torch.zeros((8, 12), dtype=torch.float32), torch.zeros((8, 12), dtype=torch.uint8)
    got = _native.marshal("rip_stage_bin_mean", tuple(_bin_mean_args(arr=a, mask=m).values()))
    assert got[1] == a.data_ptr() and got[2] == m.data_ptr()
    # u16 bits in an int16 tensor, u32 bits in an int32 tensor
    cube, out = torch.zeros((2, 4, 4), dtype=torch.int16), torch.zeros((4, 4), dtype=torch.float32)
    assert _native.marshal("rip_stats_l1_diff", (None, cube, 2, 4, 4, 1, 0, out))[1] == cube.data_ptr()
    for bad, word in ((a.double(), "float64"), (a.to(torch.int32), "int32"), (torch.zeros((8, 24))[:, ::2], "non-contiguous")):
        with pytest.raises(TypeError, match="rip_stage_bin_mean: parameter 'arr'") as e:
            _native.marshal("rip_stage_bin_mean", tuple(_bin_mean_args(arr=bad).values()))
        assert word in str(e.value)


def test_location_of_tells_host_arrays_and_refuses_the_rest():
    assert _native.location_of(np.zeros(3)) == _native.RIP_HOST
    assert _native.location_of(np.zeros((2, 3), np.uint16)[:, 1:]) == _native.RIP_HOST   # a view is a numpy array too
    for other in (None, [1.0, 2.0], 7, np.float32(1), b"abc", np.zeros(3).ctypes.data):
        with pytest.raises(TypeError, match="location_of"):
            _native.location_of(other)
    import torch

    with pytest.raises(TypeError, match="location_of"):   # host memory, but no numpy array: .numpy() says which bytes are meant
        _native.location_of(torch.zeros(3))


def test_call_needs_no_context_for_the_entries_without_one():
    assert _native.call("rip_version") == 100
    assert _native.call("rip_chain_form_for", 9, 8, _native.RIP_F32, _native.RIP_F32) == 2
    assert _native.call("rip_plan_desc_first_weight_zero", _native.PlanDesc()) == 0


# ---- what the parser refuses -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text, line", [
    ("int rip_a(int n);\nint rip_b(int n,\n          long double x);\n", 3),                      # an unknown type
    ("int rip_a(int n);\n\nint rip_b(int n, rip_thing *p);\n", 3),                                 # an undeclared struct
    ("typedef struct {\n    int32_t a;\n    int32_t b : 3;\n} rip_s;\n", 3),                       # a bit-field
    ("int rip_a(int n);\nint rip_cb(int n,\n           void (*cb)(int));\n", 2),                    # a function-pointer parameter
    ("#define RIP_N 4\ntypedef struct {\n    float t[RIP_M];\n} rip_s;\n", 3),                     # an unknown array length
    ("int rip_a(int n);\n#pragma pack(1)\n", 2),                                                  # a preprocessor line
    ("typedef struct { int32_t a; } rip_s;\nint rip_a(rip_s s);\n", 2),                            # a struct by value
])
def test_parser_refuses_what_it_does_not_know(text, line):
    with pytest.raises(_header.HeaderError, match=rf"^line {line}:"):
        _header.parse(text)


def test_parser_reads_the_declarations_the_header_uses():
    h = _header.parse("""
        #define RIP_N 4
        enum { RIP_A = 3, RIP_B = 1 << 4, RIP_C = 0x7f, RIP_D };
        typedef struct rip_ctx rip_ctx;
        typedef struct rip_t {
            int32_t a, b, c;      /* three */
            const float *p, *q;
            float t[RIP_N];
            double cd[2][2];
            double s[RIP_N + 1][RIP_N + 1];
        } rip_t;
        int rip_f(rip_ctx *ctx, const rip_t *d, int out[8], const uint8_t grow[32], const char **names, size_t n, unsigned m);
    """)
    assert h.constants == {"RIP_N": 4, "RIP_A": 3, "RIP_B": 16, "RIP_C": 127, "RIP_D": 128}
    t = h.structs["rip_t"]
    assert [(n, c) for n, c in t._fields_] == [
        ("a", C.c_int32), ("b", C.c_int32), ("c", C.c_int32), ("p", C.c_void_p), ("q", C.c_void_p), ("t", C.c_float * 4),
        ("cd", (C.c_double * 2) * 2), ("s", (C.c_double * 5) * 5)]
    f = h.prototypes["rip_f"]
    assert [q.ctype for q in f.params] == [C.c_void_p, C.POINTER(t), C.c_void_p, C.c_void_p, C.POINTER(C.c_char_p), C.c_size_t,
                                           C.c_uint]
    assert [q.elem for q in f.params] == ["rip_ctx", "rip_t", "int", "uint8_t", "char", None, None] and f.restype is C.c_int
