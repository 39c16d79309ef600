"""The binding is derived from include/vampire_hip.h by vampire_amd/_header.py.  Here the C++ compiler, which reads the
same header with a real parser, confirms what the reader took from it -- every structure's layout as ctypes lays it out,
every prototype's return and parameter types -- and small snippets hold the reader to the constructs it claims to
understand and to raising on the rest.  CPU only."""
import ctypes as C
import os
import subprocess

import pytest

from vampire_amd import _capi, _header


def test_the_compiler_agrees_with_the_reader(tmp_path):
    header = _header.read()
    assert len(header.structs) >= 33 and len(header.prototypes) >= 136
    lines = ["#include <cstddef>", "#include <type_traits>", f'#include "{_header.HEADER}"']
    for name, fields in header.structs.items():
        cls = getattr(_capi, name)
        assert [f for f, _, _ in fields] == [f for f, _ in cls._fields_]
        lines.append(f'static_assert(sizeof({name}) == {C.sizeof(cls)}, "{name}");')
        for field, _, _ in fields:
            at = getattr(cls, field)
            lines.append(f'static_assert(offsetof({name}, {field}) == {at.offset} && sizeof({name}::{field}) == {at.size}, '
                         f'"{name}.{field}");')
    for name, (ret, params) in header.prototypes.items():
        assert len(params) == len(_capi.SIGNATURES[name][1])
        types = ", ".join(t for t, _ in params)
        lines.append(f'static_assert(std::is_same<decltype(&{name}), {ret} (*)({types})>::value, "{name}");')
    for name, value in header.constants.items():
        lines.append(f'static_assert({name} == {value}, "{name}");')
    src = tmp_path / "header_binding.cpp"
    src.write_text("\n".join(lines) + "\n")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    run = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-4000:]


def test_the_compiler_would_notice(tmp_path):
    """The same kind of file with one wrong parameter type does not compile: the check above can fail."""
    src = tmp_path / "wrong.cpp"
    src.write_text(f'#include <type_traits>\n#include "{_header.HEADER}"\n'
                   'static_assert(std::is_same<decltype(&vamp_debug_checks), int (*)(float)>::value, "wrong");\n')
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    run = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert run.returncode != 0 and "wrong" in run.stderr


SNIPPET = """
/* a comment with a prototype in it: int vamp_ghost(void); */
#define VAMP_CAP 4   /* a trailing
                        comment */
#define VAMP_NONE (-1)
enum { VAMP_A = 2, VAMP_B, VAMP_C = 0x10, VAMP_D };
enum { VAMP_R_X = 0, VAMP_R_Y, VAMP_R_COUNT };
typedef struct VampSeg { const void* src; int64_t n; } VampSeg;
typedef struct {
  int32_t a, b[3];
  float lo[VAMP_CAP];
  int64_t offset[VAMP_R_COUNT];
  VampSeg seg[VAMP_CAP];
} VampAnon;
size_t vamp_bytes(const VampAnon* d);
const char* vamp_text(void);
int vamp_run(const VampAnon* d, const float* xs, const float* xs_host, const void* const* rows_host,
             int32_t patch[2], VampSeg* out, void* stream);
"""


def test_reader_constructs():
    h = _header.parse(SNIPPET)
    assert h.constants == {"VAMP_CAP": 4, "VAMP_NONE": -1, "VAMP_A": 2, "VAMP_B": 3, "VAMP_C": 16, "VAMP_D": 17,
                           "VAMP_R_X": 0, "VAMP_R_Y": 1, "VAMP_R_COUNT": 2}           # implicit enum values
    assert list(h.structs) == ["VampSeg", "VampAnon"]                                 # the anonymous typedef by its name
    assert h.structs["VampSeg"] == [("src", "const void*", ()), ("n", "int64_t", ())]
    assert h.structs["VampAnon"] == [("a", "int32_t", ()), ("b", "int32_t", (3,)), ("lo", "float", (4,)),
                                     ("offset", "int64_t", (2,)),                     # an array sized by an enum count
                                     ("seg", "VampSeg", (4,))]
    assert "vamp_ghost" not in h.prototypes
    assert h.prototypes["vamp_bytes"] == ("size_t", [("const VampAnon*", "d")])
    assert h.prototypes["vamp_text"] == ("const char*", [])
    assert h.prototypes["vamp_run"] == ("int", [
        ("const VampAnon*", "d"), ("const float*", "xs"), ("const float*", "xs_host"),     # a _host pointer
        ("const void* const*", "rows_host"),                                               # T* const*
        ("int32_t*", "patch"),                                                             # an array declarator
        ("VampSeg*", "out"), ("void*", "stream")])


def test_binding_rules_on_the_real_header():
    """What _capi makes of the kinds of parameter above, on entry points that have them."""
    sig = _capi.SIGNATURES
    names = {fn: [p for _, p in params] for fn, (_, params) in _header.read().prototypes.items()}
    arg = lambda fn, p: sig[fn][1][names[fn].index(p)]
    assert arg("vamp_render_bev_forward_ex", "ozs_host") is C.POINTER(C.c_float)
    assert arg("vamp_render_bev_forward_ex", "ozs") is _capi.TensorPtr
    assert arg("vamp_reg_loss_forward", "pred_host") is _capi.TensorPtr
    assert arg("vamp_lift_cull_words", "patch") is _capi.TensorPtr
    assert arg("vamp_lift_cull_words", "d") is C.POINTER(_capi.VampLiftDesc)
    assert arg("vamp_lift_forward_plan", "out") is C.POINTER(_capi.VampLiftForwardPlan)
    assert sig["vamp_profile_read"][1] == [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_double)]
    assert _capi.RENDERWS_REGIONS[:3] == ("packed", "grad", "gcl") and len(_capi.RENDERWS_REGIONS) == 19
    assert _capi.LIFTWS_REGIONS[0] == "feat_cl" and _capi.LIFTWS_REGIONS[-1] == "cull" and len(_capi.LIFTWS_REGIONS) == 13
    assert _capi.ABI_VERSION == _capi.VAMP_ABI_VERSION == 16 and _capi.VAMP_IMG_OUT_NONE == -1


@pytest.mark.parametrize("text,line,message", [
    ("\n\nint vamp_x(const float* a, quad b);\n", 3, "unknown type 'quad'"),
    ("typedef struct VampS { int32_t a; Missing m; } VampS;", 1, "unknown type 'Missing'"),
    ("int vamp_ok(void);\nint vamp_x(int a, int (*callback)(int));\n", 2, "cannot parse"),
    ("int vamp_ok(void);\n\nstruct VampS { int a; };\n", 3, "cannot parse"),
    ("int vamp_x(int);\n", 1, "unknown type ''"),
    ("#define VAMP_N (1 << 3)\n", 1, "cannot evaluate"),
    ("enum { VAMP_A = VAMP_NOWHERE };\n", 1, "cannot evaluate"),
    ("typedef struct VampS { float x[VAMP_NOWHERE]; } VampS;", 1, "cannot evaluate"),
    ("typedef struct VampS { float* a, b; } VampS;", 1, "one pointer field"),
    ("typedef struct VampS { int a; } VampT;", 1, "another name"),
])
def test_reader_raises_naming_the_line(text, line, message):
    with pytest.raises(_header.HeaderError) as e:
        _header.parse(text)
    assert str(e.value).startswith(f"line {line}: ") and message in str(e.value), str(e.value)
