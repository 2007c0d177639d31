"""CPU tests of the binding's one source: naruto_amd._lib derives its structures, constants and argument types from include/naruto_hip.h.
The derived layout is held to the compiler's (the one that builds the library against the same header), the parser to refusing what it does
not understand, and the NARUTO_HOST marks to the list of parameters that are host pointers.  Nothing here needs a GPU."""
import ctypes as C
import os
import subprocess

import pytest

from naruto_amd import _lib

# every parameter that points to HOST memory: function -> argument indices
HOST_ARGS = {
    "naruto_field_create": (1,), "naruto_field_levels": (1, 2, 3, 4), "naruto_active_ray_select": (9, 10), "naruto_active_ray_select_rows": (9, 10),
    "naruto_assemble_select": (5, 6), "naruto_goal_targets": (0,), "naruto_goal_aggregate": (0,), "naruto_goal_search": (7,),
    "naruto_lattice_points": (0,), "naruto_mesh_workspace": (0,), "naruto_mesh_count": (0,), "naruto_mesh_emit": (0,), "naruto_nn_grid_plan": (1, 2),
    "naruto_icp_accumulate": (7,), "naruto_icp_step": (2,), "naruto_debug_icp_solve": (0, 1, 2, 3), "naruto_rrt_workspace": (0,),
    "naruto_rrt_start": (1, 2), "naruto_segments_free": (0,), "naruto_fwd_image_bytes": (0, 1), "naruto_debug_train_plan": (4,),
    "naruto_debug_render_plan": (5,), "naruto_debug_random_lines": (4,), "naruto_debug_rodrigues": (0, 1, 2, 3), "naruto_debug_ba_poses_fields": (1,),
    "naruto_debug_pose_adam": (0, 1, 2, 3), "naruto_image_metrics": (9,),
}

# a header in the style of naruto_hip.h that uses every form the parser reads; the refusal cases below spoil one line of it
GOOD = """/* a comment with a ; and a
 * naruto_call(in, it); */
#ifndef NARUTO_MINI_H
#define NARUTO_MINI_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define NARUTO_HOST
#define NARUTO_N 3
#define NARUTO_ERR (-22)      /* negative, in parentheses */
#define NARUTO_FLAG 0x10u
#define NARUTO_BYTES(m) (4u * (m))
typedef struct NarutoThing NarutoThing;
typedef struct NarutoA {
    uint32_t n, m;                 // comma declarators
    const float *p, *q; float x;
    double box[NARUTO_N][2], lo[3];
    void* ws[2];
    int64_t* ids;
    uint8_t flag;
} NarutoA;
typedef struct NarutoB { const struct NarutoA* a; uint64_t k; } NarutoB;
const char* naruto_text(void);
void naruto_drop(NarutoThing* t);
size_t naruto_size(const NarutoThing* t, uint32_t n);
int naruto_make(const NarutoA* a, NARUTO_HOST NarutoThing** out);
int naruto_run(const NarutoThing* t, const float* x /* device */, NARUTO_HOST const double* lo, NARUTO_HOST uint32_t out[8],
               NarutoB* b, int32_t mode, double s, void* stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_every_form_of_declaration_maps_to_its_ctypes_type():
    h = _lib.Header(GOOD)
    assert h.defines == {"NARUTO_N": 3, "NARUTO_ERR": -22, "NARUTO_FLAG": 16} and h.macros == ["NARUTO_BYTES"] and h.opaque == {"NarutoThing"}
    A, B = h.structs["NarutoA"], h.structs["NarutoB"]
    want = [("n", C.c_uint32), ("m", C.c_uint32), ("p", C.c_void_p), ("q", C.c_void_p), ("x", C.c_float), ("box", (C.c_double * 2) * 3),
            ("lo", C.c_double * 3), ("ws", C.c_void_p * 2), ("ids", C.c_void_p), ("flag", C.c_uint8)]
    assert [n for n, _ in A._fields_] == [n for n, _ in want]
    assert all(got is t for (_, got), (_, t) in zip(A._fields_, want))                 # ctypes caches array and pointer types: identity
    assert B._fields_ == [("a", C.c_void_p), ("k", C.c_uint64)]
    assert list(h.functions) == ["naruto_text", "naruto_drop", "naruto_size", "naruto_make", "naruto_run"]
    assert h.functions["naruto_text"] == (C.c_char_p, []) and h.functions["naruto_drop"] == (None, [C.c_void_p])
    assert h.functions["naruto_size"] == (C.c_size_t, [C.c_void_p, C.c_uint32])
    assert h.functions["naruto_make"] == (C.c_int, [C.POINTER(A), C.POINTER(C.c_void_p)])
    assert h.functions["naruto_run"] == (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(B), C.c_int32,
                                                   C.c_double, C.c_void_p])
    assert h.host_args == {"naruto_text": (), "naruto_drop": (), "naruto_size": (), "naruto_make": (1,), "naruto_run": (2, 3)}


# (text of GOOD, what it becomes, the line of mini.h the refused declaration starts on, what the message must name)
@pytest.mark.parametrize("old,new,line,named", [
    ("uint8_t flag;", "uint16_t flag;", 21, "uint16_t flag"),                                          # a type the binding has no rule for
    ("uint32_t n);", "unsigned n);", 26, "naruto_size"),
    ("void naruto_drop(NarutoThing* t);", "void naruto_drop(NarutoOther* t);", 25, "NarutoOther"),
    ("const char* naruto_text(void);", "const char* naruto_text(void)", 24, "naruto_text"),            # a missing ;
    ("int64_t* ids;", "int64_t* ids", 20, "int64_t* ids"),
    ("} NarutoB;", "} NarutoB", 23, "NarutoB"),
    ("#define NARUTO_N 3", "#define NARUTO_N 3.0", 10, "NARUTO_N"),                                    # defines that are not one integer literal
    ("#define NARUTO_FLAG 0x10u", "#define NARUTO_FLAG (1u << 4)", 12, "NARUTO_FLAG"),
    ("#define NARUTO_ERR (-22)", "#define NARUTO_ERR", 11, "NARUTO_ERR"),
    ("#define NARUTO_ERR (-22)", "#define NARUTO_N 4", 11, "repeated"),
    ("typedef struct NarutoThing NarutoThing;", "typedef struct NarutoThing NarutoThing;\nenum NarutoMode { A, B };", 15, "enum NarutoMode"),
    ("typedef struct NarutoThing NarutoThing;", "typedef struct NarutoThing NarutoThing;\nstatic const int naruto_k = 3;", 15, "naruto_k"),
    ("#include <stdint.h>", "#include <stdint.h>\n#if NARUTO_WIDE", 6, "#if NARUTO_WIDE"),
    ("int32_t mode,", "NARUTO_HOST int32_t mode,", 28, "mode"),                                        # the mark on what is no typed pointer
    ("void* stream);", "NARUTO_HOST void* stream);", 28, "stream"),
    ("double box[NARUTO_N][2]", "double box[NARUTO_M][2]", 18, "NARUTO_M"),
])
def test_the_parser_refuses_what_it_does_not_understand(old, new, line, named):
    assert GOOD.count(old) == 1
    bad = GOOD.replace(old, new)
    with pytest.raises(_lib.HeaderError) as e:
        _lib.Header(bad, "mini.h")
    assert str(e.value).startswith(f"mini.h:{line}: ") and named in str(e.value), str(e.value)


def test_the_binding_is_the_header():
    abi = _lib.ABI
    assert len(abi.structs) >= 16 and len(abi.functions) >= 131 and _lib.SIGNATURES is abi.functions
    for name, cls in abi.structs.items():
        assert getattr(_lib, name) is cls and issubclass(cls, C.Structure)
    for name, value in abi.defines.items():
        assert getattr(_lib, name[len("NARUTO_"):]) == value and type(value) is int, name
    assert _lib.GOAL_SEARCH_MAX_TARGETS == 4096 and _lib.RRT_STATE_INTS == 16 and _lib.ICP_STATE_DOUBLES == 24
    assert len(_lib.ICP_STATUS) == 4 and _lib.ICP_STATUS[_lib.ICP_MAX_ITERATION] == "max_iteration"
    # needs_build() watches every file the build can read: nothing in csrc/ is outside the listing
    assert sorted(os.listdir(_lib.CSRC)) == _lib.SOURCES and os.path.exists(_lib.HEADER)


def test_host_pointers_are_typed_and_no_other_scalar_pointer_is():
    abi = _lib.ABI
    assert {k: v for k, v in abi.host_args.items() if v} == HOST_ARGS
    for name, (_, argtypes) in abi.functions.items():
        for i, t in enumerate(argtypes):
            typed = isinstance(t, type) and issubclass(t, C._Pointer)
            if i in abi.host_args[name]:
                assert typed and (t._type_ is C.c_void_p or t._type_ in (C.c_float, C.c_double, C.c_uint32, C.c_int32, C.c_uint64, C.c_size_t)), (name, i, t)
            else:
                assert not typed or t._type_ in abi.structs.values(), (name, i, t)      # POINTER(struct), an address, or a scalar by value
    a, b = C.c_size_t(), C.c_uint32()                          # what the marks are for: ctypes passes a bare scalar by reference
    assert C.POINTER(C.c_size_t) is abi.functions["naruto_fwd_image_bytes"][1][0] and C.POINTER(C.c_uint32) is abi.functions["naruto_fwd_image_bytes"][1][1]
    assert C.POINTER(C.c_size_t).from_param(a) is not None and C.POINTER(C.c_uint32).from_param(b) is not None


def test_layout_and_constants_equal_the_compilers(tmp_path):
    """sizeof of every struct, offsetof and size of every field and the value of every NARUTO_* define, printed by a program that includes
    the header and is built by the compiler that builds the library, against what the binding derived from the same text."""
    abi = _lib.ABI
    lines, want = [], []
    for name, cls in abi.structs.items():
        lines.append(f'printf("%zu\\n", sizeof({name}));')
        want.append((name, C.sizeof(cls)))
        for field, _ in cls._fields_:
            lines.append(f'printf("%zu %zu\\n", offsetof({name}, {field}), sizeof((({name}*)0)->{field}));')
            want += [(f"offsetof {name}.{field}", getattr(cls, field).offset), (f"sizeof {name}.{field}", getattr(cls, field).size)]
    for name, value in abi.defines.items():
        lines.append(f'printf("%lld\\n", (long long)({name}));')
        want.append((name, value))
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "naruto_hip.h"\nint main() {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-x", "c++", "-I", os.path.dirname(_lib.HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert len(got) == len(want) and len(abi.structs) >= 16 and len(abi.defines) >= 47
    assert [(what, v) for (what, _), v in zip(want, got)] == want
