"""The ctypes binding is derived from include/vaeunet.h (vaeunet_amd/_lib.py):
nothing the header declares is skipped, the parser refuses what it does not
know, and the struct layouts are the host C compiler's.  No GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from vaeunet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vaeunet.h")


def _stripped_header():
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(HEADER).read(), flags=re.S)


def test_nothing_in_the_header_is_skipped():
    """An independent loose scan of the header finds no prototype, struct or
    integer constant that the binding lacks."""
    src = _stripped_header()
    names = set(re.findall(r"\b(vu_[a-z0-9_]+)\s*\(", src))
    assert len(names) > 100 and names == set(_lib._SIGS)
    assert _lib.exported_symbols() == sorted(names)
    structs = re.findall(r"typedef\s+struct\b[^{}]*\{[^{}]*\}\s*(\w+)\s*;", src)
    assert len(structs) == src.count("typedef") >= 9
    for s in structs:
        cls = getattr(_lib, s)
        assert issubclass(cls, ctypes.Structure) and cls.__name__ == s
    defines = re.findall(r"^\s*#\s*define\s+(VU_\w+)\s+([-+]?(?:0[xX][0-9a-fA-F]+|\d+))\s*$", src, flags=re.M)
    assert len(defines) == len(re.findall(r"^\s*#\s*define\s+VU_", src, flags=re.M)) >= 28
    for name, value in defines:
        assert getattr(_lib, name) == int(value, 0), name
    assert _lib.VU_TUNE_ATTN == 22 and _lib.VU_CALIB_RANK_BINS == 1024


REFUSED = {
    "size_t argument": "int vu_f(size_t n, void* stream);",
    "function-pointer argument": "int vu_f(int (*cb)(int), void* stream);",
    "bit-field": "typedef struct S { int32_t a : 3; int32_t b; } S;",
    "struct without typedef": "struct S { int32_t a; };\nint vu_f(const struct S* s);",
    "missing semicolon": "int vu_f(int a)\nint vu_g(int b);",
    "missing last semicolon": "int vu_f(int a);\nint vu_g(int b)",
    "pointer return": "const float* vu_f(int a);",
    "pointer to pointer": "int vu_f(float** rows);",
    "unknown struct": "int vu_f(const Missing* m);",
    "uint8_t by value": "int vu_f(uint8_t flag);",
    "unsigned int": "int vu_f(unsigned int n);",
    "array argument": "int vu_f(int dims[4]);",
    "prototype without the prefix": "int other_f(int a);",
    "pointer with several declarators": "typedef struct S { float* a, b; } S;",
    "unsized array field": "typedef struct S { int32_t n; float tail[]; } S;",
    "union": "typedef union U { int32_t a; float b; } U;",
    "macro constant that is no integer": "#define VU_SCALE 1.5f\nint vu_f(void);",
    "function-like macro": "#define VU_MAX(a, b) ((a) > (b) ? (a) : (b))\nint vu_f(void);",
    "multi-line macro": "#define VU_A \\\n  3\nint vu_f(void);",
    "conditional block": "#if 0\nint vu_f(int a);\n#endif\nint vu_f(void);",
    "conditional on a macro": "#ifdef VU_WIDE\nint vu_f(int64_t a);\n#else\nint vu_f(int a);\n#endif",
    "stray text": "int vu_f(void);\nstatic const int vu_table = 3;",
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_parser_refuses_what_it_does_not_know(case):
    with pytest.raises(ValueError) as e:
        _lib.parse_header(REFUSED[case])
    assert "include/vaeunet.h" in str(e.value)


def test_parser_quotes_the_declaration_it_refuses():
    with pytest.raises(ValueError, match=r"vu_f\(size_t n, void\* stream\)"):
        _lib.parse_header("int vu_ok(void);\nint vu_f(size_t n,\n         void* stream);")
    with pytest.raises(ValueError, match="int32_t a : 3"):
        _lib.parse_header(REFUSED["bit-field"])


def test_parser_accepts_the_documented_forms():
    C = ctypes
    structs, sigs, consts = _lib.parse_header("""
        /* a comment with int vu_not_a_prototype(int); inside */
        #ifndef X_H
        #define X_H
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define VU_A 7   /* trailing comment */
        #define VU_B 0x10
        typedef struct Inner { const void* src[3]; int32_t N, H, W; } Inner;
        typedef struct { Inner a; int64_t stride[3]; float* out; double d; uint32_t u; uint64_t v; } Outer;
        int64_t vu_none(void);
        void vu_empty();
        int vu_mixed(const Outer* args, Inner by_value, const uint8_t* bytes, const int64_t* strides,
                     int n, int64_t m, uint32_t a, uint64_t b, float f, double d, void* stream);  // tail
        #ifdef __cplusplus
        }
        #endif
        #endif
        """)
    assert consts == {"VU_A": 7, "VU_B": 16}
    assert list(structs) == ["Inner", "Outer"] and list(sigs) == ["vu_none", "vu_empty", "vu_mixed"]
    Inner, Outer = structs["Inner"], structs["Outer"]
    assert Inner._fields_ == [("src", C.c_void_p * 3), ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32)]
    assert Outer._fields_ == [("a", Inner), ("stride", C.c_int64 * 3), ("out", C.c_void_p), ("d", C.c_double),
                              ("u", C.c_uint32), ("v", C.c_uint64)]
    assert Outer.stride.offset == C.sizeof(Inner) == 40
    assert sigs["vu_none"] == (C.c_int64, []) and sigs["vu_empty"] == (None, [])
    assert sigs["vu_mixed"] == (C.c_int, [C.POINTER(Outer), Inner, C.c_void_p, C.c_void_p, C.c_int, C.c_int64,
                                          C.c_uint32, C.c_uint64, C.c_float, C.c_double, C.c_void_p])


def test_pointer_arguments_of_the_real_header():
    """Host descriptors are typed, device addresses are not: a struct that the
    caller fills in host memory arrives as POINTER(Struct) (ctypes refuses
    another struct's), every device pointer as c_void_p -- among them the two
    job tables that live in device memory."""
    assert _lib._SIGS["vu_gemm_fwd"] == (_lib._i, [ctypes.POINTER(_lib.VuGemmFwd), _lib._i, _lib._p])
    assert _lib._SIGS["vu_latent_bwd"][1][:3] == [ctypes.POINTER(_lib.VuLatentJob), _lib._i,
                                                  ctypes.POINTER(_lib.VuLatentHeads)]
    assert _lib._SIGS["vu_permute4_batch"] == (_lib._i, [_lib._p, _lib._i, _lib._l, _lib._p])
    assert _lib._SIGS["vu_mt_scale_grads"] == (_lib._i, [_lib._p, _lib._i, _lib._l, _lib._p, _lib._p])
    assert _lib._DEVICE_TABLES <= set(_lib._STRUCTS)
    assert _lib.VuPermJob._fields_[0] == ("inp", _lib._p)
    # what the call sites pass where the uniform rule now says c_void_p
    for arg in (ctypes.byref(ctypes.c_int(0)), (ctypes.c_int64 * 4)(1, 2, 3, 4), None, ctypes.c_void_p(64)):
        _lib._p.from_param(arg)


@pytest.mark.skipif(shutil.which("cc") is None, reason="no host C compiler")
def test_struct_layout_matches_the_host_compiler(tmp_path):
    """sizeof of every struct and offsetof / sizeof of every field, as the
    host C compiler lays out the real header, equal the ctypes values."""
    rows, lines = [], []
    for sname, cls in _lib._STRUCTS.items():
        rows.append((sname, None, ctypes.sizeof(cls), 0))
        lines.append(f'  printf("%zu 0\\n", sizeof({sname}));')
        for fname, _ in cls._fields_:
            desc = getattr(cls, fname)
            rows.append((sname, fname, desc.size, desc.offset))
            lines.append(f'  printf("%zu %zu\\n", sizeof((({sname}*)0)->{fname}), offsetof({sname}, {fname}));')
    assert len(_lib._STRUCTS) >= 9 and len(rows) > 150
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vaeunet.h"\nint main(void) {\n'
                   + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = [tuple(int(v) for v in line.split()) for line in out if line]
    assert len(got) == len(rows)
    wrong = [(r[0], r[1], r[2:], g) for r, g in zip(rows, got) if r[2:] != g]
    assert not wrong, wrong
