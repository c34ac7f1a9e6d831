"""engine/_lib.py derives the ctypes binding from include/xsd.h.  Held here without a GPU: the parser on synthetic header text (every
form it accepts, and that anything else raises with the declaration quoted), the generated structs against the C compiler's sizeof /
offsetof, and that every parsed entry carries a signature of the declaration's length."""
import ctypes
import os
import re
import subprocess

import pytest

from xmm_superres_denoise.engine import _lib
from xmm_superres_denoise.engine._lib import XsdError, parse_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = ctypes.c_void_p

SYNTHETIC = """
/* a comment that looks like code: int xsd_foo(int) and an unbalanced ( ( paren; */
#ifndef SYN_H
#define SYN_H
#include <stdint.h>
#define SYN_MACRO(a, b) \\
    int xsd_not_an_entry(int a);
#ifdef __cplusplus
extern "C" {
#endif
typedef struct xsd_handle xsd_handle;          // opaque; int xsd_bar(void);
enum xsd_e { XSD_A = 0, XSD_B };
enum { XSD_C, XSD_D };
typedef struct xsd_s {
    int32_t a[16];   /* fixed array */
    double x, y;
    const float* p; long long n;
    int k; int64_t m; float f, g[3];
    unsigned short* bits;
} xsd_s;
typedef struct xsd_t { const xsd_s* inner; xsd_handle* h; int32_t last; } xsd_t;
const char* xsd_name(void);
void xsd_free(xsd_handle* h);
int xsd_i(int a, int32_t b, int64_t c, long long d, float e, double f);
int32_t xsd_i32(int a);
int64_t xsd_i64(int a);
long long xsd_ll(int a);
float xsd_f(int a);
double xsd_d(int a);
int xsd_ptrs(const float* a, float** b, const float* const* c, const xsd_s* defined, xsd_handle* opaque, xsd_handle** out,
             xsd_s** pp, unsigned long long* u, const uint8_t* bytes, void* stream);
int
xsd_three_lines(const xsd_t* t,
                int n);
#ifdef __cplusplus
}
#endif
#endif /* SYN_H */
"""


def test_parser_accepts_every_form_of_the_header():
    structs, entries = parse_header(SYNTHETIC)
    assert list(structs) == ["xsd_s", "xsd_t"]
    s, t = structs["xsd_s"], structs["xsd_t"]
    assert issubclass(s, ctypes.Structure) and s.__name__ == "xsd_s"
    assert s._fields_ == [("a", ctypes.c_int32 * 16), ("x", ctypes.c_double), ("y", ctypes.c_double), ("p", VP), ("n", ctypes.c_longlong),
                          ("k", ctypes.c_int), ("m", ctypes.c_int64), ("f", ctypes.c_float), ("g", ctypes.c_float * 3), ("bits", VP)]
    assert t._fields_ == [("inner", ctypes.POINTER(s)), ("h", VP), ("last", ctypes.c_int32)]
    assert list(entries) == ["xsd_name", "xsd_free", "xsd_i", "xsd_i32", "xsd_i64", "xsd_ll", "xsd_f", "xsd_d", "xsd_ptrs", "xsd_three_lines"]
    assert entries["xsd_name"] == (ctypes.c_char_p, [])                      # (void)
    assert entries["xsd_free"] == (None, [VP])
    assert entries["xsd_i"] == (ctypes.c_int, [ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_longlong, ctypes.c_float, ctypes.c_double])
    assert [entries[n][0] for n in ("xsd_i32", "xsd_i64", "xsd_ll", "xsd_f", "xsd_d")] == \
        [ctypes.c_int32, ctypes.c_int64, ctypes.c_longlong, ctypes.c_float, ctypes.c_double]
    # only a single pointer to a struct defined completely is typed
    assert entries["xsd_ptrs"] == (ctypes.c_int, [VP, VP, VP, ctypes.POINTER(s), VP, VP, VP, VP, VP, VP])
    assert entries["xsd_three_lines"] == (ctypes.c_int, [ctypes.POINTER(t), ctypes.c_int])
    # nothing inside a comment or a macro became an entry
    assert not {"xsd_foo", "xsd_bar", "xsd_not_an_entry"} & set(entries)


@pytest.mark.parametrize("decl", [
    "int xsd_bad(short a)",                              # a scalar outside the table
    "int xsd_bad(unsigned a)",
    "short xsd_bad(int a)",                              # ... as return type
    "float* xsd_bad(int a)",                             # a pointer return other than const char*
    "int xsd_bad(void (*cb)(int), int n)",               # a function-pointer parameter
    "int xsd_bad(int a[4])",                             # an array parameter
    "int xsd_bad(xsd_s by_value)",                       # a struct by value
    "int xsd_bad(int a, ...)",
    "int other_prefix(int a)",
    "typedef struct xsd_u { short a; } xsd_u",
    "typedef struct xsd_u { int (*cb)(int); } xsd_u",
    "typedef struct xsd_u { float *a, b; } xsd_u",       # two types in one statement
    "typedef struct xsd_u { int n[XSD_C]; } xsd_u",      # an array length that is no literal
    "typedef struct xsd_u { struct { int a; } in; } xsd_u",
    "typedef struct xsd_u { int a; } xsd_v",
    "typedef int xsd_int",
    "extern int xsd_global",
])
def test_parser_refuses_what_it_cannot_map(decl):
    head = "typedef struct xsd_s { int a; } xsd_s;\nenum { XSD_C = 4 };\n"
    parse_header(head + "int xsd_ok(const xsd_s* s);")
    with pytest.raises(XsdError) as e:
        parse_header(head + decl + ";\nint xsd_ok(const xsd_s* s);")
    if "struct {" not in decl:                           # (nested braces are refused before the text is cut into declarations)
        assert " ".join(decl.split()) in str(e.value)


def test_parser_refuses_a_redeclared_entry_and_loose_text():
    with pytest.raises(XsdError, match="xsd_twice"):
        parse_header("int xsd_twice(int a);\nint xsd_twice(int a);")
    with pytest.raises(XsdError):
        parse_header("int xsd_a(int a);\nint xsd_b(int b)")          # no ';' after the last declaration
    with pytest.raises(XsdError):
        parse_header("int xsd_a(int a); }")


def test_every_entry_of_the_header_has_a_signature():
    hdr = open(os.path.join(ROOT, "include", "xsd.h")).read()
    assert _lib.HEADER_PATH == os.path.join(ROOT, "include", "xsd.h")
    assert set(re.findall(r"\b(xsd_[a-z0-9_]+)\s*\(", hdr)) >= set(_lib.ABI_SYMBOLS)        # (the regex also sees names inside comments)

    class Fn:
        pass

    class Handle:
        def __getattr__(self, n):
            return self.__dict__.setdefault(n, Fn())

    L = _lib.bind(Handle())
    assert set(vars(L)) == set(_lib.ABI_SYMBOLS)
    bare = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    for n in _lib.ABI_SYMBOLS:
        fn = getattr(L, n)
        params = re.search(r"\b%s\s*\(([^)]*)\)" % n, bare).group(1)
        assert isinstance(fn.argtypes, list) and len(fn.argtypes) == (0 if params.strip() == "void" else params.count(",") + 1), n
        assert fn.restype in (None, ctypes.c_char_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double), n
        assert (fn.restype, fn.argtypes) == _lib.ENTRIES[n]
    assert L.xsd_debug_residency_ms.restype is ctypes.c_float and L.xsd_last_error.restype is ctypes.c_char_p
    assert L.xsd_loss_create.argtypes == [ctypes.POINTER(_lib.XsdLossConfig), VP]
    names = {"XsdConfig": "xsd_config", "XsdLossConfig": "xsd_loss_config", "XsdTestOut": "xsd_test_out", "XsdTestGconvArgs": "xsd_test_gconv_args",
             "XsdSwGemmView": "xsd_sw_gemm_view", "XsdRestormerConfig": "xsd_restormer_config", "XsdSwinFIRConfig": "xsd_swinfir_config",
             "XsdSwinIRConfig": "xsd_swinir_config", "XsdHATConfig": "xsd_hat_config"}
    assert set(names.values()) == set(_lib.STRUCTS)
    for alias, n in names.items():
        assert getattr(_lib, alias) is _lib.STRUCTS[n]


def test_struct_layout_matches_the_c_compiler(tmp_path):
    """sizeof of every struct and offsetof of every field, printed by a C program that includes xsd.h, against the generated classes."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "xsd.h"', 'int main(void) {']
    for n, cls in _lib.STRUCTS.items():
        lines.append(f'    printf("{n} %zu\\n", sizeof({n}));')
        lines += [f'    printf("{n}.{f} %zu\\n", offsetof({n}, {f}));' for f, _ in cls._fields_]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    cc = os.environ.get("CC", "gcc")                     # the compiler oracle/Makefile uses
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    want = {}
    for n, cls in _lib.STRUCTS.items():
        want[n] = str(ctypes.sizeof(cls))
        want.update({f"{n}.{f}": str(getattr(cls, f).offset) for f, _ in cls._fields_})
    assert len(_lib.STRUCTS) >= 9 and got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
