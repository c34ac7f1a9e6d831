"""ctypes binding of libxsd_hip.so, derived from its C ABI: include/xsd.h is parsed once at import and is the only declaration
of every entry and struct (the header's first comment lists the forms accepted).  Fails loudly if the library is missing or the
header holds a form the parser does not know."""
from __future__ import annotations

import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG_ROOT = os.path.dirname(os.path.dirname(_HERE))          # .../xmm-superres-denoise_amd
LIB_PATH = os.environ.get("XSD_LIB") or os.path.join(_PKG_ROOT, "lib", "libxsd_hip.so")   # XSD_LIB: A/B builds
CSRC_DIR = os.path.join(_PKG_ROOT, "csrc")
HEADER_PATH = os.path.join(os.path.dirname(_PKG_ROOT), "include", "xsd.h")      # csrc/ includes it as "../../include/xsd.h"

_lib = None


class XsdError(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "long long": ctypes.c_longlong,
            "float": ctypes.c_float, "double": ctypes.c_double}
_RETURNS = dict(_SCALARS, **{"void": None, "char *": ctypes.c_char_p})


def _words(text: str) -> list:
    return [w for w in text.replace("*", " * ").split() if w != "const"]


def _declarator(text: str, structs: dict, decl: str):
    """'int32_t depths[16]' -> ('depths', c_int32 * 16); 'const float* dev_x' -> ('dev_x', c_void_p).  A pointer to a struct the header
    has defined becomes POINTER(its class) and every other pointer c_void_p; what is neither that nor a scalar raises."""
    m = re.fullmatch(r"([\w\s*]+?)(\w+)\s*(?:\[(\d+)\])?", text.strip())
    words = _words(m.group(1)) if m else []
    base = words[:words.index("*")] if "*" in words else words
    if " ".join(words) in _SCALARS:
        t = _SCALARS[" ".join(words)]
    elif base and set(words[len(base):]) == {"*"}:
        t = ctypes.POINTER(structs[base[0]]) if len(words) == 2 and base[0] in structs else ctypes.c_void_p
    else:
        raise XsdError(f"include/xsd.h: unsupported type or declarator '{text.strip()}' in: {decl}")
    return m.group(2), t * int(m.group(3)) if m.group(3) else t


def _fields(body: str, structs: dict, decl: str) -> list:
    fields = []
    for stmt in filter(None, (s.strip() for s in body.split(";"))):
        first, *more = stmt.split(",")
        if more and "*" in stmt:      # `float *a, b` declares two types: not taken
            raise XsdError(f"include/xsd.h: unsupported field '{stmt}' in: {decl}")
        fields.append(_declarator(first, structs, decl))
        fields += [_declarator(first[:first.rindex(fields[-1][0])] + d, structs, decl) for d in more]
    return fields


def parse_header(text: str):
    """-> (structs {name: ctypes.Structure class}, entries {name: (restype, argtypes)}), both in the header's order."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)                                             # comments
    text = re.sub(r"^[ \t]*#ifdef __cplusplus\s.*?^[ \t]*#endif[ \t]*$", " ", text, flags=re.S | re.M)      # extern "C" { and its }
    text = re.sub(r"^[ \t]*#(?:.*\\\n)*.*$", " ", text, flags=re.M)                                         # preprocessor lines
    decls = re.findall(r"((?:[^;{}]|\{[^{}]*\})*);", text)                    # statements: up to each ';' outside braces
    if "".join(d + ";" for d in decls).strip() != text.strip():
        raise XsdError("include/xsd.h: nested or unbalanced braces, or text after the last ';'")
    structs, entries = {}, {}
    for decl in (" ".join(d.split()) for d in decls):
        if not decl or re.fullmatch(r"typedef struct (\w+) \1", decl) or re.fullmatch(r"enum( \w+)? ?\{[^{}]*\}", decl):
            continue                                                             # opaque handles and enums: nothing to bind
        m = re.fullmatch(r"typedef struct (xsd_\w+) ?\{(.*)\} ?\1", decl)
        if m:
            structs[m.group(1)] = type(m.group(1), (ctypes.Structure,), {"_fields_": _fields(m.group(2), structs, decl)})
            continue
        m = re.fullmatch(r"(.+?)\b(xsd_\w+) ?\((.*)\)", decl)
        ret, params = (" ".join(_words(m.group(1))), m.group(3).strip()) if m else ("", "")
        if ret not in _RETURNS or m.group(2) in entries or "[" in params:        # (an array parameter is a pointer in C: not taken)
            raise XsdError(f"include/xsd.h: unsupported declaration: {decl}")
        entries[m.group(2)] = (_RETURNS[ret], [] if params == "void" else [_declarator(p, structs, decl)[1] for p in params.split(",")])
    return structs, entries


with open(HEADER_PATH) as _f:
    STRUCTS, ENTRIES = parse_header(_f.read())
ABI_SYMBOLS = list(ENTRIES)          # every entry include/xsd.h declares, in its order
XsdConfig, XsdLossConfig, XsdTestOut, XsdTestGconvArgs = (STRUCTS[n] for n in ("xsd_config", "xsd_loss_config", "xsd_test_out", "xsd_test_gconv_args"))
XsdSwGemmView, XsdRestormerConfig = STRUCTS["xsd_sw_gemm_view"], STRUCTS["xsd_restormer_config"]
XsdSwinFIRConfig, XsdSwinIRConfig, XsdHATConfig = (STRUCTS[n] for n in ("xsd_swinfir_config", "xsd_swinir_config", "xsd_hat_config"))


def build(force: bool = False) -> str:
    """Compile the HIP sources for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    import subprocess
    if force:
        subprocess.check_call(["make", "-C", CSRC_DIR, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", CSRC_DIR, "-j4"], stdout=subprocess.DEVNULL)
    return LIB_PATH


def bind(L):
    """Give every entry of the header its restype and argtypes on a ctypes.CDLL handle of the library (or of a variant of it)."""
    for name, (restype, argtypes) in ENTRIES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
    return L


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise XsdError(f"{LIB_PATH} not found: build it with `make -C {CSRC_DIR}` "
                           "(or __graft_entry__.build()). There is no CPU fallback.")
        _lib = bind(ctypes.CDLL(LIB_PATH))
    return _lib


def check(rc: int):
    if rc != 0:
        raise XsdError(f"libxsd_hip error {rc}: {load().xsd_last_error().decode()}")
