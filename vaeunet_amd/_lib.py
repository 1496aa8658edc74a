"""ctypes binding of the C-ABI library ``libvaeunet_hip.so``, derived from
its header ``include/vaeunet.h`` when this module is imported: the structs,
the prototypes and the integer ``VU_*`` constants are declared there and
nowhere else.

This is the only place the product path touches native code.  There is no
CPU or PyTorch fallback: if the library or the header is missing or a launch
fails the call raises, loudly (the oracle under ``oracle/`` is test
infrastructure only).
"""
import ctypes as C
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvaeunet_hip.so")
# A/B timing of two builds of the same sources (tools/*_bench.py): an
# alternative library file; the product never sets it
if os.environ.get("VU_LIB_PATH"):
    LIB_PATH = os.environ["VU_LIB_PATH"]
HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "vaeunet.h")

F32, BF16 = 0, 1

_p = C.c_void_p
_i = C.c_int
_l = C.c_int64
_f = C.c_float

# The one type map.  A pointer to anything but a parsed struct is c_void_p.
_SCALARS = {"int": _i, "int32_t": C.c_int32, "int64_t": _l, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
            "float": _f, "double": C.c_double}
_POINTEES = set(_SCALARS) | {"void", "uint8_t"}
# Structs whose tables live in device memory: callers hold an address, not a
# ctypes object, so a pointer to one of these stays c_void_p as well.
_DEVICE_TABLES = {"VuPermJob", "VuMtEntry"}

_STRUCT = re.compile(r"\s*typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;")
_PROTO = re.compile(r"\s*([\w\s]+?)\s*\b(vu_\w+)\s*\(([^;{}()]*)\)\s*;")
_NAME = r"\w+(?:\s*\[\s*\d+\s*\])?"
_FIELD = re.compile(r"\s*(?:const\s+)?(\w+)(\s*\*\s*|\s+)(%s(?:\s*,\s*%s)*)\s*$" % (_NAME, _NAME))
_ARG = re.compile(r"\s*(?:const\s+)?(\w+)(?:(\s*\*\s*|\s+)(\w+)?)?\s*$")
_DEFINE = re.compile(r"\s*#\s*define\s+(VU_\w*)(.*)$")
# the include guard, #include and the extern "C" wrapper; no other conditional
_DIRECTIVE = re.compile(r"\s*#\s*(?:include|define|ifndef|endif|ifdef\s+__cplusplus)\b")


def _refuse(decl):
    return ValueError(f"include/vaeunet.h: declaration outside the forms the binding reads: {' '.join(decl.split())!r}")


def _ctype(base, pointer, structs, decl):
    if pointer:
        if base in structs:
            return _p if base in _DEVICE_TABLES else C.POINTER(structs[base])
        if base in _POINTEES:
            return _p
    elif base in structs:
        return structs[base]
    elif base in _SCALARS:
        return _SCALARS[base]
    raise _refuse(decl)


def _struct(name, body, structs):
    fields = []
    for decl in body.split(";"):
        if not decl.strip():
            continue
        m = _FIELD.match(decl)
        # `float* a, b` declares b a float in C: too easy to misread, refused
        if not m or ("*" in m.group(2) and "," in m.group(3)):
            raise _refuse(decl)
        ct = _ctype(m.group(1), "*" in m.group(2), structs, decl)
        for d in m.group(3).split(","):
            fname, _, n = d.replace("]", "").partition("[")
            fields.append((fname.strip(), ct * int(n) if n else ct))
    return type(name, (C.Structure,), {"_fields_": fields})


def _proto(ret, args, structs, decl):
    if ret != "void" and ret not in _SCALARS:
        raise _refuse(decl)
    argtypes = []
    for a in ([] if args.strip() in ("", "void") else args.split(",")):
        m = _ARG.match(a)
        if not m:
            raise _refuse(decl)
        argtypes.append(_ctype(m.group(1), "*" in (m.group(2) or ""), structs, decl))
    return (None if ret == "void" else _SCALARS[ret]), argtypes


def parse_header(text):
    """C header text -> (structs, prototypes, constants), each a dict by name:
    ``typedef struct [Tag] { ... } Name;`` as a ctypes.Structure subclass,
    ``<ret> vu_name(<args>);`` as (restype, argtypes), ``#define VU_NAME
    <integer>`` as an int.  Anything else raises ValueError quoting the
    declaration: nothing is guessed and nothing is skipped."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts, lines = {}, []
    for line in text.split("\n"):
        if not line.lstrip().startswith("#"):
            lines.append(line)
            continue
        m = _DEFINE.match(line)
        if line.rstrip().endswith("\\") or not _DIRECTIVE.match(line):
            raise _refuse(line)
        if m:
            try:
                consts[m.group(1)] = int(m.group(2).strip(), 0)
            except ValueError:
                raise _refuse(line) from None
    text, wrapped = re.subn(r'extern\s+"C"\s*\{', "", "\n".join(lines), count=1)
    text = text.rstrip()
    if wrapped and text.endswith("}"):
        text = text[:-1]
    structs, sigs, pos = {}, {}, 0
    while True:
        m = _STRUCT.match(text, pos)
        if m:
            structs[m.group(2)] = _struct(m.group(2), m.group(1), structs)
        else:
            m = _PROTO.match(text, pos)
            if not m:
                break
            sigs[m.group(2)] = _proto(m.group(1), m.group(3), structs, m.group(0))
        pos = m.end()
    if text[pos:].strip():   # whatever neither form matches whole
        raise _refuse(text[pos:].split(";")[0][:200])
    return structs, sigs, consts


def _load_header():
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError(f"vaeunet_amd: C header {os.path.normpath(HEADER_PATH)} is missing; the binding is derived "
                           "from it and the package runs in-tree (no fallback)")
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


# the Vu* struct classes and the VU_* constants are module attributes;
# _SIGS: name -> (restype, argtypes)
_STRUCTS, _SIGS, _CONSTS = _load_header()
globals().update(_STRUCTS)
globals().update(_CONSTS)

_lib = None


def lib():
    """Load the library once; raise if it is absent (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"vaeunet_amd: HIP library {LIB_PATH} is missing; run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (or `make`)")
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(h, name)
            fn.restype = res
            fn.argtypes = args
        _lib = h
    return _lib


def exported_symbols():
    return sorted(_SIGS)


def call(name, *args):
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise RuntimeError(f"vaeunet_amd: {name} failed with hipError {rc}")
    return rc


def query(name, *args):
    return getattr(lib(), name)(*args)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())
