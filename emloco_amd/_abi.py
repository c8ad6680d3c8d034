"""The C ABI of libemloco_hip.so as include/*.h declare it: every prototype `RET emloco_name(ARGS);` gives that function its ctypes
restype / argtypes, so a new entry point needs its declaration in a header and nothing here.  Scalars map to the ctypes type of the same
width and signedness, every pointer or array parameter to `c_void_p` (it takes byref(...), a ctypes array or pointer, an address, None),
a `const char *` return to `c_char_p`; anything else is an error, never a guess.  The structures the prototypes point to are mirrored
by hand in `_lib.py`; tests/test_abi_cpu.py holds them to the headers."""
import ctypes as C
import functools
import os
import re

HEADERS = ("emloco_sim.h", "emloco_task.h", "emloco_predictor.h")
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "unsigned": C.c_uint, "int64_t": C.c_int64,
           "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
_PROTO = re.compile(r"\s*([\w\s*]+?)\b(emloco_\w+)\s*\(([^()]*)\)\s*")


class EmlocoError(RuntimeError):
    pass


def source(header):
    """The header's text without comments and preprocessor lines."""
    with open(os.path.join(INCLUDE, header)) as f:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
    return re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)


def _ctype(decl, named, where):
    """ctypes type of a parameter declaration (`named`: its last word is the name) or of a return type."""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    scalar = " ".join(words[:-1] if named else words)          # (a parameter without a name has no type left and fails below)
    if "*" in decl or "[" in decl:
        if named:
            return C.c_void_p
        if words == ["char", "*"]:
            return C.c_char_p
    elif scalar in SCALARS:
        return SCALARS[scalar]
    raise EmlocoError(f"{where}: no ctypes mapping for `{decl.strip()}`")


@functools.lru_cache(maxsize=None)
def parse(header):
    """{name: (restype, [argtypes])} of every prototype the header declares."""
    out = {}
    for stmt in source(header).split(";"):
        if "(" in stmt:                  # (with comments and macros gone only prototypes have parentheses: anything else fails here)
            m = _PROTO.fullmatch(stmt)
            if m is None:
                raise EmlocoError(f"{header}: cannot parse `{' '.join(stmt.split())}`")
            ret, name, args = m.groups()
            args = [] if args.strip() in ("", "void") else args.split(",")
            out[name] = (_ctype(ret, False, f"{header}: {name}"), [_ctype(a, True, f"{header}: {name}") for a in args])
    return out


def prototypes():
    return {name: sig for h in HEADERS for name, sig in parse(h).items()}


def bind(lib):
    """Set restype / argtypes of every declared function on the loaded library; a declared function it lacks is an error."""
    for name, (restype, argtypes) in prototypes().items():
        if not hasattr(lib, name):
            raise EmlocoError(f"libemloco_hip.so does not export {name}, which include/ declares")
        getattr(lib, name).restype, getattr(lib, name).argtypes = restype, argtypes
    return lib
