"""ctypes binding of libcxrmate_hip.so. Prototypes, descriptor struct layouts and shared limits are all parsed from
include/cxrmate_hip.h, so the header is the single source of truth for the C ABI. There is NO fallback: if the library is missing the
product path raises."""
from __future__ import annotations

import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "cxrmate_hip.h")
LIB_PATH = os.environ.get("CXR_LIB") or os.path.join(HERE, "lib", "libcxrmate_hip.so")      # CXR_LIB: a differently BUILT library (A/B of build-time switches)

_SCALARS = {"long": ctypes.c_long, "int": ctypes.c_int, "float": ctypes.c_float, "unsigned int": ctypes.c_uint}
_CTYPES = {**_SCALARS, "hipStream_t": ctypes.c_void_p}


def _header_text(text=None):
    if text is None:
        with open(HEADER) as f:
            text = f.read()
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def parse_header(path: str = HEADER):
    """-> {name: [(ctype, argname), ...]} for every `int cxr_*(...)` prototype."""
    text = _header_text(open(path).read())
    protos = {}
    for m in re.finditer(r"\bint\s+(cxr_\w+)\s*\(([^)]*)\)\s*;", text):
        args = []
        for a in m.group(2).split(","):
            a = " ".join(a.split())
            if not a or a == "void":
                continue
            if "*" in a:
                args.append((ctypes.c_void_p, a.split("*")[-1].strip()))
            else:
                ty, name = a.rsplit(" ", 1)
                args.append((_CTYPES[ty.replace("const ", "").strip()], name))
        protos[m.group(1)] = args
    return protos


def parse_structs(text: str | None = None):
    """-> {name: ctypes.Structure subclass} for every `typedef struct cxr_X { ... } cxr_X;` of the header (or of `text`), in header order.
    Fields: any pointer (c_void_p), `long` / `int` / `float` / `unsigned int`, or an earlier struct; comma lists and `[n]` suffixes. Anything
    else raises: a field skipped here would shift every field after it."""
    text = _header_text(text)
    structs = {}
    for m in re.finditer(r"\btypedef\s+struct\s+(cxr_\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", text):
        name, fields = m.group(1), []
        if m.group(3) != name:
            raise ValueError(f"typedef struct {name} is named {m.group(3)}")
        for decl in m.group(2).split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            ptr = re.fullmatch(r"(?:const )?(?:unsigned )?\w+ ?\* ?(\w+)", decl)
            if ptr:
                fields.append((ptr.group(1), ctypes.c_void_p))
                continue
            m2 = re.fullmatch(r"(?:const )?(unsigned int|\w+) (\w+(?:\[\d+\])?(?: ?, ?\w+(?:\[\d+\])?)*)", decl)
            base = m2 and (_SCALARS.get(m2.group(1)) or structs.get(m2.group(1)))
            if not base:
                raise ValueError(f"{name}: cannot parse the field declaration `{decl}`")
            for d in m2.group(2).split(","):
                fname, _, dim = d.strip().rstrip("]").partition("[")
                fields.append((fname, base * int(dim) if dim else base))
        structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields, "__module__": __name__,
                                                         "__doc__": f"`{name}` of include/cxrmate_hip.h (layout parsed from the header)"})
    if len(structs) != len(re.findall(r"\btypedef\s+struct\s+cxr_", text)):
        raise ValueError("a `typedef struct cxr_...` of the header was not parsed")
    return structs


def parse_limits(text: str | None = None):
    """-> {name: int} for every `#define CXR_X <integer>` line: the limits kernels and callers share."""
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(CXR_\w+)[ \t]+(-?\d+)[ \t]*$", _header_text(text), flags=re.M)}


STRUCTS = parse_structs()
LIMITS = parse_limits()


class CxrError(RuntimeError):
    pass


class _Lib:
    def __init__(self):
        self._dll = None
        self._fns = {}
        self.protos = parse_header()

    def load(self):
        if self._dll is None:
            if not os.path.exists(LIB_PATH):
                raise CxrError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(cxrmate_amd has no CPU / PyTorch fallback)")
            if os.environ.get("CXR_LIB"):
                import warnings
                warnings.warn(f"CXR_LIB is set: loading {LIB_PATH} instead of the in-tree libcxrmate_hip.so (A/B of build-time switches)", RuntimeWarning, stacklevel=2)
            import torch  # noqa: F401  -- torch's HIP runtime must be resident first so that the library binds to the same one
            self._dll = ctypes.CDLL(LIB_PATH)
            for name, args in self.protos.items():
                fn = getattr(self._dll, name)
                fn.restype = ctypes.c_int
                fn.argtypes = [t for t, _ in args]
        return self._dll

    def call(self, name: str, *args):
        fn = self._fns.get(name)
        if fn is None:
            fn = self._fns[name] = getattr(self.load(), name)
        rc = fn(*args)
        if rc != 0:
            detail = ""
            if rc == -2:
                f = self._dll.cxr_last_hip_error_string
                f.restype = ctypes.c_char_p
                detail = f" [hip error {self._dll.cxr_last_hip_error()}: {f().decode()}]"
            raise CxrError(f"{name} failed with code {rc}{detail} (args: {args})")


LIB = _Lib()
