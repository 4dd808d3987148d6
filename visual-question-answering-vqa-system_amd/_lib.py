"""ctypes binding of libvqa_hip.so (the C ABI declared in include/vqa_hip.h).

The header is the one declaration of every entry: it is parsed once at import into SIGNATURES (argument ctypes), ARGNAMES (parameter
names) and the sets of entries that return a size or a count, and csrc/common.h includes it, so a definition that disagrees with it
does not compile.  There is no hand-written table to keep in step.

There is no fallback: if the header or the shared library is missing, a declaration cannot be bound or a call fails, a RuntimeError
is raised.  Every entry takes raw device pointers, explicit sizes and a hipStream_t; PyTorch owns all memory.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvqa_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "vqa_hip.h")

P, I, F, D, LL, ULL = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_longlong, C.c_ulonglong
_CTYPES = {"int": I, "float": F, "double": D, "long long": LL, "unsigned long long": ULL, "hipStream_t": P}


def parse_header(text: str):
    """The entries a header text declares: {name: (restype, parameter names, parameter ctypes, takes a stream)} for every
    `int | long long vqa_*(...);`.  A pointer of any kind is c_void_p; every other type must be one of the spellings of _CTYPES and
    every parameter must be named, else RuntimeError (naming the entry): nothing is guessed."""
    out = {}
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for ret, name, params in re.findall(r"\b(int|long long)\s+(vqa_\w+)\s*\(([^()]*)\)\s*;", text):
        names, ctypes, spelling = [], [], ""
        for prm in params.split(","):
            m = re.fullmatch(r"\s*(.*?[\s*])([A-Za-z_]\w*)\s*", prm, flags=re.S)
            spelling = " ".join(m.group(1).split()) if m else ""
            ctype = P if "*" in spelling else _CTYPES.get(spelling)
            if ctype is None:
                raise RuntimeError(f"{name}: cannot bind parameter '{' '.join(prm.split())}' (expected a named int, float, double, "
                                   "long long, unsigned long long, hipStream_t or pointer)")
            names.append(m.group(2))
            ctypes.append(ctype)
        out[name] = (_CTYPES[ret], tuple(names), ctypes, spelling == "hipStream_t")
    return out


def _declarations():
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError(f"{HEADER_PATH} is missing: the ctypes table is derived from it; there is no second copy")
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


_DECL = _declarations()
SIGNATURES = {name: d[2] for name, d in _DECL.items()}                  # name -> argument ctypes (the stream last, where there is one)
ARGNAMES = {name: d[1][:-1] if d[3] else d[1] for name, d in _DECL.items()}                  # name -> parameter names, without the stream
_RET_LL = {name for name, d in _DECL.items() if d[0] is LL}                                             # return a size (long long)
# no stream: host-only queries that return a count, not a status -- except vqa_wgrad_plan, which returns a status and is called directly
_NO_STATUS = {name for name, d in _DECL.items() if not d[3]} - {"vqa_wgrad_plan"}

_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                               "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for name, args in SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = LL if name in _RET_LL else I
        _lib = L
    return _lib


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


# Optional launch hook (kernels.py installs the live profiler of bench.py here): hook(name, args) -> closer | None
_HOOK = [None]


def call(name: str, *args):
    """Invoke a status-returning entry on the current torch stream; raise on non-zero status."""
    fn = getattr(lib(), name)
    hook = _HOOK[0]
    done = hook(name, args) if hook is not None else None
    rc = fn(*args, stream())
    if done is not None:
        done()
    if rc != 0:
        raise RuntimeError(f"{name} failed with status {rc}" + (" (argument/shape error)" if rc == 1000 else " (hipError_t)"))


def count(name: str, *args) -> int:
    assert name in _NO_STATUS
    return getattr(lib(), name)(*args)


def dt(t_or_dtype) -> int:
    d = t_or_dtype.dtype if isinstance(t_or_dtype, torch.Tensor) else t_or_dtype
    if d == torch.float32:
        return 0
    if d == torch.bfloat16:
        return 1
    raise TypeError(f"unsupported dtype {d}")
