"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/vqa_hip.h declares; the header is the one
declaration: _lib.py derives its ctypes table from it, the sources compile against it, the byte formulas read its parameter names
(no compute calls without a GPU)."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

from _pkg import REPO, sub


def _header_symbols():
    txt = open(os.path.join(REPO, "include", "vqa_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|long long)\s+(vqa_\w+)\s*\(", txt)))


def test_header_declares_the_bound_symbols():
    L = sub("_lib")
    assert _header_symbols() == sorted(L.SIGNATURES)


def test_library_builds_loads_and_exports_every_symbol():
    import __graft_entry__ as G
    G.build()
    L = sub("_lib")
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in _header_symbols():
        assert hasattr(lib, name), name


def test_header_arity_matches_ctypes_table():
    L = sub("_lib")
    txt = open(os.path.join(REPO, "include", "vqa_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for m in re.finditer(r"\b(?:int|long long)\s+(vqa_\w+)\s*\((.*?)\)\s*;", txt, flags=re.S):
        name, args = m.group(1), m.group(2)
        n = len([a for a in args.split(",") if a.strip()])
        assert n == len(L.SIGNATURES[name]), (name, n, len(L.SIGNATURES[name]))


def test_missing_library_fails_loudly(monkeypatch):
    L = sub("_lib")
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(L, "LIB_PATH", "/nonexistent/libvqa_hip.so")
    with pytest.raises(RuntimeError):
        L.lib()


# ------------------------------------------------------------------------------------------ the header is the one declaration: the parser
def test_parser_maps_every_type_spelling():
    L = sub("_lib")
    d = L.parse_header("int vqa_t(int a, float b, double c, long long d, unsigned long long e, const void* f, float* g, const uint8_t* h,\n"
                       "          const float* const* i, unsigned char* j, hipStream_t stream);")
    assert d == {"vqa_t": (L.I, tuple("abcdefghij") + ("stream",), [L.I, L.F, L.D, L.LL, L.ULL, L.P, L.P, L.P, L.P, L.P, L.P], True)}


def test_parser_skips_comments_and_joins_lines():
    L = sub("_lib")
    d = L.parse_header("/* int vqa_ghost(int a); */\n"
                       "int vqa_t(int a /* rows, of\n   any size */, float* ws /* >= 64*2*C, or NULL */,\n"
                       "          long long\n n,\n          hipStream_t   stream);\n"
                       "typedef struct s { long long calls; int n; } s;\n")
    assert d == {"vqa_t": (L.I, ("a", "ws", "n", "stream"), [L.I, L.P, L.LL, L.P], True)}


def test_parser_struct_pointer_no_stream_and_long_long_return():
    L = sub("_lib")
    d = L.parse_header("int vqa_set(vqa_step_state* state, const vqa_group_hyper* groups, hipStream_t stream);\n"
                       "long long vqa_ws(int dtype, const int* M);\nint vqa_blocks(long long rows);")
    assert d["vqa_set"] == (L.I, ("state", "groups", "stream"), [L.P, L.P, L.P], True)
    assert d["vqa_ws"] == (L.LL, ("dtype", "M"), [L.I, L.P], False)
    assert d["vqa_blocks"] == (L.I, ("rows",), [L.LL], False)


@pytest.mark.parametrize("params", ["size_t n", "unsigned n", "const int n", "long n", "int", "const float*", "unsigned long long", ""])
def test_parser_refuses_what_it_cannot_bind(params):
    """an unknown spelling or an unnamed parameter is an error that names the entry: the mapping never guesses"""
    L = sub("_lib")
    with pytest.raises(RuntimeError, match="vqa_odd"):
        L.parse_header(f"int vqa_fine(int a, hipStream_t stream);\nint vqa_odd(int a, {params}, hipStream_t stream);")


def test_missing_header_fails_loudly(monkeypatch):
    L = sub("_lib")
    monkeypatch.setattr(L, "HEADER_PATH", "/nonexistent/vqa_hip.h")
    with pytest.raises(RuntimeError, match="vqa_hip.h"):
        L._declarations()


def test_table_is_the_parse_of_the_header():
    L = sub("_lib")
    d = L.parse_header(open(os.path.join(REPO, "include", "vqa_hip.h")).read())
    assert L.SIGNATURES == {n: e[2] for n, e in d.items()}
    for n, (ret, names, types, has_stream) in d.items():
        assert L.ARGNAMES[n] == (names[:-1] if has_stream else names) and len(set(names)) == len(names), n
        assert (n in L._RET_LL) == (ret is L.LL), n
        assert (n in L._NO_STATUS) == (not has_stream and n != "vqa_wgrad_plan"), n
    assert L._RET_LL <= L._NO_STATUS and len(L._RET_LL) == 6


# ---------------------------------------------------------------------------- ... and the compiler holds every definition against it
def _syntax_only(tmp_path, definition):
    B = sub("build")
    src = tmp_path / "entry.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include "%s"\n%s\n' % (os.path.join(REPO, "include", "vqa_hip.h"), definition))
    return subprocess.run([B.HIPCC, "--offload-arch=gfx950", "-std=c++17", "--cuda-host-only", "-fsyntax-only", str(src)],
                          capture_output=True, text=True)


def test_definition_that_matches_the_header_compiles(tmp_path):
    r = _syntax_only(tmp_path, 'extern "C" int vqa_add(int dtype, const void* a, const void* b, void* out, long long n, hipStream_t st) { return 0; }')
    assert r.returncode == 0, r.stderr


def test_definition_that_disagrees_with_the_header_does_not_compile(tmp_path):
    r = _syntax_only(tmp_path, 'extern "C" int vqa_add(int dtype, const void* a, const void* b, void* out, int n, hipStream_t st) { return 0; }')
    assert r.returncode != 0 and "conflicting types for 'vqa_add'" in r.stderr, r.stderr


def test_sources_declare_nothing_a_second_time():
    csrc = os.path.join(REPO, "visual-question-answering-vqa-system_amd", "csrc")
    assert re.search(r'^#include "\.\./\.\./include/vqa_hip\.h"', open(os.path.join(csrc, "common.h")).read(), flags=re.M)
    files = sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".h")))
    assert len(files) >= 20
    for f in files:
        txt = open(os.path.join(csrc, f)).read()
        assert not re.search(r"typedef\s+struct\b[^;{]*\b(vqa_step_state|vqa_group_hyper)\b", txt), f
        assert not re.search(r"#\s*define\s+VQA_GROUPS_MAX\b", txt), f
        assert not re.search(r'extern\s+"C"\s+(int|long long)\s+vqa_\w+\s*\([^;{]*\)\s*;', txt), f


def test_stale_check_counts_the_header(tmp_path, monkeypatch):
    B = sub("build")
    assert B.HEADER == os.path.join(REPO, "include", "vqa_hip.h") and B.HEADER in B._deps()
    lib, header = tmp_path / "lib.so", tmp_path / "vqa_hip.h"
    lib.write_bytes(b"")
    header.write_text("")
    newest = max(os.path.getmtime(d) for d in B._deps())
    os.utime(lib, (newest + 10, newest + 10))
    os.utime(header, (newest + 20, newest + 20))
    monkeypatch.setattr(B, "LIB", str(lib))
    assert not B._stale()
    monkeypatch.setattr(B, "HEADER", str(header))
    assert B._stale()


# ------------------------------------------------------------------------- the byte formulas of kernels.HBM_BYTES, pinned to their parent
HBM_GOLDEN = os.path.join(REPO, "tests", "golden", "hbm_bytes.json")
PRIMES = [2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 101, 103, 107, 109, 113]


def _synthetic_args(names, ctypes_, second):
    """The i-th integer argument is the i-th prime, floats are 0.5; dtype arguments 0 and pointers non-null (first tuple) or 1 and None."""
    primes = iter(PRIMES)
    return [(None if second else 4096) if t is ctypes.c_void_p else 0.5 if t in (ctypes.c_float, ctypes.c_double)
            else int(second) if n.startswith("dtype") else next(primes) for n, t in zip(names, ctypes_)]


def test_hbm_byte_formulas_equal_the_positional_ones_they_replace():
    """golden/hbm_bytes.json: per entry two synthetic argument lists and the bytes the positional formulas (a[6] * a[7] * ...) gave for them
    before the formulas read their arguments by name.  Distinct primes: two names swapped, or one shifted, change the product."""
    K, L = sub("kernels"), sub("_lib")
    golden = json.load(open(HBM_GOLDEN))
    assert sorted(golden) == sorted(K.HBM_BYTES) and len(golden) >= 50
    for name, cases in golden.items():
        assert [c["args"] for c in cases] == [_synthetic_args(L.ARGNAMES[name], L.SIGNATURES[name], s) for s in (False, True)], name
        for c in cases:
            got = K.HBM_BYTES[name][1](c["args"])
            assert got == c["bytes"] and type(got) is int, (name, c["args"], got, c["bytes"])


if __name__ == "__main__":
    # python tests/test_cabi_cpu.py CHECKOUT: writes golden/hbm_bytes.json from the HBM_BYTES of the checkout at CHECKOUT (the parent commit
    # of a change to the formulas); parameter names come from this module's own reading of that checkout's header
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    K, L = sub("kernels"), sub("_lib")
    assert os.path.dirname(os.path.dirname(K.__file__)) == os.path.abspath(sys.argv[1])
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(sys.argv[1], "include", "vqa_hip.h")).read(), flags=re.S)
    names = {m.group(1): [re.search(r"(\w+)\s*$", a).group(1) for a in m.group(2).split(",")]
             for m in re.finditer(r"\b(?:int|long long)\s+(vqa_\w+)\s*\((.*?)\)\s*;", txt, flags=re.S)}
    out = {}
    for name, (_, fn) in K.HBM_BYTES.items():
        cases = [_synthetic_args(names[name][:-1], L.SIGNATURES[name][:-1], s) for s in (False, True)]
        out[name] = [{"args": a, "bytes": fn(a)} for a in cases]
    with open(HBM_GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(n)}: {json.dumps(c)}" for n, c in out.items()) + "\n}\n")
    print(f"{HBM_GOLDEN}: {len(out)} entries from {sys.argv[1]}")
