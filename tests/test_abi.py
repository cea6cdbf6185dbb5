"""The C ABI is typed once, from the prototypes of include/thinktwice_hip.h (`_lib.prototypes`): `lib()` binds every entry's
argument and result types, the plan recorder classifies an argument by its declared type, and every call site in the tree
passes the declared number of arguments (CPU only: nothing here launches a kernel)."""
import ast
import ctypes
import os

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_bound_entries_read_long_long_results_and_refuse_wrong_arguments(tmp_path):
    from thinktwice_amd import _lib, control, plan
    L = _lib.lib()
    # pure host arithmetic (4.3e9 floats): read whole only through the header's `long long` result type
    assert L.tt_dec_gru_scratch_floats(100_000) == 100_000 * L.tt_dec_gru_scratch_floats(1)
    f = L.tt_dec_gru_scratch_floats                         # (not a `.tt_x(` call: the call-site scan below counts those)
    with pytest.raises(TypeError):
        f()                                                 # too few arguments: refused before any C runs
    with pytest.raises(ctypes.ArgumentError):
        f(1.0)                                              # a float for an `int`
    # a type the parser has no ctypes mapping for is an error naming the declaration, never a silent `int`
    hdr = tmp_path / "h.h"
    hdr.write_text("/* int tt_commented(int a); */\nint tt_ok(const char* s, unsigned long long n, void* stream);\n"
                   "size_t tt_unknown(int a);\n")
    with pytest.raises(_lib.TTError, match="tt_unknown"):
        _lib.prototypes(str(hdr))

    # the plan recorder's argument kinds come from the declared type, not from the Python type of the argument
    V, I, LL, U, F, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_uint, ctypes.c_float, ctypes.c_double
    k = plan.arg_kind
    assert k(I, 3) == (0, 3) and k(LL, 1 << 40) == (0, 1 << 40) and k(U, 0xFFFFFFFF) == (0, 0xFFFFFFFF) and k(I, True) == (0, 1)
    assert k(F, 2) == (1, 2.0) and type(k(F, 2)[1]) is float and k(D, 0.1) == (1, 0.1)
    assert k(F, 0.1) == (1, ctypes.c_float(0.1).value)          # what a C `float` receives, not the double 0.1
    assert k(I, -1) == (0, -1) and k(U, -1) == (0, 0xFFFFFFFF)
    assert k(V, None) == (4, None) and k(V, 0) == (4, None) and k(V, V(0)) == (4, None)
    assert k(V, 0x7F0000001000) == (2, 0x7F0000001000) and k(V, V(0x7F0000001000)) == (2, 0x7F0000001000)
    arr, cfg = (ctypes.c_int * 3)(1, 2, 3), control.ActionCfg()
    assert k(V, arr) == (3, arr) and k(V, cfg) == (3, cfg) and k(V, ctypes.byref(cfg)) == (3, cfg)
    for t, a in ((I, 2.0), (I, None), (I, ctypes.c_int(3)), (LL, V(8)), (F, None), (F, "1"), (V, 1.5), (V, b"x"),
                 (V, ctypes.pointer(ctypes.c_float())), (ctypes.c_char_p, b"x")):
        assert k(t, a) is None, (t, a)


def test_every_call_site_passes_the_declared_argument_count():
    """ctypes accepts SURPLUS arguments even with argtypes set: the count of every `.tt_x(` call in the tree is checked here
    against the header.  Argument and result types are set in one place only, the binding (thinktwice_amd/_lib.py)."""
    from thinktwice_amd import _lib
    protos = _lib.prototypes()
    files = [os.path.join(ROOT, "smoke_forward.py")]
    for d in ("thinktwice_amd", "tests", "tools"):
        for r, _, fs in os.walk(os.path.join(ROOT, d)):
            files += [os.path.join(r, f) for f in fs if f.endswith(".py")]
    bad, calls = [], 0
    for f in files:
        rel = os.path.relpath(f, ROOT)
        for node in ast.walk(ast.parse(open(f).read(), f)):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr.startswith("tt_"):
                calls += 1
                name = node.func.attr
                if name not in protos:
                    bad.append(f"{rel}:{node.lineno}: {name} is not declared in the header")
                elif (node.keywords or any(isinstance(a, ast.Starred) for a in node.args)
                      or len(node.args) != len(protos[name].params)):
                    bad.append(f"{rel}:{node.lineno}: {name} takes {len(protos[name].params)} positional arguments")
            elif isinstance(node, ast.Assign) and rel != os.path.join("thinktwice_amd", "_lib.py"):
                for t in node.targets:
                    if any(isinstance(a, ast.Attribute) and a.attr in ("restype", "argtypes") for a in ast.walk(t)):
                        bad.append(f"{rel}:{node.lineno}: restype / argtypes set outside the binding")
    assert calls > 200 and not bad, "\n".join(bad)
