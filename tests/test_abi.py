"""The C ABI is typed once, from the prototypes of include/thinktwice_hip.h (`_lib.prototypes`): `lib()` binds every entry's
argument and result types, the plan recorder classifies an argument by its declared type, and every call site in the tree
passes the declared number of arguments.  Its structs and constants are generated from the same header (`_lib.structs`,
`_lib.constants`) and checked against what a C compiler makes of it (CPU only: nothing here launches a kernel)."""
import ast
import ctypes
import keyword
import os
import re
import subprocess

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
            elif isinstance(node, ast.ClassDef) and rel != os.path.join("thinktwice_amd", "_lib.py"):
                if any(ast.unparse(b).split(".")[-1] == "Structure" for b in node.bases):
                    bad.append(f"{rel}:{node.lineno}: ctypes.Structure {node.name} written out outside the binding")
    assert calls > 200 and not bad, "\n".join(bad)


def test_ctypes_mirrors_match_the_c_header_layout(tmp_path):
    """The Python host talks to the C ABI through ctypes structs and integer constants that `_lib.structs()` /
    `_lib.constants()` generate from include/thinktwice_hip.h.  The independent side: gcc compiles the header and prints sizeof
    of every struct, offsetof of every member and the value of every constant.  A member the parser mislaid or mistyped would
    otherwise shift every later pointer silently; a struct added to the header is covered without touching this test."""
    from thinktwice_amd import _lib, control, labels, ops, photometric, preprocess
    S, C = _lib.structs(), _lib.constants()
    assert len(S) >= 10 and len(C) >= 40
    header = open(_lib.HEADER).read()
    assert set(re.findall(r"typedef\s+struct\s+(\w+)\s*\{", header)) == set(S)      # none skipped quietly
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "thinktwice_hip.h"', "int main(void) {"]
    for cname, cls in S.items():
        lines.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            cfield = fname[:-1] if keyword.iskeyword(fname[:-1]) else fname       # `in` is spelled `in_`
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, cfield))
    lines += ['  printf("const %s %%lld\\n", (long long)%s);' % (n, n) for n in C]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.dirname(_lib.HEADER), str(src), "-o", str(exe)])
    got = {}
    for ln in subprocess.check_output([str(exe)], text=True).splitlines():
        c, f, v = ln.split()
        got[(c, f)] = int(v)
    for cname, cls in S.items():
        assert got[(cname, "sizeof")] == ctypes.sizeof(cls), (cname, got[(cname, "sizeof")], ctypes.sizeof(cls))
        for fname, _ in cls._fields_:
            assert got[(cname, fname)] == getattr(cls, fname).offset, (cname, fname)
    for n, v in C.items():
        assert got[("const", n)] == v, n
    # the names the package, the tools and the tests use are these objects
    assert (ops._ConvDesc, ops._ChainStage) == (S["tt_conv_desc"], S["tt_chain_stage"])
    assert (control.ActionCfg, control.ActionState) == (S["tt_action_cfg"], S["tt_action_state"])
    assert (preprocess.IdaSet, photometric.AugOp, photometric.AugProgram) == (S["tt_ida_set"], S["tt_aug_op"], S["tt_aug_program"])
    assert (labels.HsvTables, labels.SegDecodeConf) == (S["tt_hsv_tables"], S["tt_seg_decode_conf"])
    assert ops._ConvDesc._fields_[0] == ("in_", ctypes.c_void_p) and len(ops._ConvDesc._fields_) == 52
    assert all(t is ctypes.c_void_p or t in _lib._SCALARS.values() for _, t in ops._ConvDesc._fields_ + ops._ChainStage._fields_)
    assert (control.PID_WINDOW_MAX, control.ACT_STEER, control.ACT_STUCK_DETECTOR, control.ACTION_OUT) == (64, 0, 19, 24)
    assert [getattr(photometric, k) for k in photometric.KIND_NAMES] == [C["TT_AUG_" + k] for k in photometric.KIND_NAMES]
    assert (_lib.TT_F32, _lib.TT_BF16, _lib.TT_F16, _lib.ACT_NONE, _lib.ACT_SOFTPLUS_CLAMP) == (0, 1, 2, 0, 5)


@pytest.mark.parametrize("member, named", [("unsigned flags : 3", "flags"), ("size_t n", "n"), ("int (*fn)(int)", "fn"),
                                           ("union { int a; float b; } u", "u"), ("float v[n_rows]", "v")])
def test_a_struct_member_the_parser_cannot_map_is_an_error_naming_it(tmp_path, member, named):
    """A bit-field, an unknown type, a function pointer, a union, a non-constant dimension: TTError naming the struct and the
    member, never a silent `int`."""
    from thinktwice_amd import _lib
    hdr = tmp_path / "h.h"
    hdr.write_text("#define TT_N 4\ntypedef struct tt_ok { const float* p, *q; int a[2 * TT_N], in; } tt_ok;\n"
                   "typedef struct tt_s { tt_ok first; /* int commented; */ %s; int last; } tt_s;\n" % member)
    with pytest.raises(_lib.TTError, match=r"(?s)tt_s.*\b%s\b" % named):
        _lib.structs(str(hdr))
    good = tmp_path / "ok.h"
    good.write_text(hdr.read_text().split("typedef struct tt_s")[0])
    ok = _lib.structs(str(good))["tt_ok"]
    assert ok._fields_[:2] == [("p", ctypes.c_void_p), ("q", ctypes.c_void_p)]
    assert ok._fields_[2][1]._length_ == 8 and ok._fields_[3][0] == "in_" and ctypes.sizeof(ok) == 56
