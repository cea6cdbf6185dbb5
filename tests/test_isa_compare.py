"""tools/isa_compare.py's normaliser and per-symbol comparison on small hand-written assembly texts (CPU only, no compiler)."""
import importlib.util
import os

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_spec = importlib.util.spec_from_file_location("isa_compare", os.path.join(ROOT, "tools", "isa_compare.py"))
ic = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ic)


def _function(name, index, operand="v1", comment="a comment", vgprs=12):
    """One kernel as the compiler writes it: its label, two blocks, a branch, a get-pc label, its end label and its descriptor."""
    return f"""
\t.protected\t{name}
\t.globl\t{name}
\t.p2align\t8
\t.type\t{name},@function
{name}:                                 ; @{name}
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_add_u32_e32 v0, v0, {operand}      ; {comment}
\ts_cbranch_scc1 .LBB{index}_2
.LBB{index}_1:                          ; %loop
\tv_mul_f32_e32 v2, v0, v0
\ts_getpc_b64 s[2:3]
.Lpost_getpc{index + 7}:
\ts_add_u32 s2, s2, (.LBB{index}_1-.Lpost_getpc{index + 7})&4294967295
.LBB{index}_2:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {name}
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr {vgprs}
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{index}:
\t.size\t{name}, .Lfunc_end{index}-{name}
                                        ; -- End function
"""


def _file(*functions):
    return "\t.text\n\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"\n" + "".join(functions) + "\t.section\t\".note.GNU-stack\"\n"


BASE = _file(_function("kern_a", 0), _function("kern_b", 1))


def _rows(res):
    return {s: (same, desc) for s, _, _, same, desc in res["symbols"]}


def test_split_finds_bodies_and_descriptors():
    bodies, descs = ic.split_functions(BASE)
    assert set(bodies) == {"kern_a", "kern_b"} and set(descs) == {"kern_a", "kern_b"}
    assert ic.instruction_count(bodies["kern_a"]) == 7
    assert descs["kern_a"] == [".amdhsa_group_segment_fixed_size 0", ".amdhsa_next_free_vgpr 12"]
    assert not any(";" in l for l in bodies["kern_a"])


def test_swapped_order_and_renumbered_labels_are_identical():
    # the second file states the functions in the other order: every .LBB<n>_ / .Lpost_getpc<n> / .Lfunc_end<n> counter moves
    swapped = _file(_function("kern_b", 0), _function("kern_a", 1))
    res = ic.compare(BASE, swapped)
    assert _rows(res) == {"kern_a": (True, True), "kern_b": (True, True)}
    assert res["only_a"] == [] and res["only_b"] == []
    # renumbering alone, order kept
    assert _rows(ic.compare(BASE, _file(_function("kern_a", 5), _function("kern_b", 9)))) == {"kern_a": (True, True), "kern_b": (True, True)}


def test_block_numbers_inside_a_function_still_count():
    # only the file-wide counter is renamed: a branch to another block of the same function is a difference
    other = BASE.replace("s_cbranch_scc1 .LBB1_2", "s_cbranch_scc1 .LBB1_1")
    assert _rows(ic.compare(BASE, other)) == {"kern_a": (True, True), "kern_b": (False, True)}


def test_comment_only_change_is_identical():
    other = _file(_function("kern_a", 0, comment="another remark, v9"), _function("kern_b", 1))
    assert _rows(ic.compare(BASE, other)) == {"kern_a": (True, True), "kern_b": (True, True)}


def test_changed_operand_is_reported_for_its_symbol():
    other = _file(_function("kern_a", 0), _function("kern_b", 1, operand="v3"))
    res = ic.compare(BASE, other)
    assert _rows(res) == {"kern_a": (True, True), "kern_b": (False, True)}
    i, la, lb = ic.first_difference(BASE, other, "kern_b")
    assert (la, lb) == ("v_add_u32_e32 v0, v0, v1", "v_add_u32_e32 v0, v0, v3")
    lines, ok = ic.report("x.hip", res, (BASE, other))
    assert not ok and any("differs" in l and "kern_b" in l for l in lines) and not any("differs" in l and "kern_a" in l for l in lines)


def test_changed_descriptor_is_reported():
    other = _file(_function("kern_a", 0, vgprs=16), _function("kern_b", 1))
    res = ic.compare(BASE, other)
    assert _rows(res) == {"kern_a": (True, False), "kern_b": (True, True)}
    assert not ic.report("x.hip", res, (BASE, other))[1]


def test_symbol_on_one_side_only_is_listed():
    other = _file(_function("kern_a", 0), _function("kern_c", 1))
    res = ic.compare(BASE, other)
    assert res["only_a"] == ["kern_b"] and res["only_b"] == ["kern_c"]
    assert [r[0] for r in res["symbols"]] == ["kern_a"]
    lines, ok = ic.report("x.hip", res, (BASE, other))
    assert not ok and "only in parent: kern_b" in lines and "only in branch: kern_c" in lines


def test_identical_texts_report_ok():
    lines, ok = ic.report("x.hip", ic.compare(BASE, BASE), (BASE, BASE))
    assert ok and sum("identical" in l for l in lines) == 2
