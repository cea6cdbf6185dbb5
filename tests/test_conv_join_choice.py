"""tt_conv2d_plan_next (host only, no device) answers for a 1 x 1 bf16x3 layer with a joined stage (tt_conv2d_fwd_next, tt_conv_next;
csrc/conv_choose.cpp choose_join): the label of every form at and just below kJoinMinRows and at the contract's floor, the refusals, and
ops.join_ok, which routes by that label."""
import ctypes

from thinktwice_amd import _lib, ops

FORMS = [(64, 256, 64), (64, 256, 128), (128, 512, 128), (128, 512, 256), (256, 1024, 256)]
P = ops.canonical_desc("join", 4551, 64, 256, 64)[0].weight       # the stand-in for every pointer of a canonical descriptor


def _desc(rows, k1, cout, n2, in_pair=1, **change):
    """ops.canonical_desc's (tt_conv_desc, tt_conv_next) of the joined form; a change goes to whichever of the two has the field"""
    d, n = ops.canonical_desc("join", rows, k1, cout, n2)
    for f, v in dict(change, in_pair=in_pair).items():
        setattr(n if f.startswith("next_") else d, f, v)
    return d, n


def _plan(dn):
    """the label of tt_conv2d_plan_next, or "ERROR: " + tt_last_error"""
    return ops.plan_label(*dn)


def _label(k1, n2, pair=True):
    return f"conv_x3_join_kernel<{k1}, {n2}, {4 if n2 == 256 else 8}>" + (" pre-split A" if pair else "")


def test_label_of_every_form_at_and_just_below_the_threshold_and_the_floor():
    """From kJoinMinRows on the plain label; below it the same kernel, marked; at 4,096 rows (the pair format's floor) a refusal."""
    m = _lib.TT_CONV_JOIN_MIN_ROWS
    assert m == 32768
    for k1, cout, n2 in FORMS:
        for rows in (m, m + 1, 50176, 100352, 200704, 401408, 1605632):
            assert _plan(_desc(rows, k1, cout, n2)) == _label(k1, n2), (rows, k1, n2)
            assert _plan(_desc(rows, k1, cout, n2, in_pair=0)) == _label(k1, n2, pair=False), (rows, k1, n2)
        for rows in (m - 1, 12288, 4551, 4097):
            assert _plan(_desc(rows, k1, cout, n2)) == _label(k1, n2) + " below kJoinMinRows", (rows, k1, n2)
        floor = _plan(_desc(4096, k1, cout, n2))
        assert floor.startswith("ERROR") and "N*OH*OW" in floor and "4097" in floor, floor


def test_the_descriptor_alone_keeps_its_kernel_and_a_null_next_is_refused():
    L = _lib.lib()
    d, _ = _desc(1605632, 64, 256, 64)
    label = ctypes.create_string_buffer(192)
    assert L.tt_conv2d_plan(ctypes.byref(d), label, len(label)) == 0
    assert label.value.decode().startswith("conv_igemm_glds_kernel<float, 256, 4, 2, 128, 23, false, true> pre-split A")
    assert L.tt_conv2d_plan_next(ctypes.byref(d), None, label, len(label)) != 0 and "tt_conv_next" in L.tt_last_error().decode()


def test_refusals_without_a_device():
    ok = dict(rows=4551, k1=64, cout=256, n2=64)
    for change, word in ((dict(next_out=0), "next_out"), (dict(next_weight=0), "next_weight"), (dict(next_weight_x3=0), "next_weight_x3"),
                         (dict(next_weight_x3=P + 4), "next_weight_x3"), (dict(next_out_pair=0), "next_out_pair"),
                         (dict(next_out=P + 16), "next_out"), (dict(next_cout=256, next_out_cstride=256), "next_cout"),
                         (dict(next_cout=48, next_out_cstride=48), "next_cout"), (dict(next_out_cstride=72), "next_out_cstride"),
                         (dict(next_out_coff=16), "next_out_coff"), (dict(next_act=2), "next_act"), (dict(act=4), "act"),
                         (dict(weight_x3=0), "weight_x3"), (dict(dtype=1, out_dtype=1, in_pair=0), "dtype"), (dict(out_pair=1), "out_pair"),
                         (dict(in_up2=1), "in_up2"), (dict(KH=3, KW=3, pad=1), "1 x 1"), (dict(stride=2), "stride"),
                         (dict(res2=P, res2_cstride=256), "res2"), (dict(shift_n=P), "shift_n"), (dict(out2=P, out2_cstride=256), "out2"),
                         (dict(res1_up_h=1, res1_up_w=8), "res1_up"), (dict(splitk_ws=P, in_pair=0), "splitk_ws"), (dict(pixel_shuffle2=1), "pixel_shuffle2"),
                         (dict(in_cstride=72), "in_cstride"), (dict(in_nstride=1 << 20), "in_nstride"), (dict(out_nstride=1 << 21), "out"),
                         (dict(res1_coff=2), "res1"), (dict(Cout=128, out_cstride=128, res1_cstride=128), "Cout")):
        msg = _plan(_desc(ok["rows"], ok["k1"], ok["cout"], ok["n2"], **change))
        assert msg.startswith("ERROR") and word in msg, (change, msg)
    # channel counts outside the forms
    assert "Cin" in _plan(_desc(4551, 32, 128, 64))
    assert "next_cout" in _plan(_desc(4551, 256, 1024, 512))      # layer 3 -> 4: no 512-wide form


def test_join_ok_over_the_grid():
    """join_ok from plain numbers: yes for the forms the model routes (ops.JOIN_ROUTED) from 32,768 rows on, and every yes is a
    descriptor the library takes with an unmarked label."""
    from thinktwice_amd import autodiff
    assert ops.BNECK_JOIN and autodiff.TAPE is None
    yes = 0
    for rows in (2048, 4096, 4097, 4551, 16384, 32767, 32768, 50176, 100352, 1605632):
        for k1 in (32, 64, 128, 256, 512):
            for cout in (2 * k1, 4 * k1):
                for n2 in (32, 64, 128, 256, 512):
                    label = _plan(_desc(rows, k1, cout, n2))
                    taken = label.startswith("conv_x3_join_kernel<")
                    assert taken or label.startswith("ERROR: tt_conv2d_fwd: next_"), label
                    ok = ops.join_ok(rows, k1, cout, n2)
                    yes += ok
                    assert ok == (rows >= 32768 and (k1, cout, n2) in ops.JOIN_ROUTED), (rows, k1, cout, n2)
                    assert ok == (taken and not label.endswith(" below kJoinMinRows") and (k1, cout, n2) in ops.JOIN_ROUTED), \
                        (rows, k1, cout, n2, label)
                    assert (k1, cout, n2) in FORMS or not taken
    assert yes == 4 * len(ops.JOIN_ROUTED)
    assert set(ops.JOIN_ROUTED) <= set(FORMS)


def test_the_knob_and_the_tape_turn_join_ok_off(monkeypatch):
    from thinktwice_amd import autodiff
    assert ops.join_ok(1605632, 64, 256, 64)
    monkeypatch.setattr(ops, "BNECK_JOIN", False)
    assert not ops.join_ok(1605632, 64, 256, 64)
    monkeypatch.setattr(ops, "BNECK_JOIN", True)
    monkeypatch.setattr(autodiff, "TAPE", object())
    assert not ops.join_ok(1605632, 64, 256, 64)
