"""tt_conv2d_plan_next (host only, no device) answers for a 1 x 1 bf16x3 layer with a joined stage (tt_conv2d_fwd_next, tt_conv_next;
csrc/conv_choose.cpp choose_join): the label of every form at and just below kJoinMinRows and at the contract's floor, the refusals, and
ops.join_ok against the library's answer."""
import ctypes

P = 0x10000       # a stand-in for every pointer: tt_conv2d_plan looks at null-ness and alignment only

FORMS = [(64, 256, 64), (64, 256, 128), (128, 512, 128), (128, 512, 256), (256, 1024, 256)]


def _desc(rows, k1, cout, n2, in_pair=1, **change):
    """(tt_conv_desc, tt_conv_next); a change goes to whichever of the two has the field"""
    from thinktwice_amd import _lib, ops
    d, n = ops._ConvDesc(), ops._ConvNext()
    d.in_ = P; d.N = 1; d.H = 1; d.W = rows; d.Cin = k1; d.in_cstride = k1
    d.weight = P; d.Cout = cout; d.KH = d.KW = d.stride = d.dil = 1
    d.out = P; d.OH = 1; d.OW = rows; d.out_cstride = cout
    d.scale = d.shift = P
    d.res1 = P; d.res1_cstride = cout
    d.act = 1; d.dtype = d.out_dtype = _lib.TT_F32
    d.weight_x3 = P; d.in_pair = in_pair
    n.next_weight = n.next_weight_x3 = P; n.next_cout = n2
    n.next_scale = n.next_shift = P; n.next_act = 1
    n.next_out = P; n.next_out_cstride = n2; n.next_out_pair = 1
    for f, v in change.items():
        setattr(n if f.startswith("next_") else d, f, v)
    return d, n


def _plan(dn):
    """the label of tt_conv2d_plan_next, or "ERROR: " + tt_last_error"""
    from thinktwice_amd import _lib
    L = _lib.lib()
    label = ctypes.create_string_buffer(192)
    if L.tt_conv2d_plan_next(ctypes.byref(dn[0]), ctypes.byref(dn[1]), label, len(label)) != 0:
        return "ERROR: " + L.tt_last_error().decode()
    return label.value.decode()


def _label(k1, n2, pair=True):
    return f"conv_x3_join_kernel<{k1}, {n2}, {4 if n2 == 256 else 8}>" + (" pre-split A" if pair else "")


def test_label_of_every_form_at_and_just_below_the_threshold_and_the_floor():
    """From kJoinMinRows on the plain label; below it the same kernel, marked; at 4,096 rows (the pair format's floor) a refusal."""
    from thinktwice_amd import ops
    m = ops.JOIN_MIN_ROWS
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
    from thinktwice_amd import _lib
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


def test_join_ok_agrees_with_the_library():
    """join_ok = the library takes the descriptor, at or above kJoinMinRows (an unmarked label), AND the form is one the model
    routes (ops.JOIN_ROUTED)."""
    from thinktwice_amd import autodiff, ops
    assert ops.BNECK_JOIN and autodiff.TAPE is None
    yes = 0
    for rows in (2048, 4096, 4097, 4551, 16384, ops.JOIN_MIN_ROWS - 1, ops.JOIN_MIN_ROWS, 50176, 100352, 1605632):
        for k1 in (32, 64, 128, 256, 512):
            for cout in (2 * k1, 4 * k1):
                for n2 in (32, 64, 128, 256, 512):
                    label = _plan(_desc(rows, k1, cout, n2))
                    taken = label.startswith("conv_x3_join_kernel<")
                    assert taken or label.startswith("ERROR: tt_conv2d_fwd: next_"), label
                    ok = ops.join_ok(rows, k1, cout, n2)
                    yes += ok
                    assert ok == (taken and not label.endswith(" below kJoinMinRows") and (k1, cout, n2) in ops.JOIN_ROUTED), \
                        (rows, k1, cout, n2, label)
                    assert (k1, cout, n2) in FORMS or not taken
    assert yes == 4 * len(ops.JOIN_ROUTED)
    assert set(ops.JOIN_ROUTED) <= set(FORMS)


def test_the_knob_and_the_tape_turn_join_ok_off(monkeypatch):
    from thinktwice_amd import autodiff, ops
    assert ops.join_ok(1605632, 64, 256, 64)
    monkeypatch.setattr(ops, "BNECK_JOIN", False)
    assert not ops.join_ok(1605632, 64, 256, 64)
    monkeypatch.setattr(ops, "BNECK_JOIN", True)
    monkeypatch.setattr(autodiff, "TAPE", object())
    assert not ops.join_ok(1605632, 64, 256, 64)
