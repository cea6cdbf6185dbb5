"""ops.conv_desc / ops.conv_geometry: the one place that turns a convolution's plain numbers into a tt_conv_desc.

CPU only: nothing here loads the library or touches a device.  Every expected value is worked out by hand from the rule as
ops.conv2d / ops.gather_conv wrote it inline before the builder existed; that line is quoted beside the expectation.
"""
import pytest

from thinktwice_amd import _lib, autodiff, ops

F32, BF16, F16 = _lib.TT_F32, _lib.TT_BF16, _lib.TT_F16
X, W, OUT = 0x1000, 0x2000, 0x3000       # made-up element addresses


def strides(shape):
    st = [1]
    for n in reversed(shape[1:]):
        st.insert(0, st[0] * n)
    return tuple(st)


def dense(x_shape, w_shape, out_shape=None, dtype=F32, **kw):
    """The descriptor of a layer over contiguous tensors; out_shape None: the tensor conv2d would allocate."""
    geometry = {k: kw[k] for k in ("stride", "pad", "dil", "out_hw", "pixel_shuffle2", "in_up2") if k in kw}
    if out_shape is None:
        out_shape = ops.conv_geometry(x_shape, w_shape, **geometry)[4]
    return ops.conv_desc(x=X, x_shape=x_shape, x_strides=strides(x_shape), w=W, w_shape=w_shape, out=OUT, out_shape=out_shape,
                         out_strides=strides(out_shape), dtype=dtype, out_dtype=dtype, **kw)


def test_plain_3x3():
    d = dense((2, 5, 7, 32), (64, 3, 3, 32), stride=1, pad=1)
    # OH = (H + 2 * pad - dil * (KH - 1) - 1) // stride + 1        = (5 + 2 - 2 - 1) // 1 + 1
    # OW = (W + 2 * pad - dil * (KW - 1) - 1) // stride + 1        = (7 + 2 - 2 - 1) // 1 + 1
    assert (d.N, d.H, d.W, d.Cin, d.Cout, d.KH, d.KW, d.OH, d.OW) == (2, 5, 7, 32, 64, 3, 3, 5, 7)
    assert (d.stride, d.pad, d.dil, d.act, d.shift_n_mod) == (1, 1, 1, 0, 1)
    # d.in_ = x.data_ptr(); d.weight = w.data_ptr(); d.out = out.data_ptr()
    assert (d.in_, d.weight, d.out) == (X, W, OUT)
    # d.in_cstride = in_cstride or Cs; d.in_nstride = x.stride(0) if N > 1 else 0
    assert (d.in_cstride, d.in_coff, d.in_nstride) == (32, 0, 5 * 7 * 32)
    # d.out_cstride = out.shape[-1]; d.out_nstride = out_nstride or (out.stride(0) if (out.dim() == 4 and N > 1) else 0)
    assert (d.out_cstride, d.out_coff, d.out_nstride) == (64, 0, 5 * 7 * 64)
    assert (d.dtype, d.out_dtype) == (F32, F32)
    # nothing that was not asked for
    assert not (d.scale or d.shift or d.shift_n or d.res1 or d.res2 or d.weight_x3 or d.weight_h2 or d.out2 or d.splitk_ws or
                d.gather_idx or d.m_dev or d.row_perm or d.row_mask)
    assert (d.res1_cstride, d.res1_f32, d.res1_up_h, d.res1_up_w, d.res2_cstride, d.pixel_shuffle2, d.in_pair, d.out_pair, d.in_up2,
            d.splitk_slices) == (0,) * 10


def test_a_batch_of_one_has_no_image_strides():
    d = dense((1, 5, 7, 32), (64, 3, 3, 32), pad=1)
    # d.in_nstride = x.stride(0) if N > 1 else 0;  d.out_nstride = ... (out.stride(0) if (out.dim() == 4 and N > 1) else 0)
    assert (d.N, d.OH, d.OW, d.in_nstride, d.out_nstride) == (1, 5, 7, 0, 0)


def test_the_7x7_stride_2_stem():
    d = dense((1, 10, 12, 32), (64, 7, 7, 32), stride=2, pad=3)
    # OH = (10 + 6 - 6 - 1) // 2 + 1 = 5;  OW = (12 + 6 - 6 - 1) // 2 + 1 = 6
    assert (d.OH, d.OW, d.stride, d.pad) == (5, 6, 2, 3)


def test_the_row_run_form_states_its_output_size():
    # the stem as lss.py runs it: 7 rows x one run of 32 contiguous elements = 8 pixels of a bordered 4-channel image
    d = dense((1, 10, 12, 4), (64, 7, 1, 32), out_shape=(1, 2, 2, 64), stride=2, pad=0, in_cstride=4, out_hw=(2, 2))
    # the formula would give OW = (12 - 0 - 1) // 2 + 1 = 6:   if out_hw is not None: OH, OW = out_hw
    assert (d.H, d.W, d.KH, d.KW, d.Cin, d.OH, d.OW) == (10, 12, 7, 1, 32, 2, 2)
    # d.in_cstride = in_cstride or Cs
    assert d.in_cstride == 4
    assert ops.conv_geometry((1, 10, 12, 4), (64, 7, 1, 32), stride=2, out_hw=(2, 2))[4] == (1, 2, 2, 64)


def test_an_output_window_of_a_wider_buffer():
    d = dense((2, 5, 7, 32), (64, 3, 3, 32), out_shape=(2, 5, 7, 96), pad=1, out_coff=32, in_coff=0)
    # d.out_cstride = out.shape[-1]; d.out_coff = out_coff;  out.stride(0) of the [2, 5, 7, 96] buffer
    assert (d.Cout, d.out_cstride, d.out_coff, d.out_nstride) == (64, 96, 32, 5 * 7 * 96)
    # the input side of the same: d.in_cstride = in_cstride or Cs; d.in_coff = in_coff  (a 32-channel window of 48)
    d = dense((2, 5, 7, 48), (64, 3, 3, 32), pad=1, in_coff=16)
    assert (d.Cin, d.in_cstride, d.in_coff, d.in_nstride) == (32, 48, 16, 5 * 7 * 48)


def test_an_explicit_out_nstride_overrides_the_tensors():
    # d.out_nstride = out_nstride or (...)
    assert dense((2, 5, 7, 32), (64, 3, 3, 32), pad=1, out_nstride=12345).out_nstride == 12345
    assert dense((1, 5, 7, 32), (64, 3, 3, 32), pad=1, out_nstride=12345).out_nstride == 12345
    # a row-linear (not 4-D) output has no image stride:  out.dim() == 4 and N > 1
    d = ops.conv_desc(x=X, x_shape=(2, 5, 7, 32), x_strides=strides((2, 5, 7, 32)), w=W, w_shape=(64, 1, 1, 32), out=OUT,
                      out_shape=(70, 64), out_strides=(64, 1), dtype=F32, out_dtype=F32)
    assert (d.out_cstride, d.out_nstride) == (64, 0)


def test_pixel_shuffle2():
    # cr = Cout // 4 if pixel_shuffle2 else Cout;  oh, ow = (2 * OH, 2 * OW) if pixel_shuffle2 else (OH, OW)
    assert ops.conv_geometry((2, 5, 7, 32), (64, 1, 1, 32), pixel_shuffle2=True) == (5, 7, 5, 7, (2, 10, 14, 16))
    d = dense((2, 5, 7, 32), (64, 1, 1, 32), pixel_shuffle2=True)
    # d.Cout = Cout (all four groups); d.out_cstride = out.shape[-1]; out.stride(0) of the [2, 10, 14, 16] tensor
    assert (d.Cout, d.OH, d.OW, d.pixel_shuffle2, d.out_cstride, d.out_nstride) == (64, 5, 7, 1, 16, 10 * 14 * 16)


def test_in_up2_doubles_the_logical_input():
    # if in_up2: H, W = 2 * H, 2 * W   (the geometry is that of the upsampled, logical input)
    assert ops.conv_geometry((1, 4, 6, 32), (64, 3, 3, 32), pad=1, in_up2=True) == (8, 12, 8, 12, (1, 8, 12, 64))
    d = dense((1, 4, 6, 32), (64, 3, 3, 32), pad=1, in_up2=True, weight_x3=0x4000)
    assert (d.H, d.W, d.OH, d.OW, d.in_up2, d.weight_x3) == (8, 12, 8, 12, 1, 0x4000)
    d = dense((2, 4, 6, 32), (64, 3, 3, 32), pad=1, in_up2=True)
    # d.in_nstride = x.stride(0): the SOURCE tensor's image stride
    assert (d.in_nstride, d.out_nstride) == (4 * 6 * 32, 8 * 12 * 64)


def test_res1_f32_beside_16_bit_operands():
    res = dict(res1=0x5000, res1_shape=(2, 5, 7, 64), res1_coff=0)
    # if res1 is not None and res1.dtype == torch.float32 and x.dtype != torch.float32: d.res1_f32 = 1
    assert dense((2, 5, 7, 32), (64, 1, 1, 32), dtype=F16, res1_dtype=F32, **res).res1_f32 == 1
    assert dense((2, 5, 7, 32), (64, 1, 1, 32), dtype=BF16, res1_dtype=F32, **res).res1_f32 == 1
    assert dense((2, 5, 7, 32), (64, 1, 1, 32), dtype=F32, res1_dtype=F32, **res).res1_f32 == 0
    assert dense((2, 5, 7, 32), (64, 1, 1, 32), dtype=F16, res1_dtype=F16, **res).res1_f32 == 0
    assert dense((2, 5, 7, 32), (64, 1, 1, 32), dtype=F16, res1_dtype=F32).res1_f32 == 0          # no res1 at all
    # d.res1 = ptr(res1); d.res1_cstride = 0 if res1 is None else res1.shape[-1]; d.res1_coff = res1_coff
    d = dense((2, 5, 7, 32), (64, 1, 1, 32), res1=0x5000, res1_shape=(2, 5, 7, 96), res1_dtype=F32, res1_coff=8,
              res2=0x6000, res2_shape=(2, 5, 7, 80), res2_coff=16)
    assert (d.res1, d.res1_cstride, d.res1_coff, d.res2, d.res2_cstride, d.res2_coff) == (0x5000, 96, 8, 0x6000, 80, 16)


def test_res1_up_takes_the_coarse_maps_size():
    # d.res1_up_h, d.res1_up_w = res1.shape[1], res1.shape[2]
    d = dense((2, 6, 8, 32), (64, 1, 1, 32), res1=0x5000, res1_shape=(2, 3, 4, 64), res1_dtype=F32, res1_up=True)
    assert (d.res1_up_h, d.res1_up_w, d.res1_cstride, d.OH, d.OW) == (3, 4, 64, 6, 8)
    d = dense((2, 6, 8, 32), (64, 1, 1, 32), res1=0x5000, res1_shape=(2, 6, 8, 64), res1_dtype=F32)
    assert (d.res1_up_h, d.res1_up_w) == (0, 0)


def test_the_operand_modes():
    d = dense((1, 5, 7, 32), (64, 3, 3, 32), pad=1, weight_x3=0x4000, in_pair=True, out_pair=False, out2=0x7000,
              out2_shape=(1, 5, 7, 128), out2_coff=64, scale=0x8000, shift=0x9000, shift_n=0xA000, shift_n_mod=6, act=2)
    # d.in_pair, d.out_pair = int(bool(in_pair)), int(bool(out_pair));  d.out2_cstride = out2.shape[-1]; d.out2_coff = out2_coff
    assert (d.weight_x3, d.in_pair, d.out_pair, d.out2, d.out2_cstride, d.out2_coff) == (0x4000, 1, 0, 0x7000, 128, 64)
    assert (d.scale, d.shift, d.shift_n, d.shift_n_mod, d.act) == (0x8000, 0x9000, 0xA000, 6, 2)
    assert dense((1, 5, 7, 32), (64, 3, 3, 32), dtype=F16, pad=1, weight_h2=0xB000).weight_h2 == 0xB000


def test_the_gather_form():
    M, taps, Cin, Cout = 3, 27, 16, 32
    d = ops.conv_desc(x=X, x_shape=(40, Cin), x_strides=None, w=W, w_shape=(Cout, 1, taps, Cin), out=OUT, out_shape=(M, Cout),
                      out_strides=None, dtype=F32, out_dtype=F32, stride=2, shift_n_mod=0, res1=0x5000, res1_shape=(M, Cout),
                      gather=(0xC000, 0xD000, M), plan=(0xE000, 0xF000))
    # d.N = M; d.H = 1; d.W = 1; d.Cin = Cin; d.in_cstride = Cin; d.in_coff = 0; d.in_nstride = 0
    assert (d.N, d.H, d.W, d.Cin, d.in_cstride, d.in_coff, d.in_nstride) == (3, 1, 1, 16, 16, 0, 0)
    # d.Cout = Cout; d.KH = 1; d.KW = KW; d.stride = stride; d.pad = 0; d.dil = 1
    assert (d.Cout, d.KH, d.KW, d.stride, d.pad, d.dil) == (32, 1, 27, 2, 0, 1)
    # d.OH = 1; d.OW = 1; d.out_cstride = Cout; d.out_coff = 0; d.out_nstride = 0
    assert (d.OH, d.OW, d.out_cstride, d.out_coff, d.out_nstride) == (1, 1, 32, 0, 0)
    # d.res1 = ptr(res); d.res1_cstride = 0 if res is None else res.shape[-1]      (and never res1_f32: not set there)
    assert (d.res1, d.res1_cstride, d.res1_f32) == (0x5000, 32, 0)
    # d.gather_idx = nbr.data_ptr(); d.m_dev = ptr(m_dev); d.row_perm, d.row_mask = plan[0].data_ptr(), plan[1].data_ptr()
    assert (d.gather_idx, d.m_dev, d.row_perm, d.row_mask) == (0xC000, 0xD000, 0xE000, 0xF000)
    assert (d.shift_n_mod, d.in_, d.weight, d.out) == (0, X, W, OUT)


def test_the_tape_refuses_the_inference_only_options_in_the_same_words():
    assert [msg for _, msg in ops._INFERENCE_ONLY] == [
        "conv2d: half-storage (h2) layers have no backward; train in dtype torch.float32 or 'f32x3'",
        "conv2d: pair-format activations are an inference-path layout (the tape reads f32 tensors)",
        "conv2d: in_up2 is an inference-path fusion (the tape records bilinear_up2 and the convolution apart)",
        "conv2d: a joined stage is an inference-path fusion (the tape records the two convolutions apart)",
    ]


def test_each_refusal_is_raised_under_a_tape_only(monkeypatch):
    for i, (_, msg) in enumerate(ops._INFERENCE_ONLY):
        used = [j == i for j in range(4)]
        monkeypatch.setattr(autodiff, "TAPE", None)
        ops._refuse_on_tape(*used)
        monkeypatch.setattr(autodiff, "TAPE", object())
        with pytest.raises(_lib.TTError) as e:
            ops._refuse_on_tape(*used)
        assert str(e.value) == msg
    ops._refuse_on_tape(False, False, False, False)


def test_the_training_rules(monkeypatch):
    """Cout < 64 and (TAPE is not None or _no_tape): no bf16x3 operand;  x3_splitk = TAPE is None and not _no_tape."""
    w_x3 = object()
    for tape, no_tape in ((None, False), (None, True), (object(), False), (object(), True)):
        monkeypatch.setattr(autodiff, "TAPE", tape)
        training = ops._in_training_step(no_tape)
        assert training == (tape is not None or no_tape)
        assert ops._training_x3(None, 32, training) == (None, None)
        assert ops._training_x3(w_x3, 63, training) == ((None, None) if training else (w_x3, w_x3))
        assert ops._training_x3(w_x3, 64, training) == ((w_x3, None) if training else (w_x3, w_x3))


def test_when_conv2d_asks_for_a_split_k_workspace(monkeypatch):
    """_AUTO_SPLITK and splitk_ws is None and not (in_pair or out_pair or in_up2) and w_h2 is None and not res1_up and
    N * OH * OW <= 4096 and KH * KW * Cin >= 2048"""
    monkeypatch.setattr(ops, "_AUTO_SPLITK", False)
    assert not ops.auto_splitk_asks(4096, 2048)
    monkeypatch.setattr(ops, "_AUTO_SPLITK", True)
    assert ops.auto_splitk_asks(4096, 2048) and not ops.auto_splitk_asks(4097, 2048) and not ops.auto_splitk_asks(4096, 2047)
    for mode in ("splitk_ws", "pair", "in_up2", "h2", "res1_up"):
        assert not ops.auto_splitk_asks(512, 4608, **{mode: True})


def test_the_order_conv2d_passes_the_builders_arguments_in():
    """conv2d calls conv_desc by position, one line of its call per line of the signature: moving a parameter means moving it there."""
    import inspect
    assert list(inspect.signature(ops.conv_desc).parameters) == [
        "x", "x_shape", "x_strides", "w", "w_shape", "out", "out_shape", "out_strides", "dtype", "out_dtype",
        "stride", "pad", "dil", "out_hw", "pixel_shuffle2", "in_up2",
        "in_coff", "in_cstride", "out_coff", "out_nstride",
        "scale", "shift", "shift_n", "shift_n_mod", "act",
        "res1", "res1_shape", "res1_dtype", "res1_coff", "res1_up", "res2", "res2_shape", "res2_coff",
        "weight_x3", "weight_h2", "in_pair", "out_pair", "out2", "out2_shape", "out2_coff",
        "gather", "plan"]
