"""tt_conv2d_plan (host only, no device) answers for the convolution that reads its input through the bilinear x2 upsampling
(tt_conv_desc.in_up2, csrc/conv_choose.cpp choose_up2), and ops.up2_ok asks it."""
from thinktwice_amd import _lib, ops
from tools import conv_choice_sweep as sweep

UP2 = "conv_x3_run3_kernel<64, up2>"


def _plan(N, h, w, cin, cout, up2=True, **kw):
    """Label (or "ERROR: text") for the 3 x 3 / pad 1 bf16x3 layer over the [N, 2h, 2w] map; in_up2: the descriptor ops.conv2d builds
    for the [N, h, w, cin] source, else the layer over a pair-format upsampled tensor (what the two launches run)."""
    row, _ = sweep.describe(sweep.D("up2", N, 2 * h, 2 * w, cin, cout, k=3, x3=True, in_pair=not up2, **kw), _lib.lib())
    if up2:
        row.update(in_up2=1, in_nstride=h * w * cin if N > 1 else 0)
    return ops.plan_label(sweep.dict_to_desc(row))


def test_the_label_starts_with_a_prefix_the_bench_counts_three_mfmas_for():
    from thinktwice_amd import bench_forward
    assert bench_forward.mfma_per_product(UP2, "bf16x3") == 3 and bench_forward.mfma_per_product(UP2, "bf16x3h") == 3


def test_plan_names_the_family_for_the_model_layer_and_the_test_shapes():
    # unet_layer0.1: 128 -> 64 over 224 x 448 per image, 8 images per sample; B = 8 and B = 1
    for N in (64, 8):
        assert _plan(N, 112, 224, 128, 64) == UP2
        assert _plan(N, 112, 224, 128, 64, out_pair=True) == UP2
    for N, h, w, cin in ((2, 20, 40, 32), (1, 33, 37, 64), (3, 8, 100, 128), (1, 1, 2100, 32), (1, 2100, 1, 32)):
        assert _plan(N, h, w, cin, 64) == UP2, (N, h, w, cin)


def test_the_old_choice_when_the_field_is_zero():
    for N in (64, 8):
        assert _plan(N, 112, 224, 128, 64, up2=False) == "conv_igemm_glds_kernel<float, 64, 8, 1, 128, 2, false, true> pre-split A"


def test_up2_ok_over_the_grid():
    """up2_ok from plain numbers: more than 4096 output rows, Cin a multiple of 32, 64 output channels -- exactly where the library
    plans the in_up2 kernel; everything else it refuses by name."""
    yes = 0
    for h, w in ((32, 32), (32, 33), (16, 32), (64, 64)):       # 4096 rows, 4224, 2048, 16384
        for cin in (16, 32, 48, 64, 128):
            for cout in (32, 48, 64, 128):
                label = _plan(1, h, w, cin, cout)
                ok = ops.up2_ok(4 * h * w, cin, cout)
                yes += ok
                assert ok == (4 * h * w > 4096 and cin % 32 == 0 and cout == 64), (h, w, cin, cout)
                assert ok == (ops.plan_label(*ops.canonical_desc("up2", 4 * h * w, cin, cout)) == UP2), (h, w, cin, cout)
                assert (label == UP2) == ok, (h, w, cin, cout, label)
                assert ok or (label.startswith("ERROR: tt_conv2d_fwd: in_up2") and len(label) > 40), label
    assert yes == 2 * 3


def test_refusals_without_a_device():
    assert "residual" in _plan(1, 40, 64, 32, 64, res=1)
    L = _lib.lib()
    row, _ = sweep.describe(sweep.D("both", 1, 80, 128, 32, 64, k=3, x3=True, in_pair=True), L)
    row.update(in_up2=1)
    msg = ops.plan_label(sweep.dict_to_desc(row))
    assert msg.startswith("ERROR") and "in_up2" in msg and "in_pair" in msg, msg
    row, _ = sweep.describe(sweep.D("odd", 1, 81, 128, 32, 64, k=3, x3=True), L)
    row.update(in_up2=1)
    assert "even" in ops.plan_label(sweep.dict_to_desc(row))
