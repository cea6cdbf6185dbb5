"""tt_seg_feedback_chain (csrc/seg_chain.hip): the two 1 x 1 feedback convolutions of seg_res_to_image_feature (n_class -> 64 -> 16,
folded BN, ReLU) as one launch, against the two tt_conv2d_fwd launches it replaces.

The specification is bit-identity: per stage the chain runs the arithmetic the convolution dispatch picks for that layer at the
row count -- the latency kernel up to 4096 rows, the exact-f32 tiles up to 65,535, bf16x3 on the second stage beyond -- so every
row count is compared with torch.equal.  256 and 4551 rows are the first two regimes (4551 is ragged against every tile); 70,087
rows (65,536 + 4551) is the regime the forward runs in, where the second stage multiplies in bf16x3.  Also checked: nothing but the
output's channel window is written (sentinels in the channel gap and in guard rows), two runs are bit-identical, the 12-channel
input the model passes equals the 16-channel one with four zero channels, and shapes outside the contract come back as an error
code before any launch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

RELU, NONE, SIGMOID = 1, 0, 2
SENT = -77.25
GUARD = 5


def _conv(w, scale, shift, act, x3):
    from thinktwice_amd import layers
    return layers.Conv(w, scale, shift, act={RELU: "relu", NONE: "none"}[act], x3=x3)


def _case(R, cs, n2, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, R, 1, cs, generator=g)
    if cs == 16:
        x[..., 12:] = 0.0                                        # 16 channels of which 12 are real, as the padded seg logits
    w1 = torch.randn(64, 1, 1, cs, generator=g) * 0.3
    w2 = torch.randn(n2, 1, 1, 64, generator=g) * 0.2
    aff = [torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.3,
           torch.rand(n2, generator=g) + 0.5, torch.randn(n2, generator=g) * 0.3]
    return [t.cuda().contiguous() for t in (x, w1, w2, *aff)]


def _two_launches(x, cv1, cv2, out, out_coff):
    from thinktwice_amd import ops
    return cv2(cv1(x), out=out, out_coff=out_coff), ops._last_conv_kernel()


def _buffer(R, stride):
    return torch.full((R + 2 * GUARD, stride), SENT, dtype=torch.float32, device="cuda")


@pytest.mark.parametrize("R,cs,n2,second", [(256, 16, 16, "conv_small_kernel"), (4551, 16, 16, "conv_igemm_kernel<float"),
                                            (70087, 16, 16, "true>"), (70087, 12, 16, "true>"), (4551, 16, 32, "conv_igemm_kernel<float"),
                                            (70087, 16, 8, "true>")],
                         ids=["256-rows-latency-kernel", "4551-rows-ragged-f32", "70087-rows-bf16x3", "70087-rows-12-channel-input",
                              "4551-rows-N2-32", "70087-rows-N2-8"])
def test_chain_is_bit_equal_to_the_two_conv_launches(R, cs, n2, second):
    from thinktwice_amd import ops
    x, w1, w2, s1, b1, s2, b2 = _case(R, cs, n2, seed=R + cs + n2)
    cv1, cv2 = _conv(w1, s1, b1, RELU, x3=False), _conv(w2, s2, b2, RELU, x3=True)
    assert cv2.w_x3 is not None
    stride, coff = n2 + 8, 4                                     # a channel stride larger than N2: sentinels on both sides
    ref = _buffer(R, stride)
    _, kern = _two_launches(x, cv1, cv2, ref[GUARD:GUARD + R].view(1, R, 1, stride), coff)
    assert second in kern, kern                                  # the reference's second stage ran the kernel this case is about
    outs = []
    for _ in range(2):
        buf = _buffer(R, stride)
        ops.seg_feedback_chain(x, cv1, cv2, out=buf[GUARD:GUARD + R].view(1, R, 1, stride), out_coff=coff)
        outs.append(buf)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]), "two runs on the same inputs differ"
    got = outs[0]
    assert torch.equal(got[GUARD:GUARD + R, coff:coff + n2], ref[GUARD:GUARD + R, coff:coff + n2])
    assert bool((got[:GUARD] == SENT).all()) and bool((got[GUARD + R:] == SENT).all()), "guard rows written"
    assert bool((got[:, :coff] == SENT).all()) and bool((got[:, coff + n2:] == SENT).all()), "channel gap written"
    assert float(got[GUARD:GUARD + R, coff:coff + n2].abs().max()) > 0.0            # ReLU left something to compare


def test_chain_without_affine_or_activation_matches_too():
    from thinktwice_amd import ops
    R = 70087
    x, w1, w2, s1, b1, s2, b2 = _case(R, 16, 16, seed=5)
    cv1, cv2 = _conv(w1, None, b1, NONE, x3=False), _conv(w2, s2, None, NONE, x3=True)
    want = cv2(cv1(x))
    got = ops.seg_feedback_chain(x, cv1, cv2)
    assert torch.equal(got, want)


def test_twelve_channel_input_equals_the_zero_padded_one():
    from thinktwice_amd import ops
    R = 70087
    x, w1, w2, s1, b1, s2, b2 = _case(R, 16, 16, seed=9)
    a = ops.seg_feedback_chain(x, _conv(w1, s1, b1, RELU, False), _conv(w2, s2, b2, RELU, True))
    b = ops.seg_feedback_chain(x[..., :12].contiguous(), _conv(w1[..., :12].contiguous(), s1, b1, RELU, False),
                               _conv(w2, s2, b2, RELU, True))
    assert torch.equal(a, b)


def test_shapes_outside_the_contract_are_refused_before_the_launch():
    from thinktwice_amd import _lib, weights
    L = _lib.lib()
    R = 512
    x = torch.zeros(R, 32, device="cuda")
    w1 = torch.zeros(64, 16, device="cuda")
    w2 = torch.zeros(32, 64, device="cuda")
    w2p = weights.split_pairs_x3(w2)
    out = torch.full((R, 64), SENT, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(R=R, x=x.data_ptr(), x_stride=16, K1=16, w1=w1.data_ptr(), act1=RELU, w2=w2.data_ptr(), w2p=w2p.data_ptr(), N2=16,
             act2=RELU, out=out.data_ptr(), out_stride=16, out_coff=0):
        return L.tt_seg_feedback_chain(x, R, x_stride, K1, w1, None, None, act1, w2, w2p, N2, None, None, act2, out, out_stride,
                                       out_coff, st)

    assert call() == 0
    torch.cuda.synchronize()
    out.fill_(SENT)
    bad = {"K1 = 8": dict(K1=8), "K1 = 32": dict(K1=32, x_stride=32), "N2 = 12": dict(N2=12), "N2 = 64": dict(N2=64, out_stride=64),
           "no rows": dict(R=0), "x_stride below K1": dict(x_stride=12), "x_stride not a multiple of 4": dict(x_stride=18),
           "window past the row": dict(out_stride=16, out_coff=4), "out_coff not a multiple of 4": dict(out_stride=32, out_coff=2),
           "sigmoid": dict(act1=SIGMOID), "sigmoid 2": dict(act2=SIGMOID), "no pair-format weights": dict(w2p=None),
           "no w1": dict(w1=None), "misaligned x": dict(x=x.data_ptr() + 4), "misaligned out": dict(out=out.data_ptr() + 8)}
    for what, kw in bad.items():
        rc = call(**kw)
        assert rc != 0, what
        assert b"tt_seg_feedback_chain" in L.tt_last_error(), what
    torch.cuda.synchronize()
    assert bool((out == SENT).all()), "a refused call wrote something"
