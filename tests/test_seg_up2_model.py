"""unet_layer0's upsample read inside unet_layer0.1's convolution, in the forward: the small (F7-sized) configuration in the headline
precision mode, with the fused launch (the default) against the two launches (ops.SEG_UP2 = False, the TT_SEG_UP2=0 hook).  Every
tensor `forward_inference(channel_last_out=True)` returns is bit-equal, eagerly at batch 2 and through a compiled launch plan."""
import pytest
import torch

pytestmark = pytest.mark.gpu

HW, NPTS, SEED = (128, 256), 3000, 11


def _tensors(out, prefix=""):
    """Flatten a forward's result (dict / list / tuple nesting) into {path: tensor}."""
    flat = {}
    if torch.is_tensor(out):
        flat[prefix] = out
    elif isinstance(out, dict):
        for k, v in out.items():
            flat.update(_tensors(v, f"{prefix}/{k}"))
    elif isinstance(out, (list, tuple)):
        for i, v in enumerate(out):
            flat.update(_tensors(v, f"{prefix}[{i}]"))
    return flat


@pytest.fixture(scope="module")
def model_and_batch():
    from thinktwice_amd import model as tm, params, synth
    m, cfg = tm.build_thinktwice(dtype="f32x3h", final_dim=HW)
    m.load_state_dict(params.init_params(cfg, seed=SEED))
    return m, tm.batch_to_device(synth.make_batch(2, img_hw=HW, num_points=NPTS))


def _up2_launches(monkeypatch):
    """Count the convolution launches that ask for in_up2."""
    from thinktwice_amd import ops
    calls, real = [], ops.conv2d

    def counted(*a, **kw):
        if kw.get("in_up2"):
            calls.append(ops.up2_ok(a[0].shape[0] * 4 * a[0].shape[1] * a[0].shape[2], a[0].shape[3], a[1].shape[0]))
        return real(*a, **kw)
    monkeypatch.setattr(ops, "conv2d", counted)
    return calls


def test_eager_forward_is_bit_equal_with_and_without_the_fusion(model_and_batch, monkeypatch):
    from thinktwice_amd import ops
    m, batch = model_and_batch
    calls = _up2_launches(monkeypatch)
    monkeypatch.setattr(ops, "SEG_UP2", True)
    fused = {k: v.clone() for k, v in _tensors(m.forward_inference(batch, channel_last_out=True)).items()}
    n = len(calls)
    assert n >= 1 and all(calls), "the forward did not take the fused route"
    monkeypatch.setattr(ops, "SEG_UP2", False)
    plain = _tensors(m.forward_inference(batch, channel_last_out=True))
    torch.cuda.synchronize()
    assert len(calls) == n, "the hook did not select the two-launch route"
    assert fused.keys() == plain.keys() and len(fused) > 10
    for k in fused:
        assert torch.equal(fused[k], plain[k]), k


def test_planned_forward_is_bit_equal_with_and_without_the_fusion(model_and_batch, monkeypatch):
    """Batch 1 (the plan compiler records single-sample forwards): unet_layer0.1 then has 8 x 64 x 128 = 65,536 output rows."""
    from thinktwice_amd import model as tm, ops, plan as P, synth
    m, _ = model_and_batch
    batch = tm.batch_to_device(synth.make_batch(1, img_hw=HW, num_points=NPTS))
    calls = _up2_launches(monkeypatch)
    outs = []
    for up2 in (True, False):
        monkeypatch.setattr(ops, "SEG_UP2", up2)
        fp = P.compile_forward(m, batch, channel_last_out=True)
        fp.update(batch)
        got = fp.run()
        torch.cuda.synchronize()
        outs.append(({k: v.clone() for k, v in got.items()}, fp.calls))
        del fp, got
    (fused, n_fused), (plain, n_plain) = outs
    assert calls and all(calls), "the recorded forward did not take the fused route"
    assert n_fused == n_plain - 1, (n_fused, n_plain)     # the upsample launch is gone: the plan recorded one call fewer
    assert fused.keys() == plain.keys() and len(fused) > 5
    for k in fused:
        assert torch.equal(fused[k], plain[k]), k
