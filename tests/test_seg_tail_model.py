"""The fused seg feedback chain inside the forward: the small (F7-sized) configuration at batch 2 in the headline precision mode,
routed through tt_seg_feedback_chain (the default) against the two-launch form (ops.SEG_CHAIN = False, the TT_SEG_CHAIN=0 hook).
Every tensor `forward_inference(channel_last_out=True)` returns is bit-equal, eagerly and through a compiled launch plan."""
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


def _chain_calls(monkeypatch):
    """Count the launches of the fused entry through ops.seg_feedback_chain."""
    from thinktwice_amd import ops
    calls, real = [], ops.seg_feedback_chain

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(ops, "seg_feedback_chain", counted)
    return calls


def test_eager_forward_is_bit_equal_with_and_without_the_chain(model_and_batch, monkeypatch):
    from thinktwice_amd import ops
    m, batch = model_and_batch
    calls = _chain_calls(monkeypatch)
    monkeypatch.setattr(ops, "SEG_CHAIN", True)
    fused = {k: v.clone() for k, v in _tensors(m.forward_inference(batch, channel_last_out=True)).items()}
    assert len(calls) == 1, "the forward did not take the fused route"
    monkeypatch.setattr(ops, "SEG_CHAIN", False)
    plain = _tensors(m.forward_inference(batch, channel_last_out=True))
    torch.cuda.synchronize()
    assert len(calls) == 1, "the hook did not select the two-launch route"
    assert fused.keys() == plain.keys() and len(fused) > 10
    for k in fused:
        assert torch.equal(fused[k], plain[k]), k


def test_planned_forward_is_bit_equal_with_and_without_the_chain(model_and_batch, monkeypatch):
    """Batch 1: the plan compiler records single-sample forwards only (at batch 2 the decoder's (R, B) -> (B, R) transposes are
    torch copy kernels, which it refuses).  The segmentation map then has 8 x 64 x 128 = 65,536 rows, still the bf16x3 regime."""
    from thinktwice_amd import model as tm, ops, plan as P, synth
    m, _ = model_and_batch
    batch = tm.batch_to_device(synth.make_batch(1, img_hw=HW, num_points=NPTS))
    outs = []
    for chain in (True, False):
        monkeypatch.setattr(ops, "SEG_CHAIN", chain)
        fp = P.compile_forward(m, batch, channel_last_out=True)
        fp.update(batch)
        got = fp.run()
        torch.cuda.synchronize()
        outs.append(({k: v.clone() for k, v in got.items()}, fp.calls))
        del fp, got
    (fused, n_fused), (plain, n_plain) = outs
    assert n_fused == n_plain - 1, (n_fused, n_plain)     # two launches became one: the plan recorded the fused entry
    assert fused.keys() == plain.keys() and len(fused) > 5
    for k in fused:
        assert torch.equal(fused[k], plain[k]), k
