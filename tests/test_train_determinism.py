"""Two executions of one training step give the same bits: the backward's scatters (the look module's query gather and
deformable-attention sampling, csrc/look_bwd.hip; the deformable im2col's gx, csrc/glue_bwd.hip) add in a fixed order and without
float atomics.  runner.EpochRunner's bit-identical resume rests on this."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_two_backward_sweeps_of_one_batch_are_bit_identical():
    from thinktwice_amd import model as tm, ops, params, synth
    from thinktwice_amd.trainer import Trainer
    hw = (128, 256)
    m, cfg = tm.build_thinktwice(final_dim=hw, dtype="f32x3")
    tr = Trainer(m, params.init_params(cfg, seed=0), lr=1e-4, frozen_bn=False)
    batch = tm.batch_to_device(synth.make_batch(2, img_hw=hw, num_points=4096, seed=3))
    batch.update(synth.make_train_targets(2, img_hw=hw, seed=4))
    flats, buffers = [], {k: v.clone() for k, v in tr.buffers.items()}
    for _ in range(3):
        ops.DROPOUT_SEED[:] = [0x5EED, 0]                      # the same dropout masks
        for k, v in tr.buffers.items():                        # the same running statistics going in
            v.copy_(buffers[k])
        tr.backward(batch)
        flats.append(tr.grads.flat.clone())
    assert float(flats[0].norm()) > 0 and bool(torch.isfinite(flats[0]).all())
    assert torch.equal(flats[0], flats[1]) and torch.equal(flats[0], flats[2])
