"""The master weights of a training run: which state_dict entries train, their layout in ONE flat f32 device buffer, and the
device-side re-preparation of the kernels' operand formats from them.  Shared by the two owners a model can have -- the flat-buffer
`trainer.Trainer` (the fast path) and a `trainable=True` `EncoderDecoder` (torch autograd route, thinktwice_amd/autograd_route.py)
-- so both see the same parameters in the same order: the reference's `model.parameters()` order, which
`optimizer.state_dict()` indices of reference checkpoints are keyed by."""
import torch

from . import autodiff

# registered buffers of the reference modules (BatchNorm statistics; the LSS frustum / voxel grid constants, lss.py:470-476)
BUFFERS = ("running_mean", "running_var", "num_batches_tracked", "voxel_size", "voxel_coord", "voxel_num", "frustum")


def trainable(name, t):
    return torch.is_tensor(t) and t.is_floating_point() and t.dim() > 0 and not name.endswith(BUFFERS)


def strip(state_dict):
    """A checkpoint's `state_dict` without the DDP `module.` prefix and torch's `_metadata` entry."""
    return {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items() if k != "_metadata"}


def flat_masters(sd, device):
    """-> (names, flat, views): the trainable entries of `sd` in its order, one flat f32 buffer on `device` holding their
    values back to back, and {name: view of the flat buffer in the entry's shape}."""
    names = [k for k, v in sd.items() if trainable(k, v)]
    total = sum(sd[k].numel() for k in names)
    flat = torch.empty(total, dtype=torch.float32, device=device)
    views, off = {}, 0
    for k in names:
        v = sd[k]
        view = flat[off:off + v.numel()].view(v.shape)
        view.copy_(v.to(device, torch.float32))
        views[k] = view
        off += v.numel()
    return names, flat, views


def prepare_on_device(model, tensors, frozen_bn, load=None):
    """(Re)build the kernels' operand formats (folded BatchNorm affines, channel-last / pair-split weights) of `model` from
    `tensors` -- master-weight views and device-resident BatchNorm statistics under the reference's names -- with the load
    code running on the device tensors as they are: nothing crosses PCIe.  The tape's tensor -> parameter-name tables of THIS
    model are dropped first and refilled by the load (`autodiff.owned_by` inside it); in frozen-BN mode the folded scales with
    near-zero entries are flagged again (one host sync)."""
    autodiff.clear_metas(model)
    with torch.no_grad():
        (load or model.load_state_dict)(tensors)
        if frozen_bn:
            autodiff.refresh_small_scale_flags(owner=model)


def bn_calls_per_iteration(model, key):
    """nn.BatchNorm's call counter under model.train(): every BatchNorm inside the per-sweep camera pass is called once per
    SWEEP and iteration (lss.py:689-714; older sweeps run under no_grad but in train mode), the others once per iteration."""
    T = int((model.config or {}).get("queue_length", 1))
    return T if (key.startswith("img_encoder.") and "bev_multiframe_merge" not in key) else 1
