"""The master weights of a training run: which state_dict entries train, their layout in ONE flat f32 device buffer, and the
device-side re-preparation of the kernels' operand formats from them.  Shared by the two owners a model can have -- the flat-buffer
`trainer.Trainer` (the fast path) and a `trainable=True` `EncoderDecoder` (torch autograd route, thinktwice_amd/autograd_route.py)
-- so both see the same parameters in the same order: the reference's `model.parameters()` order, which
`optimizer.state_dict()` indices of reference checkpoints are keyed by."""
import torch

from . import autodiff, ops

# registered buffers of the reference modules (BatchNorm statistics; the LSS frustum / voxel grid constants, lss.py:470-476)
BUFFERS = ("running_mean", "running_var", "num_batches_tracked", "voxel_size", "voxel_coord", "voxel_num", "frustum")


def trainable(name, t):
    return torch.is_tensor(t) and t.is_floating_point() and t.dim() > 0 and not name.endswith(BUFFERS)


def strip(state_dict):
    """A checkpoint's `state_dict` without the DDP `module.` prefix and torch's `_metadata` entry."""
    return {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items() if k != "_metadata"}


class FlatLayout:
    """Where every trainable parameter lives in a flat buffer (master weights, gradient, Adam moments all share it): `names` in
    `model.parameters()` order, `layout[name]` -> (offset, numel, shape), `numel` in all.  Also the ONE place where a tape's
    parameter gradients become a flat buffer (`deposit`) and where the reached parameters become optimizer ranges."""

    def __init__(self, names, shapes):
        self.names, self._at, self.numel = list(names), {}, 0
        for k, shape in zip(self.names, shapes):
            n = int(torch.Size(shape).numel())
            self._at[k] = (self.numel, n, tuple(shape))
            self.numel += n

    def __getitem__(self, name):
        return self._at[name]

    def __contains__(self, name):
        return name in self._at

    def live_ranges(self, reached):
        """[(offset, count)] element ranges of the parameters named in `reached` (those that received a gradient; the others
        are skipped by the optimizer like torch's grad-is-None parameters): merged runs in flat-buffer order."""
        runs = []
        for k in self.names:
            off, n, _ = self._at[k]
            if k in reached:
                if runs and runs[-1][0] + runs[-1][1] == off:
                    runs[-1][1] += n
                else:
                    runs.append([off, n])
        return [tuple(r) for r in runs]

    def deposit(self, table, grads, flat, scale=None, accumulate=False):
        """flat[offset of name ...) (=|+=) scale * grads[name] for every entry of `grads` (a tape's `param_grads`), ONE launch
        of tt_grad_gather through `table` (an ops.GradSegTable); `scale`: device f32 scalar or None (1.0: the bits of the
        sources).  Elements of parameters without an entry are not written."""
        unknown = [k for k in grads if k not in self._at]
        assert not unknown, f"gradients for names outside the state_dict: {unknown[:5]}"
        srcs, offs = [], []
        for k, g in grads.items():
            off, n, _ = self._at[k]
            assert g.numel() == n and g.dtype == torch.float32, k
            srcs.append(g.reshape(-1) if g.is_contiguous() else g.contiguous().view(-1))
            offs.append(off)
        table.upload(srcs, offs, flat.numel())
        return ops.grad_gather(table, flat, scale, accumulate)


def flat_masters(sd, device):
    """-> (layout, flat, views): the FlatLayout of the trainable entries of `sd` in its order, one flat f32 buffer on `device`
    holding their values back to back, and {name: view of the flat buffer in the entry's shape}."""
    names = [k for k, v in sd.items() if trainable(k, v)]
    layout = FlatLayout(names, [sd[k].shape for k in names])
    flat = torch.empty(layout.numel, dtype=torch.float32, device=device)
    views = {}
    for k in names:
        off, n, shape = layout[k]
        views[k] = flat[off:off + n].view(shape)
        views[k].copy_(sd[k].to(device, torch.float32))
    return layout, flat, views


def operand_tensors(keys, params, buffers, other=None):
    """What the load code prepares the kernels' operands from, in the order of `keys`: the master parameter (detached) where
    `params` has the name, else the device-resident buffer, else `other`'s entry (KeyError without one)."""
    return {k: (params[k].detach() if k in params else buffers[k] if k in buffers or other is None else other[k]) for k in keys}


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
