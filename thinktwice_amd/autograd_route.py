"""The torch-autograd route of the training step: what a `trainable=True` EncoderDecoder needs so that the reference's own
training lines (apis/mmdet_train.py:70-97, configs/thinktwice.py:282-287) run on it unchanged --

    MMDistributedDataParallel(model.cuda(), ...)      wraps a module that HAS parameters
    build_optimizer(model, cfg.optimizer)              iterates model.parameters(), builds torch.optim.AdamW
    OptimizerHook: optimizer.zero_grad(); outputs['loss'].backward(); clip_grad_norm_(params, 100); optimizer.step()
    CheckpointHook: model.state_dict(), optimizer.state_dict()

  * `MasterState`: the master weights as nn.Parameters that are views of ONE flat f32 device buffer (masters.flat_masters: the
    layout trainer.Trainer uses), hung under the reference's names on a tree of empty container modules, with the BatchNorm
    running statistics, the call counters and the LSS constants as registered buffers -- `named_parameters()`, `state_dict()`
    and DistributedDataParallel then work through torch's own code.
  * `TapedLoss`: the autograd node behind `train_step(...)["loss"]`.  Its backward sweeps the tape of hand-written HIP backward
    kernels (autodiff.py) once, gathers the ~880 parameter gradients into one flat staging buffer scaled by grad_output
    (tt_grad_gather, one launch, no host sync) and RETURNS per-parameter views of it: AccumulateGrad does the accumulation,
    parameter hooks (DDP's reducer) fire, and a parameter the tape did not reach gets None, exactly as in torch.

The optimizer and the clip on this route are torch's; everything from the images to the gradients is this library's HIP.
`trainer.Trainer` remains the fast path (flat-buffer clip + AdamW in two launches, one all-reduce)."""
import torch

from . import _lib, autodiff, masters, ops

_PAD = 64          # BatchNorm statistics start on 256-byte boundaries of their flat buffer


class MasterState:
    """Master weights, buffers and their registration on `model` (an EncoderDecoder built with trainable=True)."""

    def __init__(self, model, sd):
        dev = model.device
        self.layout, self.flat, views = masters.flat_masters(sd, dev)
        self.names, self.keys = self.layout.names, list(sd)
        self.params, self.buffers = {}, {}
        # BatchNorm running statistics: views of one flat buffer (the prepared layers alias them and update them in place under
        # model.train(); one version counter tells when somebody else wrote them), call counters: views of one int64 buffer
        stat_keys = [k for k, v in sd.items() if torch.is_tensor(v) and k.endswith(("running_mean", "running_var"))]
        nbt_keys = [k for k, v in sd.items() if torch.is_tensor(v) and k.endswith("num_batches_tracked")]
        self.stats = torch.zeros(sum(-(-sd[k].numel() // _PAD) * _PAD for k in stat_keys), dtype=torch.float32, device=dev)
        self.nbt = torch.zeros(len(nbt_keys), dtype=torch.int64, device=dev)
        self.nbt_inc = torch.tensor([masters.bn_calls_per_iteration(model, k) for k in nbt_keys], dtype=torch.int64).to(dev)
        off = 0
        for k in stat_keys:
            n = sd[k].numel()
            self.buffers[k] = self.stats[off:off + n].view(sd[k].shape)
            off += -(-n // _PAD) * _PAD
        for i, k in enumerate(nbt_keys):
            self.buffers[k] = self.nbt[i]
        for k, v in sd.items():
            if k in views:
                self.params[k] = torch.nn.Parameter(views[k])          # (shares the flat buffer's storage and version counter)
            elif torch.is_tensor(v):
                if k not in self.buffers:
                    self.buffers[k] = torch.empty(v.shape, dtype=v.dtype, device=dev)
                self.buffers[k].copy_(v)
            else:
                raise _lib.TTError(f"trainable model: state_dict entry '{k}' is not a tensor")
        self._register(model)
        self.seen = None                   # (flat, stats) version counters the operands were prepared from
        self.stats_moved = False           # a train-mode forward updated the running statistics since
        self.flags_stale = True            # the frozen-BN small-scale flags belong to an earlier preparation
        self.table = ops.GradSegTable(dev)
        self.preparations = 0

    def _register(self, model):
        """Hang parameters and buffers under their dotted names: `register_parameter` refuses dots, so every name component but the
        last is an (empty) container module.  The model keeps its HIP sub-objects as plain attributes of the same top-level
        names (`model.img_encoder`, ...), so the containers go into `_modules` directly: attribute access still finds the
        sub-object, torch's traversals (named_parameters, state_dict, DDP) find the containers."""
        for k in self.keys:
            *path, leaf = k.split(".")
            mod = model
            for comp in path:
                if comp not in mod._modules:
                    mod._modules[comp] = torch.nn.Module()
                mod = mod._modules[comp]
            if k in self.params:
                mod.register_parameter(leaf, self.params[k])
            else:
                mod.register_buffer(leaf, self.buffers[k])

    @staticmethod
    def unregister(model):
        model._modules.clear()
        model._parameters.clear()
        model._buffers.clear()

    def copy_from(self, sd):
        """load_state_dict on an already trainable model: into the existing masters (parameter objects keep their identity)."""
        with torch.no_grad():
            for k, v in sd.items():
                dst = self.params.get(k, self.buffers.get(k))
                if dst is not None and torch.is_tensor(v):
                    dst.copy_(v)

    def versions(self):
        return (self.flat._version, self.stats._version)

    def operand_tensors(self):
        return masters.operand_tensors(self.keys, self.params, self.buffers)


class TapedLosses(dict):
    """forward_train's dict of loss terms (plain device scalars) carrying the tape its forward recorded: `_parse_losses` turns
    the parsed total into the graph-carrying `loss`.  Dropped without that, the tape goes with it."""
    tape = None


class _Route:
    def __init__(self, model, state, tape):
        self.model, self.state, self.tape = model, state, tape


class TapedLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, value, route, *params):
        ctx.route = route
        return value.detach().clone()

    @staticmethod
    def backward(ctx, grad_output):
        route = ctx.route
        tape, st = route.tape, route.state
        if tape is None:
            raise RuntimeError("EncoderDecoder (trainable): backward through this `loss` a second time -- its tape was released "
                               "by the first backward(); run train_step again")
        route.tape = None
        tape.backward()
        grads, tape.param_grads = tape.param_grads, {}
        # (a buffer of its own per backward: AccumulateGrad may keep the views as `.grad`)
        flat = torch.empty(st.flat.numel(), dtype=torch.float32, device=st.flat.device)
        st.layout.deposit(st.table, grads, flat, grad_output.detach().to(torch.float32).reshape(1))
        out = []
        for i, k in enumerate(st.names):
            if k in grads and ctx.needs_input_grad[2 + i]:
                off, n, shape = st.layout[k]
                out.append(flat[off:off + n].view(shape))
            else:
                out.append(None)
        return (None, None, *out)


def attach(model, state, tape, value):
    """-> `value` (the parsed total loss, a plain device scalar) as the output of the autograd node that owns `tape`."""
    return TapedLoss.apply(value, _Route(model, state, tape), *[state.params[k] for k in state.names])
