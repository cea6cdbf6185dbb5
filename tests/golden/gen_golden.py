"""Generate the committed golden fixtures by running the REFERENCE's own python modules.

Run in the build container only (needs /root/reference):
    python tests/golden/gen_golden.py [--only F3,...]

Each fixture is data: inputs (or the seeds that regenerate them) + the outputs the
reference code produced.  See tests/golden/README.md for the list.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ref_stubs  # noqa: E402


def _save(name, **arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


# ---------------------------------------------------------------------------
# F3: VoxelPooling python wrapper semantics (ops/voxel_pooling/voxel_pooling.py:10-55)
# ---------------------------------------------------------------------------
def gen_f3():
    from oracle import c_ref

    def ext_fwd(batch_size, num_points, num_channels, vx, vy, vz, geom, feats, out, memo):
        # stands in for the CUDA-only extension symbol (voxel_pooling_forward.cpp:24-37):
        # restated kernel semantics on the caller-allocated buffers
        o, m = c_ref.voxel_pool_fwd(geom.numpy(), feats.numpy(), (int(vx), int(vy), int(vz)))
        out += torch.from_numpy(o)
        sel = torch.from_numpy(m[..., 0] != -1)
        memo[sel] = torch.from_numpy(m)[sel]
        return 1

    ref_stubs.install({"voxel_pooling_ext_fwd": ext_fwd})
    vp = ref_stubs.ref_import("ops.voxel_pooling.voxel_pooling")

    g = torch.Generator().manual_seed(303)
    B, Np, C = 2, 2048, 8
    vx, vy, vz = 21, 21, 1
    geom = torch.stack([
        torch.randint(-3, vx + 3, (B, Np), generator=g),
        torch.randint(-3, vy + 3, (B, Np), generator=g),
        torch.randint(-1, vz + 1, (B, Np), generator=g),
    ], -1).to(torch.int32)
    # the (-1,0) -> 0 truncation case of LSS.voxel_pooling_method (lss.py:630-631): produce some
    # indices through the reference's own float -> .int() expression
    fl = torch.tensor([-0.999, -0.5, -1e-7, 0.0, 0.999, 20.999, 21.0, -1.0, -1.0001])
    trunc = fl.int()
    geom[0, : len(fl), 0] = trunc
    geom[0, : len(fl), 1] = 3
    geom[0, : len(fl), 2] = 0
    # long runs into a single cell (contention case) and an all-out-of-range tail
    geom[1, 100:400] = torch.tensor([5, 7, 0], dtype=torch.int32)
    geom[1, -64:] = torch.tensor([-1, -1, -1], dtype=torch.int32)
    feats = torch.randn(B, Np, C, generator=g)
    feats.requires_grad_(True)
    voxel_num = torch.tensor([vx, vy, vz])
    out = vp.voxel_pooling(geom.contiguous(), feats.contiguous(), voxel_num)  # [B,C,Y,X]
    grad_out = torch.randn(out.shape, generator=g)
    out.backward(grad_out)
    _save("f3_voxel_pool.npz", geom=geom.numpy(), feats=feats.detach().numpy(),
          voxel_num=np.array([vx, vy, vz]), out=out.detach().numpy(),
          trunc_float=fl.numpy(), trunc_int=trunc.numpy(),
          grad_out=grad_out.numpy(), grad_in=feats.grad.numpy())


# ---------------------------------------------------------------------------
# F12: camera-matrix assembly, frustum, geometry, voxel index
#      (backbones/lss.py:454-512, 629-631, 667-687)
# ---------------------------------------------------------------------------
def _lss_namespace(lss_mod):
    import types as _t
    from oracle import lss_geometry as og
    ns = _t.SimpleNamespace()
    ns.final_dim = (448, 896)
    ns.downsample_factor = 16
    ns.d_bound = [1.0, 41.0, 0.5]
    ns.frustum = lss_mod.LSS.create_frustum(ns)
    # buffers exactly as LSS.__init__ registers them (lss.py:386-397)
    x_bound, y_bound, z_bound = [-8.0, 30.4, 1.8285], [-19.2, 19.2, 1.8285], [-4, 10, 14]
    ns.voxel_size = torch.Tensor([row[2] for row in [x_bound, y_bound, z_bound]])
    ns.voxel_coord = torch.Tensor([row[0] + row[2] / 2.0 for row in [x_bound, y_bound, z_bound]])
    ns.voxel_num = torch.LongTensor([(row[1] - row[0]) / row[2] for row in [x_bound, y_bound, z_bound]])
    return ns


def gen_f12():
    from oracle import c_ref
    from oracle import lss_geometry as og
    from thinktwice_amd import synth
    captured = {}

    def ext_fwd(batch_size, num_points, num_channels, vx, vy, vz, geom, feats, out, memo):
        captured["geom_int"] = geom.clone()
        o, m = c_ref.voxel_pool_fwd(geom.numpy(), feats.numpy(), (int(vx), int(vy), int(vz)))
        out += torch.from_numpy(o)
        return 1

    ref_stubs.install({"voxel_pooling_ext_fwd": ext_fwd})
    lss = ref_stubs.ref_import("model_code.backbones.lss")
    ns = _lss_namespace(lss)
    # one non-identity curr2key for the previous sweep (dead data in the reference, A10 quirk)
    c2k = np.eye(4, dtype=np.float32)
    c2k[:2, :2] = [[np.cos(0.05), np.sin(0.05)], [-np.sin(0.05), np.cos(0.05)]]
    c2k[0, 3], c2k[1, 3] = 0.7, -0.2
    metas = synth.make_img_metas(2, curr2key=c2k)
    intr, ida, s2e, l2i, cur_ida = og.assemble_camera_mats(metas)
    # reference geometry for the key sweep (index -1), matmul formulation
    geom_ref = lss.LSS.get_geometry(ns, s2e[:, -1], intr[:, -1], ida[:, -1], None)
    B, N, D, H, W, _ = geom_ref.shape
    feats = torch.ones(B, N, D, H, W, 1)
    bev = lss.LSS.voxel_pooling_method(ns, geom_ref, feats.contiguous(), ns.voxel_num)
    idx_ref = captured["geom_int"].reshape(B, N, D, H, W, 3)
    # oracle restatement (explicit k-ordered arithmetic)
    geom_o = og.get_geometry(ns.frustum, s2e[:, -1], intr[:, -1], ida[:, -1])
    idx_o = og.voxel_index(geom_o, ns.voxel_coord, ns.voxel_size)
    mism = int((idx_o != idx_ref).any(-1).sum())
    print("geometry max abs diff", float((geom_o - geom_ref).abs().max()), "index mismatches", mism)
    hist = bev[:, 0].to(torch.int64)  # counts per cell [B,Y,X]
    inr = int(hist[0].sum())
    print("in-range points per sample:", inr, "max per cell", int(hist[0].max()))
    g = torch.Generator().manual_seed(12)
    sel = torch.randint(0, N * D * H * W, (256,), generator=g)
    _save("f12_geometry.npz",
          frustum_corners=ns.frustum[[0, 0, -1, -1], [0, -1, 0, -1], [0, -1, -1, 0]].numpy(),
          frustum_shape=np.array(ns.frustum.shape),
          intrin=intr.numpy(), ida=ida.numpy(), sensor2ego=s2e.numpy(), lidar2img=l2i.numpy(),
          cur_ida=cur_ida.numpy(), curr2key=c2k,
          voxel_size=ns.voxel_size.numpy(), voxel_coord=ns.voxel_coord.numpy(),
          voxel_num=ns.voxel_num.numpy(),
          sample_index=sel.numpy(),
          geom_sample=geom_ref.reshape(B, -1, 3)[:, sel].numpy(),
          idx_sample=idx_ref.reshape(B, -1, 3)[:, sel].numpy(),
          cell_hist=hist.numpy().astype(np.int32),
          idx_ref_packed=np.packbits(((idx_ref[0] >= 0) & (idx_ref[0] < ns.voxel_num.int())).all(-1).numpy().reshape(-1)),
          idx_mismatch_vs_oracle=np.array([mism]))


# ---------------------------------------------------------------------------
# F7: the reference EncoderDecoder (in-repo modules imported unmodified; third-party
#     arithmetic adapted onto the oracle restatements) vs the oracle, end to end.
# ---------------------------------------------------------------------------
def build_reference_model(cfg, sd):
    """Instantiate the reference EncoderDecoder under the import shims and load `sd`."""
    import torch.nn as nn
    from oracle import c_ref
    from oracle import model_ref as M

    class FnModule(nn.Module):
        def __init__(self, fn):
            super().__init__()
            self.fn = fn

        def forward(self, *a, **k):
            return self.fn(*a, **k)

        def init_weights(self):
            pass

    class BasicBlock(nn.Module):          # [3P] mmdet BasicBlock(inplanes, planes)
        def __init__(self, inplanes, planes):
            super().__init__()
            self.conv1 = nn.Conv2d(inplanes, planes, 3, padding=1, bias=False)
            self.bn1 = nn.BatchNorm2d(planes)
            self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
            self.bn2 = nn.BatchNorm2d(planes)

        def forward(self, x):
            return M.basic_block({"b." + k: v for k, v in self.state_dict(keep_vars=True).items()}, "b", x)

    class DCN(nn.Module):                 # [3P] mmcv DeformConv2dPack
        def __init__(self, in_channels, out_channels, kernel_size, padding, groups, im2col_step=128):
            super().__init__()
            self.weight = nn.Parameter(torch.zeros(out_channels, in_channels // groups, 3, 3))
            self.conv_offset = nn.Conv2d(in_channels, 18, 3, padding=1)
            self.groups = groups

        def forward(self, x):
            return M.dcn({"d." + k: v for k, v in self.state_dict(keep_vars=True).items()}, "d", x, self.groups)

    def ext_fwd(batch_size, num_points, num_channels, vx, vy, vz, geom, feats, out, memo):
        o, m = c_ref.voxel_pool_fwd(geom.numpy(), feats.detach().numpy(), (int(vx), int(vy), int(vz)),
                                    acc64=False)
        out += torch.from_numpy(o)
        sel = torch.from_numpy(m[..., 0] != -1)        # pos_memo drives the reference's backward (VP.py:57-69)
        memo[sel] = torch.from_numpy(m)[sel]
        return 1

    def msda_core(value, spatial_shapes, loc, attw):
        return M.msda_core(value, [tuple(int(v) for v in s) for s in spatial_shapes], loc, attw)

    holder = {}

    def build_backbone(c):
        c = dict(c)
        t = c.pop("type")
        if t == "LSS":
            return holder["lss"].LSS(**c)
        if t == "ResNet":
            return FnModule(lambda x: tuple(M.resnet50(sd, "img_encoder.img_backbone", x)))
        if t == "LidarNet":
            return FnModule(lambda pts: M.lidar_net(sd, "lidar_encoder", cfg, pts))
        raise KeyError(t)

    def build_neck(c):
        return FnModule(lambda feats: tuple(M.pafpn(sd, "img_encoder.img_neck", list(feats))))

    def build_head(c):
        c = dict(c)
        c.pop("type")
        return holder["dec"].ThinkTwiceDecoder(**c)

    def build_conv_layer(c, *a, **k):
        c = dict(c)
        assert c.pop("type") == "DCN"
        return DCN(**c)

    ref_stubs.install({"voxel_pooling_ext_fwd": ext_fwd, "msda_core": msda_core, "BasicBlock": BasicBlock,
                       "build_conv_layer": build_conv_layer, "build_backbone": build_backbone,
                       "build_neck": build_neck, "build_head": build_head})
    holder["lss"] = ref_stubs.ref_import("model_code.backbones.lss")
    holder["dec"] = ref_stubs.ref_import("model_code.dense_heads.thinktwice_decoder")
    edf = ref_stubs.ref_import("encoder_decoder_framework")
    tcfg = ref_stubs.ConfigDict(cfg["cfg"])
    enc = dict(cfg["img_encoder"])
    enc["final_dim"] = tuple(enc["final_dim"])
    model = edf.EncoderDecoder(
        img_encoder=enc,
        decoder=dict(type="ThinkTwiceDecoder", config=tcfg, bev_h=21, bev_w=21),
        lidar_encoder=dict(cfg["lidar_encoder"]), num_cams=4, use_depth=True, train_cfg=tcfg, test_cfg=tcfg)
    res = model.load_state_dict(sd, strict=False)
    third_party = ("img_encoder.img_backbone.", "img_encoder.img_neck.", "lidar_encoder.")
    unexpected = [k for k in res.unexpected_keys if not k.startswith(third_party)]
    assert not res.missing_keys, f"param_spec misses reference keys: {res.missing_keys[:10]}"
    assert not unexpected, f"param_spec has keys the reference lacks: {unexpected[:10]}"
    model.eval()
    return model


def _pack_pred(pred, sample_gen, nsample=256):
    out = {}
    for k, v in pred.items():
        if not torch.is_tensor(v):
            continue
        v = v.detach().float()
        if v.numel() <= 4096:
            out[k] = v.numpy()
        else:
            idx = torch.randint(0, v.numel(), (nsample,), generator=sample_gen)
            out[k + "__idx"] = idx.numpy()
            out[k + "__val"] = v.reshape(-1)[idx].numpy()
            out[k + "__stats"] = np.array([float(v.mean()), float(v.abs().mean()), float(v.abs().max())])
    return out


def _gen_forward(name, B, hw, npts, seed=0, nsample=256):
    import json
    import time
    from oracle import model_ref as M
    from thinktwice_amd import config, params, synth
    cfg = config.model_config(final_dim=hw)
    sd = params.init_params(cfg, seed=seed)
    model = build_reference_model(cfg, sd)
    # reference state_dict names/shapes of the in-repo modules (Appendix B check)
    ref_keys = {k: list(v.shape) for k, v in model.state_dict().items()}
    batch = synth.make_batch(B, img_hw=hw, num_points=npts)
    t0 = time.time()
    with torch.no_grad():
        ref = model.forward_inference(batch)
        t1 = time.time()
        ora = M.forward_inference(sd, cfg, batch, return_intermediates=True)
    t2 = time.time()
    print(f"reference forward {t1 - t0:.1f}s, oracle forward {t2 - t1:.1f}s")
    worst = 0.0
    for k, v in ref.items():
        if torch.is_tensor(v):
            e = float((v - ora[k]).abs().max() / v.abs().max().clamp_min(1e-6))
            worst = max(worst, e)
            print(f"  {k:34s} shape {tuple(v.shape)}  rel-max err oracle vs reference {e:.2e}")
    assert worst < 1e-4, worst
    g = torch.Generator().manual_seed(99)
    pack = _pack_pred(ref, g, nsample)
    g = torch.Generator().manual_seed(98)
    inter = _pack_pred({"cam_bev": ora["_cam_bev"], "lidar_bev": ora["_lidar_bev"], "flat": ora["_flat"],
                        "seg": ora["_cam"]["seg"], "depth": ora["_cam"]["depth"],
                        "context": ora["_cam"]["context"],
                        "fpn0": ora["_cam"]["fpn_feats"][0], "fpn3": ora["_cam"]["fpn_feats"][3]}, g, nsample)
    pack.update({"inter__" + k: v for k, v in inter.items()})
    pack["look_max_len"] = np.array([i["max_len"] for i in ora["_look_info"]])
    pack["look_count"] = torch.stack([i["count"] for i in ora["_look_info"]]).numpy()
    pack["meta"] = np.array([B, hw[0], hw[1], npts, seed])
    pack["oracle_vs_reference_worst_rel_err"] = np.array([worst])
    _save(name, **pack)
    return ref_keys


def gen_f7():
    import json
    keys = _gen_forward("f7_forward_small_b2.npz", 2, (128, 256), 20000)
    with open(os.path.join(HERE, "reference_state_dict_keys.json"), "w") as f:
        json.dump(keys, f, indent=0, sort_keys=True)


def gen_f8():
    _gen_forward("f8_forward_full_b1.npz", 1, (448, 896), 65536)


def gen_f14():
    """BASELINE configs 2 / 3: the reference's forward_inference at batch 8, thinktwice.py size (the SCA batch
    coupling of multi_scale_deformable_attn_function.py:338-341 makes B=8 different arithmetic from B=1/2)."""
    _gen_forward("f14_forward_full_b8.npz", 8, (448, 896), 65536, nsample=2048)


# ---------------------------------------------------------------------------
# F9: closed-loop post-processing (EDF:268-390, code/utils.py:7-29) -- a 16-tick sequence through the
#     reference model's process_action / control_pid (stateful PID windows)
# ---------------------------------------------------------------------------
def gen_f9():
    from thinktwice_amd import config, params
    cfg = config.model_config(final_dim=(128, 256))
    sd = params.init_params(cfg, seed=0, parts=("fusion", "decoder", "img_encoder"))
    model = build_reference_model(cfg, sd)
    g = torch.Generator().manual_seed(9)
    rec = {k: [] for k in ("mu", "sigma", "wp", "speed", "target", "pa", "pid")}
    for t in range(16):
        mu = torch.rand(1, 6, 2, generator=g) * 3.0
        sigma = torch.rand(1, 6, 2, generator=g) * 3.0
        if t % 4 == 1:
            mu[:, -1] = mu[:, -1] * 0.2           # alpha <= 1 branches
        if t % 4 == 2:
            sigma[:, -1] = sigma[:, -1] * 0.2
        wp = torch.cumsum(torch.rand(1, 4, 2, generator=g) * torch.tensor([0.6, 1.5]) + torch.tensor([-0.3, 0.1]), 1)
        speed = torch.rand(1, generator=g) * (0.005 if t == 5 else 8.0)
        target = (torch.randn(2, generator=g) * torch.tensor([3.0, 10.0]) + torch.tensor([0.0, 12.0])).numpy()
        pred = {"mu_branches": mu, "sigma_branches": sigma}
        s1, th1, b1, _ = model.process_action(pred, 3, speed, target)
        s2, th2, b2, m2 = model.control_pid(wp, speed, target.copy())
        rec["mu"].append(mu.numpy()); rec["sigma"].append(sigma.numpy()); rec["wp"].append(wp.numpy())
        rec["speed"].append(speed.numpy()); rec["target"].append(target)
        rec["pa"].append([s1, th1, b1])
        rec["pid"].append([s2, th2, float(b2), m2["desired_speed"], m2["angle"], m2["angle_last"], m2["angle_target"],
                           m2["angle_final"], m2["delta"]])
    _save("f9_control.npz", **{k: np.asarray(v, dtype=np.float64) for k, v in rec.items()})


def gen_f10():
    """F10: the reference's TRAINING forward (`EncoderDecoder.forward_train`: teacher-forcing pass + every loss term)
    under model.eval() (running-statistics BN), B=2 128x256, synthetic supervision; oracle/train_ref.py must
    reproduce every loss."""
    from oracle import train_ref as TR
    from thinktwice_amd import config, params, synth
    B, hw, npts, seed = 2, (128, 256), 20000, 0
    cfg = config.model_config(final_dim=hw)
    sd = params.init_params(cfg, seed=seed)
    model = build_reference_model(cfg, sd)
    batch = synth.make_batch(B, img_hw=hw, num_points=npts)
    batch.update(synth.make_train_targets(B, img_hw=hw))
    with torch.no_grad():
        ref = model.forward_train(batch)
        ora, _ = TR.forward_train(sd, cfg, batch)
    pack, worst = {}, 0.0
    assert set(ref) == set(ora), (sorted(set(ref) ^ set(ora)))
    for k, v in ref.items():
        v = v.detach().float()
        e = float((v - ora[k]).abs().max() / v.abs().max().clamp_min(1e-12))
        worst = max(worst, e)
        print(f"  {k:40s} {tuple(v.shape)} ref {float(v.mean()):+.6e}  oracle rel err {e:.2e}")
        pack[k] = v.numpy()
    assert worst < 1e-5, worst
    pack["meta"] = np.array([B, hw[0], hw[1], npts, seed])
    pack["oracle_vs_reference_worst_rel_err"] = np.array([worst])
    _save("f10_train_losses_b2.npz", **pack)


TRAIN_CALIB_JITTER = 77      # seed of the per-(sample, camera) calibration jitter of the train-mode goldens F11 / F16


def gen_f11():
    """F11: as F10 but under model.train(): batch-statistics BatchNorm everywhere (each sweep through the camera trunk
    on its own) and the live ASPP Dropout(0.5); the same torch seed is set before the reference and the oracle
    forward so both draw the same dropout masks."""
    from oracle import train_ref as TR
    from thinktwice_amd import config, params, synth
    B, hw, npts, seed, rng = 2, (128, 256), 20000, 0, 20240607
    cfg = config.model_config(final_dim=hw)
    sd = params.init_params(cfg, seed=seed)
    model = build_reference_model(cfg, sd)
    batch = synth.make_batch(B, img_hw=hw, num_points=npts, jitter_calib=TRAIN_CALIB_JITTER)   # (see synth.make_img_metas)
    batch.update(synth.make_train_targets(B, img_hw=hw))
    model.train()
    with torch.no_grad(), TR.train_mode():            # the third-party stand-ins call the oracle blocks: same switch
        torch.manual_seed(rng)
        ref = model.forward_train(batch)
        torch.manual_seed(rng)
        ora, _ = TR.forward_train(sd, cfg, batch)
    model.eval()
    pack, worst = {}, 0.0
    assert set(ref) == set(ora), (sorted(set(ref) ^ set(ora)))
    for k, v in ref.items():
        v = v.detach().float()
        e = float((v - ora[k]).abs().max() / v.abs().max().clamp_min(1e-12))
        worst = max(worst, e)
        print(f"  {k:40s} {tuple(v.shape)} ref {float(v.mean()):+.6e}  oracle rel err {e:.2e}")
        pack[k] = v.numpy()
    assert worst < 1e-5, worst
    pack["meta"] = np.array([B, hw[0], hw[1], npts, seed, rng, TRAIN_CALIB_JITTER])
    pack["oracle_vs_reference_worst_rel_err"] = np.array([worst])
    _save("f11_train_losses_trainmode_b2.npz", **pack)


def _grad_leaves(sd):
    skip = ("running_mean", "running_var", "num_batches_tracked", "voxel_size", "voxel_coord", "voxel_num", "frustum")
    return {k: (v.clone().requires_grad_() if v.is_floating_point() and not k.endswith(skip) else v)
            for k, v in sd.items()}


def gen_f16():
    """F16: F13 under model.train() -- the reference's TRAINING semantics (batch-statistics BatchNorm everywhere, each
    sweep through the camera trunk on its own; live ASPP Dropout(0.5) drawing from torch's global RNG, seeded right before
    each forward): total loss, every loss term and the gradient of the total loss w.r.t. every parameter, reference autograd
    vs autograd through the oracle restatement in train mode."""
    # B = 4: the model's BatchNorm1d layers (output_fc.2 over B rows, the shared flatten tail over 4 B rows) are batch-size
    # conditioned -- over TWO rows the normalised value is +-1 / sqrt(1 + 4 eps / d^2), whose derivative reaches 1 / (2 sqrt(eps))
    # = 158 wherever the two samples nearly agree; measured at B = 2: 1e-6 differences of two f32 implementations grow to 1e-4
    # at `flat` and ~4e-3 (median) on the gradients.  Four rows need four near-equal samples for the same blow-up.
    _gen_gradients("f16_train_gradients_trainmode_b4.npz", train=True, B=4)


def gen_f13():
    _gen_gradients("f13_train_gradients_b2.npz", train=False)


def gen_f13b():
    """F13b: F13 at the thinktwice.py size (B=1, 448x896, 65536 points): on full-size maps a flipped ReLU mask is a
    negligible share of a channel's gradient sum, so the HIP backward can be held to 1e-3 on the gradient norms.  Reference
    backward only (the oracle's own backward at this size would double the CPU time; F13 / F16 pin the oracle)."""
    _gen_gradients("f13b_train_gradients_fullsize_b1.npz", train=False, B=1, hw=(448, 896), npts=65536, with_oracle=False)


def _gen_gradients(fname, train, B=2, hw=(128, 256), npts=20000, with_oracle=True):
    """F13: BACKWARD of the training step.  The reference's own autograd graph (its custom VoxelPooling Function,
    the detach() / no_grad placements of lss.py:589,711 and thinktwice_decoder.py:429-430, `_parse_losses`) against
    autograd through the oracle restatement, model.eval(), B=2 128x256: gradient of the total loss w.r.t. every
    parameter.  Stored: per-parameter gradient norm, 8 sampled entries each, and the set of parameters that receive
    no gradient (the dead branches: they need find_unused_parameters in the reference's DDP, mmdet_train.py:72)."""
    from oracle import train_ref as TR
    from thinktwice_amd import config, params, synth
    seed = 0
    cfg = config.model_config(final_dim=hw)
    sd = params.init_params(cfg, seed=seed)
    batch = synth.make_batch(B, img_hw=hw, num_points=npts, jitter_calib=TRAIN_CALIB_JITTER if train else None)
    batch.update(synth.make_train_targets(B, img_hw=hw))
    import contextlib
    rng = 20240607
    sd_ref = _grad_leaves(sd)                      # leaves for the third-party stand-ins (they read `sd` directly)
    model = build_reference_model(cfg, sd_ref)
    mode = TR.train_mode if train else contextlib.nullcontext
    if train:
        model.train()
    with mode():                                   # (the third-party stand-ins call the oracle blocks: same switch)
        torch.manual_seed(rng)
        losses = model.forward_train(batch)
        loss_ref, _ = model._parse_losses(losses)
        loss_ref.backward()
    model.eval()
    own = dict(model.named_parameters())
    sd_ora = _grad_leaves(sd)
    if with_oracle:
        with mode():
            torch.manual_seed(rng)
            lo, _ = TR.forward_train(sd_ora, cfg, batch)
            loss_ora = TR.total_loss(lo)
            loss_ora.backward()
        print(f"total loss reference {float(loss_ref):.6f} oracle {float(loss_ora):.6f}")
    else:
        print(f"total loss reference {float(loss_ref):.6f}")
    g = torch.Generator().manual_seed(5)
    names, norms, samples, idxs, dead, worst, noise = [], [], [], [], [], 0.0, []
    for k, v in sd_ora.items():
        if not (torch.is_tensor(v) and v.requires_grad):
            continue
        gr = own[k].grad if k in own else sd_ref[k].grad
        go = v.grad if with_oracle else gr
        assert (gr is None) == (go is None), k
        if gr is None:
            dead.append(k)
            continue
        e = float((gr - go).norm() / gr.norm().clamp_min(1e-20))
        if train and e > 1e-3 and k.endswith(".bias") and float(gr.norm()) < 2e-3:
            # a conv bias in front of a batch-statistics BatchNorm: its gradient is analytically ZERO (the mean subtraction
            # removes it); what autograd returns is rounding noise of the two reduction terms, different in every
            # implementation.  Recorded by name; the tests bound its magnitude instead of comparing values.
            noise.append(k)
            print(f"  {k:70s} |g| {float(gr.norm()):.3e} (analytically zero: noise)")
        else:
            worst = max(worst, e)
            if e > 1e-4:
                print(f"  {k:70s} |g| {float(gr.norm()):.3e} rel err {e:.2e}")
        idx = torch.randint(0, gr.numel(), (8,), generator=g)
        names.append(k)
        norms.append(float(gr.norm()))
        idxs.append(idx.numpy())
        samples.append(gr.reshape(-1)[idx].numpy())
    print(f"{len(names)} parameters with gradient, {len(dead)} without, worst relative gradient error {worst:.2e}")
    assert worst < 1e-3, worst
    extra = {}
    if train:       # the loss terms too (F11 holds them for the no-grad forward; here from the run the gradients belong to)
        extra = {"loss__" + k: v.detach().float().numpy() for k, v in losses.items()}
        extra["rng"] = np.array([rng])
        extra["calib_jitter"] = np.array([TRAIN_CALIB_JITTER])
        extra["noise"] = np.array(noise)
    _save(fname, names=np.array(names), norms=np.array(norms), idx=np.stack(idxs),
          samples=np.stack(samples), dead=np.array(dead), total_loss=np.array([float(loss_ref)]),
          meta=np.array([B, hw[0], hw[1], npts, seed]), oracle_vs_reference_worst_rel_err=np.array([worst]), **extra)


# ---------------------------------------------------------------------------
# F15: pose matrices (leaderboard/team_code/thinktwice_agent.py:47-92) and the brake / throttle arbitration + stuck detector
#      (:463-509) of the closed-loop agent, produced by executing the reference's OWN definitions / statements (extracted
#      with ast at generation time: importing the module needs carla)
# ---------------------------------------------------------------------------
def gen_f15():
    import ast
    import math
    path = os.path.join(ref_stubs.REF_ROOT if hasattr(ref_stubs, "REF_ROOT") else "/root/reference", "leaderboard",
                        "team_code", "thinktwice_agent.py")
    tree = ast.parse(open(path).read())
    want = {"obtain_transform_matrix", "InverseRotateVector", "obtain_inv_transform_matrix"}
    mod = ast.Module(body=[n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in want], type_ignores=[])
    ns = {"math": math, "np": np}
    exec(compile(mod, path, "exec"), ns)
    rng = np.random.default_rng(15)
    poses = np.concatenate([rng.uniform(-200, 200, (24, 2)), rng.uniform(-2 * np.pi, 2 * np.pi, (24, 1))], 1)
    fwd = np.stack([ns["obtain_transform_matrix"](*p) for p in poses])
    inv = np.stack([ns["obtain_inv_transform_matrix"](*p) for p in poses])

    # --- the brake / throttle arbitration + stuck detector of a tick (thinktwice_agent.py:463-509).  It is not a function
    # in the reference but a run of statements inside `run_step` (after the `control_pid` call, inside `with
    # torch.no_grad()`); the statements are lifted out of the parsed tree unmodified and wrapped into a function whose
    # arguments are the names they read.  carla.VehicleControl is a plain attribute bag here (carla is not installed).
    def find_arbitration(tree):
        for cls in [n for n in tree.body if isinstance(n, ast.ClassDef)]:
            for fn in [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "run_step"]:
                for w in [n for n in ast.walk(fn) if isinstance(n, ast.With)]:
                    for i, st in enumerate(w.body):
                        if isinstance(st, ast.Assign) and isinstance(st.targets[0], ast.Tuple) and \
                                [getattr(e, "id", None) for e in st.targets[0].elts][:3] == ["steer_traj", "throttle_traj",
                                                                                              "brake_traj"]:
                            return w.body[i + 1:]
        raise SystemExit("arbitration block not found in thinktwice_agent.py")
    stmts = find_arbitration(tree)
    argn = ["self", "steer_ctrl", "throttle_ctrl", "brake_ctrl", "throttle_traj", "brake_traj", "gt_velocity", "tick_data"]
    fn = ast.FunctionDef(name="_arbitrate", args=ast.arguments(posonlyargs=[], args=[ast.arg(arg=a) for a in argn],
                                                               kwonlyargs=[], kw_defaults=[], defaults=[]),
                         body=list(stmts) + [ast.Return(value=ast.Name(id="control", ctx=ast.Load()))], decorator_list=[])
    amod = ast.fix_missing_locations(ast.Module(body=[fn], type_ignores=[]))

    class _Control:
        steer = throttle = brake = 0.0

    class _Carla:
        VehicleControl = _Control
    import contextlib
    import io
    import types
    ans = {"np": np, "carla": _Carla, "torch": torch}
    exec(compile(amod, path, "exec"), ans)
    agent = types.SimpleNamespace(stuck_detector=0, stuck_threshold=40, step=0)
    arng = np.random.default_rng(1515)
    arb_in, arb_out = [], []
    for t in range(400):
        speed = 0.0 if 100 <= t < 200 else float(arng.uniform(0, 6))        # a long standstill trips the stuck detector
        if t in (250, 251):
            speed = 0.5                                                      # neither branch of the detector update
        a = [float(arng.uniform(-0.3, 0.3)), float(arng.uniform(0, 1) * (arng.random() < 0.6)), float(arng.uniform(0, 1)),
             float(arng.uniform(0, 0.75) * (arng.random() < 0.7)), float(arng.integers(0, 2)), speed]
        agent.step = t
        with contextlib.redirect_stdout(io.StringIO()):
            c = ans["_arbitrate"](agent, a[0], a[1], a[2], a[3], a[4], torch.FloatTensor([speed]), {"speed": speed})
        arb_in.append(a)
        arb_out.append([float(c.steer), float(c.throttle), float(c.brake), float(agent.stuck_detector)])
    assert max(o[3] for o in arb_out) > 40, "the scripted sequence must trip the stuck detector"
    _save("f15_agent_transforms.npz", poses=poses, fwd=fwd, inv=inv, arb_in=np.asarray(arb_in), arb_out=np.asarray(arb_out),
          arb_stuck_threshold=np.array([40]))



# ---------------------------------------------------------------------------
# F17: the evaluation image pipeline (datasets/pipelines/transform.py): IDAImageTransform.__call__ :275-341 (undistortion
# grid_sample, per-camera img_transform :346-378 = T.Resize + crop, ida_mats) followed by ImageTransformMulti(aug=False)
# :154-156 (/255, Normalize :144).  The module is imported from where it lies; its third-party imports are stand-ins:
# torchvision Resize / Normalize / Compose (ref_stubs, documented torchvision-0.13 tensor semantics), the registries, and
# cv2.initUndistortRectifyMap -> thinktwice_amd.calib.undistort_rectify_map (OpenCV is not installed: the table itself is
# therefore the restated one, everything downstream of it is the reference's own code).
# ---------------------------------------------------------------------------
def gen_f17():
    import importlib.util
    import types
    from thinktwice_amd import calib
    ref_stubs.install()
    cv2 = sys.modules["cv2"]
    cv2.initUndistortRectifyMap = lambda mtx, dist, R, newmtx, size, m1type: calib.undistort_rectify_map(size[0], size[1])
    for name in ("matplotlib", "matplotlib.pyplot", "imgaug", "imgaug.augmenters", "mmcv.parallel", "mmdet.datasets",
                 "mmdet.datasets.builder", "mmdet.datasets.pipelines"):
        ref_stubs._mod(name)
    sys.modules["mmdet.datasets.builder"].PIPELINES = ref_stubs._Registry("pipelines")
    sys.modules["mmcv.parallel"].DataContainer = lambda x, **k: x
    sys.modules["mmdet.datasets.pipelines"].to_tensor = torch.as_tensor
    path = os.path.join(ref_stubs.OLT, "code", "datasets", "pipelines", "transform.py")
    spec = importlib.util.spec_from_file_location("ttref_transform", path)
    tr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tr)

    cfg = dict(img_size=(448, 896), camera_names=["rgb_front", "rgb_left", "rgb_right", "rgb_back"], undistort=True,
               unreal_coord=True, use_depth=False, use_seg=False, num_cams=4, queue_length=2)   # configs/thinktwice.py:41-120
    ida_aug_conf = {"resize_lim": (0.56, 0.6255), "final_dim": (448, 896), "rot_lim": (0, 0), "H": 900, "W": 1600,
                    "rand_flip": True, "bot_pct_lim": (0.0, 0.0)}                               # configs/thinktwice.py:111-119
    from thinktwice_amd import synth
    raw = synth.raw_camera_frames(seed=17)
    T_, N = raw.shape[:2]
    queue = [{"img": types.SimpleNamespace(data=raw[t]), "img_metas": types.SimpleNamespace(data={})} for t in range(T_)]
    with torch.no_grad():
        queue = tr.IDAImageTransform(cfg, ida_aug_conf, is_train=False)(queue)
        ida = torch.stack([q["img_metas"].data["ida_mats"] for q in queue]).numpy()            # [T, N, 4, 4]
        meta0 = queue[-1]["img_metas"].data
        queue = tr.ImageTransformMulti(aug=False, batch_size=1)(queue)
    out = torch.stack([q["img"] for q in queue]).numpy()                                        # [T, N, 3, 448, 896]
    assert out.shape == (T_, N, 3, 448, 896), out.shape
    rng = np.random.default_rng(1717)
    idx = rng.choice(out.size, size=16384, replace=False)
    _save("f17_image_pipeline.npz", seed=np.array([17]), sample_idx=idx.astype(np.int64), sample_val=out.reshape(-1)[idx],
          per_image_mean=out.mean(axis=(2, 3, 4)), per_image_abs_mean=np.abs(out).mean(axis=(2, 3, 4)),
          # one full row and one full column of every image of the key sweep: dense checks along both axes
          row_200=out[-1, :, :, 200, :], col_431=out[-1, :, :, :, 431],
          ida_mats=ida, cam_intrinsic=meta0["cam_intrinsic"].numpy(), lidar2img=meta0["lidar2img"].numpy(),
          lidar2cam=meta0["lidar2cam"].numpy())

def _json_config(v):
    """Config values -> JSON; tuples keep their type as {"__tuple__": [...]} (the model builder sees what the file wrote)."""
    if isinstance(v, dict):
        return {k: _json_config(x) for k, x in v.items()}
    if isinstance(v, tuple):
        return {"__tuple__": [_json_config(x) for x in v]}
    if isinstance(v, list):
        return [_json_config(x) for x in v]
    return v


def gen_cfg():
    """configs/thinktwice.py (with its _base_ files) as parsed by thinktwice_amd.cfgfile.Config.fromfile: the `model` and
    `optimizer` entries, stored as data for tests/test_host_logic.py."""
    import json
    from thinktwice_amd.cfgfile import Config
    cfg = Config.fromfile(os.path.join(ref_stubs.REF_ROOT, "open_loop_training", "configs", "thinktwice.py"))
    path = os.path.join(HERE, "reference_config.json")
    with open(path, "w") as f:
        json.dump({"model": _json_config(cfg.model), "optimizer": _json_config(cfg.optimizer)}, f, indent=1)
        f.write("\n")
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


FIXTURES = {"F17": gen_f17, "F3": gen_f3, "F12": gen_f12, "F7": gen_f7, "F8": gen_f8, "F9": gen_f9, "F10": gen_f10, "F11": gen_f11,
            "F13": gen_f13, "F13b": gen_f13b, "F14": gen_f14, "F15": gen_f15, "F16": gen_f16, "CFG": gen_cfg}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    if not ref_stubs.reference_available():
        raise SystemExit("needs /root/reference (build container only)")
    names = [n for n in args.only.split(",") if n] or list(FIXTURES)
    for n in names:
        print(f"== {n}")
        FIXTURES[n]()


if __name__ == "__main__":
    main()
