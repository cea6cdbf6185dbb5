"""TEST INFRASTRUCTURE: the reference's training image pipeline restated with torch CPU ops -- IDAImageTransform(is_train=True)
(datasets/pipelines/transform.py:275-341: undistortion `grid_sample` through the [-1, 1]-normalised map, per camera
T.Resize = F.interpolate(bilinear, align_corners=False), crop, flip; depth_transform :386-396 the same for the label maps) +
ImageTransformMulti(aug=False) (:144,163).  PINNED by golden F18 (tests/golden/gen_f18_train_pipeline.py runs the
reference's own module; tests/test_train_image_pipeline.py holds this file to it)."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from thinktwice_amd import calib


def _grid(mapx, mapy, n):
    H, W = mapx.shape
    gx = (torch.as_tensor(mapx) - W / 2) / (W / 2)
    gy = (torch.as_tensor(mapy) - H / 2) / (H / 2)
    return torch.stack([gx, gy], -1).unsqueeze(0).repeat(n, 1, 1, 1)


def _ida(x, p, final_dim):
    """x [K, C, H, W] of one camera -> resize, crop, flip with that camera's draw."""
    fh, fw = final_dim
    x = F.interpolate(x, size=(p.resized_h, p.resized_w), mode="bilinear", align_corners=False)
    x = x[..., p.crop_y:p.crop_y + fh, p.crop_x:p.crop_x + fw]
    return torch.flip(x, dims=[-1]) if p.flip else x


def restate(raw, params, mapx, mapy, depth=None, seg=None, final_dim=(calib.FINAL_H, calib.FINAL_W)):
    """One sample.  raw uint8 [T, N, H, W, 3], depth / seg f32 [N, H, W] (numpy or torch), params: N IdaParams;
    mapx = mapy = None: no undistortion.  Returns dict(img [T, N, 3, fh, fw], depth / seg [N, fh, fw]) of f32 tensors."""
    raw = torch.as_tensor(raw)
    T, N, H, W, _ = raw.shape
    with torch.no_grad():
        img = raw.to(torch.float32).view(-1, H, W, 3).permute(0, 3, 1, 2)
        if mapx is not None:
            img = F.grid_sample(img, _grid(mapx, mapy, T * N), align_corners=False)
        img = img.view(T, N, 3, H, W)
        res = torch.stack([_ida(img[:, n], params[n], final_dim) for n in range(N)], 1)         # [T, N, 3, fh, fw]
        mean = torch.tensor(calib.IMAGENET_MEAN).view(1, 1, 3, 1, 1)
        std = torch.tensor(calib.IMAGENET_STD).view(1, 1, 3, 1, 1)
        out = {"img": (res / 255.0 - mean) / std}
        for name, lab in (("depth", depth), ("seg", seg)):
            if lab is not None:
                lab = torch.as_tensor(lab).to(torch.float32).view(N, 1, H, W)
                if mapx is not None:
                    lab = F.grid_sample(lab, _grid(mapx, mapy, N), align_corners=False)
                out[name] = torch.stack([_ida(lab[n:n + 1], params[n], final_dim)[0, 0] for n in range(N)])
    return out


def f18():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f18_train_image_pipeline.npz"))


def f18_params():
    """The four draws golden F18 logged, as IdaParams."""
    from thinktwice_amd.preprocess import IdaParams
    return [IdaParams(float(r[0]), int(r[1]), int(r[2]), int(r[3]), int(r[4]), bool(r[5])) for r in f18()["params"]]


@functools.lru_cache(maxsize=1)
def seed18():
    """Inputs of golden F18 and their restatement, computed once per test process and left unchanged:
    (raw [2, 4, 900, 1600, 3] uint8, depth, seg [4, 900, 1600] f32, params, restate(...))."""
    from thinktwice_amd import synth
    raw = synth.raw_camera_frames(seed=18)
    depth, seg = synth.raw_label_maps(seed=18)
    mx, my = calib.undistort_rectify_map()
    params = f18_params()
    return raw, depth, seg, params, restate(raw, params, mx, my, depth, seg)


def errors_against_f18(img, depth, seg):
    """{kind: (max, mean)} absolute errors of f32 arrays img [2, 4, 3, 448, 896], depth / seg [4, 448, 896] against the
    reference pipeline's own outputs (sampled values, one full row and column of the key sweep / of each label map), and
    the worst per-image mean difference as `<kind>_image_mean`."""
    g = f18()
    errs = {"img": [np.abs(img.reshape(-1)[g["sample_idx"]] - g["sample_val"]), np.abs(img[-1, :, :, 200, :] - g["row_200"]),
                    np.abs(img[-1, :, :, :, 431] - g["col_431"])]}
    means = {"img_image_mean": float(np.abs(img.mean(axis=(2, 3, 4)) - g["per_image_mean"]).max())}
    for name, m in (("depth", depth), ("seg", seg)):
        errs[name] = [np.abs(m.reshape(-1)[g["label_idx"]] - g[f"{name}_val"]), np.abs(m[:, 200, :] - g[f"{name}_row_200"]),
                      np.abs(m[:, :, 431] - g[f"{name}_col_431"])]
        means[f"{name}_image_mean"] = float(np.abs(m.mean(axis=(1, 2)) - g[f"{name}_mean"]).max())
    out = {k: (max(float(e.max()) for e in v), max(float(e.mean()) for e in v)) for k, v in errs.items()}
    out.update(means)
    return out
