"""The last stage of the reference's sample assembly, `union2one` (open_loop_training/code/datasets/carla_dataset.py:252-334):
the multi-sweep LiDAR cloud of a training batch on the device (tt_lidar_union_sweeps, csrc/lidar_union.hip) and the sweep metas
on the host.  Next to preprocess.TrainImagePipeline, with no edit to the model or the trainer:

    union = sweeps.SweepUnion(device="cuda")
    out = union(data["sweeps"], data["can_bus"])                # [B][T] raw (n, 4) clouds, [B][T][18] can_bus vectors
    metas = [sweeps.sweep_metas(cb, l2c, ps) for cb, l2c, ps in zip(data["can_bus"], data["lidar2cam"], out["points_size"])]
    sweeps.fill_sweeps(data, out, metas)                        # points, img_metas[b][t]["currlidar2keycam"], ...

What the reference does, quirks included, and this module restates:
  * every older sweep's cloud is moved into the key frame by the FULL 4x4 `curr2key` applied to (x, y, z, intensity): the
    intensity stands where the homogeneous coordinate would, so the translation is scaled by it (:323);
  * the key sweep comes first, the older sweeps follow going back in time, a fifth column carries 0, -1, -2, ... (:315-326);
  * in the rewritten can_bus the OLDEST frame of the queue is the one zeroed and marked prev_bev = False (:270-287);
  * a one-frame queue keeps its four-column cloud, because :327-328 sit inside the loop: `SweepUnion` refuses T == 1.

[3P] unpinned.  mmcv is not installed where this was written, so no fixture pins how its `collate` stacks the ragged clouds of a
batch: a DataContainer with stack=True, pad_dims=2, padding_value=0 is padded with zero ROWS at the end of the shorter samples,
which the voxeliser then treats as real points at the origin.  That convention lives in ONE place, `SweepUnion` and its `pad_to`;
a session that has mmcv can pin it by editing that class and nothing else."""
import numpy as np
import torch

from . import _lib, ops
from .ops import check, lib, ptr

UnionSweep = _lib.structs()["tt_union_sweep"]


# ------------------------------------------------------------------------------------------------------- host restatements
def ego_shift(dx, dy, yaw_deg):
    """get_ego_shift (carla_dataset.py:252-259), in float64 as there: (shift_x, shift_y)."""
    length = np.sqrt(dx ** 2 + dy ** 2)
    angle = np.arctan2(dy, dx) / np.pi * 180
    bev_angle = yaw_deg - angle
    return length * np.sin(bev_angle / 180 * np.pi), length * np.cos(bev_angle / 180 * np.pi)


def curr2key_matrix(key_can_bus, curr_can_bus):
    """The 4x4 f32 `curr2key` of carla_dataset.py:292-310 from the two frames' ORIGINAL can_bus vectors (entries 0, 1: the
    position, entry -2: the yaw in radians).  The trigonometry and get_ego_shift run in float64 and are rounded into the f32
    matrices R (rotation by key_yaw - curr_yaw) and T (translation by the shift), as torch.Tensor(...) / `T[0, 3] = ...` do
    there; `R @ T` is an f32 product.  Of its sixteen entries only the two translation entries involve arithmetic, and they
    are written out in closed form -- the two non-zero terms of the dot product:

        m[0, 3] = f32(f32(c * tx) + f32(s * ty))        m[1, 3] = f32(f32(-s * tx) + f32(c * ty))

    two rounded products and one rounded add, no fused multiply-add; every other entry is R's or exactly 0 / 1.  torch's own
    4x4 matmul may fuse or reorder, so the two entries agree with the reference within twice gamma_2 * (|c tx| + |s ty|)
    (tests/test_sweep_union_ref.py), the rest bit for bit.  This function is the single owner of that rounding."""
    key, cur = np.asarray(key_can_bus, dtype=np.float64), np.asarray(curr_can_bus, dtype=np.float64)
    sx, sy = ego_shift(key[0] - cur[0], key[1] - cur[1], key[-2] / np.pi * 180)
    angle = key[-2] - cur[-2]
    c, s = np.float32(np.cos(angle)), np.float32(np.sin(angle))
    tx, ty = np.float32(sx), np.float32(sy)
    m = np.eye(4, dtype=np.float32)
    m[0, 0], m[0, 1], m[1, 0], m[1, 1] = c, s, -s + np.float32(0), c          # (+ 0: the product's -0 * 1 + c * 0 is +0)
    m[0, 3] = np.float32(c * tx) + np.float32(s * ty)
    m[1, 3] = np.float32(-s * tx) + np.float32(c * ty)
    return m


def curr2key_matrices(can_bus):
    """[T, 4, 4] f32 of one queue's can_bus [T, 18]: identity for the key frame T - 1 (:290), curr2key_matrix for the rest."""
    can_bus = np.asarray(can_bus, dtype=np.float64)
    T = can_bus.shape[0]
    return np.stack([curr2key_matrix(can_bus[-1], can_bus[t]) for t in range(T - 1)] + [np.eye(4, dtype=np.float32)])


def sweep_metas(can_bus, lidar2cam, points_size):
    """The meta part of union2one for one queue: can_bus [T, 18] (float64, as get_data_info builds it), lidar2cam
    [T, N, 4, 4], points_size (the T point counts) -> a list of T dicts, oldest frame first:
      can_bus           float64 [18], rewritten as :270-287 do: entries 0..2 and -1 become the difference to the frame before;
                        the OLDEST frame's are zeroed and it alone has prev_bev = False
      prev_bev          bool
      curr2key          f32 [4, 4] tensor (identity for the key frame)
      currlidar2keycam  f32 [N, 4, 4] tensor, lidar2cam @ curr2key as an f32 product (:312); the key frame's is its lidar2cam
      points_size       the list, shared by all T as there"""
    can_bus = np.asarray(can_bus, dtype=np.float64)
    if can_bus.ndim != 2 or can_bus.shape[1] < 4:
        raise ValueError(f"can_bus must be [T, 18], got {can_bus.shape}")
    T = can_bus.shape[0]
    lidar2cam = np.asarray(lidar2cam, dtype=np.float32)
    if lidar2cam.ndim != 4 or lidar2cam.shape[0] != T or lidar2cam.shape[2:] != (4, 4):
        raise ValueError(f"lidar2cam must be [{T}, N, 4, 4], got {lidar2cam.shape}")
    points_size = [int(n) for n in points_size]
    if len(points_size) != T:
        raise ValueError(f"points_size must have {T} entries")
    mats = curr2key_matrices(can_bus)
    metas = []
    for t in range(T):
        cb = can_bus[t].copy()
        if t == 0:
            cb[:3] = 0
            cb[-1] = 0
        else:
            cb[:3] -= can_bus[t - 1, :3]
            cb[-1] -= can_bus[t - 1, -1]
        l2k = lidar2cam[t].copy() if t == T - 1 else np.matmul(lidar2cam[t], mats[t])
        metas.append({"can_bus": cb, "prev_bev": t > 0, "curr2key": torch.from_numpy(mats[t].copy()),
                      "currlidar2keycam": torch.from_numpy(np.ascontiguousarray(l2k)), "points_size": points_size})
    return metas


# ---------------------------------------------------------------------------------------------------------- device pipeline
class SweepUnion:
    """union2one's multi-sweep clouds of a whole batch in one launch, collated: `(sweeps, can_bus) -> points [B, 1, Np, 5]`.

    `pad_to`: the row count Np of every sample of the result; None = the batch's largest per-sample total.  The rows a sample
    does not fill are zero rows -- mmcv's `collate` convention ([3P] unpinned, see the module docstring); this class and
    `pad_to` are its one owner."""

    def __init__(self, device="cuda", pad_to=None):
        self.device = torch.device(device)
        if pad_to is not None and (isinstance(pad_to, bool) or int(pad_to) != pad_to or pad_to < 0):
            raise ValueError(f"pad_to must be a non-negative integer or None, got {pad_to!r}")
        self.pad_to = None if pad_to is None else int(pad_to)

    def __call__(self, sweeps, can_bus=None, curr2key=None):
        """sweeps[b][t]: (n, 4) f32 (x, y, z, intensity), numpy array or torch tensor, on the host or on the device, oldest
        frame first, the same T >= 2 for every sample.  can_bus [B][T][18]: the frames' original can_bus vectors; `curr2key`
        ([B, T, 4, 4] f32, the key frame's entry unused) overrides it.  Whatever lives on the host goes up as ONE pinned
        copy; sweeps already on the device are joined behind it by one device concatenation.  Returns dict(points
        [B, 1, Np, 5] f32 on the device, curr2key [B, T, 4, 4] f32 on the host, points_size [B][T])."""
        B = len(sweeps)
        if B == 0:
            raise ValueError("sweeps is empty")
        T = len(sweeps[0])
        if any(len(s) != T for s in sweeps):
            raise ValueError("every sample needs the same number of sweeps")
        if T == 1:
            raise ValueError("T == 1: the reference leaves a one-frame queue its four-column cloud (carla_dataset.py:327-328 "
                             "sit inside the loop over the older sweeps), so there is nothing to build")
        if B * T > _lib.TT_UNION_MAX_SWEEPS:
            raise ValueError(f"{B} x {T} sweeps in one call: at most {_lib.TT_UNION_MAX_SWEEPS}")
        if curr2key is None:
            if can_bus is None:
                raise ValueError("need `can_bus` or `curr2key`")
            if len(can_bus) != B or any(len(c) != T for c in can_bus):
                raise ValueError(f"can_bus must be [{B}][{T}][18]")
            mats = np.stack([curr2key_matrices(c) for c in can_bus])
        else:
            mats = np.ascontiguousarray(torch.as_tensor(curr2key).cpu().numpy() if isinstance(curr2key, torch.Tensor)
                                        else curr2key, dtype=np.float32)
            if mats.shape != (B, T, 4, 4):
                raise ValueError(f"curr2key must be [{B}, {T}, 4, 4], got {mats.shape}")

        flat = []
        for b, sample in enumerate(sweeps):
            for t, s in enumerate(sample):
                s = torch.from_numpy(s) if isinstance(s, np.ndarray) else s
                if not isinstance(s, torch.Tensor) or s.dtype != torch.float32 or s.dim() != 2 or s.shape[1] != 4:
                    raise ValueError(f"sample {b} sweep {t}: need an (n, 4) float32 array or tensor")
                flat.append(s)
        sizes = [[int(flat[b * T + t].shape[0]) for t in range(T)] for b in range(B)]
        most = max(sum(s) for s in sizes)
        Np = most if self.pad_to is None else self.pad_to
        if Np < most:
            raise ValueError(f"pad_to = {Np}, but a sample of the batch has {most} points")

        # one buffer: [the host sweeps, uploaded as one pinned copy | the device sweeps], in the order they came
        on_host = [i for i, s in enumerate(flat) if not s.is_cuda]
        first, row = [0] * len(flat), 0
        for i in on_host + [i for i, s in enumerate(flat) if s.is_cuda]:
            first[i], row = row, row + int(flat[i].shape[0])
        parts = []
        if on_host:
            n_host = sum(int(flat[i].shape[0]) for i in on_host)
            staged = torch.empty(n_host, 4, dtype=torch.float32, pin_memory=True)
            for i in on_host:
                staged[first[i]:first[i] + flat[i].shape[0]] = flat[i]
            parts.append(staged.to(self.device, non_blocking=True))
        parts += [flat[i] for i in range(len(flat)) if flat[i].is_cuda]
        pts = parts[0] if len(parts) == 1 else torch.cat(parts)
        pts = pts.contiguous()
        device = pts.device

        table = (UnionSweep * (B * T))()
        for i in range(B * T):
            table[i].first_row, table[i].count = first[i], int(flat[i].shape[0])
            table[i].m[:] = mats[i // T, i % T].ravel().tolist()
        out = torch.empty(B, 1, Np, 5, dtype=torch.float32, device=device)
        with torch.cuda.device(device):
            check(lib().tt_lidar_union_sweeps(ptr(pts) if row else None, row, table, B, T, Np, ptr(out), ops.cur_stream(device)),
                  "tt_lidar_union_sweeps")
        return {"points": out, "curr2key": torch.from_numpy(mats.copy()), "points_size": sizes}


def fill_sweeps(data, out, metas):
    """Hand a SweepUnion result and the batch's sweep metas ([B] lists from sweep_metas) to a `forward_train` batch: `points`
    and, in every img_metas[b][t], can_bus, prev_bev, curr2key, currlidar2keycam and points_size (what union2one leaves in
    the queue).  The counterpart of preprocess.fill_batch; keys it does not name (ida_mats, cam_intrinsic, ...) are untouched."""
    if out["points"].dim() != 4 or out["points"].shape[1] != 1 or out["points"].shape[3] != 5:
        raise ValueError("fill_sweeps takes the [B, 1, Np, 5] form of `points`")
    B = out["points"].shape[0]
    if len(data["img_metas"]) != B or len(metas) != B:
        raise ValueError(f"img_metas and metas must have {B} samples")
    for per_sweep, new in zip(data["img_metas"], metas):
        if len(per_sweep) != len(new):
            raise ValueError("img_metas and metas differ in the number of sweeps")
    data["points"] = out["points"]
    for per_sweep, new in zip(data["img_metas"], metas):
        for meta, m in zip(per_sweep, new):
            for k in ("can_bus", "prev_bev", "curr2key", "currlidar2keycam", "points_size"):
                meta[k] = m[k]
    return data
