"""Which inference-only form a layer takes, as the caller-side predicates of thinktwice_amd/ops.py answer from plain numbers:
pair_ok, up2_ok, join_ok, stem_pool_ok, res1_up_ok and auto_splitk_asks, with every knob on, no tape and eval-mode BatchNorm.

  grid   both sides of every threshold: rows 2,048 ... 1,605,632 x cin 16 ... 2,048 x cout (9, 12, 18 and 20 among them) x k 1 / 3
         for pair_ok, and a grid of its own for each of the others;
  sites  the numbers every call site of thinktwice_amd/lss.py asks with at B = 1, 2 and 8 under the reference config
         (config.MODEL: image size, cameras, sweeps; the ResNet-50 / PAFPN / DepthNet / UNet strides and widths), printed by --sites.

Pure Python on the host: no device, and where a predicate asks the library it is tt_conv2d_plan (host only).  --out FILE writes
{"cases": [[predicate, [arguments], answer, site or null]]}.  tests/route_cases.json is this tool's output at the commit before the
predicates began to ask the library (they restated its contracts then, and the PAFPN site spelled `rows > 4096` itself);
tests/test_routes.py replays it.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

ROWS = (2048, 4096, 4097, 8192, 16384, 32767, 32768, 65536, 200704, 1605632)
CIN = (16, 32, 48, 64, 128, 512, 1024, 2048)
COUT = (4, 8, 9, 12, 16, 18, 20, 32, 48, 64, 96, 128, 256, 512)


def ask(fn, args):
    """The predicate's answer from plain numbers (stem_pool_ok: (B, T, N, H, W) of an f32 image that is never allocated)."""
    import torch
    from thinktwice_amd import ops
    if fn == "stem_pool_ok":
        B, T, N, H, W = args
        return bool(ops.stem_pool_ok(torch.empty(B, T, N, 3, H, W, device="meta"), torch.empty(64, 7, 1, 32, device="meta")))
    return bool(getattr(ops, fn)(*args))


def grid():
    out = [("pair_ok", [r, ci, co, k * k]) for r in ROWS for ci in CIN for co in COUT for k in (1, 3)]
    # (the rows of an upsampled map: multiples of 4)
    out += [("up2_ok", [(r + 3) // 4 * 4, ci, co]) for r in ROWS for ci in (16, 32, 48, 64, 128) for co in (32, 48, 64, 128)]
    out += [("join_ok", [r, k1, m * k1, n2]) for r in ROWS + (4551, 50176, 100352) for k1 in (32, 64, 128, 256, 512) for m in (2, 4)
            for n2 in (32, 64, 128, 256, 512)]
    out += [("stem_pool_ok", [1, 1, n, h, w]) for n in (1, 2) for h, w in ((64, 128), (128, 128), (128, 130), (64, 96), (63, 96), (448, 896))]
    out += [("res1_up_ok", [r]) for r in ROWS]
    out += [("auto_splitk_asks", [r, k]) for r in ROWS + (3136,) for k in (1024, 2032, 2048, 4608)]
    return [(fn, args, None) for fn, args in out]


def sites(B):
    """(predicate, arguments, site) of every routing question one forward of the reference model asks at batch size B."""
    from thinktwice_amd import config
    enc = config.MODEL["img_encoder"]
    H, W = enc["final_dim"]
    NI = B * enc["queue_len"] * config.MODEL["num_cams"]
    out = [("stem_pool_ok", [B, enc["queue_len"], config.MODEL["num_cams"], H, W], "stem")]
    blocks = [(li, b, 64 << li, 2 if (b == 0 and li > 0) else 1) for li, nb in enumerate((3, 4, 6, 3)) for b in range(nb)]
    h, w = H // 4, W // 4                   # the max-pooled stem output
    for i, (li, b, width, s) in enumerate(blocks):
        name = f"layer{li + 1}.{b}"
        rows_in, rows = NI * h * w, NI * (h // s) * (w // s)
        h, w = h // s, w // s
        out.append(("pair_ok", [rows, width, width, 9], name + ".conv2 in_pair"))
        for conv, r, k in (("conv1", rows_in, 4 * width if b else (2 * width if li else 64)), ("conv2", rows, 9 * width), ("conv3", rows, width)):
            out.append(("auto_splitk_asks", [r, k], f"{name}.{conv}"))
        if i + 1 < len(blocks):
            out.append(("join_ok", [rows, width, 4 * width, blocks[i + 1][2]], name + ".conv3 + next conv1"))
    for lvl in range(3):
        out.append(("res1_up_ok", [NI * (H >> (2 + lvl)) * (W >> (2 + lvl))], f"PAFPN lateral {lvl}"))
    mid = enc["depth_net_conf"]["mid_channels"]
    rows = NI * (H // enc["downsample_factor"]) * (W // enc["downsample_factor"])
    out += [("pair_ok", [rows, mid, mid, 9], "depth_conv blocks"), ("pair_ok", [rows, 4 * mid, mid, 1], "ASPP concat"),
            ("auto_splitk_asks", [rows, 9 * mid], "depth_conv blocks"), ("auto_splitk_asks", [rows, 4 * mid], "ASPP conv1")]
    rows = NI * (H // 2) * (W // 2)
    out += [("pair_ok", [rows, 128, 64, 9], "unet_layer0.1 in_pair"), ("up2_ok", [rows, 128, 64], "unet_layer0.1 in_up2"),
            ("pair_ok", [rows, 64, enc["seg_net_conf"]["out_channels"], 9], "seg head in_pair")]
    return [(fn, args, f"B={B} {site}") for fn, args, site in out]


def cases():
    from thinktwice_amd import autodiff, layers, ops
    assert autodiff.TAPE is None and not layers.BN_TRAIN
    assert ops.PAIR and ops.BNECK_JOIN and ops.SEG_UP2 and ops.STEM_POOL and ops._AUTO_SPLITK, "record with every knob at its default"
    return [[fn, args, ask(fn, args), site] for fn, args, site in grid() + sites(1) + sites(2) + sites(8)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sites", action="store_true", help="print the call sites' questions and answers")
    ap.add_argument("--out")
    a = ap.parse_args()
    rows = cases()
    if a.sites:
        for fn, args, ans, site in rows:
            if site:
                print(f"{site:40s} {fn}({', '.join(map(str, args))}) -> {ans}")
    if a.out:
        lines = [", ".join(json.dumps(c, separators=(",", ":")) for c in rows[i:i + 4]) for i in range(0, len(rows), 4)]
        open(a.out, "w").write("{\"cases\": [\n" + ",\n".join(lines) + "\n]}\n")
    print(f"{len(rows)} cases, {sum(c[2] for c in rows)} yes, {sum(c[3] is not None for c in rows)} at call sites", file=sys.stderr)


if __name__ == "__main__":
    main()
