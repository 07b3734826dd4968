"""Workload for timing the box branch of the fused loss ("IoU-family box loss"): D0 at
512x512, B = 32, bf16, ldb = 40, targets from Anchors.generate_targets_batched over 8 synthetic
ground-truth boxes an image, the gradient written in place as in the training step.

  rocprofv3 --kernel-trace --stats -d OUT -- python scripts/box_iou_bench.py --mode plain|iou [--kind ciou]

  plain  edet_detection_loss with NC = 1: k_loss, whose box blocks are the Huber-only yardstick
  iou    edet_detection_loss_iou with NC = 1: k_loss over its class blocks alone, then k_box_iou
NC = 1 keeps the class blocks small, and k_loss(plain) - k_loss(iou) is the box blocks' share.
Prints the positive fraction; the kernel times are the profiler's."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tf2mv_amd import _lib as L  # noqa: E402
from tf2mv_amd.anchors import Anchors  # noqa: E402
from tf2mv_amd.config import get_efficientdet_config  # noqa: E402
from tf2mv_amd.runtime import stream, vp  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["plain", "iou"], required=True)
    ap.add_argument("--kind", default="ciou", choices=list(L.IOU_LOSS))
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs cuda:0"
    dev = torch.device("cuda", 0)
    cfg = get_efficientdet_config("efficientdet-d0", {})
    S, B, G, A, NC, ldb, ldc = cfg.image_size, 32, 8, 9, 1, 40, 16
    an = Anchors(cfg.min_level, cfg.max_level, (S, S), cfg.num_scales, cfg.aspect_ratios, cfg.anchor_scale, device=dev)
    rng = np.random.default_rng(0)
    size = np.exp(rng.uniform(np.log(24), np.log(360), (B, G, 1)))
    hw = size * np.sqrt(rng.uniform(0.5, 2.0, (B, G, 1))) ** np.array([1.0, -1.0])
    c = rng.uniform(0, S, (B, G, 2))
    gt = torch.tensor(np.concatenate([c - hw / 2, c + hw / 2], -1), dtype=torch.float32)
    t = an.generate_targets_batched(gt, torch.ones(B, G, dtype=torch.int32), torch.full((B,), G, dtype=torch.int32))
    pyr = t.pyr
    npos = t.mask.sum().float().reshape(1)
    print(f"positives {int(npos)} of {pyr.rows * A} anchors: {float(npos) / (pyr.rows * A):.4%}")
    gen = torch.Generator(device=dev).manual_seed(0)
    box0 = (t.box.view(pyr.rows, A * 4) + 0.2 * torch.randn(pyr.rows, A * 4, device=dev, generator=gen))
    box0 = torch.nn.functional.pad(box0, (0, ldb - A * 4)).bfloat16()
    cls0 = torch.randn(pyr.rows, ldc, device=dev, generator=gen).bfloat16()
    box, cls = box0.clone(), cls0.clone()
    acc, parts, iparts = (torch.zeros(n, dtype=torch.float32, device=dev) for n in (1, 2 * L.MAX_SEG, L.MAX_SEG))
    head = (L.BF16, vp(cls), ldc, vp(box), ldb, pyr.c, A, NC, vp(t.cls), vp(t.box), vp(npos), 0.25, 1.5, 0.1, 50.0, 1.0,
            vp(cls), vp(box), vp(acc), vp(parts))
    for _ in range(args.calls):
        box.copy_(box0)
        cls.copy_(cls0)
        if args.mode == "plain":
            L.call("edet_detection_loss", *head, stream())
        else:
            L.call("edet_detection_loss_iou", *head, vp(an.flat), vp(t.mask), L.IOU_LOSS[args.kind], 1.0, vp(iparts), stream())
    torch.cuda.synchronize()
    print(f"{args.mode}: {args.calls} calls, loss {float(acc) / args.calls:.6f}, iou term {float(iparts.sum()) / args.calls:.6f}")


if __name__ == "__main__":
    main()
