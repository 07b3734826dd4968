"""Time Anchors.detect_per_class(select="topk") with nms="soft" beside nms="hard" on the same
inputs in one process ("Per-class detection", Soft-NMS measurements).

  python scripts/softnms_bench.py [--reps 100] [--windows 9]

Two workloads: the logits and regressions of a randomly initialised bf16 D0 (512x512, NC = 81,
B = 32) at score_threshold 0.05, and the worst case for the per-image block, a 128x128
pyramid (levels 3-7, NC = 5, B = 2, fp32) whose candidates all sit in one class.  Each figure
is the median over --windows windows of --reps back-to-back public calls between two device
events, the two modes alternating window by window, after 10 warm-up calls of each."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tf2mv_amd.anchors import Anchors  # noqa: E402
from tf2mv_amd.config import efficientnet_b0_blocks, get_efficientdet_config  # noqa: E402
from tf2mv_amd.model import EfficientDetNet  # noqa: E402


def measure(name, an, bl, cl, reps, windows):
    run = {nms: (lambda nms=nms: an.detect_per_class(bl, cl, 100, 0.5, 0.05, "iou", select="topk", nms=nms))
           for nms in ("hard", "soft")}
    out = {nms: fn() for nms, fn in run.items()}
    print(f"{name}: candidates per image min {int(out['soft'][4].min())} max {int(out['soft'][4].max())}, "
          f"kept hard {int(out['hard'][3].sum())} soft {int(out['soft'][3].sum())}")
    for fn in run.values():
        for _ in range(10):
            fn()
    us = {nms: [] for nms in run}
    for _ in range(windows):
        for nms, fn in run.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                fn()
            e.record()
            torch.cuda.synchronize()
            us[nms].append(s.elapsed_time(e) * 1e3 / reps)
    for nms, v in us.items():
        print(f"  {nms}: median {np.median(v):8.1f} us  (min {min(v):.1f}, max {max(v):.1f}; {reps} calls x {windows})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=9)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs cuda:0"
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)

    cfg = get_efficientdet_config("efficientdet-d0", {"num_classes": 81})
    S, B = cfg.image_size, 32
    an = Anchors(cfg.min_level, cfg.max_level, (S, S), cfg.num_scales, cfg.aspect_ratios, cfg.anchor_scale, device=dev)
    model = EfficientDetNet(efficientnet_b0_blocks(), cfg, dtype="bf16")
    bl, cl = model(torch.rand(B, S, S, 3, device=dev, generator=g))
    measure(f"D0 {S}x{S} NC=81 bf16 B={B}, random initialisation", an, bl, cl, args.reps, args.windows)
    # (that head's bias puts every score near 0.01: no candidates.)  The same shapes with logits
    # N(-6.43, 1), about 1 000 candidates per image (scripts/kbench.py --detect)
    pyr, A = an.pyramid(B), model.A
    rel = (0.3 * torch.randn(pyr.rows, A * 4, device=dev, generator=g)).bfloat16()
    lg = (torch.randn(pyr.rows, A * 81, device=dev, generator=g) - 6.43).bfloat16()
    bl = tuple(rel[pyr.seg_slice(s)].view(B, h, w, A, 4) for s, (h, w) in enumerate(an.level_sizes))
    cl = tuple(lg[pyr.seg_slice(s)].view(B, h, w, A, 81) for s, (h, w) in enumerate(an.level_sizes))
    measure(f"D0 {S}x{S} NC=81 bf16 B={B}, logits N(-6.43, 1)", an, bl, cl, args.reps, args.windows)

    A, NC, B = 9, 5, 2
    an = Anchors(3, 7, (128, 128), 3, [(1.0, 1.0), (1.4, 0.7), (0.7, 1.4)], 4.0, device=dev)
    pyr = an.pyramid(B)
    rel = 0.3 * torch.randn(pyr.rows, A * 4, device=dev, generator=g)
    lg = torch.full((pyr.rows, A, NC), -20.0, device=dev)
    lg[:, :, 2] = 2.0 * torch.randn(pyr.rows, A, device=dev, generator=g) - 0.75
    lg = lg.view(pyr.rows, A * NC)
    bl = tuple(rel[pyr.seg_slice(s)].view(B, h, w, A, 4) for s, (h, w) in enumerate(an.level_sizes))
    cl = tuple(lg[pyr.seg_slice(s)].view(B, h, w, A, NC) for s, (h, w) in enumerate(an.level_sizes))
    measure("one class, 128x128 NC=5 fp32 B=2", an, bl, cl, args.reps, args.windows)


if __name__ == "__main__":
    main()
