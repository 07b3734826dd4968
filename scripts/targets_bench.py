"""Timing of target assignment ("Force-match target assignment"): D0 at 512x512,
B = 32 and B = 1, G = 8 and G = 100 synthetic ground truths an image.

  python scripts/targets_bench.py [--out FILE]
  EDET_LIB=tensorflow2-machine-vision_amd/lib/libedet_dev.so python scripts/targets_bench.py --ap 1,2,4

Variants: edet_generate_targets (k_targets, the legacy kernel) and edet_generate_targets_matched
with force_match 0 and 1.  --ap (development library only) adds every variant of the new entry
point with the pair pass pinned to that many anchors per thread (development slot 62); without it
the planner's rule chooses.  Device events around `--calls` back-to-back calls per window, the
variants alternating window by window in one process after a warm-up; prints the median, the
minimum and the maximum of the windows in microseconds per call, one JSON line per workload.  The
force_match = 0 outputs are compared with the legacy kernel's, bit for bit, at every workload."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tf2mv_amd import _lib as L  # noqa: E402
from tf2mv_amd.anchors import Anchors, Targets  # noqa: E402
from tf2mv_amd.config import get_efficientdet_config  # noqa: E402
from tf2mv_amd.runtime import stream, vp  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ap", default="", help="comma-separated anchors per thread to pin (development library)")
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs cuda:0"
    dev = torch.device("cuda", 0)
    cfg = get_efficientdet_config("efficientdet-d0", {})
    S, A = cfg.image_size, 9
    an = Anchors(cfg.min_level, cfg.max_level, (S, S), cfg.num_scales, cfg.aspect_ratios, cfg.anchor_scale, device=dev)
    pins = [0] + [int(v) for v in args.ap.split(",") if v]
    lines = []
    loads = [(32, 8), (32, 100), (1, 8), (1, 100)]
    if len(pins) > 1:
        loads += [(8, 8), (8, 100)]  # the sweep alone: a block count between the two batch sizes
    for B, G in loads:
        rng = np.random.default_rng(B * 1000 + G)
        size = np.exp(rng.uniform(np.log(8), np.log(360), (B, G, 1)))
        hw = size * np.sqrt(rng.uniform(0.5, 2.0, (B, G, 1))) ** np.array([1.0, -1.0])
        c = rng.uniform(0, S, (B, G, 2))
        gt = torch.tensor(np.concatenate([c - hw / 2, c + hw / 2], -1), dtype=torch.float32, device=dev)
        gc = torch.tensor(rng.integers(1, 91, (B, G)), dtype=torch.int32, device=dev)
        ng = torch.full((B,), G, dtype=torch.int32, device=dev)
        pyr = an.pyramid(B)
        t0, t1 = Targets(pyr, A, dev), Targets(pyr, A, dev)
        for t in (t0, t1):
            t.box.zero_(), t.cls.zero_(), t.mask.zero_()
        best = torch.empty((B, G), dtype=torch.int64, device=dev)
        ga = torch.empty((B, G), dtype=torch.int32, device=dev)
        head = (vp(an.flat), pyr.c, A, vp(gt), vp(gc), vp(ng), G, 0.5)

        def legacy():
            L.call("edet_generate_targets", *head, vp(t0.box), vp(t0.cls), vp(t0.mask), stream())

        def matched(force):
            def run():
                L.call("edet_generate_targets_matched", *head, vp(t1.box), vp(t1.cls), vp(t1.mask), force, vp(best),
                       vp(ga), stream())
            return run

        variants = {"legacy": (0, legacy)}
        for pin in pins:
            for force in (0, 1):
                variants[f"matched force={force} ap={pin or 'rule'}"] = (pin, matched(force))

        def select(pin):
            if len(pins) > 1:
                L.call("edet_dev_set", 62, pin)

        legacy()
        for name, (pin, fn) in variants.items():  # warm-up, and results that must not change
            select(pin)
            for _ in range(20):
                fn()
            if "force=0" in name:
                assert torch.equal(t0.box, t1.box) and torch.equal(t0.cls, t1.cls) and torch.equal(t0.mask, t1.mask), name
        times = {name: [] for name in variants}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.windows):
            for name, (pin, fn) in variants.items():
                select(pin)
                e0.record()
                for _ in range(args.calls):
                    fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / args.calls)
        forced = int((ga >= 0).sum())
        res = {"B": B, "G": G, "anchors": int(an.flat.shape[0]), "forced": forced, "positives": int(t1.mask.sum()),
               "us": {k: [round(float(np.median(v)), 2), round(min(v), 2), round(max(v), 2)] for k, v in times.items()}}
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
