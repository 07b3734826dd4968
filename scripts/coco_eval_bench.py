"""Time metrics.CocoEvaluator beside the host numpy evaluation of the same tensors (DESIGN.md,
"COCO evaluation", measurements).

  python scripts/coco_eval_bench.py [--images 5000] [--windows 9] [--host-runs 3]

Workload: --images images x 100 detection slots, NC = 91, 16 ground-truth rows an image, 32
images per add; the detections are jittered ground truths plus false positives (the generator of
tests/test_coco_eval_gpu.py).  Device figures: the wall time of reset + every add + summarize
(which ends in the one host synchronisation), and, between two device events, the adds alone
(the match kernel) on the LDS-table route and with table_pairs = 0, where every image recomputes
its IoUs; the routes alternate window by window after 3 warm-up runs of each.  Host figure: the
test's numpy reference, including the device-to-host copies of the seven tensors it needs.  Each
figure is the median over its windows, with min and max."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import test_coco_eval_gpu as T  # noqa: E402
from tf2mv_amd.metrics import CocoEvaluator  # noqa: E402

NC, M, G, B = 91, 100, 16, 32


def show(name, v, unit="ms"):
    print(f"  {name}: median {np.median(v):9.3f} {unit}  (min {min(v):.3f}, max {max(v):.3f}; {len(v)} windows)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--host-runs", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs cuda:0"
    n = args.images
    per_add = [B] * (n // B) + ([n % B] if n % B else [])
    host = T.random_case(7, n, NC, M, G, per_add, 1, None, None, 1024, 3)
    dev = [tuple(torch.as_tensor(a).cuda() for a in b) for b in host]
    evs = {"table": CocoEvaluator(NC, M, n), "on the fly": CocoEvaluator(NC, M, n, table_pairs=0)}

    def run(ev, timed_adds=False):
        ev.reset()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for b in dev:
            ev.add(*b)
        e.record()
        out = ev.summarize()
        return (out, s.elapsed_time(e)) if timed_adds else out

    outs = {k: run(ev) for k, ev in evs.items()}
    assert torch.equal(evs["table"].tp, evs["on the fly"].tp), "the two routes disagree"
    for ev in evs.values():
        for _ in range(3):
            run(ev)
    wall, adds = {k: [] for k in evs}, {k: [] for k in evs}
    for _ in range(args.windows):
        for k, ev in evs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, a = run(ev, True)
            wall[k].append((time.perf_counter() - t0) * 1e3)
            adds[k].append(a)
    print(f"{n} images x {M} detections, NC = {NC}, G = {G}, {B} images per add ({len(per_add)} adds)")
    for k in evs:
        print(f"device, {k} route: AP {outs[k]['AP']:.6f}")
        show("reset + adds + summarize, wall", wall[k])
        show("adds alone (k_eval_match), device", adds[k])
        show("match share of the wall time", [100 * a / w for a, w in zip(adds[k], wall[k])], "%")
        show("k_eval_match per add", [1e3 * a / len(per_add) for a in adds[k]], "us")
    ht = []
    for _ in range(args.host_runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref = T.reference([tuple(a.cpu().numpy() for a in b) for b in dev], NC, M)
        ht.append((time.perf_counter() - t0) * 1e3)
    valid = ref["ap"] >= 0
    print(f"host numpy reference: AP {ref['ap'][valid].mean():.6f}")
    show("copies + evaluation, wall", ht)
    err = np.abs(outs["table"]["per_class_ap"].cpu().numpy() - ref["ap"]).max()
    print(f"max |AP[c,k] device - host| = {err:.3e}; host / device wall = {np.median(ht) / np.median(wall['table']):.1f}")


if __name__ == "__main__":
    main()
