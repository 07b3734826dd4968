"""Anchors.detect_per_class(nms="soft") (edet_detect_per_class_soft, k_softnms_pc): per-class
Gaussian Soft-NMS against a plain fp64 numpy loop of the semantics in include/edet.h, over the
boxes Anchors.convert_outputs_boxes decodes and the logits as stored.

Identities are compared exactly.  Both sides hold the scores in fp64 with the same op order, so
only exp differs: <= 1 ulp on either side plus <= 1 ulp of the product's rounding, <= 3 ulp =
6.7e-16 relative per decay, <= 7e-14 after max_out = 100 decays.  The reference reports the
smallest relative gap between a pick and its runner-up (exact ties apart) and of a tested score
from min_score; the seeds keep both >= 1e-9, four orders above that bound.  Both sides round an
emitted score to fp32 once (rtol 2^-23), and the seeds keep the outputs and the first emission
behind them, where their fp64 scores differ, more than 2 fp32 ulps apart.

Logits are N(mu - 0.75 ((c - 1) % 4), 2) for class c: in "base" the classes hold about 380, 190,
90 and 35 candidates, on both sides of the kernel's 256-candidate switch from a wave to the
block.  Checked once with the reference on the CPU: in "base" and "drop" hard NMS at 0.5 differs."""
import ctypes

import numpy as np
import pytest
import torch

from test_detect_per_class_gpu import ASPECTS
from tf2mv_amd import _lib

A = 9
# name, dtype, NC, B, score_threshold, sigma, max_candidates, max_output_size, select, mu, seed
CASES = [
    ("base", "f32", 5, 2, 0.05, 0.5, 4096, 100, "first", -5.25, 0),
    ("bf16", "bf16", 5, 2, 0.05, 0.5, 4096, 100, "first", -5.25, 0),
    ("nodrop", "f32", 5, 2, 0.0, 0.5, 4096, 20, "first", -5.25, 0),  # first-K overflow; classes stop at 20 picks
    ("one-class", "f32", 5, 2, 0.05, 0.5, 4096, 100, "first", 0.0, 0),  # > 1024 in class 2: the whole-block route
    ("drop", "f32", 5, 3, 0.3, 0.1, 4096, 100, "first", -2.0, 0),  # heavy dropping; image 1 is empty
    ("topk", "f32", 81, 2, 0.0, 0.5, 4096, 100, "topk", -5.25, 0),  # ~245 k candidates, 80 classes in 128 KiB of LDS
    ("hand", "f32", 5, 1, 0.05, 0.5, 4096, 100, "first", 0.0, 0),  # exact ties: lower anchor, then lower class
]


def build(name, pyr, level_sizes, NC, mu, rng):
    """The pyramid buffers [rows, ld] of regressions and logits (fp64 values, cast by the caller)."""
    cls_of = np.arange(A * NC + 7) % NC  # (the 7 pad columns are never read)
    rel = rng.normal(0, 0.3, (pyr.rows, A * 4))
    logits = rng.normal(0, 2, (pyr.rows, A * NC + 7)) + mu - 0.75 * ((cls_of - 1) % 4)
    if name == "one-class":
        logits[:, cls_of != 2] = -20.0
    if name == "drop":
        for s, (fh, fw) in enumerate(level_sizes):
            logits[pyr.row_off[s] + fh * fw: pyr.row_off[s] + 2 * fh * fw] = -8.0
    if name == "hand":  # level 3, anchor 0 of cells (0,0), (8,8), (15,15): 32-pixel boxes 64 pixels apart
        rel[:], logits[:] = 0.0, -20.0
        r0 = pyr.row_off[0]
        logits[r0, 1] = logits[r0 + 255, 1] = logits[r0 + 136, 1] = logits[r0 + 136, 2] = 2.0
    return rel, logits


def reference(boxes, logits, t, cap, topk, max_out, sigma, min_score):
    """One image: boxes [N,4] fp64, logits [N,NC] fp32.  Returns the outputs' (anchor, class, fp64
    score), total, overflow, the three margins of the module docstring and (largest class, classes
    stopped at max_out with candidates left, exact ties between a pick and its runner-up)."""
    NC = logits.shape[1]
    ok = logits >= t
    ok[:, 0] = False  # class 0 is background
    flat = np.flatnonzero(ok.reshape(-1))  # ascending flat id i*NC + c
    total, v = len(flat), logits.reshape(-1)[flat]
    flat = flat[np.lexsort((flat, -v))[:cap]] if topk else flat[:cap]  # logit descending, flat id ascending
    i, c = flat // NC, flat % NC
    s_all = 1.0 / (1.0 + np.exp(-logits.reshape(-1)[flat].astype(np.float64)))
    em, g_pick, g_min, largest, stops, ties = [], np.inf, np.inf, 0, 0, 0
    w = lambda x: np.maximum(0.0, x[..., 3] - x[..., 1]) * np.maximum(0.0, x[..., 2] - x[..., 0])  # area, iou_tf's order
    for cls in np.unique(c):
        an, s = i[c == cls], s_all[c == cls].copy()
        b, live, picks = boxes[an], np.ones(len(an), bool), 0
        largest = max(largest, len(an))
        while live.any() and picks < max_out:
            o = np.flatnonzero(live)
            o = o[np.lexsort((an[o], -s[o]))]  # score descending, anchor ascending
            j, o = o[0], o[1:]
            if len(o) and s[o[0]] == s[j]:
                ties += 1
            elif len(o):
                g_pick = min(g_pick, (s[j] - s[o[0]]) / s[j])
            em.append((an[j], cls, s[j]))
            live[j], picks = False, picks + 1
            ih = np.maximum(0.0, np.minimum(b[j, 2], b[o, 2]) - np.maximum(b[j, 0], b[o, 0]))
            iw = np.maximum(0.0, np.minimum(b[j, 3], b[o, 3]) - np.maximum(b[j, 1], b[o, 1]))
            uni = (w(b[j]) + w(b[o])) - iw * ih
            ov = np.where(uni == 0, 0.0, iw * ih / np.where(uni == 0, 1.0, uni))
            s[o] = s[o] * np.exp(-(ov * ov) / sigma)
            if len(o) and min_score > 0:
                g_min = min(g_min, np.abs(s[o] / min_score - 1).min())
            live[o[s[o] < min_score]] = False
        stops += int(live.any())
    ea, ec, es = (np.asarray(x) for x in zip(*em)) if em else (np.zeros(0, np.int64),) * 3
    order = np.lexsort((ec, ea, -es.astype(np.float32)))[:max_out + 1]
    s64, s32 = es[order], es[order].astype(np.float32).astype(np.float64)
    d = s64[:-1] != s64[1:]
    g_out = ((s32[:-1] - s32[1:])[d] / s32[:-1][d]).min() if d.any() else np.inf
    k = order[:max_out]
    return ea[k], ec[k], es[k], total, int(total > cap), (g_pick, g_min, g_out), (largest, stops, ties)


@pytest.mark.gpu
@pytest.mark.parametrize("name,dt,NC,B,s_thr,sigma,cap,max_out,select,mu,seed", CASES, ids=[c[0] for c in CASES])
def test_soft_nms_matches_fp64_reference(name, dt, NC, B, s_thr, sigma, cap, max_out, select, mu, seed):
    from tf2mv_amd.anchors import Anchors
    a = Anchors(3, 7, (128, 128), 3, ASPECTS, 4.0, device="cuda")
    pyr = a.pyramid(B)
    rel, logits = build(name, pyr, a.level_sizes, NC, mu, np.random.default_rng(seed))
    tdt = torch.float32 if dt == "f32" else torch.bfloat16
    rel_g = torch.tensor(rel, dtype=torch.float32).to("cuda", tdt)
    log_g = torch.tensor(logits, dtype=torch.float32).to("cuda", tdt)
    box_levels, cls_levels = [], []
    for s, (fh, fw) in enumerate(a.level_sizes):
        sl = pyr.seg_slice(s)
        box_levels.append(rel_g[sl].view(B, fh, fw, A, 4))
        cls_levels.append(log_g[sl, : A * NC].view(B, fh, fw, A, NC))
    ob, oc, os_, cnt, total, over = (x.cpu().numpy() for x in a.detect_per_class(
        tuple(box_levels), tuple(cls_levels), max_out, 0.5, s_thr, "iou", cap, select=select, nms="soft", sigma=sigma))
    dec = a.convert_outputs_boxes(tuple(box_levels))
    t = np.float32(np.log(s_thr / (1 - s_thr))) if s_thr else np.float32(-np.inf)
    for b in range(B):
        boxes = np.concatenate([d[b].reshape(-1, 4).cpu().numpy() for d in dec]).astype(np.float64)
        lg = np.concatenate([c[b].reshape(-1, NC).float().cpu().numpy() for c in cls_levels])
        ri, rc, rs, rtotal, rover, (g_pick, g_min, g_out), (largest, stops, ties) = reference(
            boxes, lg, t, cap, select == "topk", max_out, sigma, s_thr)
        print(f"image {b}: total {rtotal} overflow {rover} out {len(ri)} largest class {largest} stopped {stops} "
              f"ties {ties} margins {g_pick:.3g} {g_min:.3g} {g_out:.3g} | gpu count {cnt[b]} total {total[b]} "
              f"overflow {over[b]}")
        # conditions on the inputs, from the reference alone
        assert g_pick >= 1e-9 and g_min >= 1e-9, "a choice sits on fp64 noise: pick another seed"
        assert g_out > 2 * 2.0 ** -23, "two output scores within 2 fp32 ulps: pick another seed"
        assert (rtotal == 0) == (name == "drop" and b == 1)
        assert name != "one-class" or largest > 1024
        assert name != "topk" or rover == 1
        assert name != "nodrop" or stops >= 1
        assert name != "hand" or ties >= 2
        assert (total[b], over[b], cnt[b]) == (rtotal, rover, len(ri))
        k = len(ri)
        np.testing.assert_array_equal(oc[b, :k], rc)
        want = boxes[ri]
        mag_y = np.abs(want[:, 0] + want[:, 2]) / 2 + np.abs(want[:, 2] - want[:, 0]) / 2
        mag_x = np.abs(want[:, 1] + want[:, 3]) / 2 + np.abs(want[:, 3] - want[:, 1]) / 2
        tol = 4 * np.finfo(np.float32).eps * np.stack([mag_y, mag_x, mag_y, mag_x], -1)
        assert (np.abs(ob[b, :k] - want) <= tol).all()
        np.testing.assert_allclose(os_[b, :k], rs, rtol=2.0 ** -23, atol=0)


@pytest.mark.parametrize("metric,sigma,min_score,msg", [(0, 0.0, 0.05, "sigma"), (0, float("inf"), 0.05, "sigma"),
                                                        (0, 0.5, 1.0, "min_score"), (1, 0.5, 0.05, "metric")])
def test_detect_per_class_soft_rejects_bad_arguments(metric, sigma, min_score, msg):
    """Argument validation happens before any HIP call (no GPU needed)."""
    lib = _lib.lib()
    pyr = _lib.Pyramid()
    pyr.nseg, pyr.batch, pyr.H[0], pyr.W[0] = 1, 1, 4, 4
    d = ctypes.c_void_p(16)
    rc = lib.fns["edet_detect_per_class_soft"](0, d, d, 36, d, 45, ctypes.byref(pyr), 9, 5, 4096, 100, -2.9, metric, 0,
                                               sigma, min_score, d, d, d, d, d, d, d, None)
    assert rc == -1 and msg in lib.last_error()
    from tf2mv_amd.anchors import Anchors
    with pytest.raises(ValueError, match="nms"):
        Anchors.detect_per_class(None, (), (), nms="gaussian")
