"""Anchors.detect_per_class (edet_detect_per_class): multi-label candidates, NMS within a class.

The selection is checked against a plain numpy fp64 restatement of the semantics in
include/edet.h on the boxes Anchors.convert_outputs_boxes decodes from the same regressions
(that decode is pinned by test_generate_targets_and_decode).  The GPU evaluates overlaps in
fp32, so a pair whose overlap sat on the threshold could go either way: the reference reports
the smallest |overlap - iou_threshold| it consulted and every case's seed keeps it >= 1e-5
(fp32 vs fp64 IoU of the same boxes differs by <~ 5e-7, 1-2 ulp on coordinates of ~1e2 adds
<~ 2e-6; 1e-5 is five times the sum)."""
import ctypes

import numpy as np
import pytest
import torch

from tf2mv_amd import _lib

ASPECTS = [(1.0, 1.0), (1.4, 0.7), (0.7, 1.4)]


def overlap(k, b, metric):
    """fp64 IoU / DIoU (iou.py:27-100, divide_no_nan) of the kept boxes k [n,4] with box b."""
    area = lambda x: np.maximum(0, x[..., 3] - x[..., 1]) * np.maximum(0, x[..., 2] - x[..., 0])
    ih = np.maximum(0, np.minimum(k[:, 2], b[2]) - np.maximum(k[:, 0], b[0]))
    iw = np.maximum(0, np.minimum(k[:, 3], b[3]) - np.maximum(k[:, 1], b[1]))
    union = area(k) + area(b) - iw * ih
    v = np.where(union == 0, 0, iw * ih / np.where(union == 0, 1, union))
    if metric == "diou":
        e2 = ((k[:, 0] + k[:, 2]) / 2 - (b[0] + b[2]) / 2) ** 2 + ((k[:, 1] + k[:, 3]) / 2 - (b[1] + b[3]) / 2) ** 2
        d2 = (np.maximum(k[:, 2], b[2]) - np.minimum(k[:, 0], b[0])) ** 2 + \
             (np.maximum(k[:, 3], b[3]) - np.minimum(k[:, 1], b[1])) ** 2
        v = v - np.where(d2 == 0, 0, e2 / np.where(d2 == 0, 1, d2))
    return v


def reference(boxes, logits, t, cap, max_out, iou_thr, metric):
    """One image: boxes [N,4] fp64, logits [N,NC] fp32.  Returns the detections' (anchor, class,
    logit), the candidates found, the overflow flag and the smallest |overlap - iou_thr| consulted."""
    NC = logits.shape[1]
    lg = logits.copy()
    lg[:, 0] = -np.inf  # class 0 is background
    flat = np.flatnonzero(lg.reshape(-1) >= t)  # ascending flat id i*NC + c
    total, flat = len(flat), flat[:cap]
    i, c, v = flat // NC, flat % NC, lg.reshape(-1)[flat].astype(np.float64)
    kept, gap = [], np.inf
    for cls in np.unique(c):
        sel = np.flatnonzero(c == cls)
        ks = []
        for q in sel[np.lexsort((i[sel], -v[sel]))]:  # logit descending, anchor ascending
            if len(ks) == max_out:
                break
            if ks:
                ov = overlap(boxes[i[ks]], boxes[i[q]], metric)
                gap = min(gap, float(np.abs(ov - iou_thr).min()))
                if (ov >= iou_thr).any():
                    continue
            ks.append(q)
        kept += ks
    kept = np.asarray(kept, np.int64)
    kept = kept[np.lexsort((c[kept], i[kept], -v[kept]))][:max_out]
    return i[kept], c[kept], v[kept], total, int(total > cap), gap


# size, NC, B, dtype, metric, score_threshold, max_candidates, max_output_size, quiet image, seed
CASES = [
    (128, 5, 3, "f32", "iou", 0.9, 4096, 1000, None, 8),    # chunk boundaries, classes share waves, m not 2^k
    (128, 5, 3, "f32", "diou", 0.9, 4096, 1000, None, 1),
    (128, 5, 3, "bf16", "iou", 0.9, 4096, 1000, None, 5),
    (128, 5, 3, "bf16", "diou", 0.9, 4096, 1000, None, 0),
    (128, 2, 2, "f32", "iou", 0.5, 4096, 1000, None, 7),    # one class: multi-tile wave NMS, kept-list pass
    (256, 81, 2, "f32", "iou", 0.9992, 4096, 1000, None, 0),  # more classes than waves, empty classes, ldc 729+7
    (128, 5, 2, "f32", "iou", 0.05, 256, 100, None, 0),    # overflow: the first 256 in flat order
    (128, 5, 3, "f32", "iou", 0.9, 4096, 10, 1, 0),        # final truncation and tie order; an empty image
]


@pytest.mark.gpu
@pytest.mark.parametrize("size,NC,B,dt,metric,s_thr,cap,max_out,quiet,seed", CASES)
def test_detect_per_class_matches_fp64_reference(size, NC, B, dt, metric, s_thr, cap, max_out, quiet, seed):
    from tf2mv_amd.anchors import Anchors
    rng = np.random.default_rng(seed)
    a = Anchors(3, 7, (size, size), 3, ASPECTS, 4.0, device="cuda")
    A, pyr = 9, a.pyramid(B)
    tdt = torch.float32 if dt == "f32" else torch.bfloat16
    ld_b, ld_c = A * 4, A * NC + 7  # an unaligned logits stride, like inference's A*NC
    rel, logits = torch.zeros(pyr.rows, ld_b), torch.zeros(pyr.rows, ld_c)
    for s, (fh, fw) in enumerate(a.level_sizes):
        sl, n = pyr.seg_slice(s), pyr.seg_rows(s)
        rel[sl] = torch.tensor(rng.normal(0, 0.3, (n, ld_b)), dtype=torch.float32)
        logits[sl] = torch.tensor(np.round(rng.normal(0, 2, (n, ld_c)) * 4) / 4, dtype=torch.float32)  # exact ties
        if quiet is not None:
            logits[sl.start + quiet * fh * fw: sl.start + (quiet + 1) * fh * fw] = -8.0
    rel_g, log_g = rel.to("cuda", tdt), logits.to("cuda", tdt)
    box_levels, cls_levels = [], []
    for s, (fh, fw) in enumerate(a.level_sizes):
        sl = pyr.seg_slice(s)
        box_levels.append(rel_g[sl].view(B, fh, fw, A, 4))
        cls_levels.append(log_g[sl, : A * NC].view(B, fh, fw, A, NC))
    ob, oc, os_, cnt, total, over = (x.cpu().numpy() for x in a.detect_per_class(
        tuple(box_levels), tuple(cls_levels), max_out, 0.5, s_thr, metric, cap))
    dec = a.convert_outputs_boxes(tuple(box_levels))
    t = np.float32(np.log(s_thr / (1 - s_thr)))
    for b in range(B):
        boxes = np.concatenate([d[b].reshape(-1, 4).cpu().numpy() for d in dec]).astype(np.float64)
        lg = np.concatenate([c[b].reshape(-1, NC).float().cpu().numpy() for c in cls_levels])
        ri, rc, rv, rtotal, rover, gap = reference(boxes, lg, t, cap, max_out, 0.5, metric)
        print(f"image {b}: total {rtotal} overflow {rover} kept {len(ri)} gap {gap:.3g} | gpu count {cnt[b]} "
              f"total {total[b]} overflow {over[b]}")
        assert gap >= 1e-5, "the inputs put an overlap on the threshold: pick another seed"
        assert (total[b], over[b], cnt[b]) == (rtotal, rover, len(ri))
        assert (len(ri) == 0) == (b == quiet) and (rover == 1) == (cap < 4096)
        k = len(ri)
        np.testing.assert_array_equal(oc[b, :k], rc)
        want = boxes[ri]
        mag_y = np.abs(want[:, 0] + want[:, 2]) / 2 + np.abs(want[:, 2] - want[:, 0]) / 2
        mag_x = np.abs(want[:, 1] + want[:, 3]) / 2 + np.abs(want[:, 3] - want[:, 1]) / 2
        tol = 4 * np.finfo(np.float32).eps * np.stack([mag_y, mag_x, mag_y, mag_x], -1)
        assert (np.abs(ob[b, :k] - want) <= tol).all()
        np.testing.assert_allclose(os_[b, :k], 1 / (1 + np.exp(-rv)), rtol=3e-7, atol=0)


@pytest.mark.parametrize("cap,NC,null_cls,msg", [(4097, 5, False, "max_candidates"), (4096, 1, False, "NC"),
                                                 (4096, 5, True, "null")])
def test_detect_per_class_rejects_bad_arguments(cap, NC, null_cls, msg):
    """Argument validation happens before any HIP call (no GPU needed)."""
    lib = _lib.lib()
    pyr = _lib.Pyramid()
    pyr.nseg, pyr.batch, pyr.H[0], pyr.W[0] = 1, 1, 4, 4
    d = ctypes.c_void_p(16)
    rc = lib.fns["edet_detect_per_class"](0, d, d, 36, None if null_cls else d, 9 * NC, ctypes.byref(pyr), 9, NC, cap,
                                          100, 0.5, 0.05, 0, d, d, d, d, d, d, d, None)
    assert rc == -1 and msg in lib.last_error()
