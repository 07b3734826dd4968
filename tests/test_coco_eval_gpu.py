"""metrics.CocoEvaluator (csrc/evalmap.hip) against a numpy fp64 restatement of the contract in
include/edet.h, "COCO evaluation": TP masks, ground-truth counts, AR and the -1 pattern compare
exactly (the IoUs are the same IEEE operations on both sides); AP within 2 * 100 * 2^-53, the
two sides differing only in the order of a 101-term sum of values in [0, 1]."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tf2mv_amd import _lib as L

IOU_THR, REC_THR = np.linspace(0.5, 0.95, 10), np.linspace(0.0, 1.0, 101)
AP_TOL = 2 * 100 * 2.0 ** -53
F64 = np.float64


def iou64(d, g):
    """[nd, ng] fp64 IoUs of fp32 (y1, x1, y2, x2) boxes, the differences formed in fp64."""
    d, g = d[:, None, :], g[None, :, :]
    ih = np.maximum(0.0, np.minimum(d[..., 2], g[..., 2]).astype(F64) - np.maximum(d[..., 0], g[..., 0]).astype(F64))
    iw = np.maximum(0.0, np.minimum(d[..., 3], g[..., 3]).astype(F64) - np.maximum(d[..., 1], g[..., 1]).astype(F64))
    inter = ih * iw
    area = [(b[..., 2].astype(F64) - b[..., 0].astype(F64)) * (b[..., 3].astype(F64) - b[..., 1].astype(F64))
            for b in (d, g)]
    uni = (area[0] + area[1]) - inter
    return np.where(uni > 0, inter / np.where(uni > 0, uni, 1.0), 0.0)


def reference(batches, NC, M):
    """batches: [(boxes, classes, scores, counts, gt_boxes, gt_classes, n_gt)] numpy arrays of
    successive add calls.  Returns the records per slot, the counts, AP / AR and the ties met."""
    n_img = sum(len(b[3]) for b in batches)
    tp, slot_cls = np.zeros(n_img * M, np.int64), np.full(n_img * M, -1, np.int64)
    slot_score = np.zeros(n_img * M, np.float32)
    n_gt_class, iou_ties, max_pairs, i = np.zeros(NC, np.int64), 0, 0, 0
    for boxes, classes, scores, counts, gt_boxes, gt_classes, n_gt in batches:
        for b in range(len(counts)):
            cnt, ng = int(counts[b]), int(n_gt[b])
            order = np.lexsort((np.arange(cnt), -scores[b, :cnt].astype(F64), classes[b, :cnt]))
            slot_cls[i * M:i * M + cnt], slot_score[i * M:i * M + cnt] = classes[b, order], scores[b, order]
            gcls, pairs = gt_classes[b, :ng], 0
            n_gt_class += np.bincount(gcls[(gcls >= 1) & (gcls < NC)], minlength=NC)
            for c in np.unique(classes[b, :cnt]):
                rows, gidx = np.nonzero(classes[b, order] == c)[0], np.nonzero(gcls == c)[0]
                if c < 1 or not len(gidx):
                    continue
                iou = iou64(boxes[b, order[rows]], gt_boxes[b, gidx])
                pairs += iou.size
                for k, t in enumerate(IOU_THR):
                    free = np.ones(len(gidx), bool)
                    for a, r in enumerate(rows):
                        v = np.where(free, iou[a], -1.0)
                        if v.max() >= min(t, 1 - 1e-10):
                            w = np.nonzero(v == v.max())[0]
                            iou_ties += len(w) > 1
                            free[w[-1]] = False  # the higher index wins an exact tie
                            tp[i * M + r] |= 1 << k
            max_pairs, i = max(max_pairs, pairs), i + 1
    ap, ar, score_ties = np.full((NC, 10), -1.0), np.full((NC, 10), -1.0), 0
    for c in range(1, NC):
        n = int(n_gt_class[c])
        if n == 0:
            continue
        sl = np.nonzero(slot_cls == c)[0]
        sl = sl[np.lexsort((sl, -slot_score[sl].astype(F64)))]
        nd = len(sl)
        score_ties += int((np.diff(slot_score[sl]) == 0).sum())
        for k in range(10):
            tpc = np.cumsum((tp[sl] >> k) & 1)
            rc, pr = tpc / n, tpc / ((np.arange(nd) + 1) + 2.0 ** -52)
            pr = np.maximum.accumulate(pr[::-1])[::-1]
            j = np.searchsorted(rc, REC_THR, "left")
            q = np.where(j < nd, pr[np.minimum(j, nd - 1)], 0.0) if nd else np.zeros(101)
            ap[c, k], ar[c, k] = q.sum() / 101, rc[-1] if nd else 0.0
    return dict(tp=tp, slot_cls=slot_cls, used=slot_cls >= 0, n_gt=n_gt_class, ap=ap, ar=ar, iou_ties=iou_ties, score_ties=score_ties,
                max_pairs=max_pairs, n_img=n_img)


def jitter(rng, gt, scale):
    """gt boxes moved and resized by up to `scale` of their size: IoUs from about 0.3 to 1."""
    h, w = gt[:, 2] - gt[:, 0], gt[:, 3] - gt[:, 1]
    return (gt + rng.uniform(-1, 1, gt.shape) * scale[:, None] * np.stack([h, w, h, w], 1)).astype(np.float32)


def random_boxes(rng, n, size=200.0):
    p, s = rng.uniform(0, size, (n, 2)), rng.uniform(8, 60, (n, 2))
    return np.concatenate([p, p + s], 1).astype(np.float32)


def random_case(seed, n_img, NC, M, G, per_add, heavy, dets_only, gts_only, quant, copies):
    """Detections are jittered ground truths plus random false positives, scores quantised to
    1 / quant.  Class `heavy` takes about 60 % of both; `dets_only` / `gts_only` have no ground
    truths / detections.  Image 0 is full, image 1 has no detections, image 2 no ground truths;
    rows past the counts hold boxes that would change the result if read."""
    rng = np.random.default_rng(seed)
    det_cls = [c for c in range(1, NC) if c != gts_only]
    gt_cls = [c for c in range(1, NC) if c != dets_only]
    boxes, gtb = np.zeros((n_img, M, 4), np.float32), np.zeros((n_img, G, 4), np.float32)
    cls, gtc = np.zeros((n_img, M), np.int32), np.zeros((n_img, G), np.int32)
    counts, n_gt = rng.integers(M // 2, M + 1, n_img).astype(np.int32), rng.integers(G // 2, G + 1, n_img).astype(np.int32)
    for i in range(n_img):
        gtb[i] = random_boxes(rng, G)
        gtc[i] = np.where(rng.random(G) < 0.6, heavy, rng.choice(gt_cls, G))
        src = rng.integers(0, G, M)
        boxes[i] = np.where((np.arange(M) < copies * G)[:, None], jitter(rng, gtb[i, src], rng.uniform(0, 0.25, M)),
                            random_boxes(rng, M))
        cls[i] = np.where(np.arange(M) < copies * G, gtc[i, src], np.where(rng.random(M) < 0.6, heavy, rng.choice(det_cls, M)))
        cls[i] = np.where(cls[i] == gts_only, heavy, cls[i])
    counts[:3], n_gt[:3] = (M, 0, M // 2), (G, G // 2, 0)
    scores = (rng.integers(1, quant, (n_img, M)) / quant).astype(np.float32)
    return [(boxes[s:s + n], cls[s:s + n], scores[s:s + n], counts[s:s + n], gtb[s:s + n], gtc[s:s + n], n_gt[s:s + n])
            for s, n in zip(np.cumsum([0] + per_add[:-1]), per_add)]


def hand_case():
    """One image, integer coordinates.  Class 1: detection 0 covers half of ground truth 0, IoU
    exactly 0.5 (a match at k = 0 only); detection 3 and ground truth 3 have zero area.  Class
    2: detection 1 meets ground truths 1 and 2 at IoU 0.5 each and takes 2, the higher index;
    detection 2 (lower score) overlaps ground truth 1 only and matches because 1 is still free."""
    det = np.array([[[0, 0, 10, 5], [0, 0, 10, 10], [0, 10, 10, 20], [5, 5, 5, 5]]], np.float32)
    gt = np.array([[[0, 0, 10, 10], [0, 0, 10, 20], [0, -10, 10, 10], [3, 3, 3, 3]]], np.float32)
    return [(det, np.array([[1, 2, 2, 1]], np.int32), np.array([[0.5, 0.9, 0.8, 0.7]], np.float32),
             np.array([4], np.int32), gt, np.array([[1, 2, 2, 1]], np.int32), np.array([4], np.int32))]


@functools.lru_cache(maxsize=None)
def case(name):
    """(batches, NC, M, the reference's result), built once; the conditions on the inputs are
    asserted from the reference alone."""
    if name == "base":
        b, NC, M = random_case(1, 3, 5, 100, 12, [2, 1], 1, 4, 3, 64, 4), 5, 100
    elif name == "hand":
        b, NC, M = hand_case(), 3, 4
    elif name == "many-gt":
        b, NC, M = random_case(2, 3, 2, 128, 300, [3], 1, None, None, 4096, 0.3), 2, 128
    else:  # "long": class 1 holds most records, over 101 ground truths; class 2 has fewer than 101
        b, NC, M = random_case(3, 210, 91, 100, 8, [32] * 6 + [18], 1, None, None, 256, 1), 91, 100
    ref = reference(b, NC, M)
    det_classes = set(ref["slot_cls"][ref["used"]])
    if name == "base":  # class 3: ground truths only; class 4: detections only
        assert ref["score_ties"] >= 1 and 0 < ref["max_pairs"] <= L.EVAL_TABLE_PAIRS
        assert ref["n_gt"][3] > 0 and 3 not in det_classes and ref["n_gt"][4] == 0 and 4 in det_classes
    if name == "hand":  # slots: class 1 by score (0.7 degenerate, 0.5), then class 2 (0.9, 0.8)
        assert ref["iou_ties"] >= 1 and list(ref["tp"]) == [0, 1, 1, 1]
    if name == "many-gt":
        assert ref["max_pairs"] > L.EVAL_TABLE_PAIRS
    if name == "long":
        assert ref["n_img"] * M > 2 * L.EVAL_CHUNK and ref["n_gt"][1] > 101 > ref["n_gt"][2] > 0
        assert (ref["slot_cls"] == 1).sum() > L.EVAL_CHUNK  # its segment crosses sort chunks
    return b, NC, M, ref


@pytest.mark.gpu
@pytest.mark.parametrize("name,table_pairs", [("base", None), ("base", 0), ("hand", None), ("many-gt", None),
                                              ("long", None)])
def test_coco_evaluator_matches_reference(name, table_pairs):
    from tf2mv_amd.metrics import CocoEvaluator
    batches, NC, M, ref = case(name)
    ev = CocoEvaluator(NC, max_dets=M, capacity_images=ref["n_img"] + 1, table_pairs=table_pairs)
    for b in batches:
        ev.add(*(torch.as_tensor(a).cuda() for a in b))
    out = ev.summarize()
    n, used = ref["n_img"] * M, ref["used"]
    assert np.array_equal(ev.tp.cpu().numpy()[:n][used], ref["tp"][used])
    assert np.array_equal(ev.keys.cpu().numpy()[:n] != -1, used) and (ev.keys.cpu().numpy()[n:] == -1).all()
    assert np.array_equal(ev.n_gt.cpu().numpy(), ref["n_gt"])
    ap, ar = out["per_class_ap"].cpu().numpy(), out["per_class_ar"].cpu().numpy()
    assert np.array_equal(ap == -1, ref["ap"] == -1) and np.array_equal(ar, ref["ar"])
    err = np.abs(ap - ref["ap"]).max()
    print(f"{name}: max |AP[c,k] - reference| = {err:.3e} (bound {AP_TOL:.3e})")
    assert err <= AP_TOL
    valid = ref["ap"] >= 0
    for key, v, m in (("AP", ref["ap"], valid), ("AP50", ref["ap"][:, 0], valid[:, 0]),
                      ("AP75", ref["ap"][:, 5], valid[:, 5]), ("AR", ref["ar"], valid)):
        assert abs(out[key] - v[m].mean()) <= AP_TOL * m.sum(), key
    with pytest.raises(ValueError):  # capacity: one image is left
        ev.add(*(torch.as_tensor(np.concatenate([a, a])[:2]).cuda() for a in batches[0]))
    with pytest.raises(ValueError):  # shape mismatch
        ev.add(*(torch.as_tensor(a[:, :1] if a.ndim > 1 else a).cuda() for a in batches[0]))


@pytest.mark.gpu
def test_eval_step_adds_the_detections_of_detect_mode():
    """EfficientDetNetTrain.eval_step leaves the evaluator as an add of the mode's own detections does."""
    from tf2mv_amd.anchors import Anchors
    from tf2mv_amd.config import efficientnet_b0_blocks, get_efficientdet_config
    from tf2mv_amd.metrics import CocoEvaluator
    from tf2mv_amd.model import EfficientDetNetTrain
    c = get_efficientdet_config("efficientdet-d0", {"image_size": 128, "num_classes": 5, "survival_prob": None})
    anchors = Anchors(c.min_level, c.max_level, (128, 128), c.num_scales, c.aspect_ratios, c.anchor_scale)
    m = EfficientDetNetTrain(efficientnet_b0_blocks(), c, anchors, dtype="f32", seed=1, lr_schedule={"fixed_lr": 0.01})
    m.detect_mode = "per_class_soft"
    x = torch.tensor(np.random.default_rng(0).random((2, 128, 128, 3), dtype=np.float32)).cuda()
    gt = (torch.tensor([[[20.0, 30.0, 70.0, 90.0]], [[60.0, 10.0, 120.0, 50.0]]]), torch.tensor([[1], [3]]),
          torch.tensor([1, 1]))
    ev, want = CocoEvaluator(5, 100, 4), CocoEvaluator(5, 100, 4)
    m.eval_step((x, *gt), ev)
    bo, co = m.call(x, training=False)
    want.add(*anchors.detect_per_class(bo, co, select="topk", nms="soft")[:4], *gt)
    assert ev.images == 2 and all(torch.equal(getattr(ev, a), getattr(want, a)) for a in ("keys", "tp", "n_gt"))
    assert ev.n_gt.tolist() == [0, 1, 0, 1, 0] and 0.0 <= ev.summarize()["AP"] <= 1.0


def test_eval_entry_points_refuse_bad_arguments():
    """EDET_EINVAL with a naming message before any HIP call (runs without a GPU)."""
    lib = L.lib()
    p, thr = ctypes.c_void_p(16), ctypes.c_void_p(16)

    def match(M=100, G=8, NC=91, image0=0, cap=10, B=2, ptr=p):
        return lib.fns["edet_eval_match"](ptr, p, p, p, p, p, p, B, M, G, NC, thr, image0, cap, -1, p, p, p, None)

    sort, ap = lib.fns["edet_eval_sort"], lib.fns["edet_eval_ap"]
    for call, word in ((lambda: match(ptr=None), "null"), (lambda: match(M=129), "M 129"),
                       (lambda: match(NC=129), "NC 129"), (lambda: match(G=1025), "G 1025"),
                       (lambda: match(image0=9), "capacity overflow"), (lambda: match(cap=1 << 19, M=128), "2^25"),
                       (lambda: sort(None, 8, p, None), "null"), (lambda: sort(p, (1 << 25) + 1, p, None), "2^25"),
                       (lambda: ap(p, 8, p, p, 91, p, None, p, None), "null"),
                       (lambda: ap(p, 8, p, p, 129, p, p, p, None), "NC 129")):
        rc = call()
        assert rc == -1 and word in lib.last_error(), (rc, word, lib.last_error())
