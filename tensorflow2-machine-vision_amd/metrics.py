"""Per-image mAP of the reference's evaluation step (host numpy, like the reference).

Restates ``AIServer/ai_api/ai_models/utils/mAP.py`` (``Get_TPFP`` :3-64, ``Get_AP`` :66-101,
``Get_mAP`` :103-110, ``Get_mAP_one`` :114-126), which ``EfficientDetNetTrain.test_step``
(efficientdet_net_train.py:160-167) calls through ``tf.numpy_function`` once per image.  The
arithmetic and its quirks are kept so the metric matches the reference number for number:

  * one TP per ground truth: the prediction with the highest IoU for that ground truth
    (np.argmax, first maximum) becomes TP if that IoU >= thresh;
  * rows sorted by score with ``np.argsort(...)[::-1]`` (ties: reverse of argsort order);
  * the precision list goes into ``mrec`` and the recall list into ``mpre`` (the reference's
    variable names are swapped; the envelope and the area are computed on them as written);
  * every class id in [0, class_num) is averaged, the background class 0 included.

``np.float`` in the reference is the builtin float (float64).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from .runtime import stream, vp


def get_tpfp(data, class_id, thresh=0.5):
    tp = []
    gt_num = 0
    for d in data:
        gt = np.array(d["groud_truth"], dtype=np.float64).reshape(-1, 5)
        gt = gt[gt[..., 4] == class_id]
        gt = np.expand_dims(gt, axis=0)
        gt_num += gt.shape[1]
        pred = np.array(d["prediction"], dtype=np.float64).reshape(-1, 6)
        pred = pred[pred[..., 4] == class_id]
        pred = np.expand_dims(pred, axis=1)
        if gt.shape[1] == 0 or pred.shape[0] == 0:
            continue
        gt_min, gt_max = gt[..., 0:2], gt[..., 2:4]
        gt_wh = gt_max - gt_min
        p_min, p_max = pred[..., 0:2], pred[..., 2:4]
        p_wh = p_max - p_min
        i_wh = np.maximum(np.minimum(gt_max, p_max) - np.maximum(gt_min, p_min), 0.0)
        inter = i_wh[..., 0] * i_wh[..., 1]
        iou = inter / (gt_wh[..., 0] * gt_wh[..., 1] + p_wh[..., 0] * p_wh[..., 1] - inter)
        tp_one = np.zeros((pred.shape[0],))
        best = np.argmax(iou, axis=0)
        for i in range(best.shape[0]):
            if iou[best[i], i] >= thresh:
                tp_one[best[i]] = 1
        tp.append(np.concatenate([tp_one[:, None], pred[:, 0, 5:6]], axis=-1))
    tp = np.concatenate(tp, 0) if tp else np.zeros((0, 2))
    tp = tp[np.argsort(tp[:, 1])[::-1], :]
    return tp, gt_num


def get_ap(data, class_id, thresh=0.5):
    tp, gt_num = get_tpfp(data, class_id, thresh)
    precision, recall = [], []
    tp_sum = 0.0
    for i in range(tp.shape[0]):
        if tp[i][0] == 1:
            tp_sum += 1.0
        precision.append(tp_sum / (i + 1))
        recall.append(tp_sum / gt_num)
    mrec = np.concatenate(([0.0], precision, [1.0]))
    mpre = np.concatenate(([0.0], recall, [0.0]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1]))


def get_map(data, class_num, thresh=0.5):
    return sum(get_ap(data, c, thresh) for c in range(class_num)) / class_num


def get_map_one(ground_truth, prediction, class_num, thresh=0.5):
    """ground_truth [[y1, x1, y2, x2, class]], prediction [[y1, x1, y2, x2, class, score]]."""
    return get_map([{"image_path": "*.jpg", "groud_truth": ground_truth, "prediction": prediction}], class_num, thresh)


class CocoEvaluator:
    """COCO bbox AP averaged over IoU 0.50:0.05:0.95 on the device (include/edet.h, "COCO
    evaluation"; csrc/evalmap.hip): area range "all", one detection cap, no crowd annotations.

    ``add`` takes what ``Anchors.detect_per_class`` returns plus the ground truths and only
    launches the match kernel; ``summarize`` sorts the records and runs the AP kernel.  The state
    is three plain tensors: ``keys`` [capacity_images * max_dets] int64 (the bits of class |
    score descending | slot; -1 in unused slots), ``tp`` (int16 masks, bit k = matched at
    threshold k) and ``n_gt`` [num_classes] int32.  ``table_pairs`` bounds the match block's LDS
    table of IoUs (None: the library's 16384); 0 makes every image recompute them."""

    def __init__(self, num_classes: int, max_dets: int = 100, capacity_images: int = 5000, device="cuda",
                 table_pairs=None):
        if not 2 <= num_classes <= L.EVAL_MAX_CLASSES:
            raise ValueError(f"num_classes {num_classes} outside 2..{L.EVAL_MAX_CLASSES}")
        if not 1 <= max_dets <= L.EVAL_MAX_DETS:
            raise ValueError(f"max_dets {max_dets} outside 1..{L.EVAL_MAX_DETS}")
        if capacity_images < 1 or capacity_images * max_dets > 1 << L.EVAL_SLOT_BITS:
            raise ValueError(f"capacity_images {capacity_images} x max_dets {max_dets} outside "
                             f"1..2^{L.EVAL_SLOT_BITS} slots")
        self.num_classes, self.max_dets, self.capacity_images = num_classes, max_dets, capacity_images
        self.table_pairs = -1 if table_pairs is None else int(table_pairs)
        self.device = torch.device(device)
        slots = capacity_images * max_dets
        self.keys = torch.empty(slots, dtype=torch.int64, device=self.device)
        self.tp = torch.empty(slots, dtype=torch.int16, device=self.device)
        self.n_gt = torch.empty(num_classes, dtype=torch.int32, device=self.device)
        self.iou_thr = torch.tensor(np.linspace(0.5, 0.95, L.EVAL_THRESHOLDS), dtype=torch.float64, device=self.device)
        self.rec_thr = torch.tensor(np.linspace(0.0, 1.0, L.EVAL_RECALL_STEPS), dtype=torch.float64,
                                    device=self.device)
        self.reset()

    def reset(self):
        self.keys.fill_(-1)
        self.tp.zero_()
        self.n_gt.zero_()
        self.images = 0

    def add(self, boxes, classes, scores, counts, gt_boxes, gt_classes, n_gt):
        """One batch: boxes [B,M,4], classes / scores [B,M], counts [B] (M = max_dets), gt_boxes
        [B,G,4], gt_classes [B,G], n_gt [B].  Launches only; ValueError on a shape mismatch or
        when the batch does not fit the capacity."""
        B, M = int(boxes.shape[0]), self.max_dets
        G = int(gt_boxes.shape[1]) if gt_boxes.dim() == 3 else -1
        if (tuple(boxes.shape) != (B, M, 4) or tuple(classes.shape) != (B, M) or tuple(scores.shape) != (B, M)
                or tuple(counts.shape) != (B,) or tuple(gt_boxes.shape) != (B, G, 4)
                or tuple(gt_classes.shape) != (B, G) or tuple(n_gt.shape) != (B,)):
            raise ValueError(f"CocoEvaluator.add: shapes {tuple(boxes.shape)}, {tuple(classes.shape)}, "
                             f"{tuple(scores.shape)}, {tuple(counts.shape)}, {tuple(gt_boxes.shape)}, "
                             f"{tuple(gt_classes.shape)}, {tuple(n_gt.shape)} do not fit max_dets {M}")
        if G > L.EVAL_MAX_GT:
            raise ValueError(f"CocoEvaluator.add: {G} ground-truth rows an image, at most {L.EVAL_MAX_GT}")
        if self.images + B > self.capacity_images:
            raise ValueError(f"CocoEvaluator.add: {self.images} + {B} images exceed capacity_images "
                             f"{self.capacity_images}")
        if B == 0:
            return

        def dev(t, dtype):
            return t.to(device=self.device, dtype=dtype).contiguous()

        if G == 0:  # the kernel wants a row to point at; n_gt = 0 keeps it unread
            gt_boxes, gt_classes, n_gt, G = gt_boxes.new_zeros(B, 1, 4), gt_classes.new_zeros(B, 1), n_gt * 0, 1
        args = (dev(boxes, torch.float32), dev(classes, torch.int32), dev(scores, torch.float32),
                dev(counts, torch.int32), dev(gt_boxes, torch.float32), dev(gt_classes, torch.int32),
                dev(n_gt, torch.int32))
        L.call("edet_eval_match", *(vp(a) for a in args), B, M, G, self.num_classes, vp(self.iou_thr), self.images,
               self.capacity_images, self.table_pairs, vp(self.keys), vp(self.tp), vp(self.n_gt), stream())
        self.images += B

    def summarize(self):
        """{"AP", "AP50", "AP75", "AR": floats (nan without a valid class), "per_class_ap",
        "per_class_ar": [num_classes, 10] fp64 tensors, -1 for class 0 and classes without ground
        truths}."""
        n = self.images * self.max_dets
        npad = max(1, -(-n // L.EVAL_CHUNK)) * L.EVAL_CHUNK
        scratch = torch.empty(2 * npad, dtype=torch.int64, device=self.device)
        ap = torch.empty((self.num_classes, L.EVAL_THRESHOLDS), dtype=torch.float64, device=self.device)
        ar = torch.empty_like(ap)
        L.call("edet_eval_sort", vp(self.keys), n, vp(scratch), stream())
        L.call("edet_eval_ap", vp(scratch), n, vp(self.tp), vp(self.n_gt), self.num_classes, vp(self.rec_thr),
               vp(ap), vp(ar), stream())
        valid = ap >= 0

        def mean(v, m):
            return float(torch.where(m, v, torch.zeros_like(v)).sum() / m.sum())

        return {"AP": mean(ap, valid), "AP50": mean(ap[:, 0], valid[:, 0]), "AP75": mean(ap[:, 5], valid[:, 5]),
                "AR": mean(ar, valid), "per_class_ap": ap, "per_class_ar": ar}
