"""Anchors.detect_per_class(select="topk") (edet_detect_per_class_select, EDET_SELECT_TOPK): on
overflow the candidates that enter NMS are the first max_candidates by (logit descending, flat
id ascending).  The fp64 reference selects them with one lexsort, sets every other logit to -inf
and runs the per-class reference of test_detect_per_class_gpu on what is left; the seeds keep
that reference's smallest |overlap - iou_threshold| >= 1e-5, as there."""
import ctypes

import numpy as np
import pytest
import torch

from test_detect_per_class_gpu import ASPECTS, reference
from tf2mv_amd import _lib

# size, NC, B, dtype, logits, score_threshold, max_candidates, boundary tie required, seed
CASES = [
    (128, 5, 2, "f32", "ties", 0.05, 256, True, 1),     # boundary ties go to the lower flat id; top-K != first-K
    (128, 5, 2, "bf16", "ties", 0.05, 256, True, 0),    # the two-digit bf16 path
    (128, 5, 2, "f32", "const", 0.0, 256, False, 0),    # one bin on every digit: pure flat-id selection
    (128, 5, 2, "f32", "ulps", 0.0, 300, True, 1),      # the last digit decides; signs; -0 = +0; cap not 2^k
    (256, 81, 2, "f32", "ties", 0.0, 4096, False, 1),   # ~982 k candidates per image, the full LDS budget
    (128, 5, 3, "f32", "quiet", 0.9, 4096, False, 0),   # no overflow: equals select="first"; an empty image
    (128, 5, 2, "f32", "sparse", 0.05, 256, False, 0),  # image 0 overflows, image 1 does not (the early exit)
]


def make_logits(kind, rng, n, ld_c, used):
    """One image's [n, ld_c] fp32 logits in pyramid-row order (`used` real columns, then pad)."""
    if kind == "const":
        return np.full((n, ld_c), -4.595, np.float32)
    if kind == "ulps":  # +-(1 + k 2^-23), 5 % of the entries +-0
        v = (1 + rng.integers(0, 4096, (n, ld_c)) * 2.0 ** -23) * np.where(rng.random((n, ld_c)) < 0.05, 0.0, 1.0)
        return (v * rng.choice([-1.0, 1.0], (n, ld_c))).astype(np.float32)
    if kind in ("all-quiet", "all-sparse"):
        v = np.full((n, ld_c), -8.0, np.float32)
        if kind == "all-sparse":
            v[:, :used].flat[rng.choice(n * used, 50, replace=False)] = 3.0
        return v
    return (np.round(rng.normal(0, 2, (n, ld_c)) * 4) / 4).astype(np.float32)  # exact ties


@pytest.mark.gpu
@pytest.mark.parametrize("size,NC,B,dt,kind,s_thr,cap,tie,seed", CASES)
def test_detect_topk_matches_fp64_reference(size, NC, B, dt, kind, s_thr, cap, tie, seed):
    from tf2mv_amd.anchors import Anchors
    rng = np.random.default_rng(seed)
    a = Anchors(3, 7, (size, size), 3, ASPECTS, 4.0, device="cuda")
    A, pyr, max_out = 9, a.pyramid(B), min(cap, 1000)
    tdt = torch.float32 if dt == "f32" else torch.bfloat16
    ld_b, ld_c = A * 4, A * NC + 7
    rel = torch.tensor(rng.normal(0, 0.3, (pyr.rows, ld_b)), dtype=torch.float32)
    logits, per_image = torch.zeros(pyr.rows, ld_c), sum(fh * fw for fh, fw in a.level_sizes)
    for b in range(B):  # image 1 of the quiet / sparse cases is all -8 (but for the sparse case's 50 entries)
        k = kind if kind not in ("quiet", "sparse") else "all-" + kind if b == 1 else "ties"
        img, r0 = torch.tensor(make_logits(k, rng, per_image, ld_c, A * NC)), 0
        for s, (fh, fw) in enumerate(a.level_sizes):
            start = pyr.seg_slice(s).start + b * fh * fw
            logits[start: start + fh * fw] = img[r0: r0 + fh * fw]
            r0 += fh * fw
    rel_g, log_g = rel.to("cuda", tdt), logits.to("cuda", tdt)
    box_levels, cls_levels = [], []
    for s, (fh, fw) in enumerate(a.level_sizes):
        sl = pyr.seg_slice(s)
        box_levels.append(rel_g[sl].view(B, fh, fw, A, 4))
        cls_levels.append(log_g[sl, : A * NC].view(B, fh, fw, A, NC))
    run = lambda select: a.detect_per_class(tuple(box_levels), tuple(cls_levels), max_out, 0.5, s_thr, "iou", cap,
                                            select=select)
    got = run("topk")
    ob, oc, os_, cnt, total, over = (x.cpu().numpy() for x in got)
    if kind == "quiet":  # no overflow: bit for bit the first-K path
        first = run("first")
        assert all(torch.equal(g, f) for g, f in zip(got[3:], first[3:]))
        assert all(torch.equal(g[b, : cnt[b]], f[b, : cnt[b]]) for g, f in zip(got[:3], first[:3]) for b in range(B))
    dec = a.convert_outputs_boxes(tuple(box_levels))
    t = np.float32(np.log(s_thr / (1 - s_thr))) if s_thr else np.float32(-np.inf)
    for b in range(B):
        boxes = np.concatenate([d[b].reshape(-1, 4).cpu().numpy() for d in dec]).astype(np.float64)
        lg = np.concatenate([c[b].reshape(-1, NC).float().cpu().numpy() for c in cls_levels])
        ok = lg >= t
        ok[:, 0] = False  # class 0 is background
        flat = np.flatnonzero(ok.ravel())
        v = lg.ravel()[flat]
        order = np.lexsort((flat, -v))  # logit descending, flat id ascending
        sel = flat[order[:cap]]
        rtotal, rover = len(flat), int(len(flat) > cap)
        masked = np.full_like(lg, -np.inf)
        masked.ravel()[sel] = lg.ravel()[sel]
        # (a finite threshold below every logit: the masked-out entries must not count)
        ri, rc, rv, _, _, gap = reference(boxes, masked, np.finfo(np.float32).min, masked.size, max_out, 0.5, "iou")
        print(f"image {b}: total {rtotal} overflow {rover} kept {len(ri)} gap {gap:.3g} | gpu count {cnt[b]} "
              f"total {total[b]} overflow {over[b]}")
        # conditions on the inputs, from the reference alone
        assert gap >= 1e-5, "the inputs put an overlap on the threshold: pick another seed"
        assert rover == int(kind != "quiet" and not (kind == "sparse" and b == 1))
        assert (rtotal == 0) == (kind == "quiet" and b == 1)
        if rover and kind != "const":
            assert sel.max() > flat[cap - 1], "top-K equals first-K: pick another seed"
        if rover and kind == "const":  # every score equal: the selection IS the first cap flat ids
            assert np.array_equal(np.sort(sel), flat[:cap])
        if rover and tie:  # the boundary score is shared by a selected and an unselected candidate
            assert v[order[cap - 1]] == v[order[cap]], "no tie on the boundary: pick another seed"
        assert (total[b], over[b], cnt[b]) == (rtotal, rover, len(ri))
        k = len(ri)
        np.testing.assert_array_equal(oc[b, :k], rc)
        want = boxes[ri]
        mag_y = np.abs(want[:, 0] + want[:, 2]) / 2 + np.abs(want[:, 2] - want[:, 0]) / 2
        mag_x = np.abs(want[:, 1] + want[:, 3]) / 2 + np.abs(want[:, 3] - want[:, 1]) / 2
        tol = 4 * np.finfo(np.float32).eps * np.stack([mag_y, mag_x, mag_y, mag_x], -1)
        assert (np.abs(ob[b, :k] - want) <= tol).all()
        np.testing.assert_allclose(os_[b, :k], 1 / (1 + np.exp(-rv)), rtol=3e-7, atol=0)


def test_detect_per_class_select_rejects_bad_select():
    """Argument validation happens before any HIP call (no GPU needed)."""
    lib = _lib.lib()
    pyr = _lib.Pyramid()
    pyr.nseg, pyr.batch, pyr.H[0], pyr.W[0] = 1, 1, 4, 4
    d = ctypes.c_void_p(16)
    rc = lib.fns["edet_detect_per_class_select"](0, d, d, 36, d, 45, ctypes.byref(pyr), 9, 5, 4096, 100, 0.5, 0.05, 0,
                                                 2, d, d, d, d, d, d, d, None)
    assert rc == -1 and "select" in lib.last_error()
    from tf2mv_amd.anchors import Anchors
    with pytest.raises(ValueError, match="select"):
        Anchors.detect_per_class(None, (), (), select="best")
