"""Force-match target assignment (edet_generate_targets_matched, include/edet.h) against a numpy
restatement of its four rules over oracle.ref_anchors: IoU bit-exact fp32 on both sides, so masks,
class indices and gt_anchor compare exactly; encodings under test_generate_targets_and_decode's
bound for logf.

The ground truths (128 x 128, levels 3-7, 9 anchors a location, 3069 anchors an image): boxes 0-4
reach IoU <= 0.064 and get no positive under the plain rule; their maxima are attained by 7 to 16
anchors each (lowest index wins); boxes 0, 1, 2 all pick anchor 1 (lowest k wins), 3 and 4 pick
anchor 928 whose own arg-max is another box, 5 and 6 anchor 2628 in level 4; box 7 is degenerate
and forces nothing.

Batch sizes reach the planner's routes (csrc/match.hip, match_ap: the largest AP that leaves 512
blocks of 256 * AP anchors when forcing, of 4, 2, 1; 2048 blocks, of 2, 1, when not).  At 3069
anchors an image is 12 / 6 / 3 chunks at AP 1 / 2 / 4, the last ragged in each.  Larger batches
repeat the three images."""
import numpy as np
import pytest
import torch

from oracle import ref_anchors as RA
from tf2mv_amd import _lib as L
from tf2mv_amd.anchors import Anchors, Targets
from tf2mv_amd.runtime import stream, vp

pytestmark = pytest.mark.gpu
ASPECTS = [(1.0, 1.0), (1.4, 0.7), (0.7, 1.4)]
GT8 = np.array([[1, 1, 9, 9], [2, 2, 8, 8], [0, 1, 9, 8], [60, 60, 68, 68], [61, 61, 67, 67], [40, 40, 100, 100],
                [41, 41, 99, 99], [20, 20, 20, 30]], np.float32)
CLS8 = np.arange(1, 9, dtype=np.int32)
ROUTES = {1: 3, 2: 86, 4: 171}  # forcing: anchors per thread -> a batch size that selects it at 3069 anchors
ROUTES_OFF = {1: 3, 2: 342}  # the same with force_match = 0


def reference(flat, boxes, classes, thr, force=True):
    """Rules 1-4 for one image: (encodings [N,4], classes [N], mask [N], gt_anchor [n])."""
    N, n = flat.shape[0], boxes.shape[0]
    if n == 0:
        return np.zeros((N, 4), np.float32), np.zeros(N, np.int32), np.zeros(N, np.uint8), np.zeros(0, np.int32)
    v = RA.iou(flat[:, None, :], boxes[None, :, :])
    best, pos = v.argmax(1), v.max(1) >= np.float32(thr)
    f = np.where(v.max(0) > 0, v.argmax(0), -1).astype(np.int32) if force else np.full(n, -1, np.int32)
    for k in reversed(range(n)):  # the lowest k of an anchor is written last
        if f[k] >= 0:
            best[f[k]], pos[f[k]] = k, True
    enc = np.where(pos[:, None], RA.encode(flat, boxes[best]), np.float32(0))
    return enc, np.where(pos, classes[best], 0).astype(np.int32), pos.astype(np.uint8), f


def batch_inputs(B, G=8):
    """Image 0: all eight boxes; image 1: a permutation of a subset, its padding a box that
    would change the result if read; image 2: no ground truth; then the same again."""
    sel = [6, 3, 0, 7, 2]
    boxes = np.tile(np.array([0, 0, 128, 128], np.float32), (3, G, 1))
    cls = np.full((3, G), 77, np.int32)
    boxes[0, :8], cls[0, :8] = GT8, CLS8
    boxes[1, :5], cls[1, :5] = GT8[sel], CLS8[sel]
    rep = -(-B // 3)
    return np.tile(boxes, (rep, 1, 1))[:B], np.tile(cls, (rep, 1))[:B], np.tile(np.array([8, 5, 0], np.int32), rep)[:B]


def per_image(a, t, B):
    """Targets in each image's flat [level][H][W][A] order: box [B,N,4], cls [B,N], mask [B,N]."""
    out = []
    for arr in (t.box.cpu().numpy(), t.cls.cpu().numpy(), t.mask.cpu().numpy()):
        lv = [arr[t.pyr.seg_slice(s)].reshape(B, H * W * t.A, *arr.shape[2:]) for s, (H, W) in enumerate(a.level_sizes)]
        out.append(np.concatenate(lv, 1))
    return out


def check(a, t, boxes, cls, n, thr, distinct):
    B = boxes.shape[0]
    flat = a.flat.cpu().numpy()
    tb, tc, tm = per_image(a, t, B)
    ga = t.gt_anchor.cpu().numpy()
    for b in range(distinct):
        enc, rc, rm, f = reference(flat, boxes[b, : n[b]], cls[b, : n[b]], thr)
        for i in range(b, B, distinct):  # the images that repeat image b
            np.testing.assert_array_equal(tm[i], rm)
            np.testing.assert_array_equal(tc[i], rc)
            np.testing.assert_array_equal(ga[i], np.concatenate([f, np.full(ga.shape[1] - n[b], -1, np.int32)]))
            np.testing.assert_allclose(tb[i], enc, rtol=2e-6, atol=1e-6)
    return tm, ga


@pytest.mark.parametrize("thr", [0.5, 0.0])
@pytest.mark.parametrize("size,ap", [((128, 128), 1), ((128, 128), 2), ((128, 128), 4), ((128, 192), 1)])
def test_forced_assignment_matches_reference(size, ap, thr):
    B = ROUTES[ap]
    a = Anchors(3, 7, size, 3, ASPECTS, 4.0)
    boxes, cls, n = batch_inputs(B)
    t = a.generate_targets_batched(torch.tensor(boxes), torch.tensor(cls), torch.tensor(n), thr, force_match=True)
    tm, ga = check(a, t, boxes, cls, n, thr, 3)
    if size == (128, 128):
        assert a.flat.shape[0] == 3069 and ga[0].tolist() == [1, 1, 1, 928, 928, 2628, 2628, -1]
        plain = a.generate_targets_batched(torch.tensor(boxes), torch.tensor(cls), torch.tensor(n), thr)
        pm = per_image(a, plain, B)[2]
        assert plain.gt_anchor is None
        if thr == 0.5:  # the small boxes are unreachable without the feature
            assert pm[0][[1, 928]].tolist() == [0, 0] and tm[0][[1, 928]].tolist() == [1, 1]
            assert int(tm[0].sum()) == int(pm[0].sum()) + 2


@pytest.mark.parametrize("thr", [0.5, 0.0])
@pytest.mark.parametrize("ap", [1, 2])
def test_force_off_equals_generate_targets(ap, thr):
    """force_match = 0 through the new entry point: edet_generate_targets' bits in all three
    outputs, gt_anchor all -1 (the scratch may then be null)."""
    B = ROUTES_OFF[ap]
    a = Anchors(3, 7, (128, 128), 3, ASPECTS, 4.0)
    boxes, cls, n = batch_inputs(B)
    gb, gc, ng = (torch.tensor(v).cuda() for v in (boxes, cls, n))
    want = a.generate_targets_batched(gb, gc, ng, thr)
    got = Targets(want.pyr, want.A, a.device)
    ga = torch.zeros((B, 8), dtype=torch.int32, device=a.device)
    L.call("edet_generate_targets_matched", vp(a.flat), got.pyr.c, got.A, vp(gb), vp(gc), vp(ng), 8, thr, vp(got.box),
           vp(got.cls), vp(got.mask), 0, None, vp(ga), stream())
    for w, g in zip(per_image(a, want, B), per_image(a, got, B)):
        np.testing.assert_array_equal(w.view(np.uint8), g.view(np.uint8))  # bit for bit
    assert bool((ga == -1).all())


def test_more_ground_truths_than_the_lds_tile():
    rng = np.random.default_rng(130)
    B, G = 2, 130
    a = Anchors(3, 7, (128, 128), 3, ASPECTS, 4.0)
    hw, c = rng.uniform(4, 100, (B, G, 2)), rng.uniform(0, 128, (B, G, 2))
    boxes = np.concatenate([c - hw / 2, c + hw / 2], -1).astype(np.float32)
    cls, n = rng.integers(1, 81, (B, G)).astype(np.int32), np.array([130, 129], np.int32)
    t = a.generate_targets_batched(torch.tensor(boxes), torch.tensor(cls), torch.tensor(n), force_match=True)
    _, ga = check(a, t, boxes, cls, n, 0.5, B)
    assert (ga[0] >= 0).all() and len(set(ga[0].tolist())) < G  # every box forced, some anchors contested


def test_public_surface_and_repeatability():
    a = Anchors(3, 7, (128, 128), 3, ASPECTS, 4.0)
    boxes, cls, n = (torch.tensor(v) for v in batch_inputs(ROUTES[4]))
    plain = a.generate_targets_batched(boxes, cls, n)
    one = a.generate_targets(GT8, CLS8, 9)
    a.force_match = True
    t, t2 = a.generate_targets_batched(boxes, cls, n), a.generate_targets_batched(boxes, cls, n)
    for x, y in ((t.box, t2.box), (t.cls, t2.cls), (t.mask, t2.mask), (t.gt_anchor, t2.gt_anchor)):
        assert torch.equal(x, y)
    assert plain.gt_anchor is None and t.gt_anchor.dtype == torch.int32 and tuple(t.gt_anchor.shape) == (ROUTES[4], 8)
    # positives: the plain count plus the forced anchors that were not positive already
    pm, ga = per_image(a, plain, ROUTES[4])[2], t.gt_anchor.cpu().numpy()
    extra = sum(int((pm[b][np.unique(ga[b][ga[b] >= 0])] == 0).sum()) for b in range(ROUTES[4]))
    cnt = torch.zeros(2, dtype=torch.float32, device=a.device)
    L.call("edet_count_positives", vp(plain.mask), plain.mask.numel(), vp(cnt[0:]), stream())
    L.call("edet_count_positives", vp(t.mask), t.mask.numel(), vp(cnt[1:]), stream())
    assert extra > 0 and float(cnt[1]) == float(cnt[0]) + extra
    forced = a.generate_targets(GT8, CLS8, 9)  # the per-image form follows the attribute too
    assert int(sum(m.sum() for m in forced[2])) == int(sum(m.sum() for m in one[2])) + 2
    assert forced[1][0].reshape(-1, 9)[1].tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 0]  # anchor 1 -> box 0, class 1
